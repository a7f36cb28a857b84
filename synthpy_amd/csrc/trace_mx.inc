// Included by trace.hip inside its anonymous namespace (needs VolDev, TraceArgs, StepTab, find_cell, queue_push, write_outputs,
// the hand-off helpers, hi_word).
//
// Precision of the mixed build.  What must be float64 is what carries absolute position: the state y (lateral position,
// velocity, phase, time) and the difference (position - node) that places the ray in its cell.  Everything that is an
// INCREMENT within one step -- weights in [0, 1], the blended field values (float32 data to begin with), 1/v_a, the RK4 slopes
// and their weighted sum -- is float32: an increment of relative accuracy 6e-8 changes a 2e-8 m position step by 1e-15 m.
// Constant factors (omega, h/6) multiply in float64 at the accumulation.  A wave64 VALU instruction holds its SIMD for 4
// cycles whatever the type, so the stage is written for PACKED float32 (v_pk_fma_f32 / v_pk_mul_f32), every pair in an aligned
// register pair: a voxel is {d_b, d_c | d_a, n-1}, the two halves of the float4 are the pairs the blend works on.
// (Round 1's k_trace_mixed, which also took sub-steps and the optional terms in this arithmetic, spilled 20 registers and is
// gone since round 4: `precision="mixed"` with substeps > 1 or with kappa / Faraday fields runs the float64 kernels, whose
// results need no edge guard -- trace.hip, sr_rays_trace.)
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 splat(float s) { return f2{s, s}; }
__host__ __device__ inline size_t mixed_lds_bytes(int nb, int nc) { return sizeof(double) * 2 * (size_t)(nb + nc); }

// k_trace_mx: the mixed-precision plane-stepping RK4 for the common case (one step per cell, no optional terms), the
// structure of k_trace_f64 with the arithmetic above: float64 state, positions and accumulation; float32 stage
// arithmetic in packed pairs.  Against round 1's kernel:
//
//  * planes as float32 bilinear COEFFICIENTS {A, B, C, D} per field pair, f = A + w_b*B + w_c*(C + w_b*D): a stage's
//    blend is 3 packed FMAs per half-plane from the two weights alone (was: 2 packed FMAs for (w, 1-w), 2 packed
//    multiplies for the corner weights, 1 multiply + 3 FMAs per half-plane).  The differences B, C, D are formed once
//    per new plane (4 packed subtractions per half-plane) and are rounded relative to THEMSELVES, not to the corner
//    values;
//  * the multiply-adds whose addend is a plane coefficient are written as three-address v_pk_fma_f32 with the weight
//    broadcast by op_sel: the compiler's two-address form costs a v_mov_b64 (4.3 cycles, as much as the FMA) per operand;
//  * "still in the cached cell" is one unsigned compare on max(bits(w_b), bits(w_c)) (0 <= w < 1 - 2^-12); the
//    rarely-taken region has ONE level: it searches the node tables at the float64 position (SciPy's rule) and re-reads
//    the planes, whether the lane changed cell, came in through a lateral face or was outside the volume -- no
//    neighbour stepping, no "lost" rays, no second level for them.  Outside the volume a ray holds a virtual cell
//    (weight pinned inside [0, 1) by a reciprocal width of +-1e-30) and its field slopes are scaled by 0;
//  * node plane k+2 is requested at the end of step k straight into the dead lower buffer, as raw corner records, and
//    turned into coefficients in place after stage 1 of step k+1: nothing waits for it and it costs no register.
//  * EDGE GUARD (deposit.hip): the kernel keeps, per ray, a sum E that bounds the float32 rounding of its lateral
//    velocity changes, and writes guard = kGuardK * 2^-24 * E / v_a [rad] beside its outputs (kGuardK = 8).  Two kinds of
//    rounding enter a stage's lateral slope F / v_a:
//      - relative to the slope itself: the reciprocal 1/v_a, the products and the RK4 sums (and, through the position
//        increments, the entry direction);
//      - relative to the plane's bilinear COEFFICIENTS {A, B, C, D}: the blend A + w_b*B + w_c*(C + w_b*D) rounds each
//        partial sum, and the float32 weights (cell offset, reciprocal width) carry 2^-24 of themselves into w*B, w*C,
//        w*D.  Where the interpolated field crosses zero inside a cell, |F| is small and these are not; a ray that keeps
//        its weights from plane to plane (a collimated beam on a field that does not vary along the probing axis) makes
//        the same rounding at every step, so it adds up linearly.
//    Hence E = |v_b| + |v_c| at entry + sum_k h_k/6 * (|K_b| + |K_c|)  (K = k1 + 2 k2 + 2 k3 + k4)
//            + sum_k h_k/6 * (M_b + M_c) * (1/v_a + 2/v_a + 2/v_a + 1/v_a),  M = max(|A|, |B|, |C|, |D|) of d_b (d_c) on node
//    plane k+1 of the ray's cell: each partial sum of the blend and each w*B, w*C, w*D is at most 2 M, so the blend rounds
//    at a few 2^-24 M whatever |F|; every node plane is weighted 6/v_a once (the steps before and after it weigh it 3 + 3),
//    read from the upper plane that the step holds in registers anyway (a few float32 instructions per step, no register;
//    k_trace_mx +3 % on C2).  Measured largest |angle error| / guard: 0.04 on the BASELINE turbulence and 0.07 on the C1
//    blob (tests/test_gpu_parity.py::test_edge_guard_bound_holds), 0.21 on collimated beams near the zero crossings of a
//    field that varies along one lateral axis (tests/test_edge_guard.py), where the first two sums alone were exceeded up
//    to 940-fold.  The price: refractometry traces 2.8 % / 4.0 % of the rays again on C2 / C4's share (was 0.9 % / 1.3 %).
//    An exact-counts deposit re-traces in float64 every ray whose detector coordinate lies within that bound (times the
//    chain's lever) of a bin edge or of an aperture's edge.
typedef unsigned int u32;
constexpr float kGuardK = 8.f * 5.9604644775390625e-8f;  // 8 * 2^-24

__device__ __forceinline__ f2 pkfma_lo(f2 s, f2 x, f2 y) {  // {s.x*x.x + y.x, s.x*x.y + y.y}, into a register pair of its own
  f2 r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(r) : "v"(s), "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ f2 pkfma_hi(f2 s, f2 x, f2 y) {  // {s.y*x.x + y.x, s.y*x.y + y.y}
  f2 r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "=v"(r) : "v"(s), "v"(x), "v"(y));
  return r;
}

struct CoefF {
  f2 A[2], B[2], C[2], D[2];  // [0]: fields (d_b, d_c), [1]: (d_a, n-1)
};

// A plane requested for LATER use sits in its buffer as the four raw corner records (A = b0c0, C = b0c1, B = b1c0,
// D = b1c1: the loads land where the coefficients will be) and is turned into coefficients in place when first needed.
__device__ __forceinline__ void finalize_plane(CoefF &p) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    p.D[h] = p.D[h] - p.C[h];
    p.B[h] = p.B[h] - p.A[h];
    p.C[h] = p.C[h] - p.A[h];
    p.D[h] = p.D[h] - p.B[h];
  }
}

#ifndef SR_MX_WAVES
#define SR_MX_WAVES 4
#endif
template <bool PHASE>
__global__ __launch_bounds__(256, SR_MX_WAVES) void k_trace_mx(TraceArgs A) {
  extern __shared__ double lds[];
  const VolDev &V = A.V;
  double *sgb = lds, *srb = lds + V.nb, *sgc = lds + 2 * V.nb, *src = lds + 2 * V.nb + V.nc;
  for (int t = threadIdx.x; t < V.nb; t += blockDim.x) {
    sgb[t] = V.g[1][t];
    srb[t] = V.rg[1][t];
  }
  for (int t = threadIdx.x; t < V.nc; t += blockDim.x) {
    sgc[t] = V.g[2][t];
    src[t] = V.rg[2][t];
  }
  __syncthreads();

  // A list-driven launch (A.in_list, A.recover): the queue's slots, workgroups past its end leave
  // at once, no XCD remap (see k_trace_f64)
  const unsigned chunk = gridDim.x / 8;
  const unsigned bid = A.in_list ? blockIdx.x : (blockIdx.x % 8) * chunk + blockIdx.x / 8;  // one contiguous run of sorted rays per XCD
  if (bid >= A.n_blocks) return;
  const int64_t slot = (int64_t)bid * blockDim.x + threadIdx.x;
  if (A.in_list && (int64_t)bid * blockDim.x >= (int64_t)*A.in_count) return;  // uniform over the workgroup
  const bool have = slot < (A.in_list ? (int64_t)*A.in_count : A.N);
  const int64_t j = A.in_list ? (have ? (int64_t)A.in_list[slot] : 0) : slot;
  const int64_t N = A.N;
  const int a = A.axis, b = (a + 1) % 3, c = (a + 2) % 3;
  const int64_t i = have ? (int64_t)A.perm[j] : 0;

  double pa = 0, y0 = 0, y1 = 0, y2 = 1, y3 = 0, y4 = 0, y5 = 0, y6 = 0;
  if (have) {
    pa = A.s0[a * N + i];
    y0 = A.s0[b * N + i];
    y1 = A.s0[c * N + i];
    y2 = A.s0[(3 + a) * N + i];
    y3 = A.s0[(3 + b) * N + i];
    y4 = A.s0[(3 + c) * N + i];
    y5 = A.s0[7 * N + i];
  }
  const double ga0 = V.g[0][0];
  bool alive = have && (y2 > 0) && (pa <= ga0);
  if (alive && pa < ga0) {  // vacuum drift onto the entry plane
    const double tau = (ga0 - pa) / y2;
    if (tau >= A.t_end) {
      alive = false;
    } else {
      y0 = y0 + y3 * tau;
      y1 = y1 + y4 * tau;
      y6 = tau;
    }
  }
  if (A.handoff & SR_HANDOFF_ENTER) alive = handoff_enter(A, have, j, y0, y1, y2, y3, y4, y5, y6);  // A12
  // a NaN anywhere in the state is not a plane-form ray (the time-stepping form returns NaN for it, as SciPy would)
  alive = alive && (y0 == y0) && (y1 == y1) && (y3 == y3) && (y4 == y4) && (y5 == y5) && (y2 < 1e30) && (y2 > 1e-30);
  float eacc = (fabsf((float)y3) + fabsf((float)y4)) * A.guard_ih6;  // edge guard (header): E in units of the largest h/6
  if (A.recover && (A.handoff & SR_HANDOFF_ENTER) && have) eacc = A.guard[j];  // the tile path: the sum so far rides in guard[]

  const int64_t sc = kSC, sb = (int64_t)V.nc * 8;  // lateral neighbours in the packed node order

  // cached lateral cell: lower nodes (float64), reciprocal widths (float32 pair), the scale of the field slopes (1 in
  // the volume, 0 in a virtual cell outside it; hs = fs/2 for the mid-step plane), the column.  No cell yet: lo_b = +inf.
  double lo_b = __builtin_inf(), lo_c = 0.0;
  f2 rw = f2{1.f, 0.f};
  float fs = 0.f, hs = 0.f;
  int64_t col = 0;  // col8(cb, cc) of the (clamped) cell: always a valid column
  int cb = 0, cc = 0;
  CoefF PA, PB;
#pragma unroll
  for (int h = 0; h < 2; ++h) PA.A[h] = PA.B[h] = PA.C[h] = PA.D[h] = PB.A[h] = PB.B[h] = PB.C[h] = PB.D[h] = f2{0.f, 0.f};

  auto load_raw = [&](int k, CoefF &p) {  // the corner records into the buffer, unconverted (no wait)
    const float4 *q = V.P + col + koff(V, k);
    const float4 v0 = q[0], v1 = q[sc], v2 = q[sb], v3 = q[sb + sc];
    p.A[0] = f2{v0.x, v0.y}; p.A[1] = f2{v0.z, PHASE ? v0.w : 0.f};
    p.C[0] = f2{v1.x, v1.y}; p.C[1] = f2{v1.z, PHASE ? v1.w : 0.f};
    p.B[0] = f2{v2.x, v2.y}; p.B[1] = f2{v2.z, PHASE ? v2.w : 0.f};
    p.D[0] = f2{v3.x, v3.y}; p.D[1] = f2{v3.z, PHASE ? v3.w : 0.f};
  };
  auto load_plane = [&](int k, CoefF &p) {
    load_raw(k, p);
    finalize_plane(p);
  };
  auto add_into = [&](CoefF &LO, const CoefF &HI) {  // LO := LO + HI, the mid-step plane (times two)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      LO.A[h] = LO.A[h] + HI.A[h];
      LO.B[h] = LO.B[h] + HI.B[h];
      LO.C[h] = LO.C[h] + HI.C[h];
      LO.D[h] = LO.D[h] + HI.D[h];
    }
  };
  constexpr u32 kInsideF = 0x3F7FF000u;  // bits(w) <u this  <=>  0 <= w < 1 - 2^-12
  // one axis of the cell search (see trace_f64.inc): the neighbour the weight points at first, then the general search
  // (as trace_f64.inc's: the neighbour each weight points at first, the six table entries of both axes read before any
  // branch, the general search otherwise)
  auto neighbour = [&](int ci, float w, int n) { return min(max(ci + (w < 0.f ? -1 : (__float_as_uint(w) >= kInsideF ? 1 : 0)), 0), n - 2); };
  auto search = [&](const double *g, const double *rg, int n, double q, int &ci, double &lo, float &r) -> bool {
    // the volume's bounds are read from the table here, in the branch that needs them: held across the loop they cost 12
    // registers (VGPRs, or SGPRs that the kernel no longer has: it spilled them into v_writelane / v_readlane pairs)
    const double g0 = g[0], gL = g[n - 1];
    if (q >= g0 && q <= gL) {
      ci = find_cell(g, n, q, g0, (n - 1) / (gL - g0));
      lo = g[ci];
      r = (float)rg[ci];
      return true;
    }
    ci = q < g0 ? 0 : n - 2;
    lo = q < g0 ? g0 : gL;
    r = q < g0 ? -1e-30f : 1e-30f;
    return false;
  };
  auto locate2 = [&](double qb, double qc, f2 w, float &rb, float &rc, bool &in_b, bool &in_c) {
    const int nb_ = neighbour(cb, w.x, V.nb), nc_ = neighbour(cc, w.y, V.nc);
    double lb = sgb[nb_], ub = sgb[nb_ + 1], tb = srb[nb_], lc = sgc[nc_], uc = sgc[nc_ + 1], tc = src[nc_];
    asm("" : "+v"(lb), "+v"(ub), "+v"(tb), "+v"(lc), "+v"(uc), "+v"(tc));  // not volatile (see trace_f64.inc)
    if ((qb >= lb) & (qb < ub)) {
      cb = nb_;
      lo_b = lb;
      rb = (float)tb;
      in_b = true;
    } else {
      in_b = search(sgb, srb, V.nb, qb, cb, lo_b, rb);
    }
    if ((qc >= lc) & (qc < uc)) {
      cc = nc_;
      lo_c = lc;
      rc = (float)tc;
      in_c = true;
    } else {
      in_c = search(sgc, src, V.nc, qc, cc, lo_c, rc);
    }
  };

  const int k_end = A.k_last >= 0 ? A.k_last : V.na - 1;  // the planes this launch steps between (k_trace_f64 has the same)
  StepTab Tn = A.tab[A.k_first];

  auto layer = [&](int k, CoefF &LO, CoefF &HI) {
    const StepTab S = Tn;  // wave-uniform constants of this step; the next entry is requested now
    Tn = A.tab[k + 2 < V.na ? k + 1 : 0];
    if (alive) {
      const float va = (float)y2;
      const f2 vbc = f2{(float)y3, (float)y4};
      f2 dcell = f2{(float)(y0 - lo_b), (float)(y1 - lo_c)};  // offset in the cached cell, exact to float32
      f2 kpos, kbc, kan;  // slopes of (p_b, p_c), (v_b, v_c), (v_a, phase/omega)
      f2 apos, abc, aan;  // k1 + 2 k2 + 2 k3 (+ k4)
      float at;
      bool ok = true;
      auto stage = [&](auto SI) {
        constexpr int s = decltype(SI)::value;
        const float wf = s == 3 ? S.hf : S.hhf;
        float t2 = va;
        f2 tbc = vbc, dq = dcell;
        if (s > 0) {  // stage 2 steps along stage 1's slopes, which were written straight into the sums (no copy)
          dq = fma2(splat(wf), s == 1 ? apos : kpos, dcell);
          t2 = fmaf(wf, s == 1 ? aan.x : kan.x, va);
          tbc = fma2(splat(wf), s == 1 ? abc : kbc, vbc);
          ok = ok && (t2 > 0.f);
        }
        f2 w = dq * rw;
        if (max(__float_as_uint(w.x), __float_as_uint(w.y)) >= kInsideF) {  // the rarely-taken region
          const f2 kprev = s == 1 ? apos : kpos;
          const double qb = s > 0 ? fma((double)wf, (double)kprev.x, y0) : y0, qc = s > 0 ? fma((double)wf, (double)kprev.y, y1) : y1;
          float rb, rc;
          bool in_b, in_c;
          locate2(qb, qc, w, rb, rc, in_b, in_c);
          rw = f2{rb, rc};
          fs = (in_b && in_c) ? 1.f : 0.f;  // outside on either axis: the fill value
          hs = (in_b && in_c) ? 0.5f : 0.f;
          col = col8(V, cb, cc);
          if (s < 3) load_plane(k, LO);  // stage 4 reads HI only and the lower buffer is dead after it
          if (s == 0)
            load_raw(k + 1, HI);  // during stage 1 the upper plane is still raw: converted for every lane after it
          else
            load_plane(k + 1, HI);
          if (s == 1 || s == 2) add_into(LO, HI);
          dcell = f2{(float)(y0 - lo_b), (float)(y1 - lo_c)};
          dq = s > 0 ? fma2(splat(wf), kprev, dcell) : dcell;
          w = dq * rw;
        }
        const CoefF &P = s == 3 ? HI : LO;
        const f2 Fbc = pkfma_hi(w, pkfma_lo(w, P.D[0], P.C[0]), pkfma_lo(w, P.B[0], P.A[0]));
        const f2 Fan = pkfma_hi(w, pkfma_lo(w, P.D[1], P.C[1]), pkfma_lo(w, P.B[1], P.A[1]));
        const float iv = __builtin_amdgcn_rcpf(t2);
        const float ivf = iv * ((s == 1 || s == 2) ? hs : fs);  // the mid plane holds LO + HI; 0 outside the volume
        if (s == 0) {  // k1 goes straight into the sums
          apos = tbc * splat(iv);
          abc = Fbc * splat(ivf);
          aan = Fan * splat(ivf);
          at = iv;
        } else {
          kpos = tbc * splat(iv);
          kbc = Fbc * splat(ivf);
          kan = Fan * splat(ivf);
          if (s == 3) {
            apos = apos + kpos; abc = abc + kbc; aan = aan + kan; at = at + iv;
          } else {
            apos = fma2(splat(2.f), kpos, apos);
            abc = fma2(splat(2.f), kbc, abc);
            aan = fma2(splat(2.f), kan, aan);
            at = fmaf(2.f, iv, at);
          }
        }
      };
      stage(std::integral_constant<int, 0>{});
      finalize_plane(HI);  // requested at the end of the step before (or just now, by a lane that changed cell)
      add_into(LO, HI);    // node plane k is done with: LO becomes the mid plane (times two)
      stage(std::integral_constant<int, 1>{});
      stage(std::integral_constant<int, 2>{});
      stage(std::integral_constant<int, 3>{});
      // float64 accumulation of the step; omega and h/6 enter here, unrounded
      y0 = fma(S.h6, (double)apos.x, y0);
      y1 = fma(S.h6, (double)apos.y, y1);
      y2 = fma(S.h6, (double)aan.x, y2);
      y3 = fma(S.h6, (double)abc.x, y3);
      y4 = fma(S.h6, (double)abc.y, y4);
      if (PHASE) y5 = fma(S.h6w, (double)aan.y, y5);
      y6 = fma(S.h6, (double)at, y6);
      // edge guard (header): the slopes' own size, then the scale the blend rounds at, the largest coefficient of plane k+1
      eacc += fabsf(abc.x) + fabsf(abc.y);
      const float mb = fmaxf(fmaxf(fabsf(HI.A[0].x), fabsf(HI.B[0].x)), fmaxf(fabsf(HI.C[0].x), fabsf(HI.D[0].x)));
      const float mc = fmaxf(fmaxf(fabsf(HI.A[0].y), fabsf(HI.B[0].y)), fmaxf(fabsf(HI.C[0].y), fabsf(HI.D[0].y)));
      eacc = fmaf(mb + mc, at, eacc);
      if (!ok || !(y2 > 0)) alive = false;  // turned around: not a plane-form ray
      if (k + 2 < V.na) load_raw(k + 2, LO);  // node plane k+2 goes where the dead lower plane was, raw until used
    }
  };

  for (int k = A.k_first; k < k_end; k += 2) {
    if (!__any(alive)) break;
    layer(k, PA, PB);
    if (k + 1 < k_end) layer(k + 1, PB, PA);
  }

  double amp = 0, pol = 0;
  if (have) handoff_amp_pol(A, j, i, amp, pol);
  bool took_all = alive;
  if ((A.handoff & SR_HANDOFF_EXIT) && A.recover) {
    // the tile path's recovery inside the volume: the state on node plane k_last goes back into the ray's record (NaN when the
    // plane form lost it: the last segment's launch queues such records), the error sum into guard[]; nothing is queued
    // here and the ray's steps are counted where it finishes
    if (have) {
      handoff_exit(A, alive, j, i, y0, y1, y2, y3, y4, y5, y6, amp, pol);
      A.guard[j] = eacc;
    }
    return;
  }
  if (A.handoff & SR_HANDOFF_EXIT) {  // A12: on this slab's last node plane, hand the state over
    if (alive) handoff_exit(A, true, j, i, y0, y1, y2, y3, y4, y5, y6, amp, pol);
  } else {
    const bool finished = alive && y6 <= A.t_end;
    if (finished) {  // on the exit plane; vacuum to t_end (every RHS term is 0 outside the volume)
      const double rem = A.t_end - y6;
      write_outputs(A, j, fma(y2, rem, V.g[0][V.na - 1]), fma(y3, rem, y0), fma(y4, rem, y1), y2, y3, y4, y5, amp, pol);
      if (A.guard) A.guard[j] = kGuardK * eacc * A.guard_h6 / (float)y2;
    }
    took_all = finished;
  }
  // every ray this kernel does not finish goes to the next level with its input (s0 or the hand-off record) untouched
  queue_push(A.out_count, A.out_list, have && !took_all, (uint32_t)j);
  unsigned long long tot = took_all ? (unsigned long long)(V.na - 1) : 0ull;
  for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
  if ((threadIdx.x & 63) == 0 && tot) atomicAdd(sr::stripe(A.counters, A.step_stripe), tot);
}
