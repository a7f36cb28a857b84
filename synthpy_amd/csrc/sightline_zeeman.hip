// Zeeman-split lines along sightlines: sr_field_sightline_voigt's lines, each split by the magnetic field B of the sample into its
// pi and sigma components, and four Stokes parameters marched per frequency instead of one intensity (sr_field_sightline_zeeman;
// include/synthray.h states the rule).  No reference counterpart.  The decomposition is the family's (line_family.inc), in chunks
// of kZeemanChunk, a lane keeping (I, Q, U, Vs, tau) in registers; what is this kernel's own:
//
// Staging: lanes 0 .. chunk-1 stage what k_sightline_voigt's do (a = 0 where the table has no LG).  Lanes chunk .. 2*chunk-1
// carry B: lane chunk+s finds sample s's cell again (the same search, the same bits), reads the 24 corner values of B into the slots a staging lane keeps
// for V, and after the march blends them, turns B into the chord's frame and writes the sample's six numbers (wL, sP, cS, cQ, cU,
// cV: zeeman_node.inc) into the head of the same staged sample.  No lane's live state is larger than a staging lane's of
// k_sightline_voigt with V (an instantiation without V keeps V's slots for B).  A sample is 16 + 6*n_line float64: at 32 lines
// 1664 bytes, 16 samples a buffer (53 248 bytes; with the 8 KiB of the lattices 61 440, under the 64 KiB a workgroup may take
// without asking).
// March: per sample, line and component one shifted centre; a component is dropped when x*x > cut, exactly, and a wavefront skips
// a component whose window holds none of its frequencies (zeeman_outside).  The component table (q, g, s per component, an offset
// per line) is the same for every sample and lane: it is read where it lies with addresses that depend on the loop counters alone
// -- wavefront-uniform, scalar loads through the constant cache -- and takes no LDS.
// Instantiated per (dtype, Te field?, Z field?, Ti field?, V field?, FL); continuum, LK and LG are uniform branches.  Compiled with
// -ffp-contract=off, as its siblings.  With B NULL the entry is sr_field_sightline_voigt.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "emission_march.inc"

namespace {
#include "table_node.inc"

#include "sightline_march.inc"

#include "line_node.inc"

#include "voigt_node.inc"

#include "zeeman_node.inc"

#include "line_family.inc"

constexpr int kZeemanChunk = 16;  // samples staged at a time (sr_zeeman_chunk)
constexpr int kHead = 10 + kZeemanWords;  // float64 of a staged sample before its lines: k_sightline_voigt's ten and the six of B
static_assert(sizeof(double) * 2 * kZeemanChunk * (kHead + kVoigtWords * SR_MAX_LINES) + sizeof(double) * 2 * kMaxLattice <= kLdsBudget,
              "two buffers at 32 lines and the lattices must fit the LDS budget");
static_assert(2 * kZeemanChunk <= 64, "the staging lanes and the lanes that carry B are one wavefront");

struct ZeemanArgs {
  const double *omega, *e_ph, *c_omega;  // (n_freq)
  int n_freq, n_tiles;
  const double *LT, *LD, *w0, *ci, *LJ, *LK, *LG;  // the packed table where it lies
  int nT, nD, n_line, has_lk, has_lg, continuum;
  double cut, kL;
  const void *B;
  const double *frame;  // (n, 9): n^, e1, e2 of every chord
  const double *comp;   // (sum n_comp, 3): q, g, s
  const int *off;       // (n_line + 1): line l's components are off[l] .. off[l+1]-1
  double *Q, *U, *Vs;   // (n, n_freq)
};

template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI, bool HAS_V, int FL>
__global__ void __launch_bounds__(FL) k_sightline_zeeman(EmArgs A, LineArgs L, FlowArgs W, ZeemanArgs X) {
  extern __shared__ double s_stage[];  // [2][kZeemanChunk][kHead + 6*n_line]
  __shared__ double s_lat[2 * kMaxLattice];
  const int64_t i = blockIdx.x / (unsigned)X.n_tiles;
  const int tile = (int)(blockIdx.x % (unsigned)X.n_tiles);
  const int lane = (int)threadIdx.x;
  const int f = tile * FL + lane;
  const bool active = f < X.n_freq;
  const int64_t at = i * X.n_freq + f;
  const Line l = line_of(L, i);
  if (!l.hit) {  // the whole workgroup: one chord
    if (active) {
      A.I[at] = A.back ? A.back[at] : 0.0;
      X.Q[at] = 0.0;
      X.U[at] = 0.0;
      X.Vs[at] = 0.0;
      A.tau[at] = 0.0;
    }
    if (tile == 0 && lane == 0) {
      L.column[i] = 0.0;
      L.chord[i] = 0.0;
      L.steps[i] = 0;
    }
    return;
  }
  for (int k = lane; k < X.nT; k += FL) s_lat[k] = X.LT[k];
  for (int k = lane; k < X.nD; k += FL) s_lat[kMaxLattice + k] = X.LD[k];
  const int sT = top_step(X.nT), sD = top_step(X.nD);
  __syncthreads();
  const int n = l.n, NL = X.n_line;
  const int stride = kHead + kVoigtWords * NL;
  const double h = l.h, cut = X.cut;
  const int64_t sy = L.f.n[2], sx = (int64_t)L.f.n[1] * sy;
  const int k0 = A.toward > 0 ? 0 : n - 1, dk = A.toward > 0 ? 1 : -1;
  const double su = (double)A.toward / sqrt((l.d0 * l.d0 + l.d1 * l.d1) + l.d2 * l.d2);  // len of line_of, the same bits
  const bool cont = X.continuum != 0, has_lk = X.has_lk != 0, has_lg = X.has_lg != 0;
  const double *frame = X.frame + 9 * i;
  const LaneFreq w = lane_freq(X, f, active);
  double I = (active && A.back) ? A.back[at] : 0.0;
  double Q = 0.0, U = 0.0, Vs = 0.0, tau = 0.0, column = 0.0;

  // lanes 0 .. chunk-1 stage sample `mine` of a chunk, lanes chunk .. 2*chunk-1 carry its B
  const bool stager = lane < kZeemanChunk, carrier = lane >= kZeemanChunk && lane < 2 * kZeemanChunk;
  const int mine = stager ? lane : lane - kZeemanChunk;
  FlowSample<T, HAS_TE, HAS_Z, HAS_TI, true> cur{};
  if (stager && mine < n) fetch_staged<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, W, L.f, sx, sy, l, k0 + mine * dk, cur);
  if (carrier && mine < n) fetch_vector<T, HAS_TE, HAS_Z, HAS_TI>(X.B, L.f, sx, sy, l, k0 + mine * dk, cur);
  int buf = 0;
  for (int m0 = 0; m0 < n; m0 += kZeemanChunk, buf ^= 1) {
    const int cnt = min(kZeemanChunk, n - m0);
    // this chunk's samples (their reads were issued a chunk ago): blend, the lattice search, the lines' constants, to LDS
    if (stager && mine < cnt) {
      double ne, Te, Z, Ti, V[3];
      blend_staged<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, cur, ne, Te, Z, Ti, V);
      const TableTerms t = table_terms(s_lat, X.nT, sT, s_lat + kMaxLattice, X.nD, sD, 1.0, ne, Te, Z);
      const bool dark = t.dark || Ti <= 0.0;  // outside the box ne = 0: dark
      double beta = 0.0;
      if (HAS_V) beta = ((((V[0] * l.d0 + V[1] * l.d1) + V[2] * l.d2)) * su) / sr::kC;
      double *S = s_stage + (size_t)(buf * kZeemanChunk + mine) * stride;
      stage_head(S, cont, dark, ne, Te, Z, h);
      if (!dark) {
        const int o = t.o * NL, st = X.nD * NL;
#pragma unroll 1
        for (int q = 0; q < NL; ++q) {
          double *P = S + kHead + kVoigtWords * q;
          if (has_lg) {
            const VoigtConst k = voigt_const(X.w0[q], X.ci[q], X.LJ, X.LK, X.LG, has_lk, o + q, NL, st, t.ft, t.fd, beta, Ti);
            P[0] = k.wc, P[1] = k.iw, P[2] = k.aJ, P[3] = k.aK, P[4] = k.a;
          } else {  // Gaussian components through the same V: a = 0
            const LineConst k = line_const(X.w0[q], X.ci[q], X.LJ, X.LK, has_lk, o + q, NL, st, t.ft, t.fd, beta, Ti);
            P[0] = k.wc, P[1] = k.iw, P[2] = k.aJ, P[3] = k.aK, P[4] = 0.0;
          }
        }
      }
    }
    if (carrier && mine < cnt) {
      double B[3];
      blend_vector<T, HAS_TE, HAS_Z, HAS_TI>(cur, B);
      const ZeemanSample z = zeeman_sample(B, frame, X.kL);
      double *S = s_stage + (size_t)(buf * kZeemanChunk + mine) * stride + 10;
      S[0] = z.wL, S[1] = z.sP, S[2] = z.cS, S[3] = z.cQ, S[4] = z.cU, S[5] = z.cV;
    }
    __syncthreads();
    // the next chunk's cells and corner reads, in flight during this chunk's march
    cur.s.in = false;
    if (stager && m0 + kZeemanChunk + mine < n)
      fetch_staged<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, W, L.f, sx, sy, l, k0 + (m0 + kZeemanChunk + mine) * dk, cur);
    if (carrier && m0 + kZeemanChunk + mine < n)
      fetch_vector<T, HAS_TE, HAS_Z, HAS_TI>(X.B, L.f, sx, sy, l, k0 + (m0 + kZeemanChunk + mine) * dk, cur);
    if (active) {
#pragma unroll 1
      for (int s = 0; s < cnt; ++s) {
        const double *S = s_stage + (size_t)(buf * kZeemanChunk + s) * stride;
        const int flags = (int)S[1];
        double jI = 0.0, jQ = 0.0, jU = 0.0, jV = 0.0, aL = 0.0;
        bool counted = false;
        if (!(flags & 2)) {
          ZeemanSample z;
          z.wL = S[10], z.sP = S[11], z.cS = S[12], z.cQ = S[13], z.cU = S[14], z.cV = S[15];
#pragma unroll 1
          for (int q = 0; q < NL; ++q) {
            const double *P = S + kHead + kVoigtWords * q;
            const double wc = P[0], iw = P[1], a = P[4];
            double P0 = 0.0, Pp = 0.0, Pm = 0.0;
            bool any = false;
            const int k1 = X.off[q + 1];
#pragma unroll 1
            for (int k = X.off[q]; k < k1; ++k) {
              const double cq = X.comp[3 * k], sh = X.comp[3 * k + 1] * z.wL, sk = X.comp[3 * k + 2];
              if (zeeman_outside(wc, sh, iw, w.wmin, w.wmax, cut)) continue;  // the same for every lane of the wavefront
              double x;
              if (zeeman_term(w.om, wc, sh, iw, cut, x)) {
                const double v = sk * voigt(a, x);
                if (cq == 0.0)
                  P0 = P0 + v;
                else if (cq > 0.0)
                  Pp = Pp + v;
                else
                  Pm = Pm + v;
                any = true;
              }
            }
            if (any) {
              zeeman_line(z, P[2], P[3], P0, Pp, Pm, jI, jQ, jU, jV, aL);
              counted = true;
            }
          }
        }
        double ac = 0.0, Sc = 0.0;
        if (cont) {
          NodeTerms t;
          t.dark = (flags & 1) != 0;
          t.Te = S[2], t.n = S[3], t.wp = S[4], t.L = S[5], t.num = S[6], t.zc = S[7], t.it = S[8];
          node_band(t, w.om, w.eph, w.com, ac, Sc);
        }
        if (counted) {
          zeeman_update(ac, Sc, jI, jQ, jU, jV, aL, h, I, Q, U, Vs, tau);
        } else {
          continuum_update(cont, ac, Sc, h, I, Q, U, Vs, tau);
        }
        column = column + S[0];
      }
    }
  }
  if (active) {
    A.I[at] = I;
    X.Q[at] = Q;
    X.U[at] = U;
    X.Vs[at] = Vs;
    A.tau[at] = tau;
  }
  if (tile == 0 && lane == 0) {
    L.column[i] = column;
    L.chord[i] = l.chord;
    L.steps[i] = n;
  }
}

}  // namespace

extern "C" int sr_zeeman_chunk(void) { return kZeemanChunk; }

extern "C" int sr_field_sightline_zeeman(const sr_field *ne, const sr_field *Te, const sr_field *Ti, const sr_field *Z, const sr_field *V,
                                         const sr_field *B, const sr_zeeman_table *lines, const sr_voigt_params *p, int64_t n,
                                         const double *origin, const double *dir, const double *ref, int32_t n_freq, const double *omega,
                                         const double *e_ph, const double *c_omega, const double *backlight, double *I, double *Q,
                                         double *U, double *Vs, double *tau, double *column, double *chord, int32_t *steps,
                                         double *kernel_ms) {
  const char *who = "sr_field_sightline_zeeman";
  Family F{who, ne, Te, Ti, Z, V, p ? &p->march : nullptr, n, origin, dir, n_freq, omega, e_ph, c_omega, backlight, I, tau, column, chord,
           steps, kernel_ms};
  Polarised P{B, ref, Q, U, Vs, lines};
  if (B == nullptr) return without_field(F, P, p);
  SR_RC(check_family(F, [&] {  // LG NULL does not delegate: wing is always read
    SR_RC(check_zeeman_table(who, lines));
    return check_wing(who, p->wing);
  }, &P));
  ZeemanArgs X{};
  X.cut = p->wing * p->wing;
  X.kL = kLineE / (2.0 * kZeemanMe);
  const size_t lds = sizeof(double) * 2 * kZeemanChunk * (kHead + kVoigtWords * (size_t)lines->voigt.lines.n_line);  // at most 53 248 bytes
  return run_family<kPolarisedArgs>(F, &lines->voigt, &P, X, lds, [](auto f64, auto te, auto z, auto ti, auto v, auto narrow) {
    return &k_sightline_zeeman<std::conditional_t<f64(), double, float>, te(), z(), ti(), v(), narrow() ? 64 : 256>;
  });
}
