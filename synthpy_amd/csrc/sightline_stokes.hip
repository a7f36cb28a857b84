// Polarised transfer along sightlines: sr_field_sightline_zeeman's chords, samples, components and coefficients, with the full 4 x 4
// absorption matrix in the update -- dichroism (hQ, hU, hV), magneto-optical rotation inside the lines (rQ, rU, rV, from the
// imaginary part of w(x + i a)) and Faraday rotation of the continuum -- and a polarised backlight (sr_field_sightline_stokes;
// include/synthray.h states the rule).  No reference counterpart.  k_sightline_zeeman's decomposition, word for word: a workgroup
// owns one chord and one tile of FL frequencies, a lane one frequency with its (I, Q, U, Vs, tau) in registers; the chord's samples
// go through LDS in chunks of kStokesChunk, in two buffers; lanes 0 .. chunk-1 stage the samples, lanes chunk .. 2*chunk-1 carry B
// and write the sample's six angular numbers and, as a seventh word, B.n^ itself (for the continuum's rotation).  A sample is
// 18 + 6*n_line float64: at 32 lines 1680 bytes, 16 samples a buffer (53 760 bytes; with the 8 KiB of the lattices 61 952, under
// the 64 KiB a workgroup may take without asking).
// March: per sample, line and component one voigt_w -- both profiles from one evaluation -- under k_sightline_zeeman's window tests;
// the 4 x 4 propagator O and the particular solution p of stokes_update are live only after the line loop, when the Voigt
// temporaries are dead, in registers.  A sample and frequency without dichroism and rotation takes zeeman_update's operations.
// Instantiated per (dtype, Te field?, Z field?, Ti field?, V field?, FL); continuum, LK, LG, faraday and pol are uniform branches.
// Compiled with -ffp-contract=off, as its siblings.  With B NULL the entry is sr_field_sightline_voigt.
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

#include "stokes_node.inc"

constexpr int kStokesChunk = 16;  // samples staged at a time (sr_stokes_chunk)
constexpr int kHead = 10 + kStokesWords;  // float64 of a staged sample before its lines: an even number keeps a line's reads 16-byte
static_assert(sizeof(double) * 2 * kStokesChunk * (kHead + kVoigtWords * SR_MAX_LINES) + sizeof(double) * 2 * kMaxLattice <= kLdsBudget,
              "two buffers at 32 lines and the lattices must fit the LDS budget");
static_assert(2 * kStokesChunk <= 64, "the staging lanes and the lanes that carry B are one wavefront");
static_assert(kHead % 2 == 0, "a staged line starts on 16 bytes");

struct StokesArgs {
  const double *omega, *e_ph, *c_omega;  // (n_freq)
  int n_freq, n_tiles;
  const double *LT, *LD, *w0, *ci, *LJ, *LK, *LG;  // the packed table where it lies
  int nT, nD, n_line, has_lk, has_lg, continuum, faraday, has_pol;
  double cut, kL, kF2;  // kF2 = 2.0*kF
  double pq, pu, pv;    // the backlight's (q, u, v); not read where has_pol is 0
  const void *B;
  const double *frame;  // (n, 9): n^, e1, e2 of every chord
  const double *comp;   // (sum n_comp, 3): q, g, s
  const int *off;       // (n_line + 1): line l's components are off[l] .. off[l+1]-1
  double *Q, *U, *Vs;   // (n, n_freq)
};

template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI, bool HAS_V, int FL>
__global__ void __launch_bounds__(FL) k_sightline_stokes(EmArgs A, LineArgs L, FlowArgs W, StokesArgs X) {
  extern __shared__ double s_stage[];  // [2][kStokesChunk][kHead + 6*n_line]
  __shared__ double s_lat[2 * kMaxLattice];
  const int64_t i = blockIdx.x / (unsigned)X.n_tiles;
  const int tile = (int)(blockIdx.x % (unsigned)X.n_tiles);
  const int lane = (int)threadIdx.x;
  const int f = tile * FL + lane;
  const bool active = f < X.n_freq;
  const int64_t at = i * X.n_freq + f;
  const Line l = line_of(L, i);
  const bool has_pol = X.has_pol != 0;
  // the march starts at I0*(1, q, u, v); a chord that misses the box returns this start
  double I = (active && A.back) ? A.back[at] : 0.0;
  double Q = has_pol ? I * X.pq : 0.0, U = has_pol ? I * X.pu : 0.0, Vs = has_pol ? I * X.pv : 0.0;
  if (!l.hit) {  // the whole workgroup: one chord
    if (active) {
      A.I[at] = I;
      X.Q[at] = Q;
      X.U[at] = U;
      X.Vs[at] = Vs;
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
  const bool cont = X.continuum != 0, has_lk = X.has_lk != 0, has_lg = X.has_lg != 0, faraday = X.faraday != 0;
  const double *frame = X.frame + 9 * i;
  // the frequency's constants; an idle lane of the last tile takes the last frequency's and stores nothing
  const int fc = active ? f : X.n_freq - 1;
  const double om = X.omega[fc], eph = X.e_ph[fc], com = X.c_omega[fc];
  // the wavefront's span of frequencies: idle lanes widen nothing
  const double wmin = wave_extreme<true>(active ? om : HUGE_VAL), wmax = wave_extreme<false>(active ? om : -HUGE_VAL);
  double tau = 0.0, column = 0.0;

  // lanes 0 .. chunk-1 stage sample `mine` of a chunk, lanes chunk .. 2*chunk-1 carry its B
  const bool stager = lane < kStokesChunk, carrier = lane >= kStokesChunk && lane < 2 * kStokesChunk;
  const int mine = stager ? lane : lane - kStokesChunk;
  FlowSample<T, HAS_TE, HAS_Z, HAS_TI, true> cur{};
  if (stager && mine < n) fetch_staged<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, W, L.f, sx, sy, l, k0 + mine * dk, cur);
  if (carrier && mine < n) fetch_vector<T, HAS_TE, HAS_Z, HAS_TI>(X.B, L.f, sx, sy, l, k0 + mine * dk, cur);
  int buf = 0;
  for (int m0 = 0; m0 < n; m0 += kStokesChunk, buf ^= 1) {
    const int cnt = min(kStokesChunk, n - m0);
    // this chunk's samples (their reads were issued a chunk ago): blend, the lattice search, the lines' constants, to LDS
    if (stager && mine < cnt) {
      double ne, Te, Z, Ti, V[3];
      blend_staged<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, cur, ne, Te, Z, Ti, V);
      const TableTerms t = table_terms(s_lat, X.nT, sT, s_lat + kMaxLattice, X.nD, sD, 1.0, ne, Te, Z);
      const bool dark = t.dark || Ti <= 0.0;  // outside the box ne = 0: dark
      double beta = 0.0;
      if (HAS_V) beta = ((((V[0] * l.d0 + V[1] * l.d1) + V[2] * l.d2)) * su) / sr::kC;
      double *S = s_stage + (size_t)(buf * kStokesChunk + mine) * stride;
      int flags = dark ? 2 : 0;
      S[0] = ne * h;
      if (cont) {
        const NodeTerms c = node_terms(ne, Te, Z);
        flags |= c.dark ? 1 : 0;
        S[2] = c.Te, S[3] = c.n, S[4] = c.wp, S[5] = c.L, S[6] = c.num, S[7] = c.zc, S[8] = c.it;
      }
      S[1] = (double)flags;
      if (!dark) {
        const int o = t.o * NL, st = X.nD * NL;
#pragma unroll 1
        for (int q = 0; q < NL; ++q) {
          double *P = S + kHead + kVoigtWords * q;
          if (has_lg) {
            const VoigtConst k = voigt_const(X.w0[q], X.ci[q], X.LJ, X.LK, X.LG, has_lk, o + q, NL, st, t.ft, t.fd, beta, Ti);
            P[0] = k.wc, P[1] = k.iw, P[2] = k.aJ, P[3] = k.aK, P[4] = k.a;
          } else {  // Gaussian components through the same w: a = 0
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
      double *S = s_stage + (size_t)(buf * kStokesChunk + mine) * stride + 10;
      S[0] = z.wL, S[1] = z.sP, S[2] = z.cS, S[3] = z.cQ, S[4] = z.cU, S[5] = z.cV;
      S[6] = (B[0] * frame[0] + B[1] * frame[1]) + B[2] * frame[2];  // zeeman_sample's Bn, the same bits
    }
    __syncthreads();
    // the next chunk's cells and corner reads, in flight during this chunk's march
    cur.s.in = false;
    if (stager && m0 + kStokesChunk + mine < n)
      fetch_staged<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, W, L.f, sx, sy, l, k0 + (m0 + kStokesChunk + mine) * dk, cur);
    if (carrier && m0 + kStokesChunk + mine < n)
      fetch_vector<T, HAS_TE, HAS_Z, HAS_TI>(X.B, L.f, sx, sy, l, k0 + (m0 + kStokesChunk + mine) * dk, cur);
    if (active) {
#pragma unroll 1
      for (int s = 0; s < cnt; ++s) {
        const double *S = s_stage + (size_t)(buf * kStokesChunk + s) * stride;
        const int flags = (int)S[1];
        double jI = 0.0, jQ = 0.0, jU = 0.0, jV = 0.0, hI = 0.0, hQ = 0.0, hU = 0.0, hV = 0.0, rQ = 0.0, rU = 0.0, rV = 0.0;
        bool counted = false;
        if (!(flags & 2)) {
          ZeemanSample z;
          z.wL = S[10], z.sP = S[11], z.cS = S[12], z.cQ = S[13], z.cU = S[14], z.cV = S[15];
#pragma unroll 1
          for (int q = 0; q < NL; ++q) {
            const double *P = S + kHead + kVoigtWords * q;
            const double wc = P[0], iw = P[1], a = P[4];
            double P0 = 0.0, Pp = 0.0, Pm = 0.0, R0 = 0.0, Rp = 0.0, Rm = 0.0;
            bool any = false;
            const int k1 = X.off[q + 1];
#pragma unroll 1
            for (int k = X.off[q]; k < k1; ++k) {
              const double cq = X.comp[3 * k], sh = X.comp[3 * k + 1] * z.wL, sk = X.comp[3 * k + 2];
              if (zeeman_outside(wc, sh, iw, wmin, wmax, cut)) continue;  // the same for every lane of the wavefront
              double x;
              if (zeeman_term(om, wc, sh, iw, cut, x)) {
                double H, D;
                voigt_w(a, x, &H, &D);
                const double v = sk * H, d = sk * D;
                if (cq == 0.0)
                  P0 = P0 + v, R0 = R0 + d;
                else if (cq > 0.0)
                  Pp = Pp + v, Rp = Rp + d;
                else
                  Pm = Pm + v, Rm = Rm + d;
                any = true;
              }
            }
            if (any) {
              stokes_line(z, P[2], P[3], P0, Pp, Pm, R0, Rp, Rm, jI, jQ, jU, jV, hI, hQ, hU, hV, rQ, rU, rV);
              counted = true;
            }
          }
        }
        if (faraday) rV = rV + ((X.kF2 * (S[0] / h)) * S[16]) / (om * om);
        double ac = 0.0, Sc = 0.0;
        if (cont) {
          NodeTerms t;
          t.dark = (flags & 1) != 0;
          t.Te = S[2], t.n = S[3], t.wp = S[4], t.L = S[5], t.num = S[6], t.zc = S[7], t.it = S[8];
          node_band(t, om, eph, com, ac, Sc);
        }
        const bool scalar = hQ == 0.0 && hU == 0.0 && hV == 0.0 && rQ == 0.0 && rU == 0.0 && rV == 0.0;
        if (!scalar) {
          stokes_update(ac, Sc, jI, jQ, jU, jV, hI, hQ, hU, hV, rQ, rU, rV, h, I, Q, U, Vs, tau);
        } else if (counted) {  // sr_field_sightline_zeeman's update, its operations
          zeeman_update(ac, Sc, jI, jQ, jU, jV, hI, h, I, Q, U, Vs, tau);
        } else if (cont) {
          const double dtau = ac * h;
          const double E = exp(-dtau);
          I = I * E + Sc * (-expm1(-dtau));
          Q = Q * E;
          U = U * E;
          Vs = Vs * E;
          tau = tau + dtau;
        } else {  // that update with ac = Sc = 0, as the siblings write it
          I = I + 0.0;
          Q = Q + 0.0;
          U = U + 0.0;
          Vs = Vs + 0.0;
          tau = tau + 0.0;
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

extern "C" int sr_stokes_chunk(void) { return kStokesChunk; }

extern "C" int sr_field_sightline_stokes(const sr_field *ne, const sr_field *Te, const sr_field *Ti, const sr_field *Z, const sr_field *V,
                                         const sr_field *B, const sr_zeeman_table *lines, const sr_voigt_params *p, int64_t n,
                                         const double *origin, const double *dir, const double *ref, int32_t n_freq, const double *omega,
                                         const double *e_ph, const double *c_omega, const double *backlight, const double *pol,
                                         int32_t faraday, double *I, double *Q, double *U, double *Vs, double *tau, double *column,
                                         double *chord, int32_t *steps, double *kernel_ms) {
  const char *who = "sr_field_sightline_stokes";
  SR_CHECK(faraday == 0 || faraday == 1, "%s: faraday must be 0 or 1, got %d", who, faraday);
  if (pol) {
    SR_CHECK(std::isfinite(pol[0]) && std::isfinite(pol[1]) && std::isfinite(pol[2]), "%s: non-finite pol", who);
    SR_CHECK((pol[0] * pol[0] + pol[1] * pol[1]) + pol[2] * pol[2] <= 1.0 + kStokesPolTol,
             "%s: pol = (%g, %g, %g) lies outside the unit ball", who, pol[0], pol[1], pol[2]);
  }
  if (B == nullptr) {  // no field: sr_field_sightline_voigt's rule, kernel and bits; the component table and ref are not read
    SR_CHECK(!faraday, "%s: faraday needs B", who);
    SR_CHECK(pol == nullptr, "%s: pol needs B", who);
    SR_CHECK(lines != nullptr, "%s: NULL line table", who);
    SR_CHECK(n >= 0 && n_freq >= 0, "%s: n and n_freq must not be negative, got %lld and %d", who, (long long)n, n_freq);
    if (int rc = sr_field_sightline_voigt(ne, Te, Ti, Z, V, &lines->voigt, p, n, origin, dir, n_freq, omega, e_ph, c_omega, backlight, I,
                                          tau, column, chord, steps, kernel_ms))
      return rc;
    const size_t bytes = sizeof(double) * (size_t)n * (size_t)n_freq;
    for (double *out : {Q, U, Vs})
      if (out && bytes) memset(out, 0, bytes);
    return SR_OK;
  }
  // sr_field_sightline_zeeman's checks, in its order
  SR_CHECK(p != nullptr && origin != nullptr && dir != nullptr && I != nullptr && tau != nullptr, "%s: NULL argument", who);
  SR_CHECK(ref != nullptr && Q != nullptr && U != nullptr && Vs != nullptr, "%s: NULL ref, Q, U or Vs (B is given)", who);
  SR_CHECK(omega != nullptr && e_ph != nullptr && c_omega != nullptr, "%s: NULL omega, e_ph or c_omega", who);
  SR_CHECK(n >= 0, "%s: n must not be negative, got %lld", who, (long long)n);
  SR_CHECK(n_freq >= 0, "%s: n_freq must not be negative, got %d", who, n_freq);
  if (n_freq != 0) SR_RC(check_bands(who, "frequency", n_freq, SR_MAX_FREQS, omega, e_ph, c_omega));
  const sr_lines_params *m = &p->march;
  SR_RC(check_march(who, m->toward, m->step, m->max_steps));
  SR_RC(check_zeeman_table(who, lines));
  SR_CHECK(p->wing > 0.0, "%s: wing must be positive (+inf is allowed), got %g", who, p->wing);
  const int fl = lane_width(n_freq);
  const int64_t n_tiles = (n_freq + fl - 1) / fl;
  SR_CHECK(n_tiles == 0 || n <= (int64_t)2147483647 / n_tiles, "%s: n x frequency tiles exceeds 2^31 - 1 workgroups", who);
  std::vector<double> frames;
  SR_RC(chord_frames(who, n, m->toward, dir, ref, frames));
  SR_RC(check_lines(who, n, origin, dir, ne, Te, Z));
  SR_RC(sr::check_fields(who, ne, "ne", {{"Ti", Ti, 1}, {"V", V, 3}, {"B", B, 3}}));
  if (kernel_ms) *kernel_ms = 0.0;
  if (n == 0 || n_freq == 0) return SR_OK;
  SR_RC(sr::ensure_init());
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;

  const sr_line_table *lt = &lines->voigt.lines;
  const size_t nl = (size_t)lt->n_line, entries = (size_t)lt->nT * lt->nD * nl;
  std::vector<double> pack = pack_line_table(lt);
  if (lines->voigt.LG) {  // pack_voigt_table's block
    const size_t cells = (size_t)lt->nT * lt->nD, start = pack.size();
    pack.resize(start + entries);
    for (size_t q = 0; q < nl; ++q)
      for (size_t k = 0; k < cells; ++k) pack[start + k * nl + q] = lines->voigt.LG[q * cells + k];
  }
  std::vector<int> off(nl + 1, 0);
  for (size_t q = 0; q < nl; ++q) off[q + 1] = off[q] + lines->n_comp[q];
  const size_t n_comp = (size_t)off[nl];
  const size_t nf = (size_t)n_freq, map_bytes = sizeof(double) * nf * (size_t)n, freq_bytes = sizeof(double) * nf;

  // one scratch block: the chords' pieces (take_lines) | Q | U | Vs | frames | omega | e_ph | c_omega | table | components | offsets
  EmArgs A{};
  LineArgs L{};
  FlowArgs W{};
  StokesArgs X{};
  double *tab = nullptr;
  sr::Carve carve;
  take_lines(carve, A, L, ne, n, m->step, m->max_steps, nf, backlight != nullptr);
  carve.take(&X.Q, nf * (size_t)n);
  carve.take(&X.U, nf * (size_t)n);
  carve.take(&X.Vs, nf * (size_t)n);
  carve.take(&X.frame, frames.size());
  carve.take(&X.omega, nf);
  carve.take(&X.e_ph, nf);
  carve.take(&X.c_omega, nf);
  carve.take(&tab, pack.size());
  carve.take(&X.comp, 3 * n_comp);
  carve.take(&X.off, off.size());
  if (!carve.alloc()) return SR_ERR_HIP;
  fill_fields(A, ne, Te, Z, m->toward, m->Te, m->Z, 0, nullptr, nullptr, nullptr);  // the frequencies' constants are X's
  W.Ti = Ti ? Ti->data : nullptr;
  W.V = V ? V->data : nullptr;
  X.B = B->data;
  X.n_freq = n_freq;
  X.n_tiles = (int)n_tiles;
  X.LT = tab;
  X.LD = X.LT + lt->nT;
  X.w0 = X.LD + lt->nD;
  X.ci = X.w0 + nl;
  X.LJ = X.ci + nl;
  X.LK = X.LJ + entries;  // not read where has_lk is false
  X.LG = lt->LK ? X.LK + entries : X.LK;  // not read where has_lg is false
  X.nT = lt->nT;
  X.nD = lt->nD;
  X.n_line = lt->n_line;
  X.has_lk = lt->LK != nullptr;
  X.has_lg = lines->voigt.LG != nullptr;
  X.continuum = m->continuum != 0;
  X.faraday = faraday;
  X.has_pol = pol != nullptr;
  if (pol) X.pq = pol[0], X.pu = pol[1], X.pv = pol[2];
  X.cut = p->wing * p->wing;
  X.kL = kLineE / (2.0 * kZeemanMe);
  X.kF2 = 2.0 * (((kLineE * kLineE) * kLineE) / ((((2.0 * kStokesEps0) * kZeemanMe) * kZeemanMe) * kStokesC));

  SR_RC(upload_lines(A, L, origin, dir, backlight, map_bytes, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(X.frame), frames.data(), sizeof(double) * frames.size(), hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(X.omega), omega, freq_bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(X.e_ph), e_ph, freq_bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(X.c_omega), c_omega, freq_bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(tab, pack.data(), sizeof(double) * pack.size(), hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(X.comp), lines->comp, sizeof(double) * 3 * n_comp, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<int *>(X.off), off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, st));
  SR_HIP(hipEventRecord(c.ev[0], st));
  const unsigned grid = (unsigned)(n * n_tiles);
  const size_t lds = sizeof(double) * 2 * kStokesChunk * (kHead + kVoigtWords * nl);  // at most 53 760 bytes
  sr::with_flags(
      [&](auto f64, auto te, auto z, auto ti, auto v, auto narrow) {
        using T = std::conditional_t<decltype(f64)::value, double, float>;
        constexpr int kFl = decltype(narrow)::value ? 64 : 256;
        hipLaunchKernelGGL((k_sightline_stokes<T, decltype(te)::value, decltype(z)::value, decltype(ti)::value, decltype(v)::value, kFl>),
                           dim3(grid), dim3(kFl), lds, st, A, L, W, X);
      },
      (bool)ne->is_f64, Te != nullptr, Z != nullptr, Ti != nullptr, V != nullptr, fl == 64);
  // finish_lines, with Q, U and Vs beside I and tau
  SR_HIP(hipGetLastError());
  SR_HIP(hipEventRecord(c.ev[1], st));
  SR_HIP(hipMemcpyAsync(Q, X.Q, map_bytes, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(U, X.U, map_bytes, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(Vs, X.Vs, map_bytes, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(I, A.I, map_bytes, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(tau, A.tau, map_bytes, hipMemcpyDeviceToHost, st));
  const size_t N = (size_t)n;
  if (column) SR_HIP(hipMemcpyAsync(column, L.column, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  if (chord) SR_HIP(hipMemcpyAsync(chord, L.chord, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  if (steps) SR_HIP(hipMemcpyAsync(steps, L.steps, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
  return sr::finish_timed(c, kernel_ms);
}
