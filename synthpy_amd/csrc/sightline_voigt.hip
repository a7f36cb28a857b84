// Voigt lines along sightlines: sr_field_sightline_lines' Doppler-shifted lines with a Lorentzian (Stark, natural) half-width from
// the table, so that every line is a Voigt profile (sr_field_sightline_voigt; include/synthray.h states the rule).  No reference
// counterpart.  The decomposition is the family's (line_family.inc), in chunks of kVoigtChunk; what is this kernel's own:
//
// Staging: per line one more bilinear read and exp than k_sightline_lines, for the damping parameter a = gam*iw (voigt_node.inc's
// voigt_const).  A staged line is five float64 padded to six -- three 16-byte reads, every marching lane at the same address, a
// broadcast -- and a sample 10 + 6*n_line float64: at 32 lines 1616 bytes, so the two buffers hold 16 samples each (51 712 bytes;
// with the 8 KiB of the lattices 59 904, under the 64 KiB a workgroup may take without asking).
// March: a term is dropped when x*x > cut (cut = wing*wing from the host, +inf: never), exactly, so a wavefront skips a line whose
// window holds none of its frequencies (voigt_outside on the wavefront's least and greatest frequency).  A counted term costs one
// V(a, x).  Every lane of a wavefront has the same a, so V's branches on a are uniform; the branch on x*x + a*a is not, and the
// compiler's exec-mask branches already leave a region out when no lane of the wavefront is in it -- the far wing, one division
// and about a hundred multiply-adds, is the common case and the first one tested, and a wavefront wholly in it never enters the
// sampled sum (14 or 19 divisions, three exp, three sincos).
// The table is pack_line_table's block followed by LG[nT][nD][n_line].  Instantiated per (dtype, Te field?, Z field?, Ti field?,
// V field?, FL); continuum and LK are uniform branches.  Compiled with -ffp-contract=off, as its siblings: column, chord and steps
// are the bits k_sightlines gives, and where every term is dropped I and tau are the bits of k_sightline_spectra.  With LG NULL
// the entry is sr_field_sightline_lines.
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

constexpr int kVoigtChunk = 16;  // samples staged at a time (sr_voigt_chunk)
constexpr int kHead = 10;        // float64 of a staged sample before its lines: the family's head
static_assert(sizeof(double) * 2 * kVoigtChunk * (kHead + kVoigtWords * SR_MAX_LINES) + sizeof(double) * 2 * kMaxLattice <= kLdsBudget,
              "two buffers at 32 lines and the lattices must fit the LDS budget");

struct VoigtArgs {
  const double *omega, *e_ph, *c_omega;  // (n_freq)
  int n_freq, n_tiles;
  const double *LT, *LD, *w0, *ci, *LJ, *LK, *LG;  // the packed table where it lies
  int nT, nD, n_line, has_lk, continuum;
  double cut;
};

template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI, bool HAS_V, int FL>
__global__ void __launch_bounds__(FL) k_sightline_voigt(EmArgs A, LineArgs L, FlowArgs W, VoigtArgs X) {
  extern __shared__ double s_stage[];  // [2][kVoigtChunk][kHead + 6*n_line]
  __shared__ double s_lat[2 * kMaxLattice];
  const int64_t i = blockIdx.x / (unsigned)X.n_tiles;
  const int tile = (int)(blockIdx.x % (unsigned)X.n_tiles);
  const int lane = (int)threadIdx.x;
  const int f = tile * FL + lane;
  const bool active = f < X.n_freq;
  const int64_t at = i * X.n_freq + f;
  const Line l = line_of(L, i);
  if (!l.hit) {  // the whole workgroup: one chord
    store_missed(A, L, i, at, active, tile, lane);
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
  const bool cont = X.continuum != 0, has_lk = X.has_lk != 0;
  const LaneFreq w = lane_freq(X, f, active);
  double I = (active && A.back) ? A.back[at] : 0.0;
  double tau = 0.0, column = 0.0;

  FlowSample<T, HAS_TE, HAS_Z, HAS_TI, HAS_V> cur{};
  if (lane < kVoigtChunk && lane < n) fetch_sample<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, W, L.f, sx, sy, l, k0 + lane * dk, cur);
  int buf = 0;
  for (int m0 = 0; m0 < n; m0 += kVoigtChunk, buf ^= 1) {
    const int cnt = min(kVoigtChunk, n - m0);
    // this chunk's samples (their reads were issued a chunk ago): blend, the lattice search, the lines' constants, to LDS
    if (lane < cnt) {
      double ne, Te, Z, Ti, V[3];
      blend_sample<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, cur, ne, Te, Z, Ti, V);
      const TableTerms t = table_terms(s_lat, X.nT, sT, s_lat + kMaxLattice, X.nD, sD, 1.0, ne, Te, Z);
      const bool dark = t.dark || Ti <= 0.0;  // outside the box ne = 0: dark
      double beta = 0.0;
      if (HAS_V) beta = ((((V[0] * l.d0 + V[1] * l.d1) + V[2] * l.d2)) * su) / sr::kC;
      double *S = s_stage + (size_t)(buf * kVoigtChunk + lane) * stride;
      stage_head(S, cont, dark, ne, Te, Z, h);
      if (!dark) {
        const int o = t.o * NL, st = X.nD * NL;
#pragma unroll 1
        for (int q = 0; q < NL; ++q) {
          const VoigtConst k = voigt_const(X.w0[q], X.ci[q], X.LJ, X.LK, X.LG, has_lk, o + q, NL, st, t.ft, t.fd, beta, Ti);
          double *P = S + kHead + kVoigtWords * q;
          P[0] = k.wc, P[1] = k.iw, P[2] = k.aJ, P[3] = k.aK, P[4] = k.a;
        }
      }
    }
    __syncthreads();
    // the next chunk's cells and corner reads, in flight during this chunk's march
    cur.s.in = false;
    if (lane < kVoigtChunk && m0 + kVoigtChunk + lane < n)
      fetch_sample<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, W, L.f, sx, sy, l, k0 + (m0 + kVoigtChunk + lane) * dk, cur);
    if (active) {
#pragma unroll 1
      for (int s = 0; s < cnt; ++s) {
        const double *S = s_stage + (size_t)(buf * kVoigtChunk + s) * stride;
        const int flags = (int)S[1];
        double j = 0.0, aL = 0.0;
        bool counted = false;
        if (!(flags & 2)) {
#pragma unroll 1
          for (int q = 0; q < NL; ++q) {
            const double *P = S + kHead + kVoigtWords * q;
            const double wc = P[0], iw = P[1];
            if (voigt_outside(wc, iw, w.wmin, w.wmax, cut)) continue;  // the same for every lane of the wavefront
            double x;
            if (voigt_term(w.om, wc, iw, cut, x)) {
              const double phi = voigt(P[4], x);
              j = j + P[2] * phi;
              aL = aL + P[3] * phi;
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
          line_update(ac, Sc, j, aL, h, I, tau);
        } else {
          continuum_update(cont, ac, Sc, h, I, tau);
        }
        column = column + S[0];
      }
    }
  }
  if (active) {
    A.I[at] = I;
    A.tau[at] = tau;
  }
  if (tile == 0 && lane == 0) {
    L.column[i] = column;
    L.chord[i] = l.chord;
    L.steps[i] = n;
  }
}

}  // namespace

extern "C" int sr_voigt_chunk(void) { return kVoigtChunk; }

extern "C" int sr_field_sightline_voigt(const sr_field *ne, const sr_field *Te, const sr_field *Ti, const sr_field *Z, const sr_field *V,
                                        const sr_voigt_table *lines, const sr_voigt_params *p, int64_t n, const double *origin,
                                        const double *dir, int32_t n_freq, const double *omega, const double *e_ph,
                                        const double *c_omega, const double *backlight, double *I, double *tau, double *column,
                                        double *chord, int32_t *steps, double *kernel_ms) {
  const char *who = "sr_field_sightline_voigt";
  Family F{who, ne, Te, Ti, Z, V, p ? &p->march : nullptr, n, origin, dir, n_freq, omega, e_ph, c_omega, backlight, I, tau, column, chord,
           steps, kernel_ms};
  SR_RC(check_family(F, [&] {  // wing is read only with LG
    SR_RC(check_voigt_table(who, lines));
    return lines->LG ? check_wing(who, p->wing) : SR_OK;
  }));
  if (lines->LG == nullptr)  // Gaussian lines: that entry's rule and its kernel
    return sr_field_sightline_lines(ne, Te, Ti, Z, V, &lines->lines, F.m, n, origin, dir, n_freq, omega, e_ph, c_omega, backlight, I, tau,
                                    column, chord, steps, kernel_ms);
  VoigtArgs X{};
  X.cut = p->wing * p->wing;
  const size_t lds = sizeof(double) * 2 * kVoigtChunk * (kHead + kVoigtWords * (size_t)lines->lines.n_line);  // at most 51 712 bytes
  return run_family<kVoigtArgs>(F, lines, nullptr, X, lds, [](auto f64, auto te, auto z, auto ti, auto v, auto narrow) {
    return &k_sightline_voigt<std::conditional_t<f64(), double, float>, te(), z(), ti(), v(), narrow() ? 64 : 256>;
  });
}
