// Line spectra along sightlines: Doppler-shifted, thermally broadened spectral lines, optionally on the NRL continuum
// (sr_field_sightline_lines; include/synthray.h states the rule).  No reference counterpart.  The decomposition is the family's
// (line_family.inc: a workgroup per chord and tile of FL frequencies, a lane per frequency, the samples through LDS in chunks of
// kLinesChunk in two buffers); what is this kernel's own:
//
// Staging: lane s < kLinesChunk takes sample s of the chunk -- the cell search and the 8 corner reads of ne, Te, Z, Ti and the three
// components of V (sightline_march.inc's FlowSample), the blend, line_family.inc's stage_head, and then per line its centre, inverse
// width, peak emission and peak absorption (line_node.inc's line_const: two bilinear reads and two exp a line) -- and writes them
// to LDS, a sample's lines one after the other, the four constants of a line adjacent (two 16-byte reads; every marching lane
// reads the same address, a broadcast).  A sample is 10 + 4*n_line float64: at 32 lines 1104 bytes, and the two buffers of 24
// samples 52 KiB -- with the 8 KiB of the lattices under the 64 KiB a workgroup may take without asking, two workgroups to a CU's
// 160 KiB; the LDS is sized by n_line at launch, so a single line takes 5 KiB.
// March: after one barrier every active lane walks the staged samples in order and the lines of a sample in ascending order.  A
// term with x*x > 40 is dropped, which is exact, so a WAVEFRONT skips a line whose window holds none of its frequencies
// (line_outside on the least and the greatest frequency of the wavefront, found once with six shuffles each): lanes hold consecutive
// list entries, so a sorted list makes most of a narrow line's tests one comparison per wavefront.  The skip changes no bit: it
// only leaves out terms every lane would have dropped.  What a lane does per counted term is one exp and five multiply-adds worth
// of float64; per sample with a counted term an exp, an expm1 and a division, and with the continuum node_band's log and expm1.
// No scratch (the line loop runs over LDS, never over a register array), no atomics.
// The line table is packed line-innermost, LT | LD | w0 | ci | LJ[nT][nD][n_line] | LK[nT][nD][n_line]: what a staging lane reads
// for the lines of its sample are four contiguous runs per table.  The lattices are staged in LDS for the searches.
// Instantiated per (dtype, Te field?, Z field?, Ti field?, V field?, FL); continuum and LK are uniform branches.
// Compiled with -ffp-contract=off, as its siblings: column, chord and steps are the bits k_sightlines gives, and where every term
// is dropped I and tau are the bits of k_sightline_spectra.
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

constexpr int kLinesChunk = 24;  // samples staged at a time (sr_lines_chunk)
constexpr int kHead = 10;        // float64 of a staged sample before its lines: the family's head

struct LinesArgs {
  const double *omega, *e_ph, *c_omega;  // (n_freq)
  int n_freq, n_tiles;
  const double *LT, *LD, *w0, *ci, *LJ, *LK;  // the packed table where it lies
  int nT, nD, n_line, has_lk, continuum;
};

template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI, bool HAS_V, int FL>
__global__ void __launch_bounds__(FL) k_sightline_lines(EmArgs A, LineArgs L, FlowArgs W, LinesArgs X) {
  extern __shared__ double s_stage[];  // [2][kLinesChunk][kHead + 4*n_line]
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
  const int stride = kHead + kLineWords * NL;
  const double h = l.h;
  const int64_t sy = L.f.n[2], sx = (int64_t)L.f.n[1] * sy;
  const int k0 = A.toward > 0 ? 0 : n - 1, dk = A.toward > 0 ? 1 : -1;
  const double su = (double)A.toward / sqrt((l.d0 * l.d0 + l.d1 * l.d1) + l.d2 * l.d2);  // len of line_of, the same bits
  const bool cont = X.continuum != 0, has_lk = X.has_lk != 0;
  const LaneFreq w = lane_freq(X, f, active);
  double I = (active && A.back) ? A.back[at] : 0.0;
  double tau = 0.0, column = 0.0;

  FlowSample<T, HAS_TE, HAS_Z, HAS_TI, HAS_V> cur{};
  if (lane < kLinesChunk && lane < n) fetch_sample<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, W, L.f, sx, sy, l, k0 + lane * dk, cur);
  int buf = 0;
  for (int m0 = 0; m0 < n; m0 += kLinesChunk, buf ^= 1) {
    const int cnt = min(kLinesChunk, n - m0);
    // this chunk's samples (their reads were issued a chunk ago): blend, the lattice search, the lines' constants, to LDS
    if (lane < cnt) {
      double ne, Te, Z, Ti, V[3];
      blend_sample<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, cur, ne, Te, Z, Ti, V);
      const TableTerms t = table_terms(s_lat, X.nT, sT, s_lat + kMaxLattice, X.nD, sD, 1.0, ne, Te, Z);
      const bool dark = t.dark || Ti <= 0.0;  // outside the box ne = 0: dark
      double beta = 0.0;
      if (HAS_V) beta = ((((V[0] * l.d0 + V[1] * l.d1) + V[2] * l.d2)) * su) / sr::kC;
      double *S = s_stage + (size_t)(buf * kLinesChunk + lane) * stride;
      stage_head(S, cont, dark, ne, Te, Z, h);
      if (!dark) {
        const int o = t.o * NL, st = X.nD * NL;
#pragma unroll 1
        for (int q = 0; q < NL; ++q) {
          const LineConst k = line_const(X.w0[q], X.ci[q], X.LJ, X.LK, has_lk, o + q, NL, st, t.ft, t.fd, beta, Ti);
          double *P = S + kHead + kLineWords * q;
          P[0] = k.wc, P[1] = k.iw, P[2] = k.aJ, P[3] = k.aK;
        }
      }
    }
    __syncthreads();
    // the next chunk's cells and corner reads, in flight during this chunk's march
    cur.s.in = false;
    if (lane < kLinesChunk && m0 + kLinesChunk + lane < n)
      fetch_sample<T, HAS_TE, HAS_Z, HAS_TI, HAS_V>(A, W, L.f, sx, sy, l, k0 + (m0 + kLinesChunk + lane) * dk, cur);
    if (active) {
#pragma unroll 1
      for (int s = 0; s < cnt; ++s) {
        const double *S = s_stage + (size_t)(buf * kLinesChunk + s) * stride;
        const int flags = (int)S[1];
        double j = 0.0, aL = 0.0;
        bool counted = false;
        if (!(flags & 2)) {
#pragma unroll 1
          for (int q = 0; q < NL; ++q) {
            const double *P = S + kHead + kLineWords * q;
            const double wc = P[0], iw = P[1];
            if (line_outside(wc, iw, w.wmin, w.wmax)) continue;  // the same for every lane of the wavefront
            double x2;
            if (line_term(w.om, wc, iw, x2)) {
              const double phi = exp(-x2);
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

extern "C" int sr_lines_chunk(void) { return kLinesChunk; }

extern "C" int sr_field_sightline_lines(const sr_field *ne, const sr_field *Te, const sr_field *Ti, const sr_field *Z, const sr_field *V,
                                        const sr_line_table *lines, const sr_lines_params *p, int64_t n, const double *origin,
                                        const double *dir, int32_t n_freq, const double *omega, const double *e_ph,
                                        const double *c_omega, const double *backlight, double *I, double *tau, double *column,
                                        double *chord, int32_t *steps, double *kernel_ms) {
  const char *who = "sr_field_sightline_lines";
  Family F{who, ne, Te, Ti, Z, V, p, n, origin, dir, n_freq, omega, e_ph, c_omega, backlight, I, tau, column, chord, steps, kernel_ms};
  SR_RC(check_family(F, [&] { return check_line_table(who, lines); }));
  const sr_voigt_table t{*lines, nullptr};
  LinesArgs X{};
  const size_t lds = sizeof(double) * 2 * kLinesChunk * (kHead + kLineWords * (size_t)lines->n_line);  // at most 52 992 bytes
  return run_family<kLinesArgs>(F, &t, nullptr, X, lds, [](auto f64, auto te, auto z, auto ti, auto v, auto narrow) {
    return &k_sightline_lines<std::conditional_t<f64(), double, float>, te(), z(), ti(), v(), narrow() ? 64 : 256>;
  });
}
