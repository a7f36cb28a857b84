// Sightline spectra: many frequencies along each chord (sr_field_sightline_spectra; include/synthray.h states the rule by
// reference to sr_field_sightlines').  No reference counterpart.  k_sightlines puts a line on a lane and carries up to SR_MAX_BANDS
// bands; a spectrometer's 16 chords times 2048 frequencies are 16 lanes there, 512 calls long.  Here the parallelism is across
// FREQUENCY, with k_thomson's pattern: a workgroup owns one line and one tile of FL frequencies, a lane owns one frequency and
// keeps its (I, tau) in registers.
//
// The samples of the line go through LDS in chunks of FL, in march order.  Staging: lane l takes sample l of the chunk -- the cell
// search, the 8 corner reads per field and the blend (sightline_march.inc: the code k_sightlines runs), then the part of the node
// that no frequency changes (node_terms of nrl_node.inc: 7 numbers and a flag; table_terms of table_node.inc: the two searches,
// 4 numbers, the cell and a flag) and ne*h -- and writes them to LDS.  March: after one barrier every lane walks the staged
// samples in order, all lanes at the same LDS address (a broadcast), and does its own frequency's node_band / table_band and
// update.  The gather and the searches happen once per line and tile, not once per frequency; what a lane does per sample and
// frequency is the float64 log, exp and two expm1 of the rule, which bound the kernel.  Two staging buffers and one barrier per
// chunk: the corner reads of chunk c+1 are issued before the march of chunk c and blended after it, so they are in flight under
// that arithmetic; chunk c+1 is written to the buffer chunk c-1 was read from, which every lane left before the barrier of chunk c.
// Trip counts are uniform in a workgroup (one line has one n), a missed line leaves before the first barrier (uniformly), the
// last tile's idle lanes stage but neither march nor store, tile 0's lane 0 sums column in march order and writes the line's
// column, chord and steps.  No scratch, no atomics, no cross-lane operation but the barrier.
//
// FL = 256 or 64 (tiles of a single wavefront), whichever leaves fewer lanes of a line's last tile idle, 256 where they tie:
// idle lanes stage but do not march, and a 256-lane workgroup's four wavefronts and 34 KiB of LDS hold a CU's slots whether they
// march or not.  Measured on 128^2 lines (tools/sightline_spectra_rate.py, case c): full tiles of 256 are 5 % faster than four
// times as many of 64, which repeat the gather; at 64 to 128 frequencies tiles of 64 take 0.4 to 0.65 of the time, at 320 0.7.
// A table is packed group-innermost, LT | LD | LA[nT][nD][F] | LE[nT][nD][F]: the four corners a wavefront reads per sample and
// table are four contiguous runs.  The lattices (at most 2 x 512 float64) are staged in LDS for the searches, the opacities are
// read where they lie, through L2.  Instantiated per (dtype, Te field?, Z field?, node, FL).
// Compiled with -ffp-contract=off, as sightlines.hip: I[i][f] and tau[i][f] are the bits k_sightlines gives band f of line i.
// This unit holds the kernel, its dispatch, lane_width, the workgroup-count check and the group-innermost packing; what the entry does
// around them is sightline_march.inc's host section, shared with sightlines.hip, and emission_march.inc's (bands, EmArgs).
#include <cstdlib>
#include <vector>

#include "emission_march.inc"

namespace {
#include "table_node.inc"

#include "sightline_march.inc"

struct SpecArgs {
  const double *omega, *e_ph, *c_omega;  // (n_freq); omega is not read with a table
  int n_freq, n_tiles;
  const double *LT, *LD, *LA, *LE;       // the table where it lies: LT[nT], LD[nD], LA[nT][nD][n_freq], LE the same (has_le)
  int nT, nD, has_le;
  double m_ion;
};

template <typename T, bool HAS_TE, bool HAS_Z, bool TABLE, int FL>
__global__ void __launch_bounds__(FL) k_sightline_spectra(EmArgs A, LineArgs L, SpecArgs X) {
  constexpr int KV = TABLE ? 5 : 8;  // staged float64 per sample, ne*h last
  __shared__ double s_val[2][KV][FL];
  __shared__ int s_flag[2][FL];      // dark; with a table also the cell: (o << 1) | dark
  __shared__ double s_lat[TABLE ? 2 * kMaxLattice : 1];
  const int64_t i = blockIdx.x / (unsigned)X.n_tiles;
  const int tile = (int)(blockIdx.x % (unsigned)X.n_tiles);
  const int lane = (int)threadIdx.x;
  const int f = tile * FL + lane;
  const bool active = f < X.n_freq;
  const int64_t at = i * X.n_freq + f;
  const Line l = line_of(L, i);
  if (!l.hit) {  // the whole workgroup: one line
    if (active) {
      A.I[at] = A.back ? A.back[at] : 0.0;
      A.tau[at] = 0.0;
    }
    if (tile == 0 && lane == 0) {
      L.column[i] = 0.0;
      L.chord[i] = 0.0;
      L.steps[i] = 0;
    }
    return;
  }
  int sT = 0, sD = 0;
  if constexpr (TABLE) {
    for (int k = lane; k < X.nT; k += FL) s_lat[k] = X.LT[k];
    for (int k = lane; k < X.nD; k += FL) s_lat[kMaxLattice + k] = X.LD[k];
    sT = top_step(X.nT);
    sD = top_step(X.nD);
    __syncthreads();
  }
  const int n = l.n;
  const double h = l.h;
  const int64_t sy = L.f.n[2], sx = (int64_t)L.f.n[1] * sy;
  const int k0 = A.toward > 0 ? 0 : n - 1, dk = A.toward > 0 ? 1 : -1;
  // the frequency's constants; an idle lane of the last tile takes the last frequency's and stores nothing
  const int fc = active ? f : X.n_freq - 1;
  const double om = TABLE ? 0.0 : X.omega[fc], eph = X.e_ph[fc], com = X.c_omega[fc];
  const int64_t F = X.n_freq, st = (int64_t)X.nD * F;
  const bool has_le = X.has_le != 0;
  double I = (active && A.back) ? A.back[at] : 0.0;
  double tau = 0.0, column = 0.0;

  Sample<T, HAS_TE, HAS_Z> cur{};
  if (lane < n) fetch_sample<T, HAS_TE, HAS_Z>(A, L.f, sx, sy, l, k0 + lane * dk, cur);
  int buf = 0;
  for (int m0 = 0; m0 < n; m0 += FL, buf ^= 1) {
    const int cnt = min(FL, n - m0);
    // this chunk's samples (their reads were issued a chunk ago): blend, the node's shared part, to LDS
    if (lane < cnt) {
      double ne, Te, Z;
      blend_sample<T, HAS_TE, HAS_Z>(A, cur, ne, Te, Z);
      if constexpr (TABLE) {
        const TableTerms t = table_terms(s_lat, X.nT, sT, s_lat + kMaxLattice, X.nD, sD, X.m_ion, ne, Te, Z);
        s_val[buf][0][lane] = t.Te;
        s_val[buf][1][lane] = t.ft;
        s_val[buf][2][lane] = t.fd;
        s_val[buf][3][lane] = t.rho;
        s_flag[buf][lane] = (t.o << 1) | (t.dark ? 1 : 0);
      } else {
        const NodeTerms t = node_terms(ne, Te, Z);
        s_val[buf][0][lane] = t.Te;
        s_val[buf][1][lane] = t.n;
        s_val[buf][2][lane] = t.wp;
        s_val[buf][3][lane] = t.L;
        s_val[buf][4][lane] = t.num;
        s_val[buf][5][lane] = t.zc;
        s_val[buf][6][lane] = t.it;
        s_flag[buf][lane] = t.dark ? 1 : 0;
      }
      s_val[buf][KV - 1][lane] = ne * h;
    }
    __syncthreads();
    // the next chunk's cells and corner reads, in flight during this chunk's march
    cur.in = false;
    if (m0 + FL + lane < n) fetch_sample<T, HAS_TE, HAS_Z>(A, L.f, sx, sy, l, k0 + (m0 + FL + lane) * dk, cur);
    if (active) {
      for (int j = 0; j < cnt; ++j) {
        const int flag = s_flag[buf][j];
        double al, S;
        if constexpr (TABLE) {
          TableTerms t;
          t.dark = (flag & 1) != 0;
          t.o = flag >> 1;
          t.Te = s_val[buf][0][j];
          t.ft = s_val[buf][1][j];
          t.fd = s_val[buf][2][j];
          t.rho = s_val[buf][3][j];
          const int64_t o = (int64_t)t.o * F + f;
          const double la = bilinear(X.LA, o, F, st, t.ft, t.fd);
          const double le = has_le ? bilinear(X.LE, o, F, st, t.ft, t.fd) : 0.0;
          table_band(t, la, le, has_le, eph, com, al, S);
        } else {
          NodeTerms t;
          t.dark = flag != 0;
          t.Te = s_val[buf][0][j];
          t.n = s_val[buf][1][j];
          t.wp = s_val[buf][2][j];
          t.L = s_val[buf][3][j];
          t.num = s_val[buf][4][j];
          t.zc = s_val[buf][5][j];
          t.it = s_val[buf][6][j];
          node_band(t, om, eph, com, al, S);
        }
        const double dtau = al * h;
        I = I * exp(-dtau) + S * (-expm1(-dtau));
        tau = tau + dtau;
        column = column + s_val[buf][KV - 1][j];
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

extern "C" int sr_field_sightline_spectra(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_table *table,
                                          const sr_spectra_params *p, int64_t n, const double *origin, const double *dir,
                                          int32_t n_freq, const double *omega, const double *e_ph, const double *c_omega,
                                          const double *backlight, double *I, double *tau, double *column, double *chord,
                                          int32_t *steps, double *kernel_ms) {
  const char *who = "sr_field_sightline_spectra";
  SR_CHECK(p != nullptr && origin != nullptr && dir != nullptr && I != nullptr && tau != nullptr, "%s: NULL argument", who);
  SR_CHECK(e_ph != nullptr && c_omega != nullptr, "%s: NULL e_ph or c_omega", who);
  SR_CHECK(table != nullptr || omega != nullptr, "%s: NULL omega without a table", who);
  SR_CHECK(n >= 0, "%s: n must not be negative, got %lld", who, (long long)n);
  SR_RC(check_bands(who, "frequency", n_freq, SR_MAX_FREQS, table ? nullptr : omega, e_ph, c_omega));
  SR_RC(check_march(who, p->toward, p->step, p->max_steps));
  size_t tab_words = 0;
  if (table) {
    if (table->nT >= 2 && table->nT <= kMaxLattice && table->nD >= 2 && table->nD <= kMaxLattice) {  // before any entry is read
      tab_words = (size_t)table->nT + table->nD + (size_t)table->nT * table->nD * n_freq * (table->LE ? 2 : 1);
      SR_CHECK(tab_words <= (size_t)2147483647, "%s: the packed table holds %zu values, more than 2^31 - 1", who, tab_words);
    }
    SR_RC(check_table(who, table, n_freq));
  }
  const int fl = lane_width(n_freq);
  const int64_t n_tiles = (n_freq + fl - 1) / fl;
  SR_CHECK(n <= (int64_t)2147483647 / n_tiles, "%s: n x frequency tiles exceeds 2^31 - 1 workgroups", who);
  SR_RC(check_lines(who, n, origin, dir, ne, Te, Z));
  if (kernel_ms) *kernel_ms = 0.0;
  if (n == 0) return SR_OK;
  SR_RC(sr::ensure_init());
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;

  // the table group-innermost: LT | LD | LA[nT][nD][F] | LE[nT][nD][F]
  std::vector<double> pack;
  if (table) {
    const size_t cells = (size_t)table->nT * table->nD, nf = (size_t)n_freq;
    pack.resize(tab_words);
    double *q = pack.data();
    q = std::copy(table->LT, table->LT + table->nT, q);
    q = std::copy(table->LD, table->LD + table->nD, q);
    for (const double *src : {table->LA, table->LE}) {
      if (!src) continue;
      for (size_t b = 0; b < nf; ++b)
        for (size_t k = 0; k < cells; ++k) q[k * nf + b] = src[b * cells + k];
      q += cells * nf;
    }
  }
  const size_t nf = (size_t)n_freq, map_bytes = sizeof(double) * nf * (size_t)n, freq_bytes = sizeof(double) * nf;

  // one scratch block: the lines' pieces (take_lines) | omega | e_ph | c_omega | table
  EmArgs A{};
  LineArgs L{};
  SpecArgs X{};
  double *tab = nullptr;
  sr::Carve carve;
  take_lines(carve, A, L, ne, n, p->step, p->max_steps, nf, backlight != nullptr);
  if (!table) carve.take(&X.omega, nf);
  carve.take(&X.e_ph, nf);
  carve.take(&X.c_omega, nf);
  carve.take(&tab, tab_words);
  if (!carve.alloc()) return SR_ERR_HIP;
  fill_fields(A, ne, Te, Z, p->toward, p->Te, p->Z, 0, nullptr, nullptr, nullptr);  // the frequencies' constants are X's
  X.n_freq = n_freq;
  X.n_tiles = (int)n_tiles;
  if (table) {
    const size_t entries = (size_t)table->nT * table->nD * nf;
    X.LT = tab;
    X.LD = X.LT + table->nT;
    X.LA = X.LD + table->nD;
    X.LE = X.LA + entries;
    X.nT = table->nT;
    X.nD = table->nD;
    X.has_le = table->LE != nullptr;
    X.m_ion = table->m_ion;
  }

  SR_RC(upload_lines(A, L, origin, dir, backlight, map_bytes, st));
  if (!table) SR_HIP(hipMemcpyAsync(const_cast<double *>(X.omega), omega, freq_bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(X.e_ph), e_ph, freq_bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(X.c_omega), c_omega, freq_bytes, hipMemcpyHostToDevice, st));
  if (table) SR_HIP(hipMemcpyAsync(tab, pack.data(), sizeof(double) * tab_words, hipMemcpyHostToDevice, st));
  SR_HIP(hipEventRecord(c.ev[0], st));
  const unsigned grid = (unsigned)(n * n_tiles);
  sr::with_flags(
      [&](auto f64, auto te, auto z, auto tb, auto narrow) {
        using T = std::conditional_t<decltype(f64)::value, double, float>;
        constexpr int kFl = decltype(narrow)::value ? 64 : 256;
        hipLaunchKernelGGL((k_sightline_spectra<T, decltype(te)::value, decltype(z)::value, decltype(tb)::value, kFl>), dim3(grid),
                           dim3(kFl), 0, st, A, L, X);
      },
      (bool)ne->is_f64, Te != nullptr, Z != nullptr, table != nullptr, fl == 64);
  return finish_lines(A, L, map_bytes, I, tau, column, chord, steps, kernel_ms);
}
