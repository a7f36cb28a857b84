// The step before the path: volume synthesis (gaussian3D.domain_fft, src/field_generator/gaussian3D.py:215-271; the cosine
// mode sum of gaussian{1,2,3}D.cos, sr_field_modesum at the end of this file).
// The reference shapes complex Gaussian noise with sqrt(S(k)) and takes np.fft.ifftn(...).real / max|.| on the host
// (15 s of the 25 s a 512^3 volume takes there).  Here the noise and the float32 amplitude sqrt(S) arrive from the
// host (the noise must come from the caller's seeded np.random stream to reproduce the reference's field), the
// product, the 3-D inverse FFT (hipFFT Z2Z, bound at first use like RCCL) and the normalisation run on the GPU.
#include <dlfcn.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "common.hpp"
#include "fft.hpp"

namespace sr {

int fft_lib(Fft **out) {
  static Fft F;
  if (!F.h) {
    const char *names[] = {"libhipfft.so", "libhipfft.so.0", "/opt/rocm/lib/libhipfft.so"};
    for (const char *n : names) {
      F.h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
      if (F.h) break;
    }
    if (!F.h) return sr::fail(SR_ERR_HIP, "cannot load libhipfft.so: %s", dlerror());
#define SR_SYM(field, name)                                                   \
  F.field = reinterpret_cast<decltype(F.field)>(dlsym(F.h, name));            \
  if (!F.field) return sr::fail(SR_ERR_HIP, "libhipfft.so lacks symbol %s", name);
    SR_SYM(Plan3d, "hipfftPlan3d")
    SR_SYM(Plan2d, "hipfftPlan2d")
    SR_SYM(Plan1d, "hipfftPlan1d")
    SR_SYM(SetStream, "hipfftSetStream")
    SR_SYM(ExecZ2Z, "hipfftExecZ2Z")
    SR_SYM(Destroy, "hipfftDestroy")
#undef SR_SYM
  }
  *out = &F;
  return SR_OK;
}

// Plans are kept for the life of the process: creating one costs 1-2 s (rocFFT builds its kernels at run time), using
// it milliseconds.  Key: (rank, n0, n1, n2), the sizes past the rank 0.
int fft_plan(Fft *F, int rank, int n0, int n1, int n2, hipfftHandle *out) {
  static std::map<std::tuple<int, int, int, int>, hipfftHandle> cache;
  const auto key = std::make_tuple(rank, n0, rank > 1 ? n1 : 0, rank > 2 ? n2 : 0);
  auto it = cache.find(key);
  if (it == cache.end()) {
    hipfftHandle plan = nullptr;
    char who[64];
    snprintf(who, sizeof who, "fft_plan(%d: %d, %d, %d)", rank, n0, n1, n2);
    SR_FFT(who, rank == 3 ? F->Plan3d(&plan, n0, n1, n2, HIPFFT_Z2Z) : rank == 2 ? F->Plan2d(&plan, n0, n1, HIPFFT_Z2Z) : F->Plan1d(&plan, n0, HIPFFT_Z2Z, 1));
    it = cache.emplace(key, plan).first;
  }
  *out = it->second;
  return SR_OK;
}

}  // namespace sr

namespace {

using sr::Fft;
using sr::fft_lib;
using sr::fft_plan;

// fft_field = noise * sqrt(S): complex128 times float32 promoted to float64, as numpy does
__global__ void k_shape_noise(double2 *__restrict__ w, const float *__restrict__ amp, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double a = (double)amp[i];
    double2 v = w[i];
    v.x *= a;
    v.y *= a;
    w[i] = v;
  }
}

// field = Re(ifft) = Re(unnormalised backward transform) * (1/N); max |field| by one atomic per wavefront
__global__ void k_real_scaled(const double2 *__restrict__ w, int64_t n, double inv_n, double *__restrict__ out,
                              unsigned long long *__restrict__ vmax_bits) {
  double m = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = w[i].x * inv_n;
    out[i] = v;
    const double a = fabs(v);
    m = a > m ? a : m;  // NaN never wins: an all-NaN field keeps 0
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(m, off, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(vmax_bits, (unsigned long long)__double_as_longlong(m));  // non-negative doubles order as integers
}

__global__ void k_divide(double *__restrict__ f, int64_t n, const unsigned long long *__restrict__ vmax_bits) {
  const double m = __longlong_as_double((long long)*vmax_bits);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) f[i] = f[i] / m;
}

__global__ void k_to_complex(const double *__restrict__ r, int64_t n, double2 *__restrict__ w) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) w[i] = make_double2(r[i], 0.0);
}

// The power spectrum's one binning pass (power_spectrum.py: radial_*Dspectrum, scalar*D_fft, scalar*D_knyquist).
// Mode (i, j, l) of an (n0, n1, n2) transform (C order, n2 fastest; n1 = n2 = 1 in 1-D) has the magnitude
// m = sqrt((a0[i]^2 + a1[j]^2) + a2[l]^2), grouped as numpy's (KX**2 + KY**2) + KZ**2 and, the library being built with
// -ffp-contract=off, rounded as numpy rounds it (sqrt is correctly rounded): bin membership is numpy's, bit for bit.
// A NaN coordinate drops the mode.  p = (re^2 + im^2) / norm is summed and counted per bin:
//   SR_SPECTRUM_EDGES: bin b holds edges[b] <= m < edges[b+1] (binary search over the n_bins+1 ascending edges);
//   SR_SPECTRUM_SHELL: bin rint(m) (the reference's int(np.round(rk))); a shell >= n_bins is counted in *over.
// Bins go to per-workgroup copies in LDS when they fit (lds != 0), else straight to the global atomics.
constexpr int kMaxLdsBins = 2048;  // 32 KiB of sums and counts per workgroup

template <int RULE>
__global__ void k_spectrum_bins(const double2 *__restrict__ F, int64_t n, int64_t n1, int64_t n2,
                                const double *__restrict__ a0, const double *__restrict__ a1,
                                const double *__restrict__ a2, const double *__restrict__ edges, int n_bins,
                                double norm, int lds, double *__restrict__ sum, unsigned long long *__restrict__ cnt,
                                unsigned long long *__restrict__ over) {
  extern __shared__ double lds_bins[];  // [n_bins] sums, then [n_bins] counts
  double *lsum = lds_bins;
  unsigned long long *lcnt = reinterpret_cast<unsigned long long *>(lds_bins + (lds ? n_bins : 0));
  if (lds)
    for (int t = threadIdx.x; t < n_bins; t += blockDim.x) {
      lsum[t] = 0.0;
      lcnt[t] = 0ull;
    }
  __syncthreads();
  unsigned long long n_over = 0;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = q % n2, r = q / n2;
    const int64_t j = r % n1, i = r / n1;
    const double x = a0[i], y = a1[j], z = a2[l];
    const double m = sqrt((x * x + y * y) + z * z);
    int b;
    if (RULE == SR_SPECTRUM_EDGES) {
      if (!(m >= edges[0] && m < edges[n_bins])) continue;  // NaN fails both
      int lo = 0, hi = n_bins;  // edges[lo] <= m < edges[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (m < edges[mid])
          hi = mid;
        else
          lo = mid;
      }
      b = lo;
    } else {
      if (m != m) continue;
      const double s = rint(m);  // round half to even, as np.round; m is the sqrt of an integer, so never a tie
      if (s >= (double)n_bins) {
        ++n_over;
        continue;
      }
      b = (int)s;
    }
    const double2 v = F[q];
    const double p = (v.x * v.x + v.y * v.y) / norm;
    if (lds) {
      atomicAdd(&lsum[b], p);
      atomicAdd(&lcnt[b], 1ull);
    } else {
      atomicAdd(&sum[b], p);
      atomicAdd(&cnt[b], 1ull);
    }
  }
  if (RULE == SR_SPECTRUM_SHELL && n_over) atomicAdd(over, n_over);  // an error case: rare, one add per thread at most
  __syncthreads();
  if (lds)
    for (int t = threadIdx.x; t < n_bins; t += blockDim.x)
      if (lcnt[t]) {
        atomicAdd(&sum[t], lsum[t]);
        atomicAdd(&cnt[t], lcnt[t]);
      }
}

// One transform + one binning pass; axis[d] (n[d] values, host) are the coordinates of the unshifted indices of axis d.
int spectrum_nd(const char *who, const double *field, int ndim, const int64_t n[3], const double *const axis[3], int rule,
                const double *edges, int n_bins, double norm, double *sum, uint64_t *count, uint64_t *over) {
  int rc = sr::ensure_init();
  if (rc) return rc;
  Fft *F;
  if ((rc = fft_lib(&F))) return rc;
  hipStream_t st = sr::ctx().stream;
  const int64_t nn = n[0] * n[1] * n[2];
  const int64_t n_axes = n[0] + n[1] + n[2];
  const int n_edges = rule == SR_SPECTRUM_EDGES ? n_bins + 1 : 0;
  sr::CallBuffers buf;
  double *d_r = nullptr, *d_k = nullptr, *d_sum = nullptr;
  double2 *d_w = nullptr;
  unsigned long long *d_cnt = nullptr;
  hipfftHandle plan = nullptr;
  // d_k: the axes' coordinates, then the edges; d_cnt: n_bins counts, then the overflow count
  SR_RC(buf.alloc(&d_r, (size_t)nn));
  SR_RC(buf.alloc(&d_w, (size_t)nn));
  SR_RC(buf.alloc(&d_k, (size_t)(n_axes + n_edges)));
  SR_RC(buf.alloc(&d_sum, (size_t)n_bins));
  SR_RC(buf.alloc(&d_cnt, (size_t)n_bins + 1));
  SR_HIP(hipMemcpyAsync(d_r, field, sizeof(double) * nn, hipMemcpyHostToDevice, st));
  for (int d = 0; d < 3; ++d)
    SR_HIP(hipMemcpyAsync(d_k + (d > 0 ? n[0] : 0) + (d > 1 ? n[1] : 0), axis[d], sizeof(double) * n[d], hipMemcpyHostToDevice, st));
  if (n_edges) SR_HIP(hipMemcpyAsync(d_k + n_axes, edges, sizeof(double) * n_edges, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemsetAsync(d_sum, 0, sizeof(double) * n_bins, st));
  SR_HIP(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * (n_bins + 1), st));
  const int block = 256;
  hipLaunchKernelGGL(k_to_complex, dim3(sr::capped_grid((nn + block - 1) / block, 32)), dim3(block), 0, st, (const double *)d_r, nn, d_w);
  SR_RC(fft_plan(F, ndim, (int)n[0], (int)n[1], (int)n[2], &plan));
  SR_FFT(who, F->SetStream(plan, st));
  SR_FFT(who, F->ExecZ2Z(plan, d_w, d_w, HIPFFT_FORWARD));
  const int lds = n_bins <= kMaxLdsBins;
  const size_t lds_bytes = lds ? (sizeof(double) + sizeof(unsigned long long)) * (size_t)n_bins : 0;
  const unsigned bgrid = sr::capped_grid((nn + block - 1) / block, 8);
  const double *k0 = d_k, *k1 = d_k + n[0], *k2 = d_k + n[0] + n[1];
  if (rule == SR_SPECTRUM_EDGES)
    hipLaunchKernelGGL(k_spectrum_bins<SR_SPECTRUM_EDGES>, dim3(bgrid), dim3(block), lds_bytes, st, (const double2 *)d_w, nn,
                       n[1], n[2], k0, k1, k2, (const double *)(d_k + n_axes), n_bins, norm, lds, d_sum, d_cnt,
                       d_cnt + n_bins);
  else
    hipLaunchKernelGGL(k_spectrum_bins<SR_SPECTRUM_SHELL>, dim3(bgrid), dim3(block), lds_bytes, st, (const double2 *)d_w, nn,
                       n[1], n[2], k0, k1, k2, (const double *)nullptr, n_bins, norm, lds, d_sum, d_cnt, d_cnt + n_bins);
  uint64_t n_over = 0;
  SR_RC(sr::stage_out(st, {{sum, d_sum, sizeof(double) * n_bins}, {count, d_cnt, sizeof(uint64_t) * n_bins}, {&n_over, d_cnt + n_bins, sizeof(uint64_t)}}));
  if (over) *over = n_over;
  return SR_OK;
}

// ---- gaussian{1,2,3}D.cos (src/field_generator/gaussian{1,2,3}D.py): the cosine mode sum -------------------------------
// The reference evaluates amp_m * cos(kx x + ky y + kz z + psi_s) for every cell, mode and term: ~4 float64 cosines per
// point-mode.  Here the cosines are factored into phasors per axis.  On the kernel's axes (a0, a1, a2) = (i, j, l), l
// fastest in `out`, with X[i,m] = amp_m e^{i k0 x0_i}, Y[j,m] = e^{i k1 x1_j}, Z[l,m] = e^{i k2 x2_l}, P_s = e^{i psi_s}:
//   Zp = Z P1 + conj(Z) P2,  Zm = Z P3 + conj(Z) P4,  S = Zp + Zm,  D = Zp - Zm
//   G = Y Zp + conj(Y) Zm:   G.re = Y.re S.re - Y.im D.im,   G.im = Y.re S.im + Y.im D.re
//   out[i,j,l] = sum_m Re(X G) = sum_m X.re G.re - X.im G.im
// which is the reference's sum of the four terms (++ P1, +- P2, -+ P3, -- P4).  A problem of fewer axes keeps its last axis
// on a2 (the lanes) and gives the missing ones one cell at coordinate 0 with k = 0 (e^{i0} = 1 exactly):
//   3-D (x, y, z): P1..P4 = psi_1..psi_4;   2-D (x, -, y): P1 = phi (+ky), P2 = psi (-ky);   1-D (-, -, x): P1 = phi;
// an absent P_s is 0.  float64 throughout (arguments reach ~pi n rad).
//
// k_modesum_tables: the per-axis tables, mode-major ([m][index]) so that a wave's per-lane S, D loads are coalesced and a
// tile's rows of X and Y are consecutive.  X and Y are padded to p0 >= n0 and p1 >= n1 rows (whole tiles; a padding row
// repeats the last cell, and what it adds is never stored), so the main kernel reads them without clamping.  One float64
// sincos per table value: (p0 + p1 + n2) M of them.
__global__ void k_modesum_tables(const double *__restrict__ c, const double *__restrict__ k, const double *__restrict__ amp,
                                 const double *__restrict__ ph, int pmask, int M, int64_t n0, int64_t n1, int64_t n2,
                                 int64_t p0, int64_t p1, double2 *__restrict__ X, double2 *__restrict__ Y,
                                 double2 *__restrict__ S, double2 *__restrict__ D) {
  const int64_t nx = p0 * M, ny = p1 * M, n = (p0 + p1 + n2) * M;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    double sn, cs;
    if (q < nx) {
      const int64_t m = q / p0, i = q - m * p0;
      sincos(k[m] * c[i < n0 ? i : n0 - 1], &sn, &cs);
      X[q] = make_double2(amp[m] * cs, amp[m] * sn);
    } else if (q < nx + ny) {
      const int64_t r = q - nx, m = r / p1, j = r - m * p1;
      sincos(k[M + m] * c[n0 + (j < n1 ? j : n1 - 1)], &sn, &cs);
      Y[r] = make_double2(cs, sn);
    } else {
      const int64_t r = q - nx - ny, m = r / n2, l = r - m * n2;
      sincos(k[2 * M + m] * c[n0 + n1 + l], &sn, &cs);
      double2 p[4];
      for (int s = 0; s < 4; ++s) {
        p[s] = make_double2(0.0, 0.0);
        if (pmask >> s & 1) sincos(ph[s * M + m], &p[s].y, &p[s].x);
      }
      // Z P = (cs + i sn) P,  conj(Z) P = (cs - i sn) P
      const double zp_re = (cs * p[0].x - sn * p[0].y) + (cs * p[1].x + sn * p[1].y);
      const double zp_im = (cs * p[0].y + sn * p[0].x) + (cs * p[1].y - sn * p[1].x);
      const double zm_re = (cs * p[2].x - sn * p[2].y) + (cs * p[3].x + sn * p[3].y);
      const double zm_im = (cs * p[2].y + sn * p[2].x) + (cs * p[3].y - sn * p[3].x);
      S[r] = make_double2(zp_re + zm_re, zp_im + zm_im);
      D[r] = make_double2(zp_re - zm_re, zp_im - zm_im);
    }
  }
}

// k_modesum: a wave owns a tile of T rows i x JT rows j x 64 lanes l.  Per mode it loads S, D for its lane (coalesced, one
// mode ahead), the tile's T values of X and JT of Y (wave-uniform: scalar loads), forms G once per (j, l) in registers and
// adds it into T x JT accumulators: 4 JT + 2 T JT float64 FMA-class operations per mode for T JT points.  Modes are summed
// in order, one accumulator per point, no atomics: a repeated call returns the identical field.  A lane past n2 reads the
// last column and stores nothing; rows past n0, n1 are the tables' padding and are not stored.
constexpr int kModesumBlock = 256;  // 4 waves, each its own tile

template <int T, int JT>
__global__ __launch_bounds__(kModesumBlock) void k_modesum(const double2 *__restrict__ X, const double2 *__restrict__ Y,
                                                           const double2 *__restrict__ S, const double2 *__restrict__ D,
                                                           int M, int64_t n0, int64_t n1, int64_t n2, int64_t p0, int64_t p1,
                                                           int64_t tiles_l, int64_t n_tiles, double *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = kModesumBlock / 64;
  const int64_t wave = (int64_t)blockIdx.x * waves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t tiles_j = p1 / JT;
  for (int64_t w = wave; w < n_tiles; w += (int64_t)gridDim.x * waves) {
    const int64_t r = w / tiles_l;
    const int64_t l = (w - r * tiles_l) * 64 + lane, j0 = (r % tiles_j) * JT, i0 = (r / tiles_j) * T;
    const int64_t lc = l < n2 ? l : n2 - 1;
    double acc[T][JT];
    for (int t = 0; t < T; ++t)
      for (int u = 0; u < JT; ++u) acc[t][u] = 0.0;
    const double2 *xs = X + i0, *ys = Y + j0, *ss = S + lc, *ds = D + lc;
    double2 s_next = *ss, d_next = *ds;
    for (int m = 0; m < M; ++m) {
      const double2 s = s_next, d = d_next;
      if (m + 1 < M) {  // the next mode's S, D in flight during this mode's arithmetic
        ss += n2;
        ds += n2;
        s_next = *ss;
        d_next = *ds;
      }
      double gr[JT], gi[JT];
#pragma unroll
      for (int u = 0; u < JT; ++u) {
        const double2 y = ys[u];
        gr[u] = fma(-y.y, d.y, y.x * s.x);
        gi[u] = fma(y.y, d.x, y.x * s.y);
      }
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const double2 x = xs[t];
#pragma unroll
        for (int u = 0; u < JT; ++u) acc[t][u] = fma(-x.y, gi[u], fma(x.x, gr[u], acc[t][u]));
      }
      xs += p0;
      ys += p1;
    }
    if (l < n2)
      for (int t = 0; t < T; ++t)
        for (int u = 0; u < JT; ++u)
          if (i0 + t < n0 && j0 + u < n1) out[((i0 + t) * n1 + (j0 + u)) * n2 + l] = acc[t][u];
  }
}

// The tables for a T x JT tile (padded rows p0, p1), then the sum.
template <int T, int JT>
void run_modesum(const double *d_in, int pmask, int M, const int64_t n[3], double2 *d_tab, double *out, hipStream_t st) {
  const int64_t p0 = (n[0] + T - 1) / T * T, p1 = (n[1] + JT - 1) / JT * JT, n_axes = n[0] + n[1] + n[2];
  double2 *X = d_tab, *Y = X + p0 * M, *S = Y + p1 * M, *D = S + n[2] * M;
  const int block = 256;
  const int64_t n_tab = (p0 + p1 + n[2]) * M;
  const unsigned tgrid = sr::capped_grid((n_tab + block - 1) / block, 32);
  hipLaunchKernelGGL(k_modesum_tables, dim3(tgrid), dim3(block), 0, st, d_in, d_in + n_axes, d_in + n_axes + 3 * M,
                     d_in + n_axes + 4 * M, pmask, M, n[0], n[1], n[2], p0, p1, X, Y, S, D);
  const int64_t tiles_l = (n[2] + 63) / 64, n_tiles = tiles_l * (p1 / JT) * (p0 / T);
  const int64_t waves = kModesumBlock / 64;
  const unsigned grid = sr::capped_grid((n_tiles + waves - 1) / waves, 64);
  hipLaunchKernelGGL((k_modesum<T, JT>), dim3(grid), dim3(kModesumBlock), 0, st, (const double2 *)X, (const double2 *)Y,
                     (const double2 *)S, (const double2 *)D, M, n[0], n[1], n[2], p0, p1, tiles_l, n_tiles, out);
}

// table entries of a T x JT tile
template <int T, int JT>
size_t modesum_table_len(int64_t M, const int64_t n[3]) {
  return (size_t)(((n[0] + T - 1) / T * T + (n[1] + JT - 1) / JT * JT + 2 * n[2]) * M);
}

}  // namespace

extern "C" int sr_power_spectrum(const double *field, int ndim, const int64_t *shape, const double *coords, int rule,
                                 const double *edges, int n_bins, double norm, double *sum, uint64_t *count,
                                 uint64_t *overflow) {
  SR_CHECK(field && shape && coords && sum && count, "sr_power_spectrum: NULL argument");
  SR_CHECK(ndim >= 1 && ndim <= 3, "sr_power_spectrum: ndim %d (1, 2 or 3)", ndim);
  SR_CHECK(rule == SR_SPECTRUM_EDGES || rule == SR_SPECTRUM_SHELL, "sr_power_spectrum: unknown rule %d", rule);
  SR_CHECK(rule == SR_SPECTRUM_SHELL || edges, "sr_power_spectrum: the edges rule needs edges");
  SR_CHECK(n_bins >= 1, "sr_power_spectrum: n_bins %d", n_bins);
  static const double zero = 0.0;  // the coordinate of the one index of an axis past ndim
  int64_t n[3] = {1, 1, 1};
  const double *axis[3] = {&zero, &zero, &zero};
  int64_t off = 0;
  for (int d = 0; d < ndim; ++d) {
    SR_CHECK(shape[d] >= 1 && shape[d] <= INT32_MAX, "sr_power_spectrum: bad size %lld of axis %d", (long long)shape[d], d);
    n[d] = shape[d];
    axis[d] = coords + off;
    off += shape[d];
  }
  return spectrum_nd("sr_power_spectrum", field, ndim, n, axis, rule, edges, n_bins, norm, sum, count, overflow);
}

// After the path: radially binned 2-D power spectrum of a detector image (radial_2Dspectrum,
// src/utils/power_spectrum.py:372-421): |fft2(img)|^2/(n0*n1)^2 summed and counted over the wavenumber bins
// [edges[b], edges[b+1]), the N-D path's edges rule.
extern "C" int sr_radial_spectrum2d(const double *img, int n0, int n1, const double *k0, const double *k1,
                                    const double *edges, int n_edges, double *sum, uint64_t *count) {
  SR_CHECK(img && k0 && k1 && edges && sum && count, "sr_radial_spectrum2d: NULL argument");
  SR_CHECK(n0 > 0 && n1 > 0 && n_edges >= 2, "sr_radial_spectrum2d: bad sizes");
  static const double zero = 0.0;
  const int64_t n[3] = {n0, n1, 1};
  const double *axis[3] = {k0, k1, &zero};
  const double nn = (double)n0 * (double)n1;
  return spectrum_nd("sr_radial_spectrum2d", img, 2, n, axis, SR_SPECTRUM_EDGES, edges, n_edges - 1, nn * nn, sum, count,
                     nullptr);
}

extern "C" int sr_field_ifft_real(const double *noise, const float *amp, int n0, int n1, int n2, int normalise, double *out) {
  SR_CHECK(noise && amp && out, "sr_field_ifft_real: NULL argument");
  SR_CHECK(n0 > 0 && n1 > 0 && n2 > 0, "sr_field_ifft_real: bad shape (%d, %d, %d)", n0, n1, n2);
  int rc = sr::ensure_init();
  if (rc) return rc;
  Fft *F;
  if ((rc = fft_lib(&F))) return rc;
  hipStream_t st = sr::ctx().stream;
  const int64_t n = (int64_t)n0 * n1 * n2;
  sr::CallBuffers buf;
  double2 *d_w = nullptr;
  float *d_a = nullptr;
  double *d_f = nullptr;
  unsigned long long *d_m = nullptr;
  hipfftHandle plan = nullptr;
  SR_RC(buf.alloc(&d_w, (size_t)n));
  SR_RC(buf.alloc(&d_a, (size_t)n));
  SR_RC(buf.alloc(&d_m, 1));
  SR_HIP(hipMemcpyAsync(d_w, noise, sizeof(double2) * n, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(d_a, amp, sizeof(float) * n, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemsetAsync(d_m, 0, sizeof(unsigned long long), st));
  const int block = 256;
  const int64_t blocks = (n + block - 1) / block;  // one capped_grid per launch: each is counted (sr_grid_stats)
  hipLaunchKernelGGL(k_shape_noise, dim3(sr::capped_grid(blocks, 32)), dim3(block), 0, st, d_w, (const float *)d_a, n);
  SR_HIP(hipGetLastError());
  SR_RC(fft_plan(F, 3, n0, n1, n2, &plan));  // C order: n2 fastest, as the NumPy array
  SR_FFT("sr_field_ifft_real", F->SetStream(plan, st));
  SR_FFT("sr_field_ifft_real", F->ExecZ2Z(plan, d_w, d_w, HIPFFT_BACKWARD));
  buf.release(d_a);  // before d_f: the call's peak stays at the transform's buffer plus one field
  SR_RC(buf.alloc(&d_f, (size_t)n));
  hipLaunchKernelGGL(k_real_scaled, dim3(sr::capped_grid(blocks, 32)), dim3(block), 0, st, (const double2 *)d_w, n, 1.0 / (double)n, d_f, d_m);
  if (normalise) hipLaunchKernelGGL(k_divide, dim3(sr::capped_grid(blocks, 32)), dim3(block), 0, st, d_f, n, (const unsigned long long *)d_m);
  return sr::stage_out(st, {{out, d_f, sizeof(double) * n}});
}

extern "C" int sr_field_modesum(int ndim, const int64_t *shape, const double *coords, int nmodes, const double *k,
                                const double *amp, const double *phase, double *out) {
  SR_CHECK(shape && coords && k && amp && phase && out, "sr_field_modesum: NULL argument");
  SR_CHECK(ndim >= 1 && ndim <= 3, "sr_field_modesum: ndim %d (1, 2 or 3)", ndim);
  SR_CHECK(nmodes >= 1, "sr_field_modesum: nmodes %d (>= 1)", nmodes);
  for (int d = 0; d < ndim; ++d)
    SR_CHECK(shape[d] >= 1 && shape[d] <= INT32_MAX, "sr_field_modesum: bad size %lld of axis %d", (long long)shape[d], d);
  // the problem's axes on the kernel's (a0, a1, a2): the last axis on a2; 2-D leaves a1, 1-D a0 and a1 at one cell
  static const int kAxis[3][3] = {{2, -1, -1}, {0, 2, -1}, {0, 1, 2}};
  static const int kPmask[3] = {0x1, 0x3, 0xf};  // P1; P1, P2; P1..P4
  const int64_t M = nmodes;
  int64_t n[3] = {1, 1, 1}, cpos[3] = {0, 0, 0};
  int64_t off = 0;
  for (int d = 0; d < ndim; ++d) {
    n[kAxis[ndim - 1][d]] = shape[d];
    cpos[d] = off;
    off += shape[d];
  }
  SR_CHECK(n[0] * n[1] <= INT64_MAX / n[2], "sr_field_modesum: field too large");
  const int64_t n_cells = n[0] * n[1] * n[2], n_axes = n[0] + n[1] + n[2];
  // staging: [coords on a0, a1, a2 (n_axes) | k on a0, a1, a2 (3 M) | amp (M) | P1..P4 (4 M)]; missing entries 0
  std::vector<double> h((size_t)(n_axes + 8 * M), 0.0);
  for (int d = 0; d < ndim; ++d) {
    const int a = kAxis[ndim - 1][d];
    const int64_t dst = (a > 0 ? n[0] : 0) + (a > 1 ? n[1] : 0);
    std::copy(coords + cpos[d], coords + cpos[d] + shape[d], h.begin() + dst);
    std::copy(k + d * M, k + (d + 1) * M, h.begin() + n_axes + a * M);
  }
  std::copy(amp, amp + M, h.begin() + n_axes + 3 * M);
  std::copy(phase, phase + ((int64_t)1 << (ndim - 1)) * M, h.begin() + n_axes + 4 * M);
  int rc = sr::ensure_init();
  if (rc) return rc;
  hipStream_t st = sr::ctx().stream;
  sr::CallBuffers buf;
  double *d_in = nullptr, *d_out = nullptr;
  double2 *d_tab = nullptr;
  const bool tile_j = n[1] > 1;  // 3-D: G is reused over T = 8 rows i and formed for 4 rows j; Y == 1: 16 rows i
  SR_RC(buf.alloc(&d_in, h.size()));
  SR_RC(buf.alloc(&d_tab, tile_j ? modesum_table_len<8, 4>(M, n) : modesum_table_len<16, 1>(M, n)));
  SR_RC(buf.alloc(&d_out, (size_t)n_cells));
  SR_HIP(hipMemcpyAsync(d_in, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, st));
  if (tile_j)
    run_modesum<8, 4>(d_in, kPmask[ndim - 1], nmodes, n, d_tab, d_out, st);
  else
    run_modesum<16, 1>(d_in, kPmask[ndim - 1], nmodes, n, d_tab, d_out, st);
  return sr::stage_out(st, {{out, d_out, sizeof(double) * (size_t)n_cells}});
}
