// Wave optics: a paraxial split-step Fourier march of a complex field through a domain's electron density along a grid axis
// (sr_field_wave) and the ideal relay to the detector with a Fourier-plane mask (sr_wave_image); include/synthray.h states the rule
// every mode and pixel follows, operation for operation.  No reference counterpart.
//
// The field (mu x mv complex128, C order) stays in one device buffer for the whole march.  Per cell: hipFFT forward (the library's
// cached 2-D Z2Z plan, in place, on the library's stream), k_spectral (the Fresnel factor and the 1/(mu mv) of the pair of
// transforms, one mode per lane), hipFFT inverse, k_screen (the cell's phase and absorption screen, four pixels 256 apart per lane
// so that the power sum's first level is in registers).  A pixel's lateral cell and weights do not depend on the plane: they are
// two tables of mu + mv entries the host builds once with the rule's own arithmetic.
//
// LAYOUT.  The fields are C order (nx, ny, nz).  A node plane of axis x is one contiguous (ny, nz) block and one of axis y is nx
// rows of nz: in both the frame's fast index j runs along z, the contiguous one, and k_screen gathers the planes in place.  A node
// plane of axis z is the strided direction: gathered in place, every element costs a 128-byte line of which 8 (4) bytes are used,
// and the same lines come back for each of the next 15 (31) planes.  k_slab brings the volume in as SLABS of kSlab = 32 node planes
// instead: a workgroup reads 64 columns x 32 planes with the planes on the lanes (256 contiguous bytes per column in float64),
// turns the tile in LDS (rows padded by one element: the column-major read-back is conflict-free) and writes it plane-major with
// the columns on the lanes, 512 contiguous bytes per plane.  Two slab buffers per field alternate, so the two planes of a cell that
// straddles a slab boundary are both present; every plane of the volume is read from its strided home exactly once.
// No atomics anywhere: a repeated call returns identical bits.  Compiled with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "fft.hpp"

namespace {

constexpr int kSlab = 32;      // node planes per slab of a z march
constexpr int kGroup = 1024;   // pixels per workgroup of k_screen: one partial sum of the power

#include "nrl_node.inc"  // the absorption coefficient of a node: sr_field_emission's own

// D(d) between the two transforms: th = -(pd*(fu^2 + fv^2)), the complex product and the scale
__global__ void __launch_bounds__(256) k_spectral(double2 *__restrict__ U, int mv, int64_t npix, const double *__restrict__ fu,
                                                  const double *__restrict__ fv, double pd, double scale) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= npix) return;
  const int64_t i = t / mv;
  const int j = (int)(t - i * mv);
  const double a = fu[i], b = fv[j];
  const double th = -(pd * (a * a + b * b));
  double si, co;
  sincos(th, &si, &co);
  const double2 u = U[t];
  U[t] = make_double2((u.x * co - u.y * si) * scale, (u.x * si + u.y * co) * scale);
}

struct MaskArgs {
  double pd, scale, lf, Ra2, Rs2, knife_offset, knife_dir;
  int flags, knife_axis;
};

// sr_wave_image between its two transforms: the defocus factor, the scale, the Fourier-plane masks
__global__ void __launch_bounds__(256) k_mask(double2 *__restrict__ U, int mv, int64_t npix, const double *__restrict__ fu,
                                              const double *__restrict__ fv, MaskArgs M) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= npix) return;
  const int64_t i = t / mv;
  const int j = (int)(t - i * mv);
  const double a = fu[i], b = fv[j];
  const double th = -(M.pd * (a * a + b * b));
  double si, co;
  sincos(th, &si, &co);
  const double2 u = U[t];
  double re = (u.x * co - u.y * si) * M.scale, im = (u.x * si + u.y * co) * M.scale;
  const double xf = M.lf * a, yf = M.lf * b;
  const double r2 = xf * xf + yf * yf;
  bool rej = false;
  if (M.flags & SR_WAVE_APERTURE) rej = rej || r2 > M.Ra2;
  if (M.flags & SR_WAVE_STOP) rej = rej || r2 < M.Rs2;
  if (M.flags & SR_WAVE_KNIFE) {
    const double x = M.knife_axis ? yf : xf;
    rej = rej || (M.knife_dir > 0.0 ? x > M.knife_offset : x < M.knife_offset);
  }
  if (rej) re = im = 0.0;
  U[t] = make_double2(re, im);
}

// planes p_lo .. p_lo + np - 1 (np <= kSlab) of a (ncol, nz) array -> dst[(p - p_lo)*ncol + col]
template <typename T>
__global__ void __launch_bounds__(256) k_slab(const T *__restrict__ src, T *__restrict__ dst, int64_t ncol, int nz, int p_lo, int np) {
  __shared__ T tile[64][kSlab + 1];
  const int64_t col0 = (int64_t)blockIdx.x * 64;
  {
    const int k = threadIdx.x & (kSlab - 1), c = threadIdx.x / kSlab;  // 8 columns per pass
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int cc = c + 8 * r;
      const int64_t col = col0 + cc;
      if (col < ncol && k < np) tile[cc][k] = src[col * nz + p_lo + k];
    }
  }
  __syncthreads();
  {
    const int c = threadIdx.x & 63, k = threadIdx.x >> 6;  // 4 planes per pass
    const int64_t col = col0 + c;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int kk = k + 4 * r;
      if (col < ncol && kk < np) dst[(int64_t)kk * ncol + col] = tile[c][kk];
    }
  }
}

struct ScreenArgs {
  const void *ne[2], *Te[2], *Z[2];  // node (0, 0) of plane k and of plane k'
  int64_t su, sv;                    // element strides of the lateral node indices (iu, iv)
  const int *cu, *cv;                // the lateral cell of a frame row / column, -1: outside the grid
  const double *tu, *tv;             // its weight
  const double *wu, *wv;             // the edge absorber's windows
  double2 *U;
  int mv;
  int64_t npix;
  double k0h, h, omega, Zu;
  double *partial;                   // the groups' sums of |U|^2 for this cell: group g at partial[g * n_cells]
  int n_cells;
};

template <typename T>
__device__ __forceinline__ double plane_value(const void *base, int64_t off, int64_t su, int64_t sv, double w00, double w01, double w10,
                                              double w11) {
  const T *f = static_cast<const T *>(base) + off;
  return (((double)f[0] * w00 + (double)f[sv] * w01) + (double)f[su] * w10) + (double)f[su + sv] * w11;
}

// n - 1 of one plane; opaque: the plane is over-critical here
__device__ __forceinline__ double index_m1(double ne, double omega, bool &opaque) {
  if (ne <= 0.0) return 0.0;
  const double wp = 5.64e4 * sqrt(ne * 1e-6);
  const double r = wp / omega;
  const double q = r * r;
  if (q >= 1.0) {
    opaque = true;
    return 0.0;
  }
  return -q / (1.0 + sqrt(1.0 - q));
}

template <typename T, bool HAS_TE, bool HAS_Z, bool POWER>
__global__ void __launch_bounds__(256) k_screen(ScreenArgs A) {
  const int64_t first = (int64_t)blockIdx.x * kGroup + threadIdx.x;
  double p[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t t = first + 256 * r;
    p[r] = 0.0;
    if (t >= A.npix) continue;
    const int64_t i = t / A.mv;
    const int j = (int)(t - i * A.mv);
    const int ci = A.cu[i], cj = A.cv[j];
    double m0 = 0.0, m1 = 0.0, al0 = 0.0, al1 = 0.0;
    bool opaque = false;
    if (ci >= 0 && cj >= 0) {
      const double wu_ = A.tu[i], wv_ = A.tv[j];
      const double uu = 1.0 - wu_, uv = 1.0 - wv_;
      const double w00 = uu * uv, w01 = uu * wv_, w10 = wu_ * uv, w11 = wu_ * wv_;
      const int64_t off = (int64_t)ci * A.su + (int64_t)cj * A.sv;
      const double ne0 = plane_value<T>(A.ne[0], off, A.su, A.sv, w00, w01, w10, w11);
      const double ne1 = plane_value<T>(A.ne[1], off, A.su, A.sv, w00, w01, w10, w11);
      m0 = index_m1(ne0, A.omega, opaque);
      m1 = index_m1(ne1, A.omega, opaque);
      if (HAS_TE) {
        const double Te0 = plane_value<T>(A.Te[0], off, A.su, A.sv, w00, w01, w10, w11);
        const double Te1 = plane_value<T>(A.Te[1], off, A.su, A.sv, w00, w01, w10, w11);
        const double Z0 = HAS_Z ? plane_value<T>(A.Z[0], off, A.su, A.sv, w00, w01, w10, w11) : A.Zu;
        const double Z1 = HAS_Z ? plane_value<T>(A.Z[1], off, A.su, A.sv, w00, w01, w10, w11) : A.Zu;
        al0 = node_alpha(node_terms(ne0, Te0, Z0), A.omega);
        al1 = node_alpha(node_terms(ne1, Te1, Z1), A.omega);
      }
    }
    const double ph = A.k0h * (0.5 * (m0 + m1));
    double a = 1.0;
    if (HAS_TE) {
      const double dtau = (0.5 * (al0 + al1)) * A.h;
      a = exp(-(0.5 * dtau));
    }
    const double w = (a * A.wu[i]) * A.wv[j];
    double si, co;
    sincos(ph, &si, &co);
    const double2 u = A.U[t];
    double re = (u.x * co - u.y * si) * w, im = (u.x * si + u.y * co) * w;
    if (opaque) re = im = 0.0;
    A.U[t] = make_double2(re, im);
    p[r] = re * re + im * im;
  }
  if (POWER) {
    __shared__ double s_w[4];
    double s = ((p[0] + p[1]) + p[2]) + p[3];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) A.partial[(int64_t)blockIdx.x * A.n_cells] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
  }
}

// power[c] = the groups' sums of cell c in ascending order; partial is (n_groups, n_cells), so the lanes (one cell each) read
// consecutive words of a group's row
__global__ void __launch_bounds__(64) k_power(const double *__restrict__ partial, int64_t n_groups, int n_cells, double *__restrict__ power) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n_cells) return;
  double s = 0.0;
  for (int64_t g = 0; g < n_groups; ++g) s = s + partial[g * n_cells + c];
  power[c] = s;
}

template <typename T>
void launch_screen(bool has_te, bool has_z, bool power, unsigned grid, hipStream_t st, const ScreenArgs &A) {
  sr::with_flags(
      [&](auto te, auto z, auto pw) {
        constexpr bool kTe = decltype(te)::value, kZ = decltype(z)::value, kPw = decltype(pw)::value;
        if constexpr (kTe || !kZ) hipLaunchKernelGGL((k_screen<T, kTe, kZ, kPw>), dim3(grid), dim3(256), 0, st, A);
      },
      has_te, has_te && has_z, power);
}

using sr::positive;

// sr_field_resample's `cell` rule for the pixels x0 + i*dx of one lateral axis; cell -1: outside
void lateral_table(const std::vector<double> &g, int m, double x0, double dx, int *cell, double *w) {
  const int n = (int)g.size();
  for (int i = 0; i < m; ++i) {
    const double p = x0 + (double)i * dx;
    cell[i] = -1;
    w[i] = 0.0;
    if (!(p >= g[0] && p <= g[n - 1])) continue;
    int c = (int)(std::upper_bound(g.begin(), g.end(), p) - g.begin()) - 1;  // the largest c with g[c] <= p
    c = c < 0 ? 0 : (c > n - 2 ? n - 2 : c);
    cell[i] = c;
    w[i] = (p - g[c]) / (g[c + 1] - g[c]);
  }
}

int check_frame(const char *who, int mu, int mv, const double *fu, const double *fv, const double *U_in, const double *U_out) {
  SR_CHECK(fu != nullptr && fv != nullptr && U_in != nullptr && U_out != nullptr, "%s: NULL argument (fu, fv, U_in or U_out)", who);
  SR_CHECK(mu >= 2 && mv >= 2, "%s: the frame needs mu, mv >= 2, got %d x %d", who, mu, mv);
  SR_CHECK((int64_t)mu * mv <= ((int64_t)1 << 30), "%s: the frame %d x %d has more than 2^30 pixels", who, mu, mv);
  return SR_OK;
}

// the events of a march timed by parts: one between all the launches, summed by kind afterwards
struct Parts {
  bool on = false;
  std::vector<hipEvent_t> ev;
  std::vector<int> kind;  // of the work between ev[k] and ev[k + 1]: 0 hipFFT, 1 the library's kernels
  int mark(int k, hipStream_t st) {
    if (!on) return SR_OK;
    hipEvent_t e;
    SR_HIP(hipEventCreate(&e));
    ev.push_back(e);
    kind.push_back(k);
    SR_HIP(hipEventRecord(e, st));
    return SR_OK;
  }
  int sums(double *ms) {
    ms[0] = ms[1] = 0.0;
    for (size_t k = 0; k + 1 < ev.size(); ++k) {
      float t = 0.f;
      SR_HIP(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
      ms[kind[k + 1]] += t;  // an event is marked AFTER the work it closes, with that work's kind
    }
    return SR_OK;
  }
  ~Parts() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
};

}  // namespace

extern "C" int sr_field_wave(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_wave_params *p, const double *fu,
                             const double *fv, const double *wu, const double *wv, const double *U_in, double *U_out, double *power,
                             double *kernel_ms) {
  const char *who = "sr_field_wave";
  SR_CHECK(p != nullptr, "%s: NULL argument (p)", who);
  if (int rc = check_frame(who, p->mu, p->mv, fu, fv, U_in, U_out)) return rc;
  SR_CHECK(positive(p->lambda), "%s: lambda must be finite and positive", who);
  SR_CHECK(positive(p->omega) && positive(p->k0) && positive(p->pi_l), "%s: omega, k0 and pi_l must be finite and positive", who);
  SR_CHECK(positive(p->du) && positive(p->dv), "%s: du and dv must be finite and positive", who);
  SR_CHECK(std::isfinite(p->u0) && std::isfinite(p->v0), "%s: non-finite u0 or v0", who);
  SR_CHECK(p->toward == 1 || p->toward == -1, "%s: toward must be +1 or -1, got %d", who, p->toward);
  SR_CHECK(p->axis >= 0 && p->axis <= 2, "%s: axis must be 0, 1 or 2, got %d", who, p->axis);
  SR_CHECK(ne != nullptr, "%s: NULL ne field", who);
  if (int rc = sr::check_fields(who, ne, "ne", {{"ne", ne, 1}, {"Te", Te, 1}, {"Z", Z, 1}})) return rc;
  SR_CHECK(Te == nullptr || Z != nullptr || std::isfinite(p->Z), "%s: non-finite uniform Z", who);
  if (int rc = sr::ensure_init()) return rc;
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;
  sr::Fft *F;
  if (int rc = sr::fft_lib(&F)) return rc;
  hipfftHandle plan = nullptr;
  const int mu = p->mu, mv = p->mv, axis = p->axis;
  if (int rc = sr::fft_plan(F, 2, mu, mv, 0, &plan)) return rc;

  const bool has_te = Te != nullptr, has_z = has_te && Z != nullptr;
  const int n_fields = 1 + (has_te ? 1 : 0) + (has_z ? 1 : 0);
  const sr_field *fld[3] = {ne, has_te ? Te : nullptr, has_z ? Z : nullptr};
  const int n = ne->n[axis], n_cells = n - 1;
  const int ua = axis == 0 ? 1 : 0, va = axis == 2 ? 1 : 2;  // the lateral axes
  const int64_t ny = ne->n[1], nz = ne->n[2];
  const int64_t npix = (int64_t)mu * mv, n_groups = (npix + kGroup - 1) / kGroup;
  const size_t elem = ne->is_f64 ? sizeof(double) : sizeof(float);
  const int64_t ncol = (int64_t)ne->n[0] * ny;  // columns of a z march

  // the lateral tables
  std::vector<int> cells((size_t)mu + mv);
  std::vector<double> tab(3 * ((size_t)mu + mv));  // weights | windows | frequencies, each (u then v)
  lateral_table(ne->hg[ua], mu, p->u0, p->du, cells.data(), tab.data());
  lateral_table(ne->hg[va], mv, p->v0, p->dv, cells.data() + mu, tab.data() + mu);
  double *win = tab.data() + mu + mv, *frq = win + mu + mv;
  for (int i = 0; i < mu; ++i) win[i] = wu ? wu[i] : 1.0;
  for (int j = 0; j < mv; ++j) win[mu + j] = wv ? wv[j] : 1.0;
  memcpy(frq, fu, sizeof(double) * mu);
  memcpy(frq + mu, fv, sizeof(double) * mv);

  // one scratch block: U | tables | cells | partial sums | power | the slab buffers of a z march
  const size_t b_slab = axis == 2 ? sr::up256(elem * (size_t)kSlab * (size_t)ncol) : 0;
  double2 *d_U;
  double *d_tab, *d_part, *d_pow;
  int *d_cell;
  char *d_slab;  // [field][parity]
  sr::Carve carve;
  carve.take(&d_U, (size_t)npix);
  carve.take(&d_tab, tab.size());
  carve.take(&d_cell, cells.size());
  carve.take(&d_part, power ? (size_t)n_groups * n_cells : 0);
  carve.take(&d_pow, power ? (size_t)n_cells : 0);
  carve.take(&d_slab, b_slab * 2 * n_fields);
  if (!carve.alloc()) return SR_ERR_HIP;
  const double *d_fu = d_tab + 2 * ((size_t)mu + mv), *d_fv = d_fu + mu;

  if (int rc = sr::upload_sync(d_U, U_in, sizeof(double2) * (size_t)npix, st)) return rc;
  SR_HIP(hipMemcpyAsync(d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(d_cell, cells.data(), sizeof(int) * cells.size(), hipMemcpyHostToDevice, st));
  SR_FFT(who, F->SetStream(plan, st));

  ScreenArgs A{};
  A.cu = d_cell;
  A.cv = d_cell + mu;
  A.tu = d_tab;
  A.tv = d_tab + mu;
  A.wu = d_tab + mu + mv;
  A.wv = A.wu + mu;
  A.U = d_U;
  A.mv = mv;
  A.npix = npix;
  A.omega = p->omega;
  A.Zu = has_z ? 0.0 : p->Z;
  A.su = axis == 0 ? nz : (axis == 1 ? ny * nz : ny);  // z: the plane-major slabs, (nx, ny) per plane
  A.sv = 1;
  int loaded[2] = {-1, -1};  // the slab each buffer parity holds
  Parts parts;
  parts.on = kernel_ms != nullptr && p->time_parts != 0;

  // node (0, 0) of physical plane pl of field f; a z march loads the plane's slab first
  auto plane_ptr = [&](int f, int pl) -> const void * {
    const char *base = static_cast<const char *>(fld[f]->data);
    if (axis == 0) return base + elem * (size_t)pl * (size_t)(ny * nz);
    if (axis == 1) return base + elem * (size_t)pl * (size_t)nz;
    const int s = pl / kSlab;
    return d_slab + b_slab * (size_t)(2 * f + (s & 1)) + elem * (size_t)(pl - s * kSlab) * (size_t)ncol;
  };
  auto need_slab = [&](int pl) {
    const int s = pl / kSlab;
    if (axis != 2 || loaded[s & 1] == s) return;
    const int p_lo = s * kSlab, np = std::min(kSlab, n - p_lo);
    const unsigned grid = (unsigned)((ncol + 63) / 64);
    for (int f = 0; f < n_fields; ++f) {
      void *dst = d_slab + b_slab * (size_t)(2 * f + (s & 1));
      if (ne->is_f64)
        hipLaunchKernelGGL(k_slab<double>, dim3(grid), dim3(256), 0, st, static_cast<const double *>(fld[f]->data),
                           static_cast<double *>(dst), ncol, (int)nz, p_lo, np);
      else
        hipLaunchKernelGGL(k_slab<float>, dim3(grid), dim3(256), 0, st, static_cast<const float *>(fld[f]->data),
                           static_cast<float *>(dst), ncol, (int)nz, p_lo, np);
    }
    loaded[s & 1] = s;
  };
  const std::vector<double> &g = ne->hg[axis];
  auto plane_of = [&](int m) { return p->toward > 0 ? m : n - 1 - m; };
  auto cell_h = [&](int cc) { return std::fabs(g[plane_of(cc + 1)] - g[plane_of(cc)]); };
  const double scale = 1.0 / ((double)mu * (double)mv);
  const unsigned grid_pix = (unsigned)((npix + 255) / 256);
  auto diffract = [&](double d) -> int {
    SR_FFT(who, F->ExecZ2Z(plan, reinterpret_cast<hipfftDoubleComplex *>(d_U), reinterpret_cast<hipfftDoubleComplex *>(d_U), HIPFFT_FORWARD));
    if (int rc = parts.mark(0, st)) return rc;
    hipLaunchKernelGGL(k_spectral, dim3(grid_pix), dim3(256), 0, st, d_U, mv, npix, d_fu, d_fv, p->pi_l * d, scale);
    if (int rc = parts.mark(1, st)) return rc;
    SR_FFT(who, F->ExecZ2Z(plan, reinterpret_cast<hipfftDoubleComplex *>(d_U), reinterpret_cast<hipfftDoubleComplex *>(d_U), HIPFFT_BACKWARD));
    return parts.mark(0, st);
  };

  SR_HIP(hipEventRecord(c.ev[0], st));
  if (int rc = parts.mark(1, st)) return rc;
  for (int cc = 0; cc < n_cells; ++cc) {
    const double h = cell_h(cc);
    const double d = cc == 0 ? 0.5 * h : 0.5 * (cell_h(cc - 1) + h);
    if (int rc = diffract(d)) return rc;
    const int k0p = plane_of(cc), k1p = plane_of(cc + 1);
    need_slab(k0p);
    need_slab(k1p);
    for (int f = 0; f < n_fields; ++f) {
      const void **dst = f == 0 ? A.ne : (f == 1 ? A.Te : A.Z);
      dst[0] = plane_ptr(f, k0p);
      dst[1] = plane_ptr(f, k1p);
    }
    A.h = h;
    A.k0h = p->k0 * h;
    A.partial = power ? d_part + cc : nullptr;
    A.n_cells = n_cells;
    if (ne->is_f64)
      launch_screen<double>(has_te, has_z, power != nullptr, (unsigned)n_groups, st, A);
    else
      launch_screen<float>(has_te, has_z, power != nullptr, (unsigned)n_groups, st, A);
    if (int rc = parts.mark(1, st)) return rc;
  }
  if (int rc = diffract(0.5 * cell_h(n_cells - 1))) return rc;
  if (power) {
    hipLaunchKernelGGL(k_power, dim3((unsigned)((n_cells + 63) / 64)), dim3(64), 0, st, (const double *)d_part, n_groups, n_cells, d_pow);
    if (int rc = parts.mark(1, st)) return rc;
  }
  SR_HIP(hipGetLastError());
  SR_HIP(hipEventRecord(c.ev[1], st));
  SR_HIP(hipMemcpyAsync(U_out, d_U, sizeof(double2) * (size_t)npix, hipMemcpyDeviceToHost, st));
  if (power) SR_HIP(hipMemcpyAsync(power, d_pow, sizeof(double) * n_cells, hipMemcpyDeviceToHost, st));
  if (int rc = sr::finish_timed(c, kernel_ms)) return rc;
  if (kernel_ms) {
    kernel_ms[1] = kernel_ms[2] = 0.0;
    if (parts.on) return parts.sums(kernel_ms + 1);
  }
  return SR_OK;
}

extern "C" int sr_wave_image(const sr_wave_image_params *p, const double *fu, const double *fv, const double *U_in, double *U_out,
                             double *kernel_ms) {
  const char *who = "sr_wave_image";
  SR_CHECK(p != nullptr, "%s: NULL argument (p)", who);
  if (int rc = check_frame(who, p->mu, p->mv, fu, fv, U_in, U_out)) return rc;
  SR_CHECK(std::isfinite(p->pi_l) && std::isfinite(p->defocus) && std::isfinite(p->lf), "%s: non-finite pi_l, defocus or lf", who);
  SR_CHECK((p->flags & ~(SR_WAVE_APERTURE | SR_WAVE_STOP | SR_WAVE_KNIFE)) == 0, "%s: unknown bits in flags %d", who, p->flags);
  SR_CHECK(!(p->flags & SR_WAVE_APERTURE) || std::isfinite(p->Ra), "%s: non-finite Ra", who);
  SR_CHECK(!(p->flags & SR_WAVE_STOP) || std::isfinite(p->Rs), "%s: non-finite Rs", who);
  if (p->flags & SR_WAVE_KNIFE) {
    SR_CHECK(std::isfinite(p->knife_offset), "%s: non-finite knife_offset", who);
    SR_CHECK(p->knife_axis == 0 || p->knife_axis == 1, "%s: knife_axis must be 0 or 1, got %d", who, p->knife_axis);
    SR_CHECK(p->knife_dir > 0.0 || p->knife_dir < 0.0, "%s: knife_dir must be > 0 or < 0", who);
  }
  if (int rc = sr::ensure_init()) return rc;
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;
  sr::Fft *F;
  if (int rc = sr::fft_lib(&F)) return rc;
  hipfftHandle plan = nullptr;
  const int mu = p->mu, mv = p->mv;
  if (int rc = sr::fft_plan(F, 2, mu, mv, 0, &plan)) return rc;
  const int64_t npix = (int64_t)mu * mv;
  double2 *d_U;
  double *d_f;
  sr::Carve carve;
  carve.take(&d_U, (size_t)npix);
  carve.take(&d_f, (size_t)mu + mv);
  if (!carve.alloc()) return SR_ERR_HIP;
  if (int rc = sr::upload_sync(d_U, U_in, sizeof(double2) * (size_t)npix, st)) return rc;
  SR_HIP(hipMemcpyAsync(d_f, fu, sizeof(double) * mu, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(d_f + mu, fv, sizeof(double) * mv, hipMemcpyHostToDevice, st));
  SR_FFT(who, F->SetStream(plan, st));
  MaskArgs M{};
  M.pd = p->pi_l * p->defocus;
  M.scale = 1.0 / ((double)mu * (double)mv);
  M.lf = p->lf;
  M.Ra2 = p->Ra * p->Ra;
  M.Rs2 = p->Rs * p->Rs;
  M.knife_offset = p->knife_offset;
  M.knife_dir = p->knife_dir;
  M.flags = p->flags;
  M.knife_axis = p->knife_axis;
  SR_HIP(hipEventRecord(c.ev[0], st));
  SR_FFT(who, F->ExecZ2Z(plan, reinterpret_cast<hipfftDoubleComplex *>(d_U), reinterpret_cast<hipfftDoubleComplex *>(d_U), HIPFFT_FORWARD));
  hipLaunchKernelGGL(k_mask, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, d_U, mv, npix, (const double *)d_f,
                     (const double *)(d_f + mu), M);
  SR_HIP(hipGetLastError());
  SR_FFT(who, F->ExecZ2Z(plan, reinterpret_cast<hipfftDoubleComplex *>(d_U), reinterpret_cast<hipfftDoubleComplex *>(d_U), HIPFFT_BACKWARD));
  SR_HIP(hipEventRecord(c.ev[1], st));
  SR_HIP(hipMemcpyAsync(U_out, d_U, sizeof(double2) * (size_t)npix, hipMemcpyDeviceToHost, st));
  return sr::finish_timed(c, kernel_ms);
}
