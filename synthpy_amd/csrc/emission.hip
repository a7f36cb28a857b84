// Self-emission images: emission with self-absorption along a grid axis (sr_field_emission; include/synthray.h states the rule
// every node, cell and column follows, operation for operation).
//
// An ORDERED recurrence per column, I <- I*a + b cell by cell, where k_project's line integral is an unordered sum.  The fields are
// C order (nx, ny, nz), so the two kinds of axis want two kernels; in both, consecutive lanes read consecutive addresses, every
// field is read once for all bands (the band loop is innermost), and values are float64 from the load on.
//   axis z (k_emission_z): a column is contiguous.  One WAVEFRONT per column, 64 planes at a time, one plane per lane: the lanes
//     form alpha and S of their nodes in parallel, a lane takes its cell's other node from the lane before it (lane 0 from the last
//     lane of the chunk before: the cell across the chunk boundary), forms the cell's (a, b, dtau), and a fixed shuffle tree composes
//     the up to 64 affine maps in march order -- (a1, b1) then (a2, b2) -> (a1*a2, b1*a2 + b2) -- before lane 0's total is composed
//     onto the carried (I, tau).  Lanes without a cell hold the identity (1, 0, 0), which composes exactly.
//   axis x or y (k_emission_xy): the lateral z index is contiguous.  One LANE per column marches serially; the loads of the planes
//     one and two steps ahead are in flight while a plane's arithmetic runs.
// toward = -1 walks the same addresses backwards.  No LDS, no atomics: a repeated call returns identical bits.
// Compiled with -ffp-contract=off: products and sums round separately, as the NumPy restatement's do (tests/test_emission.py).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"

namespace {

struct EmArgs {
  const void *ne, *Te, *Z;  // (nx, ny, nz) C order; Te, Z unused where the kernel is instantiated without them
  const double *g;          // node coordinates of the marched axis (float32 values widened)
  const double *back;       // (n_band, ncol) or nullptr
  double *I, *tau;          // (n_band, ncol)
  int n, toward;            // planes along the axis; +1 | -1
  int64_t ncol;
  int64_t nv, row_stride, plane_stride;  // k_emission_xy: column c = (iu, iv) = (c / nv, c % nv) starts at iu*row_stride + iv
  double omega[SR_MAX_BANDS], e_ph[SR_MAX_BANDS], c_omega[SR_MAX_BANDS];
  double uTe, uZ;
};

// numpy's maximum: a NaN operand gives NaN
__device__ __forceinline__ double nmax(double a, double b) { return (a > b || a != a) ? a : b; }

// alpha [1/m] and S of one node: what every band shares, then one band.  A dark node's zeros are selected at the end; an early
// return here left the callers' per-band arrays in scratch.
struct NodeTerms {
  bool dark;  // Te <= 0 or ne <= 0: alpha = S = 0
  double Te, n, wp, L, num, zc, it;
};
__device__ __forceinline__ NodeTerms node_terms(double ne, double Te, double Z) {
  NodeTerms t;
  const double q = sqrt(Te);
  t.dark = Te <= 0.0 || ne <= 0.0;
  t.Te = Te;
  t.n = ne * 1e-6;
  t.wp = 5.64e4 * sqrt(t.n);
  t.L = nmax(Z * 1.602176634e-19 / Te, 2.760428269727312e-10 / q);
  t.num = 4.19e5 * q;
  t.zc = (3.1e-5 * Z) * sr::kC;
  t.it = 1.0 / (Te * q);
  return t;
}
__device__ __forceinline__ void node_band(const NodeTerms &t, double omega, double e_ph, double c_omega, double &al, double &S) {
  const double w = nmax(t.wp, omega);
  const double lnL = nmax(2.0, log(t.num / (w * t.L)));
  const double r = t.n / omega;
  al = t.dark ? 0.0 : (((t.zc * (r * r)) * lnL) * t.it) / sr::kC;
  S = t.dark ? 0.0 : c_omega / expm1(e_ph / t.Te);
}
template <int NB>
__device__ __forceinline__ void node(const EmArgs &A, double ne, double Te, double Z, double (&al)[NB], double (&S)[NB]) {
  const NodeTerms t = node_terms(ne, Te, Z);
#pragma unroll
  for (int b = 0; b < NB; ++b) node_band(t, A.omega[b], A.e_ph[b], A.c_omega[b], al[b], S[b]);
}

template <typename T, bool HAS_TE, bool HAS_Z, int NB>
__device__ __forceinline__ void load_node(const EmArgs &A, int64_t at, double &ne, double &Te, double &Z) {
  ne = (double)static_cast<const T *>(A.ne)[at];
  Te = HAS_TE ? (double)static_cast<const T *>(A.Te)[at] : A.uTe;
  Z = HAS_Z ? (double)static_cast<const T *>(A.Z)[at] : A.uZ;
}

// the cell between two nodes of the march: I -> I*a + b, tau -> tau + dt
template <int NB>
__device__ __forceinline__ void cell(double h, const double (&al0)[NB], const double (&S0)[NB], const double (&al1)[NB],
                                     const double (&S1)[NB], double (&a)[NB], double (&b)[NB], double (&dt)[NB]) {
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    dt[k] = (0.5 * (al0[k] + al1[k])) * h;
    a[k] = exp(-dt[k]);
    b[k] = (0.5 * (S0[k] + S1[k])) * (-expm1(-dt[k]));
  }
}

template <typename T, bool HAS_TE, bool HAS_Z, int NB>
__global__ void __launch_bounds__(256) k_emission_z(EmArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t col = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); col < A.ncol; col += waves) {
    const int64_t base = col * A.n;
    double I[NB], tau[NB], al_c[NB], S_c[NB];  // the running (I, tau); alpha, S of the last plane of the chunk before
    double g_c = 0.0;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      I[k] = A.back ? A.back[k * A.ncol + col] : 0.0;
      tau[k] = al_c[k] = S_c[k] = 0.0;
    }
    for (int m0 = 0; m0 < A.n; m0 += 64) {
      const int m = m0 + lane;  // position in the march; the whole wavefront runs every chunk (the shuffles need all lanes)
      const bool live = m < A.n;
      const int p = A.toward > 0 ? m : A.n - 1 - m;
      double al[NB], S[NB], g = 0.0;
      if (live) {
        double ne, Te, Z;
        load_node<T, HAS_TE, HAS_Z, NB>(A, base + p, ne, Te, Z);
        g = A.g[p];
        node<NB>(A, ne, Te, Z, al, S);
      } else {
#pragma unroll
        for (int k = 0; k < NB; ++k) al[k] = S[k] = 0.0;
      }
      // the node before this one in the march: the lane below, for lane 0 the last plane of the chunk before
      double alp[NB], Sp[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const double x = __shfl_up(al[k], 1, 64), y = __shfl_up(S[k], 1, 64);
        alp[k] = lane == 0 ? al_c[k] : x;
        Sp[k] = lane == 0 ? S_c[k] : y;
      }
      const double gl = __shfl_up(g, 1, 64);
      const double gp = lane == 0 ? g_c : gl;
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        al_c[k] = __shfl(al[k], 63, 64);
        S_c[k] = __shfl(S[k], 63, 64);
      }
      g_c = __shfl(g, 63, 64);
      double a[NB], b[NB], dt[NB];
      if (live && m > 0) {
        cell<NB>(fabs(g - gp), alp, Sp, al, S, a, b, dt);
      } else {
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          a[k] = 1.0;
          b[k] = dt[k] = 0.0;
        }
      }
      // lane l ends with the composition of lanes l .. l + 2s - 1 in march order wherever that range lies inside the wavefront;
      // lane 0 reads only such lanes
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          const double a2 = __shfl_down(a[k], s, 64), b2 = __shfl_down(b[k], s, 64), t2 = __shfl_down(dt[k], s, 64);
          b[k] = b[k] * a2 + b2;
          a[k] = a[k] * a2;
          dt[k] = dt[k] + t2;
        }
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        I[k] = I[k] * __shfl(a[k], 0, 64) + __shfl(b[k], 0, 64);
        tau[k] = tau[k] + __shfl(dt[k], 0, 64);
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        A.I[k * A.ncol + col] = I[k];
        A.tau[k * A.ncol + col] = tau[k];
      }
    }
  }
}

template <typename T, bool HAS_TE, bool HAS_Z, int NB>
__global__ void __launch_bounds__(64) k_emission_xy(EmArgs A) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.ncol) return;
  const int64_t iu = c / A.nv, iv = c - iu * A.nv;
  const int n = A.n;
  const int64_t step = A.toward > 0 ? A.plane_stride : -A.plane_stride;
  const int64_t first = iu * A.row_stride + iv + (A.toward > 0 ? 0 : (int64_t)(n - 1) * A.plane_stride);
  const int p0 = A.toward > 0 ? 0 : n - 1, dp = A.toward > 0 ? 1 : -1;
  double I[NB], tau[NB], alp[NB], Sp[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    I[k] = A.back ? A.back[k * A.ncol + c] : 0.0;
    tau[k] = 0.0;
  }
  double ne0, Te0, Z0, ne1, Te1, Z1, ne2, Te2, Z2;
  load_node<T, HAS_TE, HAS_Z, NB>(A, first, ne0, Te0, Z0);
  load_node<T, HAS_TE, HAS_Z, NB>(A, first + step, ne1, Te1, Z1);  // a field has at least 2 planes
  load_node<T, HAS_TE, HAS_Z, NB>(A, first + (n > 2 ? 2 : 1) * step, ne2, Te2, Z2);
  node<NB>(A, ne0, Te0, Z0, alp, Sp);
  double gp = A.g[p0];
  for (int m = 1; m < n; ++m) {
    const double ne = ne1, Te = Te1, Z = Z1;
    ne1 = ne2, Te1 = Te2, Z1 = Z2;
    // the plane two steps ahead (the last plane again where there is none): in flight during this plane's arithmetic
    load_node<T, HAS_TE, HAS_Z, NB>(A, first + (int64_t)(m + 2 < n ? m + 2 : n - 1) * step, ne2, Te2, Z2);
    double al[NB], S[NB], a[NB], b[NB], dt[NB];
    node<NB>(A, ne, Te, Z, al, S);
    const double g = A.g[p0 + m * dp];
    cell<NB>(fabs(g - gp), alp, Sp, al, S, a, b, dt);
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      I[k] = I[k] * a[k] + b[k];
      tau[k] = tau[k] + dt[k];
      alp[k] = al[k];
      Sp[k] = S[k];
    }
    gp = g;
  }
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    A.I[k * A.ncol + c] = I[k];
    A.tau[k * A.ncol + c] = tau[k];
  }
}

template <typename T>
void launch(const EmArgs &A, int axis, bool has_te, bool has_z, int n_band, hipStream_t st) {
  sr::with_flags(
      [&](auto te, auto z) {
        sr::with_count<SR_MAX_BANDS>(
            [&](auto nb) {
              constexpr bool kTe = decltype(te)::value, kZ = decltype(z)::value;
              constexpr int kNb = decltype(nb)::value;
              if (axis == 2) {
                // one wavefront per column, 4 to a workgroup; at most 8 workgroups per CU, the remaining columns by grid stride
                const unsigned grid = (unsigned)std::min<int64_t>((A.ncol + 3) / 4, (int64_t)sr::ctx().n_cu * 8);
                hipLaunchKernelGGL((k_emission_z<T, kTe, kZ, kNb>), dim3(grid), dim3(256), 0, st, A);
              } else {
                hipLaunchKernelGGL((k_emission_xy<T, kTe, kZ, kNb>), dim3(sr::grid_for(A.ncol, 64)), dim3(64), 0, st, A);
              }
            },
            n_band);
      },
      has_te, has_z);
}

}  // namespace

extern "C" int sr_field_emission(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_params *p,
                                 const double *backlight, double *I, double *tau, double *kernel_ms) {
  SR_CHECK(p != nullptr && I != nullptr && tau != nullptr, "sr_field_emission: NULL argument");
  SR_CHECK(p->n_band >= 1 && p->n_band <= SR_MAX_BANDS, "sr_field_emission: n_band must be 1..%d, got %d", SR_MAX_BANDS, p->n_band);
  for (int b = 0; b < p->n_band; ++b) {
    SR_CHECK(std::isfinite(p->omega[b]) && p->omega[b] > 0.0, "sr_field_emission: omega of band %d must be finite and positive", b);
    SR_CHECK(std::isfinite(p->e_ph[b]) && std::isfinite(p->c_omega[b]), "sr_field_emission: non-finite e_ph or c_omega of band %d", b);
  }
  SR_CHECK(p->toward == 1 || p->toward == -1, "sr_field_emission: toward must be +1 or -1, got %d", p->toward);
  SR_CHECK(p->axis >= 0 && p->axis <= 2, "sr_field_emission: axis must be 0, 1 or 2, got %d", p->axis);
  SR_CHECK(ne != nullptr, "sr_field_emission: NULL ne field");
  const sr_field *all[3] = {ne, Te, Z};
  const char *names[3] = {"ne", "Te", "Z"};
  for (int f = 0; f < 3; ++f) {
    if (!all[f]) continue;
    SR_CHECK(all[f]->n_comp == 1, "sr_field_emission: %s is a vector field", names[f]);
    SR_CHECK(all[f]->is_f64 == ne->is_f64, "sr_field_emission: %s and ne differ in dtype", names[f]);
    for (int k = 0; k < 3; ++k)
      SR_CHECK(all[f]->n[k] == ne->n[k] && memcmp(all[f]->hg[k].data(), ne->hg[k].data(), sizeof(double) * ne->n[k]) == 0,
               "sr_field_emission: the grids of %s and ne differ on axis %d", names[f], k);
  }
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;
  const int axis = p->axis, nb = p->n_band;
  const int64_t nx = ne->n[0], ny = ne->n[1], nz = ne->n[2];
  const int64_t ncol = nx * ny * nz / ne->n[axis];
  const size_t map_bytes = sizeof(double) * (size_t)nb * (size_t)ncol;
  double *block = static_cast<double *>(sr::scratch(map_bytes * (backlight ? 3 : 2)));
  if (!block) return SR_ERR_HIP;

  EmArgs A{};
  A.ne = ne->data;
  A.Te = Te ? Te->data : nullptr;
  A.Z = Z ? Z->data : nullptr;
  A.g = ne->g[axis];
  A.I = block;
  A.tau = block + (size_t)nb * ncol;
  A.back = backlight ? block + 2 * (size_t)nb * ncol : nullptr;
  A.n = ne->n[axis];
  A.toward = p->toward;
  A.ncol = ncol;
  A.nv = axis == 0 ? ncol : nz;       // x: the (y, z) plane is one contiguous run; y: rows of nz, one per ix
  A.row_stride = axis == 0 ? 0 : ny * nz;
  A.plane_stride = axis == 0 ? ny * nz : nz;
  for (int b = 0; b < nb; ++b) {
    A.omega[b] = p->omega[b];
    A.e_ph[b] = p->e_ph[b];
    A.c_omega[b] = p->c_omega[b];
  }
  A.uTe = p->Te;
  A.uZ = p->Z;
  if (backlight) SR_HIP(hipMemcpyAsync(const_cast<double *>(A.back), backlight, map_bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipEventRecord(c.ev[0], st));
  if (ne->is_f64)
    launch<double>(A, axis, Te != nullptr, Z != nullptr, nb, st);
  else
    launch<float>(A, axis, Te != nullptr, Z != nullptr, nb, st);
  SR_HIP(hipGetLastError());
  SR_HIP(hipEventRecord(c.ev[1], st));
  SR_HIP(hipMemcpyAsync(I, A.I, map_bytes, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(tau, A.tau, map_bytes, hipMemcpyDeviceToHost, st));
  SR_HIP(hipStreamSynchronize(st));
  if (kernel_ms) {
    float ms = 0.f;
    SR_HIP(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    *kernel_ms = ms;
  }
  sr::scratch_trim();
  return SR_OK;
}
