// The march of the self-emission images, shared by emission.hip (sr_field_emission: the NRL node) and emission_table.hip
// (sr_field_emission_table: the tabulated node); include/synthray.h states the rule every node, cell and column follows.  The two
// sightline units take EmArgs, the NRL policy and, of the host section at the end, check_bands and fill_fields.
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
// toward = -1 walks the same addresses backwards.  No atomics: a repeated call returns identical bits.
//
// What alpha and S of a node are is a POLICY P, the kernels' last template argument:
//   typename P::Args                    what the host hands it, the kernels' second argument
//   P::kXYBlock                         the workgroup size of k_emission_xy
//   __device__ P(const Args &)          run by every thread of the workgroup before any leaves (it may stage into LDS and wait)
//   template <int NB> void eval(A, ne, Te, Z, al, S) const     alpha [1/m] and S of one node for the NB bands
#include <algorithm>
#include <cmath>

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

#include "nrl_node.inc"  // nmax and the NRL node (shared with wave.hip)

// the NRL node as a policy (emission.hip, sightlines.hip); the tabulated one is table_node.inc
struct NrlNode {
  struct Args {};
  static constexpr int kXYBlock = 64;
  __device__ __forceinline__ explicit NrlNode(const Args &) {}
  template <int NB>
  __device__ __forceinline__ void eval(const EmArgs &A, double ne, double Te, double Z, double (&al)[NB], double (&S)[NB]) const {
    const NodeTerms t = node_terms(ne, Te, Z);
#pragma unroll
    for (int b = 0; b < NB; ++b) node_band(t, A.omega[b], A.e_ph[b], A.c_omega[b], al[b], S[b]);
  }
};

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

template <typename T, bool HAS_TE, bool HAS_Z, int NB, typename P>
__global__ void __launch_bounds__(256) k_emission_z(EmArgs A, typename P::Args X) {
  const P node(X);
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
        node.template eval<NB>(A, ne, Te, Z, al, S);
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

template <typename T, bool HAS_TE, bool HAS_Z, int NB, typename P>
__global__ void __launch_bounds__(P::kXYBlock) k_emission_xy(EmArgs A, typename P::Args X) {
  const P node(X);
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
  node.template eval<NB>(A, ne0, Te0, Z0, alp, Sp);
  double gp = A.g[p0];
  for (int m = 1; m < n; ++m) {
    const double ne = ne1, Te = Te1, Z = Z1;
    ne1 = ne2, Te1 = Te2, Z1 = Z2;
    // the plane two steps ahead (the last plane again where there is none): in flight during this plane's arithmetic
    load_node<T, HAS_TE, HAS_Z, NB>(A, first + (int64_t)(m + 2 < n ? m + 2 : n - 1) * step, ne2, Te2, Z2);
    double al[NB], S[NB], a[NB], b[NB], dt[NB];
    node.template eval<NB>(A, ne, Te, Z, al, S);
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

// One instantiation per (dtype, Te field?, Z field?, bands); lds_bytes: the dynamic LDS the policy's constructor fills.
template <typename T, typename P>
void launch(const EmArgs &A, const typename P::Args &X, size_t lds_bytes, int axis, bool has_te, bool has_z, int n_band,
            hipStream_t st) {
  sr::with_flags(
      [&](auto te, auto z) {
        sr::with_count<SR_MAX_BANDS>(
            [&](auto nb) {
              constexpr bool kTe = decltype(te)::value, kZ = decltype(z)::value;
              constexpr int kNb = decltype(nb)::value;
              if (axis == 2) {
                // one wavefront per column, 4 to a workgroup; at most 8 workgroups per CU, the remaining columns by grid stride
                const unsigned grid = sr::capped_grid((A.ncol + 3) / 4, 8);
                hipLaunchKernelGGL((k_emission_z<T, kTe, kZ, kNb, P>), dim3(grid), dim3(256), lds_bytes, st, A, X);
              } else {
                hipLaunchKernelGGL((k_emission_xy<T, kTe, kZ, kNb, P>), dim3(sr::grid_for(A.ncol, P::kXYBlock)), dim3(P::kXYBlock),
                                   lds_bytes, st, A, X);
              }
            },
            n_band);
      },
      has_te, has_z);
}

// ---- host: what the entries share; `who` names the entry in the error text, every check runs before the device is touched.

// The per-band constants of all four entries: n of them, 1..max; `what` is "band" or "frequency" (n_band, n_freq: its first four
// letters).  omega is NULL where a table gives alpha and omega is not read.
inline int check_bands(const char *who, const char *what, int n, int max, const double *omega, const double *e_ph,
                       const double *c_omega) {
  SR_CHECK(n >= 1 && n <= max, "%s: n_%.4s must be 1..%d, got %d", who, what, max, n);
  for (int b = 0; b < n; ++b) {
    SR_CHECK(!omega || (std::isfinite(omega[b]) && omega[b] > 0.0), "%s: omega of %s %d must be finite and positive", who, what, b);
    SR_CHECK(std::isfinite(e_ph[b]) && std::isfinite(c_omega[b]), "%s: non-finite e_ph or c_omega of %s %d", who, what, b);
  }
  return SR_OK;
}

// The checks the two grid marches share.
inline int check_fields(const char *who, const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_params *p) {
  SR_CHECK(p->toward == 1 || p->toward == -1, "%s: toward must be +1 or -1, got %d", who, p->toward);
  SR_CHECK(p->axis >= 0 && p->axis <= 2, "%s: axis must be 0, 1 or 2, got %d", who, p->axis);
  SR_CHECK(ne != nullptr, "%s: NULL ne field", who);
  return sr::check_fields(who, ne, "ne", {{"ne", ne, 1}, {"Te", Te, 1}, {"Z", Z, 1}});
}

// The field half of EmArgs (the grid marches and both sightline entries); n_band = 0 where the frequencies' constants live elsewhere.
inline void fill_fields(EmArgs &A, const sr_field *ne, const sr_field *Te, const sr_field *Z, int toward, double uTe, double uZ,
                        int n_band, const double *omega, const double *e_ph, const double *c_omega) {
  A.ne = ne->data;
  A.Te = Te ? Te->data : nullptr;
  A.Z = Z ? Z->data : nullptr;
  A.toward = toward;
  for (int b = 0; b < n_band; ++b) {
    A.omega[b] = omega[b];
    A.e_ph[b] = e_ph[b];
    A.c_omega[b] = c_omega[b];
  }
  A.uTe = uTe;
  A.uZ = uZ;
}

// Scratch for the maps (+ `extra` bytes behind them: *extra_at), the kernel's arguments, the backlight's upload.
inline int prepare(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_params *p, const double *backlight,
                   size_t extra, EmArgs &A, size_t &map_bytes, char **extra_at) {
  sr::Context &c = sr::ctx();
  const int axis = p->axis, nb = p->n_band;
  const int64_t ny = ne->n[1], nz = ne->n[2];
  const int64_t ncol = (int64_t)ne->n[0] * ny * nz / ne->n[axis];
  map_bytes = sizeof(double) * (size_t)nb * (size_t)ncol;
  A = EmArgs{};
  char *behind;
  sr::Carve carve;
  carve.take(&A.I, (size_t)nb * ncol);
  carve.take(&A.tau, (size_t)nb * ncol);
  if (backlight) carve.take(&A.back, (size_t)nb * ncol);
  carve.take(extra_at ? extra_at : &behind, extra);
  if (!carve.alloc()) return SR_ERR_HIP;
  fill_fields(A, ne, Te, Z, p->toward, p->Te, p->Z, nb, p->omega, p->e_ph, p->c_omega);
  A.g = ne->g[axis];
  A.n = ne->n[axis];
  A.ncol = ncol;
  A.nv = axis == 0 ? ncol : nz;       // x: the (y, z) plane is one contiguous run; y: rows of nz, one per ix
  A.row_stride = axis == 0 ? 0 : ny * nz;
  A.plane_stride = axis == 0 ? ny * nz : nz;
  if (backlight) SR_HIP(hipMemcpyAsync(const_cast<double *>(A.back), backlight, map_bytes, hipMemcpyHostToDevice, c.stream));
  return SR_OK;
}

// After the launch: the maps come back, the kernel's time is read.
inline int finish(const EmArgs &A, size_t map_bytes, double *I, double *tau, double *kernel_ms) {
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;
  SR_HIP(hipGetLastError());
  SR_HIP(hipEventRecord(c.ev[1], st));
  SR_HIP(hipMemcpyAsync(I, A.I, map_bytes, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(tau, A.tau, map_bytes, hipMemcpyDeviceToHost, st));
  return sr::finish_timed(c, kernel_ms);
}

}  // namespace
