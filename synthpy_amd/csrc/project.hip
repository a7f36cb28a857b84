// Line integrals of a volume along its probing axis: sr_volume_project (include/synthray.h, SR_PROJ_*).
//
// The packed node order (common.hpp, sr::node_index) is the order this sum wants: inside an octet of node planes the lateral
// columns are contiguous and one column's eight planes are one 128-byte line of float4 records.  Lane l of a wavefront takes plane
// l & 7 of column (l >> 3) of its group of eight columns: the 64 lanes read 1024 consecutive bytes of P (256 of L, 512 of K,
// 2048 of Q), every record exactly once, and walk from octet to octet with a stride of nb*nc records.  Each lane keeps its own
// float64 partial sums over the octets (its plane's trapezoid weight times its node's value); the eight lanes of a column are
// then added by one fixed xor tree and lane 0 of the column stores.  No atomics: a repeated call returns identical bits.
// The weights of the pad planes of the last octet are zero (and the records there are zero: volume.hip clears them).
// Compiled with -ffp-contract=off: products and sums round separately.
#include "common.hpp"

namespace {

struct ProjArgs {
  const float4 *P;
  const float *L;
  const double4 *Q;
  const double *K;
  const double *w;  // n_oct * 8 trapezoid weights, 0 for the pad planes
  double *maps;     // (SR_PROJ_MAPS, n_u, n_v)
  int64_t ncol;     // nb * nc
  int n_oct, nb, nc;
  int axis;         // physical index of the probing axis: picks B_a, and for y the (z, x) -> (x, z) transposition
  double ne_scale;  // omega^2 * 1e6 / 5.64e4^2
};

__device__ __forceinline__ double column_sum(double v) {
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 1, 64);
  return v;
}

template <bool PHASE, bool KAPPA, bool FARADAY>
__global__ void __launch_bounds__(256) k_project(ProjArgs A) {
  const int plane = threadIdx.x & 7;
  const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
  const int64_t step = ((int64_t)gridDim.x * blockDim.x) >> 3;
  // the eight lanes of a column share `col`: they enter and leave the loop together, so the xor partners are always live
  for (int64_t col = first; col < A.ncol; col += step) {
    double s_b = 0.0, s_c = 0.0, s_m = 0.0, s_ne = 0.0, s_k = 0.0, s_neb = 0.0;
    int64_t q = col * 8 + plane;
#pragma unroll 4
    for (int o = 0; o < A.n_oct; ++o, q += A.ncol * 8) {
      const double w = A.w[o * 8 + plane];
      const float4 p = A.P[q];
      s_b += w * (double)p.x;
      s_c += w * (double)p.y;
      if (PHASE) {
        const double m = (double)p.w + (double)A.L[q];
        s_m += w * m;
        s_ne += w * (-(m * (2.0 + m)) * A.ne_scale);
      }
      if (KAPPA) s_k += w * A.K[q];
      if (FARADAY) {
        const double4 r = A.Q[q];
        const double B_a = A.axis == 0 ? r.y : (A.axis == 1 ? r.z : r.w);
        s_neb += w * (r.x * B_a);
      }
    }
    s_b = column_sum(s_b);
    s_c = column_sum(s_c);
    if (PHASE) {
      s_m = column_sum(s_m);
      s_ne = column_sum(s_ne);
    }
    if (KAPPA) s_k = column_sum(s_k);
    if (FARADAY) s_neb = column_sum(s_neb);
    if (plane == 0) {
      // device lateral order (b, c) = ((a+1)%3, (a+2)%3): (y, z), (z, x), (x, y); the maps are (u, v) in x < y < z order
      const int64_t ib = col / A.nc, ic = col - ib * A.nc;
      const bool swap = A.axis == 1;
      const int64_t pix = swap ? ic * A.nb + ib : col;
      A.maps[(int64_t)SR_PROJ_GRAD1 * A.ncol + pix] = swap ? s_c : s_b;
      A.maps[(int64_t)SR_PROJ_GRAD2 * A.ncol + pix] = swap ? s_b : s_c;
      A.maps[(int64_t)SR_PROJ_NM1 * A.ncol + pix] = s_m;
      A.maps[(int64_t)SR_PROJ_NE * A.ncol + pix] = s_ne;
      A.maps[(int64_t)SR_PROJ_KAPPA * A.ncol + pix] = s_k;
      A.maps[(int64_t)SR_PROJ_NEB * A.ncol + pix] = s_neb;
    }
  }
}

}  // namespace

extern "C" {

int sr_volume_project(const sr_volume *v, double *maps, uint32_t *have) {
  SR_CHECK(v != nullptr && maps != nullptr, "sr_volume_project: NULL argument");
  SR_CHECK(v->na >= 2 && (int)v->hg[0].size() == v->na, "sr_volume_project: the trapezoid rule needs at least 2 node planes, the volume has %d", v->na);
  hipStream_t st = sr::ctx().stream;
  const int n_oct = (v->na + 7) / 8;
  const int64_t ncol = (int64_t)v->nb * v->nc;
  // trapezoid weights on the volume's own float64 node coordinates of the probing axis (a slab: its own planes)
  const std::vector<double> &g = v->hg[0];
  std::vector<double> w((size_t)n_oct * 8, 0.0);
  const int n = v->na;
  w[0] = (g[1] - g[0]) / 2;
  for (int k = 1; k + 1 < n; ++k) w[k] = (g[k + 1] - g[k - 1]) / 2;
  w[n - 1] = (g[n - 1] - g[n - 2]) / 2;

  const size_t map_bytes = sizeof(double) * (size_t)SR_PROJ_MAPS * (size_t)ncol;
  char *block = static_cast<char *>(sr::scratch(map_bytes + sizeof(double) * w.size()));
  if (!block) return SR_ERR_HIP;
  ProjArgs A{};
  A.P = v->P;
  A.L = v->L;
  A.K = v->K;
  A.Q = reinterpret_cast<const double4 *>(v->Q);
  A.maps = reinterpret_cast<double *>(block);
  double *d_w = reinterpret_cast<double *>(block + map_bytes);
  A.w = d_w;
  A.ncol = ncol;
  A.n_oct = n_oct;
  A.nb = v->nb;
  A.nc = v->nc;
  A.axis = v->axis;
  A.ne_scale = (v->omega * v->omega) * 1e6 / (5.64e4 * 5.64e4);
  SR_HIP(hipMemcpyAsync(d_w, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, st));
  // memory-bound: at most 8 blocks of 256 threads per CU, the remaining column groups by grid stride
  const int block_threads = 256;
  const unsigned grid = sr::capped_grid((ncol * 8 + block_threads - 1) / block_threads, 8);
  const bool ph = v->L != nullptr, ka = v->K != nullptr, fa = v->Q != nullptr;
#define SR_PROJ_LAUNCH(PH, KA, FA) hipLaunchKernelGGL((k_project<PH, KA, FA>), dim3(grid), dim3(block_threads), 0, st, A)
  switch ((ph ? 1 : 0) | (ka ? 2 : 0) | (fa ? 4 : 0)) {
    case 0: SR_PROJ_LAUNCH(false, false, false); break;
    case 1: SR_PROJ_LAUNCH(true, false, false); break;
    case 2: SR_PROJ_LAUNCH(false, true, false); break;
    case 3: SR_PROJ_LAUNCH(true, true, false); break;
    case 4: SR_PROJ_LAUNCH(false, false, true); break;
    case 5: SR_PROJ_LAUNCH(true, false, true); break;
    case 6: SR_PROJ_LAUNCH(false, true, true); break;
    default: SR_PROJ_LAUNCH(true, true, true); break;
  }
#undef SR_PROJ_LAUNCH
  SR_HIP(hipGetLastError());
  SR_HIP(hipMemcpyAsync(maps, A.maps, map_bytes, hipMemcpyDeviceToHost, st));
  SR_HIP(hipStreamSynchronize(st));
  sr::scratch_trim();
  if (have)
    *have = (1u << SR_PROJ_GRAD1) | (1u << SR_PROJ_GRAD2) | (ph ? (1u << SR_PROJ_NM1) | (1u << SR_PROJ_NE) : 0u) |
            (ka ? 1u << SR_PROJ_KAPPA : 0u) | (fa ? 1u << SR_PROJ_NEB : 0u);
  return SR_OK;
}

}  // extern "C"
