// Oblique lines of sight: a device-resident source field (sr_field) and its affine, trilinear resample onto another rectilinear
// grid (sr_field_resample; include/synthray.h states the rule each output node follows, operation for operation).
//
// A gather whose access pattern depends on the angle.  One thread per output node, no LDS, no atomics: a workgroup of 256
// threads takes a BRICK of BX x BY x BZ output nodes (z fastest inside it, so a wavefront stores runs of BZ consecutive values),
// whose source footprint is a compact, slanted box at every orientation -- a row of 256 nodes along z would cut through up to
// 256 source lines per corner row.  Bricks are numbered supertile by supertile (4 x 4 x 4 bricks, z fastest inside and between
// them) and the numbering is dealt to the workgroups so that the workgroups that share an XCD's L2 (blockIdx % 8 equal) walk ONE
// contiguous eighth of it, in order: what is resident on an XCD at one time is a few neighbouring supertiles, whose source lines
// overlap.  The brick count per axis is padded to a multiple of 4; a padded brick is skipped by its whole workgroup.
// The brick is to be a measured choice (tools/resample_rate.py sweeps the instantiated ones and writes profiles/resample_rate.txt;
// SYNTHRAY_RESAMPLE_BRICK=BXxBYxBZ picks one for such a measurement): 4 x 4 x 16 is the default until that table exists.
// Compiled with -ffp-contract=off: products and sums round separately, as the NumPy restatement's do (tests/test_resample.py).
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.hpp"

namespace {

constexpr int kSuper = 4;  // bricks per supertile and axis

struct ResampleArgs {
  const void *src;
  void *out;
  const double *g[3];  // source axes
  const double *o[3];  // view axes, float32 coordinates widened to float64
  int n[3], m[3];
  double inv_h[3];
  double M[9], t[3], V[9], fill[3];
  int use_V;
  int nb[3];    // bricks per axis
  int ns[3];    // supertiles per axis
  int64_t nvb;  // ns[0] * ns[1] * ns[2] * kSuper^3: numbered bricks, the padded ones included
};

using sr::locate;  // the cell of p on one source axis (common.hpp)

template <typename T, int NC, int BX, int BY, int BZ>
__global__ void __launch_bounds__(256) k_resample(ResampleArgs A) {
  static_assert(BX * BY * BZ == 256, "a brick is one workgroup of 256 output nodes");
  const T *__restrict__ src = static_cast<const T *>(A.src);
  T *__restrict__ out = static_cast<T *>(A.out);
  const int lz = threadIdx.x % BZ, ly = (threadIdx.x / BZ) % BY, lx = threadIdx.x / (BZ * BY);
  const int64_t sy_stride = (int64_t)A.n[2] * NC, sx_stride = (int64_t)A.n[1] * sy_stride;
  const int64_t per_xcd = A.nvb >> 3;  // nvb is a multiple of 64 and gridDim.x of 8: v % 8 == blockIdx.x % 8 in every round
  for (int64_t v = blockIdx.x; v < A.nvb; v += gridDim.x) {
    const int64_t lin = (v & 7) * per_xcd + (v >> 3);
    const int64_t s = lin >> 6;
    const int wi = (int)(lin & 63);
    const int sz = (int)(s % A.ns[2]), sy = (int)((s / A.ns[2]) % A.ns[1]), sx = (int)(s / ((int64_t)A.ns[2] * A.ns[1]));
    const int bx = sx * kSuper + (wi >> 4), by = sy * kSuper + ((wi >> 2) & 3), bz = sz * kSuper + (wi & 3);
    if (bx >= A.nb[0] || by >= A.nb[1] || bz >= A.nb[2]) continue;
    const int ix = bx * BX + lx, iy = by * BY + ly, iz = bz * BZ + lz;
    if (ix >= A.m[0] || iy >= A.m[1] || iz >= A.m[2]) continue;
    const double q0 = A.o[0][ix], q1 = A.o[1][iy], q2 = A.o[2][iz];
    const double px = ((A.M[0] * q0 + A.M[1] * q1) + A.M[2] * q2) + A.t[0];
    const double py = ((A.M[3] * q0 + A.M[4] * q1) + A.M[5] * q2) + A.t[1];
    const double pz = ((A.M[6] * q0 + A.M[7] * q1) + A.M[8] * q2) + A.t[2];
    int ci = 0, cj = 0, ck = 0;
    double wx = 0, wy = 0, wz = 0;
    const bool in_x = locate(A.g[0], A.n[0], A.inv_h[0], px, ci, wx);
    const bool in_y = locate(A.g[1], A.n[1], A.inv_h[1], py, cj, wy);
    const bool in_z = locate(A.g[2], A.n[2], A.inv_h[2], pz, ck, wz);
    double val[NC];
    if (in_x && in_y && in_z) {
      const double ux = 1.0 - wx, uy = 1.0 - wy, uz = 1.0 - wz;
      const double w00 = uy * uz, w01 = uy * wz, w10 = wy * uz, w11 = wy * wz;
      const T *lo = src + ((int64_t)ci * sx_stride + (int64_t)cj * sy_stride + (int64_t)ck * NC);
      const T *hi = lo + sx_stride;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const double s0 = (((double)lo[c] * w00 + (double)lo[NC + c] * w01) + (double)lo[sy_stride + c] * w10) +
                          (double)lo[sy_stride + NC + c] * w11;
        const double s1 = (((double)hi[c] * w00 + (double)hi[NC + c] * w01) + (double)hi[sy_stride + c] * w10) +
                          (double)hi[sy_stride + NC + c] * w11;
        val[c] = ux * s0 + wx * s1;
      }
      if (NC == 3 && A.use_V) {
        const double b0 = val[0], b1 = val[NC > 1 ? 1 : 0], b2 = val[NC > 2 ? 2 : 0];
#pragma unroll
        for (int c = 0; c < NC; ++c) val[c] = (A.V[3 * c] * b0 + A.V[3 * c + 1] * b1) + A.V[3 * c + 2] * b2;
      }
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c) val[c] = A.fill[c];
    }
    const int64_t node = ((int64_t)ix * A.m[1] + iy) * A.m[2] + iz;
#pragma unroll
    for (int c = 0; c < NC; ++c) out[node * NC + c] = (T)val[c];
  }
}

int check_axis(const char *who, const char *name, const float *x, int n) {
  SR_CHECK(x != nullptr, "%s: %s coordinates are NULL", who, name);
  SR_CHECK(n >= 2, "%s: %s needs at least 2 nodes", who, name);
  for (int i = 0; i + 1 < n; ++i)
    SR_CHECK(x[i + 1] > x[i], "%s: %s coordinates must be strictly ascending (node %d)", who, name, i);
  return SR_OK;
}

struct Brick {
  int bx, by, bz;
};
constexpr Brick kBricks[] = {{4, 4, 16}, {8, 8, 4}, {8, 4, 8}, {2, 8, 16}, {16, 1, 16}, {1, 1, 256}};
constexpr int kDefaultBrick = 0;

int pick_brick() {
  const char *e = getenv("SYNTHRAY_RESAMPLE_BRICK");
  if (e) {
    int a = 0, b = 0, c = 0;
    if (sscanf(e, "%dx%dx%d", &a, &b, &c) == 3)
      for (int k = 0; k < (int)(sizeof(kBricks) / sizeof(kBricks[0])); ++k)
        if (kBricks[k].bx == a && kBricks[k].by == b && kBricks[k].bz == c) return k;
  }
  return kDefaultBrick;
}

template <typename T, int NC>
void launch(int brick, unsigned grid, hipStream_t st, const ResampleArgs &A) {
  switch (brick) {
    case 0: hipLaunchKernelGGL((k_resample<T, NC, 4, 4, 16>), dim3(grid), dim3(256), 0, st, A); break;
    case 1: hipLaunchKernelGGL((k_resample<T, NC, 8, 8, 4>), dim3(grid), dim3(256), 0, st, A); break;
    case 2: hipLaunchKernelGGL((k_resample<T, NC, 8, 4, 8>), dim3(grid), dim3(256), 0, st, A); break;
    case 3: hipLaunchKernelGGL((k_resample<T, NC, 2, 8, 16>), dim3(grid), dim3(256), 0, st, A); break;
    case 4: hipLaunchKernelGGL((k_resample<T, NC, 16, 1, 16>), dim3(grid), dim3(256), 0, st, A); break;
    default: hipLaunchKernelGGL((k_resample<T, NC, 1, 1, 256>), dim3(grid), dim3(256), 0, st, A); break;
  }
}

}  // namespace

extern "C" {

int sr_field_create(sr_field **out, const void *data, int is_f64, int n_comp, int nx, int ny, int nz, const float *x,
                    const float *y, const float *z) {
  SR_CHECK(out != nullptr && data != nullptr, "sr_field_create: NULL argument");
  *out = nullptr;
  SR_CHECK(n_comp == 1 || n_comp == 3, "sr_field_create: n_comp must be 1 or 3, got %d", n_comp);
  const int n[3] = {nx, ny, nz};
  const float *co[3] = {x, y, z};
  const char *names[3] = {"x", "y", "z"};
  for (int k = 0; k < 3; ++k) {
    const int rc = check_axis("sr_field_create", names[k], co[k], n[k]);
    if (rc) return rc;
  }
  int rc = sr::ensure_init();
  if (rc) return rc;
  hipStream_t st = sr::ctx().stream;
  sr_field *f = new sr_field();
  f->n_comp = n_comp;
  f->is_f64 = is_f64 != 0;
  const size_t bytes = (size_t)nx * ny * nz * n_comp * (is_f64 ? sizeof(double) : sizeof(float));
  hipError_t e = sr::dev_alloc_bytes(&f->data, bytes);
  if (e != hipSuccess) {
    f->data = nullptr;
    delete f;
    return sr::fail(SR_ERR_HIP, "sr_field_create: allocating %zu bytes failed: %s", bytes, hipGetErrorString(e));
  }
  rc = sr::upload_sync(f->data, data, bytes, st);
  for (int k = 0; k < 3 && !rc; ++k) {
    f->n[k] = n[k];
    std::vector<double> g(co[k], co[k] + n[k]);
    f->hg[k] = g;
    f->inv_h[k] = (n[k] - 1) / (g[n[k] - 1] - g[0]);
    rc = sr::dev_alloc(&f->g[k], (size_t)n[k]);
    if (!rc) rc = sr::upload_sync(f->g[k], g.data(), sizeof(double) * g.size(), st);
  }
  if (rc) {
    sr_field_destroy(f);
    return rc;
  }
  *out = f;
  return SR_OK;
}

int sr_field_resample(const sr_field *f, const sr_resample_params *p, int mx, int my, int mz, const float *ox,
                      const float *oy, const float *oz, void *out, double *kernel_ms) {
  SR_CHECK(p != nullptr && out != nullptr, "sr_field_resample: NULL argument");
  SR_CHECK(ox != nullptr && oy != nullptr && oz != nullptr, "sr_field_resample: NULL view coordinates");
  SR_CHECK(mx >= 1 && my >= 1 && mz >= 1, "sr_field_resample: the view grid needs at least one node per axis, got %d x %d x %d", mx, my, mz);
  for (int k = 0; k < 9; ++k) {
    SR_CHECK(std::isfinite(p->M[k]), "sr_field_resample: non-finite entry %d of M", k);
    SR_CHECK(!p->use_V || std::isfinite(p->V[k]), "sr_field_resample: non-finite entry %d of V", k);
  }
  for (int k = 0; k < 3; ++k) SR_CHECK(std::isfinite(p->t[k]), "sr_field_resample: non-finite entry %d of t", k);
  SR_CHECK(f != nullptr, "sr_field_resample: NULL field");
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;
  const int m[3] = {mx, my, mz};
  const float *oc[3] = {ox, oy, oz};
  const size_t elem = f->is_f64 ? sizeof(double) : sizeof(float);
  const size_t out_bytes = (size_t)mx * my * mz * f->n_comp * elem;
  std::vector<double> o((size_t)mx + my + mz);
  for (int k = 0, at = 0; k < 3; at += m[k], ++k)
    for (int i = 0; i < m[k]; ++i) o[at + i] = (double)oc[k][i];
  char *block;
  double *d_o;
  sr::Carve carve;
  carve.take(&block, out_bytes);
  carve.take(&d_o, o.size());
  if (!carve.alloc()) return SR_ERR_HIP;

  ResampleArgs A{};
  A.src = f->data;
  A.out = block;
  const int brick = pick_brick();
  const int bdim[3] = {kBricks[brick].bx, kBricks[brick].by, kBricks[brick].bz};
  A.nvb = kSuper * kSuper * kSuper;
  for (int k = 0, at = 0; k < 3; at += m[k], ++k) {
    A.g[k] = f->g[k];
    A.o[k] = d_o + at;
    A.n[k] = f->n[k];
    A.m[k] = m[k];
    A.inv_h[k] = f->inv_h[k];
    A.t[k] = p->t[k];
    A.fill[k] = p->fill[k];
    A.nb[k] = (m[k] + bdim[k] - 1) / bdim[k];
    A.ns[k] = (A.nb[k] + kSuper - 1) / kSuper;
    A.nvb *= A.ns[k];
  }
  memcpy(A.M, p->M, sizeof(A.M));
  memcpy(A.V, p->V, sizeof(A.V));
  A.use_V = f->n_comp == 3 && p->use_V ? 1 : 0;

  SR_HIP(hipMemcpyAsync(d_o, o.data(), sizeof(double) * o.size(), hipMemcpyHostToDevice, st));
  // a gather bound by memory latency: 8 workgroups of 256 threads per CU, the remaining bricks by grid stride (a multiple of 8)
  const unsigned grid = sr::capped_grid(A.nvb, 8);
  SR_HIP(hipEventRecord(c.ev[0], st));
  if (f->is_f64) {
    if (f->n_comp == 3)
      launch<double, 3>(brick, grid, st, A);
    else
      launch<double, 1>(brick, grid, st, A);
  } else {
    if (f->n_comp == 3)
      launch<float, 3>(brick, grid, st, A);
    else
      launch<float, 1>(brick, grid, st, A);
  }
  SR_HIP(hipGetLastError());
  SR_HIP(hipEventRecord(c.ev[1], st));
  SR_HIP(hipMemcpyAsync(out, block, out_bytes, hipMemcpyDeviceToHost, st));
  return sr::finish_timed(c, kernel_ms);
}

int64_t sr_field_bytes(const sr_field *f) {
  if (!f) return 0;
  const int64_t nodes = (int64_t)f->n[0] * f->n[1] * f->n[2];
  return nodes * f->n_comp * (int64_t)(f->is_f64 ? sizeof(double) : sizeof(float)) +
         (int64_t)sizeof(double) * ((int64_t)f->n[0] + f->n[1] + f->n[2]);
}

void sr_field_destroy(sr_field *f) {
  if (!f) return;
  sr::dev_free(f->data);
  for (int k = 0; k < 3; ++k) sr::dev_free(f->g[k]);
  delete f;
}

}  // extern "C"
