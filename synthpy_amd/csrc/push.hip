// Proton radiography: independent charged particles pushed through prescribed E and B fields (sr_particles_push; include/synthray.h
// states the rule every particle follows, operation for operation).  No reference counterpart.
//
// One particle per lane, 256-lane workgroups, the state (x, u, the step count and the last sqrt) in registers for the whole loop; no
// LDS, no scratch, no atomics.  k_push is instantiated per (E given, B given, float32 / float64 source), so an absent field costs no
// gather and none of its arithmetic.  A step's only memory traffic is the trilinear gather at the midpoint: per field four corner
// ROWS of 2 nodes x 3 components, contiguous in the (nx, ny, nz, 3) layout (48 B in float64, 24 B in float32), each read as one run.
// Lanes that have left the box idle until their wavefront ends (tools/push_rate.py measures how many lane-steps that is).
// Compiled with -ffp-contract=off: products and sums round separately, as the NumPy restatement's do (tests/test_radiography.py).
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace {

struct PushArgs {
  const void *E, *B;   // (nx, ny, nz, 3), or nullptr
  sr::FieldGrid f;     // lo, hi: the box
  double hq, hd, ic2, det_pos, hit_scale;
  int max_steps, axis;
  int64_t np;
  const double *s0;  // (6, np)
  double *sf;        // (6, np)
  double *hits;      // (2, np)
  int32_t *steps;
  uint8_t *flags;
};

#include "push_blend.inc"  // Row, blend, norm2

template <bool HAS_E, bool HAS_B, typename T>
__global__ void __launch_bounds__(256) k_push(PushArgs A) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= A.np) return;
  const int64_t N = A.np;
  double x0 = A.s0[i], x1 = A.s0[N + i], x2 = A.s0[2 * N + i];
  double u0 = A.s0[3 * N + i], u1 = A.s0[4 * N + i], u2 = A.s0[5 * N + i];
  const T *__restrict__ fE = static_cast<const T *>(A.E);
  const T *__restrict__ fB = static_cast<const T *>(A.B);
  const int64_t sy = (int64_t)A.f.n[2] * 3, sx = (int64_t)A.f.n[1] * sy;
  const double hq = A.hq, hd = A.hd, ic2 = A.ic2;
  int steps = 0;
  bool inside;
  double g = sqrt(1.0 + norm2(u0, u1, u2) * ic2);
  do {
    const double d = hd / g;
    const double m0 = x0 + u0 * d, m1 = x1 + u1 * d, m2 = x2 + u2 * d;
    double E[3] = {0.0, 0.0, 0.0}, B[3] = {0.0, 0.0, 0.0};
    int ci = 0, cj = 0, ck = 0;
    double wx = 0, wy = 0, wz = 0;
    const bool in_x = sr::locate_in<true>(A.f.g[0], A.f.n[0], A.f.inv_h[0], A.f.lo[0], A.f.hi[0], m0, ci, wx);
    const bool in_y = sr::locate_in<true>(A.f.g[1], A.f.n[1], A.f.inv_h[1], A.f.lo[1], A.f.hi[1], m1, cj, wy);
    const bool in_z = sr::locate_in<true>(A.f.g[2], A.f.n[2], A.f.inv_h[2], A.f.lo[2], A.f.hi[2], m2, ck, wz);
    if (in_x && in_y && in_z) {
      const double ux = 1.0 - wx, uy = 1.0 - wy, uz = 1.0 - wz;
      const double w00 = uy * uz, w01 = uy * wz, w10 = wy * uz, w11 = wy * wz;
      if (HAS_E) blend<T>(fE, sx, sy, ci, cj, ck, ux, wx, w00, w01, w10, w11, E);
      if (HAS_B) blend<T>(fB, sx, sy, ci, cj, ck, ux, wx, w00, w01, w10, w11, B);
    }
    double p0 = u0, p1 = u1, p2 = u2;  // um, then up
    if (HAS_E) {
      p0 = u0 + hq * E[0];
      p1 = u1 + hq * E[1];
      p2 = u2 + hq * E[2];
    }
    if (HAS_B) {
      const double gm = sqrt(1.0 + norm2(p0, p1, p2) * ic2);
      const double k = hq / gm;
      const double t0 = k * B[0], t1 = k * B[1], t2 = k * B[2];
      const double f = 2.0 / (1.0 + norm2(t0, t1, t2));
      const double s0 = t0 * f, s1 = t1 * f, s2 = t2 * f;
      const double w0 = p0 + (p1 * t2 - p2 * t1), w1 = p1 + (p2 * t0 - p0 * t2), w2 = p2 + (p0 * t1 - p1 * t0);
      p0 = p0 + (w1 * s2 - w2 * s1);
      p1 = p1 + (w2 * s0 - w0 * s2);
      p2 = p2 + (w0 * s1 - w1 * s0);
    }
    if (HAS_E) {
      u0 = p0 + hq * E[0];
      u1 = p1 + hq * E[1];
      u2 = p2 + hq * E[2];
    } else {
      u0 = p0;
      u1 = p1;
      u2 = p2;
    }
    g = sqrt(1.0 + norm2(u0, u1, u2) * ic2);  // gn: this step's second half drift, and the next step's g (same inputs, same operations)
    const double dn = hd / g;
    x0 = m0 + u0 * dn;
    x1 = m1 + u1 * dn;
    x2 = m2 + u2 * dn;
    ++steps;
    inside = x0 >= A.f.lo[0] && x0 <= A.f.hi[0] && x1 >= A.f.lo[1] && x1 <= A.f.hi[1] && x2 >= A.f.lo[2] && x2 <= A.f.hi[2];
  } while (inside && steps < A.max_steps);

  // the detector plane: coordinate[axis] == det_pos; (b, c) the two other axes in x < y < z order
  const int a = A.axis;
  const double xa = a == 0 ? x0 : (a == 1 ? x1 : x2), ua = a == 0 ? u0 : (a == 1 ? u1 : u2);
  const double xb = a == 0 ? x1 : x0, ub = a == 0 ? u1 : u0;
  const double xc = a == 2 ? x1 : x2, uc = a == 2 ? u1 : u2;
  const double tau = (A.det_pos - xa) / ua;
  const bool reaches = tau > 0.0 && tau <= 1.7976931348623157e308;  // finite and positive (a NaN fails both)
  A.sf[i] = x0;
  A.sf[N + i] = x1;
  A.sf[2 * N + i] = x2;
  A.sf[3 * N + i] = u0;
  A.sf[4 * N + i] = u1;
  A.sf[5 * N + i] = u2;
  A.hits[i] = (xb + ub * tau) * A.hit_scale;
  A.hits[N + i] = (xc + uc * tau) * A.hit_scale;
  A.steps[i] = steps;
  A.flags[i] = (uint8_t)((inside ? SR_PUSH_UNFINISHED : 0) | (reaches ? 0 : SR_PUSH_MISSED));
}

// [0] UNFINISHED, [1] MISSED over the flags of a call: a grid-stride count, one atomic per wavefront of a bounded grid
__global__ void __launch_bounds__(256) k_push_flags(const uint8_t *__restrict__ flags, int64_t n, unsigned long long *__restrict__ out) {
  unsigned long long unfinished = 0ull, missed = 0ull;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned f = flags[i];
    unfinished += (f & SR_PUSH_UNFINISHED) ? 1u : 0u;
    missed += (f & SR_PUSH_MISSED) ? 1u : 0u;
  }
  for (int off = 32; off > 0; off >>= 1) {
    unfinished += __shfl_down(unfinished, off, 64);
    missed += __shfl_down(missed, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (unfinished) atomicAdd(&out[0], unfinished);
    if (missed) atomicAdd(&out[1], missed);
  }
}

template <typename T>
void launch(bool has_e, bool has_b, unsigned grid, hipStream_t st, const PushArgs &A) {
  sr::with_flags(
      [&](auto e, auto b) {
        if constexpr (e.value || b.value) hipLaunchKernelGGL((k_push<e.value, b.value, T>), dim3(grid), dim3(256), 0, st, A);
      },
      has_e, has_b);
}

}  // namespace

extern "C" int sr_particles_push(const sr_field *E, const sr_field *B, const sr_push_params *p, int64_t n, const double *s0,
                                 double *sf, double *hits, int32_t *steps, uint8_t *flags, sr_image *img, sr_push_stats *stats) {
  SR_CHECK(p != nullptr && s0 != nullptr, "sr_particles_push: NULL argument (p or s0)");
  SR_CHECK(n >= 0, "sr_particles_push: n must not be negative, got %lld", (long long)n);
  SR_CHECK(std::isfinite(p->dt) && p->dt > 0.0, "sr_particles_push: dt must be finite and positive");
  SR_CHECK(std::isfinite(p->qm), "sr_particles_push: non-finite qm");
  SR_CHECK(std::isfinite(p->det_pos), "sr_particles_push: non-finite det_pos");
  SR_CHECK(std::isfinite(p->hit_scale), "sr_particles_push: non-finite hit_scale");
  SR_CHECK(p->max_steps >= 1, "sr_particles_push: max_steps must be at least 1, got %d", p->max_steps);
  SR_CHECK(p->axis >= 0 && p->axis <= 2, "sr_particles_push: axis must be 0, 1 or 2, got %d", p->axis);
  SR_CHECK(img == nullptr || img->kind == SR_IMG_COUNTS, "sr_particles_push: the image must be of kind SR_IMG_COUNTS");
  SR_CHECK(E != nullptr || B != nullptr, "sr_particles_push: E and B are both NULL");
  const sr_field *F = E ? E : B;
  if (int rc = sr::check_fields("sr_particles_push", F, E ? "E" : "B", {{"E", E, 3}, {"B", B, 3}})) return rc;
  if (stats) *stats = sr_push_stats{0.0, 0, 0, 0, 0};
  if (n == 0) return SR_OK;
  if (int rc = sr::ensure_init()) return rc;
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;

  // one scratch block: s0 | sf | hits | steps | flags | counters {unfinished, missed, deposited}
  PushArgs A{};
  unsigned long long *counters = nullptr;
  sr::Carve carve;
  carve.take(&A.s0, 6 * (size_t)n);
  carve.take(&A.sf, 6 * (size_t)n);
  carve.take(&A.hits, 2 * (size_t)n);
  carve.take(&A.steps, (size_t)n);
  carve.take(&A.flags, (size_t)n);
  carve.take(&counters, 3);
  if (!carve.alloc()) return SR_ERR_HIP;
  A.E = E ? E->data : nullptr;
  A.B = B ? B->data : nullptr;
  A.f = sr::grid_of(F);
  A.hq = (p->qm * p->dt) * 0.5;
  A.hd = p->dt * 0.5;
  A.ic2 = 1.0 / (sr::kC * sr::kC);
  A.det_pos = p->det_pos;
  A.hit_scale = p->hit_scale;
  A.max_steps = p->max_steps;
  A.axis = p->axis;
  A.np = n;

  if (int rc = sr::upload_sync(const_cast<double *>(A.s0), s0, sizeof(double) * 6 * (size_t)n, st)) return rc;
  SR_HIP(hipMemsetAsync(counters, 0, 3 * sizeof(unsigned long long), st));
  SR_HIP(hipEventRecord(c.ev[0], st));
  if (F->is_f64)
    launch<double>(E != nullptr, B != nullptr, sr::grid_for(n, 256), st, A);
  else
    launch<float>(E != nullptr, B != nullptr, sr::grid_for(n, 256), st, A);
  SR_HIP(hipGetLastError());
  SR_HIP(hipEventRecord(c.ev[1], st));
  if (stats) {
    hipLaunchKernelGGL(k_push_flags, dim3(std::min<unsigned>(sr::grid_for(n, 256), 1024u)), dim3(256), 0, st, A.flags, n, counters);
    SR_HIP(hipGetLastError());
  }
  if (img)
    if (int rc = sr::counts_deposit_device(A.hits, A.hits + n, A.flags, n, img, counters + 2, st)) return rc;
  if (sf) SR_HIP(hipMemcpyAsync(sf, A.sf, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost, st));
  if (hits) SR_HIP(hipMemcpyAsync(hits, A.hits, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
  if (steps) SR_HIP(hipMemcpyAsync(steps, A.steps, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
  if (flags) SR_HIP(hipMemcpyAsync(flags, A.flags, (size_t)n, hipMemcpyDeviceToHost, st));
  unsigned long long hc[3] = {0, 0, 0};
  if (stats) SR_HIP(hipMemcpyAsync(hc, counters, sizeof(hc), hipMemcpyDeviceToHost, st));
  if (int rc = sr::finish_timed(c, stats ? &stats->kernel_ms : nullptr)) return rc;
  if (stats) {
    stats->unfinished = (int64_t)hc[0];
    stats->finished = n - (int64_t)hc[0];
    stats->missed = (int64_t)hc[1];
    stats->deposited = (int64_t)hc[2];
  }
  return SR_OK;
}
