// Proton radiography through matter: sr_particles_push's step with collisional stopping (Bethe, free and bound electrons) and the
// Fermi-Eyges moments of the multiple-scattering power along each path (sr_particles_push_matter; include/synthray.h states the
// rule every particle follows, operation for operation).  No reference counterpart.
//
// One particle per lane, 256-lane workgroups; the state, the path length s and the three moments stay in registers for the whole
// loop; no LDS, no scratch, no atomics.  k_push_matter is instantiated per (E given, B given, Z a field or uniform, float32 /
// float64 source).  Beside k_push's vector gathers a step reads ne (and Z) at the same midpoint with the same cell and weights:
// per scalar field four corner ROWS of 2 nodes, contiguous in the (nx, ny, nz) layout (16 B in float64, 8 B in float32), each read
// as one run.  The matter lines sit under one branch: a wavefront whose lanes partly see matter runs them masked, and a lane that
// stops idles like one that has left the box.  Compiled with -ffp-contract=off, as push.hip is; log is the device library's.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace {

#include "push_blend.inc"  // Row, blend, norm2

struct MatterArgs {
  const void *E, *B;    // (nx, ny, nz, 3), or nullptr
  const void *ne, *Z;   // (nx, ny, nz); Z or nullptr
  sr::FieldGrid f;      // lo, hi: the box
  double hq, hd, ic2, det_pos, hit_scale;
  double dt, mass, mc2, A2, HW, I, Zn, Zu, KS, KT, stop_energy;
  int max_steps, axis;
  int64_t np;
  const double *s0;  // (6, np)
  double *sf;        // (6, np)
  double *hits;      // (2, np)
  double *energy;    // (np)
  double *moments;   // (4, np)
  int32_t *steps;
  uint8_t *flags;
};

template <typename T>
struct Row2 {  // one corner row of a scalar field: nodes k, k + 1 of z
  T v[2];
};

// one scalar field at the cell (ci, cj, ck) with the blend of sr_field_resample's rule; sx, sy: the node strides of x and y
template <typename T>
__device__ __forceinline__ double blend1(const T *__restrict__ src, int64_t sx, int64_t sy, int ci, int cj, int ck, double ux, double wx,
                                         double w00, double w01, double w10, double w11) {
  const T *p = src + ((int64_t)ci * sx + (int64_t)cj * sy + (int64_t)ck);
  const Row2<T> a0 = *reinterpret_cast<const Row2<T> *>(p), a1 = *reinterpret_cast<const Row2<T> *>(p + sy);
  const Row2<T> b0 = *reinterpret_cast<const Row2<T> *>(p + sx), b1 = *reinterpret_cast<const Row2<T> *>(p + sx + sy);
  const double s0 = (((double)a0.v[0] * w00 + (double)a0.v[1] * w01) + (double)a1.v[0] * w10) + (double)a1.v[1] * w11;
  const double s1 = (((double)b0.v[0] * w00 + (double)b0.v[1] * w01) + (double)b1.v[0] * w10) + (double)b1.v[1] * w11;
  return ux * s0 + wx * s1;
}

template <bool HAS_E, bool HAS_B, bool HAS_Z, typename T>
__global__ void __launch_bounds__(256) k_push_matter(MatterArgs A) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= A.np) return;
  const int64_t N = A.np;
  double x0 = A.s0[i], x1 = A.s0[N + i], x2 = A.s0[2 * N + i];
  double u0 = A.s0[3 * N + i], u1 = A.s0[4 * N + i], u2 = A.s0[5 * N + i];
  const T *__restrict__ fE = static_cast<const T *>(A.E);
  const T *__restrict__ fB = static_cast<const T *>(A.B);
  const T *__restrict__ fN = static_cast<const T *>(A.ne);
  const T *__restrict__ fZ = static_cast<const T *>(A.Z);
  const int64_t ty = (int64_t)A.f.n[2], tx = (int64_t)A.f.n[1] * ty;  // a scalar field's strides
  const int64_t sy = ty * 3, sx = tx * 3;                             // a vector field's
  const double hq = A.hq, hd = A.hd, ic2 = A.ic2;
  int steps = 0;
  bool inside, stopped = false;
  double s = 0.0, M0 = 0.0, M1 = 0.0, M2 = 0.0;
  double g = sqrt(1.0 + norm2(u0, u1, u2) * ic2);
  do {
    const double d = hd / g;
    const double m0 = x0 + u0 * d, m1 = x1 + u1 * d, m2 = x2 + u2 * d;
    double E[3] = {0.0, 0.0, 0.0}, B[3] = {0.0, 0.0, 0.0};
    double ne = 0.0, Z = HAS_Z ? 0.0 : A.Zu;
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
      ne = blend1<T>(fN, tx, ty, ci, cj, ck, ux, wx, w00, w01, w10, w11);
      if (HAS_Z) Z = blend1<T>(fZ, tx, ty, ci, cj, ck, ux, wx, w00, w01, w10, w11);
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
    const double uu = norm2(u0, u1, u2);
    const double q = uu * ic2;
    g = sqrt(1.0 + q);  // gn: k_push's, from the same operations
    const double un = sqrt(uu);
    const double v = un / g;
    const double ds = v * A.dt;
    const bool matter = ne > 0.0 && Z > 0.0;  // a midpoint outside left ne = 0; a NaN fails both
    if (matter && !(uu > 0.0)) {  // at rest in matter
      stopped = true;
    } else if (matter) {
      const double pv = (A.mass * uu) / g;
      const double Ts = (A.KT * (ne / Z)) / (pv * pv);
      const double sm = s + 0.5 * ds;
      const double t = Ts * ds;
      M0 = M0 + t;
      M1 = M1 + t * sm;
      M2 = M2 + (t * sm) * sm;
    }
    s = s + ds;
    if (matter && !stopped) {
      const double aq = A.A2 * q, b2 = q / (g * g);
      const double Lf = log(aq / (A.HW * sqrt(ne))) - b2;
      const double Lb = log(aq / A.I) - b2;
      const double dz = A.Zn - Z;
      const double nb = (ne * (dz > 0.0 ? dz : 0.0)) / Z;
      const double Nn = ne * (Lf > 0.0 ? Lf : 0.0) + nb * (Lb > 0.0 ? Lb : 0.0);
      const double S = (A.KS / (v * v)) * Nn;
      const double fac = 1.0 - ((S / A.mass) * A.dt) / un;
      const bool moves = fac > 0.0;
      u0 = moves ? u0 * fac : 0.0;
      u1 = moves ? u1 * fac : 0.0;
      u2 = moves ? u2 * fac : 0.0;
      const double qd = norm2(u0, u1, u2) * ic2;
      g = sqrt(1.0 + qd);
      stopped = !moves || (A.mc2 * qd) / (g + 1.0) < A.stop_energy;
    }
    ++steps;
    if (stopped) {  // ends where it is: the midpoint
      x0 = m0;
      x1 = m1;
      x2 = m2;
      inside = false;
    } else {
      const double dn = hd / g;
      x0 = m0 + u0 * dn;
      x1 = m1 + u1 * dn;
      x2 = m2 + u2 * dn;
      inside = x0 >= A.f.lo[0] && x0 <= A.f.hi[0] && x1 >= A.f.lo[1] && x1 <= A.f.hi[1] && x2 >= A.f.lo[2] && x2 <= A.f.hi[2];
    }
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
  A.energy[i] = (A.mc2 * (norm2(u0, u1, u2) * ic2)) / (g + 1.0);
  A.moments[i] = M0;
  A.moments[N + i] = M1;
  A.moments[2 * N + i] = M2;
  A.moments[3 * N + i] = s;
  A.steps[i] = steps;
  A.flags[i] = (uint8_t)((inside ? SR_PUSH_UNFINISHED : 0) | (reaches ? 0 : SR_PUSH_MISSED) | (stopped ? SR_PUSH_STOPPED : 0));
}

// [0] UNFINISHED, [1] MISSED, [2] STOPPED over the flags of a call: a grid-stride count, one atomic per wavefront of a bounded grid
__global__ void __launch_bounds__(256) k_push_matter_flags(const uint8_t *__restrict__ flags, int64_t n, unsigned long long *__restrict__ out) {
  unsigned long long unfinished = 0ull, missed = 0ull, stopped = 0ull;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned f = flags[i];
    unfinished += (f & SR_PUSH_UNFINISHED) ? 1u : 0u;
    missed += (f & SR_PUSH_MISSED) ? 1u : 0u;
    stopped += (f & SR_PUSH_STOPPED) ? 1u : 0u;
  }
  for (int off = 32; off > 0; off >>= 1) {
    unfinished += __shfl_down(unfinished, off, 64);
    missed += __shfl_down(missed, off, 64);
    stopped += __shfl_down(stopped, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (unfinished) atomicAdd(&out[0], unfinished);
    if (missed) atomicAdd(&out[1], missed);
    if (stopped) atomicAdd(&out[2], stopped);
  }
}

template <typename T>
void launch(bool has_e, bool has_b, bool has_z, unsigned grid, hipStream_t st, const MatterArgs &A) {
  sr::with_flags(
      [&](auto e, auto b, auto z) { hipLaunchKernelGGL((k_push_matter<e.value, b.value, z.value, T>), dim3(grid), dim3(256), 0, st, A); },
      has_e, has_b, has_z);
}

}  // namespace

extern "C" int sr_particles_push_matter(const sr_field *E, const sr_field *B, const sr_field *ne, const sr_field *Z,
                                        const sr_push_matter_params *p, int64_t n, const double *s0, double *sf, double *hits,
                                        int32_t *steps, uint8_t *flags, double *energy, double *moments, sr_image *img,
                                        sr_push_matter_stats *stats) {
  SR_CHECK(p != nullptr && s0 != nullptr, "sr_particles_push_matter: NULL argument (p or s0)");
  const sr_push_params &q = p->push;
  SR_CHECK(n >= 0, "sr_particles_push_matter: n must not be negative, got %lld", (long long)n);
  SR_CHECK(std::isfinite(q.dt) && q.dt > 0.0, "sr_particles_push_matter: dt must be finite and positive");
  SR_CHECK(std::isfinite(q.qm), "sr_particles_push_matter: non-finite qm");
  SR_CHECK(std::isfinite(q.det_pos), "sr_particles_push_matter: non-finite det_pos");
  SR_CHECK(std::isfinite(q.hit_scale), "sr_particles_push_matter: non-finite hit_scale");
  SR_CHECK(q.max_steps >= 1, "sr_particles_push_matter: max_steps must be at least 1, got %d", q.max_steps);
  SR_CHECK(q.axis >= 0 && q.axis <= 2, "sr_particles_push_matter: axis must be 0, 1 or 2, got %d", q.axis);
  SR_CHECK(sr::positive(p->mass), "sr_particles_push_matter: mass must be finite and positive");
  SR_CHECK(std::isfinite(p->z), "sr_particles_push_matter: non-finite z");
  SR_CHECK(sr::positive(p->Zn), "sr_particles_push_matter: Zn must be finite and positive");
  SR_CHECK(sr::positive(p->I), "sr_particles_push_matter: I must be finite and positive");
  SR_CHECK(std::isfinite(p->lnLs) && p->lnLs >= 0.0, "sr_particles_push_matter: lnLs must be finite and not negative");
  SR_CHECK(std::isfinite(p->stop_energy) && p->stop_energy >= 0.0, "sr_particles_push_matter: stop_energy must be finite and not negative");
  SR_CHECK(Z != nullptr || sr::positive(p->Z), "sr_particles_push_matter: without a Z field the uniform Z must be finite and positive");
  SR_CHECK(img == nullptr || img->kind == SR_IMG_COUNTS, "sr_particles_push_matter: the image must be of kind SR_IMG_COUNTS");
  SR_CHECK(ne != nullptr, "sr_particles_push_matter: ne is NULL");
  if (int rc = sr::check_fields("sr_particles_push_matter", ne, "ne", {{"ne", ne, 1}, {"Z", Z, 1}, {"E", E, 3}, {"B", B, 3}})) return rc;
  if (stats) *stats = sr_push_matter_stats{0.0, 0, 0, 0, 0, 0};
  if (n == 0) return SR_OK;
  if (int rc = sr::ensure_init()) return rc;
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;

  // one scratch block: s0 | sf | hits | energy | moments | steps | flags | counters {unfinished, missed, stopped, deposited}
  MatterArgs A{};
  unsigned long long *counters = nullptr;
  sr::Carve carve;
  carve.take(&A.s0, 6 * (size_t)n);
  carve.take(&A.sf, 6 * (size_t)n);
  carve.take(&A.hits, 2 * (size_t)n);
  carve.take(&A.energy, (size_t)n);
  carve.take(&A.moments, 4 * (size_t)n);
  carve.take(&A.steps, (size_t)n);
  carve.take(&A.flags, (size_t)n);
  carve.take(&counters, 4);
  if (!carve.alloc()) return SR_ERR_HIP;
  constexpr double e = 1.602176634e-19, m_e = 9.1093837015e-31, eps0 = 8.8541878128e-12, hbar = 1.054571817e-34, pi = 3.141592653589793;
  const double e2 = e * e;
  const double ze = (p->z * e2) / ((4.0 * pi) * eps0);
  A.E = E ? E->data : nullptr;
  A.B = B ? B->data : nullptr;
  A.ne = ne->data;
  A.Z = Z ? Z->data : nullptr;
  A.f = sr::grid_of(ne);
  A.hq = (q.qm * q.dt) * 0.5;
  A.hd = q.dt * 0.5;
  A.ic2 = 1.0 / (sr::kC * sr::kC);
  A.det_pos = q.det_pos;
  A.hit_scale = q.hit_scale;
  A.dt = q.dt;
  A.mass = p->mass;
  A.mc2 = p->mass * (sr::kC * sr::kC);
  A.A2 = (2.0 * m_e) * (sr::kC * sr::kC);
  A.HW = hbar * sqrt(e2 / (eps0 * m_e));
  A.I = p->I;
  A.Zn = p->Zn;
  A.Zu = p->Z;
  A.KS = ((p->z * p->z) * (e2 * e2)) / ((((4.0 * pi) * eps0) * eps0) * m_e);
  A.KT = (((8.0 * pi) * (p->Zn * (p->Zn + 1.0))) * (ze * ze)) * p->lnLs;
  A.stop_energy = p->stop_energy;
  A.max_steps = q.max_steps;
  A.axis = q.axis;
  A.np = n;

  if (int rc = sr::upload_sync(const_cast<double *>(A.s0), s0, sizeof(double) * 6 * (size_t)n, st)) return rc;
  SR_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(unsigned long long), st));
  SR_HIP(hipEventRecord(c.ev[0], st));
  if (ne->is_f64)
    launch<double>(E != nullptr, B != nullptr, Z != nullptr, sr::grid_for(n, 256), st, A);
  else
    launch<float>(E != nullptr, B != nullptr, Z != nullptr, sr::grid_for(n, 256), st, A);
  SR_HIP(hipGetLastError());
  SR_HIP(hipEventRecord(c.ev[1], st));
  if (stats) {
    hipLaunchKernelGGL(k_push_matter_flags, dim3(std::min<unsigned>(sr::grid_for(n, 256), 1024u)), dim3(256), 0, st, A.flags, n, counters);
    SR_HIP(hipGetLastError());
  }
  if (img)
    if (int rc = sr::counts_deposit_device(A.hits, A.hits + n, A.flags, n, img, counters + 3, st)) return rc;
  if (sf) SR_HIP(hipMemcpyAsync(sf, A.sf, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost, st));
  if (hits) SR_HIP(hipMemcpyAsync(hits, A.hits, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
  if (energy) SR_HIP(hipMemcpyAsync(energy, A.energy, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
  if (moments) SR_HIP(hipMemcpyAsync(moments, A.moments, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost, st));
  if (steps) SR_HIP(hipMemcpyAsync(steps, A.steps, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
  if (flags) SR_HIP(hipMemcpyAsync(flags, A.flags, (size_t)n, hipMemcpyDeviceToHost, st));
  unsigned long long hc[4] = {0, 0, 0, 0};
  if (stats) SR_HIP(hipMemcpyAsync(hc, counters, sizeof(hc), hipMemcpyDeviceToHost, st));
  if (int rc = sr::finish_timed(c, stats ? &stats->kernel_ms : nullptr)) return rc;
  if (stats) {
    stats->unfinished = (int64_t)hc[0];
    stats->finished = n - (int64_t)hc[0];
    stats->missed = (int64_t)hc[1];
    stats->stopped = (int64_t)hc[2];
    stats->deposited = (int64_t)hc[3];
  }
  return SR_OK;
}
