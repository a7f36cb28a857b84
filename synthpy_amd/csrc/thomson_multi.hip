// Optical Thomson scattering of a plasma with several ion species and drifting electrons: sr_field_thomson's spectral density
// function with 1..SR_MAX_SPECIES Maxwellian ion species (mass number A_j, charge Z_j, relative abundance f_j; one Ti and one flow)
// and an electron drift Vd against the ions (sr_field_thomson_multi; include/synthray.h states the rule every sample follows,
// operation for operation).  No reference counterpart.
//
// k_thomson's decomposition (thomson.hip, which this file leaves alone): one workgroup of 256 lanes per (volume, tile of 256
// wavelengths), a lane owns one wavelength and keeps its sum in a register; the quadrature points are taken in chunks of up to
// 64, gathered by the first wavefront -- one point per lane -- and reduced to the numbers that do not depend on the wavelength:
// w*ne, 1/v_te, ne e/(eps0 Te), V.ks, V.ki, Vd.ks, Vd.ki, a kept flag and per species 1/v_ti_j, g_j Te/Ti, g_j = Z_j^2 n_j/ne.
// That is 64 x (7 + 3 x 4) doubles = 9.5 KiB of LDS.  After a barrier every lane walks the chunk from LDS by broadcast reads.  The
// species loop is unrolled over SR_MAX_SPECIES with a uniform exit at n_species, so exp(-xi_j^2) of the first pass stays in
// registers (statically indexed: no scratch) for the ion term of the second.  A species whose g_j is 0 at a point adds exact zeros
// and is skipped: g_j is the same for every lane.  No atomics; points and species are summed in ascending order, so a repeated
// call returns identical bits, and one species with f = 1 returns k_thomson's bits.  k_thomson_multi is instantiated per (V given,
// Vd given, float32 / float64 source).  Compiled with -ffp-contract=off (tests/test_thomson_multi.py restates the rule in NumPy).
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace {

constexpr int kChunk = 64;   // quadrature points staged in LDS at a time: one wavefront gathers them
constexpr int kTile = 256;   // wavelengths per workgroup, one per lane
constexpr int kNS = SR_MAX_SPECIES;

constexpr double kE = 1.602176634e-19, kMe = 9.1093837015e-31, kMp = 1.67262192369e-27, kEps0 = 8.8541878128e-12;
constexpr double kPi = 3.141592653589793;
constexpr double kSP = 1.7724538509055159, kTSP = 3.5449077018110318, kISP = 0.5641895835477563;

struct MultiArgs {
  const void *ne, *Te, *Ti, *V, *Vd;  // Ti, V, Vd may be nullptr
  const void *Z[kNS], *F[kNS];        // a nullptr entry: the uniform Zu[j], fu[j]
  double Zu[kNS], fu[kNS], ci[kNS];
  int ns;
  sr::FieldGrid f;
  const double *pts;     // (n_vol, nq, 3)
  const double *wts;     // (n_vol, nq)
  const double *ki, *ks; // (n_vol, 3)
  const double *lam;     // (n_lambda)
  double *P;             // (n_vol, n_lambda)
  double *weight;        // (n_vol)
  int nq, n_lambda, n_tiles;
  double tpc, ce, ee0, wi, kin;
};

using sr::blend;  // one scalar at a cell with the blend of sr_field_resample's rule (common.hpp)

// D(x) of sr_field_thomson's rule: Dawson's function F and E = exp(-x^2); the same operations as thomson.hip's
__device__ __forceinline__ void dawson(double x, double &F, double &E) {
  constexpr double C[13] = {0.9394130628134758,     0.569782824730923,      0.2096113871510978,     0.04677062238395898,
                            0.006329715427485747,   0.0005195746821548384,  2.586810022265412e-05,  7.811489408304491e-07,
                            1.4307241918567688e-08, 1.5893910094516368e-10, 1.0709232382508077e-12, 4.37661850287085e-15,
                            1.0848552640429378e-17};
  const double n0 = 2.0 * rint(2.0 * x);
  const double xp = x - 0.25 * n0;
  const double g = exp(-(xp * xp));
  double p = exp(0.5 * xp);
  double m = 1.0 / p;
  const double p2 = p * p, m2 = m * m, d0 = n0 * n0;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 13; ++j) {
    const double n = (double)(2 * j + 1);
    s = s + C[j] * ((p * (n0 - n) + m * (n0 + n)) / (d0 - n * n));
    p = p * p2;
    m = m * m2;
  }
  F = (g * s) * kISP;
  E = exp(-(x * x));
}

template <bool HAS_V, bool HAS_VD, typename T>
__global__ void __launch_bounds__(256) k_thomson_multi(MultiArgs A) {
  __shared__ double s_wn[kChunk], s_ivte[kChunk], s_pe[kChunk], s_vs[kChunk], s_vi[kChunk], s_ds[kChunk], s_di[kChunk];
  __shared__ double s_ivti[kNS][kChunk], s_zt[kNS][kChunk], s_g[kNS][kChunk];
  __shared__ int s_keep[kChunk];
  const int64_t vol = blockIdx.x / (unsigned)A.n_tiles;
  const int tile = (int)(blockIdx.x % (unsigned)A.n_tiles);
  const int l = tile * kTile + (int)threadIdx.x;
  const bool active = l < A.n_lambda;
  const int ns = A.ns;
  const double ki0 = A.ki[vol * 3], ki1 = A.ki[vol * 3 + 1], ki2 = A.ki[vol * 3 + 2];
  const double ks0 = A.ks[vol * 3], ks1 = A.ks[vol * 3 + 1], ks2 = A.ks[vol * 3 + 2];
  const double cth = (ki0 * ks0 + ki1 * ks1) + ki2 * ks2;
  const double wi = A.wi, kin = A.kin;
  // the wavelength's constants; an idle lane of the last tile takes the probe's own wavelength and stores nothing
  const double lam = active ? A.lam[l] : A.tpc / wi;
  const double ws = A.tpc / lam;
  const double w = ws - wi;
  const double ksc = ws / sr::kC;
  const double k2 = (ksc * ksc + kin * kin) - ((2.0 * ksc) * kin) * cth;
  const double k = sqrt(k2);
  const double rk = 1.0 / k, rk2 = 1.0 / k2;
  const double pre = kTSP * rk;

  const int64_t sy = A.f.n[2], sx = (int64_t)A.f.n[1] * sy;
  double acc = 0.0, wsum = 0.0;
  for (int q0 = 0; q0 < A.nq; q0 += kChunk) {
    const int cnt = min(kChunk, A.nq - q0);
    __syncthreads();  // the chunk before this one has been read by every lane
    if ((int)threadIdx.x < cnt) {
      const int j = (int)threadIdx.x;
      const int64_t q = vol * A.nq + q0 + j;
      const double px = A.pts[q * 3], py = A.pts[q * 3 + 1], pz = A.pts[q * 3 + 2];
      int ci = 0, cj = 0, ck = 0;
      double wx = 0, wy = 0, wz = 0;
      const bool in_x = sr::locate_in<true>(A.f.g[0], A.f.n[0], A.f.inv_h[0], A.f.lo[0], A.f.hi[0], px, ci, wx);
      const bool in_y = sr::locate_in<true>(A.f.g[1], A.f.n[1], A.f.inv_h[1], A.f.lo[1], A.f.hi[1], py, cj, wy);
      const bool in_z = sr::locate_in<true>(A.f.g[2], A.f.n[2], A.f.inv_h[2], A.f.lo[2], A.f.hi[2], pz, ck, wz);
      bool keep = false;
      if (in_x && in_y && in_z) {
        const double ux = 1.0 - wx, uy = 1.0 - wy, uz = 1.0 - wz;
        const double w00 = uy * uz, w01 = uy * wz, w10 = wy * uz, w11 = wy * wz;
        auto scalar = [&](const void *p) { return blend<T>(static_cast<const T *>(p), 1, 0, sx, sy, ci, cj, ck, ux, wx, w00, w01, w10, w11); };
        auto vector = [&](const void *p, int c) { return blend<T>(static_cast<const T *>(p), 3, c, sx, sy, ci, cj, ck, ux, wx, w00, w01, w10, w11); };
        const double ne = scalar(A.ne);
        const double Te = scalar(A.Te);
        const double Ti = A.Ti ? scalar(A.Ti) : Te;
        double vs = 0.0, vi = 0.0, ds = 0.0, di = 0.0;
        if (HAS_V) {
          const double V0 = vector(A.V, 0), V1 = vector(A.V, 1), V2 = vector(A.V, 2);
          vs = (V0 * ks0 + V1 * ks1) + V2 * ks2;
          vi = (V0 * ki0 + V1 * ki1) + V2 * ki2;
        }
        if (HAS_VD) {
          const double D0 = vector(A.Vd, 0), D1 = vector(A.Vd, 1), D2 = vector(A.Vd, 2);
          ds = (D0 * ks0 + D1 * ks1) + D2 * ks2;
          di = (D0 * ki0 + D1 * ki1) + D2 * ki2;
        }
        double Z[kNS], fr[kNS];
        bool species_ok = true;  // Z_j >= 0 and f_j >= 0 are false for a NaN
        double zb = 0.0;
#pragma unroll
        for (int s = 0; s < kNS; ++s) {
          Z[s] = fr[s] = 0.0;
          if (s < ns) {
            Z[s] = A.Z[s] ? scalar(A.Z[s]) : A.Zu[s];
            fr[s] = A.F[s] ? scalar(A.F[s]) : A.fu[s];
            species_ok = species_ok && Z[s] >= 0.0 && fr[s] >= 0.0;
            zb = zb + fr[s] * Z[s];
          }
        }
        // ne, Te, Ti > 0 is false for a NaN; a NaN component of V or Vd makes its projections NaN (the directions are finite)
        keep = ne > 0.0 && Te > 0.0 && Ti > 0.0 && species_ok && vs == vs && vi == vi && ds == ds && di == di;
        if (keep) {
          s_wn[j] = A.wts[q] * ne;
          s_ivte[j] = 1.0 / sqrt(A.ce * Te);
          s_pe[j] = (ne * A.ee0) / Te;
          s_vs[j] = vs;
          s_vi[j] = vi;
          s_ds[j] = ds;
          s_di[j] = di;
#pragma unroll
          for (int s = 0; s < kNS; ++s) {
            if (s < ns) {
              const double c = zb > 0.0 ? (fr[s] * Z[s]) / zb : 0.0;
              const double g = Z[s] * c;
              s_g[s][j] = g;
              s_zt[s][j] = (g * Te) / Ti;
              s_ivti[s][j] = 1.0 / sqrt(A.ci[s] * Ti);
            }
          }
        }
      }
      s_keep[j] = keep ? 1 : 0;
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      if (!s_keep[j]) continue;  // the same for every lane
      const double wn = s_wn[j];
      wsum = wsum + wn;
      if (!active) continue;  // the last tile's idle lanes: a wavefront made of them skips the arithmetic
      double wp = w;
      if (HAS_V) wp = w - (ksc * s_vs[j] - kin * s_vi[j]);
      const double ivte = s_ivte[j];
      const double a = wp * rk;
      double ae = a;
      if (HAS_VD) ae = (wp - (ksc * s_ds[j] - kin * s_di[j])) * rk;
      const double xe = ae * ivte;
      const double al = s_pe[j] * rk2;
      double Fe, Ee;
      dawson(xe, Fe, Ee);
      const double cer = al * (1.0 - (2.0 * xe) * Fe), cei = al * ((kSP * xe) * Ee);
      double er = 1.0 + cer, ei = cei, sr_ = 1.0, si = 0.0;
      double Ei[kNS];
#pragma unroll
      for (int s = 0; s < kNS; ++s) {
        Ei[s] = 0.0;
        if (s < ns && s_g[s][j] != 0.0) {  // uniform; a species with g = 0 adds exact zeros
          const double xi = a * s_ivti[s][j];
          const double az = al * s_zt[s][j];
          double Fi;
          dawson(xi, Fi, Ei[s]);
          const double cir = az * (1.0 - (2.0 * xi) * Fi), cii = az * ((kSP * xi) * Ei[s]);
          er = er + cir;
          ei = ei + cii;
          sr_ = sr_ + cir;
          si = si + cii;
        }
      }
      const double ie2 = 1.0 / (er * er + ei * ei);
      const double n1 = sr_ * sr_ + si * si;
      const double n2 = cer * cer + cei * cei;
      const double t = n2 * ie2;
      double ion = 0.0;
#pragma unroll
      for (int s = 0; s < kNS; ++s)
        if (s < ns && s_g[s][j] != 0.0) ion = ion + ((s_g[s][j] * t) * Ei[s]) * s_ivti[s][j];
      const double S = pre * (((n1 * ie2) * Ee) * ivte + ion);
      acc = acc + wn * S;
    }
  }
  if (active) A.P[vol * A.n_lambda + l] = acc * ((1.0 + (2.0 * w) / wi) * (sr::kC / (lam * lam)));
  if (tile == 0 && threadIdx.x == 0) A.weight[vol] = wsum;
}

template <typename T>
void launch(bool has_v, bool has_vd, unsigned grid, hipStream_t st, const MultiArgs &A) {
  sr::with_flags([&](auto v, auto d) { hipLaunchKernelGGL((k_thomson_multi<v.value, d.value, T>), dim3(grid), dim3(256), 0, st, A); },
                 has_v, has_vd);
}

using sr::positive;

bool not_negative(double v) { return std::isfinite(v) && v >= 0.0; }

constexpr const char *kZName[kNS] = {"Z0", "Z1", "Z2", "Z3"};
constexpr const char *kFName[kNS] = {"f0", "f1", "f2", "f3"};

}  // namespace

extern "C" int sr_field_thomson_multi(const sr_field *ne, const sr_field *Te, const sr_field *Ti, const sr_field *V, const sr_field *Vd,
                                      const sr_field *const *Zs, const sr_field *const *fracs, const sr_thomson_multi_params *p,
                                      int64_t n_vol, int32_t n_quad, const double *pts, const double *wts, const double *ki,
                                      const double *ks, int32_t n_lambda, const double *lambda, double *P, double *weight,
                                      double *kernel_ms) {
  SR_CHECK(p != nullptr && pts != nullptr && wts != nullptr && ki != nullptr && ks != nullptr && lambda != nullptr && P != nullptr &&
               weight != nullptr,
           "sr_field_thomson_multi: NULL argument (p, pts, wts, ki, ks, lambda, P or weight)");
  SR_CHECK(n_vol >= 0 && n_quad >= 0 && n_lambda >= 0,
           "sr_field_thomson_multi: counts must not be negative, got n_vol %lld, n_quad %d, n_lambda %d", (long long)n_vol, n_quad, n_lambda);
  SR_CHECK(positive(p->lambda_i), "sr_field_thomson_multi: lambda_i must be finite and positive");
  SR_CHECK(p->n_species >= 1 && p->n_species <= kNS, "sr_field_thomson_multi: n_species must be 1..%d, got %d", kNS, p->n_species);
  const int ns = p->n_species;
  const sr_field *Zf[kNS] = {}, *Ff[kNS] = {};
  for (int j = 0; j < ns; ++j) {
    Zf[j] = Zs ? Zs[j] : nullptr;
    Ff[j] = fracs ? fracs[j] : nullptr;
    SR_CHECK(positive(p->A[j]), "sr_field_thomson_multi: A[%d] must be finite and positive", j);
    SR_CHECK(Zf[j] != nullptr || not_negative(p->Z[j]), "sr_field_thomson_multi: uniform Z[%d] must be finite and not negative", j);
    SR_CHECK(Ff[j] != nullptr || not_negative(p->frac[j]), "sr_field_thomson_multi: uniform frac[%d] must be finite and not negative", j);
  }
  for (int32_t l = 0; l < n_lambda; ++l)
    SR_CHECK(positive(lambda[l]), "sr_field_thomson_multi: lambda[%d] must be finite and positive", l);
  for (int64_t m = 0; m < n_vol; ++m) {
    const double *a = ki + 3 * m, *b = ks + 3 * m;
    const double na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], nb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    SR_CHECK(std::fabs(na - 1.0) <= 1e-12, "sr_field_thomson_multi: ki of volume %lld is not a finite unit vector", (long long)m);
    SR_CHECK(std::fabs(nb - 1.0) <= 1e-12, "sr_field_thomson_multi: ks of volume %lld is not a finite unit vector", (long long)m);
    const double cth = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    SR_CHECK(!(a[0] == b[0] && a[1] == b[1] && a[2] == b[2]) && cth < 1.0,
             "sr_field_thomson_multi: ki equals ks in volume %lld (no scattering wavevector)", (long long)m);
  }
  const int64_t n_tiles = ((int64_t)n_lambda + kTile - 1) / kTile;
  SR_CHECK(n_tiles == 0 || n_vol <= (int64_t)2147483647 / n_tiles,
           "sr_field_thomson_multi: n_vol x wavelength tiles exceeds 2^31 - 1 workgroups");
  SR_CHECK(ne != nullptr && Te != nullptr, "sr_field_thomson_multi: NULL field (ne or Te)");
  if (int rc = sr::check_fields("sr_field_thomson_multi", ne, "ne",
                                {{"ne", ne, 1}, {"Te", Te, 1}, {"Ti", Ti, 1}, {"V", V, 3}, {"Vd", Vd, 3},
                                 {kZName[0], Zf[0], 1}, {kFName[0], Ff[0], 1}, {kZName[1], Zf[1], 1}, {kFName[1], Ff[1], 1},
                                 {kZName[2], Zf[2], 1}, {kFName[2], Ff[2], 1}, {kZName[3], Zf[3], 1}, {kFName[3], Ff[3], 1}}))
    return rc;
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_vol == 0 || n_lambda == 0) return SR_OK;
  if (int rc = sr::ensure_init()) return rc;
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;

  // one scratch block: pts | wts | ki | ks | lambda | P | weight
  const size_t nv = (size_t)n_vol, nq = (size_t)n_quad, nl = (size_t)n_lambda;
  MultiArgs A{};
  double *d_pts, *d_wts, *d_ki, *d_ks, *d_lam;
  sr::Carve carve;
  carve.take(&d_pts, 3 * nv * nq);
  carve.take(&d_wts, nv * nq);
  carve.take(&d_ki, 3 * nv);
  carve.take(&d_ks, 3 * nv);
  carve.take(&d_lam, nl);
  carve.take(&A.P, nv * nl);
  carve.take(&A.weight, nv);
  if (!carve.alloc()) return SR_ERR_HIP;
  A.ne = ne->data;
  A.Te = Te->data;
  A.Ti = Ti ? Ti->data : nullptr;
  A.V = V ? V->data : nullptr;
  A.Vd = Vd ? Vd->data : nullptr;
  A.ns = ns;
  for (int j = 0; j < ns; ++j) {
    A.Z[j] = Zf[j] ? Zf[j]->data : nullptr;
    A.F[j] = Ff[j] ? Ff[j]->data : nullptr;
    A.Zu[j] = Zf[j] ? 0.0 : p->Z[j];
    A.fu[j] = Ff[j] ? 0.0 : p->frac[j];
    A.ci[j] = (2.0 * kE) / (p->A[j] * kMp);
  }
  A.f = sr::grid_of(ne);
  A.pts = d_pts;
  A.wts = d_wts;
  A.ki = d_ki;
  A.ks = d_ks;
  A.lam = d_lam;
  A.nq = n_quad;
  A.n_lambda = n_lambda;
  A.n_tiles = (int)n_tiles;
  A.tpc = (2.0 * kPi) * sr::kC;
  A.ce = (2.0 * kE) / kMe;
  A.ee0 = kE / kEps0;
  A.wi = A.tpc / p->lambda_i;
  A.kin = A.wi / sr::kC;

  if (nq) {
    if (int rc = sr::upload_sync(d_pts, pts, sizeof(double) * 3 * nv * nq, st)) return rc;
    if (int rc = sr::upload_sync(d_wts, wts, sizeof(double) * nv * nq, st)) return rc;
  }
  SR_HIP(hipMemcpyAsync(d_ki, ki, sizeof(double) * 3 * nv, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(d_ks, ks, sizeof(double) * 3 * nv, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(d_lam, lambda, sizeof(double) * nl, hipMemcpyHostToDevice, st));
  SR_HIP(hipEventRecord(c.ev[0], st));
  const unsigned grid = (unsigned)(n_vol * n_tiles);
  if (ne->is_f64)
    launch<double>(V != nullptr, Vd != nullptr, grid, st, A);
  else
    launch<float>(V != nullptr, Vd != nullptr, grid, st, A);
  SR_HIP(hipGetLastError());
  SR_HIP(hipEventRecord(c.ev[1], st));
  SR_HIP(hipMemcpyAsync(P, A.P, sizeof(double) * nv * nl, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(weight, A.weight, sizeof(double) * nv, hipMemcpyDeviceToHost, st));
  return sr::finish_timed(c, kernel_ms);
}
