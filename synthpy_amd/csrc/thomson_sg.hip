// Optical Thomson scattering from super-Gaussian (Langdon) electrons: sr_field_thomson_multi's spectral density function with the
// electron distribution f(v) ~ exp(-(v/v_m)^m), whose order m, 2 <= m <= 5, is a scalar field gathered at every quadrature point
// or one uniform number (sr_field_thomson_sg; include/synthray.h states the rule every sample follows, operation for operation).
// The ions -- 1..SR_MAX_SPECIES Maxwellian species, flow, drift -- are sr_field_thomson_multi's.  No reference counterpart.
//
// k_thomson_multi's decomposition (thomson_multi.hip, which this file leaves alone): one workgroup of 256 lanes per (volume, tile
// of 256 wavelengths), a lane owns one wavelength and keeps its sum in a register; the quadrature points are taken in chunks of up
// to 64, gathered by the first wavefront -- one point per lane -- and reduced to what does not depend on the wavelength: the
// numbers k_thomson_multi stages (64 x (7 + 3 x 4) doubles) and, for a super-Gaussian point, m, r, b, c, T, fe, pi*b, 2/m and
// GAM(2/m) (64 x 9 doubles).  After a barrier all 256 lanes together fill the points' tables g_i = exp(-(T s_i^2)^m), i < 48
// (64 x 48 doubles = 24 KiB; one pow and one exp per entry, 12 entries per lane and chunk; a Maxwellian or dropped point has no
// table).  That is 38.3 KiB of LDS per workgroup, so four workgroups share a CU's 160 KiB.  After a second barrier every lane walks
// the chunk from LDS by broadcast reads.  The node abscissae s_i^2 and weights 2 w_i s_i are compile-time constants (kS2, kV:
// constant memory, read by scalar loads in the sample loop, where the node index is uniform).
//
// Branches.  Uniform over the workgroup, so no wavefront diverges on them: a dropped point, the Maxwellian / super-Gaussian choice
// (m belongs to the point), the species loop and its g_j == 0 skip, the idle lanes of the last tile (whole wavefronts but one).
// Per lane, and they CAN diverge inside a wavefront: |xi| < T against |xi| >= T (coherent: xi is monotone in the wavelength, so at
// most the wavefronts that straddle +-T run both sums); a quadrature node within 1e-6 of |xi| (rare: the Taylor form runs for the
// whole wavefront's node while the other lanes wait); the incomplete gamma function's series (y < 2/m + 1) against its continued
// fraction, and their trip counts (neighbouring wavelengths have neighbouring y, so the counts differ by a few; a wavefront runs
// its longest).  One division per quadrature node serves both signs of t.  No atomics; points and species are summed in ascending
// order, so a repeated call returns identical bits, and a point with m - 2 <= 2^-30 runs k_thomson_multi's sample lines and returns
// its bits.  k_thomson_sg is instantiated per (V given, Vd given, float32 / float64 source).  Float64 throughout, compiled with
// -ffp-contract=off (tests/test_thomson_sg.py restates the rule in NumPy).
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace {

constexpr int kChunk = 64;   // quadrature points staged in LDS at a time: one wavefront gathers them
constexpr int kTile = 256;   // wavelengths per workgroup, one per lane
constexpr int kNS = SR_MAX_SPECIES;
constexpr int kNN = 48;      // Gauss-Legendre nodes per sign of t
constexpr int kItMax = 100;  // the most terms of the incomplete gamma function's series or continued fraction

constexpr double kE = 1.602176634e-19, kMe = 9.1093837015e-31, kMp = 1.67262192369e-27, kEps0 = 8.8541878128e-12;
constexpr double kPi = 3.141592653589793;
constexpr double kSP = 1.7724538509055159, kTSP = 3.5449077018110318, kISP = 0.5641895835477563;
constexpr double kOrderEps = 9.313225746154785e-10;  // 2^-30
constexpr double kNear = 1e-6, kEps = 1e-16, kTiny = 1e-300;

// s_i^2 and 2 w_i s_i of the 48-point Gauss-Legendre rule (s_i, w_i) on [0, 1], ascending, rounded to float64
__constant__ const double kS2[48] = {
    3.776057933972995e-07, 1.0464667725774222e-05, 6.30072104933835e-05, 0.00021621360724148508,
    0.0005525390135329406, 0.0011769465530495093, 0.002214684226351606, 0.0038086165447951685,
    0.0061161579754197915, 0.009305862406902165, 0.013553729034751516, 0.01903929022374357,
    0.025941550950880653, 0.034434852293860445, 0.04468473305869298, 0.05684386400696272,
    0.07104812824074143, 0.08741291914512875, 0.10602972390977727, 0.1269630561070508,
    0.1502477951708024, 0.17588698398965527, 0.20385012831244823, 0.2340720333864615,
    0.26645220434933087, 0.30085482752191095, 0.337109340058547, 0.37501158556549147,
    0.4143255434625064, 0.45478561020193803, 0.4960994011358455, 0.5379510329916999,
    0.5800048387291957, 0.6219094591426657, 0.663302249070374, 0.7038139305835446,
    0.7430734211475583, 0.7807127615504919, 0.8163720664363447, 0.8497044195998134,
    0.8803806368190431, 0.9080938209419213, 0.9325636372596039, 0.9535402421739638,
    0.9708078061534887, 0.9841875909333202, 0.9935406369340766, 0.9987713848582195};
__constant__ const double kV[48] = {
    1.9377197144373026e-06, 2.370400572514343e-05, 9.110293832805722e-05, 0.00022908143231549464,
    0.0004611003791369082, 0.0008086339518752003, 0.0012907033853146828, 0.0019234539825272498,
    0.002719782918615556, 0.003689024512086719, 0.004836698653385073, 0.0061643270062072845,
    0.007669320445015031, 0.009344939980463058, 0.011180332173536669, 0.013160638770058469,
    0.015267179021227916, 0.01747770191430658, 0.019766704341362004, 0.022105810103284124,
    0.02446420360014816, 0.026809111115060624, 0.02910632177282649, 0.03132073956107341,
    0.033416957251610514, 0.03535984266312359, 0.03711512746958756, 0.03864998868610586,
    0.03993361305660854, 0.04093773482453188, 0.041637137784089055, 0.0420101130791753,
    0.042038864929925694, 0.041709857311656995, 0.04101409557339142, 0.039947338047475446,
    0.038510233850487, 0.03670838429007968, 0.03455232655374399, 0.03205743964615488,
    0.02924377385027084, 0.026135806323042264, 0.022762126887449177, 0.01915506007821862,
    0.015350234290628354, 0.011386131640906483, 0.007303849895551119, 0.0031514083325914015};
// the Chebyshev coefficients of the gamma function on [1, 2] in tau = 2 w - 3, rounded to float64; the next one is below 1e-18
__constant__ const double kGC[24] = {
    0.9417855977954946, 0.004415381324841007, 0.05685043681599363, -0.00421983539641856,
    0.0013268081812124603, -0.00018930245297988805, 3.606925327441245e-05, -6.056761904460864e-06,
    1.0558295463022833e-06, -1.811967365542384e-07, 3.117724964715322e-08, -5.354219639019687e-09,
    9.193275519859589e-10, -1.5779412802883398e-10, 2.7079806229349544e-11, -4.64681865382573e-12,
    7.97335019200742e-13, -1.368078209830916e-13, 2.3473194865638007e-14, -4.027432614949067e-15,
    6.910051747372101e-16, -1.185584500221993e-16, 2.034148542496374e-17, -3.490054341717406e-18};

struct SgArgs {
  const void *ne, *Te, *Ti, *V, *Vd, *order;  // Ti, V, Vd, order may be nullptr
  const void *Z[kNS], *F[kNS];                // a nullptr entry: the uniform Zu[j], fu[j]
  double Zu[kNS], fu[kNS], ci[kNS];
  double mu;                                  // the uniform order where order is nullptr
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

// D(x) of sr_field_thomson's rule: Dawson's function F and E = exp(-x^2); the same operations as thomson_multi.hip's
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

// GAM(z) of the rule, 0.2 <= z <= 2.5: the gamma function by its Chebyshev series on [1, 2] (Clenshaw) and one recurrence step
__device__ __forceinline__ double gam(double z) {
  const double w = z < 1.0 ? z + 1.0 : (z > 2.0 ? z - 1.0 : z);
  const double tau = 2.0 * w - 3.0;
  const double t2 = 2.0 * tau;
  double b1 = 0.0, b2 = 0.0;
#pragma unroll
  for (int k = 23; k >= 1; --k) {
    const double b0 = (kGC[k] + t2 * b1) - b2;
    b2 = b1;
    b1 = b0;
  }
  const double P = (kGC[0] + tau * b1) - b2;
  return z < 1.0 ? P / z : (z > 2.0 ? (z - 1.0) * P : P);
}

// The electron lines of a super-Gaussian sample: R_m(xs) and Gamma(2/m, |xs|^m).  gt: the point's table g_i in LDS.
__device__ __forceinline__ void sg_electron(double xs, double m, double b, double T, double z2, double G2, const double *gt, double &R,
                                            double &gx, double &Q) {
  const double x = fabs(xs);
  const double y = pow(x, m);
  gx = exp(-y);
  const double x2 = x * x;
  if (x < T) {
    const double tx = 2.0 * x;
    const double L = log((T - x) / (T + x));
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < kNN; ++i) {
      const double t = T * kS2[i];
      const double e = t - x;
      const double dg = gt[i] - gx;
      double h;
      if (fabs(e) < kNear) {  // the 1/(t - x) half by Taylor's form, the 1/(t + x) half as it stands
        const double pm1 = m * pow(x, m - 1.0);
        const double g1 = -(pm1 * gx);
        const double g2 = gx * (pm1 * pm1 - (m * (m - 1.0)) * pow(x, m - 2.0));
        h = (g1 + (0.5 * g2) * e) - dg / (t + x);
      } else {
        h = (dg * tx) / (t * t - x2);
      }
      s = s + kV[i] * h;
    }
    R = 1.0 + (x * b) * (T * s + gx * L);
  } else {
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < kNN; ++i) {
      const double t = T * kS2[i];
      const double tt = t * t;
      s = s + kV[i] * ((gt[i] * (2.0 * tt)) / (tt - x2));
    }
    R = (b * T) * s;
  }
  const double xg = x2 * gx;  // y^(2/m) exp(-y)
  if (y < z2 + 1.0) {
    double ap = z2, de = 1.0 / z2;
    double sm = de;
    for (int n = 0; n < kItMax; ++n) {
      ap = ap + 1.0;
      de = de * (y / ap);
      sm = sm + de;
      if (fabs(de) < fabs(sm) * kEps) break;
    }
    Q = G2 - sm * xg;
  } else {
    double bb = (y + 1.0) - z2;
    double cc = 1.0 / kTiny;
    double d = 1.0 / bb;
    double h = d;
    if (y <= 1.7976931348623157e308) {  // y = inf: h = 0 and xg = 0 already
      for (int i = 1; i <= kItMax; ++i) {
        const double an = -(double)i * ((double)i - z2);
        bb = bb + 2.0;
        d = an * d + bb;
        if (fabs(d) < kTiny) d = kTiny;
        cc = bb + an / cc;
        if (fabs(cc) < kTiny) cc = kTiny;
        d = 1.0 / d;
        const double de = d * cc;
        h = h * de;
        if (fabs(de - 1.0) < kEps) break;
      }
    }
    Q = xg * h;
  }
}

template <bool HAS_V, bool HAS_VD, typename T>
__global__ void __launch_bounds__(256) k_thomson_sg(SgArgs A) {
  __shared__ double s_wn[kChunk], s_ivte[kChunk], s_pe[kChunk], s_vs[kChunk], s_vi[kChunk], s_ds[kChunk], s_di[kChunk];
  __shared__ double s_ivti[kNS][kChunk], s_zt[kNS][kChunk], s_g[kNS][kChunk];
  __shared__ double s_m[kChunk], s_r[kChunk], s_b[kChunk], s_c[kChunk], s_T[kChunk], s_fe[kChunk], s_pib[kChunk], s_z2[kChunk], s_G2[kChunk];
  __shared__ double s_gt[kChunk][kNN];
  __shared__ int s_keep[kChunk];  // 0: dropped; 1: Maxwellian sample lines; 2: super-Gaussian
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
      int kind = 0;
      if (in_x && in_y && in_z) {
        const double ux = 1.0 - wx, uy = 1.0 - wy, uz = 1.0 - wz;
        const double w00 = uy * uz, w01 = uy * wz, w10 = wy * uz, w11 = wy * wz;
        auto scalar = [&](const void *p) { return blend<T>(static_cast<const T *>(p), 1, 0, sx, sy, ci, cj, ck, ux, wx, w00, w01, w10, w11); };
        auto vector = [&](const void *p, int c) { return blend<T>(static_cast<const T *>(p), 3, c, sx, sy, ci, cj, ck, ux, wx, w00, w01, w10, w11); };
        const double ne = scalar(A.ne);
        const double Te = scalar(A.Te);
        const double Ti = A.Ti ? scalar(A.Ti) : Te;
        const double mo = A.order ? scalar(A.order) : A.mu;
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
        const bool keep = ne > 0.0 && Te > 0.0 && Ti > 0.0 && species_ok && vs == vs && vi == vi && ds == ds && di == di && mo == mo;
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
          const double m = fmin(fmax(mo, 2.0), 5.0);
          s_m[j] = m;
          kind = m - 2.0 > kOrderEps ? 2 : 1;
        }
      }
      if (kind == 2) {  // the constants of a super-Gaussian point, once what the gather held in registers is dead
        const double m = s_m[j];
        const double im = 1.0 / m;
        const double z2 = 2.0 * im;
        const double G1 = gam(im), G2 = gam(z2), G3 = gam(3.0 * im), G5 = gam(5.0 * im);
        const double r = sqrt((2.0 * G5) / (3.0 * G3));
        const double b = m / (2.0 * G1);
        s_r[j] = r;
        s_b[j] = b;
        s_c[j] = (G1 * G5) / ((3.0 * G3) * G3);
        s_T[j] = pow(40.0, im);
        s_fe[j] = (kSP * r) / (2.0 * G3);
        s_pib[j] = kPi * b;
        s_z2[j] = z2;
        s_G2[j] = G2;
      }
      s_keep[j] = kind;
    }
    __syncthreads();
    // the tables of the chunk's super-Gaussian points, by all lanes together
    for (int idx = (int)threadIdx.x; idx < cnt * kNN; idx += 256) {
      const int j = idx / kNN, i = idx - j * kNN;
      if (s_keep[j] == 2) s_gt[j][i] = exp(-pow(s_T[j] * kS2[i], s_m[j]));
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const int kind = s_keep[j];
      if (!kind) continue;  // the same for every lane
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
      double cer, cei, Ee;
      if (kind == 2) {  // uniform: m belongs to the point
        const double xs = xe * s_r[j];
        double R, gx, Q;
        sg_electron(xs, s_m[j], s_b[j], s_T[j], s_z2[j], s_G2[j], s_gt[j], R, gx, Q);
        const double ac = al * s_c[j];
        cer = ac * R;
        cei = ac * ((s_pib[j] * xs) * gx);
        Ee = s_fe[j] * Q;
      } else {
        double Fe;
        dawson(xe, Fe, Ee);
        cer = al * (1.0 - (2.0 * xe) * Fe);
        cei = al * ((kSP * xe) * Ee);
      }
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
void launch(bool has_v, bool has_vd, unsigned grid, hipStream_t st, const SgArgs &A) {
  sr::with_flags([&](auto v, auto d) { hipLaunchKernelGGL((k_thomson_sg<v.value, d.value, T>), dim3(grid), dim3(256), 0, st, A); },
                 has_v, has_vd);
}

using sr::positive;

bool not_negative(double v) { return std::isfinite(v) && v >= 0.0; }

constexpr const char *kZName[kNS] = {"Z0", "Z1", "Z2", "Z3"};
constexpr const char *kFName[kNS] = {"f0", "f1", "f2", "f3"};

}  // namespace

extern "C" int sr_field_thomson_sg(const sr_field *ne, const sr_field *Te, const sr_field *Ti, const sr_field *V, const sr_field *Vd,
                                   const sr_field *const *Zs, const sr_field *const *fracs, const sr_field *order,
                                   const sr_thomson_sg_params *p, int64_t n_vol, int32_t n_quad, const double *pts, const double *wts,
                                   const double *ki, const double *ks, int32_t n_lambda, const double *lambda, double *P, double *weight,
                                   double *kernel_ms) {
  SR_CHECK(p != nullptr && pts != nullptr && wts != nullptr && ki != nullptr && ks != nullptr && lambda != nullptr && P != nullptr &&
               weight != nullptr,
           "sr_field_thomson_sg: NULL argument (p, pts, wts, ki, ks, lambda, P or weight)");
  SR_CHECK(n_vol >= 0 && n_quad >= 0 && n_lambda >= 0,
           "sr_field_thomson_sg: counts must not be negative, got n_vol %lld, n_quad %d, n_lambda %d", (long long)n_vol, n_quad, n_lambda);
  SR_CHECK(positive(p->lambda_i), "sr_field_thomson_sg: lambda_i must be finite and positive");
  SR_CHECK(p->n_species >= 1 && p->n_species <= kNS, "sr_field_thomson_sg: n_species must be 1..%d, got %d", kNS, p->n_species);
  const int ns = p->n_species;
  const sr_field *Zf[kNS] = {}, *Ff[kNS] = {};
  for (int j = 0; j < ns; ++j) {
    Zf[j] = Zs ? Zs[j] : nullptr;
    Ff[j] = fracs ? fracs[j] : nullptr;
    SR_CHECK(positive(p->A[j]), "sr_field_thomson_sg: A[%d] must be finite and positive", j);
    SR_CHECK(Zf[j] != nullptr || not_negative(p->Z[j]), "sr_field_thomson_sg: uniform Z[%d] must be finite and not negative", j);
    SR_CHECK(Ff[j] != nullptr || not_negative(p->frac[j]), "sr_field_thomson_sg: uniform frac[%d] must be finite and not negative", j);
  }
  SR_CHECK(order != nullptr || (p->order >= 2.0 && p->order <= 5.0),  // false for a NaN
           "sr_field_thomson_sg: the uniform order must lie in [2, 5], got %g", p->order);
  for (int32_t l = 0; l < n_lambda; ++l)
    SR_CHECK(positive(lambda[l]), "sr_field_thomson_sg: lambda[%d] must be finite and positive", l);
  for (int64_t m = 0; m < n_vol; ++m) {
    const double *a = ki + 3 * m, *b = ks + 3 * m;
    const double na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], nb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    SR_CHECK(std::fabs(na - 1.0) <= 1e-12, "sr_field_thomson_sg: ki of volume %lld is not a finite unit vector", (long long)m);
    SR_CHECK(std::fabs(nb - 1.0) <= 1e-12, "sr_field_thomson_sg: ks of volume %lld is not a finite unit vector", (long long)m);
    const double cth = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    SR_CHECK(!(a[0] == b[0] && a[1] == b[1] && a[2] == b[2]) && cth < 1.0,
             "sr_field_thomson_sg: ki equals ks in volume %lld (no scattering wavevector)", (long long)m);
  }
  const int64_t n_tiles = ((int64_t)n_lambda + kTile - 1) / kTile;
  SR_CHECK(n_tiles == 0 || n_vol <= (int64_t)2147483647 / n_tiles,
           "sr_field_thomson_sg: n_vol x wavelength tiles exceeds 2^31 - 1 workgroups");
  SR_CHECK(ne != nullptr && Te != nullptr, "sr_field_thomson_sg: NULL field (ne or Te)");
  if (int rc = sr::check_fields("sr_field_thomson_sg", ne, "ne",
                                {{"ne", ne, 1}, {"Te", Te, 1}, {"Ti", Ti, 1}, {"V", V, 3}, {"Vd", Vd, 3}, {"order", order, 1},
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
  SgArgs A{};
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
  A.order = order ? order->data : nullptr;
  A.mu = order ? 2.0 : p->order;
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
