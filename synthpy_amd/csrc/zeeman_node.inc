// The Zeeman node of include/synthray.h's "Zeeman-split lines along sightlines" section: what the magnetic field of one sample gives
// every line (zeeman_sample: the Larmor frequency and the five angular factors, from B in the chord's frame, no trigonometry), the
// window test of one component's shifted centre (zeeman_outside, zeeman_term: voigt_outside and voigt_term with the shift between
// the subtraction and the product), what a line's three profile sums add to the four emission coefficients (zeeman_line), the
// update of (I, Q, U, Vs, tau) with ONE scalar attenuation (zeeman_update), and on the host the chord frames and the checks of an
// sr_zeeman_table.  Included inside the including unit's anonymous namespace, after voigt_node.inc.

constexpr double kZeemanMe = 9.1093837015e-31;
constexpr double kZeemanGroupTol = 1e-9;  // every q group's strengths sum to 1 within this
constexpr double kZeemanRefTol = 1e-6;    // ref's part across the chord must exceed this fraction of ref's length
constexpr int kZeemanWords = 6;           // what a staged sample's head gains: wL, sP, cS, cQ, cU, cV

struct ZeemanSample {
  double wL, sP, cS, cQ, cU, cV;
};

// B in the chord's frame F = (n0 n1 n2 | e1 | e2), nine float64
__device__ __forceinline__ ZeemanSample zeeman_sample(const double (&B)[3], const double *F, double kL) {
  const double Bn = (B[0] * F[0] + B[1] * F[1]) + B[2] * F[2];
  const double Bu = (B[0] * F[3] + B[1] * F[4]) + B[2] * F[5];
  const double Bv = (B[0] * F[6] + B[1] * F[7]) + B[2] * F[8];
  const double T = Bu * Bu + Bv * Bv;
  const double B2 = T + Bn * Bn;
  ZeemanSample z;
  if (B2 == 0.0) {
    z.wL = 0.0, z.sP = 1.0, z.cS = 0.5, z.cQ = 0.0, z.cU = 0.0, z.cV = 0.0;
  } else {  // B2 > 0, or a NaN, which this makes of all six
    const double r = sqrt(B2);
    z.wL = kL * r;
    z.sP = T / B2;
    z.cS = 0.5 * (1.0 + (Bn * Bn) / B2);
    z.cQ = (Bu * Bu - Bv * Bv) / B2;
    z.cU = ((2.0 * Bu) * Bv) / B2;
    z.cV = Bn / r;
  }
  return z;
}

// voigt_outside at the centre shifted by sh = g*wL: x = ((omega - wc) - sh)*iw is monotone in omega as rounded (iw >= 0), so the two
// ends decide for all between; a NaN wc, sh or iw skips nothing
__device__ __forceinline__ bool zeeman_outside(double wc, double sh, double iw, double wmin, double wmax, double cut) {
  const double xa = ((wmax - wc) - sh) * iw, xb = ((wmin - wc) - sh) * iw;
  return (xa < 0.0 && xa * xa > cut) || (xb > 0.0 && xb * xb > cut);
}

// one component's term at one frequency: dropped (false) when x*x > cut; a NaN is not dropped
__device__ __forceinline__ bool zeeman_term(double omega, double wc, double sh, double iw, double cut, double &x) {
  x = ((omega - wc) - sh) * iw;
  return !(x * x > cut);
}

// a line's profile sums (P0: pi, Pp: q = +1, Pm: q = -1) into the sample's coefficients
__device__ __forceinline__ void zeeman_line(const ZeemanSample &z, double aJ, double aK, double P0, double Pp, double Pm, double &jI,
                                            double &jQ, double &jU, double &jV, double &aL) {
  const double Ps = Pp + Pm;
  const double eI = 0.5 * (z.sP * P0) + (0.5 * z.cS) * Ps;
  const double eP = 0.5 * (P0 - 0.5 * Ps);
  const double eV = 0.5 * (Pp - Pm);
  jI = jI + aJ * eI;
  jQ = jQ + aJ * (eP * z.cQ);
  jU = jU + aJ * (eP * z.cU);
  jV = jV + aJ * (eV * z.cV);
  aL = aL + aK * eI;
}

// line_update on four parameters: one attenuation exp(-dtau) for all
__device__ __forceinline__ void zeeman_update(double ac, double Sc, double jI, double jQ, double jU, double jV, double aL, double h,
                                              double &I, double &Q, double &U, double &Vs, double &tau) {
  const double a = ac + aL;
  const double dtau = a * h;
  if (dtau == 0.0) {
    I = I + jI * h;
    Q = Q + jQ * h;
    U = U + jU * h;
    Vs = Vs + jV * h;
  } else {  // dtau > 0, or a NaN, which this makes of all five
    const double E = exp(-dtau), F = -expm1(-dtau);
    I = I * E + ((ac * Sc + jI) / a) * F;
    Q = Q * E + (jQ / a) * F;
    U = U * E + (jU / a) * F;
    Vs = Vs * E + (jV / a) * F;
    tau = tau + dtau;
  }
}

// ---- what the kernels that march Stokes parameters share (sightline_zeeman.hip, sightline_stokes.hip)

// sightline_march.inc's fetch_sample and blend_sample of a FlowSample, on a sample that always has V's slots (a lane that carries
// B fills them with B's corners): the same operations, so the same bits
template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI, bool HAS_V>
__device__ __forceinline__ void fetch_staged(const EmArgs &A, const FlowArgs &W, const sr::FieldGrid &f, int64_t sx, int64_t sy,
                                             const Line &l, int k, FlowSample<T, HAS_TE, HAS_Z, HAS_TI, true> &s) {
  const double t = l.t0 + ((double)k + 0.5) * l.dt;
  fetch<T, HAS_TE, HAS_Z>(A, f, sx, sy, l.o0 + l.d0 * t, l.o1 + l.d1 * t, l.o2 + l.d2 * t, s.s, [&](int ci, int cj, int ck) {
    if (HAS_TI) s.Ti = sr::corners_load(static_cast<const T *>(W.Ti), 1, 0, sx, sy, ci, cj, ck);
    if (HAS_V) {
      s.V0 = sr::corners_load(static_cast<const T *>(W.V), 3, 0, sx, sy, ci, cj, ck);
      s.V1 = sr::corners_load(static_cast<const T *>(W.V), 3, 1, sx, sy, ci, cj, ck);
      s.V2 = sr::corners_load(static_cast<const T *>(W.V), 3, 2, sx, sy, ci, cj, ck);
    }
  });
}
template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI, bool HAS_V>
__device__ __forceinline__ void blend_staged(const EmArgs &A, const FlowSample<T, HAS_TE, HAS_Z, HAS_TI, true> &s, double &ne, double &Te,
                                             double &Z, double &Ti, double (&V)[3]) {
  blend_sample<T, HAS_TE, HAS_Z>(A, s.s, ne, Te, Z);
  Ti = Te;
  V[0] = V[1] = V[2] = 0.0;
  if (s.s.in) {
    const Sample<T, HAS_TE, HAS_Z> &c = s.s;
    if (HAS_TI) Ti = sr::corners_blend(s.Ti, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
    if (HAS_V) {
      V[0] = sr::corners_blend(s.V0, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
      V[1] = sr::corners_blend(s.V1, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
      V[2] = sr::corners_blend(s.V2, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
    }
  }
}

// ---- host: the chord frames, and the checks of a Zeeman table beyond check_voigt_table's

// F[9*i ..]: n^ = d*su, e1 = ref minus its part along n^, normalised, e2 = n^ x e1 -- the header's operations in its order.  Runs
// before check_lines (whose last word is on the fields): a direction that is zero or not finite is left for it to name.
inline int chord_frames(const char *who, int64_t n, int toward, const double *dir, const double *ref, std::vector<double> &F) {
  F.resize(9 * (size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const double d0 = dir[i], d1 = dir[n + i], d2 = dir[2 * n + i];
    const double r0 = ref[i], r1 = ref[n + i], r2 = ref[2 * n + i];
    if (!(std::isfinite(d0) && std::isfinite(d1) && std::isfinite(d2)) || (d0 == 0.0 && d1 == 0.0 && d2 == 0.0)) continue;
    SR_CHECK(std::isfinite(r0) && std::isfinite(r1) && std::isfinite(r2), "%s: non-finite ref of line %lld", who, (long long)i);
    const double su = (double)toward / sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    const double n0 = d0 * su, n1 = d1 * su, n2 = d2 * su;
    const double p = (r0 * n0 + r1 * n1) + r2 * n2;
    const double t0 = r0 - p * n0, t1 = r1 - p * n1, t2 = r2 - p * n2;
    const double t = sqrt((t0 * t0 + t1 * t1) + t2 * t2), rl = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
    SR_CHECK(t > kZeemanRefTol * rl, "%s: ref of line %lld is parallel to the chord (or zero)", who, (long long)i);
    const double u0 = t0 / t, u1 = t1 / t, u2 = t2 / t;
    double *f = F.data() + 9 * (size_t)i;
    f[0] = n0, f[1] = n1, f[2] = n2;
    f[3] = u0, f[4] = u1, f[5] = u2;
    f[6] = n1 * u2 - n2 * u1, f[7] = n2 * u0 - n0 * u2, f[8] = n0 * u1 - n1 * u0;
  }
  return SR_OK;
}

inline int check_zeeman_table(const char *who, const sr_zeeman_table *t) {
  SR_CHECK(t != nullptr, "%s: NULL line table", who);
  if (int rc = check_voigt_table(who, &t->voigt)) return rc;
  SR_CHECK(t->n_comp != nullptr && t->comp != nullptr, "%s: NULL component table (n_comp or comp)", who);
  const double *c = t->comp;
  for (int l = 0; l < t->voigt.lines.n_line; ++l) {
    const int nc = t->n_comp[l];
    SR_CHECK(nc >= 1 && nc <= SR_MAX_ZEEMAN, "%s: n_comp of line %d must be 1..%d, got %d", who, l, SR_MAX_ZEEMAN, nc);
    double sum[3] = {0.0, 0.0, 0.0};
    bool has[3] = {false, false, false};
    for (int k = 0; k < nc; ++k, c += 3) {
      SR_CHECK(c[0] == -1.0 || c[0] == 0.0 || c[0] == 1.0, "%s: q of component %d of line %d must be -1, 0 or +1", who, k, l);
      SR_CHECK(std::isfinite(c[1]), "%s: non-finite g of component %d of line %d", who, k, l);
      SR_CHECK(std::isfinite(c[2]) && c[2] > 0.0, "%s: s of component %d of line %d must be finite and positive", who, k, l);
      sum[(int)c[0] + 1] += c[2];
      has[(int)c[0] + 1] = true;
    }
    for (int q = 0; q < 3; ++q)
      SR_CHECK(!has[q] || std::fabs(sum[q] - 1.0) <= kZeemanGroupTol, "%s: the strengths of the q = %d group of line %d sum to %.17g, not 1",
               who, q - 1, l, sum[q]);
  }
  return SR_OK;
}
