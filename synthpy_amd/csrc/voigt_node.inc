// The Voigt node of include/synthray.h's "Voigt lines along sightlines" section: the Voigt function V(a, x) = Re w(x + i a), the
// constants of one line at one sample with its damping parameter a (voigt_const: line_node.inc's line_const and one more bilinear
// read and exp), one frequency's term against the host's cut (voigt_term, voigt_outside), and on the host the checks and the
// packing of an sr_voigt_table.  Included inside the including unit's anonymous namespace, after line_node.inc.
//
// V has four regions in z2 = x*x + a*a and a; within a wavefront every lane has the same a (one sample, one line), so only the
// far / not far branch can diverge:
//   z2 >= 1e17 (or a NaN)   the leading term of the asymptotic series, ISP a / z2
//   z2 >= 100               Laplace's continued fraction, 10 levels, as ONE rational function: numerator and denominator by the
//                           backward recurrence (N, D) <- (z N - (k/2) D, N), one division at the end
//   a >= 2                  the same with 40 levels
//   a <= 0.5 | 0.5 < a < 2  Rybicki's sampling of Dawson's function at the complex argument, h = 1/4 with 13 pairs of terms | h = 3/16
//                           with 18: H = exp(a^2 - x^2) cos(2 a x) - (2/sqrt(pi)) Im F(z); the powers of exp(2 h z') by complex
//                           multiplication, a pair of terms n, -n over one denominator: three exp, three sin, three cos and 14 | 19
//                           divisions.  The smaller step keeps the aliasing term exp(-(pi/2h)^2 + pi a/h) below 1e-16 up to a = 2.
// No register arrays indexed at run time: the loops over the coefficient tables are unrolled, the coefficients are literals.

constexpr int kVoigtWords = 6;  // a staged line: wc, iw, aJ, aK, a and one of padding -- three 16-byte LDS reads

struct VoigtConst {
  double wc, iw, aJ, aK, a;
};

// Laplace's continued fraction of w(z), K levels, as one rational function
template <int K>
__device__ __forceinline__ double voigt_cf(double a, double x) {
  double Nr = x, Ni = a, Dr = 1.0, Di = 0.0;
#pragma unroll
  for (int k = K; k >= 1; --k) {
    const double c = 0.5 * k;
    const double tr = (Nr * x - Ni * a) - c * Dr;
    const double ti = (Nr * a + Ni * x) - c * Di;
    Dr = Nr, Di = Ni, Nr = tr, Ni = ti;
  }
  return (kLineISP * (Dr * Ni - Di * Nr)) / (Nr * Nr + Ni * Ni);
}

// Rybicki's sampling with step h (ih2 = 0.5/h as rounded, h2 = 2h) and the NP coefficients C[k] = exp(-((2k + 1) h)^2)
template <int NP>
__device__ __forceinline__ double voigt_sampled(double a, double x, double h, double ih2, double h2, const double (&C)[NP]) {
  const double n0 = 2.0 * rint(ih2 * x);
  const double xp = x - h * n0;
  const double a2 = a * a;
  const double g = exp(a2 - xp * xp);
  const double th = (2.0 * a) * xp;
  const double Gr = g * cos(th), Gi = -(g * sin(th));
  const double pe = exp(h2 * xp);
  const double me = 1.0 / pe;
  const double ca = cos(h2 * a), sa = sin(h2 * a);
  double pr = pe * ca, pi = pe * sa, mr = me * ca, mi = -(me * sa);
  const double p2r = pr * pr - pi * pi, p2i = (2.0 * pr) * pi;
  const double m2r = mr * mr - mi * mi, m2i = (2.0 * mr) * mi;
  const double d0 = n0 * n0;
  double Sr = 0.0, Si = 0.0;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const double n = 2 * k + 1;
    const double q = C[k] / (d0 - n * n);
    Sr = Sr + q * (pr * (n0 - n) + mr * (n0 + n));
    Si = Si + q * (pi * (n0 - n) + mi * (n0 + n));
    const double tp = pr * p2r - pi * p2i, tm = mr * m2r - mi * m2i;
    pi = pr * p2i + pi * p2r, mi = mr * m2i + mi * m2r;
    pr = tp, mr = tm;
  }
  const double imF = (Gr * Si + Gi * Sr) * kLineISP;
  return exp(a2 - x * x) * cos((2.0 * a) * x) - (2.0 * kLineISP) * imF;
}

// V(a, x): the header's algorithm, region by region
__device__ __forceinline__ double voigt(double a, double x) {
  const double z2 = x * x + a * a;
  if (!(z2 < 1e17)) return (kLineISP * a) / z2;
  if (z2 >= 100.0) return voigt_cf<10>(a, x);
  if (a >= 2.0) return voigt_cf<40>(a, x);
  if (a <= 0.5) {
    constexpr double C[13] = {0.9394130628134758,     0.569782824730923,      0.2096113871510978,     0.04677062238395898,
                              0.006329715427485747,   0.0005195746821548384,  2.586810022265412e-05,  7.811489408304491e-07,
                              1.4307241918567688e-08, 1.5893910094516368e-10, 1.0709232382508077e-12, 4.37661850287085e-15,
                              1.0848552640429378e-17};
    return voigt_sampled<13>(a, x, 0.25, 2.0, 0.5, C);
  }
  constexpr double C[18] = {0.9654545521978378,     0.7287633299194912,     0.4152368286818413,     0.17859113461243561,
                            0.0579800525002544,     0.014208622931196246,   0.002628330960567707,   0.0003669972327972938,
                            3.8681223753184774e-05, 3.0774591584232196e-06, 1.8481578772048032e-07, 8.378003053124454e-09,
                            2.866794996873118e-10,  7.404699497933558e-12,  1.4436865682659833e-13, 2.1246777523216493e-15,
                            2.3603037795421644e-17, 1.9792352186549065e-19};
  return voigt_sampled<18>(a, x, 0.1875, 2.6666666666666665, 0.375, C);
}

// ---- the whole of w(x + i a): H = Re w with voigt()'s operations and bits, L = Im w (the dispersion profile) from the same
// intermediates (include/synthray.h's "Polarised transfer along sightlines" section).  voigt() and what it calls stay as they are.
template <int K>
__device__ __forceinline__ void voigt_cf_w(double a, double x, double &H, double &L) {
  double Nr = x, Ni = a, Dr = 1.0, Di = 0.0;
#pragma unroll
  for (int k = K; k >= 1; --k) {
    const double c = 0.5 * k;
    const double tr = (Nr * x - Ni * a) - c * Dr;
    const double ti = (Nr * a + Ni * x) - c * Di;
    Dr = Nr, Di = Ni, Nr = tr, Ni = ti;
  }
  const double den = Nr * Nr + Ni * Ni;
  H = (kLineISP * (Dr * Ni - Di * Nr)) / den;
  L = (kLineISP * (Dr * Nr + Di * Ni)) / den;
}

template <int NP>
__device__ __forceinline__ void voigt_sampled_w(double a, double x, double h, double ih2, double h2, const double (&C)[NP], double &H,
                                                double &L) {
  const double n0 = 2.0 * rint(ih2 * x);
  const double xp = x - h * n0;
  const double a2 = a * a;
  const double g = exp(a2 - xp * xp);
  const double th = (2.0 * a) * xp;
  const double Gr = g * cos(th), Gi = -(g * sin(th));
  const double pe = exp(h2 * xp);
  const double me = 1.0 / pe;
  const double ca = cos(h2 * a), sa = sin(h2 * a);
  double pr = pe * ca, pi = pe * sa, mr = me * ca, mi = -(me * sa);
  const double p2r = pr * pr - pi * pi, p2i = (2.0 * pr) * pi;
  const double m2r = mr * mr - mi * mi, m2i = (2.0 * mr) * mi;
  const double d0 = n0 * n0;
  double Sr = 0.0, Si = 0.0;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const double n = 2 * k + 1;
    const double q = C[k] / (d0 - n * n);
    Sr = Sr + q * (pr * (n0 - n) + mr * (n0 + n));
    Si = Si + q * (pi * (n0 - n) + mi * (n0 + n));
    const double tp = pr * p2r - pi * p2i, tm = mr * m2r - mi * m2i;
    pi = pr * p2i + pi * p2r, mi = mr * m2i + mi * m2r;
    pr = tp, mr = tm;
  }
  const double imF = (Gr * Si + Gi * Sr) * kLineISP;
  const double reF = (Gr * Sr - Gi * Si) * kLineISP;
  const double e = exp(a2 - x * x), t2 = (2.0 * a) * x;
  H = e * cos(t2) - (2.0 * kLineISP) * imF;
  L = (2.0 * kLineISP) * reF - e * sin(t2);
}

__device__ __forceinline__ void voigt_w(double a, double x, double *H, double *L) {
  const double z2 = x * x + a * a;
  if (!(z2 < 1e17)) {
    *H = (kLineISP * a) / z2;
    *L = (kLineISP * x) / z2;
  } else if (z2 >= 100.0) {
    voigt_cf_w<10>(a, x, *H, *L);
  } else if (a >= 2.0) {
    voigt_cf_w<40>(a, x, *H, *L);
  } else if (a <= 0.5) {
    constexpr double C[13] = {0.9394130628134758,     0.569782824730923,      0.2096113871510978,     0.04677062238395898,
                              0.006329715427485747,   0.0005195746821548384,  2.586810022265412e-05,  7.811489408304491e-07,
                              1.4307241918567688e-08, 1.5893910094516368e-10, 1.0709232382508077e-12, 4.37661850287085e-15,
                              1.0848552640429378e-17};
    voigt_sampled_w<13>(a, x, 0.25, 2.0, 0.5, C, *H, *L);
  } else {
    constexpr double C[18] = {0.9654545521978378,     0.7287633299194912,     0.4152368286818413,     0.17859113461243561,
                              0.0579800525002544,     0.014208622931196246,   0.002628330960567707,   0.0003669972327972938,
                              3.8681223753184774e-05, 3.0774591584232196e-06, 1.8481578772048032e-07, 8.378003053124454e-09,
                              2.866794996873118e-10,  7.404699497933558e-12,  1.4436865682659833e-13, 2.1246777523216493e-15,
                              2.3603037795421644e-17, 1.9792352186549065e-19};
    voigt_sampled_w<18>(a, x, 0.1875, 2.6666666666666665, 0.375, C, *H, *L);
  }
}

// line_const's four and a = gam*iw, gam = exp(l(LG)): LG is packed line-innermost as LJ and LK are
__device__ __forceinline__ VoigtConst voigt_const(double w0, double ci, const double *LJ, const double *LK, const double *LG, bool has_lk,
                                                  int o, int sd, int st, double ft, double fd, double beta, double Ti) {
  const LineConst k = line_const(w0, ci, LJ, LK, has_lk, o, sd, st, ft, fd, beta, Ti);
  VoigtConst v;
  v.wc = k.wc, v.iw = k.iw, v.aJ = k.aJ, v.aK = k.aK;
  v.a = exp(bilinear(LG, o, sd, st, ft, fd)) * k.iw;
  return v;
}

// line_outside against the host's cut = wing*wing (+inf: nothing is outside); a NaN wc or iw skips nothing
__device__ __forceinline__ bool voigt_outside(double wc, double iw, double wmin, double wmax, double cut) {
  const double xa = (wmax - wc) * iw, xb = (wmin - wc) * iw;
  return (xa < 0.0 && xa * xa > cut) || (xb > 0.0 && xb * xb > cut);
}

// one line's term at one frequency: dropped (false) when x*x > cut; a NaN is not dropped
__device__ __forceinline__ bool voigt_term(double omega, double wc, double iw, double cut, double &x) {
  x = (omega - wc) * iw;
  return !(x * x > cut);
}

// ---- host: the checks of a Voigt table beyond check_line_table's, and its packing
inline int check_voigt_table(const char *who, const sr_voigt_table *t) {
  SR_CHECK(t != nullptr, "%s: NULL line table", who);
  if (int rc = check_line_table(who, &t->lines)) return rc;
  if (t->LG) {
    const size_t cells = (size_t)t->lines.nT * t->lines.nD, entries = cells * t->lines.n_line;
    for (size_t k = 0; k < entries; ++k)
      SR_CHECK(std::isfinite(t->LG[k]), "%s: LG has a non-finite entry (line %d)", who, (int)(k / cells));
  }
  return SR_OK;
}

// pack_line_table's block, then LG[nT][nD][n_line] where LG is given
inline std::vector<double> pack_voigt_table(const sr_voigt_table *t) {
  std::vector<double> pack = pack_line_table(&t->lines);
  if (!t->LG) return pack;
  const size_t cells = (size_t)t->lines.nT * t->lines.nD, nl = (size_t)t->lines.n_line, at = pack.size();
  pack.resize(at + cells * nl);
  double *q = pack.data() + at;
  for (size_t l = 0; l < nl; ++l)
    for (size_t k = 0; k < cells; ++k) q[k * nl + l] = t->LG[l * cells + k];
  return pack;
}
