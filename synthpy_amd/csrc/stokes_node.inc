// The Stokes node of include/synthray.h's "Polarised transfer along sightlines" section: what a line's six profile sums (P0, Pp, Pm
// of H = Re w and R0, Rp, Rm of L = Im w: voigt_node.inc's voigt_w) add to the sample's emission, absorption and rotation
// coefficients (stokes_line: zeeman_line's operations for jI .. jV and aL = hI, and the same sums for the other six), and the update
// of (I, Q, U, Vs, tau) with the 4 x 4 absorption matrix K (stokes_update: X <- exp(-K h) X + (int_0^h exp(-K s) ds) eps by scaling
// and squaring, +, -, *, / only).  Included inside the including unit's anonymous namespace, after zeeman_node.inc.

constexpr int kStokesWords = 8;        // what a staged sample's head gains: zeeman_node.inc's six, B.n^, and one of padding
constexpr double kStokesTheta = 0.25;  // the scaled step has (row-sum norm of K)*h' <= theta
constexpr int kStokesOrder = 13;       // Horner Taylor sums of this order: theta^14/14! = 4.3e-20, under u/4 = 2.8e-17
constexpr double kStokesEps0 = 8.8541878128e-12, kStokesC = 299792458.0;
constexpr double kStokesPolTol = 1e-12;  // a pol whose squares sum to at most 1 + this is inside the unit ball: a unit vector as rounded

// zeeman_line, and the same sums with aK for (hQ, hU, hV) and with (R0, Rp, Rm) for (rQ, rU, rV); hI is zeeman_line's aL.  The
// rotation coefficients carry the sign +1 (the header derives it from its anchors).
__device__ __forceinline__ void stokes_line(const ZeemanSample &z, double aJ, double aK, double P0, double Pp, double Pm, double R0,
                                            double Rp, double Rm, double &jI, double &jQ, double &jU, double &jV, double &hI, double &hQ,
                                            double &hU, double &hV, double &rQ, double &rU, double &rV) {
  const double Ps = Pp + Pm;
  const double eI = 0.5 * (z.sP * P0) + (0.5 * z.cS) * Ps;
  const double eP = 0.5 * (P0 - 0.5 * Ps);
  const double eV = 0.5 * (Pp - Pm);
  const double Rs = Rp + Rm;
  const double fP = 0.5 * (R0 - 0.5 * Rs);
  const double fV = 0.5 * (Rp - Rm);
  jI = jI + aJ * eI;
  jQ = jQ + aJ * (eP * z.cQ);
  jU = jU + aJ * (eP * z.cU);
  jV = jV + aJ * (eV * z.cV);
  hI = hI + aK * eI;
  hQ = hQ + aK * (eP * z.cQ);
  hU = hU + aK * (eP * z.cU);
  hV = hV + aK * (eV * z.cV);
  rQ = rQ + aK * (fP * z.cQ);
  rU = rU + aK * (fP * z.cU);
  rV = rV + aK * (fV * z.cV);
}

// X <- O X + p over one sample of length h with constant coefficients.  Every array below is indexed by constants after the
// unrolling: registers.  Returns s, the number of squarings.
__device__ __forceinline__ int stokes_update(double ac, double Sc, double jI, double jQ, double jU, double jV, double hI, double hQ,
                                             double hU, double hV, double rQ, double rU, double rV, double h, double &I, double &Q,
                                             double &U, double &Vs, double &tau) {
  const double eI = ac + hI;
  const double K[16] = {eI, hQ, hU, hV, hQ, eI, rV, -rU, hU, -rV, eI, rQ, hV, rU, -rQ, eI};
  double nrm = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double r = ((fabs(K[4 * i]) + fabs(K[4 * i + 1])) + fabs(K[4 * i + 2])) + fabs(K[4 * i + 3]);
    if (i == 0 || r > nrm) nrm = r;
  }
  double t = nrm * h, hs = h;
  int s = 0;
  if (t <= 1.7976931348623157e308) {  // a NaN or an infinite norm takes s = 0 and makes NaN of all five
#pragma unroll 1
    while (t > kStokesTheta) {
      t = 0.5 * t;
      hs = 0.5 * hs;
      ++s;
    }
  }
  // the seven numbers of A = -K h' and b = eps h'
  const double g0 = -(eI * hs), gQ = -(hQ * hs), gU = -(hU * hs), gV = -(hV * hs), fQ = -(rQ * hs), fU = -(rU * hs), fV = -(rV * hs);
  const double b[4] = {(ac * Sc + jI) * hs, jQ * hs, jU * hs, jV * hs};
  double O[16] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  double p[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int k = kStokesOrder; k >= 1; --k) {
    const double c = (double)k;
    const double a0 = g0 / c, aQ = gQ / c, aU = gU / c, aV = gV / c, cQ = fQ / c, cU = fU / c, cV = fV / c;
    const double A[16] = {a0, aQ, aU, aV, aQ, a0, cV, -cU, aU, -cV, a0, cQ, aV, cU, -cQ, a0};
    double N[16], q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        N[4 * i + j] = ((A[4 * i] * O[j] + A[4 * i + 1] * O[4 + j]) + A[4 * i + 2] * O[8 + j]) + A[4 * i + 3] * O[12 + j];
      q[i] = (((A[4 * i] * p[0] + A[4 * i + 1] * p[1]) + A[4 * i + 2] * p[2]) + A[4 * i + 3] * p[3]) + b[i] / c;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) O[i] = (i % 5 == 0) ? 1.0 + N[i] : N[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = q[i];
  }
#pragma unroll 1
  for (int m = 0; m < s; ++m) {
    double N[16], q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      q[i] = p[i] + (((O[4 * i] * p[0] + O[4 * i + 1] * p[1]) + O[4 * i + 2] * p[2]) + O[4 * i + 3] * p[3]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        N[4 * i + j] = ((O[4 * i] * O[j] + O[4 * i + 1] * O[4 + j]) + O[4 * i + 2] * O[8 + j]) + O[4 * i + 3] * O[12 + j];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) O[i] = N[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = q[i];
  }
  const double X[4] = {I, Q, U, Vs};
  double Y[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) Y[i] = (((O[4 * i] * X[0] + O[4 * i + 1] * X[1]) + O[4 * i + 2] * X[2]) + O[4 * i + 3] * X[3]) + p[i];
  I = Y[0], Q = Y[1], U = Y[2], Vs = Y[3];
  tau = tau + eI * h;
  return s;
}
