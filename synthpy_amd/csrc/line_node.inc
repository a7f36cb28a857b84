// The spectral-line node of include/synthray.h's line-spectra section: what a Doppler-shifted, thermally broadened line adds to
// the emission and absorption coefficient of one sample at one frequency, in three parts as nrl_node.inc's and table_node.inc's
// nodes are: what a sample gives every line (the lattice search: table_node.inc's table_terms; beta), the constants of one line at
// that sample (line_const: centre, inverse width, peak emission and absorption), and one frequency's term (line_term).  With them
// the sample's update (line_update), the wavefront's least and greatest frequency for the skip of a whole line (wave_extreme: the
// family's one definition) and, on the host, the checks and the packing of a line table.  Included inside the including
// unit's anonymous namespace, after table_node.inc (bilinear, check_lattice, kMaxLattice).

constexpr double kLineE = 1.602176634e-19, kLineMp = 1.67262192369e-27, kLineISP = 0.5641895835477563;
constexpr double kLineCut = 40.0;  // a term with x*x above it is dropped: exp(-40) = 4e-18 of the line's peak

// The constants of one line at one sample, as they lie in LDS: four float64, a line after a line
struct LineConst {
  double wc, iw, aJ, aK;
};
constexpr int kLineWords = 4;

// LJ, LK: the tables line-innermost, (nT, nD, n_line); o = (i*nD + j)*n_line + l: the cell's first corner of line l.  LK is not
// read where has_lk is false.
__device__ __forceinline__ LineConst line_const(double w0, double ci, const double *LJ, const double *LK, bool has_lk, int o, int sd,
                                                int st, double ft, double fd, double beta, double Ti) {
  LineConst k;
  k.wc = w0 * (1.0 + beta);
  const double wd = w0 * (sqrt(ci * Ti) / sr::kC);
  k.iw = 1.0 / wd;
  const double g = kLineISP * k.iw;
  k.aJ = exp(bilinear(LJ, o, sd, st, ft, fd)) * g;
  k.aK = has_lk ? exp(bilinear(LK, o, sd, st, ft, fd)) * g : 0.0;
  return k;
}

// Is every frequency in [wmin, wmax] outside the line's window?  x = (omega - wc)*iw and x*x are monotone in omega as they are
// rounded (iw >= 0), so the two ends decide for all that lie between, exactly: no term this skips would have been counted.  A NaN
// wc or iw skips nothing.
__device__ __forceinline__ bool line_outside(double wc, double iw, double wmin, double wmax) {
  const double xa = (wmax - wc) * iw, xb = (wmin - wc) * iw;
  return (xa < 0.0 && xa * xa > kLineCut) || (xb > 0.0 && xb * xb > kLineCut);
}

// one line's term at one frequency: dropped (false) when x*x > 40; a NaN is not dropped
__device__ __forceinline__ bool line_term(double omega, double wc, double iw, double &x2) {
  const double x = (omega - wc) * iw;
  x2 = x * x;
  return !(x2 > kLineCut);
}

// The update of (I, tau) by one sample whose lines gave (j, aL) at this frequency on the continuum (ac, Sc)
__device__ __forceinline__ void line_update(double ac, double Sc, double j, double aL, double h, double &I, double &tau) {
  const double a = ac + aL;
  const double dtau = a * h;
  if (dtau == 0.0) {
    I = I + j * h;
  } else {  // dtau > 0, or a NaN, which this makes of I and of tau
    I = I * exp(-dtau) + ((ac * Sc + j) / a) * (-expm1(-dtau));
    tau = tau + dtau;
  }
}

// the least (LEAST) or the greatest value of a wavefront, in every lane
template <bool LEAST>
__device__ __forceinline__ double wave_extreme(double v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double o = __shfl_xor(v, s, 64);
    v = LEAST ? (o < v ? o : v) : (o > v ? o : v);
  }
  return v;
}

// ---- host: the checks of a line table (`who` names the entry in the error text) and its packing
inline int check_line_table(const char *who, const sr_line_table *t) {
  SR_CHECK(t != nullptr, "%s: NULL line table", who);
  SR_CHECK(t->LT != nullptr && t->LD != nullptr && t->w0 != nullptr && t->A != nullptr && t->LJ != nullptr,
           "%s: NULL line-table member (LT, LD, w0, A or LJ)", who);
  SR_CHECK(t->n_line >= 1 && t->n_line <= SR_MAX_LINES, "%s: n_line must be 1..%d, got %d", who, SR_MAX_LINES, t->n_line);
  SR_CHECK(t->nT >= 2 && t->nT <= kMaxLattice, "%s: nT must be 2..%d, got %d", who, kMaxLattice, t->nT);
  SR_CHECK(t->nD >= 2 && t->nD <= kMaxLattice, "%s: nD must be 2..%d, got %d", who, kMaxLattice, t->nD);
  for (int l = 0; l < t->n_line; ++l) {
    SR_CHECK(std::isfinite(t->w0[l]) && t->w0[l] > 0.0, "%s: w0 of line %d must be finite and positive", who, l);
    SR_CHECK(std::isfinite(t->A[l]) && t->A[l] > 0.0, "%s: A of line %d must be finite and positive", who, l);
  }
  if (int rc = check_lattice(who, "LT", t->LT, t->nT)) return rc;
  if (int rc = check_lattice(who, "LD", t->LD, t->nD)) return rc;
  const size_t cells = (size_t)t->nT * t->nD, entries = cells * t->n_line;
  for (size_t k = 0; k < entries; ++k) {
    SR_CHECK(std::isfinite(t->LJ[k]), "%s: LJ has a non-finite entry (line %d)", who, (int)(k / cells));
    SR_CHECK(!t->LK || std::isfinite(t->LK[k]), "%s: LK has a non-finite entry (line %d)", who, (int)(k / cells));
  }
  return SR_OK;
}

// LT | LD | w0 | ci | LJ[nT][nD][n_line] | LK[nT][nD][n_line] (where given) as the kernel reads them: ci = (2e)/(A m_p) per line
inline std::vector<double> pack_line_table(const sr_line_table *t) {
  const size_t cells = (size_t)t->nT * t->nD, nl = (size_t)t->n_line;
  std::vector<double> pack((size_t)t->nT + t->nD + 2 * nl + cells * nl * (t->LK ? 2 : 1));
  double *q = pack.data();
  q = std::copy(t->LT, t->LT + t->nT, q);
  q = std::copy(t->LD, t->LD + t->nD, q);
  q = std::copy(t->w0, t->w0 + nl, q);
  for (size_t l = 0; l < nl; ++l) *q++ = (2.0 * kLineE) / (t->A[l] * kLineMp);
  for (const double *src : {t->LJ, t->LK}) {
    if (!src) continue;
    for (size_t l = 0; l < nl; ++l)
      for (size_t k = 0; k < cells; ++k) q[k * nl + l] = src[l * cells + k];
    q += cells * nl;
  }
  return pack;
}
