// The tabulated node of include/synthray.h's table section: alpha [1/m] and S of one node from an opacity table, the policy
// emission_march.inc's kernels and sightlines.hip's kernel take as their last template argument.  Shared by emission_table.hip
// (sr_field_emission_table) and sightlines.hip (sr_field_sightlines with a table), so that the two cannot drift apart; with it go
// the host's checks of a table and its packing.  Included inside the including unit's anonymous namespace, after emission_march.inc
// (EmArgs, nmax).
//
// The host packs LT | LD | LA | LE (LE absent for LTE) into one run of float64.  Where that run is at most kLdsBudget bytes
// (64 KiB: what a workgroup may take without asking the runtime for more, and 2 workgroups of 256 to a CU when it is used in
// full -- one 10x10 band is 1.8 KB and costs no occupancy) every workgroup copies it into LDS once, before its first node, and the
// searches and the 8 gathered reads per band and table are LDS reads; a larger run is read where it lies, through L2
// (TableNode<false>).  A lane's two searches take a number of steps fixed by the lattice's size alone (at most 9: 512 nodes), every
// probe clamped into the lattice: no lane loops longer than another and no index leaves the table, NaN or not.

constexpr size_t kLdsBudget = 64 * 1024;
constexpr int kMaxLattice = 512;  // at most 9 search steps

struct TabArgs {
  const double *tab;  // device: LT[nT] | LD[nD] | LA[n_band][nT][nD] | LE[n_band][nT][nD] (has_le)
  int nT, nD, n_band, has_le;
  int words;          // float64 values in tab
  double m_ion;       // [g]
};

// numpy's minimum: a NaN operand gives NaN
__device__ __forceinline__ double nmin(double a, double b) { return (a < b || a != a) ? a : b; }

// The largest i in [0, n-2] with L[i] <= x (0 where there is none, or x is NaN) and the fraction of x in that cell clipped to
// [0, 1]: outside the lattice the edge value holds.  s0 = top_step(n): the search takes the same log2(s0) + 1 steps in every lane.
__device__ __forceinline__ int top_step(int n) {
  int s = 1;
  while (2 * s <= n - 2) s *= 2;
  return s;
}
__device__ __forceinline__ void locate(const double *L, int n, int s0, double x, int &i, double &f) {
  int lo = 0;
#pragma unroll 1
  for (int s = s0; s >= 1; s >>= 1) {
    const int c = lo + s;
    const double v = L[c <= n - 2 ? c : n - 2];
    lo = (c <= n - 2 && v <= x) ? c : lo;
  }
  i = lo;
  const double l0 = L[lo], l1 = L[lo + 1];
  f = nmin(nmax((x - l0) / (l1 - l0), 0.0), 1.0);
}

// sd, st: the strides of the density and the temperature index (1 and nD band by band, int; F and nD*F where the F groups are
// innermost, int64_t: nT*nD*F passes 2^31)
template <typename Ix>
__device__ __forceinline__ double bilinear(const double *T, Ix o, Ix sd, Ix st, double ft, double fd) {
  const double t00 = T[o], t01 = T[o + sd], t10 = T[o + st], t11 = T[o + st + sd];
  const double p0 = t00 + fd * (t01 - t00);
  const double p1 = t10 + fd * (t11 - t10);
  return p0 + ft * (p1 - p0);
}

// A node in two parts, as nrl_node.inc's: what every band shares (the two searches, dark, rho), then one band from its
// interpolated la = l(LA) and le = l(LE) (le is not used where has_le is false).
struct TableTerms {
  bool dark;  // Te <= 0, ne <= 0 or Z <= 0: alpha = S = 0
  int o;      // i*nD + j: the cell's first corner in a (nT, nD) band
  double Te, ft, fd, rho;
};
__device__ __forceinline__ TableTerms table_terms(const double *LT, int nT, int sT, const double *LD, int nD, int sD, double m_ion,
                                                  double ne, double Te, double Z) {
  TableTerms t;
  t.dark = Te <= 0.0 || ne <= 0.0 || Z <= 0.0;
  t.Te = Te;
  const double ni = (ne * 1e-6) / Z;
  int i, j;
  locate(LT, nT, sT, log(Te), i, t.ft);
  locate(LD, nD, sD, log(ni), j, t.fd);
  t.o = i * nD + j;
  t.rho = ni * m_ion;
  return t;
}
__device__ __forceinline__ void table_band(const TableTerms &t, double la, double le, bool has_le, double e_ph, double c_omega,
                                           double &al, double &S) {
  const double planck = c_omega / expm1(e_ph / t.Te);
  double s = planck;
  if (has_le) s = exp(le - la) * planck;
  al = t.dark ? 0.0 : (exp(la) * t.rho) * 100.0;
  S = t.dark ? 0.0 : s;
}

template <bool LDS>
struct TableNode {
  using Args = TabArgs;
  static constexpr int kXYBlock = 256;
  const double *LT, *LD, *LA, *LE;
  int nT, nD, sT, sD;  // lattice nodes; the searches' first steps
  bool has_le;  // false: LTE, LE is not read
  double m_ion;

  __device__ __forceinline__ explicit TableNode(const Args &X) {
    const double *base = X.tab;
    if constexpr (LDS) {
      extern __shared__ double s_tab[];
      for (int k = threadIdx.x; k < X.words; k += blockDim.x) s_tab[k] = X.tab[k];
      __syncthreads();
      base = s_tab;
    }
    nT = X.nT;
    nD = X.nD;
    sT = top_step(nT);
    sD = top_step(nD);
    m_ion = X.m_ion;
    LT = base;
    LD = LT + nT;
    LA = LD + nD;
    LE = LA + X.n_band * nT * nD;
    has_le = X.has_le != 0;
  }

  template <int NB>
  __device__ __forceinline__ void eval(const EmArgs &A, double ne, double Te, double Z, double (&al)[NB], double (&S)[NB]) const {
    const TableTerms t = table_terms(LT, nT, sT, LD, nD, sD, m_ion, ne, Te, Z);
    const int band = nT * nD;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const double la = bilinear(LA + b * band, t.o, 1, nD, t.ft, t.fd);
      const double le = has_le ? bilinear(LE + b * band, t.o, 1, nD, t.ft, t.fd) : 0.0;
      table_band(t, la, le, has_le, A.e_ph[b], A.c_omega[b], al[b], S[b]);
    }
  }
};

// ---- host: the checks of a table (`who` names the entry in the error text) and its packing
inline int check_lattice(const char *who, const char *name, const double *L, int n) {
  for (int k = 0; k < n; ++k) {
    SR_CHECK(std::isfinite(L[k]), "%s: %s[%d] is not finite", who, name, k);
    SR_CHECK(k == 0 || L[k] > L[k - 1], "%s: %s is not strictly increasing at %d", who, name, k);
  }
  return SR_OK;
}

inline int check_table(const char *who, const sr_emission_table *t, int n_band) {
  SR_CHECK(t != nullptr, "%s: NULL table", who);
  SR_CHECK(t->LT != nullptr && t->LD != nullptr && t->LA != nullptr, "%s: NULL table member (LT, LD or LA)", who);
  SR_CHECK(t->nT >= 2 && t->nT <= kMaxLattice, "%s: nT must be 2..%d, got %d", who, kMaxLattice, t->nT);
  SR_CHECK(t->nD >= 2 && t->nD <= kMaxLattice, "%s: nD must be 2..%d, got %d", who, kMaxLattice, t->nD);
  SR_CHECK(std::isfinite(t->m_ion) && t->m_ion > 0.0, "%s: m_ion must be finite and positive", who);
  if (int rc = check_lattice(who, "LT", t->LT, t->nT)) return rc;
  if (int rc = check_lattice(who, "LD", t->LD, t->nD)) return rc;
  const size_t band = (size_t)t->nT * t->nD, entries = band * n_band;
  for (size_t k = 0; k < entries; ++k) {
    SR_CHECK(std::isfinite(t->LA[k]), "%s: LA has a non-finite entry (band %d)", who, (int)(k / band));
    SR_CHECK(!t->LE || std::isfinite(t->LE[k]), "%s: LE has a non-finite entry (band %d)", who, (int)(k / band));
  }
  return SR_OK;
}

// LT | LD | LA | LE as the kernel reads them
inline std::vector<double> pack_table(const sr_emission_table *t, int n_band) {
  const size_t entries = (size_t)t->nT * t->nD * n_band;
  std::vector<double> pack;
  pack.reserve(t->nT + t->nD + entries * (t->LE ? 2 : 1));
  pack.insert(pack.end(), t->LT, t->LT + t->nT);
  pack.insert(pack.end(), t->LD, t->LD + t->nD);
  pack.insert(pack.end(), t->LA, t->LA + entries);
  if (t->LE) pack.insert(pack.end(), t->LE, t->LE + entries);
  return pack;
}

// the kernel's view of a packed table that lies at `tab` on the device
inline TabArgs tab_args(const sr_emission_table *t, int n_band, const char *tab, size_t words) {
  TabArgs X{};
  X.tab = reinterpret_cast<const double *>(tab);
  X.nT = t->nT;
  X.nD = t->nD;
  X.n_band = n_band;
  X.has_le = t->LE != nullptr;
  X.words = (int)words;
  X.m_ion = t->m_ion;
  return X;
}
