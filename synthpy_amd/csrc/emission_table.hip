// Self-emission from tabulated opacities (sr_field_emission_table; include/synthray.h states the rule): emission_march.inc's
// march with a node whose absorption and emission opacities are interpolated, bilinearly in (log Te, log ni) on the logarithms of
// the table, from a temperature x ion-density lattice (PROPACEOS tables, or anything laid out that way).
//
// The host packs LT | LD | LA | LE (LE absent for LTE) into one run of float64 behind the maps.  Where that run is at most
// kLdsBudget bytes (64 KiB: what a workgroup may take without asking the runtime for more, and 2 workgroups of 256 to a CU when it
// is used in full -- one 10x10 band is 1.8 KB and costs no occupancy) every workgroup copies it into LDS once, before its first
// node, and the searches and the 8 gathered reads per band and table are LDS reads; a larger run is read where it lies, through L2
// (TableNode<false>).  k_emission_xy runs 256-lane workgroups here, not the NRL node's 64: a workgroup stages the table once for
// its 256 columns (for 512^2 columns 1024 copies of the table come out of L2, not 4096); k_emission_z's 256-lane workgroups stride
// over the columns, so there a copy serves ncol / grid columns.  A lane's two searches take a number of steps fixed by the lattice's
// size alone (at most 9: 512 nodes), every probe clamped into the lattice: no lane loops longer than another and no index leaves the table, NaN
// or not.  No scratch, no atomics.  Compiled with -ffp-contract=off.
#include <vector>

#include "emission_march.inc"

namespace {

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

__device__ __forceinline__ double bilinear(const double *T, int o, int nD, double ft, double fd) {
  const double t00 = T[o], t01 = T[o + 1], t10 = T[o + nD], t11 = T[o + nD + 1];
  const double p0 = t00 + fd * (t01 - t00);
  const double p1 = t10 + fd * (t11 - t10);
  return p0 + ft * (p1 - p0);
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
    const bool dark = Te <= 0.0 || ne <= 0.0 || Z <= 0.0;
    const double ni = (ne * 1e-6) / Z;
    int i, j;
    double ft, fd;
    locate(LT, nT, sT, log(Te), i, ft);
    locate(LD, nD, sD, log(ni), j, fd);
    const int o = i * nD + j, band = nT * nD;
    const double rho = ni * m_ion;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const double la = bilinear(LA + b * band, o, nD, ft, fd);
      const double planck = A.c_omega[b] / expm1(A.e_ph[b] / Te);
      double s = planck;
      if (has_le) s = exp(bilinear(LE + b * band, o, nD, ft, fd) - la) * planck;
      al[b] = dark ? 0.0 : (exp(la) * rho) * 100.0;
      S[b] = dark ? 0.0 : s;
    }
  }
};

int check_lattice(const char *name, const double *L, int n) {
  for (int k = 0; k < n; ++k) {
    SR_CHECK(std::isfinite(L[k]), "sr_field_emission_table: %s[%d] is not finite", name, k);
    SR_CHECK(k == 0 || L[k] > L[k - 1], "sr_field_emission_table: %s is not strictly increasing at %d", name, k);
  }
  return SR_OK;
}

}  // namespace

extern "C" int sr_field_emission_table(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_table *t,
                                       const sr_emission_params *p, const double *backlight, double *I, double *tau,
                                       double *kernel_ms) {
  SR_CHECK(p != nullptr && I != nullptr && tau != nullptr, "sr_field_emission_table: NULL argument");
  SR_CHECK(p->n_band >= 1 && p->n_band <= SR_MAX_BANDS, "sr_field_emission_table: n_band must be 1..%d, got %d", SR_MAX_BANDS,
           p->n_band);
  for (int b = 0; b < p->n_band; ++b)
    SR_CHECK(std::isfinite(p->e_ph[b]) && std::isfinite(p->c_omega[b]), "sr_field_emission_table: non-finite e_ph or c_omega of band %d",
             b);
  SR_CHECK(t != nullptr, "sr_field_emission_table: NULL table");
  SR_CHECK(t->LT != nullptr && t->LD != nullptr && t->LA != nullptr, "sr_field_emission_table: NULL table member (LT, LD or LA)");
  SR_CHECK(t->nT >= 2 && t->nT <= kMaxLattice, "sr_field_emission_table: nT must be 2..%d, got %d", kMaxLattice, t->nT);
  SR_CHECK(t->nD >= 2 && t->nD <= kMaxLattice, "sr_field_emission_table: nD must be 2..%d, got %d", kMaxLattice, t->nD);
  SR_CHECK(std::isfinite(t->m_ion) && t->m_ion > 0.0, "sr_field_emission_table: m_ion must be finite and positive");
  if (int rc = check_lattice("LT", t->LT, t->nT)) return rc;
  if (int rc = check_lattice("LD", t->LD, t->nD)) return rc;
  const size_t band = (size_t)t->nT * t->nD, entries = band * p->n_band;
  for (size_t k = 0; k < entries; ++k) {
    SR_CHECK(std::isfinite(t->LA[k]), "sr_field_emission_table: LA has a non-finite entry (band %d)", (int)(k / band));
    SR_CHECK(!t->LE || std::isfinite(t->LE[k]), "sr_field_emission_table: LE has a non-finite entry (band %d)", (int)(k / band));
  }
  if (int rc = check_fields("sr_field_emission_table", ne, Te, Z, p)) return rc;

  std::vector<double> pack;
  pack.reserve(t->nT + t->nD + entries * (t->LE ? 2 : 1));
  pack.insert(pack.end(), t->LT, t->LT + t->nT);
  pack.insert(pack.end(), t->LD, t->LD + t->nD);
  pack.insert(pack.end(), t->LA, t->LA + entries);
  if (t->LE) pack.insert(pack.end(), t->LE, t->LE + entries);
  const size_t tab_bytes = sizeof(double) * pack.size();

  EmArgs A;
  size_t map_bytes = 0;
  char *tab = nullptr;
  if (int rc = prepare(ne, Te, Z, p, backlight, tab_bytes, A, map_bytes, &tab)) return rc;
  sr::Context &c = sr::ctx();
  SR_HIP(hipMemcpyAsync(tab, pack.data(), tab_bytes, hipMemcpyHostToDevice, c.stream));
  TabArgs X{};
  X.tab = reinterpret_cast<const double *>(tab);
  X.nT = t->nT;
  X.nD = t->nD;
  X.n_band = p->n_band;
  X.has_le = t->LE != nullptr;
  X.words = (int)pack.size();
  X.m_ion = t->m_ion;
  const bool lds = tab_bytes <= kLdsBudget;
  SR_HIP(hipEventRecord(c.ev[0], c.stream));
  sr::with_flags(
      [&](auto in_lds, auto f64) {
        using T = std::conditional_t<decltype(f64)::value, double, float>;
        constexpr bool kLds = decltype(in_lds)::value;
        launch<T, TableNode<kLds>>(A, X, kLds ? tab_bytes : 0, p->axis, Te != nullptr, Z != nullptr, p->n_band, c.stream);
      },
      lds, (bool)ne->is_f64);
  return finish(A, map_bytes, I, tau, kernel_ms);
}
