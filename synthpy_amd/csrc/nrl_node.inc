// The NRL (inverse-bremsstrahlung) node of include/synthray.h's self-emission section: alpha [1/m] and the Planck S of one node.
// Shared by emission.hip (sr_field_emission: every band of a node) and wave.hip (sr_field_wave: the absorption of a screen), so
// that the two cannot drift apart.  Included inside the including unit's anonymous namespace, after common.hpp.

// numpy's maximum: a NaN operand gives NaN
__device__ __forceinline__ double nmax(double a, double b) { return (a > b || a != a) ? a : b; }

// alpha [1/m] and S of one node: what every band shares, then one band.  A dark node's zeros are selected at the end; an early
// return here left the callers' per-band arrays in scratch.
struct NodeTerms {
  bool dark;  // Te <= 0 or ne <= 0: alpha = S = 0
  double Te, n, wp, L, num, zc, it;
};
__device__ __forceinline__ NodeTerms node_terms(double ne, double Te, double Z) {
  NodeTerms t;
  const double q = sqrt(Te);
  t.dark = Te <= 0.0 || ne <= 0.0;
  t.Te = Te;
  t.n = ne * 1e-6;
  t.wp = 5.64e4 * sqrt(t.n);
  t.L = nmax(Z * 1.602176634e-19 / Te, 2.760428269727312e-10 / q);
  t.num = 4.19e5 * q;
  t.zc = (3.1e-5 * Z) * sr::kC;
  t.it = 1.0 / (Te * q);
  return t;
}
// alpha of one band alone
__device__ __forceinline__ double node_alpha(const NodeTerms &t, double omega) {
  const double w = nmax(t.wp, omega);
  const double lnL = nmax(2.0, log(t.num / (w * t.L)));
  const double r = t.n / omega;
  return t.dark ? 0.0 : (((t.zc * (r * r)) * lnL) * t.it) / sr::kC;
}
__device__ __forceinline__ void node_band(const NodeTerms &t, double omega, double e_ph, double c_omega, double &al, double &S) {
  al = node_alpha(t, omega);
  S = t.dark ? 0.0 : c_omega / expm1(e_ph / t.Te);
}
