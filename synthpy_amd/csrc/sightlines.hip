// Sightlines: emission and absorption along arbitrary chords (sr_field_sightlines; include/synthray.h states the rule every line
// and sample follows, operation for operation).  No reference counterpart.  The radiative-transfer recurrence of emission.hip
// marched along lines that are not grid columns: a pinhole camera's converging lines, a point backlighter's diverging ones, a
// diode's single chord.
//
// One line per lane, 256-lane workgroups; the line's geometry, its running (I, tau, column) and the sample in flight stay in
// registers for the whole march: no scratch, no atomics, and LDS only where the tabulated node stages its table.  The node is the
// policy emission_march.inc's kernels take (NrlNode there, TableNode in table_node.inc: one copy each), the cell search and the
// blend are common.hpp's (sr::locate_in, sr::corners_load / corners_blend, shared with resample.hip, push.hip and thomson.hip).
// The kernel is a gather: 8 corners times up to 3 fields per sample, at addresses that depend on the line.  A sample's cell search
// and its corner reads are issued BEFORE the node arithmetic of the sample before it (two logs, an exp and an expm1 per band), so
// the reads' latency runs under that arithmetic, as k_emission_xy keeps two planes in flight.  Lanes of a wavefront finish at
// different step counts: a lane that is done is masked off, there are no cross-lane operations inside the loop.  Which lines share a
// wavefront -- the locality of the gather -- is the caller's business (synthpy_amd/sightlines.py hands a pixel grid over in 8x8
// tiles in Morton order).  k_sightlines is instantiated per (dtype, Te field?, Z field?, bands, node).  This unit holds the kernel,
// its dispatch and the entry; what the entry does around the launch is sightline_march.inc's host section, shared with
// sightline_spectra.hip, emission_march.inc's (bands, EmArgs) and table_node.inc's (the table's checks and band-major packing).
// Compiled with -ffp-contract=off: products and sums round separately, as the NumPy restatement's do (tests/test_sightlines.py).
#include <cstdlib>
#include <vector>

#include "emission_march.inc"

namespace {
#include "table_node.inc"

#include "sightline_march.inc"  // LineArgs, Sample, fetch, the clip and the step count; the host code around the kernel

template <typename T, bool HAS_TE, bool HAS_Z, int NB, typename P>
__global__ void __launch_bounds__(256) k_sightlines(EmArgs A, LineArgs L, typename P::Args X) {
  const P node(X);  // every thread of the workgroup, before any leaves
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= L.n) return;
  const int64_t N = L.n;
  double I[NB], tau[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    I[k] = A.back ? A.back[k * N + i] : 0.0;
    tau[k] = 0.0;
  }
  const Line l = line_of(L, i);
  const double chord = l.chord;
  const int n = l.n;
  double column = 0.0;
  if (l.hit) {
    const double h = l.h;
    const int64_t sy = L.f.n[2], sx = (int64_t)L.f.n[1] * sy;
    const int k0 = A.toward > 0 ? 0 : n - 1, dk = A.toward > 0 ? 1 : -1;
    Sample<T, HAS_TE, HAS_Z> cur{}, nxt{};
    fetch_sample<T, HAS_TE, HAS_Z>(A, L.f, sx, sy, l, k0, cur);
    for (int m = 0; m < n; ++m) {
      // this sample's values (its reads were issued a sample ago) ...
      double ne, Te, Z;
      blend_sample<T, HAS_TE, HAS_Z>(A, cur, ne, Te, Z);
      // ... the next sample's cell and corner reads, in flight during this sample's node arithmetic ...
      nxt.in = false;
      if (m + 1 < n) fetch_sample<T, HAS_TE, HAS_Z>(A, L.f, sx, sy, l, k0 + (m + 1) * dk, nxt);
      // ... the node and the update; a sample outside the box (within rounding of a face) has ne = 0, which either node takes
      // for dark: alpha = S = 0
      double al[NB], S[NB];
      node.template eval<NB>(A, ne, Te, Z, al, S);
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const double dtau = al[k] * h;
        I[k] = I[k] * exp(-dtau) + S[k] * (-expm1(-dtau));
        tau[k] = tau[k] + dtau;
      }
      column = column + ne * h;
      cur = nxt;
    }
  }
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    A.I[k * N + i] = I[k];
    A.tau[k * N + i] = tau[k];
  }
  L.column[i] = column;
  L.chord[i] = chord;
  L.steps[i] = n;
}

template <typename T, typename P>
void launch_lines(const EmArgs &A, const LineArgs &L, const typename P::Args &X, size_t lds_bytes, bool has_te, bool has_z,
                  int n_band, hipStream_t st) {
  sr::with_flags(
      [&](auto te, auto z) {
        sr::with_count<SR_MAX_BANDS>(
            [&](auto nb) {
              constexpr bool kTe = decltype(te)::value, kZ = decltype(z)::value;
              constexpr int kNb = decltype(nb)::value;
              hipLaunchKernelGGL((k_sightlines<T, kTe, kZ, kNb, P>), dim3(sr::grid_for(L.n, 256)), dim3(256), lds_bytes, st, A, L, X);
            },
            n_band);
      },
      has_te, has_z);
}

}  // namespace

extern "C" int sr_field_sightlines(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_table *table,
                                   const sr_sightline_params *p, int64_t n, const double *origin, const double *dir,
                                   const double *backlight, double *I, double *tau, double *column, double *chord, int32_t *steps,
                                   double *kernel_ms) {
  const char *who = "sr_field_sightlines";
  SR_CHECK(p != nullptr && origin != nullptr && dir != nullptr && I != nullptr && tau != nullptr, "%s: NULL argument", who);
  SR_CHECK(n >= 0, "%s: n must not be negative, got %lld", who, (long long)n);
  SR_RC(check_bands(who, "band", p->n_band, SR_MAX_BANDS, table ? nullptr : p->omega, p->e_ph, p->c_omega));
  SR_RC(check_march(who, p->toward, p->step, p->max_steps));
  if (table) SR_RC(check_table(who, table, p->n_band));
  SR_RC(check_lines(who, n, origin, dir, ne, Te, Z));
  if (kernel_ms) *kernel_ms = 0.0;
  if (n == 0) return SR_OK;
  SR_RC(sr::ensure_init());
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;

  std::vector<double> pack;
  if (table) pack = pack_table(table, p->n_band);
  const size_t tab_bytes = sizeof(double) * pack.size();
  const int nb = p->n_band;
  const size_t map_bytes = sizeof(double) * nb * (size_t)n;

  // one scratch block: the lines' pieces (take_lines) | table
  EmArgs A{};
  LineArgs L{};
  char *tab = nullptr;
  sr::Carve carve;
  take_lines(carve, A, L, ne, n, p->step, p->max_steps, nb, backlight != nullptr);
  carve.take(&tab, tab_bytes);
  if (!carve.alloc()) return SR_ERR_HIP;
  fill_fields(A, ne, Te, Z, p->toward, p->Te, p->Z, nb, p->omega, p->e_ph, p->c_omega);

  SR_RC(upload_lines(A, L, origin, dir, backlight, map_bytes, st));
  if (table) SR_HIP(hipMemcpyAsync(tab, pack.data(), tab_bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipEventRecord(c.ev[0], st));
  if (table) {
    const TabArgs X = tab_args(table, nb, tab, pack.size());
    sr::with_flags(
        [&](auto in_lds, auto f64) {
          using T = std::conditional_t<decltype(f64)::value, double, float>;
          constexpr bool kLds = decltype(in_lds)::value;
          launch_lines<T, TableNode<kLds>>(A, L, X, kLds ? tab_bytes : 0, Te != nullptr, Z != nullptr, nb, st);
        },
        tab_bytes <= kLdsBudget, (bool)ne->is_f64);
  } else if (ne->is_f64) {
    launch_lines<double, NrlNode>(A, L, NrlNode::Args{}, 0, Te != nullptr, Z != nullptr, nb, st);
  } else {
    launch_lines<float, NrlNode>(A, L, NrlNode::Args{}, 0, Te != nullptr, Z != nullptr, nb, st);
  }
  return finish_lines(A, L, map_bytes, I, tau, column, chord, steps, kernel_ms);
}
