// Self-emission from tabulated opacities (sr_field_emission_table; include/synthray.h states the rule): emission_march.inc's
// march with a node whose absorption and emission opacities are interpolated, bilinearly in (log Te, log ni) on the logarithms of
// the table, from a temperature x ion-density lattice (PROPACEOS tables, or anything laid out that way).  The node, the table's
// staging (LDS up to 64 KiB, global memory above that), the host's checks of a table and its packing are table_node.inc, shared
// with sightlines.hip; this unit holds the entry.
//
// k_emission_xy runs 256-lane workgroups here, not the NRL node's 64: a workgroup stages the table once for its 256 columns (for
// 512^2 columns 1024 copies of the table come out of L2, not 4096); k_emission_z's 256-lane workgroups stride over the columns, so
// there a copy serves ncol / grid columns.  No scratch, no atomics.  Compiled with -ffp-contract=off.
#include <vector>

#include "emission_march.inc"

namespace {
#include "table_node.inc"
}  // namespace

extern "C" int sr_field_emission_table(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_table *t,
                                       const sr_emission_params *p, const double *backlight, double *I, double *tau,
                                       double *kernel_ms) {
  SR_CHECK(p != nullptr && I != nullptr && tau != nullptr, "sr_field_emission_table: NULL argument");
  SR_RC(check_bands("sr_field_emission_table", "band", p->n_band, SR_MAX_BANDS, nullptr, p->e_ph, p->c_omega));  // omega is not read
  if (int rc = check_table("sr_field_emission_table", t, p->n_band)) return rc;
  if (int rc = check_fields("sr_field_emission_table", ne, Te, Z, p)) return rc;

  const std::vector<double> pack = pack_table(t, p->n_band);
  const size_t tab_bytes = sizeof(double) * pack.size();

  EmArgs A;
  size_t map_bytes = 0;
  char *tab = nullptr;
  if (int rc = prepare(ne, Te, Z, p, backlight, tab_bytes, A, map_bytes, &tab)) return rc;
  sr::Context &c = sr::ctx();
  SR_HIP(hipMemcpyAsync(tab, pack.data(), tab_bytes, hipMemcpyHostToDevice, c.stream));
  const TabArgs X = tab_args(t, p->n_band, tab, pack.size());
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
