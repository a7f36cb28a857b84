// Self-emission images: emission with self-absorption along a grid axis (sr_field_emission; include/synthray.h states the rule
// every node, cell and column follows, operation for operation).  The march -- k_emission_z, k_emission_xy, the cell, the host's
// staging and band checks, the NRL node's policy -- is emission_march.inc, shared with emission_table.hip and the two sightline
// units; the NRL node is nrl_node.inc, shared with wave.hip; this unit holds the entry.  No LDS.
// Compiled with -ffp-contract=off: products and sums round separately, as the NumPy restatement's do (tests/test_emission.py).
#include "emission_march.inc"

extern "C" int sr_field_emission(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_params *p,
                                 const double *backlight, double *I, double *tau, double *kernel_ms) {
  SR_CHECK(p != nullptr && I != nullptr && tau != nullptr, "sr_field_emission: NULL argument");
  SR_RC(check_bands("sr_field_emission", "band", p->n_band, SR_MAX_BANDS, p->omega, p->e_ph, p->c_omega));
  if (int rc = check_fields("sr_field_emission", ne, Te, Z, p)) return rc;
  EmArgs A;
  size_t map_bytes = 0;
  if (int rc = prepare(ne, Te, Z, p, backlight, 0, A, map_bytes, nullptr)) return rc;
  sr::Context &c = sr::ctx();
  SR_HIP(hipEventRecord(c.ev[0], c.stream));
  if (ne->is_f64)
    launch<double, NrlNode>(A, NrlNode::Args{}, 0, p->axis, Te != nullptr, Z != nullptr, p->n_band, c.stream);
  else
    launch<float, NrlNode>(A, NrlNode::Args{}, 0, p->axis, Te != nullptr, Z != nullptr, p->n_band, c.stream);
  return finish(A, map_bytes, I, tau, kernel_ms);
}
