"""Oblique lines of sight: a domain seen from a frame turned against the lab (no reference counterpart).

    side_on = domain.rotated(22.5, about="y")            # or orientation.rotated(domain, 22.5, about="y")
    for view in orientation.views(domain, np.arange(0, 180, 15), about="y"): ...     # the tomography sweep

The engine probes along a grid axis.  A probe line that is no grid axis is set up by turning the plasma instead: the view
frame's axes are the lab's turned by R (its axis k is column k of R, so node q of the view sits at the lab position R q) and

    ne'(q) = ne(R q)      Te'(q) = Te(R q)      Z'(q) = Z(R q)      B'(q) = R^T B(R q)      E'(q) = R^T E(R q)

-- the fields on the view's own grid, the vector fields in the view's components; Ti (external_Ti) goes as Te and the flow V
(external_V) as B when the domain holds them, the electrons' order (external_order) as Te (Thomson scattering).  The result
is an ordinary ScalarDomain of
the source's generation and flags: solve, the region loop, line_integrals and export_scalar_field work on it unchanged, and
probing it along z looks along the lab direction R e_z.  The resampling is trilinear and runs on the GPU
(engine.Field.resample -> sr_field_resample, include/synthray.h states its rule); each source field is uploaded once, and
views() keeps the uploads in HBM across the angles (fields.SourceFields, which the other field diagnostics stage through as well;
it is importable from here too).  engine.Field takes the general affine form p = M q + t.
"""
from __future__ import annotations

import numpy as np

from .fields import SourceFields, staged

_ABOUT = {"x": 0, "y": 1, "z": 2}
_QUARTER = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}  # angle -> (cos, sin), exactly
# vacuum for ne and B; Te at external_Te's floor Te_min = 1.0; Z = 1.0 (kappa() divides by neither's zero)
DEFAULT_FILL = {"ne": 0.0, "Te": 1.0, "Z": 1.0, "B": 0.0}
_E_FILL = 0.0  # a domain's E (external_E; proton radiography) is vacuum outside the source box, or fill["E"]
# the fields only some domains hold: Ti as Te, V and Vd at rest, the electrons' order Maxwellian
_EXTRA_FILL = {"E": _E_FILL, "Ti": DEFAULT_FILL["Te"], "V": 0.0, "Vd": 0.0, "order": 2.0}


def rotation_matrix(angle_deg, about="y"):
    """The right-handed rotation by angle_deg about the lab axis "x" | "y" | "z" (3x3, float64).  At multiples of 90 degrees
    the entries are exactly 0 and +-1."""
    if about not in _ABOUT:
        raise ValueError(f"about must be 'x', 'y' or 'z', got {about!r}")
    a = float(angle_deg) % 360.0
    co, si = _QUARTER[int(a)] if a in (0.0, 90.0, 180.0, 270.0) else (np.cos(np.deg2rad(a)), np.sin(np.deg2rad(a)))
    k = _ABOUT[about]
    i, j = (k + 1) % 3, (k + 2) % 3
    R = np.zeros((3, 3))
    R[k, k] = 1.0
    R[i, i], R[i, j], R[j, i], R[j, j] = co, -si, si, co
    return R


def compose(*matrices):
    """The product of rotation matrices, left to right: compose(A, B) = A @ B turns by B first."""
    R = np.eye(3)
    for M in matrices:
        M = np.asarray(M, np.float64)
        if M.shape != (3, 3):
            raise ValueError(f"a rotation matrix is 3x3, got {M.shape}")
        R = R @ M
    return R


def check_orthonormal(R, tol=1e-12):
    """R as a float64 3x3 array; ValueError unless R R^T = 1 to `tol` in every entry."""
    R = np.asarray(R, np.float64)
    if R.shape != (3, 3) or not np.all(np.isfinite(R)):
        raise ValueError(f"matrix must be a finite 3x3 array, got shape {R.shape}")
    err = float(np.max(np.abs(R @ R.T - np.eye(3))))
    if err > tol:
        raise ValueError(f"matrix is not orthonormal: max |R R^T - 1| = {err:.3e} > {tol:g} "
                         "(the general affine form is engine.Field.resample)")
    return R


def _new_domain(domain, dims, lengths):
    """An empty domain of the source's generation and flags, and its grid."""
    if hasattr(domain, "_volume_cache"):  # simulator.ScalarDomain(lengths, dims, ...)
        new = type(domain)(domain.lengths if lengths is None else lengths, domain.dims if dims is None else dims,
                           inv_brems=domain.inv_brems, phaseshift=domain.phaseshift, B_on=domain.B_on,
                           probing_direction=domain.probing_direction, auto_batching=domain.auto_batching,
                           region_count=domain.region_count, leeway_factor=domain.leeway_factor, debug=domain.debug)
        return new
    src = (domain.x, domain.y, domain.z)
    if dims is None and lengths is None:
        x, y, z = src
    else:  # solvers_legacy.ScalarDomain(x, y, z, extent, ...): the box -L/2..L/2 per axis, the source's where not given
        n = [len(a) for a in src] if dims is None else ([int(dims)] * 3 if np.ndim(dims) == 0 else [int(v) for v in dims])
        L = ([float(a[-1]) - float(a[0]) for a in src] if lengths is None
             else ([float(lengths)] * 3 if np.ndim(lengths) == 0 else [float(v) for v in lengths]))
        x, y, z = (np.linspace(-L[k] / 2, L[k] / 2, n[k]) for k in range(3))
    new = type(domain)(x, y, z, domain.extent, B_on=domain.B_on, inv_brems=domain.inv_brems, phaseshift=domain.phaseshift,
                       probing_direction=domain.probing_direction)
    new.precision, new.substeps = domain.precision, domain.substeps
    return new


def rotated(domain, angle_deg=None, about="y", *, matrix=None, fill=None, dims=None, lengths=None, source=None):
    """A new ScalarDomain of the same generation and flags holding the source's fields seen from the frame turned by R =
    rotation_matrix(angle_deg, about), or `matrix` (orthonormal to 1e-12, else ValueError): ne'(q) = ne(R q), Te and Z the
    same when they are arrays (scalars pass through), B'(q) = R^T B(R q), and E as B when the domain holds one; Ti and the
    electrons' order (external_order) go as Te and the flow V and the electron drift Vd (external_Vd) as B when the domain holds
    them.  The view grid
    is the source's lengths and dims unless `dims` / `lengths` say otherwise.  Outside the source box the fields take `fill`:
    None for the defaults
    (DEFAULT_FILL: vacuum, Te_min, Z = 1), a number for ne, or a dict over "ne", "Te", "Z", "B", "E", "Ti", "V", "Vd", "order" (Ti: Te_min, V and Vd: at rest,
    order: 2.0).  `source`: a SourceFields
    of the same domain whose uploads are reused (views())."""
    if (angle_deg is None) == (matrix is None):
        raise ValueError("give either angle_deg (with about) or matrix")
    R = check_orthonormal(rotation_matrix(angle_deg, about) if matrix is None else matrix)
    fills = dict(DEFAULT_FILL)
    if isinstance(fill, dict):
        unknown = set(fill) - set(fills) - set(_EXTRA_FILL)
        if unknown:
            raise ValueError(f"fill names {sorted(unknown)}; the fields are {sorted(set(fills) | set(_EXTRA_FILL))}")
        fills.update(fill)
    elif fill is not None:
        fills["ne"] = float(fill)
    ne = getattr(domain, "ne", None)
    if ne is None:
        raise ValueError("the domain holds no ne yet")
    new = _new_domain(domain, dims, lengths)
    grid = (new.x, new.y, new.z)
    zero = (0.0, 0.0, 0.0)
    with staged(domain, source, "source") as src:
        new.external_ne(src.get("ne", ne).resample(R, zero, grid, fill=fills["ne"]))
        for name in ("Te", "Z", "Ti", "order"):
            a = getattr(domain, name, None)
            if a is not None:
                f = fills.get(name, _EXTRA_FILL.get(name))
                setattr(new, name, src.get(name, a).resample(R, zero, grid, fill=f) if np.ndim(a) == 3 else a)
        B = getattr(domain, "B", None)
        if B is not None:
            new.B = src.get("B", B).resample(R, zero, grid, V=R.T, fill=fills["B"])
        E = getattr(domain, "E", None)
        if E is not None:
            new.E = src.get("E", E).resample(R, zero, grid, V=R.T, fill=fills.get("E", _E_FILL))
        for name in ("V", "Vd"):
            v = getattr(domain, name, None)
            if v is not None:
                setattr(new, name, src.get(name, v).resample(R, zero, grid, V=R.T, fill=fills.get(name, _EXTRA_FILL[name])))
    return new


def views(domain, angles_deg, about="y", **kw):
    """A generator of rotated(domain, angle, about, **kw) over angles_deg that uploads each source field once and keeps it in
    HBM across the angles; the uploads are released when the generator ends or is closed."""
    with staged(domain, kw.pop("source", None), "source") as src:
        for angle in angles_deg:
            yield rotated(domain, angle, about, source=src, **kw)
