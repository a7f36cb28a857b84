"""Line integrals of a domain along its probing axis: phase, deflection, areal density, absorption and rotation maps.

    proj = line_integrals(domain)            # or domain.line_integrals()
    proj.phase, proj.deflection, proj.areal_density, proj.rotation
    proj.sample(p, q, "phase")               # at the lateral positions of rays

No reference counterpart.  These are the thin-plasma predictions of what the tracer integrates along the true path
(d(phase) = omega (n-1), d(v) = dndr, d(amp) = kappa amp, d(pol) = VerdetConst n_e (B.v)): the quick look before a trace is
paid for, and what an interferogram, a schlieren image or Polarimetry.rotation() is read against.  The sums run on the GPU
over the fields the rays themselves see (engine.Volume.project -> sr_volume_project); this module scales the raw integrals
and interpolates the maps on the host.

For a ray that goes straight along the probing axis at v = c the traced phase, pol and ln(amp) EQUAL sample() of the maps
at its launch position up to rounding: RK4 from node plane to node plane integrates a field that is linear between planes
exactly as the trapezoid rule does, and the lateral interpolation commutes with the sum along the axis
(tests/test_projection.py).
"""
from __future__ import annotations

import numpy as np

from . import engine
from .fields import locate

c = engine.c

# raw integral -> the domain flag that makes the volume hold its field
_NEEDS = {"grad": None, "nm1": "phaseshift=True", "ne": "phaseshift=True", "kappa": "inv_brems=True", "neB": "B_on=True"}
_QUANTITIES = ("phase", "fringes", "areal_density", "deflection", "log_amplitude", "transmission", "rotation")


class Projection:
    """The raw line integrals of one domain and the quantities read from them.  `axes` names the two lateral axes in
    x < y < z order and `coords` holds their node coordinates (float64): every map is (len(coords[0]), len(coords[1]))."""

    def __init__(self, integrals, omega, verdet, axes, coords):
        self.axes = (str(axes[0]), str(axes[1]))
        self.coords = (np.asarray(coords[0], np.float64), np.asarray(coords[1], np.float64))
        shape = (len(self.coords[0]), len(self.coords[1]))
        self.integrals = {}
        for name in _NEEDS:
            a = integrals.get(name)
            if a is not None:
                a = np.asarray(a, np.float64)
                want = (2,) + shape if name == "grad" else shape
                if a.shape != want:
                    raise ValueError(f"integral {name!r} has shape {a.shape}, the lateral grid gives {want}")
            self.integrals[name] = a
        self.omega = float(omega)
        self.verdet = float(verdet)

    @classmethod
    def from_integrals(cls, coords, *, omega, axes=("x", "y"), verdet=0.0, grad=None, nm1=None, ne=None, kappa=None, neB=None):
        """A Projection from integrals the caller already holds (sums of slabs, another code's maps): no device involved."""
        return cls({"grad": grad, "nm1": nm1, "ne": ne, "kappa": kappa, "neB": neB}, omega, verdet, axes, coords)

    @property
    def shape(self):
        return (len(self.coords[0]), len(self.coords[1]))

    def _raw(self, name, quantity):
        a = self.integrals[name]
        if a is None:
            flag = _NEEDS[name]
            raise ValueError(f"{quantity} needs the integral {name!r}, which this projection does not hold"
                             + (f": build the domain with {flag}" if flag else ""))
        return a

    @property
    def phase(self):
        """omega/c * integral of (n-1) dl [rad], with the tracer's sign (negative in a plasma)."""
        return self.omega / c * self._raw("nm1", "phase")

    @property
    def fringes(self):
        return self.phase / (2 * np.pi)

    @property
    def areal_density(self):
        """Integral of n_e dl [m^-2]."""
        return self._raw("ne", "areal_density")

    @property
    def deflection(self):
        """(2, n_u, n_v): integral of dnd_u, dnd_v dl / c^2 [rad], the angles a ray gathers about the two lateral axes."""
        return self._raw("grad", "deflection") / c ** 2

    @property
    def log_amplitude(self):
        """Integral of kappa dl / c: ln of the amplitude a ray keeps."""
        return self._raw("kappa", "log_amplitude") / c

    @property
    def transmission(self):
        """exp(2 * log_amplitude): the intensity a ray keeps."""
        return np.exp(2 * self.log_amplitude)

    @property
    def rotation(self):
        """VerdetConst * integral of n_e B_a dl [rad]: the Faraday rotation of the polarisation."""
        return self.verdet * self._raw("neB", "rotation")

    def sample(self, p, q, what="phase"):
        """Bilinear interpolation of a quantity at the lateral positions (p along axes[0], q along axes[1]); NaN outside
        the grid.  `what` names one of the quantities above; "deflection" gives (2, N)."""
        if what not in _QUANTITIES:
            raise ValueError(f"what must be one of {_QUANTITIES}, got {what!r}")
        return bilinear(self.coords, getattr(self, what), p, q)


def bilinear(coords, m, p, q):
    """Bilinear interpolation of the maps m (..., n_u, n_v) on the node coordinates coords = (gu, gv) at the lateral positions
    (p, q); NaN outside the grid.  Projection.sample's and Emission.sample's rule."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    if p.shape != q.shape:
        raise ValueError(f"p has shape {p.shape}, q {q.shape}")
    gu, gv = coords
    with np.errstate(invalid="ignore"):
        inside = (p >= gu[0]) & (p <= gu[-1]) & (q >= gv[0]) & (q <= gv[-1])
    (i, t, _), (j, s, _) = locate(gu, np.where(inside, p, gu[0])), locate(gv, np.where(inside, q, gv[0]))
    out = ((1 - t) * (1 - s) * m[..., i, j] + t * (1 - s) * m[..., i + 1, j]
           + (1 - t) * s * m[..., i, j + 1] + t * s * m[..., i + 1, j + 1])
    return np.where(inside, out, np.nan)


def _lateral(domain, axis):
    names = [n for k, n in enumerate("xyz") if k != axis]
    return tuple(names), tuple(np.asarray(getattr(domain, n), np.float32).astype(np.float64) for n in names)


def line_integrals(domain, lwl=1064e-9, regions=None):
    """The Projection of a domain of either API generation.

    simulator.ScalarDomain: the volume propagator.solve traces through (built and cached on the domain), or -- with
    region_count > 1, the auto-batching rule, or `regions` given -- the region loop of the solve: each slab of node planes is
    built, projected and closed, and the maps are added on the host.
    solvers_legacy.ScalarDomain: the volume calc_dndr left on the device (with what set_up_interps attached); lwl is the
    one calc_dndr was given."""
    axis = engine.axis_index(domain.probing_direction)
    axes, coords = _lateral(domain, axis)
    if hasattr(domain, "_volume_cache"):
        from .simulator import propagator

        regions = propagator._regions(domain, lwl) if regions is None else max(1, int(regions))
        if regions > 1:
            total, omega, verdet = None, 0.0, 0.0
            for vol in propagator._slab_volumes(domain, lwl, regions)[1]:
                part, omega, verdet = vol.project(), vol.omega, vol.verdet
                if total is None:
                    total = part
                else:
                    for name, a in part.items():
                        if a is not None:
                            total[name] = total[name] + a
            return Projection(total, omega, verdet, axes, coords)
        vol = propagator._volume_for(domain, lwl)
    else:
        vol = getattr(domain, "_volume", None)
        if vol is None:
            raise RuntimeError("call calc_dndr(lwl) first")
        if regions not in (None, 1):
            raise ValueError("the legacy ScalarDomain holds one whole volume: regions does not apply")
    return Projection(vol.project(), vol.omega, vol.verdet, axes, coords)
