"""Self-emission images: the plasma's own light along the probing axis, emission with self-absorption.

    em = self_emission(domain, [532e-9, 100e-9])          # or domain.self_emission(...), domain.rotated(30).self_emission(...)
    em.intensity, em.optical_depth, em.transmission       # (n_band, n_u, n_v)
    em.sample(p, q, "intensity")                          # at lateral positions
    self_emission(domain, lam, fields=fields.SourceFields(domain))   # a sweep: the fields are uploaded once and kept

No reference counterpart.  Every other image of the package is an image of the probe; this is the optical fast-framing / XUV
pinhole channel.  Per band and lateral column the formal solution of dI/ds = alpha (S - I) is marched from the far plane to the
plane nearest the detector on the GPU (engine.emission -> sr_field_emission; include/synthray.h states the rule): alpha is
propagator.kappa(ne, Te, Z, omega) / c -- the NRL low-frequency (inverse-bremsstrahlung) coefficient the tracer uses, trustworthy
for hbar*omega <~ Te -- and S is the Planck function B_omega(Te), so the emissivity follows from Kirchhoff's law.  Refraction of the
emitted light, line emission and detector optics are not modelled.  Where hbar*omega is above Te -- XUV and soft-X-ray bands, where
bound-free and line opacity dominate -- the coefficient comes from an opacity table instead: table_emission below.  Both march
columns parallel to a grid axis; a pinhole camera's converging lines, a point backlighter's diverging ones and single chords at any
angle are sightlines.sightline_emission (domain.sightline_emission), with either node.

    table = OpacityTable.from_propaceos(read_propaceos(path, need_abs_opacity=True, need_emiss_opacity=True), A=12.011)
    em = table_emission(domain, table)                     # or domain.table_emission(table); a TableEmission
"""
from __future__ import annotations

import numpy as np

from . import engine
from .fields import staged, uniform
from .projection import _lateral, bilinear

c = engine.c
_QUANTITIES = ("intensity", "optical_depth", "transmission")


class _Maps:
    """What every result of the emission family has beside its optical_depth (Emission, TableEmission, sightlines.SightlineEmission,
    sightlines.SightlineSpectra)."""

    @property
    def transmission(self):
        """exp(-optical_depth): what a backlight keeps."""
        return np.exp(-self.optical_depth)

    def _d_omega(self, missing):
        """The widths of the bands in angular frequency [rad/s] from `edges` [eV]; without edges ValueError(missing)."""
        if self.edges is None:
            raise ValueError(missing)
        return (self.edges[:, 1] - self.edges[:, 0]) * engine.E_CHARGE / engine.HBAR


class Emission(_Maps):
    """The self-emission maps of one line of sight.  `axes` names the two lateral axes in x < y < z order, `coords` holds their
    node coordinates (float64); intensity [W m^-2 sr^-1 (rad/s)^-1, spectral radiance per unit angular frequency] and
    optical_depth are (n_band, len(coords[0]), len(coords[1])), band b at wavelengths[b]."""

    def __init__(self, intensity, optical_depth, axes, coords, wavelengths):
        self.axes = (str(axes[0]), str(axes[1]))
        self.coords = (np.asarray(coords[0], np.float64), np.asarray(coords[1], np.float64))
        self.wavelengths = np.atleast_1d(np.asarray(wavelengths, np.float64))
        want = (len(self.wavelengths), len(self.coords[0]), len(self.coords[1]))
        self.intensity = np.asarray(intensity, np.float64)
        self.optical_depth = np.asarray(optical_depth, np.float64)
        for name in ("intensity", "optical_depth"):
            if getattr(self, name).shape != want:
                raise ValueError(f"{name} has shape {getattr(self, name).shape}, the bands and the lateral grid give {want}")

    def sample(self, p, q, what="intensity"):
        """Bilinear interpolation of a quantity at the lateral positions (p along axes[0], q along axes[1]) -> (n_band, N);
        NaN outside the grid (Projection.sample's rule)."""
        if what not in _QUANTITIES:
            raise ValueError(f"what must be one of {_QUANTITIES}, got {what!r}")
        return bilinear(self.coords, getattr(self, what), p, q)

    def after(self, other):
        """This slab seen through nothing, with `other` behind it on the same line of sight: I = I_other * exp(-tau_self) + I_self,
        the optical depths added -- what passing other.intensity as this slab's backlight gives.  A volume too large for HBM is
        done slab by slab this way."""
        if self.axes != other.axes or not np.array_equal(self.wavelengths, other.wavelengths) or any(
                not np.array_equal(a, b) for a, b in zip(self.coords, other.coords)):
            raise ValueError("the two slabs differ in lateral axes, coordinates or wavelengths")
        return Emission(other.intensity * np.exp(-self.optical_depth) + self.intensity, other.optical_depth + self.optical_depth,
                        self.axes, self.coords, self.wavelengths)


def _toward(toward):
    if toward in ("+", +1):
        return +1
    if toward in ("-", -1):
        return -1
    raise ValueError(f"toward must be '+' (the detector behind the last plane, where the rays leave) or '-', got {toward!r}")


def _omegas(wavelengths):
    lam = np.atleast_1d(np.asarray(wavelengths, np.float64))
    if lam.ndim != 1 or not 1 <= len(lam) <= engine._ffi.MAX_BANDS:
        raise ValueError(f"between 1 and {engine._ffi.MAX_BANDS} wavelengths go in one pass, got shape {lam.shape}")
    if not np.all(np.isfinite(lam) & (lam > 0)):
        raise ValueError(f"wavelengths must be finite and positive, got {lam.tolist()}")
    return lam, 2 * np.pi * c / lam


def _check_table(table, kind):
    """ValueError unless `table` has an OpacityTable's members; kind: the class the entry takes, with its article."""
    for name in ("temperatures", "densities", "absorption", "photon_energy", "A"):
        if not hasattr(table, name):
            raise ValueError(f"table must be {kind} (utils.eos_opacity): it has no {name}")


def _upload(domain, fields, run, more=None):
    """What every emission entry shares (self_emission, table_emission, sightlines.sightline_emission, sightline_spectra and
    sightline_lines): the domain's fields
    uploaded by self_emission's rules -- a Te or Z that is a scalar (or broadcast from one) goes as a value, float32 only when
    every array is float32 (fields.SourceFields.get_all) -- then run(ne, Te, Z), whose result is returned.  more: {name: array |
    None} of further fields that go up with them, in the same dtype (sightline_lines' Ti and V); run then gets them by keyword."""
    ne, Te, Z = (getattr(domain, name, None) for name in ("ne", "Te", "Z"))
    if ne is None:
        raise ValueError("the domain holds no electron density: pass ne_type= or call external_ne()")
    if Te is None or Z is None:
        raise ValueError("self_emission needs external_Te() and external_Z()")
    shape = (len(domain.x), len(domain.y), len(domain.z))
    values = {"Te": uniform(Te), "Z": uniform(Z)}
    named = {name: np.broadcast_to(np.asarray(a), shape) for name, a in (("ne", ne), ("Te", Te), ("Z", Z)) if values.get(name) is None}
    named.update(more or {})
    with staged(domain, fields) as src:
        f = src.get_all(named)
        return run(f["ne"], f.get("Te", values["Te"]), f.get("Z", values["Z"]), **{name: f[name] for name in more or {}})


def _march(domain, toward, fields, run):
    """What self_emission and table_emission share: _upload's fields, then run(ne, Te, Z, axis, sign) -> (I, tau) along the
    probing axis; returns (I, tau, axes, coords)."""
    axis = engine.axis_index(domain.probing_direction)
    sign = _toward(toward)
    I, tau = _upload(domain, fields, lambda ne, Te, Z: run(ne, Te, Z, axis, sign))
    axes, coords = _lateral(domain, axis)
    return I, tau, axes, coords


def self_emission(domain, wavelengths, toward="+", backlight=None, fields=None):
    """The Emission of a domain of either API generation along its probing_direction, at up to 4 wavelengths [m] in one pass
    over the fields.  toward "+": the detector is where the rays leave (behind the last node plane of the axis), "-": where
    they enter.  backlight: (n_band, n_u, n_v) spectral radiance behind the far plane, or None.  The domain needs external_Te()
    and external_Z(); a Te or Z that is a scalar (or broadcast from one) is not uploaded.  fields: a fields.SourceFields of the
    domain whose uploads are reused across calls."""
    engine.axis_index(domain.probing_direction)
    _toward(toward)
    lam, omegas = _omegas(wavelengths)
    I, tau, axes, coords = _march(domain, toward, fields, lambda ne, Te, Z, axis, sign: engine.emission(ne, Te, Z, omegas, axis, sign, backlight))
    return Emission(I, tau, axes, coords, lam)


class TableEmission(Emission):
    """The Emission of a tabulated-opacity march: intensity is the spectral radiance per unit angular frequency at the table's
    photon_energy [eV] per band (wavelengths = 2 pi hbar c / (e photon_energy)).  Where the table has band edges, `edges`
    ((n_band, 2), eV) keeps them and band_radiance = intensity * (the band's width in angular frequency) [W m^-2 sr^-1]: the
    Planck function is taken at photon_energy, not integrated over the group."""

    def __init__(self, intensity, optical_depth, axes, coords, photon_energy, edges=None):
        self.photon_energy = np.atleast_1d(np.asarray(photon_energy, np.float64))
        super().__init__(intensity, optical_depth, axes, coords, 2 * np.pi * engine.HBAR * c / (engine.E_CHARGE * self.photon_energy))
        self.edges = None if edges is None else np.asarray(edges, np.float64).reshape(len(self.photon_energy), 2)

    @property
    def band_radiance(self):
        return self.intensity * self._d_omega("the table has no band edges: band_radiance needs the bands' widths")[:, None, None]


def table_emission(domain, table, toward="+", backlight=None, fields=None):
    """self_emission with the opacities of `table` (utils.eos_opacity.OpacityTable, e.g. OpacityTable.from_propaceos(
    read_propaceos(...), A)) in place of the NRL coefficient: a TableEmission, one band per band of the table
    (engine.emission_table -> sr_field_emission_table; include/synthray.h states the rule).  A node's ion density is ne / Z with
    the domain's Z; the opacities are interpolated bilinearly in (log Te, log ni) on their logarithms and held at the edge value
    outside the table; the source function is Planck's at the band's photon_energy times emission / absorption opacity (1 for a
    table without emission opacities: LTE).  toward, backlight, fields and the upload rules are self_emission's.
    Not modelled: Z from the table's own zf_table (it would need the solve ne = ni * zf(T, ni)), group-integrated Planck
    functions, refraction of the emitted light, detector optics."""
    engine.axis_index(domain.probing_direction)
    _toward(toward)
    _check_table(table, "an OpacityTable")
    I, tau, axes, coords = _march(domain, toward, fields, lambda ne, Te, Z, axis, sign: engine.emission_table(ne, Te, Z, table, axis, sign, backlight))
    return TableEmission(I, tau, axes, coords, table.photon_energy, getattr(table, "edges", None))
