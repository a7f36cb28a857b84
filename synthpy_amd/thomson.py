"""Optical Thomson scattering spectra of a domain (no reference counterpart).

    probe = thomson.Probe(532e-9, origin=(0, 0, -5e-3), direction=(0, 0, 1), polarisation=(1, 0, 0))
    coll = thomson.Collection(points, direction=(0, 1, 0), length=100e-6, n_quad=8, beam_radius=50e-6)
    sp = domain.thomson_scattering(probe, coll, wavelengths, ion_mass=12)      # or thomson.spectra(domain, probe, coll, ...)
    sp.power, sp.weight, sp.theta, sp.alpha

Each scattering volume is a quadrature along the probe (and across it) about one of the collection's points; the GPU gathers
ne, Te, Ti, Z and the flow V at every quadrature point and sums the spectral density function S(k, w) of a Maxwellian plasma over
them, per wavelength (engine.thomson -> sr_field_thomson; include/synthray.h states the rule).  Validity: non-relativistic,
unmagnetised, Maxwellian electrons and one Maxwellian ion species sharing the flow, vacuum wavenumbers (ne << n_crit), no probe
absorption or refraction, no collection optics beyond one direction per volume.

Several ion species and a current (spectra_multi; engine.thomson_multi -> sr_field_thomson_multi):

    ch = [thomson.Species(12, 6, 0.5), thomson.Species(1, 1, 0.5)]             # mass number, charge, relative number fraction
    domain.external_Vd(thomson.drift_velocity(J, domain.ne))                    # the electrons' drift against the ions, -J/(e ne)
    sp = domain.thomson_scattering_multi(probe, coll, wavelengths, ch)

1 to 4 Maxwellian ion species that share Ti and the flow; their relative Landau damping shapes the ion-acoustic feature, and the
drift shows as the asymmetry of its two peaks.  A species' charge and fraction may vary over the grid.

Super-Gaussian (Langdon) electrons (spectra_sg; engine.thomson_sg -> sr_field_thomson_sg):

    domain.external_order(thomson.langdon_order(Z, intensity, domain.Te, 351e-9))   # m = 2..5, cell by cell
    sp = domain.thomson_scattering_sg(probe, coll, wavelengths, ch)             # or order=3.2 for a uniform m

The electrons follow exp(-(v/v_m)^m) with the local order m: the electron-plasma-wave peaks move and sharpen and the ion-acoustic
peaks lose Landau damping.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import engine
from .fields import grid_f64, locate, staged

E_CHARGE = engine.E_CHARGE    # C
EPS0 = 8.8541878128e-12       # F/m (CODATA 2018)
R_E = 2.8179403262e-15        # m, the classical electron radius (CODATA 2018)
M_E = 9.1093837015e-31        # kg (CODATA 2018)

# the 7-point rule of degree 5 on the unit disc (Abramowitz & Stegun 25.4.61): the centre and a hexagon of radius sqrt(2/3);
# the weights are fractions of the disc's area
_DISC = np.array([[0.0, 0.0]] + [[np.sqrt(2.0 / 3.0) * np.cos(k * np.pi / 3), np.sqrt(2.0 / 3.0) * np.sin(k * np.pi / 3)]
                                 for k in range(6)])
_DISC_W = np.array([0.25] + [0.125] * 6)


def _unit(v, name):
    v = np.asarray(v, np.float64)
    if v.shape[-1:] != (3,) or v.ndim > 2 or not np.all(np.isfinite(v)):
        raise ValueError(f"{name} must be finite and of shape (3,) or (M, 3), got shape {v.shape}")
    n = np.sqrt(np.sum(v * v, axis=-1, keepdims=True))
    if np.any(n == 0.0):
        raise ValueError(f"{name} has zero length")
    return v / n


class Probe:
    """The probe beam: wavelength [m], a point `origin` [m] on its axis, its direction (normalised here) and, optionally, its
    linear polarisation (a vector perpendicular to the direction to 1e-6, normalised here; None: the polarisation factor is 1)."""

    def __init__(self, wavelength, origin, direction, polarisation=None):
        self.wavelength = float(wavelength)
        if not (np.isfinite(self.wavelength) and self.wavelength > 0):
            raise ValueError(f"wavelength must be finite and positive, got {wavelength!r}")
        self.origin = np.asarray(origin, np.float64)
        if self.origin.shape != (3,) or not np.all(np.isfinite(self.origin)):
            raise ValueError("origin must be three finite numbers")
        self.direction = _unit(direction, "direction")
        if self.direction.shape != (3,):
            raise ValueError("a probe has one direction (3,)")
        self.polarisation = None
        if polarisation is not None:
            e = _unit(polarisation, "polarisation")
            if e.shape != (3,) or abs(float(e @ self.direction)) > 1e-6:
                raise ValueError("polarisation must be one vector perpendicular to the probe's direction")
            self.polarisation = e


class Collection:
    """The scattering volumes: `points` (M, 3) [m], their centres, seen along the unit `direction` (3,) or (M, 3) (from the
    plasma to the collection optic).  The quadrature of a volume is n_quad Gauss-Legendre nodes along the probe's direction over
    `length` [m] centred on the point, weights in metres (they sum to `length`); with beam_radius > 0 [m] times the 7-point
    disc rule of degree 5 across the beam, weights as fractions of the disc (7 n_quad points, a top-hat beam).  quadrature =
    (points (M, Nq, 3), weights (M, Nq)) gives the points and weights [m] of every volume directly instead."""

    def __init__(self, points, direction, length=None, n_quad=None, beam_radius=0.0, *, quadrature=None):
        self.points = np.asarray(points, np.float64)
        if self.points.ndim != 2 or self.points.shape[1] != 3 or not np.all(np.isfinite(self.points)):
            raise ValueError(f"points must be finite and of shape (M, 3), got {self.points.shape}")
        M = len(self.points)
        d = _unit(direction, "direction")
        if d.shape not in ((3,), (M, 3)):
            raise ValueError(f"direction must have shape (3,) or ({M}, 3), got {d.shape}")
        self.direction = np.ascontiguousarray(np.broadcast_to(d, (M, 3)))
        self._given = None
        if quadrature is not None:
            if length is not None or n_quad is not None or beam_radius:
                raise ValueError("give either quadrature or length, n_quad and beam_radius")
            pts, wts = (np.asarray(a, np.float64) for a in quadrature)
            if pts.ndim != 3 or pts.shape[0] != M or pts.shape[2] != 3 or wts.shape != pts.shape[:2]:
                raise ValueError(f"quadrature must be (points ({M}, Nq, 3), weights ({M}, Nq)), got {pts.shape} and {wts.shape}")
            if not np.all(np.isfinite(wts)):
                raise ValueError("quadrature weights must be finite")
            self._given = (np.ascontiguousarray(pts), np.ascontiguousarray(wts))
            return
        if length is None or n_quad is None:
            raise ValueError("length and n_quad are needed (or quadrature)")
        self.length, self.n_quad, self.beam_radius = float(length), int(n_quad), float(beam_radius)
        if not (np.isfinite(self.length) and self.length > 0):
            raise ValueError(f"length must be finite and positive, got {length!r}")
        if self.n_quad < 1:
            raise ValueError(f"n_quad must be at least 1, got {n_quad!r}")
        if not (np.isfinite(self.beam_radius) and self.beam_radius >= 0):
            raise ValueError(f"beam_radius must be finite and not negative, got {beam_radius!r}")

    def quadrature(self, probe):
        """(points (M, Nq, 3), weights (M, Nq)) for `probe`."""
        if self._given is not None:
            return self._given
        t, w = np.polynomial.legendre.leggauss(self.n_quad)
        d = probe.direction
        along = (0.5 * self.length * t)[:, None] * d[None, :]                      # (n_quad, 3)
        wts = 0.5 * self.length * w
        if self.beam_radius > 0:
            a = np.eye(3)[int(np.argmin(np.abs(d)))]
            e1 = np.cross(d, a)
            e1 /= np.sqrt(e1 @ e1)
            e2 = np.cross(d, e1)
            across = self.beam_radius * (_DISC[:, :1] * e1[None, :] + _DISC[:, 1:] * e2[None, :])   # (7, 3)
            along = (along[:, None, :] + across[None, :, :]).reshape(-1, 3)
            wts = (wts[:, None] * _DISC_W[None, :]).ravel()
        pts = self.points[:, None, :] + along[None, :, :]
        return np.ascontiguousarray(pts), np.ascontiguousarray(np.broadcast_to(wts, pts.shape[:2]))


@dataclass
class ThomsonSpectra:
    wavelengths: np.ndarray   # (n_lambda) [m]
    power: np.ndarray         # (M, n_lambda): scattered energy per incident energy, per steradian and per metre of wavelength
    weight: np.ndarray        # (M): sum_q w_q ne_q over the points that scatter [m^-2]
    theta: np.ndarray         # (M): the scattering angle [rad]
    alpha: np.ndarray         # (M): 1/(k lambda_D) at the volume's centre and the probe's wavelength; NaN outside the plasma
    kernel_ms: float = 0.0    # HIP-event time of the kernel


def instrument_convolve(power, wavelengths, fwhm):
    """`power` (..., n_lambda) with a Gaussian instrument function of full width at half maximum `fwhm` [m] applied along the
    last axis: a normalised kernel on the wavelength grid, which must be uniform (ValueError otherwise).  What a sample spreads
    onto the grid adds up to the sample, also next to the ends, so the sum over the grid is kept."""
    lam = np.asarray(wavelengths, np.float64)
    power = np.asarray(power, np.float64)
    fwhm = float(fwhm)
    if not (np.isfinite(fwhm) and fwhm > 0):
        raise ValueError(f"instrument_fwhm must be finite and positive, got {fwhm!r}")
    n = len(lam)
    if n < 2:
        return power.copy()
    d = np.diff(lam)
    if not np.all(np.abs(d - d[0]) <= 1e-9 * abs(d[0])) or d[0] == 0:
        raise ValueError("the instrument function needs a uniform wavelength grid")
    sigma = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    J = int(min(n - 1, np.ceil(8.5 * sigma / abs(d[0]))))  # beyond 8.5 sigma the kernel is below 2^-52 of its peak
    g = np.exp(-0.5 * (np.arange(-J, J + 1) * d[0] / sigma) ** 2)
    norm = np.convolve(np.ones(n), g, "full")[J:J + n]
    flat = power.reshape(-1, n)
    out = np.stack([np.convolve(row / norm, g, "full")[J:J + n] for row in flat]) if len(flat) else flat.copy()
    return out.reshape(power.shape)


def _at(domain, arrays, points):
    """The trilinear values of the 3-D `arrays` at `points` (M, 3) on the host (NaN outside the grid): the volume centres."""
    cells, ws, ins = zip(*(locate(g, points[:, k]) for k, g in enumerate(grid_f64(domain))))
    inside = ins[0] & ins[1] & ins[2]
    out = []
    for a in arrays:
        v = np.zeros(len(points))
        for di in (0, 1):
            for dj in (0, 1):
                for dk in (0, 1):
                    wgt = (ws[0] if di else 1 - ws[0]) * (ws[1] if dj else 1 - ws[1]) * (ws[2] if dk else 1 - ws[2])
                    v += wgt * np.float64(a[cells[0] + di, cells[1] + dj, cells[2] + dk])
        out.append(np.where(inside, v, np.nan))
    return out


def spectra(domain, probe, collection, wavelengths, ion_mass, instrument_fwhm=None, fields=None):
    """The Thomson-scattering spectra of `domain` -- ne, Te (external_Te), Z (external_Z; an array or a number), Ti
    (external_Ti; without it Ti = Te) and the flow V (external_V; without it none) -- for `probe` and the scattering volumes of
    `collection` at `wavelengths` [m], the ion's mass number ion_mass: a ThomsonSpectra with
        power = r_e^2 (1 - (ks . e)^2) P        (the polarisation factor is 1 when the probe has no polarisation)
    P engine.thomson's, in scattered energy per incident energy, per steradian and per metre of wavelength.  instrument_fwhm
    [m]: a Gaussian instrument function applied on the host (instrument_convolve; a uniform grid).  fields: a
    fields.SourceFields of the domain whose uploads are reused across calls (a fit loop, a sweep)."""
    if not isinstance(probe, Probe) or not isinstance(collection, Collection):
        raise ValueError("probe must be a thomson.Probe and collection a thomson.Collection")
    ne, Te, Z = getattr(domain, "ne", None), getattr(domain, "Te", None), getattr(domain, "Z", None)
    if ne is None or Te is None or Z is None:
        raise ValueError("the domain needs ne, Te (external_Te) and Z (external_Z)")
    lam = _wavelengths(wavelengths)
    ion_mass = float(ion_mass)
    if not (np.isfinite(ion_mass) and ion_mass > 0):
        raise ValueError(f"ion_mass must be finite and positive, got {ion_mass!r}")
    named = _plasma_arrays(domain, probe, collection)
    named["Z"] = np.asarray(Z) if np.ndim(Z) == 3 else None
    named["V"] = named.pop("V")  # the order the fields go up in: ne, Te, Ti, Z, V
    pts, wts = collection.quadrature(probe)
    with staged(domain, fields) as src:
        f = src.get_all(named)  # the kernel reads every field in one dtype
        P, weight = engine.thomson(f["ne"], f["Te"], f["Ti"], f["Z"] if f["Z"] is not None else float(Z), f["V"],
                                   probe.wavelength, ion_mass, pts, wts, probe.direction, collection.direction, lam)
        kernel_ms = f["ne"].last_kernel_ms
    return _spectra_of(domain, probe, collection, lam, named, P, weight, kernel_ms, instrument_fwhm)


def _wavelengths(wavelengths):
    lam = np.asarray(wavelengths, np.float64)
    if lam.ndim != 1 or not np.all(np.isfinite(lam)) or np.any(lam <= 0):
        raise ValueError("wavelengths must be one-dimensional, finite and positive")
    return lam


def _vector(domain, name, shape):
    """The domain's vector field `name` as an array of the grid's shape + (3,), or None."""
    v = getattr(domain, name, None)
    if v is None:
        return None
    v = np.asarray(v)
    if v.shape != tuple(shape) + (3,):
        raise ValueError(f"{name} has shape {v.shape}, the domain needs {tuple(shape) + (3,)}")
    return v


def _plasma_arrays(domain, probe, collection):
    """What spectra and spectra_multi read alike: {ne, Te, Ti | None, V | None} as arrays on the grid, after the check that every
    volume has a scattering wavevector."""
    if np.any(np.all(collection.direction == probe.direction[None, :], axis=1)):
        raise ValueError("a collection direction equals the probe's direction: no scattering wavevector")
    ne, Te, Ti = domain.ne, domain.Te, getattr(domain, "Ti", None)
    shape = np.shape(ne)
    return {"ne": np.asarray(ne), "Te": np.asarray(Te) if np.ndim(Te) == 3 else np.full(shape, float(Te)),
            "Ti": None if Ti is None else (np.asarray(Ti) if np.ndim(Ti) == 3 else np.full(shape, float(Ti))),
            "V": _vector(domain, "V", shape)}


def _spectra_of(domain, probe, collection, lam, named, P, weight, kernel_ms, instrument_fwhm):
    """The ThomsonSpectra of the engine's P and weight: r_e^2 and the polarisation factor, the instrument function, theta, alpha."""
    ks, ki = collection.direction, probe.direction
    pol = 1.0 if probe.polarisation is None else 1.0 - (ks @ probe.polarisation) ** 2
    power = (R_E * R_E * pol * np.ones(len(ks)))[:, None] * P
    if instrument_fwhm is not None:
        power = instrument_convolve(power, lam, instrument_fwhm)
    cth = np.clip(ks @ ki, -1.0, 1.0)
    theta = np.arccos(cth)
    k = 2.0 * (2.0 * np.pi / probe.wavelength) * np.sin(0.5 * theta)
    ne_c, Te_c = _at(domain, (named["ne"], named["Te"]), collection.points)
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = np.where((ne_c > 0) & (Te_c > 0), np.sqrt(ne_c * E_CHARGE / (EPS0 * Te_c)) / k, np.nan)
    return ThomsonSpectra(lam, power, weight, theta, alpha, kernel_ms)


class Species:
    """One ion species of spectra_multi: the mass number `mass`, the charge `charge` and the relative number fraction `fraction`
    among the ions (the fractions need not sum to 1) -- charge and fraction each a number or an (nx, ny, nz) array on the domain's
    grid, finite numbers not negative (a NaN or negative node of an array drops the points that read it)."""

    def __init__(self, mass, charge, fraction=1.0):
        self.mass = float(mass)
        if not (np.isfinite(self.mass) and self.mass > 0):
            raise ValueError(f"a species' mass must be finite and positive, got {mass!r}")
        self.charge, self.fraction = (self._value(name, v) for name, v in (("charge", charge), ("fraction", fraction)))

    @staticmethod
    def _value(name, v):
        if np.ndim(v) == 0:
            v = float(v)
            if not (np.isfinite(v) and v >= 0):
                raise ValueError(f"a species' {name} must be finite and not negative, got {v!r}")
            return v
        v = np.asarray(v)
        if v.ndim != 3:
            raise ValueError(f"a species' {name} must be a number or an (nx, ny, nz) array, got shape {v.shape}")
        return v


def drift_velocity(J, ne):
    """The electrons' drift relative to the ions [m/s] of the current density J (nx, ny, nz, 3) [A/m^2] and ne (nx, ny, nz)
    [m^-3]: -J/(e ne), and 0 where ne <= 0 -- what external_Vd takes."""
    J, ne = np.asarray(J, np.float64), np.asarray(ne, np.float64)
    if J.shape != ne.shape + (3,):
        raise ValueError(f"J has shape {J.shape}, ne's {ne.shape} needs {ne.shape + (3,)}")
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((ne > 0)[..., None], -J / (E_CHARGE * ne[..., None]), 0.0)


def _species_arrays(domain, probe, collection, wavelengths, species):
    """What spectra_multi and spectra_sg check and read alike: (wavelengths, the list of Species, {name: array | None} of ne, Te,
    Ti, V, Vd and the species' arrays Z0.., f0..)."""
    if not isinstance(probe, Probe) or not isinstance(collection, Collection):
        raise ValueError("probe must be a thomson.Probe and collection a thomson.Collection")
    if getattr(domain, "ne", None) is None or getattr(domain, "Te", None) is None:
        raise ValueError("the domain needs ne and Te (external_Te)")
    lam = _wavelengths(wavelengths)
    species = list(species)
    if not 1 <= len(species) <= engine.MAX_SPECIES or not all(isinstance(s, Species) for s in species):
        raise ValueError(f"species must be 1 to {engine.MAX_SPECIES} thomson.Species, got {len(species)} entries")
    named = _plasma_arrays(domain, probe, collection)
    shape = named["ne"].shape
    named["Vd"] = _vector(domain, "Vd", shape)
    for j, s in enumerate(species):
        for name, v in ((f"Z{j}", s.charge), (f"f{j}", s.fraction)):
            if np.ndim(v) == 3:
                if v.shape != shape:
                    raise ValueError(f"the array {name} of species {j} has shape {v.shape}, the domain needs {shape}")
                named[name] = v
    return lam, species, named


def spectra_multi(domain, probe, collection, wavelengths, species, instrument_fwhm=None, fields=None):
    """spectra for a plasma of several ion species whose electrons may drift against the ions: `species` is a sequence of 1 to 4
    Species (mass number, charge, relative number fraction; domain.Z is not read), the drift is domain.Vd (external_Vd; see
    drift_velocity; without it none); ne, Te, Ti and V are read as spectra reads them, and all species share Ti and V.  A
    ThomsonSpectra, power = r_e^2 (1 - (ks . e)^2) P with P engine.thomson_multi's.  The species' arrays go up under the names
    Z0.., f0.. and the drift as Vd, so a fields.SourceFields serves a fit loop over other arguments."""
    lam, species, named = _species_arrays(domain, probe, collection, wavelengths, species)
    pts, wts = collection.quadrature(probe)
    with staged(domain, fields) as src:
        f = src.get_all(named)  # the kernel reads every field in one dtype
        triples = [(s.mass, f.get(f"Z{j}", s.charge), f.get(f"f{j}", s.fraction)) for j, s in enumerate(species)]
        P, weight = engine.thomson_multi(f["ne"], f["Te"], f["Ti"], f["V"], f["Vd"], triples, probe.wavelength, pts, wts,
                                         probe.direction, collection.direction, lam)
        kernel_ms = f["ne"].last_kernel_ms
    return _spectra_of(domain, probe, collection, lam, named, P, weight, kernel_ms, instrument_fwhm)


def langdon_order(Z, intensity, Te, wavelength):
    """The order m of the super-Gaussian electron distribution exp(-(v/v_m)^m) that inverse-bremsstrahlung heating by a laser of
    `intensity` [W/m^2] and vacuum `wavelength` [m] drives in a plasma of charge Z and electron temperature Te [eV] (Matte et al.
    1988): m = 2 + 3/(1 + 1.66/alpha^0.724), alpha = Z v_osc^2/v_t^2 with v_osc = e E/(m_e omega), I = eps0 c E^2/2 and
    v_t^2 = k Te/m_e.  Numbers or arrays (broadcast); alpha = 0 gives 2 (Maxwellian), alpha -> infinity 5.  What external_order
    takes."""
    Z, intensity, Te, wavelength = (np.asarray(a, np.float64) for a in (Z, intensity, Te, wavelength))
    omega = 2.0 * np.pi * engine.c / wavelength
    v_osc2 = (2.0 * intensity / (EPS0 * engine.c)) * (E_CHARGE / (M_E * omega)) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = Z * v_osc2 / (E_CHARGE * Te / M_E)
        m = np.where(alpha > 0, 2.0 + 3.0 / (1.0 + 1.66 / np.power(alpha, 0.724)), 2.0)
    m = np.where(np.isnan(alpha), np.nan, m)
    return float(m) if m.ndim == 0 else m


def spectra_sg(domain, probe, collection, wavelengths, species, order=None, instrument_fwhm=None, fields=None):
    """spectra_multi for super-Gaussian (Langdon) electrons, f(v) ~ exp(-(v/v_m)^m) with Te kept as 2/3 of the mean energy: what
    inverse-bremsstrahlung heating by the probe or the drive makes of the electrons.  order: the local m -- None reads
    domain.order (external_order; see langdon_order), an (nx, ny, nz) array or a number; an array's values are clamped to [2, 5]
    and a NaN node drops the points that read it, a number must lie in [2, 5].  m = 2 returns spectra_multi's bits.  The order's
    array goes up under the name "order".  A ThomsonSpectra, power = r_e^2 (1 - (ks . e)^2) P with P engine.thomson_sg's.  Not
    modelled: per-species Ti, magnetised and relativistic corrections, anisotropic distortions of the electron distribution, m
    outside [2, 5], more than one GPU."""
    lam, species, named = _species_arrays(domain, probe, collection, wavelengths, species)
    if order is None:
        order = getattr(domain, "order", None)
        if order is None:
            raise ValueError("the domain holds no order (external_order); give order=")
    if np.ndim(order) == 0:
        order = float(order)
        if not 2.0 <= order <= 5.0:
            raise ValueError(f"a uniform order must lie in [2, 5], got {order!r}")
    else:
        order = np.asarray(order)
        if order.shape != named["ne"].shape:
            raise ValueError(f"order has shape {order.shape}, the domain needs {named['ne'].shape}")
        named["order"] = order
    pts, wts = collection.quadrature(probe)
    with staged(domain, fields) as src:
        f = src.get_all(named)  # the kernel reads every field in one dtype
        triples = [(s.mass, f.get(f"Z{j}", s.charge), f.get(f"f{j}", s.fraction)) for j, s in enumerate(species)]
        P, weight = engine.thomson_sg(f["ne"], f["Te"], f["Ti"], f["V"], f["Vd"], triples, f.get("order", order), probe.wavelength,
                                      pts, wts, probe.direction, collection.direction, lam)
        kernel_ms = f["ne"].last_kernel_ms
    return _spectra_of(domain, probe, collection, lam, named, P, weight, kernel_ms, instrument_fwhm)
