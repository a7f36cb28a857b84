"""Proton (charged-particle) radiography of a domain's E and B, and of its matter (no reference counterpart).

    src = radiography.ProtonSource(14.7, position=(0, 0, -10e-3), axis="z", half_angle=0.2, n=1_000_000)
    rad = domain.proton_radiograph(src, det_pos=0.15)       # or radiography.radiograph(domain, src, 0.15)
    rad.counts, rad.fluence(), rad.hits, rad.magnification

A point source of mono-energetic particles inside a cone about a grid axis; each particle flies ballistically to the face of the
grid box where it enters (host, float64), is pushed through the trilinear fields by the GPU with a fixed step until it leaves the
box (engine.push_particles -> sr_particles_push; include/synthray.h states the rule), and is projected onto the detector plane
coordinate[axis] == det_pos.  The image shows the transverse fields with no density weighting.  Validity: prescribed fields only
(no self-fields), no scattering or stopping in the plasma, a fixed step, trilinear fields (div B is only as good as the input's).

    rad = domain.proton_radiograph(src, det_pos=0.15, material=radiography.Material.CH(), stop_energy_MeV=0.1)
    rad.energy_MeV, rad.stopped, rad.scatter_sigma(), rad.scattered(seed=1).counts, rad.counts_in(10.0, 12.0)

With a Material the particles also cross the domain's ne (mean ionisation: external_Z): Bethe stopping by the free and the bound
electrons as a drag, and the Fermi-Eyges moments of the multiple-scattering power along each path, from which scatter_sigma() and
scattered() give the blur on the detector (engine.push_particles_matter -> sr_particles_push_matter).  Validity there: a cold
target or v >> the electrons' thermal speed, no nuclear reactions, no straggling, a single material, small-angle scattering that
does not feed back on the path.
"""
from __future__ import annotations

import numpy as np

from . import engine
from .fields import grid_f64, locate, staged

c = engine.c
M_P = 1.67262192369e-27      # kg (CODATA 2018)
E_CHARGE = engine.E_CHARGE   # C
_AXES = {"x": 0, "y": 1, "z": 2}


def _axis(axis) -> int:
    if isinstance(axis, str) and axis in _AXES:
        return _AXES[axis]
    if not isinstance(axis, str) and axis in (0, 1, 2):
        return int(axis)
    raise ValueError(f"axis must be 'x', 'y', 'z' or 0, 1, 2, got {axis!r}")


def lateral_axes(axis):
    """The two axes other than `axis`, in x < y < z order: the detector's (u, v), sr_volume_project's convention."""
    return tuple(k for k in range(3) if k != axis)


class ProtonSource:
    """A point source of n particles of kinetic energy energy_MeV [MeV] at `position` [m], emitted inside a cone of half-angle
    half_angle [rad] about the grid axis `axis`, in its positive (toward = +1) or negative (-1) sense.  pattern "random":
    directions uniform in solid angle inside the cone, from numpy's default_rng(seed).  "lattice": a square lattice of
    floor(sqrt(n))^2 directions in tangent space, inscribed in the cone (|tan| <= tan(half_angle)/sqrt(2) on both lateral axes);
    n becomes that square number.  mass [kg] and charge [C] make it a source of any charged particle:
    gamma = 1 + T/(m c^2), |u| = |gamma v| = c sqrt(gamma^2 - 1)."""

    def __init__(self, energy_MeV, position, axis, toward=+1, *, half_angle, n, seed=0, pattern="random", mass=M_P,
                 charge=E_CHARGE):
        self.axis = _axis(axis)
        if toward not in (1, -1):
            raise ValueError(f"toward must be +1 or -1, got {toward!r}")
        self.toward = int(toward)
        self.position = np.asarray(position, np.float64)
        if self.position.shape != (3,) or not np.all(np.isfinite(self.position)):
            raise ValueError("position must be three finite numbers")
        self.energy_MeV, self.half_angle = float(energy_MeV), float(half_angle)
        if not (np.isfinite(self.energy_MeV) and self.energy_MeV > 0):
            raise ValueError(f"energy_MeV must be finite and positive, got {energy_MeV!r}")
        if not 0 < self.half_angle < np.pi / 2:
            raise ValueError(f"half_angle must lie in (0, pi/2), got {half_angle!r}")
        if pattern not in ("random", "lattice"):
            raise ValueError(f"pattern must be 'random' or 'lattice', got {pattern!r}")
        self.pattern, self.seed = pattern, seed
        self.mass, self.charge = float(mass), float(charge)
        if not (np.isfinite(self.mass) and self.mass > 0 and np.isfinite(self.charge)):
            raise ValueError("mass must be finite and positive and charge finite")
        n = int(n)
        if n < 1:
            raise ValueError(f"n must be at least 1, got {n}")
        self.n = int(np.floor(np.sqrt(n))) ** 2 if pattern == "lattice" else n

    @property
    def gamma(self):
        return 1.0 + self.energy_MeV * 1e6 * E_CHARGE / (self.mass * c * c)

    @property
    def u(self):
        """|gamma v| [m/s]."""
        g = self.gamma
        return c * np.sqrt(g * g - 1.0)

    @property
    def speed(self):
        return self.u / self.gamma

    @property
    def qm(self):
        return self.charge / self.mass

    def directions(self):
        """(3, n) unit vectors."""
        a = self.axis
        b, cc = lateral_axes(a)
        d = np.empty((3, self.n))
        if self.pattern == "random":
            rng = np.random.default_rng(self.seed)
            cos_t = 1.0 - rng.random(self.n) * (1.0 - np.cos(self.half_angle))
            phi = 2 * np.pi * rng.random(self.n)
            sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
            d[b], d[cc], d[a] = sin_t * np.cos(phi), sin_t * np.sin(phi), self.toward * cos_t
        else:
            m = int(round(np.sqrt(self.n)))
            T = np.tan(self.half_angle) / np.sqrt(2.0)
            t = np.linspace(-T, T, m) if m > 1 else np.zeros(1)
            tb, tc = (v.ravel() for v in np.meshgrid(t, t, indexing="ij"))
            r = np.sqrt(1.0 + tb * tb + tc * tc)
            d[b], d[cc], d[a] = tb / r, tc / r, self.toward / r
        return d

    def states(self):
        """s0 (6, n): x y z [m], ux uy uz = gamma*v [m/s], every particle at the source."""
        s = np.empty((6, self.n))
        s[:3] = self.position[:, None]
        s[3:] = self.u * self.directions()
        return s


def entry(s0, lo, hi):
    """The particles s0 (6, n) flown ballistically to where they enter the box lo..hi (3 each): (s, meets) with s a copy whose
    positions are the entry points -- the coordinate of the face that is crossed last is set to the face's value exactly; a
    particle that starts inside stays where it is -- and meets (n) bool, False for the lines that never meet the box (left as
    they are).  The slab method: per axis the parameter interval in which x + u*t lies between the faces, intersected."""
    s = np.array(s0, np.float64, copy=True)
    x, u = s[:3], s[3:]
    lo, hi = np.asarray(lo, np.float64)[:, None], np.asarray(hi, np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - x) / u, (hi - x) / u
    still = u == 0.0  # an axis without motion: inside its slab for all t, or never
    inside = (x >= lo) & (x <= hi)
    t_in = np.where(still, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
    t_out = np.where(still, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
    k = np.argmax(t_in, axis=0)
    t0, t9 = np.max(t_in, axis=0), np.min(t_out, axis=0)
    meets = t9 >= np.maximum(t0, 0.0)
    move = meets & (t0 > 0.0)
    t = np.where(move, t0, 0.0)
    x += np.where(move, u * t, 0.0)
    cols = np.nonzero(move)[0]
    face = np.where(u[k[cols], cols] > 0.0, lo[k[cols], 0], hi[k[cols], 0])
    x[k[cols], cols] = face
    return s, meets


def entry_cell_order(s, g):
    """The stable order of the states s (6, n) by the cell (x slowest, z fastest: the fields' memory order) their positions lie in;
    g: the three float64 node arrays.  Neighbouring lanes of the push kernel then gather neighbouring nodes."""
    cell = [locate(g[k], s[k])[0] for k in range(3)]
    key = (cell[0] * (len(g[1]) - 1) + cell[1]) * (len(g[2]) - 1) + cell[2]
    return np.argsort(key, kind="stable")


def project(s, axis, det_pos, hit_scale=1e3):
    """The ballistic projection of the states s (6, n) onto the plane coordinate[axis] == det_pos: (hits (2, n), missed (n) bool),
    the detector line of sr_particles_push's rule in NumPy."""
    b, cc = lateral_axes(axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = (det_pos - s[axis]) / s[3 + axis]
        hits = np.stack([(s[b] + s[3 + b] * tau) * hit_scale, (s[cc] + s[3 + cc] * tau) * hit_scale])
    return hits, ~(np.isfinite(tau) & (tau > 0.0))


MEV = 1e6 * E_CHARGE  # J
AMU = 1.66053906660e-27  # kg (CODATA 2018)


class Material:
    """What radiograph(material=...) needs of the matter the particles cross: the nuclear charge Zn and mass number A of its
    (mean) atom, the mean excitation energy I_eV [eV] of Bethe's logarithm for the bound electrons, and the logarithm of the
    multiple-scattering power, coulomb_log; None: ln(204 Zn^(-1/3)), the screened-nucleus value of Jackson 13.6 (Classical
    Electrodynamics, 3rd ed., section 13.6).  A compound is its mean atom (CH: Zn = 3.5, A = 6.5)."""

    # name: (Zn, A, I [eV]).  I: ICRU Report 49 (1993), Stopping Powers and Ranges for Protons and Alpha Particles, as tabulated
    # by NIST PSTAR's material list (CH: polystyrene); A: the standard atomic weights
    TABLE = {"CH": (3.5, 6.5095, 68.7), "Al": (13.0, 26.9815, 166.0), "Cu": (29.0, 63.546, 322.0), "W": (74.0, 183.84, 727.0)}

    def __init__(self, Zn, A, I_eV, coulomb_log=None):
        self.Zn, self.A, self.I_eV = float(Zn), float(A), float(I_eV)
        if not (np.isfinite(self.Zn) and self.Zn > 0 and np.isfinite(self.A) and self.A > 0 and np.isfinite(self.I_eV) and self.I_eV > 0):
            raise ValueError("Zn, A and I_eV must be finite and positive")
        self.coulomb_log = float(np.log(204.0 * self.Zn ** (-1.0 / 3.0))) if coulomb_log is None else float(coulomb_log)
        if not (np.isfinite(self.coulomb_log) and self.coulomb_log >= 0):
            raise ValueError(f"coulomb_log must be finite and not negative, got {coulomb_log!r}")

    @property
    def I(self):
        """The mean excitation energy [J]."""
        return self.I_eV * E_CHARGE

    def electron_density(self, rho, Z=None):
        """ne [m^-3] of the mass density rho [kg/m^3] at the mean ionisation Z (None: fully ionised, Zn)."""
        return np.asarray(rho, np.float64) * (self.Zn if Z is None else Z) / (self.A * AMU)

    @classmethod
    def named(cls, name, coulomb_log=None):
        return cls(*cls.TABLE[name], coulomb_log=coulomb_log)

    @classmethod
    def CH(cls):
        return cls.named("CH")

    @classmethod
    def Al(cls):
        return cls.named("Al")

    @classmethod
    def Cu(cls):
        return cls.named("Cu")

    @classmethod
    def W(cls):
        return cls.named("W")


def kinetic_energy(u, mass):
    """m c^2 (gamma - 1) [J] of u = gamma*v (3, n), as m c^2 q/(gamma + 1) with q = |u|^2/c^2: no cancellation."""
    q = np.sum(np.square(u), axis=0) / (c * c)
    return mass * c * c * q / (np.sqrt(1.0 + q) + 1.0)


class Radiograph:
    """counts (ny, nx) float64: particles per detector bin, x = the first lateral axis (x < y < z order) and y the second;
    edges = (x edges, y edges) in the unit of hits (mm with hit_scale = 1e3); hits (2, n), flags (n) uint8
    (engine.PUSH_UNFINISHED | engine.PUSH_MISSED | engine.PUSH_STOPPED), steps (n) int32 (0: the particle never met the box) in
    the source's order; sf (6, n) the states on leaving the box; magnification = (d_src + d_det)/d_src for the box's centre plane;
    stats: an engine.PushStats of the pushed particles.  With radiograph(material=...): energy_MeV (n) on leaving the box or
    stopping, stopped (n) bool, moments (4, n): M0, M1, M2 of the scattering power over each path and the path's length
    (sr_particles_push_matter); stats is an engine.PushMatterStats.  Without a material these three are None."""

    def __init__(self, counts, edges, hits, flags, steps, sf, magnification, stats, reference_hits, dt, max_steps, *, energy_MeV=None,
                 moments=None, axis=None, det_pos=None, hit_scale=1e3):
        self.counts, self.edges, self.hits, self.flags, self.steps, self.sf = counts, edges, hits, flags, steps, sf
        self.magnification, self.stats, self.dt, self.max_steps = magnification, stats, dt, max_steps
        self._reference_hits = reference_hits
        self.energy_MeV, self.moments = energy_MeV, moments
        self.stopped = None if moments is None else (np.asarray(flags) & engine.PUSH_STOPPED) > 0
        self.axis, self.det_pos, self.hit_scale = axis, det_pos, hit_scale

    def _need_matter(self):
        if self.moments is None:
            raise ValueError("this radiograph was made without a material: it has no energies and no scattering moments")

    def _bin(self, hits, keep):
        (x0, x1), (y0, y1) = ((e[0], e[-1]) for e in self.edges)
        h = np.ascontiguousarray(hits[:, keep])
        return engine.hist2d(h[0], h[1], len(self.edges[0]) - 1, len(self.edges[1]) - 1, x0, x1, y0, y1).astype(np.float64)

    def scatter_sigma(self):
        """(sigma_theta (n) [rad], sigma_y (n) [m]): the Fermi-Eyges standard deviations, per plane of projection, of each
        particle's direction and of its position on the detector plane, perpendicular to its flight: with L = the path
        length inside the box + the flight from there to the plane, sigma_theta^2 = M0/2 and sigma_y^2 = (L^2 M0 - 2 L M1 +
        M2)/2 (M_k the moments of the scattering power d<theta^2>/ds over the path).  NaN sigma_y for a particle that does
        not reach the plane."""
        self._need_matter()
        M0, M1, M2, s_end = self.moments
        a = self.axis
        with np.errstate(divide="ignore", invalid="ignore"):
            tau = (self.det_pos - self.sf[a]) / self.sf[3 + a]
            L = s_end + tau * np.sqrt(np.sum(np.square(self.sf[3:]), axis=0))
            var_y = 0.5 * ((L * L * M0 - 2.0 * L * M1) + M2)
            ok = np.isfinite(tau) & (tau > 0)
        return np.sqrt(0.5 * M0), np.where(ok, np.sqrt(np.maximum(var_y, 0.0)), np.nan)

    def scattered_hits(self, seed):
        """hits (2, n) displaced by multiple scattering: to each particle's point on the plane two normal deviates of
        scatter_sigma()'s sigma_y (numpy's default_rng(seed), drawn in the source's order) are added along e1 and e2, the
        two unit vectors perpendicular to its flight n^ (e1: the first lateral axis made perpendicular to n^, e2 = n^ x e1),
        and the displaced line is met with the plane: a displacement d moves the hit by d - n^ d_a/n_a.  Hits that are not
        finite, and particles without scattering, stay as they are."""
        self._need_matter()
        _, sig = self.scatter_sigma()
        n = self.hits.shape[1]
        z = np.random.default_rng(seed).standard_normal((2, n))
        a = self.axis
        b, cc = lateral_axes(a)
        with np.errstate(divide="ignore", invalid="ignore"):
            nh = self.sf[3:] / np.sqrt(np.sum(np.square(self.sf[3:]), axis=0))
            e1 = -nh[b] * nh
            e1[b] += 1.0
            e1 /= np.sqrt(np.sum(e1 * e1, axis=0))
            e2 = np.cross(nh, e1, axis=0)
            d = sig * (z[0] * e1 + z[1] * e2)
            shift = np.stack([d[b] - nh[b] * d[a] / nh[a], d[cc] - nh[cc] * d[a] / nh[a]]) * self.hit_scale
        ok = np.all(np.isfinite(shift), axis=0) & np.all(np.isfinite(self.hits), axis=0)
        return np.where(ok, self.hits + np.where(ok, shift, 0.0), self.hits)

    def scattered(self, seed):
        """This radiograph with multiple scattering sampled on the host: a new Radiograph whose hits are scattered_hits(seed)
        and whose counts are those hits (flags == 0) binned again by engine.hist2d on the same detector; everything else is
        shared.  Not modelled: sampling on the device, the correlated change of direction (only the plane's image is kept)."""
        hits = self.scattered_hits(seed)
        return Radiograph(self._bin(hits, self.flags == 0), self.edges, hits, self.flags, self.steps, self.sf, self.magnification,
                          self.stats, self._reference_hits, self.dt, self.max_steps, energy_MeV=self.energy_MeV,
                          moments=self.moments, axis=self.axis, det_pos=self.det_pos, hit_scale=self.hit_scale)

    def counts_in(self, e_lo, e_hi):
        """The image of one energy window: the counts of the particles with flags == 0 and e_lo <= energy_MeV < e_hi, what one
        layer of a film stack or one etch depth of CR-39 records."""
        self._need_matter()
        return self._bin(self.hits, (self.flags == 0) & (self.energy_MeV >= e_lo) & (self.energy_MeV < e_hi))

    def reference_counts(self):
        """The counts the same source gives without fields: its straight lines binned on the same detector."""
        (x0, x1), (y0, y1) = ((e[0], e[-1]) for e in self.edges)
        ok = np.all(np.isfinite(self._reference_hits), axis=0)
        h = self._reference_hits[:, ok]
        return engine.hist2d(h[0], h[1], len(self.edges[0]) - 1, len(self.edges[1]) - 1, x0, x1, y0, y1).astype(np.float64)

    def fluence(self):
        """counts over the no-field counts of the same source; NaN where the source sends nothing."""
        ref = self.reference_counts()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(ref > 0, self.counts / ref, np.nan)


def default_steps(domain, source, dt=None):
    """(dt, max_steps): dt, or a quarter of the smallest cell width over |v|; twice the box diagonal over |v| dt."""
    g = grid_f64(domain)
    h = min(float(np.min(np.diff(a))) for a in g)
    diag = float(np.sqrt(sum((a[-1] - a[0]) ** 2 for a in g)))
    dt = 0.25 * h / source.speed if dt is None else float(dt)
    return dt, int(np.ceil(2.0 * diag / (source.speed * dt)))


def radiograph(domain, source, det_pos, dt=None, max_steps=None, image=None, sort=True, hit_scale=1e3, bins=(256, 256),
               fields=None, material=None, stop_energy_MeV=0.0, scatter_seed=None):
    """The radiograph of `domain` (B from external_B / test_B, E from external_E; at least one) by `source` on the plane
    coordinate[source.axis] == det_pos [m].  dt, max_steps: default_steps.  image: an engine.DetectorImage of counts the pushed
    particles are added to on the device (zero it first if it is reused), or None for a detector of `bins` over the shadow of
    the box's centre plane.  sort: order the particles by entry cell before the upload (neighbouring lanes gather neighbouring
    nodes) and undo the order on the outputs; the per-particle results are the same bits either way.  fields: a
    fields.SourceFields of the domain whose uploads are reused.  Returns a Radiograph.
    material: a Material switches to the push through matter (engine.push_particles_matter -> sr_particles_push_matter): the
    particles lose energy in the domain's ne by Bethe's stopping power of the free and the bound electrons -- the mean
    ionisation is the domain's Z (external_Z: a grid or a number) -- and gather the moments of the multiple-scattering power;
    E and B may then both be absent.  stop_energy_MeV: a particle below it is stopped and not binned.  scatter_seed: not None
    returns Radiograph.scattered(scatter_seed).  Not modelled: straggling, nuclear reactions, more than one material, large-angle
    scattering, scattering that feeds back on the path, sampling on the device."""
    a = source.axis
    B, E = getattr(domain, "B", None), getattr(domain, "E", None)
    if material is None:
        if B is None and E is None:
            raise ValueError("the domain holds neither B (external_B / test_B) nor E (external_E)")
        if scatter_seed is not None or stop_energy_MeV:
            raise ValueError("stop_energy_MeV and scatter_seed need a material")
    else:
        if not isinstance(material, Material):
            raise ValueError("material must be a radiography.Material")
        ne, Z = getattr(domain, "ne", None), getattr(domain, "Z", None)
        if ne is None or Z is None:
            raise ValueError("with a material the domain needs ne and Z (external_Z: a grid or a number)")
    det_pos = float(det_pos)
    g = grid_f64(domain)
    lo, hi = np.array([v[0] for v in g]), np.array([v[-1] for v in g])
    dt, default_max = default_steps(domain, source, dt)
    max_steps = default_max if max_steps is None else int(max_steps)
    centre = 0.5 * (lo[a] + hi[a])
    d_src, d_det = centre - source.position[a], det_pos - centre
    if d_src == 0 or (d_src > 0) != (source.toward > 0) or (d_det > 0) != (source.toward > 0):
        raise ValueError("the source must look at the box's centre plane and the detector lie beyond it")
    magnification = (d_src + d_det) / d_src
    b, cc = lateral_axes(a)
    if image is None:
        rng = []
        for k in (b, cc):
            e = sorted((source.position[k] + (v - source.position[k]) * magnification) * hit_scale for v in (lo[k], hi[k]))
            rng += e
        image = engine.DetectorImage(engine.IMG_COUNTS, int(bins[0]), int(bins[1]), *rng)
        own_image = True
    else:
        if not isinstance(image, engine.DetectorImage) or image.kind != engine.IMG_COUNTS:
            raise ValueError("image must be an engine.DetectorImage of counts")
        own_image = False

    s0 = source.states()
    n = s0.shape[1]
    s_in, meets = entry(s0, lo, hi)
    ref_hits, missed = project(s0, a, det_pos, hit_scale)  # the straight lines: the no-field reference of fluence(), and where
    sf, hits = s0.copy(), ref_hits.copy()                  # the lines that never meet the box end up (steps = 0)
    flags = np.where(missed, engine.PUSH_MISSED, 0).astype(np.uint8)
    steps = np.zeros(n, np.int32)
    idx = np.nonzero(meets)[0]
    stats = engine.PushStats(0.0, 0, 0, 0, 0) if material is None else engine.PushMatterStats(0.0, 0, 0, 0, 0, 0)
    energy = moments = None
    if material is not None:  # a line that never meets the box keeps the source's energy and gathers nothing
        energy, moments = kinetic_energy(s0[3:], source.mass), np.zeros((4, n))
    with staged(domain, fields) as src:  # fields of another domain are refused whether or not a particle meets the box
        if len(idx):
            sub = s_in[:, idx]
            if sort:
                order = entry_cell_order(sub, g)
                idx, sub = idx[order], sub[:, order]
            named = {"E": None if E is None else np.asarray(E), "B": None if B is None else np.asarray(B)}
            if material is None:
                f = src.get_all(named)
                out = engine.push_particles(f["E"], f["B"], np.ascontiguousarray(sub), source.qm, dt, max_steps, a, det_pos, hit_scale,
                                            image=image)
            else:
                f = src.get_all({**named, "ne": np.asarray(ne), "Z": np.asarray(Z) if np.ndim(Z) == 3 else None})
                out = engine.push_particles_matter(f["E"], f["B"], f["ne"], f["Z"] if f["Z"] is not None else float(Z),
                                                   np.ascontiguousarray(sub), source.qm, dt, max_steps, a, det_pos, hit_scale,
                                                   mass=source.mass, z=source.charge / E_CHARGE, Zn=material.Zn, I=material.I,
                                                   lnLs=material.coulomb_log, stop_energy=stop_energy_MeV * MEV, image=image)
                energy[idx], moments[:, idx] = out["energy"], out["moments"]
            sf[:, idx], hits[:, idx], flags[idx], steps[idx], stats = out["sf"], out["hits"], out["flags"], out["steps"], out["stats"]
    counts = np.array(image.counts_f64())
    x_lo, x_hi, y_lo, y_hi = image.range
    rest = ~meets & (flags == 0)
    if np.any(rest):
        counts = counts + engine.hist2d(hits[0, rest], hits[1, rest], image.nx, image.ny, x_lo, x_hi, y_lo, y_hi)
    edges = (np.linspace(x_lo, x_hi, image.nx + 1), np.linspace(y_lo, y_hi, image.ny + 1))
    if own_image:
        image.close()
    rad = Radiograph(np.asarray(counts, np.float64), edges, hits, flags, steps, sf, magnification, stats, ref_hits, dt, max_steps,
                     energy_MeV=None if energy is None else energy / MEV, moments=moments, axis=a, det_pos=det_pos,
                     hit_scale=hit_scale)
    return rad if scatter_seed is None else rad.scattered(scatter_seed)
