"""Sightlines: emission and absorption along lines that are not grid columns (no reference counterpart).

    cam = sightlines.PinholeCamera(pinhole=(0, 0, 30e-3), look=(0, 0.2, -1), up=(0, 1, 0), det_distance=0.3, pixels=(256, 256), pitch=50e-6)
    em = domain.sightline_emission(cam, wavelengths=[532e-9])           # or sightlines.sightline_emission(domain, cam, ...)
    em.intensity, em.optical_depth, em.transmission                     # (n_band, nu, nv)
    em.column, em.chord, em.steps                                       # (nu, nv): integral of ne dl [m^-2], length in the box [m]
    bl = sightlines.PointBacklighter(source=(0, 0, -20e-3), look=(0, 0, 1), up=(0, 1, 0), det_distance=0.5, pixels=(512, 512),
                                     pitch=100e-6, radiance=[3e-7])
    domain.sightline_emission(bl, table=opacity_table)
    sightlines.Chords(origins, directions, toward=-1)                   # any lines: diodes, bolometers, spectrometer chords
    sp = domain.sightline_spectra(chords, photon_energies=np.geomspace(1, 50, 2048))   # a spectrum per line, a GPU lane per frequency
    sp.intensity, sp.signal(response)                                   # (N, n_freq); the response-weighted integral per line
    ls = domain.sightline_lines(chords, line_table, wavelengths=lam)    # Doppler-shifted, thermally broadened lines (LineSpectra)
    ls.moments(window)                                                  # per chord and line: radiance, flow velocity, Ti

emission.self_emission and table_emission march columns parallel to a grid axis.  Here the same radiative-transfer recurrence,
dI/ds = alpha (S - I), runs along half-lines from a point: a pinhole camera looks along lines that CONVERGE on the pinhole
(perspective, magnification, a view from any direction without resampling the volume with rotated()), a point-projection
backlighter (an X-pinch, a laser-driven foil) sends DIVERGING lines from its source through the plasma onto film.  Each line is
clipped to the domain's box and sampled about `step` apart, the fields interpolated trilinearly at every sample, on the GPU
(engine.sightlines -> sr_field_sightlines; include/synthray.h states the rule).  The node is self_emission's (wavelengths=: the
NRL inverse-bremsstrahlung coefficient and Planck's source function) or table_emission's (table=: an OpacityTable).

Not modelled: a finite pinhole or source size (every line is a single ray through a point), the cos^4 and solid-angle factors
that turn radiance into film exposure, refraction of the light, the detector's response, a table's own ionisation (Z is the
domain's); one GPU.
"""
from __future__ import annotations

import numpy as np

from . import engine
from .emission import _check_table, _Maps, _omegas, _upload

c = engine.c


def _vec(name, v):
    v = np.asarray(v, np.float64)
    if v.shape != (3,) or not np.all(np.isfinite(v)):
        raise ValueError(f"{name} must be three finite numbers, got {v!r}")
    return v


def frame(look, up):
    """The detector's right-handed frame (x, y, l) for a viewing direction `look` and any `up` not parallel to it: l = look / |look|,
    y = the part of up perpendicular to l, normalised, x = y cross l (so that x cross y = l)."""
    look, up = _vec("look", look), _vec("up", up)
    n = np.linalg.norm(look)
    if n == 0:
        raise ValueError("look must not be zero")
    l = look / n
    y = up - np.dot(up, l) * l
    ny = np.linalg.norm(y)
    if ny <= 1e-12 * max(np.linalg.norm(up), 1e-300):
        raise ValueError("up must not be parallel to look")
    y = y / ny
    return np.cross(y, l), y, l


def _morton(i, j):
    """Bit-interleaved (Z-order) key of the non-negative integer pairs (i, j), i in the odd bits."""
    key = np.zeros(np.shape(i), np.int64)
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    for b in range(24):
        key |= ((i >> b) & 1) << (2 * b + 1) | ((j >> b) & 1) << (2 * b)
    return key


def tile_order(nu, nv, tile=8):
    """The order in which a (nu, nv) pixel grid is handed to the kernel: perm (nu*nv) int64, line k is pixel perm[k] = i*nv + j.
    Pixels go in tiles of tile x tile (row-major inside a tile: 64 pixels, one wavefront per full tile), the tiles in Morton order,
    so that the lines of a wavefront, and of the wavefronts that run together, pass through neighbouring cells.  Tiles cut by
    the grid's edge are shorter; nothing is padded, so perm is a permutation of range(nu*nv)."""
    i, j = (a.ravel() for a in np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij"))
    inside = (i % tile) * tile + j % tile
    return np.lexsort((inside, _morton(i // tile, j // tile))).astype(np.int64)


class Chords:
    """Any lines: origins and directions (3, N) [m] (a direction need not be a unit vector), toward = +1 where the light
    travels along +direction, away from the origin (a source there), -1 where it travels towards the origin (a detector there).
    backlight: (n_band, N), (n_band,) or a number: the radiance behind the far end of every line, or None."""

    def __init__(self, origins, directions, toward, backlight=None):
        self.origins, self.directions = np.array(origins, np.float64, ndmin=2), np.array(directions, np.float64, ndmin=2)
        if self.origins.shape[0] != 3 or self.origins.ndim != 2 or self.directions.shape != self.origins.shape:
            raise ValueError(f"origins and directions must both have shape (3, N), got {self.origins.shape} and {self.directions.shape}")
        if toward not in (1, -1):
            raise ValueError(f"toward must be +1 or -1, got {toward!r}")
        self.toward = int(toward)
        self.shape = (self.origins.shape[1],)
        self.radiance = backlight

    def lines(self):
        """(origins (3, N), directions (3, N)) in the view's own order (pixel i*nv + j for a pixel grid)."""
        return self.origins, self.directions

    def order(self):
        """The order the lines are handed to the kernel in (a permutation of range(N)), or None: as they are."""
        return None

    def backlight(self, n_band):
        if self.radiance is None:
            return None
        r = np.asarray(self.radiance, np.float64)
        n = int(np.prod(self.shape))
        if r.ndim <= 1:
            r = np.broadcast_to(r.reshape(-1, 1), (n_band, n)) if r.size in (1, n_band) else None
        elif r.shape != (n_band, n):
            r = None
        if r is None:
            raise ValueError(f"the backlight must be a number, one per band ({n_band}) or (n_band, N), got shape {np.shape(self.radiance)}")
        return np.ascontiguousarray(r)


class _PixelView(Chords):
    """A flat detector of pixels = (nu, nv) pixels of size `pitch` [m]: pixel (i, j) has its centre at
    centre + u_i*x + v_j*y with u_i = (i - (nu-1)/2)*pitch, v_j = (j - (nv-1)/2)*pitch and (x, y, l) = frame(look, up)."""

    def __init__(self, point, look, up, det_distance, pixels, pitch, side, toward, radiance=None):
        self.point = _vec("the pinhole / source", point)
        self.x, self.y, self.l = frame(look, up)
        self.det_distance, self.pitch = float(det_distance), float(pitch)
        if not (np.isfinite(self.det_distance) and self.det_distance > 0 and np.isfinite(self.pitch) and self.pitch > 0):
            raise ValueError("det_distance and pitch must be finite and positive")
        nu, nv = (int(m) for m in pixels)
        if nu < 1 or nv < 1:
            raise ValueError(f"pixels must be two positive counts, got {pixels!r}")
        self.shape, self.toward, self.radiance = (nu, nv), toward, radiance
        self.u = (np.arange(nu) - (nu - 1) / 2) * self.pitch
        self.v = (np.arange(nv) - (nv - 1) / 2) * self.pitch
        self._side = side

    def pixel_centres(self):
        """(3, nu, nv) [m]."""
        centre = self.point + self._side * self.det_distance * self.l
        return (centre[:, None, None] + self.x[:, None, None] * self.u[None, :, None] + self.y[:, None, None] * self.v[None, None, :])

    def lines(self):
        pix = self.pixel_centres().reshape(3, -1)
        o = np.broadcast_to(self.point[:, None], pix.shape)
        return np.ascontiguousarray(o), self._side * (pix - o)

    def order(self):
        return tile_order(*self.shape)

    def magnification(self, object_distance):
        """Image size / object size for an object plane object_distance [m] in front of the pinhole / source along look."""
        return self.det_distance / float(object_distance)


class PinholeCamera(_PixelView):
    """An ideal pinhole at `pinhole` looking along `look`, its detector det_distance BEHIND it: pixel (i, j) has its centre at
    pinhole - l*det_distance + u_i*x + v_j*y, its line starts at the pinhole with d = pinhole - pixel (out into the scene) and the
    light travels towards the pinhole (toward = -1).  The image is inverted, as a pinhole's is: the object point pinhole + s*l + a*x
    + b*y lands at (u, v) = -(a, b) * det_distance / s.  look and up are any two non-parallel vectors: oblique views need no
    rotated().  magnification(object_distance) = det_distance / object_distance."""

    def __init__(self, pinhole, look, up, det_distance, pixels, pitch):
        super().__init__(pinhole, look, up, det_distance, pixels, pitch, side=-1, toward=-1)
        self.pinhole = self.point


class PointBacklighter(_PixelView):
    """A point source at `source` shining along `look` onto a detector det_distance away: pixel (i, j) has its centre at
    source + l*det_distance + u_i*x + v_j*y, its line starts at the source with d = pixel - source and the light travels away
    from the source (toward = +1).  radiance: the source's spectral radiance per band (a number, or one per band) -- the
    backlight of every line.  magnification(object_distance) = det_distance / object_distance (point projection)."""

    def __init__(self, source, look, up, det_distance, pixels, pitch, radiance):
        super().__init__(source, look, up, det_distance, pixels, pitch, side=+1, toward=+1, radiance=radiance)
        self.source = self.point


class _LineMaps(_Maps):
    """What the two results along lines share: the view, the two maps and the per-line column, chord and steps (view.shape)."""

    def __init__(self, view, intensity, optical_depth, column, chord, steps):
        self.view = view
        self.intensity, self.optical_depth = np.asarray(intensity, np.float64), np.asarray(optical_depth, np.float64)
        self.column, self.chord, self.steps = np.asarray(column, np.float64), np.asarray(chord, np.float64), np.asarray(steps, np.int32)

    def _expect(self, want, what, made_of):
        if self.intensity.shape != want or self.optical_depth.shape != want:
            raise ValueError(f"the {what} have shapes {self.intensity.shape} and {self.optical_depth.shape}, {made_of} give {want}")


class SightlineEmission(_LineMaps):
    """What the lines of one view see.  intensity [W m^-2 sr^-1 (rad/s)^-1, spectral radiance per unit angular frequency] and
    optical_depth are (n_band,) + view.shape -- (n_band, nu, nv) for a pixel grid, (n_band, N) for Chords; column (the integral
    of ne dl [m^-2]), chord (the length inside the domain's box [m]; 0: the line misses it) and steps (samples marched) are
    view.shape.  Bands: wavelengths [m] always; photon_energy [eV] and, where the table has them, edges ((n_band, 2), eV) and
    band_radiance for a table (emission.TableEmission's)."""

    def __init__(self, view, intensity, optical_depth, column, chord, steps, wavelengths, photon_energy=None, edges=None):
        super().__init__(view, intensity, optical_depth, column, chord, steps)
        self.wavelengths = np.atleast_1d(np.asarray(wavelengths, np.float64))
        self.photon_energy = None if photon_energy is None else np.atleast_1d(np.asarray(photon_energy, np.float64))
        self.edges = None if edges is None else np.asarray(edges, np.float64).reshape(len(self.wavelengths), 2)
        self._expect((len(self.wavelengths),) + tuple(view.shape), "maps", "the bands and the view")

    @property
    def band_radiance(self):
        d_omega = self._d_omega("no band edges: band_radiance needs a table with the bands' widths")
        return self.intensity * d_omega.reshape((-1,) + (1,) * (self.intensity.ndim - 1))


def default_step(domain):
    """Half the smallest cell edge of the domain's grid as the device holds it (float32 coordinates)."""
    return 0.5 * min(float(np.min(np.diff(np.float64(np.float32(a))))) for a in (domain.x, domain.y, domain.z))


def _check_view(view):
    if not all(hasattr(view, name) for name in ("lines", "order", "backlight", "toward", "shape")):
        raise ValueError("view must be a sightlines.PinholeCamera, PointBacklighter or Chords")


def _along(domain, view, fields, entry, n_band, axis, step, max_steps, more=None, extra=(), **node):
    """What the entries share once the node is known: the defaults of step and max_steps, the view's lines and backlight in the
    order they go to the kernel in, entry(ne, Te, Z, ...) on the domain's fields, and its five arrays -- their lines along `axis`:
    -1 (bands first, the backlight (n_band, N)) or 0 (lines first, (N, n_band)) -- back in the view's order and shape.  more:
    emission._upload's further fields, which entry gets by keyword.  extra: further maps of entry's dict, placed after the five."""
    step = default_step(domain) if step is None else float(step)
    max_steps = 4 * (len(domain.x) + len(domain.y) + len(domain.z)) if max_steps is None else int(max_steps)
    o, d = view.lines()
    back = view.backlight(n_band)
    perm = view.order()
    if perm is not None:
        o, d = o[:, perm], d[:, perm]
        back = None if back is None else back[:, perm]
    if back is not None and axis == 0:
        back = np.ascontiguousarray(back.T)
    res = _upload(domain, fields, lambda ne, Te, Z, **f: entry(ne, Te, Z, o, d, toward=view.toward, step=step, max_steps=max_steps,
                                                              backlight=back, **f, **node), more)

    def place(a):  # kernel order -> the view's order and shape
        if perm is not None:
            out = np.empty_like(a)
            out[(perm,) if axis == 0 else (..., perm)] = a
            a = out
        return a.reshape(tuple(view.shape) + a.shape[1:] if axis == 0 else a.shape[:-1] + tuple(view.shape))

    return [place(res[k]) for k in ("intensity", "optical_depth", "column", "chord", "steps") + tuple(extra)]


def sightline_emission(domain, view, wavelengths=None, table=None, step=None, max_steps=None, fields=None):
    """What `view` (a PinholeCamera, a PointBacklighter or Chords) sees of a domain of either API generation: a SightlineEmission.
    Exactly one of wavelengths (up to 4 [m]: self_emission's NRL node) and table (an utils.eos_opacity.OpacityTable:
    table_emission's node, one band per band of the table).  step [m]: the target sample spacing along a line, by default half the
    smallest cell edge; max_steps: the most samples a line gets (a longer line is sampled more coarsely), by default
    4 * (nx + ny + nz).  The domain needs external_Te() and external_Z(); its fields are uploaded by self_emission's rules, and
    fields= (a fields.SourceFields of the domain) keeps them across calls.  A pixel grid's lines go to the kernel in 8x8 tiles in
    Morton order (tile_order) and the maps come back in pixel order.  Not modelled: a finite pinhole or source, the cos^4 and
    solid-angle factors of a film's exposure, refraction, the detector's response, a table's own ionisation; one GPU."""
    if (wavelengths is None) == (table is None):
        raise ValueError("exactly one of wavelengths (the NRL node) and table (an OpacityTable) must be given")
    _check_view(view)
    if table is None:
        lam, omegas = _omegas(wavelengths)
        kw, n_band = {"omegas": omegas}, len(lam)
    else:
        _check_table(table, "an OpacityTable")
        kw, n_band = {"table": table}, len(np.atleast_1d(table.photon_energy))
    maps = _along(domain, view, fields, engine.sightlines, n_band, -1, step, max_steps, **kw)
    if table is None:
        return SightlineEmission(view, *maps, lam)
    e_ph = np.atleast_1d(np.asarray(table.photon_energy, np.float64))
    return SightlineEmission(view, *maps, 2 * np.pi * engine.HBAR * c / (engine.E_CHARGE * e_ph), e_ph, getattr(table, "edges", None))


class SightlineSpectra(_LineMaps):
    """The spectrum every line of one view sees.  intensity [W m^-2 sr^-1 (rad/s)^-1, spectral radiance per unit angular frequency]
    and optical_depth are view.shape + (n_freq,) -- (nu, nv, n_freq) for a pixel grid, (N, n_freq) for Chords: a line's spectrum
    is contiguous; column, chord and steps are view.shape, as SightlineEmission's.  omega [rad/s], photon_energy [eV] and
    wavelengths [m] are (n_freq,); edges ((n_freq, 2), eV) where a table has them, and with them band_radiance."""

    def __init__(self, view, intensity, optical_depth, column, chord, steps, omega, edges=None):
        super().__init__(view, intensity, optical_depth, column, chord, steps)
        self.omega = np.atleast_1d(np.asarray(omega, np.float64))
        self.photon_energy = engine.HBAR * self.omega / engine.E_CHARGE
        self.wavelengths = 2 * np.pi * c / self.omega
        self.edges = None if edges is None else np.asarray(edges, np.float64).reshape(len(self.omega), 2)
        self._expect(tuple(view.shape) + (len(self.omega),), "spectra", "the view and the frequencies")

    def _widths(self):
        return self._d_omega("no band edges: band_radiance needs a table with the groups' widths")

    @property
    def band_radiance(self):
        """intensity times the group's width in angular frequency [W m^-2 sr^-1], as SightlineEmission's."""
        return self.intensity * self._widths()

    def signal(self, response=None):
        """The response-weighted integral of intensity over angular frequency per line [W m^-2 sr^-1], view.shape, on the host.
        response: an array (n_freq,), a callable of the photon energy [eV] (it gets photon_energy, (n_freq,)), or None: 1.  With
        group edges the sum over groups of I * d_omega * R; for point frequencies the trapezoid in omega over the frequencies
        in ascending order (one frequency: 0)."""
        if response is None:
            R = np.ones(len(self.omega))
        elif callable(response):
            R = np.asarray(response(self.photon_energy), np.float64)
        else:
            R = np.asarray(response, np.float64)
        if R.shape != self.omega.shape:
            raise ValueError(f"response must give {len(self.omega)} value(s), one per frequency, got shape {R.shape}")
        if self.edges is not None:
            return np.sum(self.intensity * (self._widths() * R), axis=-1)
        k = np.argsort(self.omega, kind="stable")
        y, w = (self.intensity * R)[..., k], self.omega[k]
        return np.sum(0.5 * (y[..., 1:] + y[..., :-1]) * np.diff(w), axis=-1)


def _spectrum_omegas(wavelengths, photon_energies):
    given = wavelengths if photon_energies is None else photon_energies
    a = np.atleast_1d(np.asarray(given, np.float64))
    name = "wavelengths" if photon_energies is None else "photon_energies"
    if a.ndim != 1 or not 1 <= len(a) <= engine._ffi.MAX_FREQS:
        raise ValueError(f"between 1 and {engine._ffi.MAX_FREQS} {name} go in one call, got shape {a.shape}")
    if not np.all(np.isfinite(a) & (a > 0)):
        raise ValueError(f"{name} must be finite and positive")
    return 2 * np.pi * c / a if photon_energies is None else a * engine.E_CHARGE / engine.HBAR


def sightline_spectra(domain, view, wavelengths=None, photon_energies=None, table=None, step=None, max_steps=None, fields=None):
    """The spectrum `view` (Chords, a PinholeCamera or a PointBacklighter) sees of a domain of either API generation along each of
    its lines: a SightlineSpectra.  sightline_emission at up to 16384 frequencies in one call, a GPU lane per frequency
    (engine.sightline_spectra -> sr_field_sightline_spectra); every value has the bits sightline_emission gives that line at that
    frequency.  Exactly one of wavelengths [m], photon_energies [eV] (point frequencies: self_emission's NRL node) and table (an
    utils.eos_opacity.SpectralOpacityTable: table_emission's node, one frequency per group, at its photon_energy).  The NRL
    coefficient holds only for hbar*omega <~ Te: a continuum spectrum above Te needs a table (a Kramers / Gaunt free-free node is not
    part of this).  view.backlight is per frequency (a number, (n_freq,) or (n_freq, N)).  step, max_steps, fields=, the tile order
    of a pixel grid's lines and their placement back in pixel order are sightline_emission's.  Measured against the loop of
    4-band sightline_emission calls that gives the same numbers (profiles/sightline_spectra_rate.txt, 256^3): 16 chords x 2048
    frequencies 0.42 ms of kernel against 1.4 s, a 256 x 256 view x 64 frequencies 2.5 (NRL) to 3.9 (table) times faster.
    Not modelled: a finite pinhole or source size, the cos^4 and solid-angle factors that turn radiance into film exposure,
    refraction of the light, the detector's response beyond signal(), a table's own ionisation, group-integrated Planck
    functions; one GPU.  Spectral lines with their Doppler shifts and widths are sightline_lines."""
    if sum(a is not None for a in (wavelengths, photon_energies, table)) != 1:
        raise ValueError("exactly one of wavelengths, photon_energies (the NRL node) and table (a SpectralOpacityTable) must be given")
    _check_view(view)
    if table is None:
        omega = _spectrum_omegas(wavelengths, photon_energies)
        kw, edges = {"omegas": omega}, None
    else:
        _check_table(table, "a SpectralOpacityTable")
        omega = np.atleast_1d(np.asarray(table.photon_energy, np.float64)) * engine.E_CHARGE / engine.HBAR
        kw, edges = {"table": table}, getattr(table, "edges", None)
    maps = _along(domain, view, fields, engine.sightline_spectra, len(omega), 0, step, max_steps, **kw)
    return SightlineSpectra(view, *maps, omega, edges)


M_P = 1.67262192369e-27  # kg


class LineSpectra(SightlineSpectra):
    """A SightlineSpectra of spectral lines: `lines` is the utils.eos_opacity.LineTable they came from; signal() works unchanged."""

    def __init__(self, view, intensity, optical_depth, column, chord, steps, omega, lines):
        super().__init__(view, intensity, optical_depth, column, chord, steps, omega)
        self.lines = lines

    def moments(self, window):
        """What a spectrometer infers from each line, on the host, per chord and per line: a dict of "radiance", "velocity" and
        "Ti", each view.shape + (n_line,).  window: the half-width [rad/s] (a number, or one per line) of the frequency window
        |omega - omega0| <= window the moments are taken over, by the trapezoid over the frequencies in ascending order:
            radiance = int I d omega  [W m^-2 sr^-1]
            velocity = c * (int I (omega - omega0) d omega / radiance) / omega0  [m/s]: the line-of-sight velocity of the centroid,
                       positive (a blue shift) where the plasma moves towards the observer
            Ti       = A m_p c^2 var / (e omega0^2)  [eV], var the second central moment: the ion temperature of a Gaussian of
                       that variance (its 1/e half-width is omega0 sqrt(2 e Ti / (A m_p)) / c)
        Nothing is subtracted: a continuum or a neighbouring line inside the window counts.  A window with fewer than two
        frequencies or no radiance gives NaN.  Ti assumes a Gaussian line: a Voigt line (sightline_voigt) has no variance, and
        its "Ti" grows with the window without bound; use fwhm() there."""
        w0 = self.lines.omega0
        win = np.broadcast_to(np.asarray(window, np.float64), w0.shape)
        if not np.all(np.isfinite(win) & (win > 0)):
            raise ValueError(f"window must be finite and positive (a number or one per line), got {window!r}")
        k = np.argsort(self.omega, kind="stable")
        w, y = self.omega[k], self.intensity[..., k]
        out = {name: np.full(tuple(self.view.shape) + w0.shape, np.nan) for name in ("radiance", "velocity", "Ti")}

        def integral(f, x):
            return np.sum(0.5 * (f[..., 1:] + f[..., :-1]) * np.diff(x), axis=-1)

        for l in range(len(w0)):
            sel = np.abs(w - w0[l]) <= win[l]
            if np.count_nonzero(sel) < 2:
                continue
            x, f = w[sel] - w0[l], y[..., sel]
            with np.errstate(all="ignore"):
                m0 = integral(f, x)
                m1 = integral(f * x, x) / m0
                var = integral(f * (x - m1[..., None]) ** 2, x) / m0
                ok = m0 > 0
                out["radiance"][..., l] = np.where(ok, m0, np.nan)
                out["velocity"][..., l] = np.where(ok, c * m1 / w0[l], np.nan)
                out["Ti"][..., l] = np.where(ok, self.lines.mass_number[l] * M_P * c ** 2 * var / (engine.E_CHARGE * w0[l] ** 2), np.nan)
        return out

    def fwhm(self, window):
        """The full width at half maximum [rad/s] of each line, on the host, per chord and per line: view.shape + (n_line,).
        window: as moments()'.  Inside |omega - omega0| <= window, over the frequencies in ascending order, the greatest
        intensity is the maximum; on either side of it the nearest pair of neighbouring frequencies between which the intensity
        falls through half of it gives a crossing by linear interpolation, and the width is the distance of the two crossings.
        NaN where either side has no crossing (the window ends above half maximum, or holds fewer than three frequencies).
        Nothing is subtracted: a continuum or a neighbour inside the window counts, and a thick line's width is its saturated one."""
        w0 = self.lines.omega0
        win = np.broadcast_to(np.asarray(window, np.float64), w0.shape)
        if not np.all(np.isfinite(win) & (win > 0)):
            raise ValueError(f"window must be finite and positive (a number or one per line), got {window!r}")
        k = np.argsort(self.omega, kind="stable")
        w, y = self.omega[k], self.intensity[..., k]
        out = np.full((int(np.prod(self.view.shape, dtype=np.int64)), len(w0)), np.nan)
        for l in range(len(w0)):
            sel = np.abs(w - w0[l]) <= win[l]
            if np.count_nonzero(sel) < 3:
                continue
            x, f = w[sel], y[..., sel].reshape(len(out), -1)
            for r, g in enumerate(f):
                if not np.all(np.isfinite(g)) or not g.max() > 0:
                    continue
                top, half = int(np.argmax(g)), 0.5 * g.max()
                lo, hi = np.nonzero(g[:top] <= half)[0], np.nonzero(g[top + 1:] <= half)[0]
                if len(lo) == 0 or len(hi) == 0:
                    continue
                a, b = lo[-1], top + 1 + hi[0]
                left = x[a] + (x[a + 1] - x[a]) * (half - g[a]) / (g[a + 1] - g[a])
                right = x[b - 1] + (x[b] - x[b - 1]) * (g[b - 1] - half) / (g[b - 1] - g[b])
                out[r, l] = right - left
        return out.reshape(tuple(self.view.shape) + w0.shape)


def sightline_lines(domain, view, lines, wavelengths=None, photon_energies=None, continuum=False, step=None, max_steps=None,
                    fields=None):
    """The line spectrum `view` (Chords, a PinholeCamera or a PointBacklighter) sees of a domain of either API generation along
    each of its chords: a LineSpectra (engine.sightline_lines -> sr_field_sightline_lines; include/synthray.h states the rule).
    lines: an utils.eos_opacity.LineTable of 1 to 32 lines; each is a Gaussian whose centre moves with the flow's component along
    the direction the light travels (the domain's V, external_V; without it no shift) and whose width is the thermal one of the
    ion temperature (Ti, external_Ti; without it Ti = Te), sample by sample, with the table's emission and absorption at the
    sample's (Te, ne / Z).  Exactly one of wavelengths [m] and photon_energies [eV]: up to 16384 frequencies, in any order (a
    sorted list lets the kernel skip a line for whole wavefronts).  continuum=True puts the lines on sightline_spectra's NRL
    continuum, with its caveat (hbar*omega <~ Te).  view.backlight, step, max_steps, the tile order of a pixel grid and fields=
    are sightline_spectra's; Ti and V go up under the names thomson.spectra uses, so one fields.SourceFields serves both.
    Not modelled: Lorentzian, Stark and Voigt wings, Zeeman splitting, line blending through the cutoff at exp(-40), partial
    redistribution, refraction, the instrument function (convolve on the host, as thomson.instrument_convolve does); one GPU."""
    if getattr(lines, "lorentz_width", None) is not None:
        raise ValueError("lines is a VoigtLineTable: its Lorentzian widths need sightline_voigt (sightline_lines draws Gaussian lines)")
    return _line_spectra(domain, view, lines, wavelengths, photon_energies, step, max_steps, fields, engine.sightline_lines,
                         continuum=continuum)


def _line_spectra(domain, view, lines, wavelengths, photon_energies, step, max_steps, fields, call, reference=None, **opts):
    """What sightline_lines, sightline_voigt, sightline_zeeman and sightline_stokes share: the checks, the frequencies, the domain's Ti and V, and
    `call` (the engine's entry, with `opts`) along the view.  reference (sightline_zeeman alone: (3, N) in the view's order, already
    resolved): the domain's B goes up as well, the call is engine.sightline_zeeman's or engine.sightline_stokes', and a
    StokesSpectra comes back."""
    if (wavelengths is None) == (photon_energies is None):
        raise ValueError("exactly one of wavelengths [m] and photon_energies [eV] must be given")
    _check_view(view)
    for name in ("temperatures", "ion_densities", "emissivity", "omega0", "mass_number", "absorption"):
        if not hasattr(lines, name):
            raise ValueError(f"lines must be a LineTable (utils.eos_opacity): it has no {name}")
    omega = _spectrum_omegas(wavelengths, photon_energies)
    shape = (len(domain.x), len(domain.y), len(domain.z))
    Ti, V = getattr(domain, "Ti", None), getattr(domain, "V", None)
    more = {"Ti": None if Ti is None else (np.asarray(Ti) if np.ndim(Ti) == 3 else np.full(shape, float(Ti))),
            "V": None if V is None else np.asarray(V)}
    if more["V"] is not None and more["V"].shape != shape + (3,):
        raise ValueError(f"V has shape {more['V'].shape}, the domain needs {shape + (3,)}")

    if reference is not None:
        B = getattr(domain, "B", None)
        if B is None:
            raise ValueError("the domain holds no magnetic field: call external_B() (without B the lines are sightline_voigt's)")
        more["B"] = np.asarray(B)
        if more["B"].shape != shape + (3,):
            raise ValueError(f"B has shape {more['B'].shape}, the domain needs {shape + (3,)}")
        perm = view.order()
        ref = reference if perm is None else reference[:, perm]

        def stokes_entry(ne, Te, Z, o, d, Ti=None, V=None, B=None, **kw):
            return call(ne, Te, Ti, Z, V, B, o, d, ref, lines=lines, omegas=omega, **opts, **kw)

        maps = _along(domain, view, fields, stokes_entry, len(omega), 0, step, max_steps, more, extra=("Q", "U", "V"))
        return StokesSpectra(view, *maps[:5], omega, lines, *maps[5:], reference)

    def entry(ne, Te, Z, o, d, Ti=None, V=None, **kw):
        return call(ne, Te, Ti, Z, V, o, d, lines=lines, omegas=omega, **opts, **kw)

    maps = _along(domain, view, fields, entry, len(omega), 0, step, max_steps, more)
    return LineSpectra(view, *maps, omega, lines)


def sightline_voigt(domain, view, lines, wavelengths=None, photon_energies=None, continuum=False, wing=None, step=None, max_steps=None,
                    fields=None):
    """sightline_lines with Voigt profiles: a LineSpectra (engine.sightline_voigt -> sr_field_sightline_voigt; include/synthray.h
    states the rule and the algorithm of the Voigt function).  lines: an utils.eos_opacity.VoigtLineTable, whose lorentz_width is
    each line's Lorentzian half-width at half maximum [rad/s] on the lattice -- Stark and natural broadening; a line's shape at a
    sample is the Voigt function of that and the thermal width of Ti, accurate relative to itself at any distance from the centre,
    so the far wings of a thick line are right.  wing: a term further than `wing` thermal 1/e widths from its line's centre is
    dropped; None: never (a finite wing lets the kernel skip a line for whole wavefronts of a sorted frequency list, at the price
    of a step of the dropped wing's height in the spectrum).  LineSpectra.fwhm() reads each line's width, from which
    VoigtLineTable.power_law's density follows; moments()' Ti does not apply to such lines.  Everything else is sightline_lines'.
    Not modelled: Zeeman splitting, asymmetric and shifted Stark profiles (a constant Stark shift can go into the line's rest
    position), ion dynamics, blending through wing, partial redistribution, refraction, the instrument function; one GPU."""
    if getattr(lines, "lorentz_width", None) is None:
        raise ValueError("lines must be a VoigtLineTable (utils.eos_opacity): it has no lorentz_width")
    return _line_spectra(domain, view, lines, wavelengths, photon_energies, step, max_steps, fields, engine.sightline_voigt,
                         continuum=continuum, wing=np.inf if wing is None else wing)


class StokesSpectra(LineSpectra):
    """A LineSpectra with polarisation: intensity (Stokes I), Q, U, V and optical_depth, each view.shape + (n_freq,), in the frame
    of each chord -- with n^ the direction the light travels, e1 the part of `reference` ((3, N), the view's order) across n^,
    normalised, and e2 = n^ x e1: Q > 0 is linear polarisation along e1, U > 0 along the bisector of e1 and e2, V > 0 the
    helicity of a q = +1 Zeeman component emitted along +B.  moments(), fwhm() and signal() work unchanged on intensity."""

    def __init__(self, view, intensity, optical_depth, column, chord, steps, omega, lines, Q, U, V, reference=None):
        super().__init__(view, intensity, optical_depth, column, chord, steps, omega, lines)
        self.Q, self.U, self.V = (np.asarray(a, np.float64) for a in (Q, U, V))
        for name in ("Q", "U", "V"):
            if getattr(self, name).shape != self.intensity.shape:
                raise ValueError(f"{name} has shape {getattr(self, name).shape}, intensity {self.intensity.shape}")
        self.reference = reference

    def analysed(self, angle=None, circular=None):
        """The spectral radiance behind an ideal analyser, the shape of intensity.  angle=psi [rad]: a linear polariser whose
        axis is turned by psi from e1 towards e2, 0.5 (I + Q cos 2 psi + U sin 2 psi); circular=+1 or -1: a circular analyser
        that passes positive or negative helicity, 0.5 (I +- V).  Exactly one of the two."""
        if (angle is None) == (circular is None):
            raise ValueError("exactly one of angle [rad] and circular (+1 or -1) must be given")
        if circular is not None:
            if circular not in (1, -1):
                raise ValueError(f"circular must be +1 or -1, got {circular!r}")
            return 0.5 * (self.intensity + circular * self.V)
        psi = float(angle)
        if not np.isfinite(psi):
            raise ValueError(f"angle must be finite, got {angle!r}")
        return 0.5 * (self.intensity + self.Q * np.cos(2 * psi) + self.U * np.sin(2 * psi))

    def b_parallel(self, window, g_eff=None):
        """The centre-of-gravity estimate of the field along the light [T], per chord and per line: view.shape + (n_line,), on the
        host.  Inside |omega - omega0| <= window (moments()' window) the centroids of the two circular analysers' spectra,
        0.5 (I + V) and 0.5 (I - V), are taken by the trapezoid over the frequencies in ascending order; their difference divided
        by 2 g_eff kL, kL = e / (2 m_e), is the emission-weighted B . n^ a spectrometer with a circular analyser reports (positive:
        B points along the light's travel).  g_eff: a number or one per line; None: lines.g_eff.  Exact for thin lines of any
        splitting; self-absorption and a continuum inside the window bias it.  NaN where the window holds fewer than two
        frequencies or either spectrum has no radiance."""
        w0 = self.lines.omega0
        win = np.broadcast_to(np.asarray(window, np.float64), w0.shape)
        if not np.all(np.isfinite(win) & (win > 0)):
            raise ValueError(f"window must be finite and positive (a number or one per line), got {window!r}")
        g = np.broadcast_to(np.asarray(self.lines.g_eff if g_eff is None else g_eff, np.float64), w0.shape)
        if not np.all(np.isfinite(g) & (g != 0)):
            raise ValueError(f"g_eff must be finite and not zero (a number or one per line), got {g.tolist()}")
        k = np.argsort(self.omega, kind="stable")
        w = self.omega[k]
        plus, minus = (0.5 * (self.intensity + self.V))[..., k], (0.5 * (self.intensity - self.V))[..., k]
        out = np.full(tuple(self.view.shape) + w0.shape, np.nan)
        with np.errstate(all="ignore"):
            for l in range(len(w0)):
                sel = np.abs(w - w0[l]) <= win[l]
                if np.count_nonzero(sel) < 2:
                    continue
                x, dx = w[sel] - w0[l], np.diff(w[sel])
                cen = []
                for y in (plus[..., sel], minus[..., sel]):
                    m0 = np.sum(0.5 * (y[..., 1:] + y[..., :-1]) * dx, axis=-1)
                    yx = y * x
                    m1 = np.sum(0.5 * (yx[..., 1:] + yx[..., :-1]) * dx, axis=-1)
                    cen.append(np.where(m0 > 0, m1 / m0, np.nan))
                out[..., l] = (cen[0] - cen[1]) / (2.0 * g[l] * engine.LARMOR)
        return out

    def polarisation_angle(self):
        """The angle of the plane of linear polarisation from e1 towards e2 [rad], in (-pi/2, pi/2]: 0.5 arctan2(U, Q), the shape
        of intensity (0 where Q = U = 0)."""
        return 0.5 * np.arctan2(self.U, self.Q)

    def degree(self):
        """The degree of polarisation sqrt(Q^2 + U^2 + V^2) / I, the shape of intensity; NaN where there is no radiance."""
        with np.errstate(all="ignore"):
            p = np.sqrt(self.Q * self.Q + self.U * self.U + self.V * self.V)
            return np.where(self.intensity > 0, p / self.intensity, np.nan)


def default_reference(view):
    """The reference direction of every chord of `view`, (3, N) in the view's order: a pixel view's up (its frame's y), for Chords
    the lab axis least aligned with each chord (the first of them where they tie)."""
    o, d = view.lines()
    if hasattr(view, "y") and np.shape(view.y) == (3,):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(view.y, np.float64)[:, None], d.shape))
    ref = np.zeros(d.shape)
    ref[np.argmin(np.abs(d), axis=0), np.arange(d.shape[1])] = 1.0
    return ref


def _resolved_reference(view, reference):
    """reference as (3, N) in the view's order: (3,) for all chords, (3, N), or None: default_reference(view)."""
    n = int(np.prod(view.shape))
    if reference is None:
        return default_reference(view)
    ref = np.asarray(reference, np.float64)
    if ref.shape == (3,):
        ref = np.broadcast_to(ref[:, None], (3, n))
    if ref.shape != (3, n):
        raise ValueError(f"reference must have shape (3,) or (3, {n}), got {ref.shape}")
    return np.ascontiguousarray(ref)


def sightline_zeeman(domain, view, lines, wavelengths=None, photon_energies=None, continuum=False, wing=None, step=None, max_steps=None,
                     fields=None, reference=None):
    """sightline_voigt in the domain's magnetic field (external_B): a StokesSpectra (engine.sightline_zeeman ->
    sr_field_sightline_zeeman; include/synthray.h states the rule and the sign conventions).  lines: an
    utils.eos_opacity.ZeemanLineTable -- a VoigtLineTable (or, without widths, a LineTable: Gaussian components) with a Zeeman
    pattern per line (normal_triplet(), from_lande()); at every sample each line is split by B into its pi and sigma components,
    shifted by g e |B| / (2 m_e), weighted and polarised by the angle between B and the chord, and I, Q, U, V are marched with the
    line's self-absorption acting equally on all four.  reference: the direction Q is measured from -- (3,), or (3, N) in the
    view's order; None: default_reference(view), a pixel view's up, for Chords the lab axis least aligned with each chord; it must
    not be parallel to its chord.  StokesSpectra.analysed() gives what an analyser passes, b_parallel() the field a
    circular-analyser spectrometer would infer.  rotated() domains work unchanged (B is carried as R^T B(R q)).  Everything else
    is sightline_voigt's.  Not modelled: dichroism and magneto-optical (anomalous-dispersion) rotation in the absorption matrix,
    Faraday rotation of the continuum, the Paschen-Back regime, hyperfine structure, and what sightline_voigt does not model; one
    GPU."""
    if getattr(lines, "patterns", None) is None:
        raise ValueError("lines must be a ZeemanLineTable (utils.eos_opacity): it has no patterns")
    _check_view(view)
    ref = _resolved_reference(view, reference)
    return _line_spectra(domain, view, lines, wavelengths, photon_energies, step, max_steps, fields, engine.sightline_zeeman,
                         reference=ref, continuum=continuum, wing=np.inf if wing is None else wing)


def sightline_stokes(domain, view, lines, wavelengths=None, photon_energies=None, continuum=False, wing=None, step=None, max_steps=None,
                     fields=None, reference=None, polarisation=None, faraday=False):
    """sightline_zeeman with the full polarised transfer equation: a StokesSpectra (engine.sightline_stokes ->
    sr_field_sightline_stokes; include/synthray.h states the rule, the algorithm and the sign conventions).  The table's absorption
    acts through the 4 x 4 absorption matrix: it is dichroic -- an unpolarised backlight comes out of a Zeeman-split absorption
    line with the opposite polarisation of the line's emission, and a thick emission line depolarises towards its source function
    -- and the plane of polarisation turns inside the lines (magneto-optical rotation, from the dispersion profile) and, with
    faraday=True, in the continuum: by engine.FARADAY * ne * B.n^ / omega^2 per metre, from e1 towards e2 for B along the light's
    travel.  polarisation: (q, u, v), the Stokes parameters of view.backlight as fractions of its intensity, q^2 + u^2 + v^2 <= 1;
    None: unpolarised.  StokesSpectra.polarisation_angle() and degree() read the result; b_parallel() works on absorption spectra
    too.  Everything else is sightline_zeeman's; a table without absorption, faraday=False and polarisation=None give its bits.
    Not modelled: the Paschen-Back regime, hyperfine structure, cyclotron dichroism of the continuum, scattering polarisation, the
    Hanle effect, and what sightline_voigt does not model; one GPU."""
    if getattr(lines, "patterns", None) is None:
        raise ValueError("lines must be a ZeemanLineTable (utils.eos_opacity): it has no patterns")
    _check_view(view)
    ref = _resolved_reference(view, reference)
    return _line_spectra(domain, view, lines, wavelengths, photon_energies, step, max_steps, fields, engine.sightline_stokes,
                         reference=ref, continuum=continuum, wing=np.inf if wing is None else wing, polarisation=polarisation,
                         faraday=faraday)
