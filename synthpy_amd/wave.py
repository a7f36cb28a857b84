"""Wave-optics beam propagation through a domain: a paraxial split-step Fourier march of a complex field (no counterpart in
the reference's sources; its authors check their tracer against a CPU beam-propagation library).

    src = wave.Source.gaussian(shape=(1024, 1024), pitch=10e-6, wavelength=532e-9, w0=1.5e-3)
    out = domain.wave_propagate(src, absorber=0.1)               # or wave.propagate(domain, src, ...)
    out.intensity(), out.phase(), out.power
    out.image("dark_field", f=400.0, R=25.0, stop_R=1.0)         # the reference's mm arguments
    out.interferogram(n_fringes=10, deg=20)

The field lives on a uniform lateral frame of its own (pixel (i, j) at (u0 + i du, v0 + j dv) on the two axes lateral to the
domain's probing_direction, in x < y < z order) and is carried through the domain's node planes: per cell a thin screen with
the phase k0 h <n - 1> and, with absorption, the amplitude exp(-tau/2) of the cell, and between the screens a Fresnel step
(engine.wave -> sr_field_wave; include/synthray.h states the rule).  The field varies as exp(+i(kz - wt)) and the carrier is
dropped, so plasma retards the phase.  Limits: paraxial (angles well below 1 rad: the transfer function is the Fresnel one, not
the angular spectrum's), scalar (no polarisation, no Faraday rotation of the field), the frame is periodic -- leave a guard band
around the beam or absorb at the edges (edge_absorber) -- and nothing is reflected where ne approaches critical: a pixel whose
cell is over-critical is set to 0.  The detector is an ideal one-to-one relay with a mask in the Fourier plane (engine.wave_image).
"""
from __future__ import annotations

import numpy as np

from . import engine
from .fields import staged

_LATERAL = {0: ("y", "z"), 1: ("x", "z"), 2: ("x", "y")}


class Source:
    """A complex field U (mu, mv) on the frame (u0, du, v0, dv) [m] at the vacuum wavelength [m].  Built from an array, or by
    plane() / gaussian(); the frame is centred on `centre` unless u0, v0 are given."""

    def __init__(self, U, pitch, wavelength, centre=(0.0, 0.0), origin=None):
        self.U = np.ascontiguousarray(U, dtype=np.complex128)
        if self.U.ndim != 2 or min(self.U.shape) < 2:
            raise ValueError(f"U must be a complex array (mu, mv) with mu, mv >= 2, got shape {self.U.shape}")
        self.wavelength = float(wavelength)
        if not (np.isfinite(self.wavelength) and self.wavelength > 0):
            raise ValueError(f"wavelength must be finite and positive, got {wavelength!r}")
        du, dv = (float(pitch), float(pitch)) if np.ndim(pitch) == 0 else (float(pitch[0]), float(pitch[1]))
        if not (np.isfinite(du) and np.isfinite(dv) and du > 0 and dv > 0):
            raise ValueError(f"pitch must be finite and positive, got {pitch!r}")
        self.du, self.dv = du, dv
        self.u0, self.v0 = self._origin(self.U.shape, du, dv, centre, origin)

    @staticmethod
    def _origin(shape, du, dv, centre, origin):
        if origin is not None:
            return float(origin[0]), float(origin[1])
        return float(centre[0]) - 0.5 * (shape[0] - 1) * du, float(centre[1]) - 0.5 * (shape[1] - 1) * dv

    @property
    def frame(self):
        return (self.u0, self.du, self.v0, self.dv)

    @property
    def u(self):
        return self.u0 + np.arange(self.U.shape[0]) * self.du

    @property
    def v(self):
        return self.v0 + np.arange(self.U.shape[1]) * self.dv

    @classmethod
    def plane(cls, shape, pitch, wavelength, amplitude=1.0, centre=(0.0, 0.0), origin=None):
        """A plane wave along the axis."""
        return cls(np.full(shape, amplitude, np.complex128), pitch, wavelength, centre, origin)

    @classmethod
    def gaussian(cls, shape, pitch, wavelength, w0, beam_centre=(0.0, 0.0), tilt=(0.0, 0.0), amplitude=1.0, centre=(0.0, 0.0),
                 origin=None):
        """A Gaussian beam at its waist: amplitude * exp(-r^2 / w0^2) about beam_centre [m], tilted by the angles tilt [rad]
        (a linear phase k0 (tilt_u u + tilt_v v))."""
        du, dv = (float(pitch), float(pitch)) if np.ndim(pitch) == 0 else (float(pitch[0]), float(pitch[1]))
        u0, v0 = cls._origin(shape, du, dv, centre, origin)
        u, v = u0 + np.arange(shape[0]) * du, v0 + np.arange(shape[1]) * dv
        du_, dv_ = u[:, None] - float(beam_centre[0]), v[None, :] - float(beam_centre[1])
        k0 = 2 * np.pi / float(wavelength)
        U = amplitude * np.exp(-(du_ * du_ + dv_ * dv_) / float(w0) ** 2) * np.exp(1j * k0 * (float(tilt[0]) * du_ + float(tilt[1]) * dv_))
        return cls(U, pitch, wavelength, centre, origin)


def edge_absorber(mu, mv, frac=0.1):
    """The windows (wu (mu), wv (mv)) of an edge absorber: Tukey windows (simulator.fresnel_integral.tukey) whose cosine edges
    take the fraction `frac` of the frame on each side.  They multiply the field with every screen, so what reaches the edge of
    the periodic frame is damped instead of coming back in on the other side."""
    from .simulator.fresnel_integral import tukey

    frac = float(frac)
    if not 0.0 <= frac <= 0.5:
        raise ValueError(f"frac must lie in 0 .. 0.5, got {frac!r}")
    return tukey(int(mu), 2.0 * frac), tukey(int(mv), 2.0 * frac)


class WaveField:
    """A field on its frame: U (mu, mv) complex128, the pixel coordinates u, v [m], the names of the lateral axes, the wavelength,
    power (sum |U|^2 after every screen of the march, or None), kernel_ms (the march's HIP-event time) and, from a march with
    time_parts, parts_ms = (hipFFT ms, own kernels ms)."""

    def __init__(self, U, frame, wavelength, axes=("u", "v"), power=None, kernel_ms=0.0, parts_ms=None):
        self.U = U
        self.frame = tuple(float(a) for a in frame)
        self.wavelength = float(wavelength)
        self.axes = tuple(axes)
        self.power = power
        self.kernel_ms = float(kernel_ms)
        self.parts_ms = parts_ms

    @property
    def u(self):
        return self.frame[0] + np.arange(self.U.shape[0]) * self.frame[1]

    @property
    def v(self):
        return self.frame[2] + np.arange(self.U.shape[1]) * self.frame[3]

    def intensity(self):
        return self.U.real ** 2 + self.U.imag ** 2

    def phase(self):
        return np.angle(self.U)

    def image(self, kind="shadow", f=400.0, R=25.0, stop_R=1.0, defocus=0.0, knife=("u", 0.0, 1)):
        """The intensity on the detector of an ideal one-to-one relay (engine.wave_image), with the reference's arguments in mm:
        f the focal length of the relay's lenses, R their radius -- a ray of angle a passes a lens one focal length away at f a,
        which is its place in the Fourier plane, so the lens is an aperture of radius R there --, stop_R the schlieren stop's
        radius, defocus the shift of the object plane (focal_plane).  kind: "shadow" (aperture R), "dark_field" (aperture R and a
        stop of radius stop_R), "light_field" (an aperture of radius stop_R), "knife" (aperture R and a knife edge, knife =
        (axis "u" | "v", offset [mm], direction: > 0 blocks above the offset, < 0 below)).  Returns (mu, mv) float64."""
        mm = 1e-3
        kw = {}
        if kind == "shadow":
            kw["aperture"] = R * mm
        elif kind == "dark_field":
            kw["aperture"], kw["stop"] = R * mm, stop_R * mm
        elif kind == "light_field":
            kw["aperture"] = min(R, stop_R) * mm
        elif kind == "knife":
            axis = {"u": 0, "v": 1, 0: 0, 1: 1}.get(knife[0])
            if axis is None:
                raise ValueError(f"the knife's axis must be 'u' or 'v', got {knife[0]!r}")
            kw["aperture"], kw["knife"] = R * mm, (axis, float(knife[1]) * mm, float(knife[2]))
        else:
            raise ValueError(f"kind must be 'shadow', 'dark_field', 'light_field' or 'knife', got {kind!r}")
        out, _ = engine.wave_image(self.U, self.frame[1], self.frame[3], self.wavelength, f=f * mm, defocus=defocus * mm, **kw)
        return out.real ** 2 + out.imag ** 2

    def interferogram(self, n_fringes=10, deg=20):
        """|U + reference|^2 with the tilted reference beam of Interferometry.interfere_ref_beam (diagnostics.py:559-581; formed
        on the host): exp(i (2 n_fringes / 3) (xw u + yw v)) with u, v in mm, yw = arctan(deg in rad) -- deg >= 45 is taken as
        -|deg - 90| -- and xw = sqrt(1 - yw^2)."""
        if deg >= 45:
            deg = -abs(deg - 90)
        yw = np.arctan(deg * np.pi / 180)
        xw = np.sqrt(1 - yw ** 2)
        ref = np.exp(2 * n_fringes / 3 * 1.0j * (xw * (self.u * 1e3)[:, None] + yw * (self.v * 1e3)[None, :]))
        tot = self.U + ref
        return tot.real ** 2 + tot.imag ** 2


def propagate(domain, source, toward="+", absorb=False, absorber=None, fields=None, time_parts=False):
    """March `source` (a Source) through `domain` (a ScalarDomain of either API generation) along its probing_direction: a
    WaveField on the last node plane of the march.  toward "+": from the first node plane to the last (the way the rays
    travel), "-": the reverse.  absorb: inverse-bremsstrahlung absorption from the domain's Te (external_Te) and Z (external_Z; an
    array or a number).  absorber: None, a fraction (edge_absorber(mu, mv, frac)) or the windows (wu, wv) themselves.  fields: a
    fields.SourceFields of the domain whose uploads are reused across calls."""
    from .emission import _toward

    if not isinstance(source, Source):
        raise ValueError("source must be a wave.Source")
    axis = engine.axis_index(domain.probing_direction)
    sign = _toward(toward)
    ne = getattr(domain, "ne", None)
    if ne is None:
        raise ValueError("the domain holds no electron density: pass ne_type= or call external_ne()")
    named = {"ne": np.asarray(ne)}
    Z_value = 0.0
    if absorb:
        Te, Z = getattr(domain, "Te", None), getattr(domain, "Z", None)
        if Te is None or Z is None:
            raise ValueError("absorb=True needs external_Te() and external_Z()")
        named["Te"] = np.asarray(Te) if np.ndim(Te) == 3 else np.full(named["ne"].shape, float(Te))
        if np.ndim(Z) == 3:
            named["Z"] = np.asarray(Z)
        else:
            Z_value = float(Z)
    mu, mv = source.U.shape
    if absorber is not None and np.ndim(absorber) == 0:
        absorber = edge_absorber(mu, mv, absorber)
    with staged(domain, fields) as src:
        f = src.get_all(named)  # the kernel reads every field in one dtype
        res = engine.wave(f["ne"], f.get("Te"), f.get("Z", Z_value), source.U, source.frame, source.wavelength, axis, sign, absorber,
                          time_parts=time_parts)
        kernel_ms = f["ne"].last_kernel_ms
    return WaveField(res[0], source.frame, source.wavelength, _LATERAL[axis], res[1], kernel_ms, res[2] if time_parts else None)
