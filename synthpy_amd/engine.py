"""Thin object layer over the C ABI (include/synthray.h): device volumes, ray bundles,
detector images and the host-buffer entry points.  Every compute call goes to the HIP
library; nothing here does the path's arithmetic in NumPy.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import weakref
from dataclasses import dataclass

import numpy as np

from . import _ffi
from ._ffi import check, f32, f64, lib, ptr

c = 299792458.0  # scipy.constants.c, as the reference uses (full_solver.py:93)

# optic op codes (include/synthray.h)
OP_DIST, OP_LENS, OP_CIRC_AP, OP_CIRC_STOP, OP_RECT_AP, OP_KNIFE, OP_SCALE, OP_PHASE = range(8)
ROWS_LEGACY, ROWS_JAX = 0, 1
IMG_COUNTS, IMG_COMPLEX, IMG_INTENSITY = 0, 1, 2
VOL_PHASE = 1

_AXES = {"x": 0, "y": 1, "z": 2}


def axis_index(probing_direction) -> int:
    """'x' | 'y' | 'z' -> 0 | 1 | 2.  The reference prints and carries on for anything else
    (propagator.py:260, beam.py:288); the engine raises."""
    if isinstance(probing_direction, str) and probing_direction in _AXES:
        return _AXES[probing_direction]
    raise ValueError(f"probing_direction must be 'x', 'y' or 'z', got {probing_direction!r}")


def device_count() -> int:
    _ffi.gpu_touched = True  # the library's first call opens the device: from here on this process must not fork
    n = lib.sr_device_count()
    if n < 0:
        check(n)
    return n


def init(device: int = 0) -> None:
    check(lib.sr_init(int(device)))


def init_rank(local_rank: int = 0, local_world: int = 1, *, device=None, shared=False) -> int:
    """Open this rank's GPU: the one way in for every multi-process driver (bench.py, run_trace, the tests' workers).
    device None: GPU `local_rank`; a job with more local ranks than visible GPUs fails HERE, loudly, instead of putting
    two ranks on device 0 (`shared=True` says that is wanted: the one-GPU rehearsal).  Ranks that start in the same
    instant are handled in the library (sr_device_count: bounded retry of the device open before the first HIP call)."""
    n = device_count()
    if n < 1:
        check(lib.sr_init(0))  # raises with the runtime's reason
    if device is None:
        if shared:
            device = 0
        elif local_world > n:
            raise _ffi.SynthrayError(f"{local_world} local ranks but {n} visible GPU(s): one process per GPU "
                                     "(HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES hide devices)")
        else:
            device = local_rank
    device = int(device)
    if not 0 <= device < n:
        raise ValueError(f"device {device} outside 0..{n - 1}")
    init(device)
    return device


def device_memory():
    """(free, total) bytes of HBM on the selected device."""
    f, t = C.c_int64(0), C.c_int64(0)
    check(lib.sr_device_memory(C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


def compute_units() -> int:
    """Compute units of the selected device (256 on an MI355X), whatever grid_cus() has in force."""
    now, dev = C.c_int(0), C.c_int(0)
    check(lib.sr_grid_cus(-1, C.byref(now)))
    check(lib.sr_grid_cus(0, C.byref(dev)))
    if now.value != dev.value:
        check(lib.sr_grid_cus(now.value, None))
    return int(dev.value)


def grid_stats():
    """(launches sized by a grid cap since the last reset, those of them that got fewer blocks than they wanted): sr_grid_stats."""
    out = (C.c_int64 * 2)()
    check(lib.sr_grid_stats(out, 0))
    return int(out[0]), int(out[1])


@contextlib.contextmanager
def grid_cus(n: int):
    """Size every grid cap as on a device of n compute units inside the block (sr_grid_cus; 0: the device's own count): a
    measurement and test knob.  The counters of grid_stats() start at zero on entry; the previous setting comes back on exit."""
    n = int(n)
    if n < 0:
        raise ValueError(f"grid_cus: a compute-unit count or 0, got {n}")
    now = C.c_int(0)
    check(lib.sr_grid_cus(-1, C.byref(now)))
    before = 0 if now.value == compute_units() else now.value
    check(lib.sr_grid_cus(n, None))
    check(lib.sr_grid_stats(None, 1))
    try:
        yield
    finally:
        check(lib.sr_grid_cus(before, None))


def volume_bytes_estimate(n_nodes, phaseshift=False, inv_brems=False, B_on=False, ne_itemsize=8):
    """HBM a Volume of n_nodes holds (16 B per node packed, +4 with the phase, +8 kappa, +32 {n_e, B})
    plus the staging its construction needs for a moment (the uploaded n_e, float32(n_e / n_c), and for the optional terms the
    uploaded arrays)."""
    held = 16 + (4 if phaseshift else 0) + (8 if inv_brems else 0) + (32 if B_on else 0)
    staging = ne_itemsize + 4 + (8 if inv_brems else 0) + (32 if B_on else 0)
    return int(n_nodes) * (held + staging)


def release_caches():
    """Free what sr_trace keeps on the device between calls (its chunk pipeline's working set, ~1.5 GB of HBM)."""
    check(lib.sr_release_caches())


def synchronize() -> None:
    """Waits for every stream of the library."""
    check(lib.sr_synchronize())


def select_stream(index: int) -> None:
    """Queue the following calls on stream 0 (the default) or 1; see sr_stream_select in include/synthray.h."""
    check(lib.sr_stream_select(int(index)))


def stream_wait(waiting: int, on: int) -> None:
    """Work queued on stream `waiting` after this call starts once what stream `on` holds now is done (sr_stream_wait)."""
    check(lib.sr_stream_wait(int(waiting), int(on)))


def trapezoid_weights(g):
    """The weights w of the trapezoid rule on the nodes g, sum(w * f) = np.trapz(f, g): w_0 = (g_1 - g_0)/2,
    w_k = (g_{k+1} - g_{k-1})/2, w_{n-1} = (g_{n-1} - g_{n-2})/2 -- what sr_volume_project builds from the volume's float64
    node coordinates of the probing axis."""
    g = np.asarray(g, dtype=np.float64)
    if g.ndim != 1 or len(g) < 2:
        raise ValueError(f"the trapezoid rule needs at least 2 nodes on one axis, got shape {g.shape}")
    w = np.empty_like(g)
    w[0], w[-1] = (g[1] - g[0]) / 2, (g[-1] - g[-2]) / 2
    w[1:-1] = (g[2:] - g[:-2]) / 2
    return w


def default_t_end(extent: float) -> float:
    """t = sqrt(8)*extent/c: long enough for every ray to leave the volume (full_solver.py:381)."""
    return float(np.sqrt(8.0) * extent / c)


@dataclass
class TraceStats:
    ray_steps: int = 0
    fallback_rays: int = 0
    trace_kernel_ms: float = 0.0
    total_ms: float = 0.0


PRECISIONS = {"f64": 0, "mixed": 1}
DEFAULT_PRECISION = "auto"


def resolve_precision(precision, volume, *, resident=True, handoff=0, substeps=1) -> str:
    """"auto" (the default) picks the build by what the trace is for, so that EVERY default path gives the images of the
    float64 build (= the oracle's from the same s0: counts integer for integer, interferograms to 1e-5 of their maximum).

    * A volume built with the phase integral (phaseshift=True: the Jones vector feeds Interferometry) is traced in
      float64: the reference's field propagation multiplies E by exp(i*k*|dr|) with k = 2*pi/wavelength[m] against |dr|
      in mm (rtm_solver.py:380-384), 2.4e9 rad per radian of exit angle over a 400 mm leg, so only the float64 build
      (1e-14 rad from the oracle) reproduces an interferogram from the same rays
      (tests/test_gpu_parity.py::test_interferometry_end_to_end_from_s0).
    * Without the phase the detector images are counts (shadowgraphy, schlieren, refractometry).  Rays that stay in HBM
      (RayBundle.trace -> RayBundle.deposit) are traced by the mixed build (float32 stage arithmetic, 5e-11 m / 2e-8 rad
      from the oracle, twice as fast) and the deposit's EDGE GUARD traces again in float64 the ~1 % of them whose pixel
      or mask decision is not certain within the tracer's own per-ray error bound (sr_deposit_params.exact_counts).
    * Where no guard can follow -- host arrays out (`resident=False`: trace(), ScalarDomain.solve: the caller bins rf
      itself), slab hand-offs (a slab holds neither the rays' start nor the other planes) -- "auto" is float64; so it is with
      sub-steps and the optional terms, which the mixed build has no kernel for ("mixed" asked for by name runs the float64
        kernels there too).
    * Intensity images (RayBundle.deposit_intensity, Diagnostic.intensity, Polarimetry) need the Jones vector of a volume
      with the optional terms, which "auto" already traces in float64.  On a bundle traced by the mixed build the intensity
      deposit runs WITHOUT the edge guard: intensities are floating-point outputs, and the guard exists for the integer
      equality of counts.  Nothing in this function's result depends on it."""
    if precision in (None, "auto"):
        if getattr(volume, "phase", False) or not resident or handoff or substeps != 1 or getattr(volume, "aux", False):
            return "f64"
        return "mixed"
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be 'auto' or one of {sorted(PRECISIONS)}, got {precision!r}")
    return precision


HANDOFF_ENTER, HANDOFF_EXIT = 1, 2


def _trace_params(t_end, extent, axis, row_order, substeps, sort_rays, precision, dt=0.0, handoff=0):
    """precision "f64": every operation in float64 (the parity build: differs from the oracle by fused
    multiply-adds only, ~1e-17 m).  "mixed" (default): float64 state, stage positions and accumulation,
    float32 weights / blend / RK4 slopes: within 5e-11 m, 2e-8 rad and 4e-8 of the phase of the f64 build on
    the 512^3 benchmark, twice to three times as fast."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be 'auto' or one of {sorted(PRECISIONS)}, got {precision!r}")
    return _ffi.TraceParams(float(t_end), float(extent), float(dt), int(axis), int(row_order), int(substeps),
                            1 if sort_rays else 0, PRECISIONS[precision], int(handoff))


def deposit_params(kwave=0.0, ref_beam=None, lds_tiles=True, exact_counts=True):
    """sr_deposit_params.  ref_beam: None, one (n_fringes, deg) pair, or a list of up to MAX_REF_BEAMS pairs added in order."""
    refs = [] if ref_beam is None else ([tuple(ref_beam)] if np.isscalar(ref_beam[0]) else [tuple(b) for b in ref_beam])
    if len(refs) > _ffi.MAX_REF_BEAMS:
        raise ValueError(f"at most {_ffi.MAX_REF_BEAMS} reference beams per deposit, got {len(refs)}")
    p = _ffi.DepositParams()
    p.kwave = float(kwave)
    for q, (n_fringes, deg) in enumerate(refs):
        p.ref_n_fringes[q], p.ref_deg[q] = float(n_fringes), float(deg)
    p.ref_on, p.lds_tiles, p.exact_counts, p.reserved = len(refs), 1 if lds_tiles else 0, 1 if exact_counts else 0, 0
    return p


def make_chain(ops):
    """[(op, a[, b[, iarg]]), ...] -> ctypes array of sr_optic."""
    arr = (_ffi.Optic * max(1, len(ops)))()
    for k, o in enumerate(ops):
        arr[k].op = int(o[0])
        arr[k].a = float(o[1]) if len(o) > 1 else 0.0
        arr[k].b = float(o[2]) if len(o) > 2 else 0.0
        arr[k].iarg = int(o[3]) if len(o) > 3 else 0
    return arr


class Volume:
    """Device-resident fields of one ScalarDomain: the result of calc_dndr (+ n_refrac)."""

    def __init__(self, handle, shape, axis, phase=False):
        self._h = handle
        self.shape = tuple(int(s) for s in shape)
        self.axis = axis
        self.phase = bool(phase)  # the n-1 field is resident: the trace integrates the phase (A5)
        self.aux = False          # attach_aux: kappa / Faraday fields resident
        self.verdet = 0.0         # the VerdetConst attach_aux was given (Projection.rotation scales by it)

    @classmethod
    def from_ne(cls, ne, x, y, z, lwl, probing_direction="z", phaseshift=False):
        ne = np.asarray(ne)
        if ne.dtype != np.float32:
            ne = f64(ne)
        ne = np.ascontiguousarray(ne)
        x, y, z = f32(x), f32(y), f32(z)
        if ne.shape != (len(x), len(y), len(z)):
            raise ValueError(f"ne has shape {ne.shape}, coordinates give {(len(x), len(y), len(z))}")
        axis = axis_index(probing_direction)
        h = C.c_void_p()
        check(lib.sr_volume_create(C.byref(h), ptr(ne), 0 if ne.dtype == np.float32 else 1, len(x), len(y), len(z),
                                   ptr(x), ptr(y), ptr(z), float(lwl), axis, VOL_PHASE if phaseshift else 0))
        return cls(h, ne.shape, axis, phaseshift)

    @classmethod
    def from_ne_slab(cls, ne_slab, x, y, z, lwl, probing_direction, k_lo, k_hi, phaseshift=False):
        """Node planes k_lo..k_hi of the probing axis as a volume of their own (A12; BASELINE config 5).  x, y, z are
        the WHOLE domain's coordinates; ne_slab holds planes max(k_lo-1, 0)..min(k_hi+1, n-1) of the probing axis (see
        slab_source) so that the gradients equal the whole domain's bit for bit."""
        x, y, z = f32(x), f32(y), f32(z)
        axis = axis_index(probing_direction)
        n = (len(x), len(y), len(z))
        h_lo, h_hi = max(k_lo - 1, 0), min(k_hi + 1, n[axis] - 1)
        want = tuple(h_hi - h_lo + 1 if k == axis else n[k] for k in range(3))
        ne_slab = np.asarray(ne_slab)
        if ne_slab.dtype != np.float32:
            ne_slab = f64(ne_slab)
        ne_slab = np.ascontiguousarray(ne_slab)
        if ne_slab.shape != want:
            raise ValueError(f"ne_slab has shape {ne_slab.shape}; planes {h_lo}..{h_hi} of the domain give {want}")
        h = C.c_void_p()
        check(lib.sr_volume_create_slab(C.byref(h), ptr(ne_slab), 0 if ne_slab.dtype == np.float32 else 1, *n, ptr(x), ptr(y),
                                        ptr(z), float(lwl), axis, VOL_PHASE if phaseshift else 0, int(k_lo), int(k_hi)))
        shape = tuple(k_hi - k_lo + 1 if k == axis else n[k] for k in range(3))
        return cls(h, shape, axis, phaseshift)

    @classmethod
    def from_fields(cls, dndx, dndy, dndz, x, y, z, omega, probing_direction="z", nref=None):
        dndx, dndy, dndz = f32(dndx), f32(dndy), f32(dndz)
        x, y, z = f32(x), f32(y), f32(z)
        shape = (len(x), len(y), len(z))
        for a in (dndx, dndy, dndz):
            if a.shape != shape:
                raise ValueError(f"gradient volume has shape {a.shape}, coordinates give {shape}")
        nref = None if nref is None else f64(nref)
        axis = axis_index(probing_direction)
        h = C.c_void_p()
        check(lib.sr_volume_create_from_fields(C.byref(h), ptr(dndx), ptr(dndy), ptr(dndz), ptr(nref), float(omega),
                                               *shape, ptr(x), ptr(y), ptr(z), axis))
        return cls(h, shape, axis, nref is not None)

    @property
    def omega(self) -> float:
        return float(lib.sr_volume_omega(self._h))

    @property
    def nbytes(self) -> int:
        return int(lib.sr_volume_bytes(self._h))

    def fields(self, phase=False):
        """(dndx, dndy, dndz[, n-1]) read back in the reference's layout."""
        out = [np.empty(self.shape, np.float32) for _ in range(3)]
        nm1 = np.empty(self.shape, np.float64) if phase else None
        check(lib.sr_volume_fields(self._h, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(nm1)))
        return (*out, nm1) if phase else tuple(out)

    def sample(self, pts):
        """Interpolated (dndx, dndy, dndz, n-1) at pts (N,3): the gathers of dsdt, shape (4, N)."""
        pts = f64(pts).reshape(-1, 3)
        out = np.empty((4, len(pts)))
        check(lib.sr_volume_sample(self._h, ptr(pts), len(pts), ptr(out)))
        return out

    def attach_aux(self, kappa=None, ne=None, B=None, verdet=0.0):
        """The optional terms of dsdt (what set_up_interps builds, full_solver.py:276-289): kappa (nx,ny,nz) [1/s] for
        d(amp) = kappa*amp; ne (nx,ny,nz) and B (nx,ny,nz,3) with VerdetConst for d(pol) = VerdetConst*ne*(B.v)."""
        if kappa is not None:
            kappa = f64(kappa)
            if kappa.shape != self.shape:
                raise ValueError(f"kappa has shape {kappa.shape}, the volume {self.shape}")
        if (ne is None) != (B is None):
            raise ValueError("ne and B go together")
        if B is not None:
            ne, B = f64(ne), f64(B)
            if ne.shape != self.shape or B.shape != self.shape + (3,):
                raise ValueError(f"ne {ne.shape} / B {B.shape} do not match the volume {self.shape} (+ (3,))")
        check(lib.sr_volume_attach_aux(self._h, ptr(kappa), ptr(ne), ptr(B), float(verdet)))
        self.aux = kappa is not None or B is not None
        self.verdet = float(verdet)
        return self

    def project(self):
        """The line integrals of the volume along its probing axis (sr_volume_project): the trapezoid rule on the volume's
        own node coordinates, a slab over its own planes.  {"grad": (2, n_u, n_v) [u, v = the lateral axes in x < y < z
        order], "nm1", "ne", "kappa", "neB": (n_u, n_v) | None where the volume does not hold the field}."""
        if not getattr(self, "_h", None):
            raise ValueError("the volume has been closed")
        lateral = tuple(n for k, n in enumerate(self.shape) if k != self.axis)
        maps = np.empty((_ffi.PROJ_MAPS,) + lateral)
        have = C.c_uint32(0)
        check(lib.sr_volume_project(self._h, ptr(maps), C.byref(have)))
        pick = lambda k: maps[k] if have.value >> k & 1 else None
        return {"grad": maps[_ffi.PROJ_GRAD1:_ffi.PROJ_GRAD2 + 1], "nm1": pick(_ffi.PROJ_NM1), "ne": pick(_ffi.PROJ_NE),
                "kappa": pick(_ffi.PROJ_KAPPA), "neB": pick(_ffi.PROJ_NEB)}

    def sample_aux(self, pts):
        """Interpolated (kappa, ne, Bx, By, Bz) at pts (N,3): the gathers of atten / get_ne / get_B, shape (5, N)."""
        pts = f64(pts).reshape(-1, 3)
        out = np.empty((5, len(pts)))
        check(lib.sr_volume_sample_aux(self._h, ptr(pts), len(pts), ptr(out)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            lib.sr_volume_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resample_params(M, t=(0.0, 0.0, 0.0), V=None, fill=0.0):
    """sr_resample_params: p = M q + t (M 3x3, t 3), the optional component matrix V (3x3) and the fill value (one, or one per
    component)."""
    M, t = f64(M), f64(t)
    if M.shape != (3, 3) or t.shape != (3,):
        raise ValueError(f"M must be 3x3 and t have 3 entries, got {M.shape} and {t.shape}")
    p = _ffi.ResampleParams()
    p.M[:], p.t[:] = M.ravel().tolist(), t.tolist()
    if V is not None:
        V = f64(V)
        if V.shape != (3, 3):
            raise ValueError(f"V must be 3x3, got {V.shape}")
        p.V[:] = V.ravel().tolist()
    p.fill[:] = np.broadcast_to(f64(fill), (3,)).tolist()
    p.use_V, p.reserved = 0 if V is None else 1, 0
    return p


class Field:
    """A scalar (nx, ny, nz) or 3-vector (nx, ny, nz, 3) field on a rectilinear grid, resident in HBM (sr_field): uploaded
    once, resampled onto as many view grids as wanted."""

    def __init__(self, data, x, y, z):
        data = np.asarray(data)
        if data.dtype != np.float32:
            data = f64(data)
        data = np.ascontiguousarray(data)
        x, y, z = f32(x), f32(y), f32(z)
        grid = (len(x), len(y), len(z))
        if data.shape != grid and data.shape != grid + (3,):
            raise ValueError(f"the field has shape {data.shape}, coordinates give {grid} (+ (3,) for a vector field)")
        self.shape, self.dtype = data.shape, data.dtype
        self.n_comp = 3 if data.ndim == 4 else 1
        self.last_kernel_ms = 0.0
        self._h = None
        h = C.c_void_p()
        check(lib.sr_field_create(C.byref(h), ptr(data), 0 if data.dtype == np.float32 else 1, self.n_comp, *grid,
                                  ptr(x), ptr(y), ptr(z)))
        self._h = h

    @property
    def nbytes(self) -> int:
        return int(lib.sr_field_bytes(self._h))

    def resample(self, M, t, coords_out, V=None, fill=0.0):
        """The field at the nodes of the view grid coords_out = (ox, oy, oz), node q at the lab position p = M q + t:
        trilinear inside the source grid, `fill` outside (sr_field_resample; include/synthray.h states the rule).  V (3x3,
        vector fields): the output components are V times the interpolated ones.  An ndarray (mx, my, mz[, 3]) of the
        field's dtype."""
        if not getattr(self, "_h", None):
            raise ValueError("the field has been closed")
        ox, oy, oz = (f32(a) for a in coords_out)
        if V is not None and self.n_comp != 3:
            raise ValueError("V applies to a vector field (nx, ny, nz, 3)")
        p = resample_params(M, t, V, fill)
        out = np.empty((len(ox), len(oy), len(oz)) + ((3,) if self.n_comp == 3 else ()), self.dtype)
        ms = C.c_double(0.0)
        check(lib.sr_field_resample(self._h, C.byref(p), len(ox), len(oy), len(oz), ptr(ox), ptr(oy), ptr(oz), ptr(out),
                                    C.byref(ms)))
        self.last_kernel_ms = float(ms.value)
        return out

    def close(self):
        if getattr(self, "_h", None):
            lib.sr_field_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


HBAR = 6.62607015e-34 / (2 * np.pi)  # J s, from the exact h of the SI
E_CHARGE = 1.602176634e-19           # C


def spectrum_constants(omegas):
    """(omega, e_ph, c_omega), float64 (n_freq): the per-band constants of every entry of the emission family for any number of
    angular frequencies [rad/s], E_ph = hbar*omega/e [eV] and C_omega = hbar*omega^3/(4 pi^3 c^2), the Planck function's prefactor,
    B_omega(Te) = C_omega / expm1(E_ph / Te).  Formed on Python floats, here and nowhere else, so that a frequency has the bits it
    has as a band of engine.sightlines."""
    om = np.atleast_1d(f64(omegas))
    if om.ndim != 1:
        raise ValueError(f"omegas must be a scalar or one-dimensional, got shape {om.shape}")
    w = om.tolist()
    return om, f64([HBAR * v / E_CHARGE for v in w]), f64([HBAR * v ** 3 / (4 * np.pi ** 3 * c ** 2) for v in w])


def emission_params(omegas, axis, toward=+1, Te=0.0, Z=0.0):
    """sr_emission_params for the bands `omegas` [rad/s] with spectrum_constants' E_ph and C_omega per band; Te, Z: the uniform
    values of absent fields."""
    om, e_ph, c_omega = (a.tolist() for a in spectrum_constants(omegas))
    p = _ffi.EmissionParams()
    p.axis, p.toward, p.n_band, p.reserved = int(axis), int(toward), len(om), 0
    for b in range(min(len(om), _ffi.MAX_BANDS)):
        p.omega[b], p.e_ph[b], p.c_omega[b] = om[b], e_ph[b], c_omega[b]
    p.Te, p.Z = float(Te), float(Z)
    return p


def _handle(name, a, *, number=False, none=False):
    """The sr_field handle of the open Field `a`, or None for what the entry takes in a field's place: a number (a uniform value,
    which the caller passes on) and / or None."""
    if isinstance(a, Field):
        if not getattr(a, "_h", None):
            raise ValueError(f"the field {name} has been closed")
        return a._h
    if (none and a is None) or (number and a is not None and np.ndim(a) == 0):
        return None
    other = {(False, False): "", (True, False): " or a number", (False, True): " or None", (True, True): ", a number or None"}
    raise ValueError(f"{name} must be an open engine.Field{other[number, none]}")


def _emission(entry, ne, Te, Z, omegas, axis, toward, backlight, *table):
    """What emission and emission_table share: the handles, the uniform Te / Z, the backlight's shape, the maps and ne's kernel
    time; entry: the library call, table: its arguments between the fields and the params."""
    h_ne = _handle("ne", ne)
    handles = [_handle(name, a, number=True) for name, a in (("Te", Te), ("Z", Z))]
    p = emission_params(omegas, axis, toward, *(0.0 if h else float(a) for h, a in zip(handles, (Te, Z))))
    nb = p.n_band
    lateral = tuple(n for k, n in enumerate(ne.shape[:3]) if k != p.axis) if 0 <= p.axis <= 2 else ne.shape[:2]
    if backlight is not None:
        backlight = f64(backlight)
        if backlight.shape != (nb,) + lateral:
            raise ValueError(f"backlight has shape {backlight.shape}, the bands and the lateral grid give {(nb,) + lateral}")
    I, tau = np.empty((nb,) + lateral), np.empty((nb,) + lateral)
    ms = C.c_double(0.0)
    check(entry(h_ne, *handles, *table, C.byref(p), ptr(backlight), ptr(I), ptr(tau), C.byref(ms)))
    ne.last_kernel_ms = float(ms.value)
    return I, tau


def emission(ne, Te, Z, omegas, axis, toward=+1, backlight=None):
    """Self-emission with self-absorption along grid axis `axis` (0 | 1 | 2) of the fields ne [m^-3], Te [eV], Z (sr_field_emission;
    include/synthray.h states the rule): (I, tau), each (n_band, n_u, n_v) float64 with (u, v) the lateral axes in x < y < z order.
    ne is a scalar Field; Te and Z are Fields on the same grid and of the same dtype, or floats (a uniform field, which is not read).
    omegas: up to 4 angular frequencies, done in one pass over the fields.  toward = +1 puts the detector behind the last plane
    (the direction the rays travel), -1 before the first.  backlight: (n_band, n_u, n_v) behind the far plane, or None.
    I is the spectral radiance per unit angular frequency [W m^-2 sr^-1 (rad/s)^-1].  The absorption coefficient is
    propagator.kappa / c -- the NRL low-frequency (inverse-bremsstrahlung) coefficient the tracer uses, trustworthy for
    hbar*omega <~ Te; the source function is Planck's.  ne.last_kernel_ms keeps the kernel's time."""
    return _emission(lib.sr_field_emission, ne, Te, Z, omegas, axis, toward, backlight)


def emission_table_params(table):
    """sr_emission_table for an utils.eos_opacity.OpacityTable (or anything with its members), and the arrays it points into
    (keep them alive for the call): the logarithms of the lattice and of the opacities, float64."""
    LT, LD = np.log(f64(table.temperatures)), np.log(f64(table.densities))
    LA = np.ascontiguousarray(np.log(f64(table.absorption)))
    LE = None if table.emission is None else np.ascontiguousarray(np.log(f64(table.emission)))
    if LA.ndim != 3 or LA.shape[1:] != (len(LT), len(LD)) or (LE is not None and LE.shape != LA.shape):
        raise ValueError(f"the table's opacities have shape {LA.shape}, its lattice gives (n_band, {len(LT)}, {len(LD)})")
    t = _ffi.EmissionTable()
    t.nT, t.nD = len(LT), len(LD)
    t.LT, t.LD, t.LA, t.LE = ptr(LT), ptr(LD), ptr(LA), ptr(LE)
    t.m_ion = float(table.A) * 1.66053906660e-24
    return t, (LT, LD, LA, LE)


def _table_omegas(table):
    """(t, keep, omegas): emission_table_params' struct and the arrays it points into (the caller holds them until the library
    call returns), and the table's angular frequencies, one per band, at its photon_energy."""
    t, keep = emission_table_params(table)
    omegas = np.atleast_1d(f64(table.photon_energy)) * E_CHARGE / HBAR
    if len(omegas) != keep[2].shape[0]:
        raise ValueError(f"the table has {keep[2].shape[0]} band(s) and {len(omegas)} photon energies")
    return t, keep, omegas


def emission_table(ne, Te, Z, table, axis, toward=+1, backlight=None):
    """engine.emission with the absorption and emission opacities of `table` (utils.eos_opacity.OpacityTable: a temperature x
    ion-density lattice, up to 4 bands) in place of the NRL coefficient (sr_field_emission_table; include/synthray.h states the
    rule): (I, tau), each (n_band, n_u, n_v) float64.  The ion density of a node is ne / Z; alpha = opacity * ni * m_ion, the
    opacity interpolated bilinearly in (log Te, log ni) on its logarithm, the edge value outside the lattice; S is the Planck
    function at the band's photon_energy times emission / absorption opacity.  I is the spectral radiance per unit angular
    frequency at photon_energy.  Fields, uniform Te / Z, axis, toward and backlight are engine.emission's.  Not modelled: Z from
    the table's own zf_table (the solve ne = ni * zf(T, ni)), group-integrated Planck functions, refraction, detector optics."""
    _handle("ne", ne)
    t, keep, omegas = _table_omegas(table)
    return _emission(lib.sr_field_emission_table, ne, Te, Z, omegas, axis, toward, backlight, C.byref(t))


_SIGHT_WANT = ("intensity", "optical_depth", "column", "chord", "steps")


def sightline_params(omegas, toward, step, max_steps, Te=0.0, Z=0.0):
    """sr_sightline_params: the bands of emission_params(omegas, ...), the march's direction, spacing and step cap."""
    e = emission_params(omegas, 0, toward, Te, Z)
    p = _ffi.SightlineParams()
    p.toward, p.n_band, p.max_steps, p.reserved, p.step = int(toward), e.n_band, int(max_steps), 0, float(step)
    p.omega[:], p.e_ph[:], p.c_omega[:] = list(e.omega), list(e.e_ph), list(e.c_omega)
    p.Te, p.Z = e.Te, e.Z
    return p


def _sightlines(params, table_kind, ne, Te, Z, origins, directions, omegas, table, backlight, want):
    """What sightlines and sightline_spectra share: the handles, the uniform Te / Z, the lines, the table, the backlight's shape,
    the outputs and ne's kernel time.  params(omegas, n, uniform, t) -> (the library call, its params struct, the shape of I and
    tau, what that shape is made of (for the error text), the call's arguments between the directions and the backlight);
    table_kind names the table's class in the error text."""
    h_ne = _handle("ne", ne)
    handles = [_handle(name, a, number=True) for name, a in (("Te", Te), ("Z", Z))]
    if (omegas is None) == (table is None):
        raise ValueError(f"exactly one of omegas (the NRL node) and table ({table_kind}) must be given")
    unknown = set(want) - set(_SIGHT_WANT)
    if unknown:
        raise ValueError(f"want names {sorted(unknown)}; the outputs are {_SIGHT_WANT}")
    o, d = f64(origins), f64(directions)
    if o.ndim != 2 or o.shape[0] != 3 or d.shape != o.shape:
        raise ValueError(f"origins and directions must both have shape (3, n), got {o.shape} and {d.shape}")
    n = o.shape[1]
    t, keep = None, None
    if table is not None:
        t, keep, omegas = _table_omegas(table)
    entry, p, shape, made_of, between = params(omegas, n, (0.0 if h else float(a) for h, a in zip(handles, (Te, Z))), t)
    if backlight is not None:
        backlight = f64(backlight)
        if backlight.shape != shape:
            raise ValueError(f"backlight has shape {backlight.shape}, {made_of} give {shape}")
    I, tau = np.empty(shape), np.empty(shape)
    opt = {"column": np.empty(n) if "column" in want else None, "chord": np.empty(n) if "chord" in want else None,
           "steps": np.empty(n, np.int32) if "steps" in want else None}
    ms = C.c_double(0.0)
    check(entry(h_ne, *handles, None if t is None else C.byref(t), C.byref(p), n, ptr(o), ptr(d), *between, ptr(backlight), ptr(I),
                ptr(tau), ptr(opt["column"]), ptr(opt["chord"]), ptr(opt["steps"]), C.byref(ms)))
    ne.last_kernel_ms = float(ms.value)
    out = {"intensity": I, "optical_depth": tau, **opt}
    return {k: out[k] for k in _SIGHT_WANT if k in want}


def sightlines(ne, Te, Z, origins, directions, *, omegas=None, table=None, toward, step, max_steps, backlight=None,
               want=_SIGHT_WANT):
    """Emission and absorption along the n half-lines origins[:, i] + t * directions[:, i], t >= 0 (both (3, n) [m]; a direction
    need not be a unit vector), through the fields ne [m^-3], Te [eV], Z (sr_field_sightlines; include/synthray.h states the
    rule): each line is clipped to the grid's box and marched in samples about `step` apart (at most max_steps of them), the
    fields interpolated trilinearly at every sample.  Exactly one of omegas (up to 4 angular frequencies: engine.emission's NRL
    node) and table (an utils.eos_opacity.OpacityTable: engine.emission_table's node).  toward = +1: the light travels along
    +direction, away from the origin (a backlighter at the origin); -1: towards the origin (a pinhole there).  Fields, uniform Te /
    Z and handles are engine.emission's.  backlight: (n_band, n) behind the far end of every line, or None.  Returns a dict with
    the arrays named in `want`: "intensity" and "optical_depth" (n_band, n), "column" (n; the integral of ne dl [m^-2]), "chord"
    (n; the length inside the box [m], 0 for a line that misses it) and "steps" (n) int32.  ne.last_kernel_ms keeps the kernel's
    time.  Not modelled: a finite pinhole or source, the cos^4 and solid-angle factors of a film's exposure, refraction, the
    detector's response, a table's own ionisation; one GPU."""
    def params(omegas, n, uniform, t):
        p = sightline_params(omegas, toward, step, max_steps, *uniform)
        return lib.sr_field_sightlines, p, (p.n_band, n), "the bands and the lines", ()

    return _sightlines(params, "an OpacityTable", ne, Te, Z, origins, directions, omegas, table, backlight, want)


def sightline_spectra(ne, Te, Z, origins, directions, *, omegas=None, table=None, toward, step, max_steps, backlight=None,
                      want=_SIGHT_WANT):
    """engine.sightlines for a spectrum: 1 to _ffi.MAX_FREQS (16384) frequencies along every line in one call, a GPU lane per
    frequency (sr_field_sightline_spectra; include/synthray.h states the rule by reference to sr_field_sightlines').  Lines, fields,
    uniform Te / Z, toward, step, max_steps and want are engine.sightlines'.  Exactly one of omegas (angular frequencies [rad/s]:
    the NRL node, trustworthy for hbar*omega <~ Te) and table (an utils.eos_opacity.SpectralOpacityTable, or an OpacityTable: one
    frequency per group, at its photon_energy).  backlight: (n, n_freq) behind the far end of every line, or None.  Returns
    engine.sightlines' dict with "intensity" and "optical_depth" shaped (n, n_freq) -- a line's spectrum is contiguous -- whose
    every element has the bits engine.sightlines returns for that line with that frequency as one of its (up to 4) bands; "column",
    "chord", "steps" (n).  ne.last_kernel_ms keeps the kernel's time.  Not modelled: what engine.sightlines does not model;
    group-integrated Planck functions; one GPU.  Spectral lines are engine.sightline_lines."""
    def params(omegas, n, uniform, t):
        om, e_ph, c_om = spectrum_constants(omegas)
        p = _ffi.SpectraParams()
        p.toward, p.max_steps, p.step = int(toward), int(max_steps), float(step)
        p.Te, p.Z = uniform
        # om, e_ph and c_om live as long as the pointers: ndarray.ctypes.data_as keeps a reference to its array
        return (lib.sr_field_sightline_spectra, p, (n, len(om)), "the lines and the frequencies",
                (len(om), None if t is not None else ptr(om), ptr(e_ph), ptr(c_om)))

    return _sightlines(params, "a SpectralOpacityTable", ne, Te, Z, origins, directions, omegas, table, backlight, want)


LINES_CHUNK = int(lib.sr_lines_chunk())  # samples of a chord sr_field_sightline_lines' kernel stages at a time


def line_table_params(lines):
    """sr_line_table for an utils.eos_opacity.LineTable (or anything with its members), and the arrays it points into (keep them
    alive for the call): the logarithms of the lattice, of the emissivity and of the absorption, float64."""
    LT, LD = np.log(f64(lines.temperatures)), np.log(f64(lines.ion_densities))
    w0, A = np.atleast_1d(f64(lines.omega0)), np.atleast_1d(f64(lines.mass_number))
    LJ = np.ascontiguousarray(np.log(f64(lines.emissivity)))
    LK = None if lines.absorption is None else np.ascontiguousarray(np.log(f64(lines.absorption)))
    if LJ.ndim != 3 or LJ.shape[1:] != (len(LT), len(LD)) or (LK is not None and LK.shape != LJ.shape):
        raise ValueError(f"the line table's emissivity has shape {LJ.shape}, its lattice gives (n_line, {len(LT)}, {len(LD)})")
    if w0.shape != (len(LJ),) or A.shape != (len(LJ),):
        raise ValueError(f"the line table has {len(LJ)} line(s), {w0.size} rest frequencies and {A.size} mass numbers")
    t = _ffi.LineTable()
    t.nT, t.nD, t.n_line, t.reserved = len(LT), len(LD), len(LJ), 0
    t.LT, t.LD, t.w0, t.A, t.LJ, t.LK = ptr(LT), ptr(LD), ptr(w0), ptr(A), ptr(LJ), ptr(LK)
    return t, (LT, LD, w0, A, LJ, LK)


def sightline_lines(ne, Te, Ti, Z, V, origins, directions, *, lines, omegas, continuum=False, toward, step, max_steps,
                    backlight=None, want=_SIGHT_WANT):
    """Spectral lines along every chord: the spectral radiance and the optical depth of the 1 to _ffi.MAX_LINES (32) lines of
    `lines` (an utils.eos_opacity.LineTable) at 1 to _ffi.MAX_FREQS angular frequencies `omegas` [rad/s], a GPU lane per frequency
    (sr_field_sightline_lines; include/synthray.h states the rule).  Each line is a Gaussian whose centre is shifted by the flow
    V [m/s] (a vector Field, or None: no shift) along the direction the light travels and whose width is the thermal one of Ti
    [eV] (a Field, or None: Ti = Te), sample by sample; emission and absorption strength come from the table at the sample's
    (Te, ne / Z).  continuum=True puts the lines on engine.sightline_spectra's NRL continuum.  Chords, ne, Te, Z (Fields or
    uniform numbers), toward, step, max_steps, backlight ((n, n_freq)) and want are engine.sightline_spectra's, and so is the dict
    returned; where no line reaches a frequency its values have engine.sightline_spectra's bits (continuum) or are the backlight
    and 0.  ne.last_kernel_ms keeps the kernel's time.  Not modelled: Lorentzian, Stark and Voigt wings, Zeeman splitting, line
    blending through the cutoff at exp(-40), partial redistribution, refraction, the instrument function; one GPU."""
    return _line_family(lib.sr_field_sightline_lines, line_table_params, "a LineTable", ne, Te, Ti, Z, V, origins, directions, lines,
                        omegas, continuum, _NO_WING, toward, step, max_steps, backlight, want)


_NO_WING = object()  # sr_field_sightline_lines' params have no wing


def _line_family(entry, table_params, table_kind, ne, Te, Ti, Z, V, origins, directions, lines, omegas, continuum, wing, toward, step,
                 max_steps, backlight, want, polarised=None):
    """What sightline_lines, sightline_voigt, sightline_zeeman and sightline_stokes share under _sightlines: the handles of Ti and
    V, the table (table_params(lines)), the march struct (wing _NO_WING: LinesParams; else VoigtParams, its march and wing), the
    frequencies' constants and the call of the library's `entry`, whose argument order this function knows.  polarised: None, or
    (B, reference, what the entry takes between the backlight and I) for the two entries that march four Stokes parameters: B's
    handle, the reference, and the three maps beside I and tau, which `want` may then name."""
    h_Ti, h_V = _handle("Ti", Ti, none=True), _handle("V", V, none=True)
    fields, stokes_names, stokes = (), (), {}
    if polarised is not None:
        B, reference, after_backlight = polarised
        h_B = _handle("B", B, none=True)
        fields, stokes_names = (h_B,), ("Q", "U", "V")
    t, keep = table_params(lines)
    if polarised is not None:
        unknown = set(want) - set(_SIGHT_WANT) - set(stokes_names)
        if unknown:
            raise ValueError(f"want names {sorted(unknown)}; the outputs are {_SIGHT_WANT + stokes_names}")
        want_all, want = want, tuple(k for k in want if k in _SIGHT_WANT)

    def params(omegas, n, uniform, _):
        om, e_ph, c_om = spectrum_constants(omegas)
        p = _ffi.LinesParams() if wing is _NO_WING else _ffi.VoigtParams()
        m = p if wing is _NO_WING else p.march
        m.toward, m.max_steps, m.continuum, m.reserved, m.step = int(toward), int(max_steps), 1 if continuum else 0, 0, float(step)
        m.Te, m.Z = uniform
        if wing is not _NO_WING:
            p.wing = float(wing)
        after_chords = after_back = after_I = ()
        if polarised is not None:
            ref = None
            if h_B is not None:
                if reference is None:
                    raise ValueError("reference must be given with B: the direction Q is measured from, (3,) or (3, n)")
                ref = f64(reference)
                if ref.shape == (3,):
                    ref = np.repeat(ref[:, None], n, axis=1)
                if ref.shape != (3, n):
                    raise ValueError(f"reference must have shape (3,) or (3, {n}), got {ref.shape}")
                ref = np.ascontiguousarray(ref)
            for k in stokes_names:
                stokes[k] = np.empty((n, len(om)))
            after_chords, after_back, after_I = (ptr(ref),), after_backlight, tuple(ptr(stokes[k]) for k in stokes_names)

        def call(h_ne, h_Te, h_Z, _, p_, n_, o, d, nf, w, e, c, back, I, tau, *rest):  # _sightlines' argument order -> the entry's
            return entry(h_ne, h_Te, h_Ti, h_Z, h_V, *fields, C.byref(t), p_, n_, o, d, *after_chords, nf, w, e, c, back, *after_back,
                         I, *after_I, tau, *rest)

        return call, p, (n, len(om)), "the chords and the frequencies", (len(om), ptr(om), ptr(e_ph), ptr(c_om))

    out = _sightlines(params, table_kind, ne, Te, Z, origins, directions, omegas, None, backlight, want)
    if polarised is not None:
        out.update({k: stokes[k] for k in stokes_names if k in want_all})
    return out


VOIGT_CHUNK = _ffi.VOIGT_CHUNK  # samples of a chord sr_field_sightline_voigt's kernel stages at a time


def voigt_table_params(lines):
    """sr_voigt_table for an utils.eos_opacity.VoigtLineTable (or anything with its members; a table without lorentz_width, or with
    None there, gives LG NULL: Gaussian lines), and the arrays it points into (keep them alive for the call)."""
    t, keep = line_table_params(lines)
    width = getattr(lines, "lorentz_width", None)
    LG = None if width is None else np.ascontiguousarray(np.log(f64(width)))
    if LG is not None and LG.shape != keep[4].shape:
        raise ValueError(f"the line table's lorentz_width has shape {LG.shape}, its emissivity {keep[4].shape}")
    v = _ffi.VoigtTable()
    v.lines, v.LG = t, ptr(LG)
    return v, keep + (LG,)


def sightline_voigt(ne, Te, Ti, Z, V, origins, directions, *, lines, omegas, continuum=False, wing=np.inf, toward, step, max_steps,
                    backlight=None, want=_SIGHT_WANT):
    """engine.sightline_lines with Voigt profiles: every line of `lines` (an utils.eos_opacity.VoigtLineTable) has, beside its
    thermal width, the Lorentzian half-width [rad/s] the table gives at the sample's (Te, ne / Z) -- Stark and natural broadening --
    and its shape is the Voigt function of the two, accurate relative to itself far into the wings (sr_field_sightline_voigt;
    include/synthray.h states the rule and the algorithm).  wing: a term further than `wing` thermal 1/e widths from its line's
    centre is dropped (+inf, the default: never; a finite wing lets the kernel skip a line for whole wavefronts of a sorted
    frequency list).  Everything else -- the chords, the fields, continuum, toward, step, max_steps, backlight, want and the dict
    returned -- is engine.sightline_lines'; a table without lorentz_width gives that entry's bits.  ne.last_kernel_ms keeps the
    kernel's time.  Not modelled: Zeeman splitting, asymmetric and shifted Stark profiles, ion dynamics, blending through wing,
    partial redistribution, refraction, the instrument function; one GPU."""
    return _line_family(lib.sr_field_sightline_voigt, voigt_table_params, "a VoigtLineTable", ne, Te, Ti, Z, V, origins, directions,
                        lines, omegas, continuum, wing, toward, step, max_steps, backlight, want)


ZEEMAN_CHUNK = _ffi.ZEEMAN_CHUNK  # samples of a chord sr_field_sightline_zeeman's kernel stages at a time
M_ELECTRON = 9.1093837015e-31   # kg
LARMOR = E_CHARGE / (2.0 * M_ELECTRON)  # kL [rad/s/T], formed as sr_field_sightline_zeeman forms it


def zeeman_table_params(lines):
    """sr_zeeman_table for an utils.eos_opacity.ZeemanLineTable (or anything with its members: a VoigtLineTable's, where
    lorentz_width may be None -- Gaussian components -- and `patterns`, one (n, 3) array of (q, g, s) rows per line), and the arrays
    it points into (keep them alive for the call).  A table without patterns gives NULL component members: only a call without B
    accepts it."""
    v, keep = voigt_table_params(lines)
    patterns = getattr(lines, "patterns", None)
    n_comp = comp = None
    if patterns is not None:
        n_comp = np.array([len(p) for p in patterns], np.int32)
        comp = np.ascontiguousarray(np.concatenate([f64(p).reshape(-1, 3) for p in patterns], axis=0))
        if len(n_comp) != v.lines.n_line:
            raise ValueError(f"the line table has {v.lines.n_line} line(s) and {len(n_comp)} Zeeman pattern(s)")
    z = _ffi.ZeemanTable()
    z.voigt, z.n_comp, z.comp = v, ptr(n_comp), ptr(comp)
    return z, keep + (n_comp, comp)


def sightline_zeeman(ne, Te, Ti, Z, V, B, origins, directions, reference, *, lines, omegas, continuum=False, wing=np.inf, toward,
                     step, max_steps, backlight=None, want=_SIGHT_WANT + ("Q", "U", "V")):
    """engine.sightline_voigt in a magnetic field: every line of `lines` (an utils.eos_opacity.ZeemanLineTable) is split by the
    field B [T] (a vector Field on ne's grid, gathered at every sample like V) into the pi and sigma components of its pattern,
    each a Voigt profile shifted by g e |B| / (2 m_e), and the four Stokes parameters are marched along every chord with one scalar
    attenuation (sr_field_sightline_zeeman; include/synthray.h states the rule and the sign conventions).  reference: (3, n), or
    (3,) for all chords: with n^ the direction the light travels, e1 is `reference` minus its part along n^, normalised, and
    e2 = n^ x e1; Q > 0 is linear polarisation along e1, U > 0 along the bisector of e1 and e2, V > 0 the helicity of a q = +1
    component emitted along +B.  A reference parallel to its chord is an error.  Everything else -- the chords, the other fields,
    continuum, wing, toward, step, max_steps, backlight (unpolarised) and want -- is engine.sightline_voigt's, and the dict
    returned is its dict plus "Q", "U", "V", shaped as "intensity".  B = None: engine.sightline_voigt's bits and exact zeros in
    Q, U, V; the patterns and the reference are not read.  A table without lorentz_width has Gaussian components (it does NOT fall
    back to engine.sightline_lines).  ne.last_kernel_ms keeps the kernel's time.  Not modelled: dichroism and magneto-optical
    rotation in the absorption matrix (absorption acts equally on all four parameters), Faraday rotation of the continuum, the
    Paschen-Back regime, hyperfine structure, and what engine.sightline_voigt does not model; one GPU."""
    return _line_family(lib.sr_field_sightline_zeeman, zeeman_table_params, "a ZeemanLineTable", ne, Te, Ti, Z, V, origins, directions,
                        lines, omegas, continuum, wing, toward, step, max_steps, backlight, want, (B, reference, ()))


STOKES_CHUNK = _ffi.STOKES_CHUNK  # samples of a chord sr_field_sightline_stokes' kernel stages at a time
EPS0 = 8.8541878128e-12  # F/m
# kF [rad m^-1 per (m^-3 T (rad/s)^-2)]: the plane of polarisation turns by kF ne B.n^ s / omega^2; formed as the library forms it
FARADAY = ((E_CHARGE * E_CHARGE) * E_CHARGE) / ((((2.0 * EPS0) * M_ELECTRON) * M_ELECTRON) * c)


def sightline_stokes(ne, Te, Ti, Z, V, B, origins, directions, reference, *, lines, omegas, continuum=False, wing=np.inf, toward,
                     step, max_steps, backlight=None, polarisation=None, faraday=False, want=_SIGHT_WANT + ("Q", "U", "V")):
    """engine.sightline_zeeman with the whole absorption matrix of the polarised transfer equation in the update
    (sr_field_sightline_stokes; include/synthray.h states the rule, the algorithm and the sign conventions): the lines' absorption
    is dichroic (hQ, hU, hV: the sums of jQ, jU, jV with the table's absorption), the plane of polarisation turns inside the lines
    (rQ, rU, rV, from the imaginary part of the Faddeeva function) and, with faraday=True, in the continuum, by
    FARADAY * ne * B.n^ / omega^2 per metre from e1 towards e2 for B along the light's travel.  polarisation: (q, u, v), the
    backlight's Stokes parameters as fractions of its intensity, q^2 + u^2 + v^2 <= 1; None: unpolarised.  Everything else -- the
    chords, the fields, reference, continuum, wing, toward, step, max_steps, backlight, want and the dict returned -- is
    engine.sightline_zeeman's; with a table without absorption, faraday=False and polarisation=None it returns that entry's bits,
    with B = None engine.sightline_voigt's (faraday or polarisation are then errors).  ne.last_kernel_ms keeps the kernel's time.
    Not modelled: the Paschen-Back regime, hyperfine structure, cyclotron dichroism of the continuum, scattering polarisation, the
    Hanle effect, and what engine.sightline_voigt does not model; one GPU."""
    pol = None
    if polarisation is not None:
        pol = f64(polarisation)
        if pol.shape != (3,):
            raise ValueError(f"polarisation must be (q, u, v), got shape {pol.shape}")
        pol = np.ascontiguousarray(pol)
    return _line_family(lib.sr_field_sightline_stokes, zeeman_table_params, "a ZeemanLineTable", ne, Te, Ti, Z, V, origins, directions,
                        lines, omegas, continuum, wing, toward, step, max_steps, backlight, want,
                        (B, reference, (ptr(pol), 1 if faraday else 0)))


PUSH_UNFINISHED, PUSH_MISSED = _ffi.PUSH_UNFINISHED, _ffi.PUSH_MISSED
_PUSH_WANT = ("sf", "hits", "steps", "flags")


@dataclass
class PushStats:
    kernel_ms: float   # HIP-event time of the push kernel alone
    finished: int      # particles that left the grid box
    unfinished: int    # still inside after max_steps (PUSH_UNFINISHED)
    missed: int        # do not reach the detector plane (PUSH_MISSED)
    deposited: int     # binned inside the image


def push_params(qm, dt, max_steps, axis, det_pos, hit_scale=1e3):
    """sr_push_params."""
    p = _ffi.PushParams()
    p.qm, p.dt, p.max_steps, p.axis, p.det_pos, p.hit_scale = float(qm), float(dt), int(max_steps), int(axis), float(det_pos), float(hit_scale)
    return p


def push_particles(E, B, s0, qm, dt, max_steps, axis, det_pos, hit_scale=1e3, image=None, want=_PUSH_WANT):
    """Push the particles s0 (6, n: x y z [m], ux uy uz = gamma*v [m/s]) of charge/mass qm [C/kg] through the vector Fields E [V/m]
    and B [T] (either may be None: zero) with the fixed step dt until they leave the grid box or have made max_steps steps, and
    project them onto the plane coordinate[axis] == det_pos (sr_particles_push; include/synthray.h states the rule).  Returns a
    dict with the arrays named in `want` -- "sf" (6, n), "hits" (2, n; times hit_scale), "steps" (n) int32, "flags" (n) uint8
    (PUSH_UNFINISHED | PUSH_MISSED) -- and "stats" (PushStats).  image: a counts DetectorImage the particles with flags == 0 are
    added to on the device."""
    h_E, h_B = _handle("E", E, none=True), _handle("B", B, none=True)
    s0 = f64(s0)
    if s0.ndim != 2 or s0.shape[0] != 6:
        raise ValueError(f"s0 must have shape (6, n), got {s0.shape}")
    unknown = set(want) - set(_PUSH_WANT)
    if unknown:
        raise ValueError(f"want names {sorted(unknown)}; the outputs are {_PUSH_WANT}")
    if image is not None and not isinstance(image, DetectorImage):
        raise ValueError("image must be an engine.DetectorImage of counts")
    n = s0.shape[1]
    out = {}
    if "sf" in want:
        out["sf"] = np.empty((6, n))
    if "hits" in want:
        out["hits"] = np.empty((2, n))
    if "steps" in want:
        out["steps"] = np.empty(n, np.int32)
    if "flags" in want:
        out["flags"] = np.empty(n, np.uint8)
    p = push_params(qm, dt, max_steps, axis, det_pos, hit_scale)
    st = _ffi.PushStats()
    check(lib.sr_particles_push(h_E, h_B, C.byref(p), n, ptr(s0),
                                ptr(out.get("sf")), ptr(out.get("hits")), ptr(out.get("steps")), ptr(out.get("flags")),
                                None if image is None else image._h, C.byref(st)))
    out["stats"] = PushStats(float(st.kernel_ms), int(st.finished), int(st.unfinished), int(st.missed), int(st.deposited))
    return out


PUSH_STOPPED = _ffi.PUSH_STOPPED
_PUSH_MATTER_WANT = _PUSH_WANT + ("energy", "moments")


@dataclass
class PushMatterStats(PushStats):
    stopped: int       # stopped in the matter (PUSH_STOPPED); they count as finished


def push_matter_params(qm, dt, max_steps, axis, det_pos, hit_scale=1e3, *, mass, z, Zn, I, lnLs, Z=0.0, stop_energy=0.0):
    """sr_push_matter_params."""
    p = _ffi.PushMatterParams()
    p.push = push_params(qm, dt, max_steps, axis, det_pos, hit_scale)
    p.mass, p.z, p.Zn, p.I, p.lnLs, p.Z, p.stop_energy = float(mass), float(z), float(Zn), float(I), float(lnLs), float(Z), float(stop_energy)
    return p


def push_particles_matter(E, B, ne, Z, s0, qm, dt, max_steps, axis, det_pos, hit_scale=1e3, *, mass, z, Zn, I, lnLs, stop_energy=0.0,
                          image=None, want=_PUSH_MATTER_WANT):
    """push_particles through matter (sr_particles_push_matter; include/synthray.h states the rule): beside E and B (both may be
    None) the particles cross the electron density ne [m^-3] (a scalar Field) of mean ionisation Z (a scalar Field, or a number:
    a uniform value, which is not read), in which they lose energy by Bethe's stopping power of the free and the bound electrons
    and gather the moments of the multiple-scattering power.  mass [kg] and z: the projectile's mass and charge number; Zn, I [J],
    lnLs: the material's nuclear charge, mean excitation energy and scattering logarithm; stop_energy [J]: a particle whose
    kinetic energy falls below it is stopped (PUSH_STOPPED) and not binned.  Returns push_particles' dict with, when named in
    `want`, "energy" (n) [J] on leaving or stopping and "moments" (4, n): M0, M1, M2 of the scattering power over the path
    length, and the path length; "stats" is a PushMatterStats."""
    unknown = set(want) - set(_PUSH_MATTER_WANT)
    if unknown:
        raise ValueError(f"want names {sorted(unknown)}; the outputs are {_PUSH_MATTER_WANT}")
    h_E, h_B = _handle("E", E, none=True), _handle("B", B, none=True)
    h_ne, h_Z = _handle("ne", ne), _handle("Z", Z, number=True)
    s0 = f64(s0)
    if s0.ndim != 2 or s0.shape[0] != 6:
        raise ValueError(f"s0 must have shape (6, n), got {s0.shape}")
    if image is not None and not isinstance(image, DetectorImage):
        raise ValueError("image must be an engine.DetectorImage of counts")
    n = s0.shape[1]
    shapes = {"sf": ((6, n), np.float64), "hits": ((2, n), np.float64), "steps": (n, np.int32), "flags": (n, np.uint8),
              "energy": (n, np.float64), "moments": ((4, n), np.float64)}
    out = {name: np.empty(*shapes[name]) for name in _PUSH_MATTER_WANT if name in want}
    p = push_matter_params(qm, dt, max_steps, axis, det_pos, hit_scale, mass=mass, z=z, Zn=Zn, I=I, lnLs=lnLs,
                           Z=0.0 if h_Z else float(Z), stop_energy=stop_energy)
    st = _ffi.PushMatterStats()
    check(lib.sr_particles_push_matter(h_E, h_B, h_ne, h_Z, C.byref(p), n, ptr(s0),
                                       *(ptr(out.get(name)) for name in _PUSH_MATTER_WANT),
                                       None if image is None else image._h, C.byref(st)))
    out["stats"] = PushMatterStats(float(st.kernel_ms), int(st.finished), int(st.unfinished), int(st.missed), int(st.deposited),
                                   int(st.stopped))
    return out


MAX_SPECIES = _ffi.MAX_SPECIES  # the ion species thomson_multi takes at most


def thomson(ne, Te, Ti, Z, V, lambda_i, ion_mass, points, weights, ki, ks, wavelengths):
    """The Thomson-scattering spectral density summed over the quadrature of each scattering volume (sr_field_thomson;
    include/synthray.h states the rule): (P (M, n_lambda), weight (M)) float64, P = (1/2pi) sum_q w_q ne_q S_q (1 + 2w/wi)
    |dw/dlambda| and weight = sum_q w_q ne_q over the points that lie inside the grid with ne, Te, Ti > 0.  ne [m^-3] and Te [eV]
    are scalar Fields; Ti [eV] a Field or None (Ti = Te); Z a Field or a float (a uniform charge, which is not read); V [m/s] a
    vector Field or None (no flow) -- all on one grid and of one dtype.  lambda_i: the probe's wavelength [m]; ion_mass: the mass
    number A; points (M, Nq, 3) [m] and weights (M, Nq) [m]; ki, ks: the unit probe and collection directions, (3,) or (M, 3);
    wavelengths (n_lambda) [m].  ne.last_kernel_ms keeps the kernel's time."""
    handles = [_handle("ne", ne), _handle("Te", Te), _handle("Ti", Ti, none=True), _handle("Z", Z, number=True),
               _handle("V", V, none=True)]
    p = _ffi.ThomsonParams()
    p.lambda_i, p.A, p.Z = float(lambda_i), float(ion_mass), 0.0 if isinstance(Z, Field) else float(Z)
    return _thomson(lib.sr_field_thomson, ne, handles, p, points, weights, ki, ks, wavelengths)


def _thomson(entry, ne, head, p, points, weights, ki, ks, wavelengths):
    """What thomson and thomson_multi share: the volumes' arrays, the outputs and ne's kernel time; entry: the library call, head: its
    arguments before the params p."""
    points, weights = f64(points), f64(weights)
    if points.ndim != 3 or points.shape[2] != 3 or weights.shape != points.shape[:2]:
        raise ValueError(f"points must be (M, Nq, 3) and weights (M, Nq), got {points.shape} and {weights.shape}")
    M, nq = weights.shape
    dirs = []
    for name, d in (("ki", ki), ("ks", ks)):
        d = f64(d)
        if d.shape not in ((3,), (M, 3)):
            raise ValueError(f"{name} must have shape (3,) or ({M}, 3), got {d.shape}")
        dirs.append(np.ascontiguousarray(np.broadcast_to(d, (M, 3))))
    lam = f64(wavelengths)
    if lam.ndim != 1:
        raise ValueError(f"wavelengths must be one-dimensional, got shape {lam.shape}")
    P, weight = np.zeros((M, len(lam))), np.zeros(M)
    ms = C.c_double(0.0)
    check(entry(*head, C.byref(p), M, nq, ptr(points), ptr(weights), ptr(dirs[0]), ptr(dirs[1]), len(lam), ptr(lam), ptr(P), ptr(weight),
                C.byref(ms)))
    ne.last_kernel_ms = float(ms.value)
    return P, weight


def _species_head(p, ne, Te, Ti, V, Vd, species, lambda_i):
    """What thomson_multi and thomson_sg share: the handles of the fields and of the species' charges and fractions (the call's
    arguments before the params), and the params p with lambda_i and the species filled in."""
    head = [_handle("ne", ne), _handle("Te", Te), _handle("Ti", Ti, none=True), _handle("V", V, none=True), _handle("Vd", Vd, none=True)]
    species = [tuple(s) for s in species]
    n = len(species)
    if not 1 <= n <= _ffi.MAX_SPECIES or any(len(s) != 3 for s in species):
        raise ValueError(f"species must be 1 to {_ffi.MAX_SPECIES} entries (A, Z, fraction), got {n}")
    p.lambda_i, p.n_species, p.reserved = float(lambda_i), n, 0
    Zs, fracs = (C.c_void_p * n)(), (C.c_void_p * n)()
    for j, (A, Z, frac) in enumerate(species):
        Zs[j], fracs[j] = _handle(f"Z{j}", Z, number=True), _handle(f"f{j}", frac, number=True)
        p.A[j], p.Z[j], p.frac[j] = float(A), 0.0 if isinstance(Z, Field) else float(Z), 0.0 if isinstance(frac, Field) else float(frac)
    return head + [Zs, fracs], p


def thomson_multi(ne, Te, Ti, V, Vd, species, lambda_i, points, weights, ki, ks, wavelengths):
    """thomson for a plasma of 1 to _ffi.MAX_SPECIES ion species whose electrons may drift against the ions
    (sr_field_thomson_multi; include/synthray.h states the rule): (P (M, n_lambda), weight (M)) float64.  ne, Te, Ti, V and the
    volumes' arguments are thomson's.  Vd [m/s]: a vector Field, the electrons' drift relative to the ions -J/(e ne), or None (no
    drift).  species: a sequence of (A, Z, fraction) -- the mass number, and the charge and the relative number fraction (they need
    not sum to 1), each a scalar Field or a float (uniform, not negative).  All fields on one grid and of one dtype.
    ne.last_kernel_ms keeps the kernel's time."""
    head, p = _species_head(_ffi.ThomsonMultiParams(), ne, Te, Ti, V, Vd, species, lambda_i)
    return _thomson(lib.sr_field_thomson_multi, ne, head, p, points, weights, ki, ks, wavelengths)


def thomson_sg(ne, Te, Ti, V, Vd, species, order, lambda_i, points, weights, ki, ks, wavelengths):
    """thomson_multi with super-Gaussian (Langdon) electrons f(v) ~ exp(-(v/v_m)^m) (sr_field_thomson_sg; include/synthray.h
    states the rule): (P (M, n_lambda), weight (M)) float64.  order: the local m -- a scalar Field on the grid and of the dtype
    of the others (gathered per point; NaN drops the point, other values are clamped to [2, 5]) or a float in [2, 5] (uniform).
    m = 2 returns thomson_multi's bits.  Everything else is thomson_multi's."""
    head, p = _species_head(_ffi.ThomsonSgParams(), ne, Te, Ti, V, Vd, species, lambda_i)
    h_order = _handle("order", order, number=True)
    p.order = 2.0 if isinstance(order, Field) else float(order)
    return _thomson(lib.sr_field_thomson_sg, ne, head + [h_order], p, points, weights, ki, ks, wavelengths)


def wave_params(frame, shape, lambda_, axis, toward=+1, Z=0.0, time_parts=False):
    """sr_wave_params for a frame (u0, du, v0, dv) [m] of shape (mu, mv) and the vacuum wavelength lambda_ [m]: omega = 2 pi c /
    lambda, k0 = omega / c and pi_l = pi * lambda are formed here, as emission_params forms its constants."""
    u0, du, v0, dv = (float(a) for a in frame)
    p = _ffi.WaveParams()
    p.axis, p.toward, p.mu, p.mv = int(axis), int(toward), int(shape[0]), int(shape[1])
    p.u0, p.du, p.v0, p.dv = u0, du, v0, dv
    lam = float(lambda_)
    p.lambda_ = lam
    p.omega = 2 * np.pi * c / lam if lam != 0 else np.inf
    p.k0 = p.omega / c
    p.pi_l = np.pi * lam
    p.Z, p.time_parts, p.reserved = float(Z), 1 if time_parts else 0, 0
    return p


def _complex_field(U, name="U"):
    U = np.ascontiguousarray(U, dtype=np.complex128)
    if U.ndim != 2:
        raise ValueError(f"{name} must be a two-dimensional complex array (mu, mv), got shape {U.shape}")
    return U


def wave(ne, Te, Z, U, frame, lambda_, axis, toward=+1, absorber=None, want_power=True, time_parts=False):
    """The paraxial split-step march of the complex field U (mu, mv) through the electron density `ne` along grid axis `axis`
    (sr_field_wave; include/synthray.h states the rule): (U_out (mu, mv) complex128 on the last plane of the march, power (n_cells)
    float64 = sum |U|^2 after every screen, or None).  ne [m^-3] is a scalar Field; Te [eV] a Field on the same grid and of the same
    dtype, or None (no absorption); Z a Field or a number (a uniform charge, which is not read), looked at only with Te.  frame =
    (u0, du, v0, dv) [m]: pixel (i, j) sits at (u0 + i du, v0 + j dv) on the lateral axes in x < y < z order.  lambda_: the vacuum
    wavelength [m].  toward = +1 marches from the first node plane to the last.  absorber: (wu (mu), wv (mv)) windows applied with
    every screen (wave.edge_absorber), or None.  The field varies as exp(+i(kz - wt)) without its carrier: plasma retards the phase.
    ne.last_kernel_ms keeps the march's HIP-event time.  time_parts=True puts an event between all the launches and returns a
    third value, (hipFFT ms, own kernels ms): a measurement mode (tools/wave_rate.py)."""
    handles = [_handle("ne", ne)] + [_handle(name, a, number=True, none=True) for name, a in (("Te", Te), ("Z", Z))]
    U = _complex_field(U)
    mu, mv = U.shape
    p = wave_params(frame, U.shape, lambda_, axis, toward, 0.0 if isinstance(Z, Field) or Z is None else float(Z), time_parts)
    fu, fv = np.fft.fftfreq(mu, p.du if p.du else 1.0), np.fft.fftfreq(mv, p.dv if p.dv else 1.0)
    wu = wv = None
    if absorber is not None:
        wu, wv = f64(absorber[0]), f64(absorber[1])
        if wu.shape != (mu,) or wv.shape != (mv,):
            raise ValueError(f"absorber must be (wu ({mu},), wv ({mv},)), got {wu.shape} and {wv.shape}")
    out = np.empty_like(U)
    n_cells = ne.shape[p.axis] - 1 if 0 <= p.axis <= 2 else 1
    power = np.zeros(n_cells) if want_power else None
    ms = (C.c_double * 3)(0.0, 0.0, 0.0)
    check(lib.sr_field_wave(*handles, C.byref(p), ptr(fu), ptr(fv), ptr(wu), ptr(wv), ptr(U), ptr(out), ptr(power), ms))
    ne.last_kernel_ms = float(ms[0])
    if time_parts:
        return out, power, (float(ms[1]), float(ms[2]))
    return out, power


def wave_image(U, du, dv, lambda_, f=1.0, defocus=0.0, aperture=None, stop=None, knife=None):
    """The field U (mu, mv) on a frame of pitch (du, dv) [m] relayed one-to-one to the detector through a mask in the Fourier plane
    of a lens of focal length f [m], with a defocus [m] (sr_wave_image; include/synthray.h states the rule): (mu, mv) complex128.
    aperture: radius [m] outside which the focal plane is blocked; stop: radius [m] inside which it is; knife: (axis 0 | 1 -- u | v
    --, offset [m], direction > 0: blocked above the offset, < 0: below).  The inequalities are the ray optics' (strict)."""
    U = _complex_field(U)
    mu, mv = U.shape
    p = _ffi.WaveImageParams()
    p.mu, p.mv, p.flags, p.knife_axis = mu, mv, 0, 0
    p.pi_l, p.defocus, p.lf = np.pi * float(lambda_), float(defocus), float(lambda_) * float(f)
    if aperture is not None:
        p.flags |= _ffi.WAVE_APERTURE
        p.Ra = float(aperture)
    if stop is not None:
        p.flags |= _ffi.WAVE_STOP
        p.Rs = float(stop)
    if knife is not None:
        p.flags |= _ffi.WAVE_KNIFE
        p.knife_axis, p.knife_offset, p.knife_dir = int(knife[0]), float(knife[1]), float(knife[2])
    du, dv = float(du), float(dv)
    if not (du > 0 and dv > 0 and np.isfinite(du) and np.isfinite(dv)):
        raise ValueError(f"du and dv must be finite and positive, got {du!r} and {dv!r}")
    fu, fv = np.fft.fftfreq(mu, du), np.fft.fftfreq(mv, dv)
    out = np.empty_like(U)
    ms = C.c_double(0.0)
    check(lib.sr_wave_image(C.byref(p), ptr(fu), ptr(fv), ptr(U), ptr(out), C.byref(ms)))
    return out, float(ms.value)


class _PinnedBlock:
    """One page-locked host block (sr_host_alloc) under a NumPy array: the array's base; goes back to the pool when the
    last array over it is collected."""
    __slots__ = ("ptr", "nbytes", "__array_interface__", "__weakref__")

    def __init__(self, ptr_, nbytes, shape, dtype):
        self.ptr, self.nbytes = ptr_, nbytes
        self.__array_interface__ = {"shape": shape, "typestr": np.dtype(dtype).str, "data": (ptr_, False), "version": 3}

    def __del__(self):
        try:
            _pinned_release(self.ptr, self.nbytes)
        except Exception:  # interpreter shutting down
            pass


PINNED_MIN_BYTES = 8 << 20    # smaller result arrays are ordinary NumPy arrays
PINNED_POOL_BYTES = 4 << 30   # free blocks kept for the next call; beyond this they are given back (sr_host_free)
# "auto": a size is page-locked from the SECOND time it is asked for (locking 1.4 GB costs ~270 ms, four times what it
# saves per call: a script that traces once keeps NumPy's pageable arrays, a loop gets the fast ones); "1" always, "0" never
PINNED_RESULTS = os.environ.get("SYNTHRAY_PINNED_RESULTS", "auto")
_pinned_free, _pinned_held, _pinned_asked = {}, [0], {}
_pinned_live = [0]  # bytes of page-locked memory under arrays the caller still holds


def _mem_total():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemTotal:"):
                return int(line.split()[1]) * 1024
    except (OSError, ValueError):
        pass
    return 64 << 30


# Page-locked memory is taken from what the host can swap or reclaim: a loop that KEEPS its results (1.4 GB per 1e7 rays)
# must not pin the machine down.  Live + pooled page-locked bytes stay under this cap (a quarter of the host's memory unless
# SYNTHRAY_PINNED_MAX_BYTES says otherwise); beyond it the arrays are ordinary NumPy arrays again.
PINNED_MAX_BYTES = int(float(os.environ.get("SYNTHRAY_PINNED_MAX_BYTES", 0)) or _mem_total() // 4)


def _pinned_release(p, nbytes):
    _pinned_live[0] -= nbytes
    if lib is None:  # interpreter shutting down after the pool was emptied
        return
    if _pinned_held[0] + nbytes <= PINNED_POOL_BYTES:
        _pinned_free.setdefault(nbytes, []).append(p)
        _pinned_held[0] += nbytes
    else:
        lib.sr_host_free(p)


def pinned_empty(shape, dtype=np.float64):
    """np.empty(shape, dtype) over page-locked memory when the array is large: the GPU writes it at link speed (pageable
    memory: a third of that, and the copy holds the host thread).  An ordinary, writeable NumPy array for the caller;
    blocks are recycled between calls (allocating page-locked memory costs more than the copy it speeds up)."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    if nbytes < PINNED_MIN_BYTES or PINNED_RESULTS == "0":
        return np.empty(shape, dtype)
    _pinned_asked[nbytes] = _pinned_asked.get(nbytes, 0) + 1
    if PINNED_RESULTS == "auto" and _pinned_asked[nbytes] < 2 and not _pinned_free.get(nbytes):
        return np.empty(shape, dtype)
    blocks = _pinned_free.get(nbytes)
    if blocks:
        p = blocks.pop()
        _pinned_held[0] -= nbytes
    else:
        if _pinned_live[0] + _pinned_held[0] + nbytes > PINNED_MAX_BYTES:  # the caller keeps its results: no more pinning
            return np.empty(shape, dtype)
        h = C.c_void_p()
        if lib.sr_host_alloc(C.byref(h), nbytes) != 0 or not h.value:  # no page-locked memory left: an ordinary array does
            return np.empty(shape, dtype)
        p = h.value
    _pinned_live[0] += nbytes
    return np.asarray(_PinnedBlock(p, nbytes, tuple(shape), dtype))


def _pinned_drain():
    """At exit: the pooled blocks go back before the library is unloaded (blocks still under live arrays are the process's
    to lose)."""
    for blocks in _pinned_free.values():
        while blocks:
            lib.sr_host_free(blocks.pop())
    _pinned_held[0] = 0


import atexit  # noqa: E402

atexit.register(_pinned_drain)


def trace(volume: Volume, s0, t_end, extent, *, row_order=ROWS_LEGACY, substeps=1, sort_rays=True,
          precision=DEFAULT_PRECISION, return_E=True, return_sf=True, dt=0.0):
    """ScalarDomain.solve / propagator.solve on host arrays: s0 (9,N) -> (sf, rf, Jf, stats).  A large bundle goes through
    in chunks on two streams (sr_trace), its result arrays page-locked: transfers run beside the trace."""
    s0 = f64(s0)
    if s0.ndim != 2 or s0.shape[0] != 9:
        raise ValueError(f"s0 must have shape (9, N), got {s0.shape}")
    N = s0.shape[1]
    sf = pinned_empty((9, N)) if return_sf else None
    rf = pinned_empty((4, N))
    Jf = pinned_empty((2, N), np.complex128) if return_E else None
    p = _trace_params(t_end, extent, volume.axis, row_order, substeps, sort_rays,
                      resolve_precision(precision, volume, resident=False, substeps=substeps), dt)
    st = _ffi.TraceStats()
    check(lib.sr_trace(volume._h, ptr(s0), N, C.byref(p), ptr(sf), ptr(rf), ptr(Jf), C.byref(st)))
    return sf, rf, Jf, TraceStats(st.ray_steps, st.fallback_rays, st.trace_kernel_ms, st.total_ms)


def ray_to_jones(sf, extent, probing_direction="z", row_order=ROWS_LEGACY, return_E=True):
    sf = f64(sf)
    N = sf.shape[1]
    rf = np.empty((4, N))
    Jf = np.empty((2, N), np.complex128) if return_E else None
    check(lib.sr_ray_to_jones(ptr(sf), N, float(extent), axis_index(probing_direction), row_order, ptr(rf), ptr(Jf)))
    return rf, Jf


class RayBundle:
    """Rays resident in HBM: upload once, trace, deposit on any number of detectors."""

    def __init__(self, n_rays: int):
        self.n = int(n_rays)
        self._h = C.c_void_p()
        self._volume, self.retraced = None, 0
        self.generation = 0              # counts every call that changes the rays: what a resident handle is checked against
        self.holders = weakref.WeakSet()  # diagnostics objects that deposit from this bundle (resident.attach)
        check(lib.sr_rays_create(C.byref(self._h), self.n))

    @property
    def alive(self) -> bool:
        return bool(getattr(self, "_h", None))

    def upload(self, s0):
        s0 = f64(s0)
        if s0.shape != (9, self.n):
            raise ValueError(f"s0 must have shape (9, {self.n}), got {s0.shape}")
        self.generation += 1
        check(lib.sr_rays_upload(self._h, ptr(s0)))
        return self

    def upload_part(self, s0, first, last=False):
        """(9, n) host rays become rays first .. first + n - 1 of the bundle; last=True on the final part (sr_rays_upload_part:
        a bundle merged from several host chunks, each its own seeded draw)."""
        s0 = f64(s0)
        if s0.ndim != 2 or s0.shape[0] != 9 or first < 0 or first + s0.shape[1] > self.n:
            raise ValueError(f"part of shape {s0.shape} at ray {first} does not fit a bundle of {self.n} rays")
        self.generation += 1
        check(lib.sr_rays_upload_part(self._h, ptr(s0), int(s0.shape[1]), int(first), 1 if last else 0))
        return self

    def generate(self, beam_size, divergence, ne_extent, beam_type="circular", probing_direction="z", seed=0, first_ray=0,
                 radial_law="legacy"):
        """Draw the bundle on the device: init_beam's distributions from a Philox stream keyed by (seed, first_ray + ray
        index).  Not NumPy's sample (use init_beam + upload to reproduce the reference's seeded rays).  radial_law
        ('circular' only): "legacy" = u = U + U folded at 1 (full_solver.py:567-572), "power" = np.random.power(2) of the
        JAX generation's Beam (src/simulator/beam.py:66-77)."""
        if beam_type == "circular":
            if radial_law not in ("legacy", "power"):
                raise ValueError("radial_law must be 'legacy' or 'power'")
            kind, a, b = (0 if radial_law == "legacy" else 3), float(beam_size), 0.0
        elif beam_type == "linear":
            kind, a, b = 2, float(beam_size), 0.0
        elif beam_type == "square":
            kind, a, b = 1, float(beam_size), float(beam_size)
        elif beam_type == "rectangular":
            kind, a, b = 1, float(beam_size[0]), float(beam_size[1])
        else:
            raise ValueError(f"beam_type {beam_type!r}: 'circular', 'square', 'rectangular' or 'linear' on the device")
        self.generation += 1
        check(lib.sr_rays_generate(self._h, kind, a, b, float(divergence), float(ne_extent), axis_index(probing_direction),
                                   int(seed), int(first_ray)))
        return self

    def download_s0(self):
        """The bundle as generated / uploaded, (9, N)."""
        s0 = np.empty((9, self.n))
        check(lib.sr_rays_download_s0(self._h, ptr(s0)))
        return s0

    def trace(self, volume: Volume, t_end, extent, *, row_order=ROWS_LEGACY, substeps=1, sort_rays=True,
              precision=DEFAULT_PRECISION, dt=0.0, want_stats=True, handoff=0, resident=True) -> TraceStats:
        """handoff (slab volumes, A12): HANDOFF_ENTER takes the state from the hand-off records instead of s0,
        HANDOFF_EXIT leaves it in the records instead of writing sf / rf / Jf.  resident=False: the caller is going to
        download rf and bin it itself, so precision "auto" may not count on the deposit's edge guard (resolve_precision)."""
        p = _trace_params(t_end, extent, volume.axis, row_order, substeps, sort_rays,
                          resolve_precision(precision, volume, resident=resident, handoff=handoff, substeps=substeps), dt, handoff)
        st = _ffi.TraceStats()
        self._volume = volume  # an exact-counts deposit may trace some rays again: the volume lives as long as the bundle needs it
        self.generation += 1
        check(lib.sr_rays_trace(self._h, volume._h, C.byref(p), C.byref(st) if want_stats else None))
        return TraceStats(st.ray_steps, st.fallback_rays, st.trace_kernel_ms, st.total_ms)

    @property
    def tile_segments(self) -> int:
        """Node-plane segments of the tile path (trace_tile.inc) in the last trace of this bundle; 0: the per-ray kernels."""
        return int(lib.sr_rays_tile_segments(self._h))

    @property
    def tile_records(self) -> bool:
        """True when the last trace's tile path ran the records kernel (sr_rays_tile_records)."""
        return bool(lib.sr_rays_tile_records(self._h))

    def launch_order(self):
        """(N,) uint32: order[j] = index of the ray in launch slot j of the last trace (sr_rays_launch_order: the identity after
        sort_rays=False, the Morton / band order of the binning otherwise).  Waits for the stream; for tests of the binning."""
        out = np.empty(self.n, np.uint32)
        check(lib.sr_rays_launch_order(self._h, ptr(out)))
        return out

    def binned_cells(self):
        """(2, N) int64: the lateral cell (ib, ic) the tile path's last binning found for each ray, -1 for none
        (sr_rays_binned_cells: by ray index after a one-segment trace from s0).  Waits for the stream; for tests."""
        out = np.empty(self.n, np.uint32)
        check(lib.sr_rays_binned_cells(self._h, ptr(out)))
        cells = np.stack([out & 0xFFFF, out >> 16]).astype(np.int64)
        cells[:, out == 0xFFFFFFFF] = -1
        return cells

    def resize(self, n_rays: int):
        """The bundle holds n_rays <= its capacity (the count it was created with) from now on, in the same device buffers; what
        it held is forgotten: upload again (sr_rays_set_count)."""
        check(lib.sr_rays_set_count(self._h, int(n_rays)))
        self.n = int(n_rays)
        self.generation += 1
        return self

    @property
    def bbox(self):
        """(min x, y, z, max x, y, z) of the launch positions of the beam these rays belong to [m], or None: what the library
        judges the ray density by when it picks the kernel (sr_rays_get_bbox)."""
        box, known = np.zeros(6), C.c_int(0)
        check(lib.sr_rays_get_bbox(self._h, ptr(box), C.byref(known)))
        return box if known.value else None

    @bbox.setter
    def bbox(self, box):
        """Name the beam of rays that arrive by hand-off (ranks > 0 of a slab pipeline): stays with the bundle across
        hand-offs until the next upload / generate; None takes it back (sr_rays_set_bbox)."""
        check(lib.sr_rays_set_bbox(self._h, None if box is None else ptr(f64(np.asarray(box, dtype=np.float64).reshape(6)))))

    def error_bound(self):
        """(N,) float32: per ray, the bound [rad] on the exit-angle difference to the float64 build (sr_rays_error_bound)."""
        out = np.empty(self.n, np.float32)
        check(lib.sr_rays_error_bound(self._h, ptr(out)))
        return out

    def trace_stats(self) -> TraceStats:
        """Totals of every trace of this bundle since its counters were last read (traces run with want_stats=False
        queue their work and return; this waits for them).  Times are those of the last trace."""
        st = _ffi.TraceStats()
        check(lib.sr_rays_trace_stats(self._h, C.byref(st)))
        return TraceStats(st.ray_steps, st.fallback_rays, st.trace_kernel_ms, st.total_ms)

    def handoff_download(self):
        """(10, N) records in launch order: p_b, p_c, v_a, v_b, v_c, phase, t, amp, pol, ray index."""
        rec = np.empty((10, self.n))
        check(lib.sr_rays_handoff_download(self._h, ptr(rec)))
        return rec

    def handoff_upload(self, rec):
        rec = f64(rec)
        if rec.shape != (10, self.n):
            raise ValueError(f"records must have shape (10, {self.n}), got {rec.shape}")
        self.generation += 1
        check(lib.sr_rays_handoff_upload(self._h, ptr(rec)))
        return self

    def handoff_send(self, comm, peer):
        check(lib.sr_rays_handoff_send(self._h, comm, int(peer)))

    def handoff_recv(self, comm, peer):
        self.generation += 1
        check(lib.sr_rays_handoff_recv(self._h, comm, int(peer)))

    def download(self, sf=True, rf=True, Jf=True):
        a = pinned_empty((9, self.n)) if sf else None
        b = pinned_empty((4, self.n)) if rf else None
        e = pinned_empty((2, self.n), np.complex128) if Jf else None
        check(lib.sr_rays_download(self._h, ptr(a), ptr(b), ptr(e)))
        return a, b, e

    def deposit(self, image: "DetectorImage", ops, *, kwave=0.0, ref_beam=None, lds_tiles=True, want_stats=True,
                exact_counts=True):
        """m_to_mm -> [reference beam] -> chain -> image.  exact_counts (counts images of a mixed-precision trace): the
        edge guard of sr_deposit_params; `self.retraced` then holds how many rays it traced again in float64."""
        chain = make_chain(ops)
        p = deposit_params(kwave, ref_beam, lds_tiles, exact_counts)
        st = _ffi.DepositStats()
        check(lib.sr_rays_deposit(self._h, chain, len(ops), C.byref(p), image._h, C.byref(st) if want_stats else None))
        self.retraced = int(st.retraced)
        return st.kernel_ms, int(st.deposited)

    def deposit_intensity(self, image: "DetectorImage", ops, analysers, lds_tiles=True, want_stats=True):
        """m_to_mm -> chain (masks and geometry only) -> np.histogram2d's bin -> image[c] += |a_c . E|^2 per analyser channel
        (sr_rays_deposit_intensity; no reference counterpart).  analysers: angles in radians from the y axis in the sense
        `pol` is measured, None = no analyser (|E|^2); as many as the image has channels.  An incoherent sum: no reference
        beam, no field propagation (its factors have modulus 1).  No edge guard on a mixed-precision bundle
        (resolve_precision).  Returns (kernel_ms, deposited rays)."""
        ab = analyser_ab(analysers)
        st = _ffi.DepositStats()
        check(lib.sr_rays_deposit_intensity(self._h, make_chain(ops), len(ops), ptr(ab), len(ab), 1 if lds_tiles else 0, image._h,
                                            C.byref(st) if want_stats else None))
        return st.kernel_ms, int(st.deposited)

    def optics(self, ops=(), *, kwave=0.0, ref_beam=None, with_E=False):
        """The deposit's front end without the detector (sr_rays_optics): exit-plane rays -> m_to_mm -> [reference beams] ->
        chain, as HOST arrays in the original ray order: (r (4, N) mm, E (2, N) | None).  ops == (): r0 = m_to_mm(rf)."""
        ops = list(ops)
        r = pinned_empty((4, self.n))
        E = pinned_empty((2, self.n), np.complex128) if with_E else None
        p = deposit_params(kwave, ref_beam)
        check(lib.sr_rays_optics(self._h, make_chain(ops), len(ops), C.byref(p), ptr(r), ptr(E)))
        return r, E

    def refine(self, diagnostics, want_stats=True):
        """The exact-counts edge guard for several diagnostics at once: [(DetectorImage, ops), ...] (at most 4; complex images
        are ignored).  ONE float64 re-trace of every ray whose pixel or mask decision is uncertain for any of them; the
        deposits that follow then have nothing left to refine.  Returns the number of rays traced again (want_stats=False:
        queued without waiting, returns 0)."""
        diagnostics = list(diagnostics)
        n = len(diagnostics)
        if n == 0:
            return 0
        keep = [make_chain(ops) for _, ops in diagnostics]
        chains = (C.c_void_p * n)(*[C.cast(k, C.c_void_p) for k in keep])
        n_ops = (C.c_int * n)(*[len(ops) for _, ops in diagnostics])
        imgs = (C.c_void_p * n)(*[img._h for img, _ in diagnostics])
        again = C.c_int64(0)
        check(lib.sr_rays_refine(self._h, n, chains, n_ops, imgs, C.byref(again) if want_stats else None))
        self.retraced = int(again.value)
        return self.retraced

    def close(self):
        for img in self.__dict__.pop("_images", {}).values():  # the detectors resident.DeviceRays kept with the bundle
            img.close()
        if getattr(self, "_h", None):
            lib.sr_rays_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DetectorImage:
    """A detector image in HBM.  kind IMG_COUNTS: nx, ny are bins (A9); IMG_COMPLEX: edges (A10); IMG_INTENSITY: bins, and
    n_channels float64 planes (polarimetry)."""

    def __init__(self, kind, nx, ny, x_lo, x_hi, y_lo, y_hi, n_channels=0):
        self.kind, self.nx, self.ny = kind, int(nx), int(ny)
        self.n_channels = int(n_channels) if kind == IMG_INTENSITY else 0
        self.range = (float(x_lo), float(x_hi), float(y_lo), float(y_hi))
        self._h = C.c_void_p()
        if kind == IMG_INTENSITY:
            check(lib.sr_image_create_intensity(C.byref(self._h), self.n_channels, self.nx, self.ny, *self.range))
        else:
            check(lib.sr_image_create(C.byref(self._h), kind, self.nx, self.ny, *self.range))

    @classmethod
    def counts(cls, bin_scale=1, pix_x=3448, pix_y=2574, Lx=18.0, Ly=13.5):
        """Detector of Rays.histogram (rtm_solver.py:156-178; KAF-8300 defaults)."""
        return cls(IMG_COUNTS, pix_x // bin_scale, pix_y // bin_scale, -Lx / 2, Lx / 2, -Ly / 2, Ly / 2)

    @classmethod
    def complex_field(cls, bin_scale=1, pix_x=3448, pix_y=2574, Lx=18.0, Ly=13.5):
        """Detector of Interferometry.interferogram: edges linspace(-L//2, L//2, pix//bin_scale) — floor
        division as written in the reference (rtm_solver.py:436-437): x in [-9, 9], y in [-7, 6] for the defaults."""
        return cls(IMG_COMPLEX, pix_x // bin_scale, pix_y // bin_scale, -Lx // 2, Lx // 2, -Ly // 2, Ly // 2)

    @classmethod
    def intensity(cls, n_channels=1, bin_scale=1, pix_x=3448, pix_y=2574, Lx=18.0, Ly=13.5):
        """n_channels analyser-weighted intensity planes on the detector of Rays.histogram (np.histogram2d's binning);
        download() gives (n_channels, ny, nx) float64.  No reference counterpart."""
        return cls(IMG_INTENSITY, pix_x // bin_scale, pix_y // bin_scale, -Lx / 2, Lx / 2, -Ly / 2, Ly / 2, n_channels=n_channels)

    def zero(self):
        check(lib.sr_image_zero(self._h))

    def rotation(self, ch_plus, ch_minus, beta):
        """IMG_INTENSITY: the rotation map alpha [ny][nx] of two channels whose analysers stand at +beta and -beta
        (rotation_map's formula, evaluated on the device: sr_image_rotation); NaN where both channels are empty."""
        a = pinned_empty((self.ny, self.nx))
        check(lib.sr_image_rotation(self._h, int(ch_plus), int(ch_minus), float(beta), ptr(a)))
        return a

    def download(self):
        if self.kind == IMG_COUNTS:
            H = np.empty((self.ny, self.nx), np.uint32)
        elif self.kind == IMG_INTENSITY:
            H = np.empty((self.n_channels, self.ny, self.nx))
        else:
            H = np.empty((2, self.ny - 1, self.nx - 1), np.complex128)
        check(lib.sr_image_download(self._h, ptr(H)))
        return H

    def counts_f64(self):
        """IMG_COUNTS as float64 [ny][nx], np.histogram2d's dtype (rtm_solver.py:171-174): converted on the device."""
        H = pinned_empty((self.ny, self.nx))
        check(lib.sr_image_counts_f64(self._h, ptr(H)))
        return H

    def amplitude(self):
        """IMG_COMPLEX: H = sqrt(Re(Ax)^2 + Re(Ay)^2) (rtm_solver.py:450)."""
        H = pinned_empty((self.ny - 1, self.nx - 1))
        check(lib.sr_image_amplitude(self._h, ptr(H)))
        return H

    @property
    def nbytes(self) -> int:
        return int(lib.sr_image_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib.sr_image_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- host-buffer entry points (A7-A11) --------------------------------------------------
def optics(r_mm, ops, E=None, kwave=0.0):
    """Apply an optic chain to r (4,N) in mm; returns (r_out, E_out)."""
    r = f64(r_mm)
    if r.ndim != 2 or r.shape[0] != 4:
        raise ValueError(f"rays must have shape (4, N), got {r.shape}")
    N = r.shape[1]
    ro = pinned_empty(r.shape)  # page-locked when large and asked for before (pinned_empty): the next step's upload is fast too
    Ei = None if E is None else np.ascontiguousarray(E, dtype=np.complex128)
    Eo = None if E is None else pinned_empty(Ei.shape, np.complex128)
    check(lib.sr_optics(make_chain(ops), len(ops), float(kwave), N, ptr(r), ptr(Ei), ptr(ro), ptr(Eo)))
    return ro, Eo


def hist2d(x, y, nxb, nyb, xlo, xhi, ylo, yhi):
    """np.histogram2d(x, y, bins=[nxb, nyb], range=...)[0].T as exact integer counts."""
    x, y = f64(x), f64(y)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("x and y must be 1-D arrays of equal length")
    H = np.empty((int(nyb), int(nxb)), np.uint32)
    check(lib.sr_hist2d(ptr(x), ptr(y), len(x), int(nxb), int(nyb), float(xlo), float(xhi), float(ylo), float(yhi), ptr(H)))
    return H


def analyser_ab(analysers):
    """[n_ch][2] float64 (a, b) = (-sin beta, cos beta) per analyser angle beta [rad], (NaN, NaN) for None (no analyser):
    formed once here, in float64, so that the host and the device work with the same two numbers."""
    if analysers is None or np.isscalar(analysers):
        analysers = [analysers]
    analysers = list(analysers)
    if not 1 <= len(analysers) <= _ffi.MAX_ANALYSERS:
        raise ValueError(f"1 to {_ffi.MAX_ANALYSERS} analyser channels per image, got {len(analysers)}")
    ab = np.empty((len(analysers), 2))
    for c, beta in enumerate(analysers):
        ab[c] = (np.nan, np.nan) if beta is None else (-np.sin(float(beta)), np.cos(float(beta)))
    return ab


def intensity2d(x, y, E, analysers, nxb, nyb, xlo, xhi, ylo, yhi):
    """I[c] = np.histogram2d(x, y, bins=[nxb, nyb], range=..., weights=|a_c . E|^2)[0].T per analyser channel, (n_ch, nyb,
    nxb) float64 (sr_intensity2d: the host-array form of RayBundle.deposit_intensity; no reference counterpart)."""
    x, y = f64(x), f64(y)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("x and y must be 1-D arrays of equal length")
    E = np.ascontiguousarray(E, dtype=np.complex128)
    if E.shape != (2, len(x)):
        raise ValueError(f"E must have shape (2, {len(x)}), got {E.shape}")
    ab = analyser_ab(analysers)
    out = np.empty((len(ab), int(nyb), int(nxb)))
    check(lib.sr_intensity2d(ptr(x), ptr(y), ptr(E), len(x), ptr(ab), len(ab), int(nxb), int(nyb), float(xlo), float(xhi),
                             float(ylo), float(yhi), ptr(out)))
    return out


def rotation_map(I_plus, I_minus, beta):
    """The polarisation rotation alpha from two intensity images taken through analysers at +beta and -beta, 0 < beta < pi/2
    (I = A^2 cos^2(alpha -+ beta)):  D = (I+ - I-)/(I+ + I-), R = hypot(sin 2beta, D cos 2beta),
    delta = atan2(D cos 2beta, sin 2beta), alpha = (delta + asin(D/R))/2; NaN where I+ + I- == 0.  Unambiguous for
    |alpha| < min(beta, pi/2 - beta); beta = pi/4 gives alpha = asin(D)/2.  Host NumPy: the formula DetectorImage.rotation
    evaluates on the device (sr_image_rotation), for images that are already on the host."""
    if not 0 < beta < np.pi / 2:
        raise ValueError("beta must lie in (0, pi/2)")
    Ip, Im = np.asarray(I_plus, dtype=np.float64), np.asarray(I_minus, dtype=np.float64)
    tot = Ip + Im
    with np.errstate(divide="ignore", invalid="ignore"):
        D = np.where(tot == 0, np.nan, (Ip - Im) / tot)
        s2, dc = np.sin(2 * beta), D * np.cos(2 * beta)
        return 0.5 * (np.arctan2(dc, s2) + np.arcsin(np.clip(D / np.hypot(s2, dc), -1.0, 1.0)))


def interferogram(x, y, E, nxe, nye, xlo, xhi, ylo, yhi, sums=False):
    """Interferometry.interferogram (rtm_solver.py:424-453): H = sqrt(Re(sum E_x)^2 + Re(sum E_y)^2),
    shape (nye-1, nxe-1); with sums=True also the per-pixel complex sums (2, nye-1, nxe-1)."""
    x, y = f64(x), f64(y)
    E = np.ascontiguousarray(E, dtype=np.complex128)
    if E.shape != (2, len(x)):
        raise ValueError(f"E must have shape (2, {len(x)}), got {E.shape}")
    amp = np.empty((2, int(nye) - 1, int(nxe) - 1), np.complex128) if sums else None
    H = np.empty((int(nye) - 1, int(nxe) - 1))
    check(lib.sr_interferogram(ptr(x), ptr(y), ptr(E), len(x), int(nxe), int(nye), float(xlo), float(xhi), float(ylo),
                               float(yhi), ptr(amp), ptr(H)))
    return (H, amp) if sums else H


def interfere_ref_beam(x, y, E, n_fringes, deg):
    x, y = f64(x), f64(y)
    Eo = np.array(E, dtype=np.complex128, order="C", copy=True)
    check(lib.sr_interfere_ref_beam(ptr(x), ptr(y), len(x), float(n_fringes), float(deg), ptr(Eo)))
    return Eo


# ---- the reference's fixed optic chains (A8) --------------------------------------------
def chain_shadow_single(L=400.0, R=25.0, focal_plane=0.0):
    """Shadowgraphy.single_lens_solve (rtm_solver.py:197-203; diagnostics.py:388-394)."""
    return [(OP_DIST, 3 * L / 4 - focal_plane), (OP_CIRC_AP, R), (OP_LENS, L / 2, L / 2), (OP_DIST, 3 * L / 2)]


def chain_shadow_two(L=400.0, R=25.0, focal_plane=0.0):
    """Shadowgraphy.two_lens_solve (rtm_solver.py:205-214; diagnostics.py:396-405) and the optics of
    Interferometry.two_lens_solve (rtm_solver.py:376-422)."""
    return [(OP_DIST, L - focal_plane), (OP_CIRC_AP, R), (OP_LENS, L / 2, L / 2), (OP_DIST, L * 2), (OP_CIRC_AP, R),
            (OP_LENS, L / 2, L / 2), (OP_DIST, L)]


def chain_shadow_exp(L=400.0, R=25.0, detL=400.0):
    """Shadowgraphy.single_exp_solve (rtm_solver.py:216-222)."""
    return [(OP_DIST, L), (OP_CIRC_AP, R), (OP_LENS, L / 2, L / 2), (OP_DIST, detL)]


def chain_schlieren(L=400.0, R=25.0, focal_plane=0.0, stop_R=1.0, dark_field=True):
    """Schlieren.DF_solve / LF_solve (rtm_solver.py:231-267; diagnostics.py:415-458)."""
    return [(OP_DIST, L - focal_plane), (OP_CIRC_AP, R), (OP_LENS, L, L), (OP_DIST, L),
            (OP_CIRC_STOP if dark_field else OP_CIRC_AP, stop_R), (OP_DIST, L), (OP_CIRC_AP, R), (OP_LENS, L, L),
            (OP_DIST, L)]


def chain_refractometry(L=400.0, R=25.0, focal_plane=0.0):
    """Refractometry.incoherent_solve (rtm_solver.py:276-286; diagnostics.py:467-481)."""
    return [(OP_DIST, 3 * L / 4 - focal_plane), (OP_CIRC_AP, R), (OP_LENS, L / 2, L / 2), (OP_DIST, 3 * L / 2),
            (OP_RECT_AP, 15, 30), (OP_CIRC_AP, R), (OP_LENS, L / 3, L / 2), (OP_DIST, L)]


def chain_refractometry_coherent(L=400.0, R=25.0, focal_plane=0.0, as_written_jax=False):
    """Refractometry.coherent_solve: use with E and kwave = 2*pi/wavelength.  Both generations are reproduced as
    written.  Legacy (rtm_solver.py:288-331): travel, aperture, lens, travel, aperture, hybrid lens, travel, where the
    field factor of the middle leg is computed between the aperture's output and input (:311-313) and is therefore 1.
    JAX file (diagnostics.py:505-524): the first aperture is applied to r0 and the chain carries on from there, so the
    first travel only contributes its field factor; the middle leg's factor is applied."""
    first, mid_flag = (OP_PHASE, 0) if as_written_jax else (OP_DIST, 1)
    return [(first, 3 * L / 4 - focal_plane), (OP_CIRC_AP, R), (OP_LENS, L / 2, L / 2), (OP_DIST, 3 * L / 2, 0.0, mid_flag),
            (OP_CIRC_AP, R), (OP_LENS, L / 3, L / 2), (OP_DIST, L)]


def slab_cuts(n_planes, n_slabs):
    """Node-plane ranges [(k_lo, k_hi), ...] of n_slabs slabs that share their boundary planes and cover 0..n_planes-1."""
    n_slabs = max(1, min(int(n_slabs), n_planes - 1))
    edges = [round(q * (n_planes - 1) / n_slabs) for q in range(n_slabs + 1)]
    return list(zip(edges[:-1], edges[1:]))


def slab_source(ne, axis, k_lo, k_hi):
    """The part of a whole-domain array a slab is built from: planes max(k_lo-1, 0)..min(k_hi+1, n-1) along `axis`."""
    n = ne.shape[axis]
    sl = [slice(None)] * 3
    sl[axis] = slice(max(k_lo - 1, 0), min(k_hi + 1, n - 1) + 1)
    return np.ascontiguousarray(ne[tuple(sl)])
