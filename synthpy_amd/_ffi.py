"""ctypes binding of libsynthray.so (include/synthray.h).

The library is the product: there is no NumPy or CPU fallback behind it.  If it has
not been built, importing this module raises; if no MI355X is visible, the first
call that needs the device raises RuntimeError with the HIP error text.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SYNTHRAY_LIB") or os.path.join(_HERE, "libsynthray.so")  # override: A/B builds of the kernels


class SynthrayError(RuntimeError):
    """A libsynthray call returned a negative status."""


class Optic(C.Structure):
    _fields_ = [("op", C.c_int32), ("iarg", C.c_int32), ("a", C.c_double), ("b", C.c_double)]


class TraceParams(C.Structure):
    _fields_ = [("t_end", C.c_double), ("extent", C.c_double), ("dt", C.c_double), ("probing_axis", C.c_int32),
                ("row_order", C.c_int32), ("substeps", C.c_int32), ("sort_rays", C.c_int32), ("precision", C.c_int32),
                ("handoff", C.c_int32)]


class TraceStats(C.Structure):
    _fields_ = [("ray_steps", C.c_int64), ("fallback_rays", C.c_int64), ("trace_kernel_ms", C.c_double),
                ("total_ms", C.c_double)]


class FresnelParams(C.Structure):
    _fields_ = [("pi_lz", C.c_double), ("psf", C.c_double), ("post_re", C.c_double), ("post_im", C.c_double),
                ("r0", C.c_int32), ("nr", C.c_int32), ("c0", C.c_int32), ("nc", C.c_int32)]


FRESNEL_STATS = 6  # SR_FRESNEL_STATS

MAX_REF_BEAMS = 4  # SR_MAX_REF_BEAMS
MAX_ANALYSERS = 4  # SR_MAX_ANALYSERS
PROJ_GRAD1, PROJ_GRAD2, PROJ_NM1, PROJ_NE, PROJ_KAPPA, PROJ_NEB, PROJ_MAPS = range(7)  # SR_PROJ_*


class DepositParams(C.Structure):
    _fields_ = [("kwave", C.c_double), ("ref_n_fringes", C.c_double * MAX_REF_BEAMS), ("ref_deg", C.c_double * MAX_REF_BEAMS),
                ("ref_on", C.c_int32), ("lds_tiles", C.c_int32), ("exact_counts", C.c_int32), ("reserved", C.c_int32)]


class ResampleParams(C.Structure):
    _fields_ = [("M", C.c_double * 9), ("t", C.c_double * 3), ("V", C.c_double * 9), ("fill", C.c_double * 3),
                ("use_V", C.c_int32), ("reserved", C.c_int32)]


MAX_BANDS = 4  # SR_MAX_BANDS


class EmissionParams(C.Structure):
    _fields_ = [("axis", C.c_int32), ("toward", C.c_int32), ("n_band", C.c_int32), ("reserved", C.c_int32),
                ("omega", C.c_double * MAX_BANDS), ("e_ph", C.c_double * MAX_BANDS), ("c_omega", C.c_double * MAX_BANDS),
                ("Te", C.c_double), ("Z", C.c_double)]


class EmissionTable(C.Structure):
    _fields_ = [("nT", C.c_int32), ("nD", C.c_int32), ("LT", C.c_void_p), ("LD", C.c_void_p), ("LA", C.c_void_p),
                ("LE", C.c_void_p), ("m_ion", C.c_double)]


class SightlineParams(C.Structure):
    _fields_ = [("toward", C.c_int32), ("n_band", C.c_int32), ("max_steps", C.c_int32), ("reserved", C.c_int32),
                ("step", C.c_double), ("omega", C.c_double * MAX_BANDS), ("e_ph", C.c_double * MAX_BANDS),
                ("c_omega", C.c_double * MAX_BANDS), ("Te", C.c_double), ("Z", C.c_double)]


MAX_FREQS = 16384  # SR_MAX_FREQS


class SpectraParams(C.Structure):
    _fields_ = [("toward", C.c_int32), ("max_steps", C.c_int32), ("step", C.c_double), ("Te", C.c_double), ("Z", C.c_double)]


MAX_LINES = 32  # SR_MAX_LINES


class LineTable(C.Structure):
    _fields_ = [("nT", C.c_int32), ("nD", C.c_int32), ("n_line", C.c_int32), ("reserved", C.c_int32), ("LT", C.c_void_p),
                ("LD", C.c_void_p), ("w0", C.c_void_p), ("A", C.c_void_p), ("LJ", C.c_void_p), ("LK", C.c_void_p)]


class LinesParams(C.Structure):
    _fields_ = [("toward", C.c_int32), ("max_steps", C.c_int32), ("continuum", C.c_int32), ("reserved", C.c_int32),
                ("step", C.c_double), ("Te", C.c_double), ("Z", C.c_double)]


class VoigtTable(C.Structure):
    _fields_ = [("lines", LineTable), ("LG", C.c_void_p)]


class VoigtParams(C.Structure):
    _fields_ = [("march", LinesParams), ("wing", C.c_double)]


MAX_ZEEMAN = 24  # SR_MAX_ZEEMAN


class ZeemanTable(C.Structure):
    _fields_ = [("voigt", VoigtTable), ("n_comp", C.c_void_p), ("comp", C.c_void_p)]


class PushParams(C.Structure):
    _fields_ = [("qm", C.c_double), ("dt", C.c_double), ("max_steps", C.c_int32), ("axis", C.c_int32),
                ("det_pos", C.c_double), ("hit_scale", C.c_double)]


class PushStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("finished", C.c_int64), ("unfinished", C.c_int64), ("missed", C.c_int64),
                ("deposited", C.c_int64)]


PUSH_UNFINISHED, PUSH_MISSED = 1, 2  # SR_PUSH_*


class PushMatterParams(C.Structure):
    _fields_ = [("push", PushParams), ("mass", C.c_double), ("z", C.c_double), ("Zn", C.c_double), ("I", C.c_double),
                ("lnLs", C.c_double), ("Z", C.c_double), ("stop_energy", C.c_double)]


class PushMatterStats(C.Structure):
    _fields_ = PushStats._fields_ + [("stopped", C.c_int64)]


PUSH_STOPPED = 4  # SR_PUSH_STOPPED


class ThomsonParams(C.Structure):
    _fields_ = [("lambda_i", C.c_double), ("A", C.c_double), ("Z", C.c_double)]


MAX_SPECIES = 4  # SR_MAX_SPECIES


class ThomsonMultiParams(C.Structure):
    _fields_ = [("lambda_i", C.c_double), ("n_species", C.c_int32), ("reserved", C.c_int32), ("A", C.c_double * MAX_SPECIES),
                ("Z", C.c_double * MAX_SPECIES), ("frac", C.c_double * MAX_SPECIES)]


class ThomsonSgParams(C.Structure):
    _fields_ = ThomsonMultiParams._fields_ + [("order", C.c_double)]


class WaveParams(C.Structure):
    _fields_ = [("axis", C.c_int32), ("toward", C.c_int32), ("mu", C.c_int32), ("mv", C.c_int32), ("u0", C.c_double),
                ("du", C.c_double), ("v0", C.c_double), ("dv", C.c_double), ("lambda_", C.c_double), ("omega", C.c_double),
                ("k0", C.c_double), ("pi_l", C.c_double), ("Z", C.c_double), ("time_parts", C.c_int32), ("reserved", C.c_int32)]


WAVE_APERTURE, WAVE_STOP, WAVE_KNIFE = 1, 2, 4  # SR_WAVE_*


class WaveImageParams(C.Structure):
    _fields_ = [("mu", C.c_int32), ("mv", C.c_int32), ("flags", C.c_int32), ("knife_axis", C.c_int32), ("pi_l", C.c_double),
                ("defocus", C.c_double), ("lf", C.c_double), ("Ra", C.c_double), ("Rs", C.c_double), ("knife_offset", C.c_double),
                ("knife_dir", C.c_double)]


class DepositStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("deposited", C.c_int64), ("retraced", C.c_int64)]


# every symbol include/synthray.h declares: name -> (restype, argtypes)
_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_pp = C.POINTER(C.c_void_p)
SYMBOLS = {
    "sr_init": (_i, [_i]),
    "sr_device_count": (_i, []),
    "sr_synchronize": (_i, []),
    "sr_device_memory": (_i, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sr_grid_cus": (_i, [_i, C.POINTER(C.c_int)]),
    "sr_grid_stats": (_i, [C.POINTER(C.c_int64), _i]),
    "sr_last_error": (C.c_char_p, []),
    "sr_version": (C.c_char_p, []),
    "sr_stream_select": (_i, [_i]),
    "sr_stream_wait": (_i, [_i, _i]),
    "sr_host_alloc": (_i, [_pp, C.c_size_t]),
    "sr_host_free": (None, [_vp]),
    "sr_alloc_probe": (_i, [C.c_size_t, _vp, _vp]),
    "sr_volume_create": (_i, [_pp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _d, _i, _i]),
    "sr_volume_create_from_fields": (_i, [_pp, _vp, _vp, _vp, _vp, _d, _i, _i, _i, _vp, _vp, _vp, _i]),
    "sr_volume_fields": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "sr_field_ifft_real": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "sr_field_modesum": (_i, [_i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "sr_radial_spectrum2d": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "sr_power_spectrum": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _d, _vp, _vp, _vp]),
    "sr_fresnel_grid": (_i, [_i64, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "sr_fresnel_propagate": (_i, [_vp, _i, _i, _vp, _vp, C.POINTER(FresnelParams), _vp]),
    "sr_fresnel_rays": (_i, [_i64, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp,
                             C.POINTER(FresnelParams), _vp, _vp]),
    "sr_volume_sample": (_i, [_vp, _vp, _i64, _vp]),
    "sr_volume_attach_aux": (_i, [_vp, _vp, _vp, _vp, _d]),
    "sr_volume_create_slab": (_i, [_pp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _d, _i, _i, _i, _i]),
    "sr_rays_handoff_download": (_i, [_vp, _vp]),
    "sr_rays_handoff_upload": (_i, [_vp, _vp]),
    "sr_rays_handoff_send": (_i, [_vp, _vp, _i]),
    "sr_rays_handoff_recv": (_i, [_vp, _vp, _i]),
    "sr_volume_sample_aux": (_i, [_vp, _vp, _i64, _vp]),
    "sr_volume_project": (_i, [_vp, _vp, C.POINTER(C.c_uint32)]),
    "sr_volume_omega": (_d, [_vp]),
    "sr_volume_bytes": (_i64, [_vp]),
    "sr_volume_destroy": (None, [_vp]),
    "sr_field_create": (_i, [_pp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sr_field_resample": (_i, [_vp, C.POINTER(ResampleParams), _i, _i, _i, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_field_emission": (_i, [_vp, _vp, _vp, C.POINTER(EmissionParams), _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_field_emission_table": (_i, [_vp, _vp, _vp, C.POINTER(EmissionTable), C.POINTER(EmissionParams), _vp, _vp, _vp,
                                     C.POINTER(C.c_double)]),
    "sr_field_sightlines": (_i, [_vp, _vp, _vp, C.POINTER(EmissionTable), C.POINTER(SightlineParams), _i64, _vp, _vp, _vp, _vp, _vp,
                                 _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_field_sightline_spectra": (_i, [_vp, _vp, _vp, C.POINTER(EmissionTable), C.POINTER(SpectraParams), _i64, _vp, _vp, C.c_int32,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_lines_chunk": (_i, []),
    "sr_field_sightline_lines": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(LineTable), C.POINTER(LinesParams), _i64, _vp, _vp, C.c_int32,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_voigt_chunk": (_i, []),
    "sr_field_sightline_voigt": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(VoigtTable), C.POINTER(VoigtParams), _i64, _vp, _vp, C.c_int32,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_zeeman_chunk": (_i, []),
    "sr_field_sightline_zeeman": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ZeemanTable), C.POINTER(VoigtParams), _i64, _vp, _vp, _vp,
                                       C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_stokes_chunk": (_i, []),
    "sr_field_sightline_stokes": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ZeemanTable), C.POINTER(VoigtParams), _i64, _vp, _vp, _vp,
                                       C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       C.POINTER(C.c_double)]),
    "sr_particles_push": (_i, [_vp, _vp, C.POINTER(PushParams), _i64, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(PushStats)]),
    "sr_particles_push_matter": (_i, [_vp, _vp, _vp, _vp, C.POINTER(PushMatterParams), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      C.POINTER(PushMatterStats)]),
    "sr_field_thomson": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(ThomsonParams), _i64, C.c_int32, _vp, _vp, _vp, _vp, C.c_int32,
                              _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_field_thomson_multi": (_i, [_vp, _vp, _vp, _vp, _vp, _pp, _pp, C.POINTER(ThomsonMultiParams), _i64, C.c_int32, _vp, _vp, _vp,
                                    _vp, C.c_int32, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_field_thomson_sg": (_i, [_vp, _vp, _vp, _vp, _vp, _pp, _pp, _vp, C.POINTER(ThomsonSgParams), _i64, C.c_int32, _vp, _vp, _vp,
                                 _vp, C.c_int32, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_field_wave": (_i, [_vp, _vp, _vp, C.POINTER(WaveParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sr_wave_image": (_i, [C.POINTER(WaveImageParams), _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "sr_field_bytes": (_i64, [_vp]),
    "sr_field_destroy": (None, [_vp]),
    "sr_trace": (_i, [_vp, _vp, _i64, C.POINTER(TraceParams), _vp, _vp, _vp, C.POINTER(TraceStats)]),
    "sr_ray_to_jones": (_i, [_vp, _i64, _d, _i, _i, _vp, _vp]),
    "sr_rays_create": (_i, [_pp, _i64]),
    "sr_rays_download_s0": (_i, [_vp, _vp]),
    "sr_rays_error_bound": (_i, [_vp, _vp]),
    "sr_rays_generate": (_i, [_vp, _i, _d, _d, _d, _d, _i, C.c_uint64, C.c_uint64]),
    "sr_rays_upload": (_i, [_vp, _vp]),
    "sr_rays_upload_part": (_i, [_vp, _vp, _i64, _i64, _i]),
    "sr_rays_trace": (_i, [_vp, _vp, C.POINTER(TraceParams), C.POINTER(TraceStats)]),
    "sr_release_caches": (_i, []),
    "sr_rays_trace_stats": (_i, [_vp, C.POINTER(TraceStats)]),
    "sr_rays_tile_segments": (_i, [_vp]),
    "sr_tile_min_density": (_d, []),
    "sr_rays_tile_records": (_i, [_vp]),
    "sr_rays_launch_order": (_i, [_vp, _vp]),
    "sr_rays_binned_cells": (_i, [_vp, _vp]),
    "sr_rays_set_count": (_i, [_vp, _i64]),
    "sr_rays_set_bbox": (_i, [_vp, _vp]),
    "sr_rays_get_bbox": (_i, [_vp, _vp, C.POINTER(C.c_int)]),
    "sr_rays_download": (_i, [_vp, _vp, _vp, _vp]),
    "sr_rays_count": (_i64, [_vp]),
    "sr_rays_destroy": (None, [_vp]),
    "sr_optics": (_i, [C.POINTER(Optic), _i, _d, _i64, _vp, _vp, _vp, _vp]),
    "sr_hist2d": (_i, [_vp, _vp, _i64, _i, _i, _d, _d, _d, _d, _vp]),
    "sr_interferogram": (_i, [_vp, _vp, _vp, _i64, _i, _i, _d, _d, _d, _d, _vp, _vp]),
    "sr_interfere_ref_beam": (_i, [_vp, _vp, _i64, _d, _d, _vp]),
    "sr_image_create": (_i, [_pp, _i, _i, _i, _d, _d, _d, _d]),
    "sr_image_zero": (_i, [_vp]),
    "sr_image_download": (_i, [_vp, _vp]),
    "sr_image_amplitude": (_i, [_vp, _vp]),
    "sr_image_counts_f64": (_i, [_vp, _vp]),
    "sr_rays_optics": (_i, [_vp, C.POINTER(Optic), _i, C.POINTER(DepositParams), _vp, _vp]),
    "sr_image_bytes": (_i64, [_vp]),
    "sr_image_destroy": (None, [_vp]),
    "sr_rays_deposit": (_i, [_vp, C.POINTER(Optic), _i, C.POINTER(DepositParams), _vp, C.POINTER(DepositStats)]),
    "sr_rays_refine": (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(C.c_int64)]),
    "sr_image_create_intensity": (_i, [_pp, _i, _i, _i, _d, _d, _d, _d]),
    "sr_rays_deposit_intensity": (_i, [_vp, C.POINTER(Optic), _i, _vp, _i, _i, _vp, C.POINTER(DepositStats)]),
    "sr_intensity2d": (_i, [_vp, _vp, _vp, _i64, _vp, _i, _i, _i, _d, _d, _d, _d, _vp]),
    "sr_image_rotation": (_i, [_vp, _i, _i, _d, _vp]),
    "sr_comm_unique_id": (_i, [_vp]),
    "sr_comm_create": (_i, [_pp, _vp, _i, _i]),
    "sr_image_reduce": (_i, [_vp, _vp, _i]),
    "sr_comm_ranks": (_i, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sr_comm_destroy": (None, [_vp]),
}

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: synthpy_amd has no CPU path. Build the HIP library first:\n"
        "    python -c 'import __graft_entry__ as g; g.build()'   (or: make -C synthpy_amd/csrc)")

# RCCL between processes (sr_comm_create, the slab hand-off) shares device buffers through dmabuf IPC; hosts whose driver has no
# legacy IPC fail in hipIpcGetMemHandle unless the runtime is told so BEFORE it starts.  A launcher that exported a value keeps it.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

lib = C.CDLL(LIB_PATH)
for _name, (_res, _args) in SYMBOLS.items():
    _fn = getattr(lib, _name)  # AttributeError here = header and library out of step
    _fn.restype = _res
    _fn.argtypes = _args

VOIGT_CHUNK = int(lib.sr_voigt_chunk())  # samples of a chord sr_field_sightline_voigt's kernel stages at a time
ZEEMAN_CHUNK = int(lib.sr_zeeman_chunk())  # and sr_field_sightline_zeeman's
STOKES_CHUNK = int(lib.sr_stokes_chunk())  # and sr_field_sightline_stokes'


def last_error() -> str:
    return lib.sr_last_error().decode("utf-8", "replace")


gpu_touched = False  # set by the first library call that goes through check(): from then on this process must not fork


def check(rc: int) -> None:
    global gpu_touched
    gpu_touched = True
    if rc != 0:
        raise SynthrayError(f"libsynthray error {rc}: {last_error()}")


def ptr(a):
    """Raw pointer of a C-contiguous NumPy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data_as(C.c_void_p)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)
