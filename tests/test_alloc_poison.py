"""No result may depend on what device memory held before a call: SYNTHRAY_ALLOC_FILL (common.hpp, include/synthray.h).

With the knob set every device buffer of the library, the WHOLE staging block of the selected stream at every hand-out and every
page-locked block of sr_host_alloc hold that byte before they are used.  Patterns: unset, 0xFF (NaN as a float or double, -1 as a
signed integer, the maximum of a counter) and 0x5A (finite garbage: 2.3e130 as a double, 1.5e16 as a float, 1.5e9 as a uint32).
Before each run engine.release_caches(), so that what the library keeps is allocated again under the pattern.  docs/ALLOCATIONS.md
names, site by site, who writes every element before it is read; the tests look for dependence on stale values, they are not
meant to make anything fault.

Liveness.  sr_alloc_probe returns the pattern from a fresh buffer and from the staging block, on both library streams and after a
staged entry has used the block: without it every other test here could pass on a knob that does nothing.

Tier A.  The seventeen staged field entries, each on the smallest configuration of its own test module that the module's "tested
inputs" test accepts (imported, with the module's cached restatement), in two carve layouts: every optional output and the
backlight asked for, and none of them (or, where an entry has no optional piece, its module's other size).  Required: (1) every
returned array bit-identical across the three patterns, compared as raw bytes so that NaN payloads count; (2) the 0xFF run passes
the module's own comparison against its restatement.  None of the seventeen entries sums through floating-point atomics (their
only atomics are integer counters), so all of them are held to both requirements.  The frequency-per-lane kernels run a frequency
count that leaves the last tile ragged at both lane widths (SYNTHRAY_SPECTRA_FL = 64 and 256).  One cross-entry case per family:
a larger call of ANOTHER entry first, unpoisoned, so that the kept block holds that entry's real data, then the entry under test:
the same bits as before.

Tier B.  Scenarios of the trace path run again as they stand (the existing test functions, called with the fixtures) under 0xFF
and 0x5A; and, where the outputs are deterministic, ray arrays, counts and step / fallback totals bit-equal between the unpoisoned
and the poisoned runs.

Nothing is masked: no output of these entries is documented as unspecified.
"""
import ctypes as C
import gc

import numpy as np
import pytest

from conftest import golden

import test_api_flow as taf
import test_deposit_layouts as tdl
import test_emission as em
import test_fresnel_layouts as tfl
import test_gpu_parity as tgp
import test_power_spectrum as tps
import test_projection as tp
import test_radiography as tr
import test_radiography_matter as trm
import test_ray_order as tro
import test_resample as rs
import test_sightline_lines as gl
import test_sightline_spectra as tsp
import test_sightline_stokes as sk
import test_sightline_voigt as vt
import test_sightline_zeeman as zt
import test_sightlines as ts
import test_table_emission as tab
import test_thomson as th
import test_thomson_multi as tm
import test_thomson_sg as tg
import test_wave as tw
from test_api_flow import c1, c1_oracle  # noqa: F401  (fixtures of the scenarios below)
from test_power_spectrum import ps  # noqa: F401
from test_ray_order import base  # noqa: F401

KNOB = "SYNTHRAY_ALLOC_FILL"
PATTERNS = (None, 0xFF, 0x5A)
_EXTRA = {}  # restatements this module needs beside the ones its siblings cache (no backlight), made once


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from synthpy_amd import _ffi

    return _ffi


@pytest.fixture(scope="module")
def eng():
    from synthpy_amd import engine

    engine.init(0)
    return engine


def _fill(monkeypatch, eng, pattern):
    """The knob for what follows (None: unset), and everything the library keeps given back, so that it is allocated again."""
    if pattern is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(pattern))
    eng.select_stream(0)
    eng.release_caches()
    # the page-locked result blocks too, and the engine's memory of which sizes it has seen ("a size is page-locked from its
    # second use": test_host_buffer_trace_in_pipelined_chunks_is_bit_identical counts on a first use, here and in its own module)
    gc.collect()
    eng._pinned_drain()
    eng._pinned_asked.clear()


def _arrays(out):
    """name -> ndarray of a result: a dict's arrays (and the integer fields of a stats object), or a tuple's by position."""
    if isinstance(out, dict):
        flat = {}
        for k, v in out.items():
            if isinstance(v, np.ndarray):
                flat[k] = v
            elif k == "stats":
                flat.update({f"stats.{n}": np.int64(getattr(v, n)) for n in ("unfinished", "finished", "missed", "deposited", "stopped")
                             if hasattr(v, n)})
        return flat
    return {str(k): np.asarray(v) for k, v in enumerate(out) if v is not None}


def _same_bits(a, b, what):
    """Every array of b has the bytes of a's: NaN payloads and signed zeros count."""
    a, b = _arrays(a), _arrays(b)
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        if a[k].tobytes() != b[k].tobytes():
            bad = np.nonzero(np.atleast_1d(a[k]).reshape(-1).view(np.uint8) != np.atleast_1d(b[k]).reshape(-1).view(np.uint8))[0]
            raise AssertionError(f"{what}: {k} differs in {bad.size} bytes, the first at byte {int(bad[0])} of {a[k].nbytes}")


# ================================================================ liveness
def _probe(built, n=4096):
    fresh, kept = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    built.check(built.lib.sr_alloc_probe(n, fresh.ctypes.data_as(C.c_void_p), kept.ctypes.data_as(C.c_void_p)))
    return fresh, kept


@pytest.mark.gpu
def test_the_knob_is_live(eng, built, monkeypatch):
    """0xA5 comes back from a fresh buffer and from the staging block, on both library streams, and from the staging block again
    after a staged entry (sr_field_resample) has left its output there; unset, the probe succeeds."""
    src, axes, out_axes, M, t, _ = rs._case1(np.float64)
    _fill(monkeypatch, eng, 0xA5)
    try:
        for stream in (0, 1):
            eng.select_stream(stream)
            for again in range(2):
                fresh, kept = _probe(built)
                assert np.all(fresh == 0xA5), (stream, again, "a fresh buffer", np.unique(fresh)[:4])
                assert np.all(kept == 0xA5), (stream, again, "the staging block", np.unique(kept)[:4])
                got = rs._resample(eng, src, axes, M, t, out_axes, fill=-7.25)  # the block now holds a resampled field
                assert np.isfinite(got).all()
        # sr_host_alloc: the page-locked block holds the byte too
        h = C.c_void_p()
        built.check(built.lib.sr_host_alloc(C.byref(h), 4096))
        try:
            assert bytes((C.c_ubyte * 4096).from_address(h.value)) == b"\xa5" * 4096
        finally:
            built.lib.sr_host_free(h)
    finally:
        eng.select_stream(0)
    _fill(monkeypatch, eng, None)
    _probe(built)
    monkeypatch.setenv(KNOB, "")  # empty counts as unset
    _probe(built)


# ================================================================ Tier A: the staged field entries
class _Entry:
    """One staged entry on its module's configuration: run(eng, layout) -> its arrays, check(out, layout) -> the module's own
    comparison against its restatement.  layouts: the two carve layouts."""
    layouts = ("all", "bare")
    env = {}


def _dark(key, make):
    if key not in _EXTRA:
        _EXTRA[key] = make()
    return _EXTRA[key]


class _Sightlines(_Entry):
    """sr_field_sightlines: the 63-line case on grid A (misses, a capped line, a one-sample line, an inside origin)."""

    def __init__(self, kind):
        self.kind, self.cfg, self.toward = kind, ts.CONFIGS[1], -1
        assert self.cfg[:2] == ("A", 63)

    def R(self):
        return ts._config(self.cfg, self.kind, self.toward, np.float64)

    def run(self, eng, layout):
        R = self.R()
        if layout == "all":
            return ts._run(eng, R, self.kind, self.toward)
        return ts._run(eng, R, self.kind, self.toward, want=("intensity", "optical_depth"), backlight=None)

    def check(self, out, layout):
        R, what = self.R(), f"sightlines {self.kind} {layout} under 0xFF"
        if layout == "all":
            ts._assert_inputs(R, self.kind, what)
            ts._assert_exact(out, R["ref"], what)
            ts._assert_close(out, R["ref"], what)
            miss = R["ref"]["miss"]
            assert np.array_equal(out["I"][:, miss], R["back"][:, miss]) and np.all(out["tau"][:, miss] == 0) and np.all(out["column"][miss] == 0)
        else:
            dark = _dark(("sightlines", self.kind), lambda: ts.restate(R["ne"], R["Te"], R["Z"], R["K"]["co"], R["o"], R["d"],
                                                                      ts._node_of(R, self.kind), self.toward, R["K"]["step"]))
            assert set(out) == {"intensity", "optical_depth", "I", "tau"}
            ts._assert_close(out, dark, what)


class _Spectra(_Entry):
    """sr_field_sightline_spectra: 257 frequencies (a ragged last tile at 64 and at 256 lanes) on 70 lines."""

    def __init__(self, fl):
        self.cfg, self.toward, self.env = tsp.CONFIGS[5], +1, {"SYNTHRAY_SPECTRA_FL": str(fl)}
        assert self.cfg[:2] == (257, 70)

    def R(self):
        return tsp._config(self.cfg, "nrl", self.toward, np.float64)

    def run(self, eng, layout):
        if layout == "all":
            return tsp._spectra(eng, self.R(), self.toward)
        return tsp._spectra(eng, self.R(), self.toward, want=("intensity", "optical_depth"), backlight=None)

    def check(self, out, layout):
        R, what = self.R(), f"sightline_spectra {self.env} {layout} under 0xFF"
        if layout == "all":
            tsp._assert_inputs(R, what)
            tsp._assert_exact(out, R["ref"], what)
            tsp._assert_close(out, R["ref"], what)
            miss = R["ref"]["miss"]
            assert np.array_equal(out["intensity"][miss], R["back"][miss]) and np.all(out["optical_depth"][miss] == 0)
        else:
            tsp._assert_close(out, _dark("spectra", lambda: tsp._restate(R, self.toward, backlight=None)), what)


class _LineFamily(_Entry):
    """sr_field_sightline_lines / _voigt / _zeeman / _stokes: the module's first case whose frequency count leaves the last tile
    ragged at both lane widths, on its six chords (misses, one sample, the cap)."""

    def __init__(self, mod, k, fl):
        self.mod, self.c, self.env = mod, mod.CASES[k], {"SYNTHRAY_SPECTRA_FL": str(fl)}
        assert self.c["nf"] % 64 and self.c["nf"] % 256 and self.c["view"] == "six", self.c
        self.maps = ("I", "tau") + (("Q", "U", "V") if mod in (zt, sk) else ())

    def run(self, eng, layout):
        R = self.mod._case(self.c)
        if layout == "all":
            return self.mod._run(eng, R)
        return self.mod._run(eng, R, want=("intensity", "optical_depth") + self.maps[2:], backlight=None)

    def check(self, out, layout):
        R, what = self.mod._case(self.c), f"{self.mod.__name__} {self.mod._id(self.c)} {self.env} {layout} under 0xFF"
        if layout == "all":
            self.mod._assert_exact(out, R["ref"], what)
            self.mod._assert_close(out, R["ref"], what)
            miss = R["ref"]["miss"]
            assert miss.any() and np.array_equal(out["I"][miss], R["back"][miss]) and not np.any(out["tau"][miss])
        else:
            dark = _dark((self.mod.__name__, self.c["k"]), lambda: self.mod._restate(R, backlight=None))
            self.mod._assert_close(out, dark, what)


class _Emission(_Entry):
    """sr_field_emission / sr_field_emission_table: three planes along x under 67 x 3 columns (a ragged last wavefront)."""

    def __init__(self, mod):
        self.mod, self.key, self.toward = mod, (0, 3, (67, 3)), -1

    def run(self, eng, layout):
        K, (axis, n, lateral) = self.mod._case(*self.key), self.key
        if self.mod is em:
            if layout == "all":
                return em._run(eng, K["ne"], K["Te"], K["Z"], K["co"], em.WAVELENGTHS, axis, self.toward, K["back"])
            return em._run(eng, K["ne"], K["Te"], K["Z"], K["co"], em.WAVELENGTHS[:1], axis, self.toward)
        if layout == "all":
            return tab._run(eng, K["ne"], K["Te"], K["Z"], K["co"], K["table"], axis, self.toward, K["back"])
        return tab._run(eng, K["ne"], K["Te"], K["Z"], K["co"], K["lte"], axis, self.toward)

    def check(self, out, layout):
        K, (axis, n, lateral) = self.mod._case(*self.key), self.key
        what = f"{self.mod.__name__} {self.key} {layout} under 0xFF"
        I, tau = out
        if layout == "all":
            ref = K["refs"][self.toward]
            assert I.shape == (4,) + lateral
        elif self.mod is em:
            one = tuple(v[:1] for v in K["bands"])
            ref = _dark(("emission",) + self.key, lambda: em.restate(K["ne"], K["Te"], K["Z"], K["co"][axis], one, axis, self.toward))
        else:
            ref = K["refs1"][self.toward]
        self.mod._assert_inputs(ref, what)
        assert np.all(np.isfinite(I)) and np.all(np.isfinite(tau))
        self.mod._assert_close(I, tau, ref, what)


class _Thomson(_Entry):
    """sr_field_thomson / _multi / _sg: float64 fields, every optional field given; the module's largest sizes (a point and a
    wavelength past the LDS chunk and the tile) and the other size of its repeated-call test."""

    def __init__(self, mod):
        self.mod = mod
        self.sizes = {"all": (130, 513), "bare": (65, 257)} if mod is tg else {"all": (65, 257), "bare": (3, 255)}
        self.config = "all fields" if mod is th else "f64 V Vd 4 fields"

    def run(self, eng, layout):
        nq, nl = self.sizes[layout]
        F = th._fields(eng, "float64", self.config) if self.mod is th else self.mod._upload(eng, self.config)
        try:
            return th._run(eng, F, nq, nl) if self.mod is th else self.mod._run(eng, F, self.config, nq, nl)
        finally:
            for f in (F.values() if self.mod is th else [F]):
                f.close()

    def check(self, out, layout):
        nq, nl = self.sizes[layout]
        P, w = out
        if self.mod is th:
            P_ref, w_ref, scale = th._reference("float64", self.config, nq, True)
            wts = th._geometry()[1]
            w_bound = 2 * (nq + 8) * th.U * np.sum(np.abs(wts[:, :nq]), axis=1) * float(np.max(th._plasma("float64")["ne"]))
        elif self.mod is tm:
            P_ref, w_ref, _, scale = tm._reference(self.config, nq)
            w_bound = tm._w_bound("float64", nq)
        else:
            P_ref, w_ref, _, scale = tg._reference(self.config)[nq]
            w_bound = tg._w_bound("float64", nq)
        ref, sc = P_ref[:, :nl], scale[:, :nl]
        assert P.shape == (5, nl) and w.shape == (5,) and np.all(np.isfinite(P)) and np.all(np.isfinite(w))
        floor = tg.UNDERFLOW if self.mod is tg else 0.0
        assert np.array_equal(np.abs(P) <= floor, np.abs(ref) <= floor) and np.array_equal(w == 0, w_ref == 0)
        assert np.all(P[4] == 0) and w[4] == 0 and w[0] > 0 and np.all(P[w_ref == 0] == 0)
        nz = np.abs(ref) > floor if self.mod is tg else sc > 0
        ratio = float(np.max(np.abs(P - ref)[nz] / (th.U * sc[nz])))
        print(f"{self.mod.__name__} {layout} under 0xFF: {ratio:.2f} of the allowed {self.mod.K_SAMPLE:g}")
        assert nz.any() and ratio <= self.mod.K_SAMPLE, ratio
        assert np.all(np.abs(w - w_ref) <= w_bound)


DET = dict(axis=2, det_pos=0.05, hit_scale=1024.0)
IMG = (32, 24, -8.0, 8.0, -6.0, 6.0)


class _Push(_Entry):
    """sr_particles_push: test_radiography's 1037 particles through E and B (float64).  all: one step, every output and a counts
    image; bare: 64 steps, the image and the totals alone."""

    def inputs(self):
        E, B = tr._fields(np.float64)
        return E, B, tr._particles()[0]

    def run(self, eng, layout):
        E, B, s0 = self.inputs()
        img = eng.DetectorImage(eng.IMG_COUNTS, *IMG)
        try:
            kw = dict(want=("sf", "hits", "steps", "flags")) if layout == "all" else dict(want=())
            out = tr._push(eng, E, B, s0, tr.QM_P, tr.DT, 1 if layout == "all" else 64, image=img, **DET, **kw)
            out["image"] = img.download()
            return out
        finally:
            img.close()

    def check(self, out, layout):
        E, B, s0 = self.inputs()
        st, H = out["stats"], out["image"]
        assert H.dtype == np.uint32 and st.deposited == int(H.sum()) and st.finished + st.unfinished == tr.N_PART
        if layout == "bare":
            _, _, rsteps, rflags = _dark("push 64", lambda: tr.restate(s0, E, B, tr.AX, tr.QM_P, tr.DT, 64, DET["axis"], DET["det_pos"], DET["hit_scale"]))
            assert set(out) == {"stats", "image"} and 0 < H.sum() <= int((rflags == 0).sum())
            assert st.unfinished == int((rflags & tr.UNFINISHED > 0).sum()) and st.missed == int((rflags & tr.MISSED > 0).sum())
            return
        ref = tr.restate_step(s0, E, B, tr.AX, tr.QM_P, tr.DT)
        inside = tr._inside(ref, tr.AX)
        _, flags = tr._detector(ref, DET["axis"], DET["det_pos"], DET["hit_scale"])
        flags = flags | np.where(inside, tr.UNFINISHED, 0).astype(np.uint8)
        assert np.array_equal(out["steps"], np.ones(tr.N_PART, np.int32)) and np.array_equal(out["flags"], flags)
        assert np.array_equal(np.isnan(out["sf"]), np.isnan(ref))
        assert (st.unfinished, st.finished, st.missed) == (int(inside.sum()), int((~inside).sum()), int((flags & tr.MISSED > 0).sum()))
        du, dx = tr._scales(s0, E, B, tr.QM_P, tr.DT)
        d = np.abs(np.where(~np.isnan(ref), out["sf"] - ref, 0.0))
        assert np.all(d[:3] <= dx) and np.all(d[3:] <= du)
        own_hits, _ = tr._detector(out["sf"], DET["axis"], DET["det_pos"], DET["hit_scale"])
        okh = np.isfinite(own_hits)
        assert np.array_equal(np.isnan(out["hits"]), np.isnan(own_hits)) and np.array_equal(np.isinf(out["hits"]), np.isinf(own_hits))
        with np.errstate(invalid="ignore"):
            assert np.all(np.abs(np.where(okh, out["hits"] - own_hits, 0.0)) <= 8 * tr.EPS * np.abs(np.where(okh, own_hits, 0.0)))
        good = out["flags"] == 0
        from synthpy_amd import engine

        assert np.array_equal(H, engine.hist2d(out["hits"][0, good], out["hits"][1, good], *IMG))


class _PushMatter(_Entry):
    """sr_particles_push_matter: the module's whole-path case (64 steps, weak E and B, matter, stop_energy 0.5 MeV), float64.  all:
    every output; bare: the totals and a counts image alone."""

    def run(self, eng, layout):
        K = trm._whole_case(np.float64)
        if layout == "all":
            return trm._push(eng, K["E"], K["B"], K["ne"], K["Z"], K["s0"], 64, stop=0.5 * trm.MEV)
        img = eng.DetectorImage(eng.IMG_COUNTS, *IMG)
        try:
            out = trm._push(eng, K["E"], K["B"], K["ne"], K["Z"], K["s0"], 64, stop=0.5 * trm.MEV, image=img, want=())
            out["image"] = img.download()
            return out
        finally:
            img.close()

    def check(self, out, layout):
        ref = trm._whole_case(np.float64)["ref"]
        st = out["stats"]
        if layout == "all":
            trm._assert_against(out, ref, 64, "push_matter, 64 steps, under 0xFF")
            assert st.stopped == int(((out["flags"] & trm.STOPPED) > 0).sum()) and st.finished + st.unfinished == trm.N_PART
            return
        border = ref["bounds"]["border"]
        sure = int((((ref["flags"] & trm.STOPPED) > 0) & ~border).sum())
        assert set(out) == {"stats", "image"} and sure > 200 and sure <= st.stopped <= sure + int(border.sum())
        assert st.deposited == int(out["image"].sum()) and st.finished + st.unfinished == trm.N_PART


class _Wave(_Entry):
    """sr_field_wave: a z march (k_slab's staged slabs) of a 33 x 17 frame through the 5 x 6 x 7 domain.  all: Te and Z fields, the
    edge absorber and the power; bare: ne alone, no power."""

    shape, axis, toward = (33, 17), 2, -1

    def run(self, eng, layout):
        P = tw.plasma("float64")
        names, windows = tw.VARIANTS["ne, Te, Z" if layout == "all" else "ne"]
        F = {k: eng.Field(P[k], *tw.AX32) for k in names}
        try:
            return eng.wave(F["ne"], F.get("Te"), F.get("Z", tw.Z_UNIFORM), tw.field_in(self.shape), tw.frame_for(self.axis, self.shape), tw.LAM,
                            self.axis, self.toward, tw._absorber(self.shape) if windows else None, want_power=layout == "all")
        finally:
            for f in F.values():
                f.close()

    def check(self, out, layout):
        names, windows = tw.VARIANTS["ne, Te, Z" if layout == "all" else "ne"]
        P = tw.plasma("float64")
        n_cells = len(tw.AX[self.axis]) - 1

        def make():
            info = {}
            return tw.restate({k: P[k] for k in names}, tw.AX, tw.field_in(self.shape), tw.frame_for(self.axis, self.shape), tw.LAM, self.axis,
                              self.toward, tw._absorber(self.shape) if windows else None, tw.Z_UNIFORM, info=info) + (info,)

        ref, p_ref, info = _dark(("wave", layout), make)
        U, power = out
        assert info["opaque"] > 0 and U.shape == self.shape and np.all(np.isfinite(U.view(float)))
        assert float(np.max(np.abs(U - ref))) <= tw.bound(n_cells, self.shape, float(np.max(np.abs(ref))))
        if layout == "all":
            assert power.shape == (n_cells,) and tw.power_close(power, p_ref, info, n_cells, self.shape)
        else:
            assert power is None


class _WaveImage(_Entry):
    """sr_wave_image on 33 x 17.  all: aperture, stop, knife and defocus; bare: none of them (the input comes back)."""

    shape, du, dv, f = (33, 17), 6e-6, 9e-6, 0.4

    def kw(self, layout):
        if layout == "bare":
            return {}
        lf, fu = tw.LAM * self.f, np.fft.fftfreq(33, self.du)
        return dict(aperture=lf * fu[9], stop=lf * fu[2], knife=(0, lf * fu[5], 1.0), defocus=3e-4)

    def run(self, eng, layout):
        return eng.wave_image(tw.field_in(self.shape, 21), self.du, self.dv, tw.LAM, self.f, **self.kw(layout))[:1]

    def check(self, out, layout):
        U = tw.field_in(self.shape, 21)
        ref = tw.restate_image(U, self.du, self.dv, tw.LAM, self.f, **self.kw(layout)) if layout == "all" else U
        assert np.any(ref != 0) and float(np.max(np.abs(out[0] - ref))) <= tw.bound(0, self.shape, float(np.max(np.abs(U))))


class _Resample(_Entry):
    """sr_field_resample: 13 x 17 x 11 onto 9 x 14 x 19 by a generic rotation, part of the view outside; float64 and float32 (the
    output piece halves, the coordinates behind it move)."""

    layouts = ("f64", "f32")

    def run(self, eng, layout):
        src, axes, out_axes, M, t, _ = rs._case1(np.float64 if layout == "f64" else np.float32)
        return {"out": rs._resample(eng, src, axes, M, t, out_axes, fill=-7.25)}

    def check(self, out, layout):
        dtype = np.float64 if layout == "f64" else np.float32
        src, axes, out_axes, M, t, (ref, outside, S) = rs._case1(dtype)
        assert out["out"].dtype == dtype and 0.1 * outside.size < outside.sum() < 0.9 * outside.size
        rs._assert_close(out["out"], ref, outside, S, rs.K_BLEND, f"resample {layout} under 0xFF", -7.25)


class _Project(_Entry):
    """sr_volume_project: 9 x 4 x 33 along y on non-uniform axes.  all: every map (phase, kappa, Faraday); bare: the gradient
    maps alone (the absent maps must come back as exact zeros, not as what the block held)."""

    shape, axis = (9, 4, 33), "y"

    def run(self, eng, layout):
        on = layout == "all"
        vol = tp._volume(eng, tp._fields(self.shape, self.axis, False), self.axis, on, on, on)
        try:
            a, (u, v) = tp._lateral(self.axis)
            from synthpy_amd import _ffi

            raw, have = np.full((_ffi.PROJ_MAPS, self.shape[u], self.shape[v]), np.nan), C.c_uint32(0xFFFFFFFF)
            _ffi.check(_ffi.lib.sr_volume_project(vol._h, _ffi.ptr(raw), C.byref(have)))
            F = tp._fields(self.shape, self.axis, False)
            out = dict(tp._flat(vol.project()), raw=raw, have=np.uint32(have.value))
            # the module's reference: the fields read back from this volume (a dict of tuples: not among the compared arrays)
            out["_ref"] = tp._reference(vol, F["xyz"[a]], self.axis, *((F["kappa"], F["ne_f"], F["B"]) if on else (None, None, None)))
            return out
        finally:
            vol.close()

    def check(self, out, layout):
        a, _ = tp._lateral(self.axis)
        maps = {k: v for k, v in out.items() if k not in ("raw", "have", "_ref")}
        assert int(out["have"]) == (0b111111 if layout == "all" else 0b11)
        for k in range(out["raw"].shape[0]):
            if not int(out["have"]) >> k & 1:
                assert np.all(out["raw"][k] == 0.0) and not np.signbit(out["raw"][k]).any(), (k, "an absent map is not exactly 0.0")
        tp._assert_maps(maps, out["_ref"], self.shape[a], f"project {layout} under 0xFF")


ENTRIES = {
    "sightlines-nrl": lambda: _Sightlines("nrl"),
    "sightlines-table": lambda: _Sightlines("table"),
    "sightline_spectra-fl64": lambda: _Spectra(64),
    "sightline_spectra-fl256": lambda: _Spectra(256),
    "sightline_lines-fl64": lambda: _LineFamily(gl, 1, 64),
    "sightline_lines-fl256": lambda: _LineFamily(gl, 1, 256),
    "sightline_voigt-fl64": lambda: _LineFamily(vt, 3, 64),
    "sightline_voigt-fl256": lambda: _LineFamily(vt, 3, 256),
    "sightline_zeeman-fl64": lambda: _LineFamily(zt, 0, 64),
    "sightline_zeeman-fl256": lambda: _LineFamily(zt, 0, 256),
    "sightline_stokes-fl64": lambda: _LineFamily(sk, 0, 64),
    "sightline_stokes-fl256": lambda: _LineFamily(sk, 0, 256),
    "emission": lambda: _Emission(em),
    "emission_table": lambda: _Emission(tab),
    "thomson": lambda: _Thomson(th),
    "thomson_multi": lambda: _Thomson(tm),
    "thomson_sg": lambda: _Thomson(tg),
    "particles_push": _Push,
    "particles_push_matter": _PushMatter,
    "wave": _Wave,
    "wave_image": _WaveImage,
    "resample": _Resample,
    "volume_project": _Project,
}
SWEEP = [(name, k) for name in ENTRIES for k in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,layout", SWEEP, ids=[f"{n}-layout{k}" for n, k in SWEEP])
def test_staged_entry_does_not_depend_on_the_fill(eng, monkeypatch, name, layout):
    """Tier A: the entry's arrays under unset / 0xFF / 0x5A are the same bytes, and the 0xFF run passes its module's comparison
    against the restatement (three runs wrong in the same way must not pass)."""
    entry = ENTRIES[name]()
    layout = entry.layouts[layout]
    for k, v in entry.env.items():
        monkeypatch.setenv(k, v)
    outs = {}
    for pattern in PATTERNS:
        _fill(monkeypatch, eng, pattern)
        outs[pattern] = entry.run(eng, layout)
    _fill(monkeypatch, eng, None)
    found = []  # every finding of the case, not only the first: which pattern shows it says what kind of dependence it is
    for what, run in [("the module's comparison of the 0xFF run", lambda: entry.check(outs[0xFF], layout))] + [
            (f"unset against {p:#x}", lambda p=p: _same_bits(outs[None], outs[p], f"{name} {layout}: unset against {p:#x}")) for p in PATTERNS[1:]]:
        try:
            run()
        except AssertionError as e:
            found.append(f"{what}: {str(e).splitlines()[0] if str(e) else type(e).__name__}")
    assert not found, "\n".join(found)


def _dirty_block(eng, other_than_resample):
    """A larger call of another entry, unpoisoned: 2 MiB of finite values about 1 at the head of the staging block (a resample
    onto 64^3 nodes), or -- for the resample itself -- 70 x 257 spectra and their lines."""
    if other_than_resample:
        src, axes, _, M, t, _ = rs._case1(np.float64)
        big = [np.float32(np.linspace(-2e-3, 2e-3, 64))] * 3
        got = rs._resample(eng, src, axes, M, t, big, fill=1.25)
        assert got.nbytes == 8 * 64 ** 3 and np.isfinite(got).all()
    else:
        out = tsp._spectra(eng, tsp._config(tsp.CONFIGS[5], "nrl", +1, np.float64), +1)
        assert np.isfinite(out["intensity"]).all()


FAMILIES = {"sightlines": "sightline_stokes-fl64", "emission": "emission_table", "thomson": "thomson_sg", "push": "particles_push_matter",
            "wave": "wave", "resample": "resample", "project": "volume_project"}


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_another_entrys_data_in_the_kept_block_changes_nothing(eng, monkeypatch, family):
    """The cross-entry ordering case of a family: the knob unset, the block kept; a larger call of a different entry leaves its
    real data in the block, then the entry under test runs: the same bytes as before, in both layouts."""
    entry = ENTRIES[FAMILIES[family]]()
    for k, v in entry.env.items():
        monkeypatch.setenv(k, v)
    _fill(monkeypatch, eng, None)
    for layout in entry.layouts:
        before = entry.run(eng, layout)
        _dirty_block(eng, family != "resample")
        after = entry.run(eng, layout)
        _same_bits(before, after, f"{family} {layout}: after another entry's call")
        entry.check(after, layout)


# ================================================================ Tier B: the trace path
TRACE = "g2_trace_blob24_x_s0"
# name -> the existing test, called as it stands with this module's fixtures (f: request.getfixturevalue).  Between them they
# touch every owner of docs/ALLOCATIONS.md: the bundle's buffers and the binning's three (every trace with sort_rays), rec / rec2 /
# order2 / strag_* (the tile scenarios, the slab chains), the step tables (every trace), the volume's P / L (every trace) and K / Q
# (the optional terms), the pipeline's ring and staging slots, images, and the guard set (the counts flows of the mixed build).
SCENARIOS = {
    "trace_vs_oracle per-ray kernel": lambda f: tgp.test_trace_vs_oracle(f("eng"), f("orc"), TRACE, 1, 0),
    "trace_vs_oracle two sub-steps": lambda f: tgp.test_trace_vs_oracle(f("eng"), f("orc"), TRACE, 2, 0),
    "trace_vs_oracle tile kernel, records": lambda f: tgp.test_trace_vs_oracle(f("eng"), f("orc"), TRACE, 1, 1),
    "trace_vs_oracle tile kernel, producers": lambda f: tgp.test_trace_vs_oracle(f("eng"), f("orc"), TRACE, 1, 2),
    "trace_mixed_vs_oracle": lambda f: tgp.test_trace_mixed_vs_oracle(f("eng"), f("orc"), TRACE, 1),
    "fallback_rays_time_stepping": lambda f: tgp.test_fallback_rays_time_stepping(f("eng"), f("orc")),
    "pipeline ring slot, per-ray kernel": lambda f: tgp.test_pipeline_ring_slot_first_used_by_a_short_chunk(f("eng"), f("monkeypatch"), "0"),
    "pipeline ring slot, tile kernel": lambda f: tgp.test_pipeline_ring_slot_first_used_by_a_short_chunk(f("eng"), f("monkeypatch"), "1"),
    "host buffer trace in pipelined chunks": lambda f: tgp.test_host_buffer_trace_in_pipelined_chunks_is_bit_identical(f("eng"), f("monkeypatch")),
    "fused_trace_deposit": lambda f: tgp.test_fused_trace_deposit(f("eng"), f("orc"), "g2_trace_blob24_y_s0"),
    "default_counts_equal_oracle_from_s0_c1": lambda f: tgp.test_default_counts_equal_oracle_from_s0_c1(f("eng"), f("orc")),
    "interferometry end to end, bin_scale 1": lambda f: tgp.test_interferometry_end_to_end_from_s0_f64(f("eng"), f("orc"), "g2_trace_blob32_z_s0", 1, 1),
    "tile_kernel_with_optional_terms": lambda f: tgp.test_tile_kernel_with_optional_terms(f("eng"), f("orc"), f("monkeypatch"), "g5_trace_aux20_x"),
    "aux_fallback_rays": lambda f: tgp.test_aux_fallback_rays(f("eng"), f("orc")),
    "slab_chain_equals_whole_volume f64": lambda f: tgp.test_slab_chain_equals_whole_volume(f("eng"), TRACE, "f64"),
    "slab_chain_equals_whole_volume mixed": lambda f: tgp.test_slab_chain_equals_whole_volume(f("eng"), TRACE, "mixed"),
    "slab_lost_rays_and_state_errors": lambda f: tgp.test_slab_lost_rays_and_state_errors(f("eng"), f("orc")),
    "trace_counters_carried_until_read": lambda f: tgp.test_trace_counters_carried_until_read(f("eng")),
    "api_flow: legacy counts flow from HBM": lambda f: taf.test_legacy_counts_flow_deposits_from_hbm_and_equals_host_flow_and_oracle(
        f("eng"), f("orc"), f("c1"), f("c1_oracle"), 10),
    "ray_order: rebinning between segments": lambda f: tro.test_rebinning_between_segments(f("eng"), True),
    "ray_order: sort over two tiles": lambda f: tro.test_tile_boundaries_of_the_sort(f("eng"), f("base"), 4097),
    "deposit_layouts: mixed trace, exact counts": lambda f: tdl.test_mixed_trace_exact_counts(f("eng"), "edges"),
    "fresnel_layouts: affine field": lambda f: tfl.test_affine_field_is_reproduced_whatever_the_triangle(f("eng"), tfl.NAMES[0]),
    "power_spectrum: odd prime sizes": lambda f: tps.test_odd_prime_sizes(f("ps")),
}


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS[1:], ids=["0xFF", "0x5A"])
@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_trace_scenario_under_poison(eng, orc, monkeypatch, request, scenario, pattern):
    """Tier B: the existing scenario, with its own assertions, on freshly allocated working sets that hold the pattern."""
    _fill(monkeypatch, eng, pattern)
    try:
        SCENARIOS[scenario](request.getfixturevalue)
    finally:
        _fill(monkeypatch, eng, None)


def _trace_and_count(eng, precision, tile):
    """One bundle through trace, download and a counts deposit (the mixed build: with its edge guard), everything it returns."""
    g = golden(TRACE)
    x, ext = g["x"], float(g["extent"])
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), str(g["pdir"]), phaseshift=bool(g["phaseshift"]))
    img = eng.DetectorImage.counts(bin_scale=10)
    try:
        with tgp._forced_kernel(tile) as fk:
            rays = eng.RayBundle(g["s0"].shape[1]).upload(np.ascontiguousarray(g["s0"], np.float64))
            st = rays.trace(vol, eng.default_t_end(ext), ext, precision=precision)
            fk.check(rays)
        sf, rf, Jf = rays.download()
        rays.deposit(img, eng.chain_shadow_two())
        return dict(sf=sf, rf=rf, Jf=Jf, H=img.download(),
                    totals=np.array([st.ray_steps, st.fallback_rays, int(rays.retraced or 0)], np.int64))
    finally:
        img.close()
        vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision,tile", [("f64", 0), ("f64", 1), ("f64", 2), ("mixed", None)], ids=["per-ray", "records", "producers", "mixed"])
def test_trace_outputs_are_the_same_bits_under_poison(eng, monkeypatch, precision, tile):
    """Tier B, the deterministic outputs: sf, rf, Jf, the counts image, the step, fallback and edge-guard totals of one bundle,
    bit-equal between the unpoisoned run and the runs under 0xFF and 0x5A, for each float64 kernel and the mixed build."""
    outs = {}
    for pattern in PATTERNS:
        _fill(monkeypatch, eng, pattern)
        outs[pattern] = _trace_and_count(eng, precision, tile)
    _fill(monkeypatch, eng, None)
    assert outs[None]["totals"][0] > 0 and outs[None]["H"].sum() > 0
    for pattern in PATTERNS[1:]:
        _same_bits(outs[None], outs[pattern], f"trace {precision} tile {tile}: unset against {pattern:#x}")


def test_every_listed_entry_is_swept():
    """The sweep names the seventeen staged entries of the header, each in two layouts (no device needed)."""
    swept = {n.split("-")[0] for n in ENTRIES}
    assert swept == {"sightlines", "sightline_spectra", "sightline_lines", "sightline_voigt", "sightline_zeeman", "sightline_stokes",
                     "emission", "emission_table", "thomson", "thomson_multi", "thomson_sg", "particles_push", "particles_push_matter",
                     "wave", "wave_image", "resample", "volume_project"}
    assert len(SCENARIOS) >= 12 and len(SWEEP) == 2 * len(ENTRIES)
