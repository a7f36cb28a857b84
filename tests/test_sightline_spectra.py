"""Sightline spectra: sr_field_sightline_spectra (sightline_spectra.hip), engine.sightline_spectra, utils.eos_opacity.
SpectralOpacityTable, sightlines.SightlineSpectra / sightline_spectra and ScalarDomain.sightline_spectra of both API generations.

THE REFERENCE for values is tests/test_sightlines.py's `restate` -- include/synthray.h's rule in NumPy float64 -- and its standards
hold here unchanged: chord, steps, column and the set of missed lines BIT-EQUAL (`_assert_exact`), I and tau within the budgets bI,
bt it derives from the operation count (`_assert_close`); a frequency of a spectrum is a band of that rule, so nothing about the
budgets changes with the number of frequencies.  The second yardstick is the library itself: every frequency f of a spectrum must
have THE SAME BITS as band f % 4 of engine.sightlines called with the frequencies 4*(f//4) .. +3 on the same fields and lines.

Tested inputs.  The grids, fields and planted lines are test_sightlines' ((9, 7, 6), (6, 9, 17), (33, 5, 5) nodes).  The
restatement loops over bands and samples in Python, so the cases here march coarsely -- step = 1/6 of the grid's x extent, max_steps
= 8 -- except the chunk-boundary cases, which march up to 600 samples and restate three of their frequencies only (a frequency's
I and tau depend on no other frequency; the others are held by the tie).  NRL frequencies are log-spaced from 1064 nm to 100 nm (the
range test_emission.WAVELENGTHS spans, the most absorbing first), ne scaled so that the thickest line has tau = 5 at the first;
many-group tables stack the opacities of make_table(10, 10, 4, seed + k) tables on the lattice of the first, each scaled by the
factors that give the first four groups tau = 5.  A case of 70 lines holds test_sightlines' planted lines and random ones, a case of 5
the planted `inside`, `column`, `long`, `graze` and `beside`, a case of 1 `inside`.  The conditions of the 70-line cases -- at most 30 %
misses, 5..40 % of a table's samples clamped, a thin and a thick line -- are asserted on the restatement alone (test 5).
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import test_emission as nrl
import test_sightlines as ts
import test_table_emission as tab
from test_sightlines import GRIDS, _assert_close, _assert_exact, _grid, _planted, geometry, restate
from test_table_emission import host_arrays, make_table

MAX_STEPS = 8
U_TE, U_Z = ts.U_TE, ts.U_Z
KINDS = ("nrl", "table", "lte")  # the NRL node, a table with emission opacities, a table in LTE (LE is not read)
# (frequencies, lines, Te a field, Z a field, grid).  The library takes tiles of 256 frequencies where they leave no more lanes
# idle than tiles of 64 would (193..256 of every 256), else tiles of 64: both widths and the thresholds between them (192 | 193,
# 256 | 257), the wavefront, workgroup and tile edges, a ragged last tile at either width (193; 65, 257, 600), one and many tiles;
# 1, 5 and 70 lines; every kind of Te / Z; the three grids
CONFIGS = ((1, 1, True, True, "A"), (63, 5, True, False, "A"), (64, 70, False, True, "B"), (65, 5, False, False, "B"),
           (256, 1, True, True, "C"), (257, 70, True, False, "C"), (600, 5, True, True, "A"), (192, 5, False, True, "C"),
           (193, 1, True, True, "B"))
FIVE = ("inside", "column", "long", "graze", "beside")
_SCALE, _REF = {}, {}


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


# ---------------------------------------------------------------- inputs
def _step(K):
    return float(K["g"][0][-1] - K["g"][0][0]) / 6


def _lines(K, count):
    if count == 5:
        P = _planted(K["g"])
        return (np.ascontiguousarray(np.array([P[k][0] for k in FIVE]).T), np.ascontiguousarray(np.array([P[k][1] for k in FIVE]).T))
    return ts._lines(K["g"], count, K["seed"] + count)


def _nrl_node(nf):
    """("nrl", (omega, e_ph, c_omega)) of nf frequencies from 1064 nm to 100 nm, log-spaced: the bits the host hands the kernel."""
    from synthpy_amd import engine

    lam = np.geomspace(max(nrl.WAVELENGTHS), min(nrl.WAVELENGTHS), nf) if nf > 1 else np.float64(nrl.WAVELENGTHS[:1])
    om, e_ph, c_om = engine.spectrum_constants(2 * np.pi * nrl.LIGHT / lam)
    return ("nrl", (om.tolist(), e_ph.tolist(), c_om.tolist()))


def _stack(nf, seed, lte, shift=None):
    """A SpectralOpacityTable of nf groups: the opacities of make_table(10, 10, 4, seed + k), k = 0, 1, .., on the lattice of the
    first; photon energies 30 .. 900 eV log-spaced, the groups' edges halfway between them (in the logarithm)."""
    from synthpy_amd.utils.eos_opacity import SpectralOpacityTable

    parts = [make_table(10, 10, 4, seed + k, lte=lte, shift=shift) for k in range((nf + 3) // 4)]
    e = np.geomspace(30.0, 900.0, nf) if nf > 1 else np.array([90.0])
    r = (e[1] / e[0]) ** 0.5 if nf > 1 else 1.25
    return SpectralOpacityTable(parts[0].temperatures, parts[0].densities, np.concatenate([p.absorption for p in parts])[:nf], e, 12.011,
                                emission=None if lte else np.concatenate([p.emission for p in parts])[:nf],
                                edges=np.stack([e / r, e * r], axis=1))


def _host(table, bands=None):
    """test_table_emission.host_arrays for a table of any number of groups: four groups at a time, joined; bands: indices."""
    idx = np.arange(table.n_band) if bands is None else np.asarray(bands)
    parts = [host_arrays(table.bands(idx[k:k + 4])) for k in range(0, len(idx), 4)]
    H = dict(parts[0])
    H["LA"] = np.concatenate([p["LA"] for p in parts])
    H["LE"] = None if parts[0]["LE"] is None else np.concatenate([p["LE"] for p in parts])
    for k in ("e_ph", "c_omega"):
        H[k] = [v for p in parts for v in p[k]]
    H["GA"] = tuple(np.concatenate([p["GA"][m] for p in parts]) for m in range(3))
    H["GE"] = None if parts[0]["GE"] is None else tuple(np.concatenate([p["GE"][m] for p in parts]) for m in range(3))
    return H


def _scale(cfg, kind):
    """(ne float64, the table's ln factors or None) of one configuration: its thickest line has tau = 5 at the first NRL frequency /
    in each of the first four groups."""
    key = (cfg[1:], kind)
    if key not in _SCALE:
        nf, count, te_f, z_f, name = cfg
        K = _grid(name)
        o, d = _lines(K, count)
        Te, Z = K["Te"] if te_f else U_TE, K["Z"] if z_f else U_Z
        if kind == "nrl":
            ne = K["ne"]["nrl"]
            t = restate(ne, Te, Z, K["co"], o, d, _nrl_node(1), +1, _step(K), MAX_STEPS)["tau"].max()
            _SCALE[key] = (ne * np.sqrt(5.0 / t), None)
        else:
            ne = K["ne"]["table"]
            t = restate(ne, Te, Z, K["co"], o, d, ("table", _host(_stack(4, K["seed"] + 1, kind == "lte"))), +1, _step(K), MAX_STEPS)["tau"].max(axis=1)
            _SCALE[key] = (ne, np.log(5.0 / t))
    return _SCALE[key]


def _node_of(R, bands=None):
    if R["kind"] == "nrl":
        data = R["node"][1]
        return R["node"] if bands is None else ("nrl", tuple([v[b] for b in bands] for v in data))
    return ("table", _host(R["table"], bands))


def _config(cfg, kind, toward, dtype, restated=True):
    """The inputs of one configuration and (restated) their restatement, cached: fields in `dtype`, widened for the restatement;
    back is (n, n_freq), the entry's layout, the restatement's arrays are (n_freq, n)."""
    key = (cfg, kind, toward, np.dtype(dtype).name)
    if key not in _REF:
        nf, count, te_f, z_f, name = cfg
        K = _grid(name)
        o, d = _lines(K, count)
        ne, shift = _scale(cfg, kind)
        R = dict(K=K, o=o, d=d, ne=ne.astype(dtype), Te=K["Te"].astype(dtype) if te_f else U_TE, Z=K["Z"].astype(dtype) if z_f else U_Z,
                 back=np.random.default_rng(K["seed"] + 3 + nf).uniform(0.0, 2e-7, (o.shape[1], nf)), nf=nf, kind=kind, step=_step(K),
                 max_steps=MAX_STEPS, table=None if kind == "nrl" else _stack(nf, K["seed"] + 1, kind == "lte", shift))
        R["node"] = _nrl_node(nf) if kind == "nrl" else None
        _REF[key] = R
    R = _REF[key]
    if restated and "ref" not in R:
        R["ref"] = _restate(R, toward)
    return R


def _restate(R, toward, bands=None, backlight="own"):
    back = R["back"] if isinstance(backlight, str) else backlight
    if back is not None and bands is not None:
        back = back[:, bands]
    return restate(R["ne"], R["Te"], R["Z"], R["K"]["co"], R["o"], R["d"], _node_of(R, bands), toward, R["step"], R["max_steps"],
                   backlight=None if back is None else back.T)


def _assert_inputs(R, what):
    """The module docstring's conditions of a 70-line case, on the restatement alone; any case: no empty line that hits."""
    ref = R["ref"]
    hit = ~ref["miss"]
    assert np.all(ref["tau"][:, hit] > 0) and np.all(ref["I"][:, hit] > 0) and np.all(ref["column"][hit] > 0), f"{what}: an empty line that hits"
    assert np.all(np.isfinite(ref["I"])) and np.all(np.isfinite(ref["tau"]))
    if len(hit) >= 63:
        assert np.mean(ref["miss"]) <= 0.30, f"{what}: {np.mean(ref['miss']):.2f} of the lines miss"
        tau = ref["tau"][0]
        assert np.any((tau > 0) & (tau < 1e-3)) and np.any((tau > 1) & (tau < 30)), f"{what}: tau spans {tau[hit].min():.2e} .. {tau.max():.2e}"
        assert np.any(ref["steps"] == MAX_STEPS) and np.any(ref["steps"] == 1) and np.any(ref["miss"])
        if R["kind"] != "nrl":
            assert 0.05 <= ref["clamped"] <= 0.40, f"{what}: clamped share {ref['clamped']:.3f}"
    return ref["clamped"]


def _upload(eng, R):
    return [eng.Field(a, *R["K"]["co"]) if np.ndim(a) else float(a) for a in (R["ne"], R["Te"], R["Z"])]


def _close(fields):
    for f in fields:
        if not isinstance(f, float):
            f.close()


def _node_kw(R, bands=None):
    """The node's keywords for engine.sightline_spectra (bands None) or for engine.sightlines with the frequencies `bands`."""
    if R["kind"] == "nrl":
        om = np.float64(R["node"][1][0])
        return dict(omegas=om if bands is None else om[bands])
    return dict(table=R["table"] if bands is None else R["table"].bands(bands))


def _spectra(eng, R, toward, fields=None, backlight="own", **kw):
    """engine.sightline_spectra (on freshly uploaded fields unless given); I, tau as the restatement lays them out: (n_freq, n)."""
    own = fields is None
    fields = _upload(eng, R) if own else fields
    try:
        out = eng.sightline_spectra(*fields, R["o"], R["d"], toward=toward, step=R["step"], max_steps=R["max_steps"],
                                    backlight=R["back"] if isinstance(backlight, str) else backlight, **_node_kw(R), **kw)
        assert fields[0].last_kernel_ms > 0
        assert out["intensity"].shape == out["optical_depth"].shape == (R["o"].shape[1], R["nf"])
        out["I"], out["tau"] = out["intensity"].T, out["optical_depth"].T
        return out
    finally:
        if own:
            _close(fields)


def _assert_tie(eng, R, toward, fields, got, what):
    """Test 7's property: frequency f of `got` has the bits of band f % 4 of engine.sightlines with the frequencies 4*(f//4) .. +3."""
    for k in range(0, R["nf"], 4):
        bands = np.arange(k, min(k + 4, R["nf"]))
        four = eng.sightlines(*fields, R["o"], R["d"], toward=toward, step=R["step"], max_steps=R["max_steps"],
                              backlight=np.ascontiguousarray(R["back"][:, bands].T), **_node_kw(R, bands))
        for name in ("intensity", "optical_depth"):
            same = got[name][:, bands].T == four[name]
            assert np.array_equal(got[name][:, bands].T, four[name], equal_nan=True), \
                f"{what}: {name} of frequencies {k}.. differs from engine.sightlines' bits in {np.sum(~same)} of {same.size} elements"
        for name in ("column", "chord", "steps"):
            assert np.array_equal(got[name], four[name], equal_nan=True), f"{what}: {name} differs from engine.sightlines' (frequencies {k}..)"


def _sub(ref, got, bands):
    """`got` cut to the restated frequencies."""
    return dict(got, I=got["I"][bands], tau=got["tau"][bands])


# the chunk-boundary cases (test 8, asserted in test 5): chords parallel to x through the box of grid A, N samples each
CHUNK_N = {64: (1, 63, 64, 65, 131), 256: (1, 255, 256, 257, 515)}
CHUNK_FREQS = {64: 5, 256: 200}   # 200 frequencies take one tile of 256 (56 lanes idle), 5 one of 64
CHUNK_CAP = 600


def _chunk_case(fl, N, kind, toward):
    """Three chords along x through grid A -- a node column, mid-cell, along a face -- with step = chord / (N - 0.5), so that
    ceil gives exactly N samples (N = CHUNK_CAP + 1: a step of chord / 10^4, every line capped at max_steps = CHUNK_CAP)."""
    nf = CHUNK_FREQS[fl]
    R = dict(_config((nf, 5, True, True, "A"), kind, toward, np.float64, restated=False))
    g = R["K"]["g"]
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    far = lo[0] - 2.0 ** -10
    o = np.array([[far, g[1][2], g[2][3]], [far, 0.37 * lo[1] + 0.63 * hi[1], 0.5 * (g[2][1] + g[2][2])], [far, lo[1], 0.5 * (lo[2] + hi[2])]]).T
    d = np.array([[1.0, 0.0, 0.0]] * 3).T
    chord = hi[0] - lo[0]
    R.update(o=np.ascontiguousarray(o), d=np.ascontiguousarray(d), back=R["back"][:3], max_steps=CHUNK_CAP,
             step=chord / (N - 0.5) if N <= CHUNK_CAP else chord / 1e4)
    return R


# ================================================================ CPU tests
def test_abi_and_signatures(built):
    """1: the header's prototype and struct, the ctypes binding and the Python signatures agree."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "synthray.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sr_field_sightline_spectra\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 19
    kinds = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]
    assert kinds[5] == "int64_t" and kinds[8] == "int32_t" and kinds[3] == "const sr_emission_table *" and kinds[4] == "const sr_spectra_params *"
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*sr_spectra_params\s*;", text)
    fields = ["toward", "max_steps", "step", "Te", "Z"]
    assert m and re.findall(r"\b(" + "|".join(fields) + r")\b", m.group(1)) == fields
    assert re.search(r"#define\s+SR_MAX_FREQS\s+16384\b", text) and built.MAX_FREQS == 16384 and built.MAX_BANDS == 4
    P = built.SpectraParams
    assert [f[0] for f in P._fields_] == fields and C.sizeof(P) == 32
    assert [getattr(P, f).offset for f in fields] == [0, 4, 8, 16, 24]
    res, args = built.SYMBOLS["sr_field_sightline_spectra"]
    assert res is C.c_int and len(args) == 19 and args[5] is C.c_int64 and args[8] is C.c_int32
    assert hasattr(built.lib, "sr_field_sightline_spectra")
    mk = open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()
    assert "sightline_spectra.hip" in mk and "sightline_march.inc" in mk  # the build id covers both
    # the rule is stated once: the new section refers to sr_field_sightlines' and does not repeat its lines
    raw = open(os.path.join(ROOT, "include", "synthray.h")).read()
    assert raw.count("t0 = max(t0, min(ta, tb))") == 1 and raw.count("dtau = alpha*h;") == 1

    from synthpy_amd import engine, sightlines
    from synthpy_amd._domain import DomainExtras
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.sightline_spectra) == names(engine.sightlines)
    par = inspect.signature(engine.sightline_spectra).parameters
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names(engine.sightline_spectra)[5:])
    assert names(sightlines.sightline_spectra) == ["domain", "view", "wavelengths", "photon_energies", "table", "step", "max_steps", "fields"]
    assert names(NewDomain.sightline_spectra) == names(OldDomain.sightline_spectra) == ["self", "view", "wavelengths", "photon_energies", "table",
                                                                                         "step", "max_steps"]
    assert NewDomain.sightline_spectra is DomainExtras.sightline_spectra is OldDomain.sightline_spectra
    for doc in (DomainExtras.sightline_spectra.__doc__, sightlines.sightline_spectra.__doc__):
        assert "cos^4" in doc and "refraction" in doc and "hbar*omega <~ Te" in doc
    om, e_ph, c_om = engine.spectrum_constants([2e15, 3e15, 4e15, 5e15, 6e15])
    e = engine.emission_params([2e15, 3e15, 4e15, 5e15], 0)
    assert list(om[:4]) == list(e.omega) and list(e_ph[:4]) == list(e.e_ph) and list(c_om[:4]) == list(e.c_omega) and len(c_om) == 5


def test_argument_checks_come_before_the_device(built):
    """2: every rejected argument is SR_ERR_INVALID with its own text and the device is never initialised: the calls carry NULL
    fields, so a call that passed every other check ends at 'NULL ne'."""
    from synthpy_amd import engine

    lib, ptr = built.lib, built.ptr
    table = _stack(5, 9, False)
    o0, d0 = np.zeros((3, 2)), np.ones((3, 2))
    out = np.zeros((2, 5))
    om0, e0, c0 = engine.spectrum_constants(np.float64(table.photon_energy) * tab.E_CHARGE / tab.HBAR)

    def params(toward=1, step=1e-4, max_steps=10):
        p = built.SpectraParams()
        p.toward, p.max_steps, p.step = toward, max_steps, step
        return p

    def call(p, n=2, o=o0, d=d0, I=out, tau=out, t=None, nf=5, om=om0, e=e0, c=c0):
        return lib.sr_field_sightline_spectra(None, None, None, None if t is None else C.byref(t), None if p is None else C.byref(p), n, ptr(o),
                                              ptr(d), nf, ptr(om), ptr(e), ptr(c), None, ptr(I), ptr(tau), None, None, None, None)

    def err(text, *a, **kw):
        assert call(*a, **kw) == -1 and text in built.last_error(), (text, built.last_error())

    err("NULL argument", None)
    for name in ("o", "d", "I", "tau"):
        err("NULL argument", params(), **{name: None})
    err("NULL e_ph or c_omega", params(), e=None)
    err("NULL e_ph or c_omega", params(), c=None)
    err("NULL omega without a table", params(), om=None)
    err("n must not be negative", params(), n=-1)
    for nf in (0, -3, built.MAX_FREQS + 1):
        err("n_freq must be 1..16384", params(), nf=nf)
    for w in (0.0, -1.0, np.nan, np.inf):
        bad = om0.copy()
        bad[4] = w
        err("omega of frequency 4", params(), om=bad)
    for name in ("e", "c"):
        bad = e0.copy()
        bad[3] = np.nan
        err("e_ph or c_omega of frequency 3", params(), **{name: bad})
    for toward in (0, 2, -3):
        err("toward", params(toward=toward))
    for step in (0.0, -1e-4, np.nan, np.inf):
        err("step must be finite and positive", params(step=step))
    for ms in (0, -5):
        err("max_steps", params(max_steps=ms))
    # the table's checks, with this entry's name; omega is ignored with a table and may be NULL
    t, keep = engine.emission_table_params(table)
    err("NULL ne", params(), t=t, om=None)
    bad = om0.copy()
    bad[0] = -1.0
    err("NULL ne", params(), t=t, om=bad)
    t.nT = 1
    err("nT must be 2..512", params(), t=t)
    t, keep = engine.emission_table_params(table)
    keep[0][1] = keep[0][0]
    err("LT is not strictly increasing at 1", params(), t=t)
    t, keep = engine.emission_table_params(table)
    keep[2][4, 2, 3] = np.inf
    err("LA has a non-finite entry (band 4)", params(), t=t)
    t, keep = engine.emission_table_params(table)
    t.m_ion = 0.0
    err("m_ion", params(), t=t)
    # a packed table of 2^31 values or more: refused from the counts alone, before an entry is read
    t, keep = engine.emission_table_params(table)
    t.nT, t.nD = 512, 512
    many = np.full(built.MAX_FREQS, 1.0)
    err("the packed table holds", params(), t=t, nf=built.MAX_FREQS, om=None, e=many, c=many)
    # n x tiles beyond the grid: refused before a line is read (65 frequencies: two tiles of 64 ... one of 256: n itself is the limit)
    err("n x frequency tiles exceeds 2^31 - 1 workgroups", params(), n=2 ** 31, nf=5)
    err("n x frequency tiles exceeds 2^31 - 1 workgroups", params(), n=2 ** 30, nf=600, om=many[:600], e=many[:600], c=many[:600])
    for name, text in (("o", "non-finite origin of line 1"), ("d", "non-finite direction of line 1")):
        for v in (np.nan, np.inf):
            a = np.ones((3, 2))
            a[2, 1] = v
            err(text, params(), **{name: a})
    dz = np.ones((3, 2))
    dz[:, 1] = 0.0
    err("the direction of line 1 is zero", params(), d=dz)
    err("NULL ne", params())        # every other argument was in order
    err("NULL ne", params(), n=0)   # n == 0 does not skip the checks
    assert "sr_field_sightline_spectra" in built.last_error()

    with pytest.raises(ValueError, match="Field"):
        engine.sightline_spectra(np.zeros((2, 2, 2)), 1.0, 1.0, o0, d0, omegas=om0, toward=1, step=1e-4, max_steps=5)


def test_spectral_opacity_table(built):
    """3: SpectralOpacityTable takes 5 and 300 bands where OpacityTable raises; bands() round-trips; packed() is the
    group-innermost transpose of logs(); validation errors name the member."""
    from synthpy_amd.utils.eos_opacity import OpacityTable, SpectralOpacityTable

    for nf in (5, 300):
        t = _stack(nf, 21, False)
        assert isinstance(t, OpacityTable) and t.n_band == nf and t.absorption.shape == t.emission.shape == (nf, 10, 10) and t.edges.shape == (nf, 2)
        with pytest.raises(ValueError, match="absorption must hold 1 to 4 bands"):
            OpacityTable(t.temperatures, t.densities, t.absorption, t.photon_energy, t.A)
        LT, LD, LA, LE = t.logs()
        PT, PD, PA, PE = t.packed()
        assert np.array_equal(PT, LT) and np.array_equal(PD, LD) and PA.shape == (10, 10, nf) and PA.flags["C_CONTIGUOUS"]
        assert np.array_equal(PA, LA.transpose(1, 2, 0)) and np.array_equal(PE, LE.transpose(1, 2, 0))
        idx = [nf - 1, 0, 3]
        b = t.bands(idx)
        assert type(b) is OpacityTable and b.n_band == 3 and np.array_equal(b.absorption, t.absorption[idx]) and np.array_equal(b.emission, t.emission[idx])
        assert np.array_equal(b.photon_energy, t.photon_energy[idx]) and np.array_equal(b.edges, t.edges[idx]) and b.A == t.A
        assert np.array_equal(b.temperatures, t.temperatures) and np.array_equal(b.densities, t.densities)
        assert np.array_equal(t.bands(slice(4, 8)).absorption, t.absorption[4:8])
        with pytest.raises(ValueError, match="absorption must hold 1 to 4 bands"):
            t.bands(slice(0, 5))
    lte = _stack(7, 21, True)
    assert lte.emission is None and lte.packed()[3] is None and lte.bands([6]).emission is None
    four = make_table(10, 10, 4, 21)
    same = SpectralOpacityTable(four.temperatures, four.densities, four.absorption, four.photon_energy, four.A, emission=four.emission, edges=four.edges)
    assert all(np.array_equal(a, b) for a, b in zip(same.logs(), four.logs()))
    T, D, A5, e5 = t.temperatures, t.densities, t.absorption[:5], t.photon_energy[:5]
    bad = A5.copy()
    bad[4, 2, 2] = -1.0
    for match, args, kw in (("temperatures must be strictly increasing", (T[::-1], D, A5, e5, 12.0), {}),
                            ("densities must be finite and positive", (T, -D, A5, e5, 12.0), {}),
                            ("absorption must be finite and positive", (T, D, bad, e5, 12.0), {}),
                            ("absorption has shape", (T, D, A5[:, :9], e5, 12.0), {}),
                            ("photon_energy must be 5", (T, D, A5, e5[:4], 12.0), {}),
                            ("photon_energy must be", (T, D, A5, -e5, 12.0), {}),
                            ("emission has shape", (T, D, A5, e5, 12.0), {"emission": A5[:4]}),
                            ("emission must be finite and positive", (T, D, A5, e5, 12.0), {"emission": bad}),
                            (r"edges must be \(5, 2\)", (T, D, A5, e5, 12.0), {"edges": np.ones((2, 5))}),
                            (r"edges must be \(5, 2\)", (T, D, A5, e5, 12.0), {"edges": np.ones(10)}),
                            ("edges must be", (T, D, A5, e5, 12.0), {"edges": np.ones((5, 2))}),
                            ("A must be a finite positive", (T, D, A5, e5, 0.0), {}),
                            ("absorption must hold 1 to 16384 bands", (T, D, np.ones((built.MAX_FREQS + 1, 10, 10)), np.ones(built.MAX_FREQS + 1), 12.0), {})):
        with pytest.raises(ValueError, match=match):
            SpectralOpacityTable(*args, **kw)
    assert "group MEANS only" in SpectralOpacityTable.__doc__


def test_signal_by_hand(built):
    """4: SightlineSpectra.signal against a hand-computed trapezoid (point frequencies, given in descending order) and group sum."""
    from synthpy_amd import engine, sightlines

    view = sightlines.Chords(np.zeros((3, 2)), np.ones((3, 2)), -1)
    I = np.array([[1.0, 2.0, 4.0], [3.0, 0.0, 5.0]])
    z = np.zeros(2)
    sp = sightlines.SightlineSpectra(view, I, np.zeros((2, 3)), z, z, z, omega=[8.0, 4.0, 2.0])
    # ascending omega 2, 4, 8 carries I = (4, 2, 1) and (5, 0, 3): 0.5*(4+2)*2 + 0.5*(2+1)*4 = 12;  0.5*5*2 + 0.5*3*4 = 11
    assert np.array_equal(sp.signal(), [12.0, 11.0])
    # R = (1, 2, 3) in the given order: I*R = (1, 4, 12), (3, 0, 15) -> ascending (12, 4, 1), (15, 0, 3): 16 + 10 = 26; 15 + 6 = 21
    assert np.array_equal(sp.signal([1.0, 2.0, 3.0]), [26.0, 21.0])
    assert np.array_equal(sp.signal(lambda e: 2.0 * np.ones_like(e)), [24.0, 22.0])
    seen = []
    sp.signal(lambda e: seen.append(e) or np.ones_like(e))
    assert np.array_equal(seen[0], engine.HBAR * np.array([8.0, 4.0, 2.0]) / engine.E_CHARGE) and np.array_equal(sp.photon_energy, seen[0])
    assert np.array_equal(sp.wavelengths, 2 * np.pi * engine.c / np.array([8.0, 4.0, 2.0])) and np.array_equal(sp.transmission, np.ones((2, 3)))
    with pytest.raises(ValueError, match="edges"):
        sp.band_radiance
    with pytest.raises(ValueError, match="response must give 3"):
        sp.signal([1.0, 2.0])
    k = engine.E_CHARGE / engine.HBAR  # (rad/s) per eV
    edges = np.array([[1.0, 3.0], [3.0, 4.0], [4.0, 8.0]])
    sg = sightlines.SightlineSpectra(view, I, np.zeros((2, 3)), z, z, z, omega=np.array([2.0, 3.5, 6.0]) * k, edges=edges)
    dw = np.array([2.0, 1.0, 4.0]) * engine.E_CHARGE / engine.HBAR
    assert np.array_equal(sg.band_radiance, I * dw)
    assert np.allclose(sg.signal(), [(1 * 2 + 2 * 1 + 4 * 4) * k, (3 * 2 + 0 + 5 * 4) * k], rtol=1e-15)
    assert np.allclose(sg.signal([0.5, 1.0, 0.0]), [(1 * 2 * 0.5 + 2 * 1) * k, (3 * 2 * 0.5) * k], rtol=1e-15)
    one = sightlines.SightlineSpectra(view, I[:, :1], np.zeros((2, 1)), z, z, z, omega=[5.0])
    assert np.array_equal(one.signal(), [0.0, 0.0])
    with pytest.raises(ValueError, match="shapes"):
        sightlines.SightlineSpectra(view, I.T, np.zeros((3, 2)), z, z, z, omega=[8.0, 4.0, 2.0])


def test_tested_inputs_meet_the_conditions(built):
    """5: the inputs of the kernel tests meet the module docstring's conditions, on the restatement alone; the chunk-boundary
    chords get exactly the step counts their names say, and the capped case the cap."""
    shares = []
    for cfg in CONFIGS:
        if cfg[1] < 63:
            continue
        for kind in KINDS:
            for dtype in (np.float32, np.float64):
                for toward in (+1, -1):
                    # the conditions concern frequency 0 and the geometry: the first four frequencies are restated
                    R = _config(cfg, kind, toward, dtype, restated=False)
                    r = dict(R, ref=_restate(R, toward, bands=np.arange(4)))
                    shares.append(_assert_inputs(r, f"{cfg} {kind} {np.dtype(dtype).name} toward {toward:+d}"))
    print(f"clamped share of the table cases {min(s for s in shares if s > 0):.3f} .. {max(shares):.3f}")
    for name in GRIDS:
        K = _grid(name)
        o, d = _lines(K, 5)
        G = geometry(K["g"], o, d, _step(K), MAX_STEPS)
        assert list(G["hit"]) == [True, True, True, True, False] and G["n"][FIVE.index("long")] == MAX_STEPS and G["n"][FIVE.index("graze")] == 1
    for fl, Ns in CHUNK_N.items():
        for N in Ns + (CHUNK_CAP + 1,):
            R = _chunk_case(fl, N, "nrl", +1)
            G = geometry(R["K"]["g"], R["o"], R["d"], R["step"], R["max_steps"])
            assert np.all(G["hit"]) and np.all(G["n"] == min(N, CHUNK_CAP)), (fl, N, G["n"])
            assert N <= CHUNK_CAP or np.all(G["chord"] / R["step"] > CHUNK_CAP)


# ================================================================ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("toward", [+1, -1], ids=["plus", "minus"])
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_against_restatement(eng, kind, toward, dtype):
    """6: every configuration -- 1, 63, 64, 65, 192, 193, 256, 257 and 600 frequencies on 1, 5 and 70 lines, Te and Z as fields or scalars,
    three grids -- chord, steps, column and the missed lines bit-equal, I and tau within the restatement's budgets."""
    for cfg in CONFIGS:
        R = _config(cfg, kind, toward, dtype)
        what = f"{cfg} {kind} {np.dtype(dtype).name} toward {toward:+d}"
        _assert_inputs(R, what)
        got = _spectra(eng, R, toward)
        _assert_exact(got, R["ref"], what)
        _assert_close(got, R["ref"], what)
        miss = R["ref"]["miss"]
        assert np.array_equal(got["intensity"][miss], R["back"][miss]) and np.all(got["optical_depth"][miss] == 0)
        if cfg == CONFIGS[3]:  # without the optional outputs and without a backlight: the same optical depths
            bare = _spectra(eng, R, toward, want=("intensity", "optical_depth"), backlight=None)
            assert set(bare) == {"intensity", "optical_depth", "I", "tau"}
            _assert_close(bare, _restate(R, toward, backlight=None), what + " no backlight")
            assert np.array_equal(bare["tau"], got["tau"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("toward", [+1, -1], ids=["plus", "minus"])
@pytest.mark.parametrize("kind", ["nrl", "table"])
@pytest.mark.parametrize("nf", [5, 130])
def test_same_bits_as_engine_sightlines(eng, nf, kind, toward, dtype):
    """7: on the same uploaded fields and 70 lines, every frequency f has the bits of band f % 4 of engine.sightlines called with the
    frequencies 4*(f//4) .. +3 (a table through table.bands): I, tau, column, chord, steps, array_equal."""
    R = _config((nf, 70, True, nf == 5, "B" if nf == 5 else "C"), kind, toward, dtype, restated=False)
    fields = _upload(eng, R)
    try:
        got = _spectra(eng, R, toward, fields=fields)
        assert np.all(got["steps"][:3] > 0) and np.any(got["steps"] == 0) and np.all(got["optical_depth"][got["steps"] > 0] > 0)
        _assert_tie(eng, R, toward, fields, got, f"{nf} frequencies {kind} {np.dtype(dtype).name} toward {toward:+d}")
    finally:
        _close(fields)


@pytest.mark.gpu
@pytest.mark.parametrize("toward", [+1, -1], ids=["plus", "minus"])
@pytest.mark.parametrize("kind", ["nrl", "table"])
@pytest.mark.parametrize("fl", [64, 256])
def test_chunk_boundaries_of_the_sample_staging(eng, fl, kind, toward):
    """8: axis-parallel chords of exactly N samples, N = 1, FL-1, FL, FL+1, 2 FL+3 at both lane widths, and lines capped at max_steps
    = 600: the first, the middle and the last frequency against the restatement, every frequency against engine.sightlines' bits."""
    for N in CHUNK_N[fl] + (CHUNK_CAP + 1,):
        R = _chunk_case(fl, N, kind, toward)
        what = f"FL {fl}, {min(N, CHUNK_CAP)} samples, {kind} toward {toward:+d}"
        bands = np.array([0, R["nf"] // 2, R["nf"] - 1])
        ref = _restate(R, toward, bands=bands)
        assert np.all(ref["steps"] == min(N, CHUNK_CAP))
        fields = _upload(eng, R)
        try:
            got = _spectra(eng, R, toward, fields=fields)
            _assert_exact(got, ref, what)
            _assert_close(_sub(ref, got, bands), ref, what)
            _assert_tie(eng, R, toward, fields, got, what)
        finally:
            _close(fields)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nrl", "table"])
def test_misses_and_empties(eng, kind):
    """9: the planted beside, corner and away lines return the backlight at every frequency, tau = 0, steps = 0, among lines that hit
    and in a call whose lines all miss; n = 0 is accepted."""
    R = _config(CONFIGS[5], kind, +1, np.float64, restated=False)
    names = list(_planted(R["K"]["g"]))
    at = [names.index(k) for k in ("beside", "corner", "away")]
    got = _spectra(eng, R, +1)
    for k in at:
        assert np.array_equal(got["intensity"][k], R["back"][k]) and np.all(got["optical_depth"][k] == 0)
        assert got["steps"][k] == 0 and got["chord"][k] == 0 and got["column"][k] == 0
    assert np.all(got["steps"][[names.index("column"), names.index("inside")]] > 0)
    for back in ("own", None):
        M = dict(R, o=np.ascontiguousarray(R["o"][:, at]), d=np.ascontiguousarray(R["d"][:, at]), back=R["back"][at])
        none = _spectra_no_time(eng, M, -1, backlight=back)
        assert np.array_equal(none["intensity"], M["back"] if back == "own" else np.zeros((3, R["nf"]))) and np.all(none["optical_depth"] == 0)
        assert np.all(none["steps"] == 0) and np.all(none["chord"] == 0) and np.all(none["column"] == 0)
    E = dict(R, o=np.zeros((3, 0)), d=np.zeros((3, 0)), back=np.zeros((0, R["nf"])))
    empty = _spectra_no_time(eng, E, +1)
    assert empty["intensity"].shape == (0, R["nf"]) and empty["steps"].shape == (0,)


def _spectra_no_time(eng, R, toward, backlight="own"):
    fields = _upload(eng, R)
    try:
        return eng.sightline_spectra(*fields, R["o"], R["d"], toward=toward, step=R["step"], max_steps=R["max_steps"],
                                     backlight=R["back"] if isinstance(backlight, str) else backlight, **_node_kw(R))
    finally:
        _close(fields)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nrl", "table"])
def test_nan_node_poisons_the_lines_through_its_cells(eng, kind):
    """10: a NaN node of ne, and one of Te, make NaN exactly the lines the restatement says pass their cells, at every frequency of
    those lines, and no other element."""
    base = _config((65, 70, True, True, "A"), kind, -1, np.float64, restated=False)
    for name, at in (("ne", (4, 3, 2)), ("Te", (1, 5, 4))):
        R = dict(base)
        a = np.array(base[name])
        a[at] = np.nan
        R[name] = a
        ref = _restate(R, -1)
        poisoned = np.isnan(ref["I"][0])
        assert 0 < poisoned.sum() < 0.5 * len(poisoned), f"NaN in {name}: {poisoned.sum()} of {len(poisoned)} lines"
        got = _spectra(eng, R, -1)
        _assert_close(got, ref, f"NaN node of {name}, {kind}")
        _assert_exact(got, ref, f"NaN node of {name}, {kind}")
        for m in ("intensity", "optical_depth"):
            assert np.array_equal(np.isnan(got[m]), np.repeat(poisoned[:, None], 65, axis=1)), f"NaN node of {name}, {kind}: the NaN set of {m}"
        assert np.array_equal(np.isnan(got["column"]), poisoned if name == "ne" else np.zeros_like(poisoned))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nrl", "table"])
def test_a_repeated_call_returns_identical_bits(eng, kind):
    """11: two calls, on fresh uploads, return identical bits."""
    R = _config(CONFIGS[5], kind, -1, np.float32, restated=False)
    a, b = _spectra(eng, R, -1), _spectra(eng, R, -1)
    assert all(np.array_equal(a[k], b[k]) for k in ("intensity", "optical_depth", "column", "chord", "steps"))
    assert np.all(np.isfinite(a["intensity"])) and a["intensity"].max() > 0


@pytest.mark.gpu
def test_end_to_end_on_both_generations(eng):
    """12: domain.sightline_spectra(Chords, photon_energies=) and (.., table=) on a domain of each generation: shapes, units,
    signal(); a PinholeCamera view comes back in pixel order: four of its frequencies are sightline_emission's maps, bit for bit."""
    from synthpy_amd import sightlines
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy import full_solver as fs

    dims, cell = (9, 7, 11), 5e-4
    lengths = tuple(cell * (m - 1) for m in dims)
    rng = np.random.default_rng(12)
    ne = (1e25 * rng.uniform(0.5, 1.5, dims)).astype(np.float32)
    Te = (80.0 * rng.uniform(0.5, 1.5, dims)).astype(np.float32)
    new = NewDomain(lengths, dims)
    old = fs.ScalarDomain(*[np.linspace(-L / 2, L / 2, m) for L, m in zip(lengths, dims)], lengths[2] / 2)
    for dom in (new, old):
        dom.external_ne(ne)
        dom.external_Te(Te)
        dom.external_Z(3.0)
    ch = sightlines.Chords([[0.0, 1e-4, 0.0], [-8e-3, -8e-3, 0.0], [1e-3, 0.0, 9e-3]], [[0.1, 0.0, 0.0], [1.0, 1.0, 0.0], [-0.05, 0.1, 1.0]], -1,
                           backlight=1e-8)
    e_ph = np.geomspace(1.0, 60.0, 70)
    table = _stack(30, 40, False)
    cam = sightlines.PinholeCamera((0, 0, 20e-3), (0.1, 0, -1), (0, 1, 0), 60e-3, (13, 9), cell * 3)
    lam = np.geomspace(1064e-9, 100e-9, 9)
    for dom in (new, old):
        sp = dom.sightline_spectra(ch, photon_energies=e_ph)
        assert isinstance(sp, sightlines.SightlineSpectra) and sp.intensity.shape == sp.optical_depth.shape == sp.transmission.shape == (3, 70)
        assert sp.column.shape == sp.chord.shape == sp.steps.shape == (3,) and sp.steps.dtype == np.int32
        assert np.allclose(sp.photon_energy, e_ph, rtol=1e-15) and np.allclose(sp.wavelengths, 1.2398419843320026e-6 / e_ph, rtol=1e-14)
        assert sp.edges is None and list(sp.steps > 0) == [True, True, False] and np.all(sp.intensity[2] == 1e-8) and np.all(sp.optical_depth[:2] > 0)
        y = sp.intensity * 0.5
        assert np.allclose(sp.signal(lambda e: 0.5 * np.ones_like(e)), np.sum(0.5 * (y[:, 1:] + y[:, :-1]) * np.diff(sp.omega), axis=1), rtol=1e-14)
        with pytest.raises(ValueError, match="exactly one"):
            dom.sightline_spectra(ch, photon_energies=e_ph, wavelengths=lam)
        with pytest.raises(ValueError, match="exactly one"):
            dom.sightline_spectra(ch)
        tb = dom.sightline_spectra(ch, table=table, max_steps=50)
        assert tb.intensity.shape == (3, 30) and np.array_equal(tb.edges, table.edges) and np.allclose(tb.photon_energy, table.photon_energy, rtol=1e-15)
        assert tb.band_radiance.shape == (3, 30) and np.allclose(tb.signal(), tb.band_radiance.sum(axis=1), rtol=1e-14) and np.all(tb.signal()[:2] > 0)
        # the pinhole's lines go to the kernel in tile order and come back in pixel order
        img = dom.sightline_spectra(cam, wavelengths=lam)
        assert img.intensity.shape == (13, 9, 9) and img.column.shape == (13, 9) and not np.array_equal(cam.order(), np.arange(13 * 9))
        pick = [0, 3, 4, 8]
        em = dom.sightline_emission(cam, wavelengths=lam[pick])
        assert np.array_equal(np.moveaxis(img.intensity[..., pick], -1, 0), em.intensity)
        assert np.array_equal(np.moveaxis(img.optical_depth[..., pick], -1, 0), em.optical_depth)
        assert np.array_equal(img.column, em.column) and np.array_equal(img.chord, em.chord) and np.array_equal(img.steps, em.steps)
        assert em.intensity.max() > 0 and 0 < (em.steps == 0).sum() < em.steps.size


@pytest.mark.gpu
def test_each_optional_output_asked_for_alone(eng, monkeypatch):
    """13: want = ("column",), ("chord",), ("steps",) on grid A, five planted lines, 5 frequencies: the dict holds that key alone and
    the array has the bits of the call that asks for everything (the three read-backs are separate branches of the host code),
    which is held to the restatement."""
    R = _config((5, 5, True, True, "A"), "nrl", -1, np.float64)
    assert R["ref"]["miss"].tolist() == [False, False, False, False, True] and np.all(R["ref"]["column"][:4] > 0)
    fields = _upload(eng, R)
    try:
        full = _spectra(eng, R, -1, fields=fields)
        _assert_exact(full, R["ref"], "five planted lines")
        _assert_close(full, R["ref"], "five planted lines")
        for name in ("column", "chord", "steps"):
            with monkeypatch.context() as m:  # an array the library does not write holds 0xA5 bytes, not a recycled buffer's
                m.setattr(np, "empty", ts._poisoned(np.empty))
                one = eng.sightline_spectra(*fields, R["o"], R["d"], toward=-1, step=R["step"], max_steps=R["max_steps"],
                                            backlight=R["back"], want=(name,), **_node_kw(R))
            assert list(one) == [name], f"want=({name!r},) returned {list(one)}"
            assert one[name].dtype == full[name].dtype and np.array_equal(one[name], full[name]), f"{name} asked for alone differs"
    finally:
        _close(fields)
