"""Polarimetry: analyser-weighted intensity images of the traced rays (no reference counterpart).

An analyser at angle beta (from the y axis, in the sense `pol` is measured) passes the component of the exit Jones vector
along (a, b) = (-sin beta, cos beta); a ray's weight in that channel is w = (a Re E_x + b Re E_y)^2 + (a Im E_x + b Im E_y)^2,
or |E_x|^2 + |E_y|^2 without analyser, and image c is the sum of w_c over the rays of a pixel, binned as np.histogram2d bins.

THE BOUND of every intensity comparison here is derived, not measured.  The independent result is
np.histogram2d(x, y, bins=[nx, ny], range=..., weights=w)[0].T on the same post-chain x, y (NaN columns dropped) and the
same E.  Per pixel and channel |dI| <= (n + 16) * 2^-53 * S, with n the rays of the pixel and S the sum of |E_x|^2 + |E_y|^2
over them: n - 1 roundings for a sum in any order, 16 for forming w with or without fused multiply-adds (at most 4 roundings
relative to |a E_x| + |b E_y| <= |E|, squared, twice).  No pixel is left out, and an empty pixel must be exactly 0.0.
"""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

DET = (-9.0, 9.0, -6.75, 6.75)  # the default detector's range [mm] (Lx = 18, Ly = 13.5)
EPS = 2.0 ** -53


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


# ---------------------------------------------------------------- the independent result: numpy
def _weight(E, beta):
    if beta is None:
        return (E[0].real ** 2 + E[0].imag ** 2) + (E[1].real ** 2 + E[1].imag ** 2)
    a, b = -np.sin(beta), np.cos(beta)
    return (a * E[0].real + b * E[1].real) ** 2 + (a * E[0].imag + b * E[1].imag) ** 2


def _numpy_images(x, y, E, analysers, nx, ny, rng=DET):
    """(I (n_ch, ny, nx), n (ny, nx), S (ny, nx)) by np.histogram2d, NaN columns dropped."""
    ok = ~(np.isnan(x) | np.isnan(y))
    x, y, E = x[ok], y[ok], np.asarray(E)[:, ok]
    kw = dict(bins=[nx, ny], range=[[rng[0], rng[1]], [rng[2], rng[3]]])
    I = np.stack([np.histogram2d(x, y, weights=_weight(E, b), **kw)[0].T for b in analysers])
    n = np.histogram2d(x, y, **kw)[0].T
    S = np.histogram2d(x, y, weights=_weight(E, None), **kw)[0].T
    return I, n, S


def _assert_within_bound(I, I_ref, n, S, what, factor=1.0):
    assert I.shape == I_ref.shape and I.dtype == np.float64, (what, I.shape, I_ref.shape)
    bound = factor * (n + 16) * EPS * S
    d = np.abs(I - I_ref)
    lit = np.broadcast_to(S > 0, d.shape)
    worst = float(np.max(d[lit] / np.broadcast_to(bound, d.shape)[lit])) if lit.any() else 0.0
    print(f"{what}: max |dI| / bound = {worst:.3f} over {int(lit.sum())} lit (pixel, channel)s, sum I_ref = {I_ref.sum():.6e}")
    assert not np.isnan(I).any(), what
    assert np.all(d <= bound), (what, worst)
    assert np.all(I[:, n == 0] == 0.0), (what, "an empty pixel is not exactly 0.0")


# ================================================================ CPU tests
def test_header_ctypes_and_python_signatures(built):
    """synthray.h declares the new entries, _ffi holds their prototypes, and every Python signature exists in both API
    generations with the defaults of the design."""
    import ctypes as C

    text = open(os.path.join(ROOT, "include", "synthray.h")).read()
    assert re.search(r"#define\s+SR_IMG_INTENSITY\s+2\b", text) and re.search(r"#define\s+SR_MAX_ANALYSERS\s+4\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("sr_image_create_intensity", 8), ("sr_rays_deposit_intensity", 8), ("sr_intensity2d", 13),
                         ("sr_image_rotation", 5)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        res, args = built.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args, name
    # every entry says that it has no reference counterpart
    assert len(re.findall(r"no reference counterpart", text)) >= 4
    assert built.SYMBOLS["sr_intensity2d"][1][3] is C.c_int64 and built.SYMBOLS["sr_image_rotation"][1][3] is C.c_double
    assert built.MAX_ANALYSERS == 4

    from synthpy_amd import engine, resident
    from synthpy_amd.simulator import diagnostics as diag
    from synthpy_amd.solvers_legacy import rtm_solver as rtm

    assert engine.IMG_INTENSITY == 2

    def defaults(f):
        return {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}

    def names(f):
        return list(inspect.signature(f).parameters)

    assert names(engine.DetectorImage.intensity.__func__)[1:] == ["n_channels", "bin_scale", "pix_x", "pix_y", "Lx", "Ly"]
    d = defaults(engine.DetectorImage.intensity.__func__)
    assert (d["bin_scale"], d["pix_x"], d["pix_y"], d["Lx"], d["Ly"]) == (1, 3448, 2574, 18.0, 13.5)
    assert names(engine.DetectorImage.rotation) == ["self", "ch_plus", "ch_minus", "beta"]
    assert names(engine.RayBundle.deposit_intensity) == ["self", "image", "ops", "analysers", "lds_tiles", "want_stats"]
    assert defaults(engine.RayBundle.deposit_intensity) == {"lds_tiles": True, "want_stats": True}
    assert callable(engine.intensity2d) and callable(resident.DeviceRays.intensity)
    for mod, base in ((diag, diag.Diagnostic), (rtm, rtm.Rays)):
        assert names(base.intensity) == ["self", "analyser", "bin_scale", "pix_x", "pix_y", "clear_mem"]
        assert defaults(base.intensity) == {"analyser": None, "bin_scale": 1, "pix_x": 3448, "pix_y": 2574, "clear_mem": False}
        for cls in ("Shadowgraphy", "Schlieren", "Refractometry", "Interferometry", "Polarimetry"):
            assert getattr(mod, cls).intensity is base.intensity
        po = mod.Polarimetry
        assert issubclass(po, base) and callable(po.two_lens_solve) and callable(po.single_lens_solve)
        assert names(po.polarogram) == ["self", "beta", "bin_scale", "pix_x", "pix_y", "clear_mem"]
        assert defaults(po.polarogram) == {"beta": np.pi / 4, "bin_scale": 1, "pix_x": 3448, "pix_y": 2574, "clear_mem": False}
        assert names(po.rotation) == ["self"]
        assert "min(beta, pi/2 - beta)" in po.rotation.__doc__
    # the analyser's axis, formed once on the host in float64
    ab = engine.analyser_ab([0.3, None, -0.3])
    assert ab.shape == (3, 2) and ab[0, 0] == -np.sin(0.3) and ab[0, 1] == np.cos(0.3) and np.isnan(ab[1]).all()
    assert ab[2, 0] == np.sin(0.3)
    assert np.isnan(engine.analyser_ab(None)).all() and engine.analyser_ab(0.5).shape == (1, 2)
    with pytest.raises(ValueError):
        engine.analyser_ab([0.1] * 5)
    with pytest.raises(ValueError):
        engine.analyser_ab([])


def test_objects_without_Jf_refuse_intensity(built):
    """Diagnostic.intensity on an object built without Jf: ValueError, before any device work."""
    from synthpy_amd.simulator import diagnostics as diag
    from synthpy_amd.solvers_legacy import rtm_solver as rtm

    for make in (lambda: diag.Polarimetry.__new__(diag.Polarimetry), lambda: rtm.Polarimetry.__new__(rtm.Polarimetry)):
        po = make()
        po._dev, po._has_Jf, po._E = None, False, None  # what the constructors leave without a field (no device needed)
        with pytest.raises(ValueError):
            po.intensity()
        with pytest.raises(ValueError):
            po.polarogram()
        with pytest.raises(ValueError):
            po.polarogram(beta=2.0)


@pytest.mark.parametrize("generation", ["simulator", "legacy"])
def test_rotation_formula_recovers_alpha(built, generation):
    """Polarimetry.rotation (the host formula the class shares with its fallback path) on numpy-built H_plus / H_minus of a
    uniform alpha: alpha back to 1e-12 inside |alpha| < min(beta, pi/2 - beta), NaN where both channels are 0."""
    from synthpy_amd.simulator import diagnostics as diag
    from synthpy_amd.solvers_legacy import rtm_solver as rtm

    cls = diag.Polarimetry if generation == "simulator" else rtm.Polarimetry
    rng = np.random.default_rng(3)
    for beta in (0.05, 0.3, np.pi / 4, 1.2):
        lim = min(beta, np.pi / 2 - beta)
        for alpha in (-0.98 * lim, -0.4 * lim, 0.0, 1e-6 * lim, 0.5 * lim, 0.98 * lim):
            A2 = rng.uniform(0.1, 5.0, (6, 8))  # the pixel's summed amp^2: drops out of D
            po = cls.__new__(cls)
            po.H_plus, po.H_minus, po.beta = A2 * np.cos(alpha - beta) ** 2, A2 * np.cos(alpha + beta) ** 2, beta
            po.H_plus[2, 3] = po.H_minus[2, 3] = 0.0
            got = po.rotation()
            assert got.shape == (6, 8) and np.isnan(got[2, 3]) and np.isnan(got).sum() == 1
            ok = ~np.isnan(got)
            assert np.max(np.abs(got[ok] - alpha)) <= 1e-12, (beta, alpha, float(np.max(np.abs(got[ok] - alpha))))
    # beta = pi/4: alpha = asin(D)/2
    from synthpy_amd import engine

    Ip, Im = np.array([0.7, 0.2]), np.array([0.3, 0.8])
    assert np.max(np.abs(engine.rotation_map(Ip, Im, np.pi / 4) - 0.5 * np.arcsin((Ip - Im) / (Ip + Im)))) <= 1e-15
    with pytest.raises(ValueError):
        engine.rotation_map(Ip, Im, 0.0)


@pytest.mark.parametrize("name", ["g5_trace_aux24_z", "g5_trace_aux20_x"])
def test_analyser_weight_is_the_reference_jones_vectors_malus_law(name):
    """The angle convention, pinned to the reference's own Jones vector: |a . E|^2 from Jf_tight equals
    sf_tight[6]^2 cos^2(sf_tight[8] - beta) to 4e-15 relative (reference-run fixtures; their pol lies in [0.096, 0.16]: a
    rotation far from 0, so a wrong sign or axis would show)."""
    g = golden(name)
    sf, Jf = g["sf_tight"], g["Jf_tight"]
    ok = ~np.isnan(sf[6]) & ~np.isnan(Jf[0])
    assert ok.sum() >= 60 and sf[8][ok].min() >= 0.09 and sf[8][ok].max() <= 0.16
    for beta in (0.0, np.pi / 4, -np.pi / 4, 1.0):
        w = _weight(Jf[:, ok], beta)
        malus = sf[6][ok] ** 2 * np.cos(sf[8][ok] - beta) ** 2
        rel = float(np.max(np.abs(w - malus) / malus))
        print(f"{name} beta {beta:+.4f}: max relative difference {rel:.2e}")
        assert rel <= 4e-15, (beta, rel)
    tot = _weight(Jf[:, ok], None)
    assert np.max(np.abs(tot - sf[6][ok] ** 2) / tot) <= 4e-15


def test_intensity_sum_over_ranks_on_the_host_plane(tmp_path, orc):
    """World 2 over gloo, on the CPU: each rank bins its shard of the rays with numpy, RayShardGroup.reduce_host sums the
    (n_ch, ny, nx) float64 images; the sum equals the one-pass image within twice the bound."""
    from test_distributed_gloo import _run_workers

    worker = """
import os, sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
from synthpy_amd.distributed import RayShardGroup
from test_polarimetry import _numpy_images, _assert_within_bound

grp = RayShardGroup(device_images=False, timeout_s=120)
g = np.load(os.path.join({root!r}, "tests", "golden", "g6_optics_extra.npz"))
x, y, E = g["rf"][0] * 1e3, g["rf"][2] * 1e3, g["E"]
an = (np.pi / 4, -np.pi / 4, None)
lo, hi = grp.shard(x.size)
I, _, _ = _numpy_images(x[lo:hi], y[lo:hi], E[:, lo:hi], an, 64, 48)
tot = grp.reduce_host(I, root=0)
if grp.rank == 0:
    I1, n, S = _numpy_images(x, y, E, an, 64, 48)
    assert tot.shape == (3, 48, 64) and tot.dtype == np.float64 and I1.sum() > 0
    _assert_within_bound(tot, I1, n, S, "reduce_host world 2", factor=2.0)
    print("RANK0 OK")
else:
    assert tot is None
grp.close()
"""
    outs = _run_workers(tmp_path, worker, 2)
    assert "RANK0 OK" in outs[0]


# ================================================================ GPU tests
def _chain_cases(eng):
    return {"empty": [], "shadow_two": eng.chain_shadow_two(), "schlieren": eng.chain_schlieren()}


CHANNELS = {"total": (None,), "two": (0.7, None), "pair": (np.pi / 4, -np.pi / 4, None), "four": (0.3, -0.3, 1.0, None)}


@pytest.mark.gpu
@pytest.mark.parametrize("channels", list(CHANNELS))
@pytest.mark.parametrize("chain", ["empty", "shadow_two", "schlieren"])
def test_intensity2d_on_reference_rays(eng, orc, chain, channels):
    """sr_intensity2d on the 3000 reference rays of g6_optics_extra (general complex E) through a chain, against numpy."""
    g = golden("g6_optics_extra")
    an = CHANNELS[channels]
    r, _ = eng.optics(g["rf"], [(eng.OP_SCALE, 1e3)] + _chain_cases(eng)[chain])
    r = np.array(r)
    for nx, ny in ((344, 257), (64, 48)):
        I = eng.intensity2d(r[0], r[2], g["E"], an, nx, ny, *DET)
        I_ref, n, S = _numpy_images(r[0], r[2], g["E"], an, nx, ny)
        assert n.sum() > 100
        _assert_within_bound(I, I_ref, n, S, f"intensity2d {chain} {channels} {nx}x{ny}")
        assert np.array_equal(n, eng.hist2d(r[0], r[2], nx, ny, *DET))


def _bundle_from_reference_rays(eng):
    """A traced bundle whose exit rays are the g6 reference rays' positions and angles: launched from them through an empty
    volume (no deflection), with amplitude, phase and polarisation drawn per ray (a bundle's Jf comes from its trace).  The
    NaN rays of the fixture stay NaN."""
    g = golden("g6_optics_extra")
    rf = g["rf"]
    N, ext = rf.shape[1], 10e-3
    rng = np.random.default_rng(11)
    s0 = np.zeros((9, N))
    t, p = np.tan(rf[1]), np.tan(rf[3])
    norm = np.sqrt(1 + t ** 2 + p ** 2)
    s0[0], s0[1], s0[2] = rf[0], rf[2], -ext
    s0[3], s0[4], s0[5] = eng.c * t / norm, eng.c * p / norm, eng.c / norm
    s0[6], s0[7], s0[8] = rng.uniform(0.2, 1.5, N), rng.uniform(0, 6, N), rng.uniform(-1.5, 1.5, N)
    x = np.linspace(-ext, ext, 16)
    vol = eng.Volume.from_ne(np.zeros((16, 16, 16)), x, x, x, 1064e-9, "z", phaseshift=True)
    rays = eng.RayBundle(N).upload(s0)
    rays.trace(vol, eng.default_t_end(ext), ext, precision="f64")
    return rays, vol


@pytest.mark.gpu
@pytest.mark.parametrize("lds_tiles", [0, 1])
@pytest.mark.parametrize("channels", list(CHANNELS))
def test_bundle_deposit_intensity(eng, orc, channels, lds_tiles):
    """RayBundle.deposit_intensity (k_deposit_intensity, with and without the LDS tile) against numpy on the bundle's own
    rf / Jf; `deposited` equals the counts image's total for the same chain; DetectorImage.rotation equals the host formula."""
    rays, vol = _bundle_from_reference_rays(eng)
    _, rf, Jf = rays.download()
    an = CHANNELS[channels]
    assert np.isnan(rf[0]).sum() >= 10 and np.nanmax(np.abs(Jf)) > 0.2
    for chain, ops in _chain_cases(eng).items():
        r_o = np.array(rays.optics(ops)[0])  # the deposit's own front end, as host arrays
        for kw, (nx, ny) in ((dict(bin_scale=10), (344, 257)), (dict(pix_x=64, pix_y=48), (64, 48))):
            img = eng.DetectorImage.intensity(len(an), **kw)
            assert (img.nx, img.ny, img.n_channels) == (nx, ny, len(an)) and img.nbytes == 8 * len(an) * nx * ny
            _, deposited = rays.deposit_intensity(img, ops, an, lds_tiles=bool(lds_tiles))
            I = img.download()
            I_ref, n, S = _numpy_images(r_o[0], r_o[2], Jf, an, nx, ny)
            _assert_within_bound(I, I_ref, n, S, f"deposit_intensity {chain} {channels} tiles={lds_tiles} {nx}x{ny}")
            cnt = eng.DetectorImage.counts(**kw)
            _, counted = rays.deposit(cnt, ops)
            assert deposited == counted == int(n.sum()) and np.array_equal(cnt.download(), n)
            if channels == "pair":
                got, want = img.rotation(0, 1, np.pi / 4), eng.rotation_map(I[0], I[1], np.pi / 4)
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(got), n == 0)
                assert np.max(np.abs(got - want)[n > 0], initial=0.0) <= 1e-14
            img.zero()
            assert not img.download().any()
    # what the entry refuses
    img = eng.DetectorImage.intensity(2, bin_scale=10)
    with pytest.raises(eng._ffi.SynthrayError, match="channels"):
        rays.deposit_intensity(img, [], (0.1, 0.2, None))
    with pytest.raises(eng._ffi.SynthrayError, match="not been traced"):
        eng.RayBundle(8).deposit_intensity(img, [], (0.1, 0.2))
    with pytest.raises(eng._ffi.SynthrayError, match="intensity"):
        rays.deposit(img, [])
    with pytest.raises(eng._ffi.SynthrayError):
        eng.DetectorImage.intensity(5)


def _g5_domain(name, generation):
    """(solve() -> (rf, Jf), the diagnostics module, a Polarimetry factory) on a g5 volume with B and kappa attached."""
    g = golden(name)
    ext, pd, x, lwl = float(g["extent"]), str(g["pdir"]), g["x"], float(g["lwl"])
    if generation == "legacy":
        from synthpy_amd.solvers_legacy import full_solver as fs, rtm_solver as rtm

        dom = fs.ScalarDomain(x, x, x, ext, B_on=True, inv_brems=True, phaseshift=True, probing_direction=pd)
        dom.external_ne(g["ne"])
        dom.external_B(g["B"])
        dom.external_Te(g["Te"])
        dom.external_Z(g["Z"])
        dom.calc_dndr(lwl)
        return g, dom, (lambda s0: dom.solve(s0, return_E=True)), rtm, (lambda rf, Jf: rtm.Polarimetry(rf, Jf))
    from synthpy_amd.simulator import diagnostics as diag, domain as d, propagator as p

    dom = d.ScalarDomain(2 * ext, len(x), B_on=True, inv_brems=True, phaseshift=True, probing_direction=pd)
    assert np.array_equal(dom.x, np.float32(x))
    dom.external_ne(g["ne"])
    dom.external_B(g["B"])
    dom.external_Te(g["Te"])
    dom.external_Z(g["Z"])
    return g, dom, (lambda s0: p.solve(s0, dom, ext, return_E=True, lwl=lwl)[:2]), diag, (lambda rf, Jf: diag.Polarimetry(lwl, rf, Jf))


def _g5_oracle(orc, g):
    x, ext, pd = g["x"], float(g["extent"]), str(g["pdir"])
    dom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), True, g["Te"], g["Z"], g["B"])
    sf, _ = orc.trace_rk4(dom, g["s0"], (x[1] - x[0]) / orc.c, orc.default_t_end(ext), pd, "planes", 1)
    rf, Jf = orc.ray_to_jones(sf, ext, pd, "legacy")
    return sf, rf, Jf


# the float64 build's distance from the oracle on aux traces (test_gpu_parity: positions 1e-13 m in the volume, smoke():
# 1e-12 m / 1e-10 rad on the exit plane); on the detector of the M = 1 telescope that is 1e-9 mm, and 1e-10 rad over the
# chain's 1600 mm of legs bounds what the angle adds before the image plane cancels it
RF_POS_TOL, RF_ANG_TOL = 1e-12, 1e-10
EDGE_TOL_MM = 1e3 * RF_POS_TOL + 1600 * RF_ANG_TOL


def _oracle_polarogram_inputs(orc, g, bin_scale=10):
    """Oracle exit rays through the two-lens chain, and which rays sit within EDGE_TOL_MM of a bin edge (their bin may flip)."""
    sf_o, rf_o, Jf_o = _g5_oracle(orc, g)
    r_o, _ = orc.optics(orc.m_to_mm(rf_o), orc.chain_shadow_two())
    nx, ny = 3448 // bin_scale, 2574 // bin_scale
    near = np.zeros(r_o.shape[1], bool)
    for row, (lo, hi, nb) in ((0, (DET[0], DET[1], nx)), (2, (DET[2], DET[3], ny))):
        edges = np.linspace(lo, hi, nb + 1)
        v = r_o[row]
        j = np.clip(np.searchsorted(edges, v), 1, nb)
        with np.errstate(invalid="ignore"):
            near |= (np.abs(v - edges[j - 1]) <= EDGE_TOL_MM) | (np.abs(v - edges[j]) <= EDGE_TOL_MM)
    return sf_o, rf_o, Jf_o, r_o, near, nx, ny


@pytest.mark.parametrize("name", ["g5_trace_aux24_z", "g5_trace_aux20_x"])
def test_edge_exclusion_cap_holds_on_the_oracle(orc, name):
    """CPU: at most 2 % of the g5 rays lie within the rf tolerance of a bin edge of the bin_scale=10 detector (the cap the
    end-to-end GPU test asserts), and the rays land on the detector."""
    g = golden(name)
    *_, r_o, near, nx, ny = _oracle_polarogram_inputs(orc, g)
    assert near.sum() <= 0.02 * near.size, (int(near.sum()), near.size)
    assert np.histogram2d(r_o[0], r_o[2], bins=[nx, ny], range=[DET[:2], DET[2:]])[0].sum() >= 0.9 * near.size


@pytest.mark.gpu
@pytest.mark.parametrize("generation", ["legacy", "simulator"])
@pytest.mark.parametrize("name", ["g5_trace_aux24_z", "g5_trace_aux20_x"])
def test_polarogram_end_to_end_from_s0(eng, orc, name, generation):
    """solve(return_E=True) -> Polarimetry.two_lens_solve() -> polarogram(bin_scale=10) on a volume with B and kappa, against
    numpy on the ORACLE's rf / Jf from the same s0.  A ray within the rf tolerance of a bin edge is binned where the GPU's own
    coordinate puts it (at most 2 % of the rays); its weight is the oracle's all the same."""
    g, dom, solve, mod, make = _g5_domain(name, generation)
    rf, Jf = solve(np.ascontiguousarray(g["s0"]))
    sf_o, rf_o, Jf_o, r_o, near, nx, ny = _oracle_polarogram_inputs(orc, g)
    dpos, dang = np.max(np.abs(rf[0::2] - rf_o[0::2])), np.max(np.abs(rf[1::2] - rf_o[1::2]))
    dJ = np.max(np.abs(Jf - Jf_o))
    print(f"{name} {generation}: max|dx| {dpos:.2e} m, max|dtheta| {dang:.2e} rad, max|dJf| {dJ:.2e}")
    assert dpos <= RF_POS_TOL and dang <= RF_ANG_TOL
    assert dJ <= 1e-9 * np.max(np.abs(sf_o[7])) * np.max(np.abs(sf_o[6]))  # the phase's tolerance (1e-9 of its maximum) times amp
    assert near.sum() <= 0.02 * near.size
    po = make(rf, Jf)
    assert po.on_device
    po.two_lens_solve()
    po.polarogram(bin_scale=10)
    assert po.on_device and po._rf is None, "polarogram() brought the rays to the host"
    assert po.beta == np.pi / 4 and po.I.shape == (3, ny, nx) and po.H_plus.shape == (ny, nx)
    assert po.xedges.shape == (nx + 1,) and po.yedges.shape == (ny + 1,) and po.xedges[0] == -9 and po.yedges[-1] == 6.75
    r_g = np.asarray(po.rf)
    x_ref, y_ref = np.where(near, r_g[0], r_o[0]), np.where(near, r_g[2], r_o[2])
    I_ref, n, S = _numpy_images(x_ref, y_ref, Jf_o, (np.pi / 4, -np.pi / 4, None), nx, ny)
    assert n.sum() >= 0.9 * near.size
    _assert_within_bound(np.stack([po.H_plus, po.H_minus, po.H_total]), I_ref, n, S, f"polarogram {name} {generation}")
    # the rotation map shows the rays' Faraday rotation: single-ray pixels give that ray's pol
    a = po.rotation()
    assert np.array_equal(np.isnan(a), n == 0)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(x_ref) < 9) & (np.abs(y_ref) < 6.75)
    ix = np.searchsorted(np.linspace(DET[0], DET[1], nx + 1), x_ref[ok], "right") - 1
    iy = np.searchsorted(np.linspace(DET[2], DET[3], ny + 1), y_ref[ok], "right") - 1
    single = n[iy, ix] == 1
    assert single.sum() > 10 and np.max(np.abs(a[iy, ix][single] - sf_o[8][ok][single])) <= 1e-9
    # pickling takes the rays to the host, as for the other classes
    import pickle

    po2 = pickle.loads(pickle.dumps(po))
    assert not po2.on_device and np.array_equal(po2.H_plus, po.H_plus)
    po2.polarogram(bin_scale=10)
    _assert_within_bound(po2.I, I_ref, n, S, f"polarogram after pickling {name} {generation}")


def _uniform_faraday(N=100_000, n=32, ext=5e-3, lwl=1064e-9, ne0=1e25, Bz=3.4):
    from synthpy_amd.solvers_legacy import full_solver as fs

    x = np.linspace(-ext, ext, n)
    dom = fs.ScalarDomain(x, x, x, ext, B_on=True, probing_direction="z")
    dom.external_ne(np.full((n, n, n), ne0))
    B = np.zeros((n, n, n, 3))
    B[..., 2] = Bz
    dom.external_B(B)
    dom.calc_dndr(lwl)
    np.random.seed(4)
    s0 = fs.init_beam(N, 4e-3, 0.0, ext, "circular", "z")
    return dom, s0, 2.62e-13 * lwl ** 2 * ne0 * Bz * (float(dom.z[-1]) - float(dom.z[0]))


@pytest.mark.gpu
def test_known_answer_uniform_faraday_rotation(eng, orc):
    """32^3, uniform n_e = 1e25 and B = (0, 0, 3.4 T), 1064 nm, z probing, 1e5 rays without divergence: every ray exits with
    pol = 2.62e-13 lambda^2 n_e B (z[-1] - z[0]) (float32 node coordinates; RK4 is exact on a constant integrand) to 1e-6,
    rotation() gives the rays' own sf[8] on every lit pixel to 1e-12 (D = sin 2 alpha at beta = pi/4, alpha ~ 0.1: conditioning
    ~ 1), and without inverse bremsstrahlung H_total is the counts image as float, within the bound."""
    from synthpy_amd.solvers_legacy import rtm_solver as rtm

    dom, s0, expected = _uniform_faraday()
    rf, Jf = dom.solve(s0, return_E=True)
    pol = dom.sf[8]
    assert 0.09 < expected < 0.11 and not np.isnan(pol).any()
    print(f"pol: expected {expected:.15e}, got {pol.mean():.15e}, spread {pol.max() - pol.min():.2e}")
    # the same pol on every ray: 31 steps x 4 stages of float64 roundings on values <= 0.1 (1.4e-15) plus as many roundings
    # of the bilinear blend of a uniform field, bounded by 1e-14
    assert pol.max() - pol.min() <= 1e-14
    assert np.max(np.abs(pol - expected)) <= 1e-6 * expected
    po = rtm.Polarimetry(rf, Jf)
    po.two_lens_solve()
    po.polarogram(bin_scale=4)
    sh = rtm.Shadowgraphy(rf)
    sh.two_lens_solve()
    sh.histogram(bin_scale=4)
    lit = sh.H > 0
    assert lit.sum() > 10_000 and sh.H.sum() == s0.shape[1]
    a = po.rotation()
    assert np.array_equal(~np.isnan(a), lit)
    err = float(np.max(np.abs(a[lit] - pol.mean())))
    print(f"rotation(): max |alpha - pol| over {int(lit.sum())} lit pixels = {err:.2e}")
    assert err <= 1e-12
    S = sh.H  # amp = 1: |E|^2 = 1 per ray
    _assert_within_bound(po.H_total[None], sh.H[None], sh.H, S, "H_total against the counts image")


@pytest.mark.gpu
@pytest.mark.parametrize("generation", ["legacy", "simulator"])
def test_attenuation_image_and_fallback(eng, orc, generation):
    """With inverse bremsstrahlung on, Shadowgraphy(...).intensity() differs from histogram() and equals numpy with weights
    |E|^2; and after a write to po.rf the image equals numpy on the edited array (the host path: sr_intensity2d)."""
    g, dom, solve, mod, make = _g5_domain("g5_trace_aux24_z", generation)
    rf, Jf = solve(np.ascontiguousarray(g["s0"]))
    sh = mod.Shadowgraphy(rf, Jf) if generation == "legacy" else mod.Shadowgraphy(float(g["lwl"]), rf, Jf)
    assert sh.on_device
    sh.two_lens_solve()
    sh.histogram(bin_scale=10)
    H = sh.H.copy()
    sh.intensity(bin_scale=10)
    assert sh.on_device and np.array_equal(sh.H, H), "intensity() touched .H"
    nx, ny = 344, 257
    r = np.asarray(sh.rf)
    I_ref, n, S = _numpy_images(r[0], r[2], np.asarray(Jf), (None,), nx, ny)
    assert sh.I.shape == (1, ny, nx) and np.array_equal(n, H)
    _assert_within_bound(sh.I, I_ref, n, S, f"attenuation image {generation}")
    assert np.max(np.abs(sh.I[0] - H)[H > 0] / H[H > 0]) > 1e-3, "inverse bremsstrahlung left no mark on the intensity image"
    # one angle, and a sequence with None inside
    sh.intensity(analyser=0.3, bin_scale=10)
    _assert_within_bound(sh.I, _numpy_images(r[0], r[2], np.asarray(Jf), (0.3,), nx, ny)[0], n, S, f"one analyser {generation}")
    # an object built without Jf
    bare = mod.Shadowgraphy(rf) if generation == "legacy" else mod.Shadowgraphy(float(g["lwl"]), rf)
    bare.two_lens_solve()
    with pytest.raises(ValueError):
        bare.intensity()
    # fallback: the caller writes to the chain's output (mm)
    po = make(rf, Jf)
    po.two_lens_solve()
    po.rf[0, ::7] += 1e-3
    edited = np.array(po.rf)
    assert not np.array_equal(edited, r, equal_nan=True)
    po.polarogram(bin_scale=10)
    assert not po.on_device
    an = (np.pi / 4, -np.pi / 4, None)
    I_ref, n, S = _numpy_images(edited[0], edited[2], np.asarray(Jf), an, nx, ny)
    _assert_within_bound(po.I, I_ref, n, S, f"fallback on the edited rf {generation}")
    # a bundle that is gone: the same answer from the host arrays
    po3 = make(rf, Jf)
    po3.two_lens_solve()
    po3._to_host()
    po3.polarogram(bin_scale=10)
    I_ref, n, S = _numpy_images(r[0], r[2], np.asarray(Jf), an, nx, ny)
    _assert_within_bound(po3.I, I_ref, n, S, f"host path {generation}")


@pytest.mark.gpu
def test_two_halves_sum_to_the_one_pass_image(eng, orc):
    """Two halves of one bundle deposited into DetectorImage.intensity and summed through RayShardGroup(world=1).reduce_image
    (one rank: both halves land in the rank's image, the reduce takes the new kind and leaves it) against the one-pass image
    of the whole bundle, within twice the bound."""
    from synthpy_amd.distributed import RayShardGroup

    g = golden("g5_trace_aux24_z")
    ext, x = float(g["extent"]), g["x"]
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    vol.attach_aux(orc.kappa(g["ne"], g["Te"], g["Z"], orc.omega(float(g["lwl"]))), g["ne"], g["B"], orc.verdet(float(g["lwl"])))
    s0 = np.tile(g["s0"], (1, 40))
    s0[0] += np.linspace(-2e-4, 2e-4, s0.shape[1])
    N, an, ops = s0.shape[1], (np.pi / 4, -np.pi / 4, None), eng.chain_shadow_two()
    whole = eng.RayBundle(N).upload(s0)
    whole.trace(vol, eng.default_t_end(ext), ext, precision="f64")
    one = eng.DetectorImage.intensity(3, bin_scale=10)
    whole.deposit_intensity(one, ops, an)
    halves = eng.DetectorImage.intensity(3, bin_scale=10)
    for part in (s0[:, : N // 2], s0[:, N // 2:]):
        b = eng.RayBundle(part.shape[1]).upload(np.ascontiguousarray(part))
        b.trace(vol, eng.default_t_end(ext), ext, precision="f64")
        b.deposit_intensity(halves, ops, an)
    grp = RayShardGroup(rank=0, world=1)
    grp.reduce_image(halves)
    _, rf, Jf = whole.download()
    r_o, _ = orc.optics(orc.m_to_mm(rf), orc.chain_shadow_two())
    I_ref, n, S = _numpy_images(r_o[0], r_o[2], Jf, an, 344, 257)
    assert n.sum() > 0.9 * N
    _assert_within_bound(one.download(), I_ref, n, S, "one pass")
    _assert_within_bound(halves.download(), one.download(), n, S, "two halves + reduce_image", factor=2.0)


@pytest.mark.gpu
def test_full_detector_at_size(eng, orc):
    """1e6 rays x 256^3 with B_on, polarogram at bin_scale=1 (3448 x 2574 x 3 channels = 213 MB): the class's image (LDS
    tiles) and the same deposit without tiles agree within twice the bound, and sum(H_total) = sum |E|^2 of the deposited
    rays to N 2^-53 relative."""
    from synthpy_amd.solvers_legacy import full_solver as fs, rtm_solver as rtm

    n, ext, lwl, N = 256, 5e-3, 1064e-9, 1_000_000
    x = np.linspace(-ext, ext, n)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij", sparse=True)
    ne = 1e25 * np.exp(-(X ** 2 + Y ** 2 + Z ** 2) / (2e-3) ** 2) + 2e24
    B = np.zeros((n, n, n, 3))
    B[..., 2] = 3.0 * (1 + X / ext)
    dom = fs.ScalarDomain(x, x, x, ext, B_on=True, probing_direction="z")
    dom.external_ne(ne)
    dom.external_B(B)
    dom.calc_dndr(lwl)
    np.random.seed(2)
    s0 = fs.init_beam(N, 4e-3, 5e-5, ext, "circular", "z")
    rf, Jf = dom.solve(s0, return_E=True)
    po = rtm.Polarimetry(rf, Jf)
    po.two_lens_solve()
    po.polarogram()
    assert po.on_device and po.I.shape == (3, 2574, 3448)
    tiled = po.I
    img = eng.DetectorImage.intensity(3)
    assert img.nbytes == 3 * 2574 * 3448 * 8
    an = (np.pi / 4, -np.pi / 4, None)
    _, deposited = po._dev.bundle.deposit_intensity(img, po._dev.ops, an, lds_tiles=False)
    plain = img.download()
    img.close()
    r = np.asarray(po.rf)
    ok = ~np.isnan(r[0]) & (np.abs(r[0]) <= 9) & (np.abs(r[2]) <= 6.75)
    assert deposited == int(ok.sum()) > 0.9 * N
    w = _weight(np.asarray(Jf)[:, ok], None)
    nn = np.histogram2d(r[0][ok], r[2][ok], bins=[3448, 2574], range=[DET[:2], DET[2:]])[0].T
    S = np.histogram2d(r[0][ok], r[2][ok], bins=[3448, 2574], range=[DET[:2], DET[2:]], weights=w)[0].T
    _assert_within_bound(tiled, plain, nn, S, "LDS tiles against global atomics", factor=2.0)
    import math

    tot, want = math.fsum(tiled[2].ravel()), math.fsum(w)
    print(f"sum H_total {tot:.15e}, sum |E|^2 {want:.15e}, relative {abs(tot - want) / want:.2e} (allowed {N * EPS:.2e})")
    assert abs(tot - want) <= N * EPS * want
    a = po.rotation()
    assert np.array_equal(~np.isnan(a), nn > 0) and 0.0 < np.nanmax(np.abs(a)) < np.pi / 4
