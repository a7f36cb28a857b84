"""Line integrals of a volume along its probing axis (no reference counterpart): sr_volume_project, engine.Volume.project,
projection.Projection and line_integrals.

The maps are trapezoid sums sum_k w_k f_k over the node planes of the probing axis, w = engine.trapezoid_weights(g) on the
volume's float64 node coordinates.  THE BOUNDS here are derived, not measured:

* kernel against the fields read back from the device (Volume.fields(phase=True), the attached float64 arrays), summed in
  np.longdouble: per pixel |d| <= (n_a + 8) * 2^-53 * sum_k |w_k f_k| -- n_a - 1 roundings for a sum in any order, the rest
  for forming f and w*f with or without fused multiply-adds.  No pixel is left out; an absent map is exactly 0.0.
* slabs / regions summed against the whole: twice that bound.
* the areal density against sum_k w_k ne_k of the ORIGINAL ne: sum_k w_k K (2^-46 |m_k| + 2^-50), K = omega^2 1e6 / 5.64e4^2,
  m = n - 1: the 48 bits n - 1 is stored with and the rounding of n = sqrt(1 - eps).
* the identity (a straight ray at v = c through a volume without gradients gathers exactly the line integrals at its launch
  position): the constants ID_TOL, 4 x what test_identity_oracle measures on the CPU (see its docstring).
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LWL = 1064e-9
EPS = 2.0 ** -53
SHAPES = [(2, 2, 2), (7, 3, 5), (8, 5, 7), (9, 4, 33), (17, 13, 6), (40, 70, 66)]
CASES = [(s, a, u) for s in SHAPES for a in "xyz" for u in (True, False)]
IDS = ["x".join(map(str, s)) + f"-{a}-" + ("uni" if u else "rnd") for s, a, u in CASES]
# relative to max |prediction| over the rays of a case: 4 x the worst test_identity_oracle measures (its docstring)
ID_TOL = {"phase": 4 * 1.02e-13, "rotation": 4 * 1.01e-15, "log_amplitude": 4 * 2.89e-12}
N_SPARSE = 4000


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


# ---------------------------------------------------------------- inputs, shared by the CPU and the GPU tests
def _coords(shape, uniform, seed):
    """float32 node coordinates inside +-4 mm: linspace, or sorted random with no two nodes closer than 1e-5 m."""
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(shape):
        half = (4e-3, 3e-3, 3.5e-3)[k]
        if uniform:
            g = np.linspace(-half, half, n)
        else:
            g = np.cumsum(rng.uniform(0.2, 1.0, n))
            g = -half + (g - g[0]) * (2 * half / (g[-1] - g[0]))
        out.append(np.float32(g))
    return out


def _omega():
    return 2 * np.pi * (299792458.0 / LWL)


def _ne_scale():
    return _omega() ** 2 * 1e6 / 5.64e4 ** 2


_FIELDS = {}


def _fields(shape, axis, uniform):
    """The fields of one case, made once: coordinates, n - 1 in [-5e-3, 0], the ne that gives it, kappa with kappa*h <= 1e-3
    per cell, and a Faraday pair (ne_f, B) with a spatially uniform B."""
    key = (shape, axis, uniform)
    if key not in _FIELDS:
        seed = 1000 * SHAPES.index(shape) + 10 * "xyz".index(axis) + int(uniform)
        rng = np.random.default_rng(seed)
        x, y, z = _coords(shape, uniform, seed + 1)
        m = -5e-3 * rng.random(shape)
        h_max = float(np.max(np.diff(np.float64((x, y, z)["xyz".index(axis)])))) / 299792458.0
        kappa = -(1e-3 / h_max) * rng.random(shape)  # absorption: kappa < 0 as the tracer's d(amp) = kappa amp reads it
        ne_f = 1e24 * (0.5 + rng.random(shape))
        B = np.empty(shape + (3,))
        B[...] = (0.3, -0.5, 0.7)
        _FIELDS[key] = dict(x=x, y=y, z=z, m=m, ne=-m * (2.0 + m) * _ne_scale(), kappa=kappa, ne_f=ne_f, B=B,
                            verdet=2.62e-13 * LWL ** 2)
        for v in _FIELDS[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _FIELDS[key]


def _lateral(axis):
    a = "xyz".index(axis)
    return a, [k for k in range(3) if k != a]


def _sum_axis(f, w, a, dtype=np.float64):
    """sum_k w_k f_k along axis a in `dtype`, and sum_k |w_k f_k| (float64)."""
    sh = [1, 1, 1]
    sh[a] = len(w)
    wf = np.asarray(f, dtype) * np.asarray(w, dtype).reshape(sh)
    return wf.sum(axis=a), np.float64(np.abs(wf).sum(axis=a))


def _wide():
    """(dtype of the reference sums, factor on the bound): np.longdouble where it carries more than 60 bits."""
    return (np.longdouble, 1.0) if np.finfo(np.longdouble).eps < 2.0 ** -60 else (np.float64, 2.0)


def _straight_rays(F, axis, n, seed, cells=None):
    """n rays along the probing axis at v = c, launched before the first node plane at random lateral positions inside the
    grid (cells: that many rays in every lateral cell instead).  (s0 (9, N), extent, t_end)."""
    a, (u, v) = _lateral(axis)
    g = [np.float64(F[k]) for k in "xyz"]
    rng = np.random.default_rng(seed)
    if cells:
        lo_u, lo_v = np.meshgrid(g[u][:-1], g[v][:-1], indexing="ij")
        hi_u, hi_v = np.meshgrid(g[u][1:], g[v][1:], indexing="ij")
        t = rng.random((2, cells) + lo_u.shape)
        pu, pv = (lo_u + t[0] * (hi_u - lo_u)).ravel(), (lo_v + t[1] * (hi_v - lo_v)).ravel()
    else:
        pu, pv = rng.uniform(g[u][0], g[u][-1], n), rng.uniform(g[v][0], g[v][-1], n)
        pu[:4] = g[u][0], g[u][-1], g[u][0], g[u][-1]  # rays on the edge lines and through nodes
        pv[:4] = g[v][0], g[v][-1], g[v][-1], g[v][0]
    extent = 5e-3
    s0 = np.zeros((9, len(pu)))
    s0[u], s0[v], s0[a] = pu, pv, -extent
    s0[3 + a] = 299792458.0
    s0[6] = 1.0
    return s0, extent, float(np.sqrt(8.0) * extent / 299792458.0)


def _identity_errors(proj, s0, sf, axis):
    """{quantity: max |traced - sample| / max |sample|} over the rays."""
    a, (u, v) = _lateral(axis)
    out = {}
    for what, got in (("phase", sf[7]), ("rotation", sf[8]), ("log_amplitude", np.log(sf[6]))):
        want = proj.sample(s0[u], s0[v], what)
        assert not np.isnan(want).any() and not np.isnan(got).any(), what
        out[what] = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    return out


# ================================================================ CPU tests
def test_header_ctypes_and_python_signatures(built):
    text = open(os.path.join(ROOT, "include", "synthray.h")).read()
    for k, name in enumerate(("GRAD1", "GRAD2", "NM1", "NE", "KAPPA", "NEB", "MAPS")):
        assert re.search(r"#define\s+SR_PROJ_%s\s+%d\b" % (name, k), text), name
        assert getattr(built, "PROJ_" + name) == k
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+sr_volume_project\s*\(([^;]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 3, m
    res, args = built.SYMBOLS["sr_volume_project"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    assert "project.hip" in open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()

    from synthpy_amd import engine, projection
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    names = lambda f: list(inspect.signature(f).parameters)
    defaults = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}
    assert names(engine.trapezoid_weights) == ["g"] and names(engine.Volume.project) == ["self"]
    assert names(projection.line_integrals) == ["domain", "lwl", "regions"]
    assert defaults(projection.line_integrals) == {"lwl": 1064e-9, "regions": None}
    assert defaults(NewDomain.line_integrals) == {"lwl": 1064e-9, "regions": None}
    assert callable(OldDomain.line_integrals) and callable(projection.Projection.from_integrals)
    for member in ("phase", "fringes", "areal_density", "deflection", "log_amplitude", "transmission", "rotation"):
        assert isinstance(getattr(projection.Projection, member), property), member
    assert names(projection.Projection.sample) == ["self", "p", "q", "what"]
    vol = engine.Volume(None, (3, 4, 5), 2)
    assert vol.verdet == 0.0


def test_argument_checks_come_before_the_device(built):
    """NULL volume or maps: SR_ERR_INVALID with its own text, on a machine with or without a GPU."""
    maps = np.zeros((6, 2, 2))
    have = C.c_uint32(7)
    for v, m in ((None, built.ptr(maps)), (None, None)):
        assert built.lib.sr_volume_project(v, m, C.byref(have)) == -1
        assert "sr_volume_project" in built.last_error() and "NULL" in built.last_error()
    from synthpy_amd import engine

    with pytest.raises(ValueError, match="closed"):
        engine.Volume(None, (3, 4, 5), 2).project()


def test_trapezoid_weights(built):
    from synthpy_amd import engine

    trapz = getattr(np, "trapezoid", None) or np.trapz
    rng = np.random.default_rng(5)
    for n in (2, 3, 8, 9, 33, 70):
        for g in (np.linspace(-1.0, 2.0, n), np.sort(rng.uniform(-3, 3, n))):
            w = engine.trapezoid_weights(g)
            assert w.dtype == np.float64 and w.shape == (n,) and np.all(w > 0)
            assert w[0] == (g[1] - g[0]) / 2 and w[-1] == (g[-1] - g[-2]) / 2
            assert abs(w.sum() - (g[-1] - g[0])) <= 4 * n * EPS * (g[-1] - g[0])
            f = rng.normal(size=(4, n))
            assert np.allclose(f @ w, trapz(f, g, axis=1), rtol=1e-13, atol=1e-13)
    for bad in (np.zeros(1), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            engine.trapezoid_weights(bad)


def test_projection_scaling_and_sample(built):
    from synthpy_amd import projection

    c = 299792458.0
    gu, gv = np.array([0.0, 1.0, 3.0]), np.array([-1.0, 0.0, 0.5, 2.0])
    U, V = np.meshgrid(gu, gv, indexing="ij")
    nm1 = -1e-3 * (1 + U + 2 * V)  # bilinear maps are reproduced exactly by bilinear interpolation
    omega, verdet = 1.7e15, 3e-25
    P = projection.Projection.from_integrals((gu, gv), omega=omega, axes=("x", "z"), verdet=verdet, nm1=nm1, ne=2e22 * (1 + U),
                                             grad=np.stack([1e12 * U, -2e12 * V]), kappa=-1e5 * (1 + U * V), neB=1e23 * V)
    assert P.axes == ("x", "z") and P.shape == (3, 4)
    assert np.array_equal(P.phase, omega / c * nm1) and np.array_equal(P.fringes, P.phase / (2 * np.pi))
    assert np.array_equal(P.areal_density, 2e22 * (1 + U))
    assert P.deflection.shape == (2, 3, 4) and np.array_equal(P.deflection[1], -2e12 * V / c ** 2)
    assert np.array_equal(P.log_amplitude, -1e5 * (1 + U * V) / c)
    assert np.array_equal(P.transmission, np.exp(2 * P.log_amplitude))
    assert np.array_equal(P.rotation, verdet * 1e23 * V)
    p = np.array([0.0, 0.25, 1.0, 2.9, 3.0, 3.0001, -1e-9, 1.0, np.nan])
    q = np.array([-1.0, 0.3, 0.5, 1.9, 2.0, 0.0, 0.0, 2.5, 0.0])
    inside = np.array([1, 1, 1, 1, 1, 0, 0, 0, 0], bool)
    got = P.sample(p, q, "phase")
    assert np.array_equal(np.isnan(got), ~inside)
    assert np.allclose(got[inside], omega / c * -1e-3 * (1 + p + 2 * q)[inside], rtol=1e-14, atol=0)
    assert np.allclose(P.sample(p, q, "rotation")[inside], verdet * 1e23 * q[inside], rtol=1e-14, atol=1e-30)
    d = P.sample(p, q, "deflection")
    assert d.shape == (2, 9) and np.allclose(d[0][inside], 1e12 * p[inside] / c ** 2, rtol=1e-14, atol=1e-30)
    # between nodes a map that is NOT bilinear is interpolated, not evaluated
    Q = projection.Projection.from_integrals((gu, gv), omega=omega, nm1=U ** 2)
    assert np.isclose(Q.sample(np.array([2.0]), np.array([0.0]), "phase")[0], omega / c * 5.0, rtol=1e-14)
    with pytest.raises(ValueError, match="what"):
        P.sample(p, q, "density")
    # an absent map names the flag that provides it
    E = projection.Projection.from_integrals((gu, gv), omega=omega, grad=np.zeros((2, 3, 4)))
    for member, flag in (("phase", "phaseshift"), ("fringes", "phaseshift"), ("areal_density", "phaseshift"),
                         ("log_amplitude", "inv_brems"), ("transmission", "inv_brems"), ("rotation", "B_on")):
        with pytest.raises(ValueError, match=flag + "=True"):
            getattr(E, member)
    assert np.array_equal(E.deflection, np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="shape"):
        projection.Projection.from_integrals((gu, gv), omega=omega, nm1=np.zeros((4, 3)))


def _numpy_projection(F, axis):
    """The Projection of a case's fields by NumPy sums (float64) over the float64 node coordinates."""
    from synthpy_amd import engine, projection

    a, (u, v) = _lateral(axis)
    g = [np.float64(F[k]) for k in "xyz"]
    w = engine.trapezoid_weights(g[a])
    S = lambda f: _sum_axis(f, w, a)[0]
    return projection.Projection.from_integrals((g[u], g[v]), omega=_omega(), axes=("xyz"[u], "xyz"[v]), verdet=F["verdet"],
                                                grad=np.zeros((2, len(g[u]), len(g[v]))), nm1=S(F["m"]), kappa=S(F["kappa"]),
                                                neB=S(F["ne_f"] * F["B"][..., a]))


@pytest.mark.parametrize("shape,axis,uniform", CASES, ids=IDS)
def test_identity_oracle(built, orc, shape, axis, uniform):
    """The identity with the CPU oracle: 4000 straight rays at v = c through a volume without gradients (nref, kappa, ne and a
    uniform B given) gather phase, pol and ln(amp) equal to Projection.sample of NumPy's trapezoid sums at their launch
    positions.  Worst max |traced - sample| / max |sample| measured over all cases of CASES on the CPU this was written on:
        phase 1.02e-13 (the oracle's cancellation in n - 1.0: an absolute rounding of order 2^-53 * omega/c * L, whatever the
        plane count; largest on (2, 2, 2) probed along z, 5e-14 .. 8e-14 elsewhere),
        pol 1.01e-15 (on (40, 70, 66) probed along y; 4e-16 .. 8e-16 on the small shapes),
        ln(amp) 2.89e-12 (RK4's truncation of the exponential at kappa*h <= 1e-3; largest on (2, 2, 2), where every cell is
        at that limit).
    ID_TOL asserts 4 x these; the GPU identity tests use the same constants."""
    F = _fields(shape, axis, uniform)
    z3 = np.zeros(shape, np.float32)
    dom = orc.Domain(F["x"], F["y"], F["z"], z3, z3, z3, _omega(), nref=1.0 + F["m"], kappa=F["kappa"], ne=F["ne_f"], B=F["B"],
                     verdet=F["verdet"])
    s0, extent, t_end = _straight_rays(F, axis, N_SPARSE, 77)
    sf, _ = orc.trace_rk4(dom, s0, 1e-13, t_end, axis, "planes", 1)
    err = _identity_errors(_numpy_projection(F, axis), s0, sf, axis)
    print("identity (oracle)", shape, axis, "uniform" if uniform else "random", {k: f"{e:.2e}" for k, e in err.items()})
    for what, e in err.items():
        assert e <= ID_TOL[what], (what, e, ID_TOL[what])


# ================================================================ GPU tests
def _volume(eng, F, axis, phase=True, kappa=True, faraday=True, ne=None, kappa_arr=None, ne_f=None):
    vol = eng.Volume.from_ne(F["ne"] if ne is None else ne, F["x"], F["y"], F["z"], LWL, axis, phaseshift=phase)
    if kappa or faraday:
        vol.attach_aux((F["kappa"] if kappa_arr is None else kappa_arr) if kappa else None,
                       (F["ne_f"] if ne_f is None else ne_f) if faraday else None, F["B"] if faraday else None, F["verdet"])
    return vol


def _reference(vol, g_a, axis, kappa=None, ne_f=None, B=None):
    """{map: (sum_k w_k f_k in the wide dtype, sum_k |w_k f_k|)} from the fields read back from the device and the float64
    arrays that were attached, w on the float64 node coordinates g_a of the volume's own planes."""
    from synthpy_amd import engine

    a, (u, v) = _lateral(axis)
    wide, _ = _wide()
    w = engine.trapezoid_weights(np.float64(g_a))
    fields = vol.fields(phase=vol.phase)
    ref = {"grad0": _sum_axis(fields[u], w, a, wide), "grad1": _sum_axis(fields[v], w, a, wide)}
    if vol.phase:
        m = np.asarray(fields[3], wide)
        K = wide(vol.omega) ** 2 * wide(1e6) / wide(5.64e4) ** 2
        ref["nm1"] = _sum_axis(m, w, a, wide)
        ref["ne"] = _sum_axis(-m * (2 + m) * K, w, a, wide)
    if kappa is not None:
        ref["kappa"] = _sum_axis(kappa, w, a, wide)
    if ne_f is not None:
        ref["neB"] = _sum_axis(np.asarray(ne_f, wide) * np.asarray(B[..., a], wide), w, a, wide)
    return ref


def _flat(maps):
    """Volume.project()'s dict with the two gradient maps under names of their own; absent maps left out."""
    out = {"grad0": maps["grad"][0], "grad1": maps["grad"][1]}
    out.update({k: maps[k] for k in ("nm1", "ne", "kappa", "neB") if maps[k] is not None})
    return out


def _assert_maps(got, ref, n_a, what, factor=1.0, bound_from=None):
    """Every pixel of every map within factor * (n_a + 8) * 2^-53 * sum |w f| of the reference (bound_from: the reference whose
    sum |w f| gives the bound, when `ref` is another device result)."""
    wide, wf = _wide()
    assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
    for name in sorted(ref):
        want = ref[name][0] if isinstance(ref[name], tuple) else ref[name]
        bound = factor * wf * (n_a + 8) * EPS * (bound_from or ref)[name][1]
        assert got[name].shape == want.shape and got[name].dtype == np.float64, (what, name, got[name].shape, want.shape)
        assert not np.isnan(got[name]).any(), (what, name)
        d = np.float64(np.abs(np.asarray(got[name], wide) - want))
        lit = bound > 0
        worst = float(np.max(d[lit] / bound[lit])) if lit.any() else 0.0
        print(f"{what} {name}: max |d| / bound = {worst:.3f}, max |map| = {float(np.max(np.abs(want))):.6e}")
        assert np.all(d <= bound), (what, name, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,axis,uniform", CASES, ids=IDS)
def test_kernel_against_readback(eng, shape, axis, uniform):
    F = _fields(shape, axis, uniform)
    a, (u, v) = _lateral(axis)
    vol = _volume(eng, F, axis)
    maps = vol.project()
    assert maps["grad"].shape == (2, shape[u], shape[v])
    assert vol.verdet == F["verdet"]
    ref = _reference(vol, F["xyz"[a]], axis, F["kappa"], F["ne_f"], F["B"])
    _assert_maps(_flat(maps), ref, shape[a], f"{shape} {axis}")
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,axis", [((9, 4, 33), "y"), ((8, 5, 7), "z")], ids=["9x4x33-y", "8x5x7-z"])
def test_have_bits_and_absent_maps(eng, shape, axis):
    from synthpy_amd import _ffi as built

    F = _fields(shape, axis, False)
    a, (u, v) = _lateral(axis)
    for phase, kap, far in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1)):
        vol = _volume(eng, F, axis, bool(phase), bool(kap), bool(far))
        raw = np.full((built.PROJ_MAPS, shape[u], shape[v]), np.nan)
        have = C.c_uint32(0xFFFFFFFF)
        built.check(built.lib.sr_volume_project(vol._h, built.ptr(raw), C.byref(have)))
        assert have.value == 0b11 | (0b1100 if phase else 0) | (0b10000 if kap else 0) | (0b100000 if far else 0), bin(have.value)
        for k in range(built.PROJ_MAPS):
            if not have.value >> k & 1:
                assert np.all(raw[k] == 0.0) and not np.signbit(raw[k]).any(), (k, "an absent map is not exactly 0.0")
        maps = vol.project()
        assert [maps[n] is not None for n in ("nm1", "ne", "kappa", "neB")] == [bool(phase), bool(phase), bool(kap), bool(far)]
        assert np.array_equal(raw[:2], maps["grad"])
        ref = _reference(vol, F["xyz"[a]], axis, F["kappa"] if kap else None, F["ne_f"] if far else None, F["B"])
        _assert_maps(_flat(maps), ref, shape[a], f"{shape} {axis} phase={phase} kappa={kap} faraday={far}")
        built.check(built.lib.sr_volume_project(vol._h, built.ptr(raw), None))  # `have` may be left out
        vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("axis", "xyz")
@pytest.mark.parametrize("uniform", (True, False), ids=("uni", "rnd"))
def test_nan_node_poisons_its_own_column_only(eng, axis, uniform):
    shape = (17, 13, 6)
    F = _fields(shape, axis, uniform)
    a, (u, v) = _lateral(axis)
    nodes = {"ne": (9, 5, 3), "kappa": (3, 11, 1), "ne_f": (16, 0, 5)}  # interior, near an edge, a corner
    arr = {k: np.array(F[k]) for k in nodes}
    for k, at in nodes.items():
        arr[k][at] = np.nan
    vol = _volume(eng, F, axis, ne=arr["ne"], kappa_arr=arr["kappa"], ne_f=arr["ne_f"])
    got = _flat(vol.project())
    with np.errstate(invalid="ignore"):
        ref = _reference(vol, F["xyz"[a]], axis, arr["kappa"], arr["ne_f"], F["B"])
    own = lambda at: tuple(at[k] for k in (u, v))
    for name, src in (("nm1", "ne"), ("ne", "ne"), ("kappa", "kappa"), ("neB", "ne_f")):
        mask = np.zeros((shape[u], shape[v]), bool)
        mask[own(nodes[src])] = True
        assert np.array_equal(np.isnan(got[name]), mask), (name, np.argwhere(np.isnan(got[name])))
    for name in ("grad0", "grad1"):
        # the columns whose np.gradient stencil touches the NaN node: what the sums of the fields read back say
        mask = np.isnan(np.float64(ref[name][0]))
        assert 1 <= mask.sum() <= 3 and np.array_equal(np.isnan(got[name]), mask), (name, np.argwhere(np.isnan(got[name])))
    # every other pixel is what it is without the NaN
    wide, wf = _wide()
    for name in ref:
        ok = ~np.isnan(np.float64(ref[name][0]))
        d = np.float64(np.abs(np.asarray(got[name], wide) - ref[name][0]))
        assert np.all(d[ok] <= wf * (shape[a] + 8) * EPS * ref[name][1][ok]), name
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("axis", "xyz")
def test_repeated_call_is_bitwise_equal(eng, axis):
    F = _fields((40, 70, 66), axis, False)
    vol = _volume(eng, F, axis)
    first, second = _flat(vol.project()), _flat(vol.project())
    for name in first:
        assert first[name].tobytes() == second[name].tobytes(), name
    vol.close()


def _cuts3(n):
    """Three slabs of unequal thickness that share their boundary planes: one cell, then about two thirds, then the rest."""
    k2 = max(2, (2 * (n - 1)) // 3)
    return [(0, 1), (1, k2), (k2, n - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,axis,uniform", [c for c in CASES if c[0] in ((9, 4, 33), (17, 13, 6), (40, 70, 66))],
                         ids=[i for c, i in zip(CASES, IDS) if c[0] in ((9, 4, 33), (17, 13, 6), (40, 70, 66))])
def test_slabs_sum_to_the_whole(eng, shape, axis, uniform):
    F = _fields(shape, axis, uniform)
    a, (u, v) = _lateral(axis)
    whole = _volume(eng, F, axis)
    ref = _reference(whole, F["xyz"[a]], axis, F["kappa"], F["ne_f"], F["B"])
    want = _flat(whole.project())
    whole.close()
    total = None
    for lo, hi in _cuts3(shape[a]):
        sl = [slice(None)] * 3
        sl[a] = slice(lo, hi + 1)
        part = lambda f: np.ascontiguousarray(f[tuple(sl)])
        vol = eng.Volume.from_ne_slab(eng.slab_source(F["ne"], a, lo, hi), F["x"], F["y"], F["z"], LWL, axis, lo, hi, phaseshift=True)
        vol.attach_aux(part(F["kappa"]), part(F["ne_f"]), part(F["B"]), F["verdet"])
        maps = _flat(vol.project())
        # a slab on its own is the integral over its own planes
        sref = _reference(vol, F["xyz"[a]][lo:hi + 1], axis, part(F["kappa"]), part(F["ne_f"]), part(F["B"]))
        _assert_maps(maps, sref, hi - lo + 1, f"{shape} {axis} planes {lo}..{hi}")
        total = maps if total is None else {k: total[k] + maps[k] for k in maps}
        vol.close()
    _assert_maps(total, want, shape[a], f"{shape} {axis} three slabs", factor=2.0, bound_from=ref)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,axis,uniform", CASES, ids=IDS)
def test_areal_density_against_ne_itself(eng, shape, axis, uniform):
    from synthpy_amd import projection

    F = _fields(shape, axis, uniform)
    a, (u, v) = _lateral(axis)
    vol = _volume(eng, F, axis, kappa=False, faraday=False)
    g = [np.float64(F[k]) for k in "xyz"]
    P = projection.Projection(vol.project(), vol.omega, vol.verdet, ("xyz"[u], "xyz"[v]), (g[u], g[v]))
    vol.close()
    wide, wf = _wide()
    w = eng.trapezoid_weights(g[a])
    want, _ = _sum_axis(F["ne"], w, a, wide)
    bound, _ = _sum_axis(_ne_scale() * (2.0 ** -46 * np.abs(F["m"]) + 2.0 ** -50), w, a)
    d = np.float64(np.abs(np.asarray(P.areal_density, wide) - want))
    print(f"{shape} {axis} areal density: max |d| / bound = {float(np.max(d / bound)):.3f}, max N_e = {float(np.max(want)):.6e} m^-2")
    assert np.all(d <= bound), float(np.max(d / bound))
    with pytest.raises(ValueError, match="inv_brems=True"):
        P.log_amplitude
    with pytest.raises(ValueError, match="B_on=True"):
        P.rotation


def _plasma(shape, seed):
    """ne, Te, Z, B for the domain classes: n - 1 down to -5e-3, a smooth B."""
    rng = np.random.default_rng(seed)
    m = -5e-3 * rng.random(shape)
    return (-m * (2.0 + m) * _ne_scale(), 50.0 + 100.0 * rng.random(shape), 1.0 + 5.0 * rng.random(shape), rng.normal(size=shape + (3,)))


@pytest.mark.gpu
@pytest.mark.parametrize("dims,axis", [((17, 13, 6), "x"), ((9, 4, 33), "y"), ((9, 4, 33), "z")], ids=["17x13x6-x", "9x4x33-y", "9x4x33-z"])
def test_simulator_domain_regions_equal_the_whole(eng, dims, axis):
    from synthpy_amd import projection
    from synthpy_amd.simulator import propagator
    from synthpy_amd.simulator.domain import ScalarDomain

    a, (u, v) = _lateral(axis)
    ne, Te, Z, B = _plasma(dims, 31)

    def domain(region_count):
        d = ScalarDomain((8e-3, 6e-3, 7e-3), dims, inv_brems=True, phaseshift=True, B_on=True, probing_direction=axis,
                         auto_batching=False, region_count=region_count)
        d.external_ne(ne), d.external_Te(Te), d.external_Z(Z), d.external_B(B)
        return d

    d1, d3 = domain(1), domain(3)
    whole = d1.line_integrals(lwl=LWL)
    assert isinstance(whole, projection.Projection) and whole.axes == ("xyz"[u], "xyz"[v]) and whole.shape == (dims[u], dims[v])
    assert np.array_equal(whole.coords[0], np.float64(getattr(d1, "xyz"[u]))) and whole.verdet == 2.62e-13 * LWL ** 2
    vol = propagator._volume_for(d1, LWL)
    assert whole.omega == vol.omega
    kap, ne_f, Bf, _ = propagator._aux_fields(d1, LWL)
    ref = _reference(vol, getattr(d1, axis), axis, kap, ne_f, Bf)
    _assert_maps(_flat(whole.integrals), ref, dims[a], f"{dims} {axis} whole domain")
    by_regions = d3.line_integrals(lwl=LWL)
    _assert_maps(_flat(by_regions.integrals), _flat(whole.integrals), dims[a], f"{dims} {axis} region_count=3", factor=2.0, bound_from=ref)
    asked = projection.line_integrals(d1, lwl=LWL, regions=3)
    for name, m in _flat(asked.integrals).items():
        assert m.tobytes() == _flat(by_regions.integrals)[name].tobytes(), name
    assert np.allclose(by_regions.phase, whole.phase, rtol=1e-12, atol=0) and by_regions.rotation.shape == whole.shape
    # without the flags the maps are absent and say which flag provides them
    bare = ScalarDomain((8e-3, 6e-3, 7e-3), dims, probing_direction=axis, auto_batching=False)
    bare.external_ne(ne)
    P = bare.line_integrals(lwl=LWL)
    assert np.array_equal(P.deflection, whole.deflection)
    with pytest.raises(ValueError, match="phaseshift=True"):
        P.phase


@pytest.mark.gpu
@pytest.mark.parametrize("axis", "xyz")
def test_legacy_domain_after_calc_dndr(eng, axis):
    from synthpy_amd import projection
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain

    shape = (9, 4, 33)
    a, (u, v) = _lateral(axis)
    x, y, z = _coords(shape, False, 3)
    ne, Te, Z, B = _plasma(shape, 32)
    dom = ScalarDomain(x, y, z, 4e-3, B_on=True, inv_brems=True, phaseshift=True, probing_direction=axis)
    dom.external_ne(ne), dom.external_Te(Te), dom.external_Z(Z), dom.external_B(B)
    with pytest.raises(RuntimeError, match="calc_dndr"):
        dom.line_integrals()
    dom.calc_dndr(LWL)
    P = dom.line_integrals()  # before set_up_interps: the phase and gradient maps only
    assert isinstance(P, projection.Projection) and P.integrals["kappa"] is None and P.integrals["neB"] is None
    dom.set_up_interps()
    P = projection.line_integrals(dom)
    assert P.axes == ("xyz"[u], "xyz"[v]) and P.omega == dom.omega and P.verdet == dom.VerdetConst
    ref = _reference(dom._volume, (x, y, z)[a], axis, dom.kappa(), np.float64(ne), np.float64(B))
    _assert_maps(_flat(P.integrals), ref, shape[a], f"legacy {axis}")
    with pytest.raises(ValueError, match="regions"):
        projection.line_integrals(dom, regions=3)


def _identity_on_the_gpu(eng, shape, axis, uniform, n, cells=None):
    from synthpy_amd import projection

    F = _fields(shape, axis, uniform)
    a, (u, v) = _lateral(axis)
    z3 = np.zeros(shape, np.float32)
    vol = eng.Volume.from_fields(z3, z3, z3, F["x"], F["y"], F["z"], _omega(), axis, nref=1.0 + F["m"])
    vol.attach_aux(F["kappa"], F["ne_f"], F["B"], F["verdet"])
    g = [np.float64(F[k]) for k in "xyz"]
    P = projection.Projection(vol.project(), vol.omega, vol.verdet, ("xyz"[u], "xyz"[v]), (g[u], g[v]))
    assert not P.deflection.any()
    s0, extent, t_end = _straight_rays(F, axis, n, 78, cells)
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    rays.trace(vol, t_end, extent, precision="f64")
    sf = rays.download(rf=False, Jf=False)[0]
    err = _identity_errors(P, s0, sf, axis)
    print("identity (GPU)", shape, axis, "uniform" if uniform else "random", f"{s0.shape[1]} rays, tile segments {rays.tile_segments}",
          {k: f"{e:.2e}" for k, e in err.items()})
    rays.close(), vol.close()
    for what, e in err.items():
        assert e <= ID_TOL[what], (what, e, ID_TOL[what])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,axis,uniform", CASES, ids=IDS)
def test_identity_sparse(eng, shape, axis, uniform):
    _identity_on_the_gpu(eng, shape, axis, uniform, N_SPARSE)


@pytest.mark.gpu
@pytest.mark.parametrize("axis", "xyz")
@pytest.mark.parametrize("uniform", (True, False), ids=("uni", "rnd"))
def test_identity_dense(eng, axis, uniform):
    """16 rays in every lateral cell: dense enough for the library to choose the tile path by itself."""
    _identity_on_the_gpu(eng, (40, 70, 66), axis, uniform, 0, cells=16)
