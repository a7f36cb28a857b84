"""Proton radiography: sr_particles_push (push.hip), engine.push_particles, radiography.ProtonSource / radiograph / Radiograph,
ScalarDomain.proton_radiograph and external_E of both API generations, and E carried by orientation.rotated.

THE REFERENCE for values is `restate_step` / `restate` below: include/synthray.h's rule in NumPy float64, operation for operation
(NumPy's elementwise products and sums are separate calls and cannot fuse; the kernel is compiled with -ffp-contract=off; +, *, /
and sqrt are correctly rounded on both sides and no other function is called).  Bit equality is therefore EXPECTED and every test
prints whether it holds.  What is ASSERTED are bounds derived from the operation count, not measured, which also hold if one
side's sqrt or division were off by one ulp.  The decisions (inside / outside, flags, steps) are asserted equal.

Units: u = 2^-53; a correctly rounded operation errs by 1 u relative, sqrt and / are budgeted at 2 u.  One side's error of ONE
step against the exact value of the rule on the same inputs, with the scales
    U   = max |u| + 2 |hq| sqrt(3) FE       the largest |u| a step can hold (FE, FB: the largest |component| of E, B)
    X   = max |g| + c dt                    the largest coordinate a particle in the box, or one free step outside it, has
    kap = X / h                             h the smallest cell width
* g = sqrt(1 + |u|^2 ic2): |u|^2 3 u (sum of positives), * ic2 4 u, + 1 <= 5 u of the result, sqrt halves it and adds 2: <= 5 u;
  d = hd/g: 7 u.  xm_a = x_a + u_a d: 8 u |u_a d| + 1 u |xm_a| <= 9 u X  (|u_a| d <= c dt/2 <= X).
* weights: w = (p - g[i])/(g[i+1] - g[i]); the node differences are exact (float32 values), p - g[i] rounds once, the division
  twice: dw <= 9 u X/h + 3 u = (9 kap + 3) u =: W u, and 1 - w adds one rounding.  A corner's weight is a product of three factors
  in [0, 1]; summed over the 8 corners the factor errors give 3 * 2 (W + 1) u and the two products per corner 2 u.  The blend puts
  a term through at most 7 roundings (product with the weight, three additions, product with ux / wx, one addition, and the
  corner's widening is exact): dF <= F (6 W + 15) u = F (54 kap + 33) u.  (If the two sides put a midpoint that lies within
  dw of a node into different cells the interpolant's continuity keeps the same bound.)  A UNIFORM field comes back as
  F (1 +- 13 u) whatever the weights' errors, because ux + wx and the four w.. sum to 1 within those roundings.
* the kicks and the rotation, with T = |hq| sqrt(3) FB <= 1/2 in every test (|t| <= T, |s| <= 2|t|, |w| <= 1.5 U): the longest
  chain from u to the new u is um (2 roundings), gm (8), k (2), t (1), |t|^2 (5), 1 + (1), f (2), s (1), w (4), up (4), u (2)
  = 32 roundings of intermediates of magnitude <= 3 U, and t enters up through two cross products with factors <= 3:
  <= 32 * 3 * 3 u U, rounded up to K_CHAIN = 300: du <= [300 U + (54 kap + 34) |hq| sqrt(3) (2 FE + 3 U FB)] u   per component.
* x_a = xm_a + u_a (hd/gn): 9 u X from xm, 8 u of the second half drift (<= X), 1 u of the sum: dx <= 18 u X + hd du.
Two sides: twice these.  Over n steps (tests 3, 5) the errors add, and an error of x changes the field a later step sees by
at most 2 sqrt(3) F dx / h; where that matters (test 5c) the fields are chosen so that the growth over the whole path is below e
and the factor 3 is used.  Uniform B (test 3): the Boris rotation preserves |u| for ANY t, so |u| drifts by the chain's roundings
only, n * 300 u; the angle per step 2 atan|t| carries t's relative error 13 u (blend) + 8 u (k) + n 300 u (gm's drift), plus
the chain: |u_n - R u_0| <= n (600 + theta_step (21 + 300 n)) u |u|.  Uniform E: each half kick errs by 14 u |hq E| + 1 u |u|, and
qm*dt rounds once: |u_n - (u_0 + n (qm dt) E)| <= n u (29 |qm dt E| + 2 max|u|) per component.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

EPS = 2.0 ** -53
LIGHT = 299792458.0
IC2 = 1.0 / (LIGHT * LIGHT)
QM_P = 1.602176634e-19 / 1.67262192369e-27
K_CHAIN = 300.0
N_PART = 1037
UNFINISHED, MISSED = 1, 2


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


# ---------------------------------------------------------------- the restatement
def _locate(g, p):
    """cell, weight, inside per particle on one axis (sr_field_resample's cell / outside lines)."""
    n = len(g)
    inside = (p >= g[0]) & (p <= g[-1])
    q = np.where(inside, p, g[0])
    i = np.clip(np.searchsorted(g, q, side="right") - 1, 0, n - 2)
    w = (q - g[i]) / (g[i + 1] - g[i])
    return i, w, inside


def _gather(F, axes, xm):
    """(3, N) float64: the blend of sr_field_resample's rule at the midpoints xm (3, N), fill 0."""
    (ci, wx, ix), (cj, wy, iy), (ck, wz, iz) = (_locate(axes[a], xm[a]) for a in range(3))
    inside = ix & iy & iz
    ux, uy, uz = 1.0 - wx, 1.0 - wy, 1.0 - wz
    w00, w01, w10, w11 = uy * uz, uy * wz, wy * uz, wy * wz
    out = np.zeros((3, xm.shape[1]))
    f = lambda di, dj, dk, c: np.float64(F[ci + di, cj + dj, ck + dk, c])
    for c in range(3):
        s = [((f(di, 0, 0, c) * w00 + f(di, 0, 1, c) * w01) + f(di, 1, 0, c) * w10) + f(di, 1, 1, c) * w11 for di in (0, 1)]
        out[c] = np.where(inside, ux * s[0] + wx * s[1], 0.0)
    return out


def _n2(a):
    return (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def restate_step(s, E, B, axes, qm, dt, dtype=np.float64, uniform=None):
    """One step of the rule on the states s (6, N): the new states.  E, B: (nx, ny, nz, 3) arrays or None (the line is skipped).
    dtype=np.longdouble with uniform=(E vector or None, B vector or None): the same formulas wide, on uniform fields."""
    with np.errstate(all="ignore"):
        x, u = s[:3].astype(dtype), s[3:].astype(dtype)
        one, two = dtype(1.0), dtype(2.0)
        ic2 = one / (dtype(LIGHT) * dtype(LIGHT)) if dtype is not np.float64 else IC2
        hq, hd = (dtype(qm) * dtype(dt)) * dtype(0.5), dtype(dt) * dtype(0.5)
        g = np.sqrt(one + _n2(u) * ic2)
        xm = x + u * (hd / g)
        if uniform is None:
            Ev = None if E is None else _gather(E, axes, xm)
            Bv = None if B is None else _gather(B, axes, xm)
        else:
            Ev, Bv = (None if v is None else np.asarray(v, dtype)[:, None] * np.ones(s.shape[1], dtype) for v in uniform)
        um = u if Ev is None else u + hq * Ev
        if Bv is None:
            up = um
        else:
            gm = np.sqrt(one + _n2(um) * ic2)
            t = (hq / gm) * Bv
            sv = t * (two / (one + _n2(t)))
            w = um + _cross(um, t)
            up = um + _cross(w, sv)
        un = up if Ev is None else up + hq * Ev
        gn = np.sqrt(one + _n2(un) * ic2)
        xn = xm + un * (hd / gn)
    return np.concatenate([xn, un])


def _inside(s, axes):
    with np.errstate(invalid="ignore"):
        return np.all([(s[a] >= axes[a][0]) & (s[a] <= axes[a][-1]) for a in range(3)], axis=0)


def _detector(s, axis, det_pos, hit_scale):
    b, c = [k for k in range(3) if k != axis]
    with np.errstate(all="ignore"):
        tau = (det_pos - s[axis]) / s[3 + axis]
        hits = np.stack([(s[b] + s[3 + b] * tau) * hit_scale, (s[c] + s[3 + c] * tau) * hit_scale])
    return hits, np.where(np.isfinite(tau) & (tau > 0), 0, MISSED).astype(np.uint8)


def restate(s0, E, B, axes, qm, dt, max_steps, axis, det_pos, hit_scale):
    """The whole rule: sf, hits, steps, flags."""
    s = np.array(s0, np.float64)
    n = s.shape[1]
    steps, active = np.zeros(n, np.int32), np.arange(n)
    for _ in range(max_steps):
        s[:, active] = restate_step(s[:, active], E, B, axes, qm, dt)
        steps[active] += 1
        active = active[_inside(s[:, active], axes)]
        if not len(active):
            break
    hits, flags = _detector(s, axis, det_pos, hit_scale)
    flags[active] |= UNFINISHED
    return s, hits, steps, flags


# ---------------------------------------------------------------- inputs
def _axes():
    """12 x 10 x 9, y non-uniform; float32 node coordinates and their float64 values."""
    x = np.float32(np.linspace(-3e-3, 3e-3, 12))
    y = np.float32(np.cumsum([0.0, 0.3, 0.5, 0.9, 0.4, 0.6, 1.0, 0.35, 0.7, 0.45]) * 1e-3 - 2.4e-3)
    z = np.float32(np.linspace(-2e-3, 2.5e-3, 9))
    return (x, y, z), tuple(np.float64(a) for a in (x, y, z))


AX32, AX = _axes()
DT = 2.4e-12            # a quarter of a typical cell at 5.2e7 m/s
FE, FB = 1e10, 500.0    # field scales [V/m], [T]: |hq| FE = 1.1e6 m/s, T = |hq| sqrt(3) FB * 4 sigma = 0.4


def _fields(dtype, seed=3):
    rng = np.random.default_rng(seed)
    shape = tuple(len(a) for a in AX) + (3,)
    E = (FE * np.clip(rng.standard_normal(shape), -4, 4)).astype(dtype)
    B = (FB * np.clip(rng.standard_normal(shape), -4, 4)).astype(dtype)
    return E, B


def _particles(seed=5):
    """1037 states: random ones inside the box, then the hand-made ones (their indices are returned by name)."""
    rng = np.random.default_rng(seed)
    n = N_PART
    lo, hi = np.array([a[0] for a in AX]), np.array([a[-1] for a in AX])
    s = np.empty((6, n))
    s[:3] = lo[:, None] + rng.random((3, n)) * (hi - lo)[:, None]
    d = rng.standard_normal((3, n))
    s[3:] = 5.4e7 * d / np.sqrt(np.sum(d * d, axis=0))
    k = {}
    # exactly on nodes (first, inner, last) and at rest: the midpoint is the node itself
    k["nodes"] = np.arange(0, 6)
    for j, (a, b, c) in zip(k["nodes"], [(0, 0, 0), (3, 4, 5), (11, 9, 8), (11, 0, 8), (5, 9, 0), (10, 8, 7)]):
        s[:, j] = (AX[0][a], AX[1][b], AX[2][c], 0, 0, 0)
    # exactly on a face, moving along it: the midpoint stays on the face
    k["faces"] = np.arange(6, 12)
    for j, (a, side) in zip(k["faces"], [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]):
        s[a, j] = (lo, hi)[side][a]
        s[3 + a, j] = 0.0
    # just inside a face, moving out: the midpoint is outside
    k["mid_out"] = np.arange(12, 18)
    for j, (a, side) in zip(k["mid_out"], [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]):
        s[a, j] = (lo, hi)[side][a] + (1e-7 if side == 0 else -1e-7)
        s[3:, j] = 0.0
        s[3 + a, j] = -5.4e7 if side == 0 else 5.4e7
    # starting outside: moving in (midpoint inside), moving along (stays outside), moving away
    k["outside"] = np.arange(18, 27)
    for j, (a, off, v) in zip(k["outside"], [(0, -2e-5, 5.4e7), (1, -2e-5, 5.4e7), (2, -2e-5, 5.4e7), (0, 2e-5, -5.4e7),
                                             (0, -1e-3, 0.0), (1, 1e-3, 0.0), (2, -1e-3, 1e3), (0, -1e-3, -5.4e7), (2, 1e-3, 5.4e7)]):
        s[a, j] = (lo[a] if off < 0 else hi[a]) + off
        s[3 + a, j] = v
    k["nan"] = np.arange(27, 30)
    for j, a in zip(k["nan"], (0, 1, 2)):
        s[a, j] = np.nan
    k["slow"] = np.arange(30, 60)  # stay inside for more than 64 steps
    s[3:, k["slow"]] *= 0.01
    return s, k


def _scales(s0, E, B, qm, dt):
    hq = abs(qm * dt) * 0.5
    fe = 0.0 if E is None else float(np.max(np.abs(E)))
    fb = 0.0 if B is None else float(np.max(np.abs(B)))
    U = float(np.nanmax(np.sqrt(np.sum(s0[3:] ** 2, axis=0)))) + 2 * hq * np.sqrt(3) * fe
    X = max(float(np.max(np.abs(a))) for a in AX) + LIGHT * dt
    kap = X / min(float(np.min(np.diff(a))) for a in AX)
    assert hq * np.sqrt(3) * fb <= 0.5, "the bound's derivation needs T <= 1/2"
    du = (K_CHAIN * U + (54 * kap + 34) * hq * np.sqrt(3) * (2 * fe + 3 * U * fb)) * EPS
    dx = 18 * EPS * X + 0.5 * dt * du
    return 2 * du, 2 * dx  # both sides


def _push(eng, E, B, s0, qm, dt, max_steps, axis=2, det_pos=0.1, hit_scale=1e3, image=None, want=("sf", "hits", "steps", "flags")):
    fe = None if E is None else eng.Field(E, *AX32)
    fb = None if B is None else eng.Field(B, *AX32)
    try:
        return eng.push_particles(fe, fb, s0, qm, dt, max_steps, axis, det_pos, hit_scale, image=image, want=want)
    finally:
        for f in (fe, fb):
            if f is not None:
                f.close()


# ================================================================ tests without a device
def test_header_ctypes_and_python_signatures(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "synthray.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sr_particles_push\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 11
    assert re.search(r"#define\s+SR_PUSH_UNFINISHED\s+1", text) and re.search(r"#define\s+SR_PUSH_MISSED\s+2", text)
    assert (built.PUSH_UNFINISHED, built.PUSH_MISSED) == (1, 2)
    p = re.search(r"typedef struct \{([^}]*)\}\s*sr_push_params;", text).group(1)
    assert re.findall(r"(\w+);", p) == [n for n, _ in built.PushParams._fields_] == ["qm", "dt", "max_steps", "axis", "det_pos", "hit_scale"]
    assert C.sizeof(built.PushParams) == 8 + 8 + 4 + 4 + 8 + 8 and built.PushParams.det_pos.offset == 24
    st = re.search(r"typedef struct \{([^}]*)\}\s*sr_push_stats;", text).group(1)
    assert re.findall(r"(\w+)[,;]", st) == [n for n, _ in built.PushStats._fields_]
    assert C.sizeof(built.PushStats) == 8 + 4 * 8
    res, args = built.SYMBOLS["sr_particles_push"]
    assert res is C.c_int and len(args) == 11 and args[3] is C.c_int64
    assert hasattr(built.lib, "sr_particles_push")
    mk = open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()
    assert "push.hip" in mk and "-ffp-contract=off" in mk

    from synthpy_amd import engine, radiography
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.push_particles) == ["E", "B", "s0", "qm", "dt", "max_steps", "axis", "det_pos", "hit_scale", "image", "want"]
    assert names(radiography.radiograph)[:7] == ["domain", "source", "det_pos", "dt", "max_steps", "image", "sort"]
    assert names(NewDomain.proton_radiograph) == names(OldDomain.proton_radiograph)
    assert names(NewDomain.external_E) == names(OldDomain.external_E) == ["self", "E"]


def test_argument_checks_come_before_the_device(built):
    """Every rejected argument is SR_ERR_INVALID with its own text, on a machine with or without a GPU (the checks that need a live
    sr_field -- scalar fields, dtypes, grids -- are exercised on the GPU)."""
    from synthpy_amd import engine

    lib, ptr = built.lib, built.ptr
    s0 = np.zeros((6, 4))

    def call(p, n=4, s=s0, img=None):
        return lib.sr_particles_push(None, None, None if p is None else C.byref(p), n, ptr(s), None, None, None, None, img, None)

    good = lambda **kw: engine.push_params(**{**dict(qm=QM_P, dt=1e-12, max_steps=4, axis=2, det_pos=0.1), **kw})
    assert call(None) == -1 and "NULL" in built.last_error()
    assert call(good(), s=None) == -1 and "NULL" in built.last_error()
    assert call(good(), n=-1) == -1 and "n must not be negative" in built.last_error()
    for dt in (0.0, -1e-12, np.nan, np.inf):
        assert call(good(dt=dt)) == -1 and "dt" in built.last_error(), built.last_error()
    for name in ("qm", "det_pos", "hit_scale"):
        for bad in (np.nan, np.inf, -np.inf):
            assert call(good(**{name: bad})) == -1 and name in built.last_error(), (name, built.last_error())
    for ms in (0, -3):
        assert call(good(max_steps=ms)) == -1 and "max_steps" in built.last_error()
    for axis in (3, -1):
        assert call(good(axis=axis)) == -1 and "axis" in built.last_error()
    assert call(good()) == -1 and "both NULL" in built.last_error()  # every other argument was in order
    assert "sr_particles_push" in built.last_error()

    with pytest.raises(ValueError, match="Field"):
        engine.push_particles(np.zeros((2, 2, 2, 3)), None, s0, QM_P, 1e-12, 4, 2, 0.1)
    with pytest.raises(ValueError, match=r"\(6, n\)"):
        engine.push_particles(None, None, np.zeros((9, 4)), QM_P, 1e-12, 4, 2, 0.1)
    with pytest.raises(ValueError, match="want"):
        engine.push_particles(None, None, s0, QM_P, 1e-12, 4, 2, 0.1, want=("rf",))
    with pytest.raises(ValueError, match="image"):
        engine.push_particles(None, None, s0, QM_P, 1e-12, 4, 2, 0.1, image=np.zeros((4, 4)))


def test_external_E_shape_checks(built):
    from synthpy_amd import radiography
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    new = NewDomain((6e-3, 5e-3, 4e-3), (6, 5, 4))
    old = OldDomain(np.linspace(-3e-3, 3e-3, 6), np.linspace(-2e-3, 2e-3, 5), np.linspace(-2e-3, 2e-3, 4), 3e-3)
    assert new.E is None and getattr(old, "E", None) is None
    for dom in (new, old):
        for shape in ((6, 5, 4), (6, 5, 4, 2), (5, 6, 4, 3), (3, 6, 5, 4)):
            with pytest.raises(ValueError, match="E has shape"):
                dom.external_E(np.zeros(shape))
        E = np.arange(6 * 5 * 4 * 3, dtype=np.float64).reshape(6, 5, 4, 3)
        dom.external_E(E)
        assert dom.E.shape == (6, 5, 4, 3) and np.array_equal(dom.E, E)
    empty = NewDomain(4e-3, 4)
    src = radiography.ProtonSource(3.0, (0, 0, -0.01), "z", half_angle=0.1, n=9)
    with pytest.raises(ValueError, match="neither B"):
        empty.proton_radiograph(src, 0.1)


def test_proton_source(built):
    from synthpy_amd.radiography import M_P, ProtonSource

    Lw = np.longdouble
    for T_MeV, mass, charge in ((14.7, M_P, 1.602176634e-19), (3.0, M_P, 1.602176634e-19), (1.0, 9.1093837015e-31, -1.602176634e-19),
                                (3.5, 4 * M_P, 2 * 1.602176634e-19)):
        src = ProtonSource(T_MeV, (1e-3, -2e-3, -10e-3), "z", half_angle=0.2, n=1000, seed=11, mass=mass, charge=charge)
        g = Lw(1) + Lw(T_MeV) * Lw(1e6) * Lw(1.602176634e-19) / (Lw(mass) * Lw(LIGHT) ** 2)
        u = Lw(LIGHT) * np.sqrt(g * g - 1)
        # gamma: 5 roundings; gamma^2 - 1 loses (gamma^2)/(gamma^2 - 1) of them: for the electron gamma = 2.96, for protons gamma - 1 >= 3e-3
        loss = float(g * g / (g * g - 1))
        assert abs(src.gamma - g) <= 6 * EPS * float(g)
        assert abs(src.u - u) <= (2 + 8 * loss) * EPS * float(u), (T_MeV, float(abs(src.u - u) / u))
        assert src.qm == charge / mass and abs(src.speed - float(u / g)) <= (4 + 8 * loss) * EPS * src.speed
        s = src.states()
        assert s.shape == (6, 1000) and np.all(s[:3] == np.array([1e-3, -2e-3, -10e-3])[:, None])
        norm = np.sqrt(np.sum(s[3:] ** 2, axis=0))
        assert np.all(np.abs(norm - src.u) <= 8 * EPS * src.u)
    p14 = ProtonSource(14.7, (0, 0, 0), "z", half_angle=0.2, n=4)
    assert 5.2e7 < p14.speed < 5.3e7 and 1.0156 < p14.gamma < 1.0157  # 14.7 MeV D-3He protons: 0.175 c

    # seeded repeatability, the cone bound, uniformity in solid angle (cos theta uniform), both senses and every axis
    for axis, toward in (("x", +1), ("y", -1), ("z", +1), (2, -1)):
        a = {"x": 0, "y": 1, "z": 2}.get(axis, axis)
        kw = dict(half_angle=0.3, n=20000)
        d1 = ProtonSource(3.0, (0, 0, 0), axis, toward, seed=4, **kw).directions()
        d2 = ProtonSource(3.0, (0, 0, 0), axis, toward, seed=4, **kw).directions()
        d3 = ProtonSource(3.0, (0, 0, 0), axis, toward, seed=5, **kw).directions()
        assert np.array_equal(d1, d2) and not np.array_equal(d1, d3)
        assert np.all(np.abs(np.sum(d1 * d1, axis=0) - 1) <= 8 * EPS)
        cos_t = toward * d1[a]
        assert np.all(cos_t >= np.cos(0.3) - 4 * EPS) and np.all(cos_t <= 1.0)
        # cos theta uniform on [cos 0.3, 1]: the mean of 20000 draws within 5 standard errors
        width = 1 - np.cos(0.3)
        assert abs(np.mean(cos_t) - (1 - width / 2)) <= 5 * width / np.sqrt(12 * 20000)
        lat = ProtonSource(3.0, (0, 0, 0), axis, toward, half_angle=0.3, n=1000, pattern="lattice")
        dl = lat.directions()
        assert lat.n == 31 * 31 and dl.shape == (3, 961) and np.all(toward * dl[a] >= np.cos(0.3) - 4 * EPS)
        tb = np.delete(dl, a, axis=0) / (toward * dl[a])
        assert np.all(np.abs(tb) <= np.tan(0.3) / np.sqrt(2) * (1 + 8 * EPS))
        assert np.allclose(np.diff(np.unique(np.round(tb[0] / (np.tan(0.3) / np.sqrt(2) / 15), 6))), 1.0)  # a regular lattice
    for bad in (dict(axis="w"), dict(toward=0), dict(half_angle=0.0), dict(half_angle=2.0), dict(n=0), dict(pattern="hex"),
                dict(energy_MeV=-1.0), dict(mass=0.0), dict(position=(0, 0))):
        kw = {**dict(energy_MeV=3.0, position=(0, 0, 0), axis="z", toward=1, half_angle=0.1, n=4), **bad}
        with pytest.raises(ValueError):
            ProtonSource(kw.pop("energy_MeV"), kw.pop("position"), kw.pop("axis"), kw.pop("toward"), **kw)


def test_entry_against_slab_intersection(built):
    """The host's ballistic entry against the slab method in np.longdouble: the entry parameter is the largest of the per-axis
    entry parameters; meets iff it does not exceed the smallest exit parameter (and that is not behind the particle)."""
    from synthpy_amd.radiography import ProtonSource, entry

    Lw = np.longdouble
    lo, hi = np.array([a[0] for a in AX]), np.array([a[-1] for a in AX])
    rng = np.random.default_rng(17)
    parts = []
    for axis, toward, pos in (("z", +1, (0.2e-3, -0.1e-3, -12e-3)), ("x", -1, (9e-3, 0.5e-3, 0.3e-3)), ("y", +1, (0.0, -7e-3, 0.0))):
        parts.append(ProtonSource(14.7, pos, axis, toward, half_angle=0.45, n=400, seed=3).states())
    inside = ProtonSource(14.7, (0.1e-3, 0.2e-3, 0.3e-3), "z", half_angle=0.4, n=50).states()  # a source inside the box stays put
    still = np.zeros((6, 4))
    still[:3] = [[0, 0, 0, 9e-3], [0, 0, 9e-3, 0], [-9e-3, -9e-3, -9e-3, -9e-3]]
    still[5] = 1e7  # along z only: u_x = u_y = 0; two of them pass beside the box
    still[3, 1] = 0.0
    s0 = np.concatenate(parts + [inside, still], axis=1)
    s, meets = entry(s0, lo, hi)
    assert s.shape == s0.shape and np.array_equal(s[3:], s0[3:]) and s0 is not s

    x, u = s0[:3].astype(Lw), s0[3:].astype(Lw)
    with np.errstate(all="ignore"):
        t1, t2 = (Lw(1) * lo[:, None] - x) / u, (Lw(1) * hi[:, None] - x) / u
    ins = (s0[:3] >= lo[:, None]) & (s0[:3] <= hi[:, None])
    t_in = np.where(u == 0, np.where(ins, -np.inf, np.inf), np.minimum(t1, t2))
    t_out = np.where(u == 0, np.where(ins, np.inf, -np.inf), np.maximum(t1, t2))
    t0, t9 = t_in.max(axis=0), t_out.min(axis=0)
    want_meets = t9 >= np.maximum(t0, 0)
    margin = np.abs(t9 - np.maximum(t0, 0)) > 1e-9 * np.abs(t9)  # not within rounding of grazing an edge
    assert margin.sum() > 0.9 * len(margin) and np.array_equal(meets[margin], want_meets[margin])
    n_in = 1200
    assert meets[n_in:n_in + 50].all() and np.array_equal(s[:, n_in:n_in + 50], s0[:, n_in:n_in + 50])
    assert list(meets[-4:]) == [True, True, False, False] and np.array_equal(s[:, ~meets], s0[:, ~meets])
    assert 100 < meets[:n_in].sum() < n_in  # cones wider than the box: some lines pass beside it
    # entry points: t0 * u + x within the roundings of (lo - x)/u (2 u), u*t (1 u) and the sum (1 u), each of magnitude <= |x| + |entry|
    mv = meets & margin & (t0 > 0)
    with np.errstate(invalid="ignore"):
        want = x + u * t0
    tol = 6 * EPS * (np.abs(s0[:3]) + np.abs(np.float64(want)))
    assert np.all(np.abs(s[:3] - want)[:, mv] <= tol[:, mv])
    k = np.argmax(t_in, axis=0)
    face = s[k, np.arange(s.shape[1])]
    assert np.all(((face == lo[k]) | (face == hi[k]))[mv]), "the coordinate of the face crossed last is the face's value exactly"
    assert np.all(_inside(s[:, mv] * (1 - 1e-12), AX))  # on the box, to a part in 1e12


def test_restatement_against_longdouble_gyration(built):
    """Test 3's yardstick: 64 steps of the float64 restatement in a uniform B against the rotation of u_0 about B by
    -n 2 atan|t| in np.longdouble (a positive charge gyrates left-handedly about B), and |u| conserved; uniform E likewise."""
    K = _uniform_case()
    s = K["s0"].copy()
    for _ in range(K["n"]):
        s = restate_step(s, None, K["Bgrid"], AX, QM_P, K["dt"])
    assert np.all(_inside(s, AX))
    _assert_gyration(s, K, "restatement")
    se = K["s0"].copy()
    for _ in range(K["n"]):
        se = restate_step(se, K["Egrid"], None, AX, QM_P, K["dt"])
    assert np.all(_inside(se, AX))
    _assert_uniform_E(se, K, "restatement")
    # one wide step of the rule equals the Rodrigues rotation: the rule itself, not only its float64 rounding
    wide = restate_step(K["s0"], None, None, AX, QM_P, K["dt"], dtype=np.longdouble, uniform=(None, K["B"]))
    one = _rotate(K["s0"][3:], K["B"], K["dt"], 1)
    assert np.all(np.abs(wide[3:] - one) <= 64 * 2.0 ** -64 * np.max(np.abs(one)))


def _uniform_case():
    rng = np.random.default_rng(23)
    n_part = N_PART
    B, E = np.array([400.0, -300.0, 600.0]), np.array([4e9, -7e9, 2.5e9])
    shape = tuple(len(a) for a in AX)
    s0 = np.zeros((6, n_part))
    s0[:3] = rng.uniform(-2e-4, 2e-4, (3, n_part))
    d = rng.standard_normal((3, n_part))
    s0[3:] = 5.4e7 * rng.uniform(0.2, 1.0, n_part) * d / np.sqrt(np.sum(d * d, axis=0))
    return dict(s0=s0, B=B, E=E, Bgrid=np.broadcast_to(B, shape + (3,)).copy(), Egrid=np.broadcast_to(E, shape + (3,)).copy(),
                dt=2.5e-13, n=64)  # 64 steps of at most 1.3e-5 m: nobody leaves the box


def _rotate(u0, B, dt, n):
    """u_0 (3, N) turned about B by -n 2 atan(|hq/gm B|), np.longdouble (Rodrigues)."""
    Lw = np.longdouble
    u0, B = u0.astype(Lw), B.astype(Lw)
    hq = (Lw(QM_P) * Lw(dt)) * Lw(0.5)
    gm = np.sqrt(1 + _n2(u0) / Lw(LIGHT) ** 2)
    Bn = np.sqrt(np.sum(B * B))
    phi = -n * 2 * np.arctan(hq / gm * Bn)
    b = (B / Bn)[:, None]
    return u0 * np.cos(phi) + _cross(b * np.ones_like(u0), u0) * np.sin(phi) + b * np.sum(b * u0, axis=0) * (1 - np.cos(phi))


def _assert_gyration(s, K, who):
    n, u0 = K["n"], K["s0"][3:]
    norm0 = np.sqrt(np.sum(u0.astype(np.longdouble) ** 2, axis=0))
    norm = np.sqrt(np.sum(s[3:].astype(np.longdouble) ** 2, axis=0))
    drift = np.abs(norm - norm0) / norm0
    want = _rotate(u0, K["B"], K["dt"], n)
    theta = 2 * np.arctan(abs(QM_P * K["dt"]) * 0.5 * np.sqrt(np.sum(K["B"] ** 2)))
    err = np.sqrt(np.sum((s[3:] - want) ** 2, axis=0)) / norm0
    b_norm, b_dir = n * K_CHAIN * EPS, n * (2 * K_CHAIN + theta * (21 + K_CHAIN * n)) * EPS
    print(f"{who}: uniform B, {n} steps of {theta:.4f} rad: max | |u| drift | / bound {float(drift.max() / b_norm):.3f}, "
          f"max |u_n - R u_0| / |u| / bound {float(err.max() / b_dir):.3f}")
    assert n * theta > 1.0 and np.all(drift <= b_norm) and np.all(err <= b_dir)


def _assert_uniform_E(s, K, who):
    n, u0 = K["n"], K["s0"][3:]
    Lw = np.longdouble
    kick = n * (Lw(QM_P) * Lw(K["dt"])) * K["E"].astype(Lw)
    want = u0.astype(Lw) + kick[:, None]
    bound = n * EPS * (29 * np.abs(np.float64(kick))[:, None] + 2 * np.maximum(np.abs(u0), np.abs(s[3:])))
    d = np.abs(s[3:] - want)
    print(f"{who}: uniform E, {n} steps: max |u_n - (u_0 + n qm dt E)| / bound {float(np.max(d / bound)):.3f}; "
          f"kick {float(np.max(np.abs(kick))):.3e} m/s")
    assert np.all(d <= bound)


# ================================================================ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("which", ["E", "B", "EB"])
def test_one_step_against_restatement(eng, which, dtype):
    """1: max_steps = 1 for every instantiation, random fields; particles on nodes and faces, midpoints outside, starts outside, NaN."""
    E, B = _fields(dtype)
    E, B = (E if "E" in which else None), (B if "B" in which else None)
    s0, k = _particles()
    out = _push(eng, E, B, s0, QM_P, DT, 1)
    ref = restate_step(s0, E, B, AX, QM_P, DT)
    inside = _inside(ref, AX)
    hits, flags = _detector(ref, 2, 0.1, 1e3)
    flags = flags | np.where(inside, UNFINISHED, 0).astype(np.uint8)
    # the decisions: equal
    assert np.array_equal(out["steps"], np.ones(N_PART, np.int32))
    assert np.array_equal(out["flags"], flags), np.nonzero(out["flags"] != flags)[0][:10]
    assert np.array_equal(np.isnan(out["sf"]), np.isnan(ref))
    st = out["stats"]
    assert (st.unfinished, st.finished, st.missed, st.deposited) == (int(inside.sum()), int((~inside).sum()), int((flags & MISSED > 0).sum()), 0)
    assert st.kernel_ms > 0
    # the hand-made particles did what they were made for
    assert inside[k["nodes"][[1, 5]]].all() and not inside[k["mid_out"]].any() and not inside[k["nan"]].any()  # inner nodes stay in
    assert np.all(np.isnan(ref[:3, k["nan"]]).any(axis=0)) and np.array_equal(ref[3:, k["nan"]], s0[3:, k["nan"]])
    assert np.array_equal(ref[3:, k["mid_out"]], s0[3:, k["mid_out"]]), "a midpoint outside the box sees no field"
    assert inside[k["outside"][:4]].all() and not inside[k["outside"][4:]].any()
    moved = np.any(ref[3:, k["nodes"]] != 0, axis=0)
    assert moved.all() if E is not None else not moved.any()  # at rest on a node: E kicks, B does not
    # the values: within the derived bound, bit equality printed
    du, dx = _scales(s0, E, B, QM_P, DT)
    ok = ~np.isnan(ref)
    d = np.abs(np.where(ok, out["sf"] - ref, 0.0))
    print(f"{which} {np.dtype(dtype).name}: bit-equal sf {np.array_equal(out['sf'], ref, equal_nan=True)}, hits "
          f"{np.array_equal(out['hits'], hits, equal_nan=True)}; max |dx| / bound {float(d[:3].max() / dx):.3g}, max |du| / bound {float(d[3:].max() / du):.3g}")
    assert np.all(d[:3] <= dx) and np.all(d[3:] <= du)


@pytest.mark.gpu
def test_loop_is_the_step_composed(eng):
    """2: a 64-step call equals max_steps = 1 calls chained on their own output, bit for bit: loop, carry, termination."""
    E, B = _fields(np.float64)
    s0, k = _particles()
    fe, fb = eng.Field(E, *AX32), eng.Field(B, *AX32)
    try:
        whole = eng.push_particles(fe, fb, s0, QM_P, DT, 64, 2, 0.1)
        s, steps, active = s0.copy(), np.zeros(N_PART, np.int32), np.arange(N_PART)
        hits, flags = np.empty((2, N_PART)), np.zeros(N_PART, np.uint8)
        for _ in range(64):
            one = eng.push_particles(fe, fb, np.ascontiguousarray(s[:, active]), QM_P, DT, 1, 2, 0.1)
            s[:, active], hits[:, active], flags[active] = one["sf"], one["hits"], one["flags"]
            steps[active] += 1
            active = active[(one["flags"] & UNFINISHED) > 0]
            if not len(active):
                break
    finally:
        fe.close()
        fb.close()
    assert (steps == 1).sum() >= 10 and (steps == 64).sum() >= 20 and len(active) >= 20  # one step; max_steps, still inside
    lateral = (flags & UNFINISHED == 0) & ((s[0] < AX[0][0]) | (s[0] > AX[0][-1]) | (s[1] < AX[1][0]) | (s[1] > AX[1][-1]))
    assert lateral.sum() > 100 and len(np.unique(steps)) > 20
    assert np.array_equal(whole["steps"], steps)
    assert np.array_equal(whole["flags"], flags)
    assert np.array_equal(whole["sf"], s, equal_nan=True)
    assert np.array_equal(whole["hits"], hits, equal_nan=True)
    assert set(np.nonzero(whole["flags"] & UNFINISHED)[0]) == set(active) and whole["stats"].unfinished == len(active)
    # and the NumPy restatement of the whole rule: the same decisions (printed: the same bits)
    rs, rh, rsteps, rflags = restate(s0, E, B, AX, QM_P, DT, 64, 2, 0.1, 1e3)
    print(f"64-step loop against the restatement: bit-equal sf {np.array_equal(rs, whole['sf'], equal_nan=True)}, "
          f"steps equal {np.array_equal(rsteps, steps)}, flags equal {np.array_equal(rflags, flags)}")


@pytest.mark.gpu
def test_uniform_fields(eng):
    """3: uniform B: |u| conserved and the direction turned by n 2 atan|k B| about B; uniform E: u_n = u_0 + n qm dt E."""
    K = _uniform_case()
    out = _push(eng, None, K["Bgrid"], K["s0"], QM_P, K["dt"], K["n"])
    assert np.all(out["steps"] == K["n"]) and np.all(out["flags"] & UNFINISHED)
    _assert_gyration(out["sf"], K, "kernel")
    oute = _push(eng, K["Egrid"], None, K["s0"], QM_P, K["dt"], K["n"])
    assert np.all(oute["steps"] == K["n"]) and np.all(oute["flags"] & UNFINISHED)
    _assert_uniform_E(oute["sf"], K, "kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_detector(eng, axis):
    """4: hits against the restatement, MISSED, the device image against sr_hist2d of the hits, deposited, image-only, repeatability."""
    E, B = _fields(np.float64)
    s0, k = _particles()
    b, c = [a for a in range(3) if a != axis]
    scale = 1024.0  # a power of two: a hit of a particle flying along the axis is its lateral coordinate times 1024, exactly
    # free flights beside the box along the axis, on bin edges of the detector (-8..8 in 32 bins, -6..6 in 24), on its outer
    # edges, and beyond them; then particles moving away from the plane and parallel to it
    edge = [(4.5, 3.0), (-8.0, 0.5), (8.0, -6.0), (8.0, 6.0), (7.5, 6.0), (8.5, 0.0), (0.0, -6.5), (-4.0, 5.5)]
    j0 = 100
    for j, (hx, hy) in enumerate(edge, j0):
        s0[:, j] = 0.0
        s0[b, j], s0[c, j], s0[axis, j], s0[3 + axis, j] = hx / scale, hy / scale, AX[axis][0] - 1e-3, 3e7
    away, par = np.arange(j0 + 8, j0 + 12), np.arange(j0 + 12, j0 + 16)
    s0[:3, away[0]:par[-1] + 1] = 0.0
    s0[c, away[0]:par[-1] + 1] = 5e-3  # beside the box: free flights, so u keeps its zeros
    s0[3:, away[0]:par[-1] + 1] = 0.0
    s0[3 + axis, away] = -3e7
    s0[3 + axis, par] = 0.0
    s0[3 + b, par] = 3e7
    det = 0.05
    img = eng.DetectorImage(eng.IMG_COUNTS, 32, 24, -8.0, 8.0, -6.0, 6.0)
    img2 = eng.DetectorImage(eng.IMG_COUNTS, 32, 24, -8.0, 8.0, -6.0, 6.0)
    fe, fb = eng.Field(E, *AX32), eng.Field(B, *AX32)
    try:
        out = eng.push_particles(fe, fb, s0, QM_P, DT, 64, axis, det, scale, image=img)
        H = img.download()
        only = eng.push_particles(fe, fb, s0, QM_P, DT, 64, axis, det, scale, image=img2, want=())
        H2 = img2.download()
        again = eng.push_particles(fe, fb, s0, QM_P, DT, 64, axis, det, scale)
        # the checks that need live fields: a scalar field, other dtypes, another grid
        sc = eng.Field(E[..., 0], *AX32)
        f32 = eng.Field(E.astype(np.float32), *AX32)
        ax2 = (AX32[0], AX32[1], np.float32(AX32[2] * 1.001))
        og = eng.Field(B, *ax2)
        try:
            for args, word in (((sc, None), "vector"), ((None, sc), "vector"), ((f32, fb), "dtype"), ((fe, og), "grids")):
                with pytest.raises(RuntimeError, match=word):
                    eng.push_particles(*args, s0, QM_P, DT, 4, axis, det, scale)
            cplx = eng.DetectorImage(eng.IMG_COMPLEX, 8, 8, -1.0, 1.0, -1.0, 1.0)
            with pytest.raises(RuntimeError, match="SR_IMG_COUNTS"):
                eng.push_particles(fe, fb, s0, QM_P, DT, 4, axis, det, scale, image=cplx)
            cplx.close()
            empty = eng.push_particles(fe, None, np.zeros((6, 0)), QM_P, DT, 4, axis, det, scale)
            assert empty["sf"].shape == (6, 0) and empty["stats"].finished == 0
        finally:
            for f in (sc, f32, og):
                f.close()
    finally:
        fe.close()
        fb.close()
        img.close()
        img2.close()
    rs, rh, rsteps, rflags = restate(s0, E, B, AX, QM_P, DT, 64, axis, det, scale)
    assert np.array_equal(out["flags"], rflags) and np.array_equal(out["steps"], rsteps)
    assert np.all(out["flags"][away] == MISSED) and np.all(out["flags"][par] == MISSED) and np.all(out["flags"][j0:j0 + 8] == 0)
    assert np.array_equal(out["hits"][:, j0:j0 + 8], np.array(edge).T), "free flights along the axis land on their own lateral coordinates"
    # hits: the restatement's detector line applied to the kernel's own final states is the same operations on the same bits;
    # against the restatement's states the hits carry the states' errors, n steps of the one-step bound, through
    # hit = (x_b + u_b tau) scale: |d hit| <= scale (dx + |tau| du + |u_b / u_a| (dx + |tau| du)) with |u_b / u_a| as it comes out
    own_hits, own_flags = _detector(out["sf"], axis, det, scale)
    okh = np.isfinite(own_hits)  # a particle parallel to the plane has tau = inf and infinite (or NaN) hits on both sides
    assert np.array_equal(np.isinf(out["hits"]), np.isinf(own_hits)) and okh.mean() > 0.9
    print(f"axis {axis}: hits bit-equal to the detector line on the kernel's states {np.array_equal(out['hits'], own_hits, equal_nan=True)}, "
          f"to the restatement's {np.array_equal(out['hits'], rh, equal_nan=True)}; sf bit-equal {np.array_equal(out['sf'], rs, equal_nan=True)}")
    assert np.array_equal(np.isnan(out["hits"]), np.isnan(own_hits))
    with np.errstate(invalid="ignore"):
        dh = np.abs(np.where(okh, out["hits"] - own_hits, 0.0))
    assert np.all(dh <= 8 * EPS * np.abs(np.where(okh, own_hits, 0.0)))
    # the image: sr_hist2d of the downloaded hits with flags == 0, integer for integer
    good = out["flags"] == 0
    want = eng.hist2d(out["hits"][0, good], out["hits"][1, good], 32, 24, -8.0, 8.0, -6.0, 6.0)
    assert H.dtype == np.uint32 and np.array_equal(H, want)
    assert out["stats"].deposited == int(H.sum()) and 0 < H.sum() < good.sum()  # some land outside the detector
    assert H[12 + 6, 16 + 9] >= 1 and H[13, 0] >= 1 and H[0, 31] >= 1 and H[23, 31] >= 2  # the edge hits: right-open bins, last edge closed
    assert np.array_equal(H2, H) and set(only) == {"stats"} and only["stats"].deposited == out["stats"].deposited
    for name in ("sf", "hits", "steps", "flags"):
        assert np.array_equal(out[name], again[name], equal_nan=True), f"a repeated call returned other bits in {name}"
    st = out["stats"]
    assert st.finished + st.unfinished == N_PART and st.unfinished == int((out["flags"] & UNFINISHED > 0).sum())
    assert st.missed == int((out["flags"] & MISSED > 0).sum()) and again["stats"].deposited == 0


# ---------------------------------------------------------------- 5: the API
@pytest.mark.gpu
def test_api_ballistic_projection(eng):
    """5a: B = 0: the hits are the source's straight lines on the detector, the magnification (d_src + d_det)/d_src.
    Bound: u is unchanged by a step in zero field (um = u + hq*0, t = 0); a position takes two half drifts per step, each the
    product u_a d (8 u of it: d carries 7 u, systematically) and one addition (1 u of |x| <= X): after N steps
    dx <= 8 u L + 2 N u X with L the path inside the box (<= its diagonal + a step), + 6 u (|x0| + X) from the host's entry point;
    the detector line turns dx into at most (1 + |u_b/u_a|) dx <= 2 dx (cone < 45 degrees) and adds 8 u |hit|."""
    from synthpy_amd.radiography import ProtonSource
    from synthpy_amd.simulator.domain import ScalarDomain

    dom = ScalarDomain((6e-3, 5e-3, 4e-3), (12, 10, 9))
    dom.external_B(np.zeros((12, 10, 9, 3)))
    src = ProtonSource(14.7, (0.3e-3, -0.2e-3, -10e-3), "z", half_angle=0.15, n=1024, pattern="lattice")
    rad = dom.proton_radiograph(src, 0.09)
    assert rad.magnification == (10e-3 + 0.09) / 10e-3 and rad.hits.shape == (2, 1024) and rad.counts.shape == (256, 256)
    Lw = np.longdouble
    s0 = src.states().astype(Lw)
    tau = (Lw(0.09) - s0[2]) / s0[5]
    want = np.stack([s0[0] + s0[3] * tau, s0[1] + s0[4] * tau]) * 1000
    assert np.all(rad.flags == 0) and rad.steps.max() <= rad.max_steps and rad.stats.unfinished == 0
    met = rad.steps > 0
    assert 100 < met.sum() <= 1024 and rad.stats.finished == met.sum()
    X = 3e-3 + LIGHT * rad.dt
    diag = np.sqrt(6e-3 ** 2 + 5e-3 ** 2 + 4e-3 ** 2) + LIGHT * rad.dt
    dx = EPS * (8 * diag + 2 * rad.steps.max() * X + 6 * (10e-3 + X))
    bound = 1e3 * 2 * dx + 8 * EPS * np.abs(np.float64(want))
    d = np.abs(rad.hits - want)
    print(f"ballistic projection: {int(met.sum())} of 1024 lines meet the box, up to {int(rad.steps.max())} steps; max |d hit| / bound "
          f"{float(np.max(d / bound)):.3f}; max |hit| {float(np.max(np.abs(rad.hits))):.2f} mm")
    assert np.all(d <= bound)
    # the object plane's image: a line through (x, y) of the box's centre plane lands at source + M (x - source)
    at_centre = np.stack([s0[0] + s0[3] * (Lw(0) - s0[2]) / s0[5], s0[1] + s0[4] * (Lw(0) - s0[2]) / s0[5]])
    proj = (np.array([0.3e-3, -0.2e-3])[:, None] + Lw(rad.magnification) * (at_centre - np.array([0.3e-3, -0.2e-3])[:, None])) * 1000
    assert np.all(np.abs(np.float64(proj - want)) <= 1e-12 * np.max(np.abs(np.float64(want))))
    inside_det = ((rad.hits[0] >= rad.edges[0][0]) & (rad.hits[0] <= rad.edges[0][-1]) & (rad.hits[1] >= rad.edges[1][0])
                  & (rad.hits[1] <= rad.edges[1][-1]))
    assert rad.counts.sum() == inside_det.sum() and rad.stats.deposited == (inside_det & met).sum()
    fl = rad.fluence()
    assert np.array_equal(np.isnan(fl), rad.reference_counts() == 0)
    # no field: the radiograph's bins hold what the reference's hold, up to the hits that rounding moves across a bin edge
    assert np.nansum(np.abs(fl - 1) > 0) <= 8


@pytest.mark.gpu
def test_api_test_B_and_sort(eng):
    """5b: ScalarDomain.proton_radiograph is radiograph; sort=True and sort=False give the same per-particle bits."""
    from synthpy_amd import radiography
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain

    dom = ScalarDomain(*AX32, 3e-3, B_on=True)
    dom.test_B(Bmax=400.0)
    src = radiography.ProtonSource(3.0, (0.1e-3, 0.2e-3, -8e-3), "z", half_angle=0.6, n=N_PART, seed=9)
    a = dom.proton_radiograph(src, 0.05, bins=(48, 40))
    b = radiography.radiograph(dom, src, 0.05, bins=(48, 40))
    c = dom.proton_radiograph(src, 0.05, bins=(48, 40), sort=False)
    assert 0 < (a.steps == 0).sum() < N_PART and a.stats.finished == (a.steps > 0).sum()  # a cone wider than the box
    for other, who in ((b, "radiograph"), (c, "sort=False")):
        for name in ("hits", "flags", "steps", "sf", "counts"):
            assert np.array_equal(getattr(a, name), getattr(other, name), equal_nan=True), (who, name)
        assert a.stats.deposited == other.stats.deposited and a.magnification == other.magnification
    # B_z = Bmax x / extent deflects in the x-y plane: the hits differ from the straight lines, |u| does not change
    ref, _ = radiography.project(src.states(), 2, 0.05)
    moved = np.abs(a.hits - ref).max(axis=0)
    assert moved[a.steps > 0].max() > 0.1 and np.all(moved[a.steps == 0] == 0)
    norm = np.sqrt(np.sum(a.sf[3:] ** 2, axis=0))
    assert np.all(np.abs(norm - src.u) <= (8 + K_CHAIN * a.steps) * EPS * src.u)
    assert a.counts.shape == (40, 48) and a.counts.sum() > 0 and a.fluence().shape == (40, 48)


class _Fixed:
    """A source with given states (radiograph reads axis, toward, position, qm, speed, states())."""

    def __init__(self, like, axis, position, s0):
        self.axis, self.toward, self.position, self.qm, self.speed, self.u, self.n = axis, like.toward, np.asarray(position, float), like.qm, like.speed, like.u, s0.shape[1]
        self._s0 = s0

    def states(self):
        return self._s0.copy()


@pytest.mark.gpu
def test_api_rotated_domain(eng):
    """5c: a domain with E and B turned by 90 degrees about y and probed along z' is the original probed along x: view axes
    x' = -z, y' = y, z' = x, so F'[i, j, k] = (-F_z, F_y, F_x)[k, j, n-1-i] -- asserted exactly -- and a particle (p, u) of the
    lab is (-p_z, p_y, p_x), (-u_z, u_y, u_x) in the view; detector (y, z) <-> (x', y') = (-z, y).
    The two runs evaluate the rule with the axes permuted, so sums round differently: each is within N steps of the one-step
    bound of the exact rule, an error of x changing the field later steps see by at most 2 sqrt(3) F dx / h; the fields are small
    enough that this growth over the path stays below e (asserted), and the factor 3 covers it:
    |d state| <= 3 N (one-step bound), both sides already in it; the detector line as in test 4."""
    from synthpy_amd import radiography
    from synthpy_amd.solvers_legacy import full_solver as fs

    n = 12
    x = np.float32((np.arange(n) - (n - 1) / 2) * 2.0 ** -11)  # dyadic, symmetric: R q lands on nodes exactly
    ext = float(x[-1])
    rng = np.random.default_rng(31)
    E = 2e7 * np.clip(rng.standard_normal((n, n, n, 3)), -4, 4)  # a few tenths of a mm of deflection on the detector, and
    B = 0.5 * np.clip(rng.standard_normal((n, n, n, 3)), -4, 4)   # weak enough for `growth` below to stay under 1
    lab = fs.ScalarDomain(x, x, x, ext, probing_direction="z")
    lab.external_ne(np.zeros((n, n, n)))
    lab.external_B(B)
    lab.external_E(E)
    view = lab.rotated(90, about="y")
    turn = lambda F: np.flip(np.transpose(np.stack([-F[..., 2], F[..., 1], F[..., 0]], axis=-1), (2, 1, 0, 3)), axis=0)
    assert np.array_equal(view.B, turn(B)) and np.array_equal(view.E, turn(E)) and view.E.dtype == np.float64
    plain = fs.ScalarDomain(x, x, x, ext)
    plain.external_ne(np.zeros((n, n, n)))
    assert not hasattr(plain.rotated(90, about="y"), "E")  # a domain without E behaves as before

    pos = np.array([-9e-3, 0.2e-3, -0.1e-3])
    src = radiography.ProtonSource(14.7, pos, "x", half_angle=0.12, n=N_PART, seed=2)
    s0 = src.states()
    s0v = np.array([-s0[2], s0[1], s0[0], -s0[5], s0[4], s0[3]])
    det = 0.06
    a = lab.proton_radiograph(src, det, bins=(32, 32))
    b = view.proton_radiograph(_Fixed(src, 2, (-pos[2], pos[1], pos[0]), s0v), det, bins=(32, 32))
    assert np.array_equal(a.steps, b.steps) and np.array_equal(a.flags, b.flags) and a.dt == b.dt
    hb = np.stack([b.hits[1], -b.hits[0]])  # (y, z) of the lab from (x', y') = (-z, y)
    sb = np.array([b.sf[2], b.sf[1], -b.sf[0], b.sf[5], b.sf[4], -b.sf[3]])
    N = int(a.steps.max())
    hq, h, dt = abs(QM_P * a.dt) * 0.5, 2.0 ** -11, a.dt
    fe, fb = float(np.abs(E).max()), float(np.abs(B).max())
    U = src.u + 2 * hq * np.sqrt(3) * fe
    growth = N * N * dt * hq * 2 * np.sqrt(3) * (fe + U * fb) / h  # N steps of du/dx = hq |grad F|, N steps of dx/du = dt
    Xs = ext + LIGHT * dt
    kap = Xs / h
    du = 2 * (K_CHAIN * U + (54 * kap + 34) * hq * np.sqrt(3) * (2 * fe + 3 * U * fb)) * EPS
    dx = 2 * (18 * EPS * Xs + 0.5 * dt * du)
    assert growth < 1.0 and hq * np.sqrt(3) * fb <= 0.5
    bx, bu = 3 * N * dx, 3 * N * du
    assert np.all(np.abs(a.sf[:3] - sb[:3]) <= bx + 8 * EPS * 9e-3) and np.all(np.abs(a.sf[3:] - sb[3:]) <= bu)
    tau = np.abs((det - a.sf[0]) / a.sf[3])
    slope = np.abs(a.sf[4:6] / a.sf[3])
    bh = 1e3 * ((1 + slope) * (bx + 8 * EPS * 9e-3 + tau * bu)) + 8 * EPS * np.abs(a.hits)
    d = np.abs(a.hits - hb)
    print(f"rotated domain: {N} steps at most, growth {growth:.3f}; bit-equal hits {np.array_equal(a.hits, hb)}; "
          f"max |d hit| / bound {float(np.max(d / bh)):.3g}, max |d hit| {float(d.max()):.3e} mm; deflection up to "
          f"{float(np.abs(a.hits - radiography.project(s0, 0, det)[0]).max()):.3f} mm")
    assert np.all(d <= bh)
    assert np.abs(a.hits - radiography.project(s0, 0, det)[0]).max() > 1e-3  # the fields did something
