"""Sightlines: sr_field_sightlines (sightlines.hip), engine.sightlines, sightlines.PinholeCamera / PointBacklighter / Chords /
sightline_emission and ScalarDomain.sightline_emission of both API generations.

THE REFERENCE for values is `restate` below: include/synthray.h's rule in NumPy float64, operation for operation.  It has two
halves, and they are held to different standards.

* The GEOMETRY (the clip, chord, the step count, the sample positions) and the trilinear GATHER (cell, weights, blend, and so
  column = sum ne*h) use only +, -, *, /, sqrt, ceil and comparisons: correctly rounded on both sides, in the same order, never
  fused (-ffp-contract=off; NumPy's elementwise calls cannot fuse).  chord, steps, column and the set of missed lines are asserted
  BIT-EQUAL.  So the blended (ne, Te, Z) a node gets, and h, are the same bits on both sides.
* I and tau go through exp, expm1 and log of another library: a BUDGET, derived from the operation count, never measured.
  Units: u = 2^-53; a correctly rounded operation errs by at most 1 u relative, a library function by 1 ulp = 2 u
  (tests/test_emission.py says where that figure comes from).  One side's error against the exact value of the rule on the same
  inputs, first order:
    - the node: E_alpha = 21 u and E_S = (4 + x) u, x = e_ph/Te, for the NRL node (tests/test_emission.py); for a table
      E_alpha = E_l(LA) + 7 and E_S = 4 + x [+ E_l(LE) + E_l(LA) + |le - la| + 3] (tests/test_table_emission.py, whose `_node`
      computes them per node and is called here per sample).  A dark sample has both 0.  Unlike the grid marches there is no
      averaging of two nodes: a sample IS a node.
    - a sample: dtau = alpha*h, h the same bits on both sides: ea = E_alpha + 1.  a = exp(-dtau): (2 + ea dtau) u.
      -expm1(-dtau), condition number <= 1: (ea + 2) u.  b = S * that: (es + ea + 3) u, es = E_S.
    - a line, marched SEQUENTIALLY (the header fixes the order): I = sum_k term_k, term_k = b_k prod_{j after k} a_j, all terms
      >= 0.  The update I <- I*a + b puts every earlier term through one product and one sum, 2 u, and a's (2 + ea dtau) u; the
      new term through the sum, 1 u.  With N_k samples after k and W_k = sum_{j after k} ea_j dtau_j, one side:
      (es_k + ea_k + 4 + 4 N_k + W_k) u term_k; the backlight is term 0 with es + ea + 4 = 0.  Both sides:
          budget_I = 2 u sum_k term_k (es_k + ea_k + 4 + 4 N_k + W_k)       + a floor of 4 n 2^-1074 for products that underflow
      accumulated forwards in `restate` (B <- a (B + (4 + ea dtau) T) + b (es + ea + 4), T <- T a + b).
    - tau = sum_j dtau_j, n - 1 sums: budget_tau = u (2 sum_j ea_j dtau_j + 2 n tau) + the same floor.
  The budgets are checked against np.longdouble (the node and the recurrence wide, on the float64 geometry and gather, which are the
  rule itself) so that the yardstick is honest.  Every comparison prints the worst observed fraction of its budget.

Tested inputs.  Three non-cubic, non-uniform grids, (9, 7, 6), (6, 9, 17) and (33, 5, 5) nodes over +-4 mm.  Te rises along x from
0.6 to 780 eV and the ion density along y from 10^16.8 to 10^21.2 cm^-3, both jittered node by node, so that between 5 % and 40 % of a
case's samples are clamped at an edge of the 10x10 table (1..500 eV x 1e17..1e21 cm^-3); Z in [1, 30].  Each case is scaled so that its
thickest line has tau = 5 (every band of a table, band 0 of the NRL node); the corner graze gives the thin line.  step is 1/32 of the grid's x extent and
max_steps = 40, so only lines longer than 1.25 x extents are capped.  Every case of 63 lines or more holds the planted lines of
`_planted` (its docstring lists them) followed by random lines from points outside the box towards points in and around it; the
one-line case is the planted line whose origin lies inside the box (one line cannot hold them all, nor a thin and a thick line or a share of clamped samples: it is held to non-empty alone).  At
most 30 % of a case's lines miss.  These conditions are asserted on the restatement alone (test 2), so that no test can pass on empty lines.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import test_emission as nrl
import test_table_emission as tab

EPS = 2.0 ** -53
TINY = 2.0 ** -1074
E_ALPHA = 21.0  # tests/test_emission.py's E_ALPHA
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_STEPS = 40


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
def geometry(g, o, d, step, max_steps):
    """The clip and the steps of the rule for the lines o + d t: dict of t0, t1, hit, chord, n, dt, h (n)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    N = o.shape[1]
    t0, t1, hit = np.zeros(N), np.full(N, np.inf), np.ones(N, bool)
    for a in range(3):
        lo, hi = np.float64(g[a][0]), np.float64(g[a][-1])
        still = d[a] == 0.0
        with np.errstate(all="ignore"):
            ta, tb = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
        hit &= np.where(still, (lo <= o[a]) & (o[a] <= hi), True)
        t0 = np.maximum(t0, np.where(still, -np.inf, np.minimum(ta, tb)))
        t1 = np.minimum(t1, np.where(still, np.inf, np.maximum(ta, tb)))
    hit &= t1 > t0
    length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    with np.errstate(all="ignore"):
        chord = np.where(hit, (t1 - t0) * length, 0.0)
        q = chord / step
        n = np.where(q >= max_steps, max_steps, np.maximum(1, np.ceil(q))).astype(np.int64)
        n = np.where(hit, n, 0)
        ns = np.maximum(n, 1)
        dt, h = np.where(hit, (t1 - t0) / ns, 0.0), chord / ns
    return dict(t0=np.where(hit, t0, 0.0), t1=t1, hit=hit, chord=chord, n=n, dt=dt, h=h)


def gather(fields, g, p, active):
    """sr_field_resample's cell / outside / blend lines at the positions p (3, N): the blended value per field (a float64
    array (nx, ny, nz), or a scalar, which is returned as it is) and `inside`."""
    cell, w, inside = [], [], active.copy()
    for a in range(3):
        with np.errstate(invalid="ignore"):
            ok = (p[a] >= g[a][0]) & (p[a] <= g[a][-1])
        ps = np.where(ok, p[a], g[a][0])
        i = np.clip(np.searchsorted(g[a], ps, side="right") - 1, 0, len(g[a]) - 2)
        cell.append(i)
        w.append((ps - g[a][i]) / (g[a][i + 1] - g[a][i]))
        inside &= ok
    (i, j, k), (wx, wy, wz) = cell, w
    ux, uy, uz = 1.0 - wx, 1.0 - wy, 1.0 - wz
    w00, w01, w10, w11 = uy * uz, uy * wz, wy * uz, wy * wz
    out = []
    for f in fields:
        if np.ndim(f) == 0:
            out.append(np.float64(f))
            continue
        with np.errstate(invalid="ignore"):
            s0 = ((f[i, j, k] * w00 + f[i, j, k + 1] * w01) + f[i, j + 1, k] * w10) + f[i, j + 1, k + 1] * w11
            s1 = ((f[i + 1, j, k] * w00 + f[i + 1, j, k + 1] * w01) + f[i + 1, j + 1, k] * w10) + f[i + 1, j + 1, k + 1] * w11
            out.append(ux * s0 + wx * s1)
    return out, inside


def restate(ne, Te, Z, co, o, d, node, toward, step, max_steps=MAX_STEPS, backlight=None, wide=False):
    """include/synthray.h's rule for sr_field_sightlines.  ne: (nx, ny, nz); Te, Z: arrays or scalars; co: the three float32
    coordinate arrays; o, d: (3, N); node: ("nrl", bands) with bands = test_emission._bands(...) or ("table", H) with H =
    test_table_emission.host_arrays(table).  Returns a dict: I, tau, bI, bt (n_band, N), column, chord (N), steps (N) int32, miss (N),
    clamped (the share of the in-box samples a table clamps; 0 for the NRL node).  wide: the node and the recurrence in
    np.longdouble on the float64 geometry and gather (the budgets stay the float64 ones)."""
    g = [np.float64(np.float32(a)) for a in co]
    F = [np.float64(a) if np.ndim(a) else float(a) for a in (ne, Te, Z)]
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    G = geometry(g, o, d, step, max_steps)
    hit, n, h = G["hit"], G["n"], G["h"]
    N = o.shape[1]
    kind, data = node
    nb = len(data[0]) if kind == "nrl" else len(data["e_ph"])
    wt = np.longdouble if wide else np.float64
    I = np.zeros((nb, N), wt) if backlight is None else np.array(backlight, wt)
    tau = np.zeros((nb, N), wt)
    T1, B, Bt = I.astype(np.float64), np.zeros((nb, N)), np.zeros((nb, N))
    column = np.zeros(N)
    n_clamped = n_inside = 0
    for m in range(int(n.max()) if N else 0):
        act = hit & (m < n)
        k = np.where(act, m if toward > 0 else n - 1 - m, 0)
        t = G["t0"] + (k + 0.5) * G["dt"]
        p = [o[a] + d[a] * t for a in range(3)]
        (ne_s, Te_s, Z_s), inside = gather(F, g, p, act)
        ne_s = np.where(inside, ne_s, 0.0)   # outside: dark, and ne counts as 0
        Te_s = np.where(inside, Te_s, 1.0) if np.ndim(Te_s) else np.full(N, Te_s)
        Z_s = np.where(inside, Z_s, 1.0) if np.ndim(Z_s) else np.full(N, Z_s)
        with np.errstate(all="ignore"):
            column = np.where(act, column + ne_s * h, column)
        a_ne, a_Te, a_Z = ne_s.astype(wt), Te_s.astype(wt), Z_s.astype(wt)
        hw = h.astype(wt)
        for b in range(nb):
            if kind == "nrl":
                al, S, x = nrl._node(a_ne, a_Te, a_Z, data[0][b], data[1][b], data[2][b])
                Ea, Es = np.where(al != 0, E_ALPHA, 0.0), np.where(al != 0, 4 + x, 0.0)
            else:
                al, S, Ea, Es, clamped, _ = tab._node(a_ne, a_Te, a_Z, data, b)
                if b == 0:
                    n_clamped += int(np.sum(np.any(clamped, axis=0) & inside))
                    n_inside += int(np.sum(inside))
            with np.errstate(all="ignore"):
                dtau = al * hw
                a = np.exp(-dtau)
                bb = S * (-np.expm1(-dtau))
                I[b] = np.where(act, I[b] * a + bb, I[b])
                tau[b] = np.where(act, tau[b] + dtau, tau[b])
                af, bf, df, ea = a.astype(np.float64), bb.astype(np.float64), dtau.astype(np.float64), Ea + 1
                B[b] = np.where(act, af * (B[b] + (4 + ea * df) * T1[b]) + bf * (Es + ea + 4), B[b])
                T1[b] = np.where(act, T1[b] * af + bf, T1[b])
                Bt[b] = np.where(act, Bt[b] + ea * df, Bt[b])
    floor = 4 * n * TINY
    with np.errstate(all="ignore"):
        bI, bt = 2 * EPS * B + floor, EPS * (2 * Bt + 2 * n * tau.astype(np.float64)) + floor
    return dict(I=I, tau=tau, bI=bI, bt=bt, column=column, chord=G["chord"], steps=n.astype(np.int32), miss=~hit,
                clamped=n_clamped / max(n_inside, 1), geometry=G)


def _assert_close(got, ref, what, extra_I=0.0, extra_tau=0.0):
    """NaN sets equal, finite where the reference is, I and tau within budget (+ extra); prints the worst fractions."""
    worst = []
    for name, bud, extra in (("I", "bI", extra_I), ("tau", "bt", extra_tau)):
        have, want, lim = np.asarray(got[name]), np.asarray(ref[name]).astype(np.float64), ref[bud] + extra
        assert have.shape == want.shape, (what, name, have.shape, want.shape)
        assert np.array_equal(np.isnan(have), np.isnan(want)), f"{what}: the NaN set of {name} differs from the restatement's"
        fin = ~np.isnan(want)
        assert np.all(np.isfinite(have[fin]) == np.isfinite(want[fin])), f"{what}: {name} is not finite where the restatement is"
        fin &= np.isfinite(want)
        dist = np.abs(have[fin] - want[fin])
        assert np.all(dist <= lim[fin]), f"{what}: {name} is off by up to {np.max(dist / np.maximum(lim[fin], TINY)):.3f} budgets"
        pos = lim[fin] > 0
        worst.append(float(np.max(dist[pos] / lim[fin][pos])) if np.any(pos) else 0.0)
    print(f"{what}: bit-equal I {np.array_equal(got['I'], ref['I'], equal_nan=True)}, tau "
          f"{np.array_equal(got['tau'], ref['tau'], equal_nan=True)}; max |d| / budget: I {worst[0]:.3f}, tau {worst[1]:.3f}")


def _assert_exact(got, ref, what):
    """chord, steps, column bit-equal to the restatement's; the missed lines are the lines with steps == 0."""
    assert np.array_equal(got["steps"], ref["steps"]), f"{what}: steps differ on lines {np.nonzero(got['steps'] != ref['steps'])[0][:8]}"
    assert np.array_equal(got["steps"] == 0, ref["miss"]), f"{what}: the set of missed lines differs"
    assert np.array_equal(got["chord"], ref["chord"]), f"{what}: chord differs on lines {np.nonzero(got['chord'] != ref['chord'])[0][:8]}"
    assert np.array_equal(got["column"], ref["column"], equal_nan=True), \
        f"{what}: column differs on lines {np.nonzero(~((got['column'] == ref['column']) | np.isnan(ref['column'])))[0][:8]}"


# ---------------------------------------------------------------- inputs
GRIDS = {"A": (9, 7, 6), "B": (6, 9, 17), "C": (33, 5, 5)}
# (grid, lines, Te a field, Z a field, bands): every line count, every kind of Te / Z and both band counts on the three grids
CONFIGS = (("A", 1, True, True, 4), ("A", 63, True, False, 1), ("B", 65, False, True, 4), ("B", 257, False, False, 1),
           ("C", 700, True, True, 4), ("A", 257, True, True, 1))
U_TE, U_Z = 37.5, 10.0
_GRID, _SCALED, _REF = {}, {}, {}


def _planted(g):
    """The planted lines of a grid with float64 node arrays g, name -> (origin, direction):
    column      axis-parallel through a node column
    face, edge  exactly along a box face / a box edge (d_a == 0 with o_a == lo_a or hi_a): hits
    beside      d_a == 0 with o_a outside the box: a miss
    corner      through a corner of the (x, y) rectangle, t1 == t0 bit for bit: a miss
    graze       the same corner a few ulp inside: one sample
    inside      the origin inside the box
    away        the origin beyond the box, pointing away: a miss
    long        corner to corner with d = hi - lo (not a unit vector): capped at max_steps
    integer     from the lo face along x: chord / step == 32 exactly
    tiny, huge  |d| = 1e-30 and 1e6 through the box's centre"""
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    mid = 0.5 * (lo + hi)
    far = lo[0] - 2.0 ** -10
    delta = 2.0 ** -10
    L = {}
    L["column"] = ((far, g[1][2], g[2][3]), (1.0, 0.0, 0.0))
    L["face"] = ((far, lo[1], mid[2]), (1.0, 0.0, 0.0))
    L["edge"] = ((far, lo[1], hi[2]), (1.0, 0.0, 0.0))
    L["beside"] = ((far, hi[1] + 1e-4, mid[2]), (1.0, 0.0, 0.0))
    L["corner"] = ((lo[0] - delta, hi[1] - delta, mid[2]), (1.0, 1.0, 0.0))
    L["graze"] = ((lo[0] - delta, (hi[1] - delta) * (1 - 8 * EPS), mid[2]), (1.0, 1.0, 0.0))
    L["inside"] = (tuple(mid + 0.1 * (hi - lo) * np.array([0.3, -0.2, 0.1])), (0.3, -0.5, 0.8))
    L["away"] = ((hi[0] + 1e-3, mid[1], mid[2]), (1.0, 0.1, 0.0))
    L["long"] = (tuple(lo - 0.25 * (hi - lo)), tuple(hi - lo))
    L["integer"] = ((lo[0], mid[1], mid[2]), (1.0, 0.0, 0.0))
    u = np.array([0.2, 0.7, -0.4])
    L["tiny"] = (tuple(mid - 0.02 * u), tuple(1e-30 * u))
    L["huge"] = (tuple(mid + 0.02 * u), tuple(-1e6 * u))
    return L


def _lines(g, count, seed):
    """(o, d) (3, count): the planted lines, then random ones; count == 1: the planted line `inside` alone."""
    P = _planted(g)
    if count == 1:
        o, d = P["inside"]
        return np.array(o)[:, None], np.array(d)[:, None]
    rng = np.random.default_rng(seed)
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    m = count - len(P)
    v = rng.normal(size=(3, m))
    src = mid[:, None] + v / np.linalg.norm(v, axis=0) * rng.uniform(8e-3, 20e-3, m)
    src[:, : m // 3] = src[:, :1]  # a third of them from ONE point: a fan, as a pinhole's lines are
    aim = mid[:, None] + half[:, None] * rng.uniform(-1.15, 1.15, (3, m))
    dirs = (aim - src) * rng.uniform(0.3, 3.0, m)
    o = np.concatenate([np.array([p[0] for p in P.values()]).T, src], axis=1)
    d = np.concatenate([np.array([p[1] for p in P.values()]).T, dirs], axis=1)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def _grid(name):
    """Coordinates, fields, table, bands and the scales of one grid, made once."""
    if name not in _GRID:
        shape = GRIDS[name]
        seed = 100 + ord(name)
        rng = np.random.default_rng(seed)
        co = [nrl._coords(m, seed + k) for k, m in enumerate(shape)]
        g = [np.float64(a) for a in co]
        fx, fy, fz = np.meshgrid(*[(a - a[0]) / (a[-1] - a[0]) for a in g], indexing="ij")
        Te = 0.6 * 1300.0 ** fx * rng.uniform(0.9, 1.1, shape)
        ni = 10.0 ** (16.8 + 4.4 * fy) * rng.uniform(0.9, 1.1, shape) * (1 + 0.2 * fz)
        Z = rng.uniform(1.0, 30.0, shape)
        ne_tab = ni * Z * 1e6
        ne_nrl = 1e26 * 10.0 ** (-2.0 * fy) * rng.uniform(0.7, 1.0, shape)
        step = float(g[0][-1] - g[0][0]) / 32
        for a in (Te, Z, ne_tab, ne_nrl):
            a.setflags(write=False)
        _GRID[name] = dict(co=co, g=g, Te=Te, Z=Z, ne={"nrl": ne_nrl, "table": ne_tab}, step=step, bands=nrl._bands(nrl.WAVELENGTHS), seed=seed)
    return _GRID[name]


def _scaled(cfg, kind):
    """ne (float64) and the table of one configuration, scaled so that its thickest line has tau = 5 in every band of a table and
    in band 0 of the NRL node (alpha is linear in a table's opacity and, but for the Coulomb logarithm, quadratic in ne)."""
    key = (cfg, kind)
    if key not in _SCALED:
        name, count, te_f, z_f, nb = cfg
        K = _grid(name)
        o, d = _lines(K["g"], count, K["seed"] + count)
        ne, Te, Z = K["ne"][kind], K["Te"] if te_f else U_TE, K["Z"] if z_f else U_Z
        if kind == "nrl":
            t = restate(ne, Te, Z, K["co"], o, d, ("nrl", tuple(v[:1] for v in K["bands"])), +1, K["step"])["tau"].max()
            _SCALED[key] = (ne * np.sqrt(5.0 / t), None)
        else:
            t = restate(ne, Te, Z, K["co"], o, d, ("table", tab.host_arrays(tab.make_table(10, 10, nb, K["seed"] + 1))), +1, K["step"])["tau"].max(axis=1)
            _SCALED[key] = (ne, tab.make_table(10, 10, nb, K["seed"] + 1, shift=np.log(5.0 / t)))
    return _SCALED[key]


def _node_of(R, kind):
    if kind == "nrl":
        return ("nrl", tuple(v[:R["nb"]] for v in R["K"]["bands"]))
    return ("table", tab.host_arrays(R["table"]))


def _config(cfg, kind, toward, dtype):
    """The inputs of one configuration and their restatement (cached): fields in `dtype`, widened for the restatement."""
    key = (cfg, kind, toward, np.dtype(dtype).name)
    if key not in _REF:
        name, count, te_f, z_f, nb = cfg
        K = _grid(name)
        o, d = _lines(K["g"], count, K["seed"] + count)
        ne, table = _scaled(cfg, kind)
        ne = ne.astype(dtype)
        Te = K["Te"].astype(dtype) if te_f else U_TE
        Z = K["Z"].astype(dtype) if z_f else U_Z
        back = np.random.default_rng(K["seed"] + 3).uniform(0.0, 2e-7, (nb, count))
        R = dict(K=K, o=o, d=d, ne=ne, Te=Te, Z=Z, back=back, nb=nb, table=table)
        R["ref"] = restate(ne, Te, Z, K["co"], o, d, _node_of(R, kind), toward, K["step"], backlight=back)
        _REF[key] = R
    return _REF[key]


def _assert_inputs(R, kind, what):
    """The module docstring's conditions, on the restatement alone."""
    ref = R["ref"]
    hit = ~ref["miss"]
    count = len(hit)
    assert np.mean(ref["miss"]) <= 0.30, f"{what}: {np.mean(ref['miss']):.2f} of the lines miss"
    assert np.all(ref["tau"][:, hit] > 0) and np.all(ref["I"][:, hit] > 0) and np.all(ref["column"][hit] > 0), f"{what}: an empty line that hits"
    assert np.all(np.isfinite(ref["I"])) and np.all(np.isfinite(ref["tau"]))
    if count >= 63:
        tau = ref["tau"][0]
        assert np.any((tau > 0) & (tau < 1e-3)) and np.any((tau > 1) & (tau < 30)), f"{what}: tau spans {tau[hit].min():.2e} .. {tau.max():.2e}"
        assert np.any(ref["steps"] == MAX_STEPS) and np.any(ref["steps"] == 1) and np.any(ref["miss"])
    if kind == "table" and count >= 63:
        assert 0.05 <= ref["clamped"] <= 0.40, f"{what}: clamped share {ref['clamped']:.3f}"
    return ref["clamped"]


def _run(eng, R, kind, toward, table=None, **kw):
    """engine.sightlines on freshly uploaded fields."""
    K = R["K"]
    fields = [eng.Field(a, *K["co"]) if np.ndim(a) else float(a) for a in (R["ne"], R["Te"], R["Z"])]
    node = dict(omegas=np.float64(K["bands"][0][:R["nb"]])) if kind == "nrl" else dict(table=table if table is not None else R["table"])
    try:
        out = eng.sightlines(*fields, R["o"], R["d"], toward=toward, step=K["step"], max_steps=MAX_STEPS,
                             backlight=kw.pop("backlight", R["back"]), **node, **kw)
        out["I"], out["tau"] = out["intensity"], out["optical_depth"]
        assert fields[0].last_kernel_ms > 0
        return out
    finally:
        for f in fields:
            if not isinstance(f, float):
                f.close()


# ================================================================ CPU tests
def test_restatement_against_longdouble(built):
    """1: the yardstick's budgets against the same node and recurrence in np.longdouble (64-bit mantissa here)."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    for cfg in (CONFIGS[1], CONFIGS[2], CONFIGS[4]):
        for kind in ("nrl", "table"):
            for toward in (+1, -1):
                R = _config(cfg, kind, toward, np.float64)
                wide = restate(R["ne"], R["Te"], R["Z"], R["K"]["co"], R["o"], R["d"], _node_of(R, kind), toward, R["K"]["step"],
                               backlight=R["back"], wide=True)
                got = dict(I=wide["I"].astype(np.float64), tau=wide["tau"].astype(np.float64))
                _assert_close(got, R["ref"], f"restatement vs longdouble {cfg} {kind} toward {toward:+d}")
                assert np.array_equal(wide["column"], R["ref"]["column"]) and np.array_equal(wide["steps"], R["ref"]["steps"])


def test_tested_inputs_meet_the_conditions(built):
    """2: every parametrisation of the kernel test meets the module docstring's conditions, and the planted lines are what their
    names say."""
    shares = []
    for cfg in CONFIGS:
        for kind in ("nrl", "table"):
            for dtype in (np.float32, np.float64):
                for toward in (+1, -1):
                    shares.append(_assert_inputs(_config(cfg, kind, toward, dtype), kind, f"{cfg} {kind} {np.dtype(dtype).name} toward {toward:+d}"))
    print(f"clamped share of the table cases {min(s for s in shares if s > 0):.3f} .. {max(shares):.3f}")
    for name in GRIDS:
        K = _grid(name)
        P = _planted(K["g"])
        names = list(P)
        o, d = np.array([p[0] for p in P.values()]).T, np.array([p[1] for p in P.values()]).T
        G = geometry(K["g"], o, d, K["step"], MAX_STEPS)
        at = names.index
        for miss in ("beside", "corner", "away"):
            assert not G["hit"][at(miss)] and G["n"][at(miss)] == 0 and G["chord"][at(miss)] == 0, (name, miss)
        for hits in set(names) - {"beside", "corner", "away"}:
            assert G["hit"][at(hits)], (name, hits)
        assert G["t1"][at("corner")] == 2.0 ** -10 and G["t1"][at("corner")] == np.maximum(0.0, (K["g"][0][0] - o[0, at("corner")]) / 1.0), name
        assert G["n"][at("graze")] == 1 and 0 < G["chord"][at("graze")] < 1e-15, (name, G["chord"][at("graze")])
        assert G["t0"][at("inside")] == 0.0 and G["t0"][at("integer")] == 0.0
        assert G["n"][at("long")] == MAX_STEPS and G["chord"][at("long")] / K["step"] > MAX_STEPS
        assert G["chord"][at("integer")] / K["step"] == 32.0 and G["n"][at("integer")] == 32
        for a in ("face", "edge", "column"):
            assert G["chord"][at(a)] == K["g"][0][-1] - K["g"][0][0], (name, a)
        assert 1 < G["n"][at("tiny")] < MAX_STEPS and G["n"][at("tiny")] == G["n"][at("huge")]
        assert abs(G["chord"][at("tiny")] / G["chord"][at("huge")] - 1) < 1e-12


def test_header_ctypes_and_python_signatures(built):
    """3: the header's struct and prototype, the ctypes declaration and the Python signatures agree."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "synthray.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sr_field_sightlines\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 15
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*sr_sightline_params\s*;", text)
    fields = ["toward", "n_band", "max_steps", "reserved", "step", "omega", "e_ph", "c_omega", "Te", "Z"]
    assert m and re.findall(r"\b(" + "|".join(fields) + r")\b", m.group(1)) == fields
    P = built.SightlineParams
    assert [f[0] for f in P._fields_] == fields
    assert C.sizeof(P) == 4 * 4 + 8 + 3 * 8 * built.MAX_BANDS + 2 * 8 and P.step.offset == 16 and P.omega.offset == 24
    res, args = built.SYMBOLS["sr_field_sightlines"]
    assert res is C.c_int and len(args) == 15 and args[5] is C.c_int64
    assert hasattr(built.lib, "sr_field_sightlines")
    mk = open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()
    assert "sightlines.hip" in mk and "table_node.inc" in mk  # the build id covers both

    from synthpy_amd import engine, sightlines
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.sightlines) == ["ne", "Te", "Z", "origins", "directions", "omegas", "table", "toward", "step", "max_steps", "backlight", "want"]
    kinds = {k: v.kind for k, v in inspect.signature(engine.sightlines).parameters.items()}
    assert all(kinds[k] is inspect.Parameter.KEYWORD_ONLY for k in names(engine.sightlines)[5:])
    assert names(sightlines.sightline_emission) == ["domain", "view", "wavelengths", "table", "step", "max_steps", "fields"]
    assert names(NewDomain.sightline_emission) == names(OldDomain.sightline_emission) == ["self", "view", "wavelengths", "table", "step", "max_steps"]
    assert names(sightlines.PinholeCamera.__init__) == ["self", "pinhole", "look", "up", "det_distance", "pixels", "pitch"]
    assert names(sightlines.PointBacklighter.__init__) == ["self", "source", "look", "up", "det_distance", "pixels", "pitch", "radiance"]
    assert names(sightlines.Chords.__init__)[:4] == ["self", "origins", "directions", "toward"]
    p = engine.sightline_params([2e15, 3e15], -1, 1e-4, 77, Te=3.0, Z=2.0)
    e = engine.emission_params([2e15, 3e15], 0)
    assert (p.toward, p.n_band, p.max_steps, p.step, p.Te, p.Z) == (-1, 2, 77, 1e-4, 3.0, 2.0)
    assert list(p.omega) == list(e.omega) and list(p.e_ph) == list(e.e_ph) and list(p.c_omega) == list(e.c_omega)


def test_argument_checks_come_before_the_device(built):
    """4: every rejected argument is SR_ERR_INVALID with its own text, on a machine with or without a GPU."""
    from synthpy_amd import engine, sightlines
    from synthpy_amd.simulator.domain import ScalarDomain

    lib, ptr = built.lib, built.ptr
    table = tab.make_table(5, 4, 2, 9)
    om = np.asarray(table.photon_energy, np.float64) * tab.E_CHARGE / tab.HBAR
    o0, d0 = np.zeros((3, 2)), np.ones((3, 2))
    out = np.zeros((2, 2))

    def call(p, n=2, o=o0, d=d0, I=out, tau=out, t=None):
        return lib.sr_field_sightlines(None, None, None, None if t is None else C.byref(t), None if p is None else C.byref(p), n, ptr(o), ptr(d),
                                       None, ptr(I), ptr(tau), None, None, None, None)

    def err(text, *a, **kw):
        assert call(*a, **kw) == -1 and text in built.last_error(), (text, built.last_error())

    good = lambda **kw: engine.sightline_params(kw.pop("om", om), kw.pop("toward", 1), kw.pop("step", 1e-4), kw.pop("max_steps", 10))
    err("NULL argument", None)
    for name in ("o", "d", "I", "tau"):
        err("NULL argument", good(), **{name: None})
    err("n must not be negative", good(), n=-1)
    for omegas in ([], [om[0]] * 5):
        err("n_band", good(om=omegas))
    for w in (0.0, -1.0, np.nan, np.inf):
        bad = good()
        bad.omega[1] = w
        err("omega of band 1", bad)
    bad = good()
    bad.e_ph[0] = np.nan
    err("e_ph or c_omega of band 0", bad)
    for toward in (0, 2, -3):
        err("toward", good(toward=toward))
    for step in (0.0, -1e-4, np.nan, np.inf):
        err("step must be finite and positive", good(step=step))
    for ms in (0, -5):
        err("max_steps", good(max_steps=ms))
    # the table's checks, with this entry's name; omega is ignored with a table
    t, keep = engine.emission_table_params(table)
    ignored = good()
    ignored.omega[0] = -1.0
    err("NULL ne", ignored, t=t)
    t.nT = 1
    err("nT must be 2..512", good(), t=t)
    t, keep = engine.emission_table_params(table)
    keep[0][1] = keep[0][0]
    err("LT is not strictly increasing at 1", good(), t=t)
    t, keep = engine.emission_table_params(table)
    keep[2][1, 2, 3] = np.inf
    err("LA has a non-finite entry (band 1)", good(), t=t)
    t, keep = engine.emission_table_params(table)
    t.m_ion = 0.0
    err("m_ion", good(), t=t)
    for name, text in (("o", "non-finite origin of line 1"), ("d", "non-finite direction of line 1")):
        for v in (np.nan, np.inf):
            a = np.ones((3, 2))
            a[2, 1] = v
            err(text, good(), **{name: a})
    dz = np.ones((3, 2))
    dz[:, 1] = 0.0
    err("the direction of line 1 is zero", good(), d=dz)
    err("NULL ne", good())  # every other argument was in order
    err("NULL ne", good(), n=0)  # n == 0 does not skip the checks
    assert "sr_field_sightlines" in built.last_error()

    with pytest.raises(ValueError, match="Field"):
        engine.sightlines(np.zeros((2, 2, 2)), 1.0, 1.0, o0, d0, omegas=om, toward=1, step=1e-4, max_steps=5)
    dom = ScalarDomain(2e-3, 4, ne_type="test_slab")
    cam = sightlines.PinholeCamera((0, 0, 0.01), (0, 0, -1), (0, 1, 0), 0.1, (3, 2), 1e-4)
    with pytest.raises(ValueError, match=r"needs external_Te\(\) and external_Z\(\)"):
        dom.sightline_emission(cam, wavelengths=[532e-9])
    dom.external_Te(50.0)
    dom.external_Z(2.0)
    for kw in ({}, {"wavelengths": [532e-9], "table": table}):
        with pytest.raises(ValueError, match="exactly one"):
            dom.sightline_emission(cam, **kw)
    with pytest.raises(ValueError, match="OpacityTable"):
        dom.sightline_emission(cam, table={"temperatures": [1.0]})
    with pytest.raises(ValueError, match="view"):
        dom.sightline_emission("z", wavelengths=[532e-9])
    with pytest.raises(ValueError, match="parallel"):
        sightlines.PinholeCamera((0, 0, 1), (0, 0, -1), (0, 0, 2), 0.1, (3, 2), 1e-4)
    with pytest.raises(ValueError, match="toward"):
        sightlines.Chords(o0, d0, 0)
    with pytest.raises(ValueError, match=r"\(3, N\)"):
        sightlines.Chords(np.zeros((2, 4)), np.zeros((2, 4)), 1)


def test_views_without_a_device(built):
    """5: PinholeCamera and PointBacklighter lines for a 3x2 detector written out by hand, oblique frames, the tile permutation,
    magnification, and both ScalarDomain generations expose the method."""
    from synthpy_amd import sightlines
    from synthpy_amd._domain import DomainExtras
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    # a pinhole at z = +2 looking down -z, up = +y: l = (0, 0, -1), y = (0, 1, 0), x = y cross l = (-1, 0, 0); the detector is at z = 2.5
    cam = sightlines.PinholeCamera((0.0, 0.0, 2.0), (0, 0, -4), (0, 3, 0), 0.5, (3, 2), 0.25)
    assert np.array_equal(cam.x, [-1, 0, 0]) and np.array_equal(cam.y, [0, 1, 0]) and np.array_equal(cam.l, [0, 0, -1])
    assert np.array_equal(cam.u, [-0.25, 0.0, 0.25]) and np.array_equal(cam.v, [-0.125, 0.125])
    pix = {(0, 0): (0.25, -0.125, 2.5), (0, 1): (0.25, 0.125, 2.5), (1, 0): (0.0, -0.125, 2.5), (1, 1): (0.0, 0.125, 2.5),
           (2, 0): (-0.25, -0.125, 2.5), (2, 1): (-0.25, 0.125, 2.5)}
    o, d = cam.lines()
    assert cam.toward == -1 and cam.shape == (3, 2) and o.shape == d.shape == (3, 6)
    for (i, j), p in pix.items():
        assert np.array_equal(cam.pixel_centres()[:, i, j], p), (i, j)
        assert np.array_equal(o[:, i * 2 + j], (0.0, 0.0, 2.0))
        assert np.array_equal(d[:, i * 2 + j], np.subtract((0.0, 0.0, 2.0), p)), (i, j)  # d = pinhole - pixel: out into the scene
    assert cam.magnification(2.0) == 0.25 and cam.backlight(2) is None
    # a backlighter at z = -2 shining along +z: x = y cross l = (1, 0, 0); the detector is at z = -2 + 4
    bl = sightlines.PointBacklighter((0.0, 0.0, -2.0), (0, 0, 1), (0, 1, 0), 4.0, (3, 2), 0.5, radiance=[1.0, 3.0])
    assert np.array_equal(bl.x, [1, 0, 0]) and bl.toward == +1
    o, d = bl.lines()
    for i, u in enumerate((-0.5, 0.0, 0.5)):
        for j, v in enumerate((-0.25, 0.25)):
            assert np.array_equal(o[:, i * 2 + j], (0, 0, -2.0)) and np.array_equal(d[:, i * 2 + j], (u, v, 4.0)), (i, j)  # d = pixel - source
    assert np.array_equal(bl.backlight(2), np.array([[1.0] * 6, [3.0] * 6])) and bl.magnification(0.5) == 8.0
    with pytest.raises(ValueError, match="backlight"):
        bl.backlight(3)
    # an oblique frame is orthonormal and right-handed, whatever up is
    x, y, l = sightlines.frame((1.0, -2.0, 0.5), (0.3, 0.1, 1.0))
    M = np.stack([x, y, l])
    assert np.allclose(M @ M.T, np.eye(3), atol=1e-15) and np.allclose(np.cross(x, y), l, atol=1e-15)
    assert np.dot(y, (0.3, 0.1, 1.0)) > 0 and np.allclose(l, np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5]))
    # the tile order: a bijection, whole tiles are runs of 64 in row-major order, tiles in Morton order
    for nu, nv in ((13, 5), (3, 2), (8, 8), (16, 24), (17, 9), (1, 70)):
        perm = sightlines.tile_order(nu, nv)
        assert perm.shape == (nu * nv,) and np.array_equal(np.sort(perm), np.arange(nu * nv)), (nu, nv)
        i, j = perm // nv, perm % nv
        tile = (i // 8) * 1000 + j // 8
        change = np.nonzero(np.diff(tile))[0]
        assert len(change) + 1 == len(np.unique(tile)), "a tile's pixels are not contiguous"
    perm = sightlines.tile_order(16, 24)
    assert np.array_equal(perm[:64], (np.arange(8)[:, None] * 24 + np.arange(8)[None, :]).ravel())
    first = perm[::64]
    assert [(p // 24 // 8, p % 24 // 8) for p in first] == [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (1, 2)]
    a = np.arange(13 * 5) * 1.5
    perm = sightlines.tile_order(13, 5)
    back = np.empty_like(a)
    back[perm] = a[perm]
    assert np.array_equal(back, a)
    ch = sightlines.Chords(np.zeros((3, 4)), np.ones((3, 4)), -1, backlight=2.0)
    assert ch.shape == (4,) and ch.order() is None and np.array_equal(ch.backlight(3), np.full((3, 4), 2.0))
    assert NewDomain.sightline_emission is DomainExtras.sightline_emission is OldDomain.sightline_emission
    assert "cos^4" in DomainExtras.sightline_emission.__doc__ and "refraction" in sightlines.sightline_emission.__doc__


# ================================================================ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("toward", [+1, -1], ids=["plus", "minus"])
@pytest.mark.parametrize("kind", ["nrl", "table"])
def test_kernel_against_restatement(eng, kind, toward, dtype):
    """6 (the issue's 1 and 2): every configuration -- 1, 63, 65, 257 and 700 lines with the planted ones, Te and Z as fields or
    scalars, 1 and 4 bands, three grids -- chord, steps, column and the missed lines bit-equal, I and tau within budget; a
    repeated call returns identical bits; a call without the optional outputs returns the same maps."""
    for cfg in CONFIGS:
        R = _config(cfg, kind, toward, dtype)
        what = f"{cfg} {kind} {np.dtype(dtype).name} toward {toward:+d}"
        _assert_inputs(R, kind, what)
        got = _run(eng, R, kind, toward)
        _assert_exact(got, R["ref"], what)
        _assert_close(got, R["ref"], what)
        miss = R["ref"]["miss"]
        assert np.array_equal(got["I"][:, miss], R["back"][:, miss]) and np.all(got["tau"][:, miss] == 0) and np.all(got["column"][miss] == 0)
    again = _run(eng, R, kind, toward)
    assert all(np.array_equal(got[k], again[k]) for k in ("I", "tau", "column", "chord", "steps")), "a repeated call returned other bits"
    bare = _run(eng, R, kind, toward, want=("intensity", "optical_depth"), backlight=None)
    assert set(bare) == {"intensity", "optical_depth", "I", "tau"}
    dark = restate(R["ne"], R["Te"], R["Z"], R["K"]["co"], R["o"], R["d"], _node_of(R, kind), toward, R["K"]["step"])
    _assert_close(bare, dark, what + " no backlight")
    assert np.array_equal(bare["tau"], got["tau"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nrl", "table"])
def test_nan_node_poisons_the_lines_through_its_cells(eng, kind):
    """7 (3): a NaN node of ne, and one of Te, make NaN exactly the lines the restatement says pass their cells."""
    base = _config(CONFIGS[5], kind, -1, np.float64)
    K = base["K"]
    for name, at in (("ne", (4, 3, 2)), ("Te", (1, 5, 4))):
        R = dict(base)
        a = np.array(base[name])
        a[at] = np.nan
        R[name] = a
        ref = restate(R["ne"], R["Te"], R["Z"], K["co"], R["o"], R["d"], _node_of(R, kind), -1, K["step"], backlight=R["back"])
        poisoned = np.isnan(ref["I"][0])
        assert 0 < poisoned.sum() < 0.5 * len(poisoned), f"NaN in {name}: {poisoned.sum()} of {len(poisoned)} lines"
        got = _run(eng, R, kind, -1)
        _assert_close(got, ref, f"NaN node of {name}, {kind}")
        assert np.array_equal(np.isnan(got["I"][0]), poisoned) and np.array_equal(np.isnan(got["tau"][0]), poisoned)
        _assert_exact(got, ref, f"NaN node of {name}, {kind}")
        assert np.array_equal(np.isnan(got["column"]), poisoned if name == "ne" else np.zeros_like(poisoned))


@pytest.mark.gpu
def test_table_branches_and_the_shared_include(eng):
    """8 (4): a table staged in LDS and one above 64 KiB read from global memory, each against the restatement; band 0 of the large
    table alone fits LDS and, its restatement being the same bits, so must the kernel's be; sr_field_emission_table returns
    identical maps before and after a sightlines call (the node and the staging are one include)."""
    from synthpy_amd.utils.eos_opacity import OpacityTable

    R = _config(CONFIGS[4], "table", +1, np.float64)
    K = R["K"]
    t_tau = R["ref"]["tau"].max(axis=1)
    big = tab.make_table(48, 48, 4, 61)
    scale = restate(R["ne"], R["Te"], R["Z"], K["co"], R["o"], R["d"], ("table", tab.host_arrays(big)), +1, K["step"])["tau"].max(axis=1)
    big = tab.make_table(48, 48, 4, 61, shift=np.log(t_tau / scale))
    one = OpacityTable(big.temperatures, big.densities, big.absorption[:1], np.asarray(big.photon_energy)[:1], big.A, emission=big.emission[:1])
    assert tab.packed_bytes(big) > tab.LDS_BUDGET >= tab.packed_bytes(one) and tab.packed_bytes(R["table"]) <= tab.LDS_BUDGET

    A = tab._case(0, 65, (5, 7))
    before = tab._run(eng, A["ne"], A["Te"], A["Z"], A["co"], A["table"], 0, +1, A["back"])
    tab._assert_close(*before, A["refs"][+1], "sr_field_emission_table before")
    res = {}
    for name, t in (("global", big), ("lds", one)):
        nb = t.n_band
        Rt = dict(R, nb=nb, back=R["back"][:nb])
        ref = restate(R["ne"], R["Te"], R["Z"], K["co"], R["o"], R["d"], ("table", tab.host_arrays(t)), +1, K["step"], backlight=Rt["back"])
        res[name] = (_run(eng, Rt, "table", +1, table=t), ref)
        _assert_exact(res[name][0], ref, f"48x48 table, {name}")
        _assert_close(res[name][0], ref, f"48x48 table, {name} ({tab.packed_bytes(t)} B)")
    assert np.array_equal(res["global"][1]["I"][0], res["lds"][1]["I"][0]) and np.array_equal(res["global"][1]["tau"][0], res["lds"][1]["tau"][0])
    assert np.array_equal(res["global"][0]["I"][0], res["lds"][0]["I"][0]), "the LDS and the global branch differ in I"
    assert np.array_equal(res["global"][0]["tau"][0], res["lds"][0]["tau"][0]), "the LDS and the global branch differ in tau"
    after = tab._run(eng, A["ne"], A["Te"], A["Z"], A["co"], A["table"], 0, +1, A["back"])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "sr_field_emission_table changed after a sightlines call"


@pytest.mark.gpu
def test_uniform_plasma_is_analytic(eng):
    """9 (5): uniform ne, Te, Z: every line, oblique ones included, has tau = alpha*chord and I = back e^-tau + S (1 - e^-tau), and
    chord is the box-clipping length computed independently in np.longdouble.
    Bounds.  The blend of a uniform field is ne times the sum of the eight weights: three (1 - w) at 1 u, two products per weight,
    a product with the corner, three sums, the product with ux or wx and the last sum -- at most 11 u from ne; alpha goes as ne^2:
    22 u, on top of the restatement's own budgets: |tau - alpha chord| <= bt + 22 u tau, |I - closed| <= bI + 22 u tau (back + S)
    e^-tau (|dI/dtau| <= (back + S) e^-tau).
    chord = (t1 - t0) * len: ta, tb carry 2 u each (a difference, a quotient), so t1 - t0 carries 2 u (|t0| + |t1|) -- the
    difference CANCELS for a far origin -- + 1 u; len 2.5 u (two roundings under the root, halved, + the root), the product 1 u:
    |chord - exact| <= u (2 (|t0| + |t1|) len + 4.5 chord)."""
    K = _grid("B")
    R = _config(CONFIGS[3], "nrl", +1, np.float64)
    ne0, Te0, Z0 = 1.0e26, 55.0, 3.5
    bands = tuple(v[:2] for v in K["bands"])
    R = dict(R, ne=np.full(GRIDS["B"], ne0), Te=Te0, Z=Z0, nb=2, back=R["back"][:1].repeat(2, axis=0))
    got = _run(eng, R, "nrl", +1)
    ref = restate(R["ne"], Te0, Z0, K["co"], R["o"], R["d"], ("nrl", bands), +1, K["step"], backlight=R["back"])
    _assert_exact(got, ref, "uniform plasma")
    wide = np.longdouble
    o, d = R["o"].astype(wide), R["d"].astype(wide)
    t0, t1, hit = np.zeros(o.shape[1], wide), np.full(o.shape[1], np.inf, wide), np.ones(o.shape[1], bool)
    for a in range(3):
        lo, hi = wide(K["g"][a][0]), wide(K["g"][a][-1])
        still = d[a] == 0
        with np.errstate(all="ignore"):
            ta, tb = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
        hit &= np.where(still, (lo <= o[a]) & (o[a] <= hi), True)
        t0 = np.maximum(t0, np.where(still, -np.inf, np.minimum(ta, tb)))
        t1 = np.minimum(t1, np.where(still, np.inf, np.maximum(ta, tb)))
    length = np.sqrt(np.sum(d * d, axis=0))
    sure = hit & (t1 - t0 > 8 * EPS * (np.abs(t0) + np.abs(t1)))  # the corner touch is decided by rounding: not a length
    assert np.all(~ref["miss"][sure]) and sure.sum() >= 0.7 * len(sure)
    chord = (t1 - t0) * length
    lim = EPS * (2 * (np.abs(t0) + np.abs(t1)) * length + 4.5 * chord)
    off = np.abs(got["chord"].astype(wide) - chord)[sure] / lim[sure]
    print(f"uniform plasma: chord against longdouble clipping, max |d| / bound {float(off.max()):.3f}")
    assert np.all(off <= 1.0)
    for b in range(2):
        al, S, _ = nrl._node(wide(ne0), wide(Te0), wide(Z0), bands[0][b], bands[1][b], bands[2][b])
        tau = al * got["chord"].astype(wide)
        closed = R["back"][b] * np.exp(-tau) + S * (-np.expm1(-tau))
        lim_t = ref["bt"][b] + 22 * EPS * np.float64(tau)
        lim_I = ref["bI"][b] + 22 * EPS * np.float64(tau * (R["back"][b] + S) * np.exp(-tau))
        ft = np.abs(got["tau"][b] - np.float64(tau))[sure] / lim_t[sure]
        fI = np.abs(got["I"][b] - np.float64(closed))[sure] / lim_I[sure]
        print(f"uniform plasma band {b}: tau up to {float(tau.max()):.2f}; max |d| / bound: tau {ft.max():.3f}, I {fI.max():.3f}")
        assert np.all(ft <= 1.0) and np.all(fI <= 1.0)
    assert float((al * got["chord"].max())) > 0.5, "the uniform plasma is thin everywhere: the closed form is not exercised"


def _dyadic(n):
    return np.float32((np.arange(n) - (n - 1) / 2) * 2.0 ** -12)


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_ties_to_the_grid_marches(eng, axis):
    """10 (6): on a uniform dyadic grid, Chords along `axis` from the lo face through every lateral node with step = the cell size
    sample the cell midpoints with weights 0, 1/2, 1 -- exact.
    column: equals the trapezoid of ne along the axis within n u relative, n the samples of a line (the issue's bound), the
    trapezoid taken with NumPy in longdouble.
    emission: with fields constant along the axis both marches see the same alpha and S in every cell, so intensity and
    optical_depth equal engine.emission's and engine.emission_table's maps within the sum of the two restatements' budgets."""
    shape = (9, 7, 6)
    co = [_dyadic(m) for m in shape]
    g = [np.float64(a) for a in co]
    n = shape[axis] - 1
    cell = float(g[axis][1] - g[axis][0])
    lat = [k for k in range(3) if k != axis]
    U, V = np.meshgrid(g[lat[0]], g[lat[1]], indexing="ij")
    o = np.empty((3, U.size))
    o[axis], o[lat[0]], o[lat[1]] = g[axis][0], U.ravel(), V.ravel()
    d = np.zeros((3, U.size))
    d[axis] = 1.0
    rng = np.random.default_rng(70 + axis)
    ne = 1e25 * 10.0 ** (-rng.random(shape))
    f_ne = eng.Field(ne, *co)
    try:
        for toward in (+1, -1):
            got = eng.sightlines(f_ne, 20.0, 2.0, o, d, omegas=[2e15], toward=toward, step=cell, max_steps=100)
            assert np.all(got["steps"] == n) and np.all(got["chord"] == n * cell)
            m = np.moveaxis(ne, axis, 0).astype(np.longdouble)
            trap = np.sum(0.5 * (m[1:] + m[:-1]) * np.longdouble(cell), axis=0).ravel()
            off = np.abs(got["column"] - trap) / (n * EPS * trap)
            print(f"column against the trapezoid, axis {'xyz'[axis]} toward {toward:+d}: max |d| / (n u) = {float(off.max()):.3f}")
            assert np.all(off <= 1.0)
    finally:
        f_ne.close()

    sh = list(shape)
    sh[axis] = 1
    per = 10.0 ** (-3 * rng.permutation(U.size) / (U.size - 1)).reshape(sh)
    ne = np.broadcast_to(2e26 * per, shape).copy()
    Te = np.broadcast_to(rng.uniform(2.0, 400.0, sh), shape).copy()
    Z = np.broadcast_to(rng.uniform(1.0, 20.0, sh), shape).copy()
    bands = tuple(v[:2] for v in nrl._bands(nrl.WAVELENGTHS))
    table = tab.make_table(10, 10, 2, 75)
    thick = tab.restate(ne, Te, Z, co[axis], tab.host_arrays(table), axis)[1].max(axis=(1, 2))
    table = tab.make_table(10, 10, 2, 75, shift=np.log(2.0 / thick))  # the thickest column of each band: tau = 2
    back = rng.uniform(0.0, 2e-7, (2,) + U.shape)
    fields = [eng.Field(a, *co) for a in (ne, Te, Z)]
    try:
        for toward in (+1, -1):
            oo = o.copy()
            oo[axis] = g[axis][0] if toward > 0 else g[axis][-1]  # the light travels along +axis for +1: away from an origin on the lo face
            dd = d * toward
            for kind, node, march, ref_march in (
                    ("nrl", dict(omegas=np.float64(bands[0])), lambda: eng.emission(*fields, np.float64(bands[0]), axis, toward, back),
                     lambda: nrl.restate(ne, Te, Z, co[axis], bands, axis, toward, back)),
                    ("table", dict(table=table), lambda: eng.emission_table(*fields, table, axis, toward, back),
                     lambda: tab.restate(ne, Te, Z, co[axis], tab.host_arrays(table), axis, toward, back))):
                I, tau = march()
                rm = ref_march()
                rs = restate(ne, Te, Z, co, oo, dd, ("nrl", bands) if kind == "nrl" else ("table", tab.host_arrays(table)), +1, cell,
                             max_steps=100, backlight=back.reshape(2, -1))
                got = eng.sightlines(*fields, oo, dd, toward=+1, step=cell, max_steps=100, backlight=back.reshape(2, -1), **node)
                assert np.all(got["steps"] == n)
                fI = np.abs(got["intensity"] - I.reshape(2, -1)) / (rs["bI"] + rm[2].reshape(2, -1))
                ft = np.abs(got["optical_depth"] - tau.reshape(2, -1)) / (rs["bt"] + rm[3].reshape(2, -1))
                print(f"{kind} emission tie, axis {'xyz'[axis]} toward {toward:+d}: tau {tau.min():.2e} .. {tau.max():.2e}; bit-equal I "
                      f"{np.array_equal(got['intensity'], I.reshape(2, -1))}; max |d| / summed budgets: I {fI.max():.3f}, tau {ft.max():.3f}")
                assert np.all(fI <= 1.0) and np.all(ft <= 1.0) and tau.max() > 0.5
    finally:
        for f in fields:
            f.close()


@pytest.mark.gpu
def test_end_to_end_views_of_both_generations(eng):
    """11 (7): domain.sightline_emission(PinholeCamera, wavelengths=) and (PointBacklighter, table=) on both API generations, the
    table read from tests/golden/g16_opac.prp: shapes, a single bright voxel in the pixel the hand geometry predicts (inverted for
    the pinhole) although the lines went to the kernel in tile order, a repeated call bit-identical, float32 fields kept resident."""
    from synthpy_amd import fields as fields_mod
    from synthpy_amd import sightlines
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy import full_solver as fs
    from synthpy_amd.utils.eos_opacity import OpacityTable, read_propaceos

    data = read_propaceos(os.path.join(GOLDEN, "g16_opac.prp"), need_ross_opacity=True, need_emiss_opacity=True, need_abs_opacity=True)
    table = OpacityTable.from_propaceos(data, A=12.011)
    dims, cell = (9, 7, 11), 5e-4
    lengths = tuple(cell * (m - 1) for m in dims)
    ne = np.full(dims, 1e23, np.float32)
    voxel = (6, 2, 5)  # two cells right of the centre node (4, 3, 5) in x, one below it in y, in the plane z = 0
    ne[voxel] = 4e26
    Te = np.full(dims, 80.0, np.float32)
    new = NewDomain(lengths, dims)
    old = fs.ScalarDomain(*[np.linspace(-L / 2, L / 2, m) for L, m in zip(lengths, dims)], lengths[2] / 2)
    for dom in (new, old):
        dom.external_ne(ne)
        dom.external_Te(Te)
        dom.external_Z(3.0)
    D, det = 20e-3, 60e-3
    pitch = cell * det / D  # a cell in the plane z = 0 is a pixel: magnification det / D = 3
    cam = sightlines.PinholeCamera((0, 0, D), (0, 0, -1), (0, 1, 0), det, (13, 9), pitch)   # x = (-1, 0, 0), inverted: pixel (6 + 2, 4 + 1)
    bl = sightlines.PointBacklighter((0, 0, -D), (0, 0, 1), (0, 1, 0), det, (13, 9), pitch, radiance=2e-7)  # x = (+1, 0, 0): pixel (6 + 2, 4 - 1)
    assert cam.magnification(D) == 3.0 and not np.array_equal(cam.order(), np.arange(13 * 9))
    P = np.array([2 * cell, -1 * cell, 0.0])
    a, b = np.dot(P - cam.pinhole, cam.x), np.dot(P - cam.pinhole, cam.y)
    cam_pixel = (int(round(-a * 3 / pitch + 6)), int(round(-b * 3 / pitch + 4)))
    assert cam_pixel == (8, 5)  # lab +x is -x of the camera, inverted back: right; lab -y inverted: up
    a, b = np.dot(P - bl.source, bl.x), np.dot(P - bl.source, bl.y)
    bl_pixel = (int(round(a * 3 / pitch + 6)), int(round(b * 3 / pitch + 4)))
    assert bl_pixel == (8, 3)
    for dom in (new, old):
        who = type(dom).__module__.split(".")[-1]
        em = dom.sightline_emission(cam, wavelengths=[532e-9, 100e-9])
        assert isinstance(em, sightlines.SightlineEmission) and em.intensity.shape == em.optical_depth.shape == (2, 13, 9)
        assert em.column.shape == em.chord.shape == em.steps.shape == (13, 9) and em.steps.dtype == np.int32 and em.photon_energy is None
        assert np.array_equal(em.wavelengths, [532e-9, 100e-9]) and np.array_equal(em.transmission, np.exp(-em.optical_depth))
        for name in ("column", "intensity", "optical_depth"):
            m = getattr(em, name)
            m = m[0] if m.ndim == 3 else m
            assert np.unravel_index(np.argmax(m), m.shape) == cam_pixel, (who, name, np.unravel_index(np.argmax(m), m.shape))
        assert abs(em.chord[6, 4] - lengths[2]) < 1e-9 and em.steps[6, 4] in (20, 21)  # the axial line; the default step: half a cell
        again = dom.sightline_emission(cam, wavelengths=[532e-9, 100e-9])
        assert all(np.array_equal(getattr(em, k), getattr(again, k)) for k in ("intensity", "optical_depth", "column", "chord", "steps"))
        with pytest.raises(ValueError, match="edges"):
            em.band_radiance

        tb = dom.sightline_emission(bl, table=table, max_steps=200)
        assert tb.intensity.shape == (1, 13, 9) and np.array_equal(tb.photon_energy, np.atleast_1d(table.photon_energy))
        assert np.allclose(tb.wavelengths, 1.2398419843320026e-6 / tb.photon_energy, rtol=1e-14)
        assert np.array_equal(tb.edges, table.edges) and tb.band_radiance.shape == tb.intensity.shape
        assert np.unravel_index(np.argmax(tb.column), (13, 9)) == bl_pixel and np.unravel_index(np.argmax(tb.optical_depth[0]), (13, 9)) == bl_pixel
        missed = tb.steps == 0  # the detector is wider than the box's shadow
        assert 0 < missed.sum() < missed.size / 2 and not missed[6, 4] and np.array_equal(missed, tb.chord == 0)
        assert np.all(tb.intensity[0][missed] == 2e-7) and np.all(tb.optical_depth[0][missed] == 0) and np.all(tb.optical_depth[0][~missed] > 0)
        # the maps are the engine's on the same lines in pixel order: the tile order changes nothing but the order
        o, d = bl.lines()
        src = fields_mod.SourceFields(dom)
        try:
            kept = sightlines.sightline_emission(dom, bl, table=table, max_steps=200, fields=src)
            f = src.get_all({"ne": np.asarray(dom.ne), "Te": np.asarray(dom.Te)})
            flat = eng.sightlines(f["ne"], f["Te"], 3.0, o, d, table=table, toward=+1, step=sightlines.default_step(dom), max_steps=200,
                                  backlight=bl.backlight(1))
        finally:
            src.close()
        assert np.array_equal(kept.intensity, tb.intensity) and np.array_equal(flat["intensity"].reshape(1, 13, 9), tb.intensity)
        assert np.array_equal(flat["column"].reshape(13, 9), tb.column) and np.array_equal(flat["steps"].reshape(13, 9), tb.steps)

    # Chords: a diode's single chord at an angle, (n_band, N) maps
    ch = sightlines.Chords([[0.0], [-8e-3], [1e-3]], [[0.1], [1.0], [-0.05]], -1)
    em = new.sightline_emission(ch, wavelengths=[100e-9])
    assert em.intensity.shape == (1, 1) and em.column.shape == (1,) and em.chord[0] > 0 and em.steps[0] > 0


def _five(nb=2):
    """Grid A, five planted lines (inside, column, long, graze and beside: a miss), nb NRL bands, float64 fields."""
    K = _grid("A")
    P = _planted(K["g"])
    names = ("inside", "column", "long", "graze", "beside")
    o = np.ascontiguousarray(np.array([P[k][0] for k in names]).T)
    d = np.ascontiguousarray(np.array([P[k][1] for k in names]).T)
    back = np.random.default_rng(K["seed"] + 5).uniform(0.0, 2e-7, (nb, len(names)))
    return dict(K=K, o=o, d=d, ne=K["ne"]["nrl"], Te=K["Te"], Z=K["Z"], back=back, nb=nb, table=None)


def _poisoned(empty):
    """np.empty with every byte 0xA5: an output the library does not write cannot hold the right values by chance, as the recycled
    buffer of an equal array can."""
    def poisoned(shape, dtype=np.float64, *args, **kw):
        a = empty(shape, dtype, *args, **kw)
        a.reshape(-1).view(np.uint8)[:] = 0xA5
        return a

    return poisoned


@pytest.mark.gpu
def test_each_optional_output_asked_for_alone(eng, monkeypatch):
    """12: want = ("column",), ("chord",), ("steps",): the dict holds that key alone and the array has the bits of the call that
    asks for everything (the three read-backs are separate branches of the host code), which is held to the restatement."""
    R = _five()
    K = R["K"]
    full = _run(eng, R, "nrl", -1)
    ref = restate(R["ne"], R["Te"], R["Z"], K["co"], R["o"], R["d"], _node_of(R, "nrl"), -1, K["step"], backlight=R["back"])
    assert ref["miss"].tolist() == [False, False, False, False, True] and np.all(ref["column"][:4] > 0)
    _assert_exact(full, ref, "five planted lines")
    _assert_close(full, ref, "five planted lines")
    fields = [eng.Field(a, *K["co"]) for a in (R["ne"], R["Te"], R["Z"])]
    try:
        for name in ("column", "chord", "steps"):
            with monkeypatch.context() as m:
                m.setattr(np, "empty", _poisoned(np.empty))
                one = eng.sightlines(*fields, R["o"], R["d"], omegas=np.float64(K["bands"][0][:2]), toward=-1, step=K["step"],
                                     max_steps=MAX_STEPS, backlight=R["back"], want=(name,))
            assert list(one) == [name], f"want=({name!r},) returned {list(one)}"
            assert one[name].dtype == full[name].dtype and np.array_equal(one[name], full[name]), f"{name} asked for alone differs"
    finally:
        for f in fields:
            f.close()


@pytest.mark.gpu
def test_no_lines(eng):
    """13: n = 0 is accepted: empty arrays of the right shapes and types, no kernel time."""
    R = _five()
    K = R["K"]
    fields = [eng.Field(a, *K["co"]) for a in (R["ne"], R["Te"], R["Z"])]
    try:
        for back in (np.zeros((2, 0)), None):
            out = eng.sightlines(*fields, np.zeros((3, 0)), np.zeros((3, 0)), omegas=np.float64(K["bands"][0][:2]), toward=+1,
                                 step=K["step"], max_steps=MAX_STEPS, backlight=back)
            assert list(out) == ["intensity", "optical_depth", "column", "chord", "steps"]
            assert out["intensity"].shape == out["optical_depth"].shape == (2, 0)
            assert out["column"].shape == out["chord"].shape == out["steps"].shape == (0,) and out["steps"].dtype == np.int32
            assert fields[0].last_kernel_ms == 0.0
    finally:
        for f in fields:
            f.close()
