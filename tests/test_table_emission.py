"""Self-emission from tabulated opacities: sr_field_emission_table (emission_table.hip), engine.emission_table,
emission.table_emission / TableEmission and ScalarDomain.table_emission of both API generations.

THE REFERENCE for values is `restate` below: include/synthray.h's rule in NumPy float64, operation for operation, marching the
cells sequentially, as tests/test_emission.py's `restate` is for sr_field_emission (its march and its budget machinery are
copied here and generalised: the error of alpha and S is now a per-node quantity).  The kernel may compose the cells of a column
in another fixed order and its exp / expm1 / log are another library's, so bit equality is NOT expected; what is ASSERTED are
bounds derived from the operation count, not measured, and every test prints the worst observed error as a fraction of its bound.

Units: u = 2^-53.  A correctly rounded operation errs by at most 1 u relative, a library function (exp, expm1, log) by 1 ulp = 2 u
(tests/test_emission.py says where that figure comes from).  One side's error against the exact value of the rule on the same
inputs, first order:

* ni = (ne*1e-6)/Z: 2 u.  lt = log(Te): Te is exact, the library leaves 2|lt| u ABSOLUTE.  ld = log(ni): 2 u from ni and 2|ld| u
  from the library: (2 + 2|ld|) u absolute.
* ft = (lt - LT[i])/(LT[i+1] - LT[i]): the subtraction CANCELS, so lt's absolute error is divided by the cell's width dT:
  2|lt|/dT u, + 3 u ft for the three roundings (ft <= 1; the clamp to [0, 1] is 1-Lipschitz).  fd: (2 + 2|ld|)/dD u + 3 u fd.
* l = p0 + ft*(p1 - p0), p_r = T[r][j] + fd*(T[r][j+1] - T[r][j]): with D_d, D_t the cell's largest corner differences along the
  density and the temperature axis and M = max|T|, p_r errs by D_d err(fd) + 2 u D_d + u M (difference, product, sum) and l by
  err(p) + D_t err(ft) + 2 u D_t + u M (the weights 1-ft and ft sum to 1).  With G_d = max over the WHOLE table of
  |T[i][j+1] - T[i][j]|/dD_j, G_t the same along the temperature axis, and dD_max, dT_max the widest cells, D_d <= G_d dD:
      E_l = G_d (2 + 2|ld| + 5 dD_max) + G_t (2|lt| + 5 dT_max) + 2 M          [u, absolute]
  Whole-table slopes, because the interpolant is continuous across lattice nodes and an lt within rounding of LT[i] may land
  in the cell on either side: the bound has to hold for either cell.
* alpha = (exp(la)*(ni*m_ion))*100: l's ABSOLUTE error becomes exp's RELATIVE error, E_l(LA), + 2 u the library, 3 u for ni*m_ion,
  2 u the products: E_alpha = E_l(LA) + 7.
* S: the Planck factor c_omega/expm1(e_ph/Te) carries (4 + x) u, x = e_ph/Te (tests/test_emission.py).  With an emission table
  the first factor exp(le - la) adds E_l(LE) + E_l(LA) + |le - la| u (the subtraction's rounding) + 2 u the library, and the
  product 1 u: E_S = 4 + x [+ E_l(LE) + E_l(LA) + |le - la| + 3].  A dark node has E_alpha = E_S = 0.
* a cell between nodes k, k': ea = max(E_alpha) + 2 for dtau; a = exp(-dtau): (2 + ea dtau) u; -expm1(-dtau), condition number <= 1:
  (ea + 2) u; the mean of the S: es = max(E_S) + 1; b: (es + ea + 3) u.
* a column: I = sum_k term_k, term_k = b_k prod_{j after k} a_j, all terms >= 0, so a bound relative to each term holds for any
  composition order: N_k roundings in the coefficient, at most N_k + 7 additions (N_k + 1 sequentially; the tree's 6 levels + the
  carry), the factors' sum_j (2 + ea_j dtau_j).  Both sides:
      budget_I = u sum_k term_k * 2 (es_k + ea_k + 10 + 4 N_k + sum_{j after k} ea_j dtau_j),   the backlight with es + ea + 3 = 0,
  + a floor of (4 * cells) * 2^-1074 for products that underflow.
* tau = sum_j dtau_j, any order: budget_tau = u (sum_j 2 ea_j dtau_j + 2 cells tau) + the same floor.

The budgets are checked against np.longdouble so that the yardstick itself is honest.

Tested inputs (the conditions test 2 asserts for every parametrisation): a 10x10 lattice, log-spaced and jittered, over 1-500 eV x
1e17-1e21 cm^-3; ln(opacity) uniform over four decades per band, emission within e^+-1 of absorption, each band shifted so that its
thickest column has tau = 2; Te log-uniform in [0.7, 700] eV, Z in [1, 30]; ni one decade node by node times 4.3 decades column
by column, 10^15.9 .. 10^21.2 cm^-3 (alpha is linear in ni, so thin columns need the spread the NRL rule gets from ne^2); photon
energies 12.4 eV (100 nm), 30, 90 and 250 eV; non-uniform planes over 8 mm.  Five nodes are planted: one beyond each table edge
and one whose Te IS a lattice temperature (lt equals LT[i] bit for bit in NumPy; the kernel's log may put it in either cell).
"""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

EPS = 2.0 ** -53
TINY = 2.0 ** -1074
LIGHT = 299792458.0
HBAR = 6.62607015e-34 / (2 * np.pi)
E_CHARGE = 1.602176634e-19
PHOTON_EV = (HBAR * (2 * np.pi * LIGHT / 100e-9) / E_CHARGE, 30.0, 90.0, 250.0)
LDS_BUDGET = 64 * 1024  # emission_table.hip's kLdsBudget: a packed table above it is read from global memory
GOLDEN = os.path.join(ROOT, "tests", "golden")


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


# ---------------------------------------------------------------- tables
def _lattice(lo, hi, n, rng):
    """n log-spaced nodes from lo to hi, the inner ones jittered by up to 0.3 of the spacing."""
    l = np.linspace(np.log(lo), np.log(hi), n)
    if n > 2:
        l[1:-1] += rng.uniform(-0.3, 0.3, n - 2) * (l[1] - l[0])
    out = np.exp(l)
    out[0], out[-1] = lo, hi
    return out


def make_table(n_t, n_d, n_band, seed, lte=False, shift=None):
    """A random OpacityTable: ln(absorption) uniform over four decades, emission within e^+-1 of it; shift: ln factor per band."""
    from synthpy_amd.utils.eos_opacity import OpacityTable

    rng = np.random.default_rng(seed)
    T, D = _lattice(1.0, 500.0, n_t, rng), _lattice(1e17, 1e21, n_d, rng)
    la = rng.uniform(np.log(1e-1), np.log(1e3), (n_band, n_t, n_d))
    le = la + rng.uniform(-1.0, 1.0, la.shape)
    if shift is not None:
        la, le = la + np.reshape(shift, (-1, 1, 1)), le + np.reshape(shift, (-1, 1, 1))
    edges = np.stack([0.8 * np.float64(PHOTON_EV[:n_band]), 1.25 * np.float64(PHOTON_EV[:n_band])], axis=1)
    return OpacityTable(T, D, np.exp(la), PHOTON_EV[:n_band], 12.011, emission=None if lte else np.exp(le), edges=edges)


def packed_bytes(table):
    """What emission_table.hip packs for the kernel: (n_tables * n_band * nT * nD + nT + nD) float64."""
    n = table.absorption.size * (1 if table.emission is None else 2) + len(table.temperatures) + len(table.densities)
    return 8 * n


def host_arrays(table, bands=None):
    """The bits the host hands the kernel (engine.emission_table_params, engine.emission_params) + the slopes of the budget;
    bands: a slice of the table's bands."""
    from synthpy_amd import engine

    t, (LT, LD, LA, LE) = engine.emission_table_params(table)
    p = engine.emission_params(np.asarray(table.photon_energy, np.float64) * engine.E_CHARGE / engine.HBAR, 2)
    sl = slice(None) if bands is None else bands
    out = dict(LT=LT, LD=LD, LA=LA[sl], LE=None if LE is None else LE[sl], e_ph=list(p.e_ph)[:p.n_band][sl],
               c_omega=list(p.c_omega)[:p.n_band][sl], m_ion=t.m_ion)
    dT, dD = np.diff(LT), np.diff(LD)

    def slopes(T):
        return (np.max(np.abs(np.diff(T, axis=2)) / dD, axis=(1, 2)), np.max(np.abs(np.diff(T, axis=1)) / dT[:, None], axis=(1, 2)),
                np.max(np.abs(T), axis=(1, 2)))

    out["GA"] = slopes(out["LA"])
    out["GE"] = None if out["LE"] is None else slopes(out["LE"])
    out["dT_max"], out["dD_max"] = dT.max(), dD.max()
    return out


# ---------------------------------------------------------------- the restatement
def _locate(L, x):
    """i = the largest index with L[i] <= x clamped to [0, n-2], and min(max((x - L[i])/(L[i+1] - L[i]), 0), 1).  A wide x is
    placed by its float64 rounding: within rounding of a lattice node either cell gives the same value (the interpolant is
    continuous)."""
    i = np.clip(np.searchsorted(L, np.float64(x), side="right") - 1, 0, len(L) - 2)
    f = np.minimum(np.maximum((x - L[i]) / (L[i + 1] - L[i]), 0), 1)
    return i, f


def _interp(T, i, j, ft, fd):
    p0 = T[i, j] + fd * (T[i, j + 1] - T[i, j])
    p1 = T[i + 1, j] + fd * (T[i + 1, j + 1] - T[i + 1, j])
    return p0 + ft * (p1 - p0)


def _node(ne, Te, Z, H, b):
    """alpha, S of every node for band b in the dtype of the inputs, and (float64) E_alpha, E_S of the module docstring."""
    dt = ne.dtype
    dark = (Te <= 0) | (ne <= 0) | (Z <= 0)
    with np.errstate(all="ignore"):
        ni = (ne * 1e-6) / Z
        lt, ld = np.log(Te), np.log(ni)
        i, ft = _locate(H["LT"].astype(dt), lt)
        j, fd = _locate(H["LD"].astype(dt), ld)
        la = _interp(H["LA"][b].astype(dt), i, j, ft, fd)
        al = (np.exp(la) * (ni * dt.type(H["m_ion"]))) * 100.0
        x = H["e_ph"][b] / Te
        S = H["c_omega"][b] / np.expm1(x)

        def E_l(G):
            return (G[0][b] * (2 + 2 * np.abs(np.float64(ld)) + 5 * H["dD_max"]) + G[1][b] * (2 * np.abs(np.float64(lt)) + 5 * H["dT_max"])
                    + 2 * G[2][b])

        Ea = E_l(H["GA"]) + 7
        Es = 4 + np.float64(x)
        if H["LE"] is not None:
            le = _interp(H["LE"][b].astype(dt), i, j, ft, fd)
            S = np.exp(le - la) * S
            Es = Es + E_l(H["GE"]) + E_l(H["GA"]) + np.abs(np.float64(le - la)) + 3
    zero = np.zeros((), dt)
    clamped = np.stack([lt < H["LT"][0], lt > H["LT"][-1], ld < H["LD"][0], ld > H["LD"][-1]])
    return np.where(dark, zero, al), np.where(dark, zero, S), np.where(dark, 0.0, Ea), np.where(dark, 0.0, Es), clamped & ~dark, lt


def restate(ne, Te, Z, g, H, axis, toward=+1, backlight=None, dtype=np.float64):
    """include/synthray.h's rule for sr_field_emission_table, sequentially.  ne, Te, Z: (nx, ny, nz) arrays or scalars; g: the
    float32 node coordinates of `axis`; H = host_arrays(table).  Returns (I, tau, budget_I, budget_tau), each (n_band, n_u, n_v);
    with dtype=np.longdouble the same recurrence wide (its budgets are still the float64 ones)."""
    shape = np.shape(ne)
    f = lambda a: np.moveaxis(np.broadcast_to(np.asarray(a), shape), axis, 0).astype(dtype)
    ne, Te, Z = f(ne), f(Te), f(Z)
    if toward < 0:
        ne, Te, Z = ne[::-1], Te[::-1], Z[::-1]
    g = np.float64(np.float32(g))
    g = g if toward > 0 else g[::-1]
    h = np.abs(g[1:] - g[:-1]).astype(dtype)
    n = len(g)
    out = []
    for b in range(len(H["e_ph"])):
        al, S, Ea, Es, _, _ = _node(ne, Te, Z, H, b)
        I = np.zeros(ne.shape[1:], dtype) if backlight is None else np.asarray(backlight[b]).astype(dtype)
        I0 = I.copy()
        tau = np.zeros(ne.shape[1:], dtype)
        cells = []
        with np.errstate(all="ignore"):
            for k in range(n - 1):
                dt = (0.5 * (al[k] + al[k + 1])) * h[k]
                a = np.exp(-dt)
                bb = (0.5 * (S[k] + S[k + 1])) * (-np.expm1(-dt))
                I = I * a + bb
                tau = tau + dt
                cells.append((np.float64(a), np.float64(bb), np.float64(dt), np.maximum(Ea[k], Ea[k + 1]) + 2, np.maximum(Es[k], Es[k + 1]) + 1))
            # the budget, from the last cell back: P = the product of the later factors, N their number, W = their sum of ea dtau
            P, W, bud, bt = np.ones(I.shape), np.zeros(I.shape), np.zeros(I.shape), np.zeros(I.shape)
            for N, (a, bb, dt, ea, es) in enumerate(reversed(cells)):
                bud = bud + bb * P * 2 * (es + ea + 10 + 4 * N + W)
                P, W = P * a, W + ea * dt
                bt = bt + 2 * ea * dt
            bud = bud + np.float64(I0) * P * 2 * (7 + 4 * (n - 1) + W)
            bt = bt + 2 * (n - 1) * np.float64(tau)
        out.append((I, tau, EPS * bud + 4 * (n - 1) * TINY, EPS * bt + 4 * (n - 1) * TINY))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def _assert_close(got_I, got_tau, ref, what, factor=1.0):
    """NaN sets equal, finite where the reference is, I and tau within factor * budget; prints the worst fractions."""
    I, tau, bI, bt = ref
    worst = []
    for name, got, want, bud in (("I", got_I, I, bI), ("tau", got_tau, tau, bt)):
        assert got.shape == want.shape, (what, name, got.shape, want.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: the NaN set of {name} differs from the restatement's"
        ok = ~np.isnan(want)
        assert np.all(np.isfinite(got[ok]) == np.isfinite(want[ok])), f"{what}: {name} is not finite where the restatement is"
        fin = ok & np.isfinite(want)
        d = np.abs(got[fin] - np.float64(want[fin]))
        frac = d / (factor * bud[fin])
        worst.append(float(frac.max()) if frac.size else 0.0)
    print(f"{what}: bit-equal I {np.array_equal(got_I, I, equal_nan=True)}, tau {np.array_equal(got_tau, tau, equal_nan=True)}; "
          f"max |d| / budget: I {worst[0]:.3f}, tau {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (what, worst)


def _assert_inputs(ref, what):
    """Every column non-empty, every budget below 1e-9 of its value, a thin and a thick column."""
    I, tau, bI, bt = ref
    assert np.all(tau > 0) and np.all(I > 0), f"{what}: an empty column"
    assert np.all(bI < 1e-9 * I) and np.all(bt < 1e-9 * tau), f"{what}: a budget above 1e-9 of its value ({np.max(bI / I):.2e}, {np.max(bt / tau):.2e})"
    assert np.any(tau < 1e-3) and np.any((tau > 1) & (tau < 30)), f"{what}: tau spans {tau.min():.2e} .. {tau.max():.2e}"


def _assert_coverage(K, what):
    """Between 5 % and 40 % of the nodes clamped at a table edge, each of the four edges hit, a node within 4 ulp of a lattice
    value in lt."""
    H = K["H"]
    _, _, _, _, clamped, lt = _node(K["ne"], K["Te"], K["Z"], H, 0)
    share = float(np.mean(np.any(clamped, axis=0)))
    assert 0.05 <= share <= 0.40, f"{what}: clamped share {share:.3f}"
    assert all(np.any(c) for c in clamped), f"{what}: edges hit {[bool(np.any(c)) for c in clamped]}"
    with np.errstate(all="ignore"):
        ulps = np.min(np.abs(lt[..., None] - H["LT"]) / np.spacing(np.abs(H["LT"])), axis=-1)
    assert np.any(ulps <= 4), f"{what}: no node within 4 ulp of a lattice temperature"
    return share


# ---------------------------------------------------------------- inputs
def _coords(n, seed, half=4e-3):
    """Non-uniform float32 node coordinates inside +-half, no two nodes closer than a fifth of the widest gap."""
    g = np.cumsum(np.random.default_rng(seed).uniform(0.2, 1.0, n))
    return np.float32(-half + (g - g[0]) * (2 * half / (g[-1] - g[0])))


AXIS_N = (2, 3, 63, 64, 65, 129)
LATERAL = ((5, 7), (67, 3))
_CASES = {}


def _fields(axis, n, lateral, seed):
    """ne, Te, Z of the module docstring's description, with the five planted nodes in plane 0 of the first five columns."""
    rng = np.random.default_rng(seed)
    shape = list(lateral)
    shape.insert(axis, n)
    col = list(lateral)
    col.insert(axis, 1)
    ncol = lateral[0] * lateral[1]
    per_col = 10.0 ** (-4.3 * rng.permutation(ncol) / (ncol - 1)).reshape(col)
    ni = 10.0 ** 21.2 * 10.0 ** (-rng.random(shape)) * per_col
    Te = 0.7 * 1000.0 ** rng.random(shape)
    Z = rng.uniform(1.0, 30.0, shape)
    return ni, Te, Z, shape


def _plant(ni, Te, axis, lateral, table):
    at = lambda c: tuple(0 if d == axis else np.unravel_index(c, lateral)[d - (d > axis)] for d in range(3))
    Te[at(0)], Te[at(1)] = 0.8, 650.0
    ni[at(2)], ni[at(3)] = 3e16, 2e21
    Te[at(4)] = table.temperatures[len(table.temperatures) // 2]


def _case(axis, n, lateral):
    """Fields and table of one shape, made once (toward only changes the march), and the restatement for both marches: 4 bands
    with an emission table and a backlight, and band 0 alone in LTE without one."""
    key = (axis, n, lateral)
    if key not in _CASES:
        seed = 1000 * axis + 10 * n + lateral[0]
        ni, Te, Z, shape = _fields(axis, n, lateral, seed)
        co = [_coords(m, 7 + k) for k, m in enumerate(shape)]
        table = make_table(10, 10, 4, seed + 1)
        _plant(ni, Te, axis, lateral, table)
        ne = ni * Z * 1e6
        tau_max = restate(ne, Te, Z, co[axis], host_arrays(table), axis)[1].max(axis=(1, 2))
        table = make_table(10, 10, 4, seed + 1, shift=np.log(2.0 / tau_max))
        lte = make_table(10, 10, 1, seed + 1, lte=True, shift=np.log(2.0 / tau_max[:1]))
        assert np.array_equal(lte.absorption, table.absorption[:1])
        H, H1 = host_arrays(table), host_arrays(lte)
        back = np.random.default_rng(seed + 2).uniform(0.0, 2e-7, (4,) + tuple(lateral))
        refs = {t: restate(ne, Te, Z, co[axis], H, axis, t, back) for t in (+1, -1)}
        refs1 = {t: restate(ne, Te, Z, co[axis], H1, axis, t) for t in (+1, -1)}
        for a in (ne, Te, Z, back) + tuple(v for r in list(refs.values()) + list(refs1.values()) for v in r):
            a.setflags(write=False)
        _CASES[key] = dict(ne=ne, Te=Te, Z=Z, co=co, table=table, lte=lte, H=H, H1=H1, back=back, refs=refs, refs1=refs1)
    return _CASES[key]


def _run(eng, ne, Te, Z, co, table, axis, toward, backlight=None):
    """engine.emission_table on freshly uploaded fields; Te, Z arrays or floats."""
    fields = [eng.Field(a, *co) if np.ndim(a) else float(a) for a in (ne, Te, Z)]
    try:
        return eng.emission_table(*fields, table, axis, toward, backlight)
    finally:
        for f in fields:
            if not isinstance(f, float):
                f.close()


# ================================================================ CPU tests
def test_restatement_against_longdouble(built):
    """1: the yardstick against the same recurrence in np.longdouble (64-bit mantissa here), within its own budget; the larger
    tables too."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    for axis, n, lateral in ((2, 65, (5, 7)), (0, 129, (5, 7)), (1, 3, (67, 3))):
        K = _case(axis, n, lateral)
        for t in (+1, -1):
            wide = restate(K["ne"], K["Te"], K["Z"], K["co"][axis], K["H"], axis, t, K["back"], dtype=np.longdouble)
            _assert_close(np.float64(wide[0]), np.float64(wide[1]), K["refs"][t], f"restatement vs longdouble axis {axis} n {n} toward {t:+d}")
            wide = restate(K["ne"], K["Te"], K["Z"], K["co"][axis], K["H1"], axis, t, dtype=np.longdouble)
            _assert_close(np.float64(wide[0]), np.float64(wide[1]), K["refs1"][t], f"restatement vs longdouble, LTE, axis {axis} n {n} toward {t:+d}")
    K = _case(2, 65, (5, 7))
    for name, table in _other_tables().items():
        H = host_arrays(table)
        ref = restate(K["ne"], K["Te"], K["Z"], K["co"][2], H, 2)
        wide = restate(K["ne"], K["Te"], K["Z"], K["co"][2], H, 2, dtype=np.longdouble)
        _assert_close(np.float64(wide[0]), np.float64(wide[1]), ref, f"restatement vs longdouble, table {name}")


def test_tested_inputs_meet_the_conditions(built):
    """2: every parametrisation of the kernel test: non-empty columns, budgets below 1e-9, a thin and a thick column -- for the
    four bands together and for the one-band LTE call -- 5 % to 40 % of the nodes clamped, every table edge hit, a node within
    4 ulp of a lattice temperature."""
    shares = []
    for axis in range(3):
        for n in AXIS_N:
            for lateral in LATERAL:
                K = _case(axis, n, lateral)
                what = f"axis {axis} n {n} lateral {lateral}"
                shares.append(_assert_coverage(K, what))
                for t in (+1, -1):
                    _assert_inputs(K["refs"][t], f"{what} toward {t:+d}")
                    _assert_inputs(K["refs1"][t], f"{what} toward {t:+d} one band LTE")
    print(f"clamped share {min(shares):.3f} .. {max(shares):.3f}")


def test_header_ctypes_and_python_signatures(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "synthray.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sr_field_emission_table\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 9
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*sr_emission_table\s*;", text)
    assert m and [w for w in re.findall(r"\b(nT|nD|LT|LD|LA|LE|m_ion)\b", m.group(1))] == ["nT", "nD", "LT", "LD", "LA", "LE", "m_ion"]
    assert C.sizeof(built.EmissionTable) == 2 * 4 + 4 * 8 + 8
    assert [f[0] for f in built.EmissionTable._fields_] == ["nT", "nD", "LT", "LD", "LA", "LE", "m_ion"]
    assert built.SYMBOLS["sr_field_emission_table"][0] is C.c_int and len(built.SYMBOLS["sr_field_emission_table"][1]) == 9
    assert hasattr(built.lib, "sr_field_emission_table")
    mk = open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()
    assert "emission_table.hip" in mk and "emission_march.inc" in mk  # the build id covers both

    from synthpy_amd import emission, engine
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain
    from synthpy_amd.utils import eos_opacity

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.emission_table) == ["ne", "Te", "Z", "table", "axis", "toward", "backlight"]
    assert names(emission.table_emission) == ["domain", "table", "toward", "backlight", "fields"]
    assert names(NewDomain.table_emission) == names(OldDomain.table_emission) == ["self", "table", "toward", "backlight"]
    assert names(eos_opacity.read_propaceos) == ["file_name", "need_zf_table", "need_en_table", "need_eion", "need_eele", "need_pion",
                                                 "need_pele", "need_ross_opacity", "need_emiss_opacity", "need_abs_opacity"]
    assert names(eos_opacity.OpacityTable.from_propaceos) == ["data", "A", "photon_energy"]
    assert issubclass(emission.TableEmission, emission.Emission)
    # what the host hands the kernel: logarithms of the table, the band constants of emission_params, the ion mass
    table = make_table(10, 10, 2, 5)
    t, (LT, LD, LA, LE) = engine.emission_table_params(table)
    assert (t.nT, t.nD) == (10, 10) and t.m_ion == 12.011 * 1.66053906660e-24
    assert np.array_equal(LT, np.log(table.temperatures)) and np.array_equal(LA, np.log(table.absorption)) and np.array_equal(LE, np.log(table.emission))
    assert t.LA == LA.ctypes.data and t.LE == LE.ctypes.data and t.LT == LT.ctypes.data and t.LD == LD.ctypes.data
    assert engine.emission_table_params(make_table(10, 10, 1, 5, lte=True))[0].LE is None
    H = host_arrays(table)
    p = engine.emission_params(np.float64(PHOTON_EV[:2]) * E_CHARGE / HBAR, 0)
    assert H["e_ph"] == list(p.e_ph)[:2] and H["c_omega"] == list(p.c_omega)[:2]
    assert abs(H["e_ph"][1] - 30.0) < 1e-13 and abs(H["e_ph"][0] - 12.398419843320026) < 1e-12


def test_argument_checks_come_before_the_device(built):
    """3: every rejected argument is SR_ERR_INVALID with its own text, on a machine with or without a GPU."""
    from synthpy_amd import emission, engine
    from synthpy_amd.simulator.domain import ScalarDomain

    lib, ptr = built.lib, built.ptr
    out = np.zeros((2, 2, 2))
    table = make_table(5, 4, 2, 9)
    om = np.asarray(table.photon_energy, np.float64) * E_CHARGE / HBAR

    def call(t, p, I=out, tau=out):
        return lib.sr_field_emission_table(None, None, None, None if t is None else C.byref(t), None if p is None else C.byref(p), None,
                                           ptr(I), ptr(tau), None)

    def tab(**change):
        t, keep = engine.emission_table_params(table)
        arrays = dict(LT=keep[0].copy(), LD=keep[1].copy(), LA=keep[2].copy(), LE=keep[3].copy())
        for k, v in change.items():
            if k in arrays:
                arrays[k] = v(arrays[k]) if callable(v) else v
            else:
                setattr(t, k, v)
        for k, a in arrays.items():
            setattr(t, k, None if a is None else a.ctypes.data)
        t._keep = arrays
        return t

    def poke(index, value):
        def f(a):
            a[index] = value
            return a
        return f

    good = engine.emission_params(om, 2)
    assert call(tab(), None) == -1 and "NULL" in built.last_error()
    assert call(tab(), good, I=None) == -1 and "NULL" in built.last_error()
    assert call(tab(), good, tau=None) == -1 and "NULL" in built.last_error()
    for omegas in ([], [om[0]] * 5):
        assert call(tab(), engine.emission_params(omegas, 2)) == -1 and "n_band" in built.last_error(), built.last_error()
    bad = engine.emission_params(om, 2)
    bad.c_omega[1] = np.inf
    assert call(tab(), bad) == -1 and "band 1" in built.last_error()
    ignored = engine.emission_params(om, 2)
    ignored.omega[0], ignored.omega[1] = -1.0, np.nan  # p->omega is ignored: the call gets as far as the fields
    assert call(tab(), ignored) == -1 and "NULL ne" in built.last_error(), built.last_error()
    assert call(None, good) == -1 and "NULL table" in built.last_error()
    for member in ("LT", "LD", "LA"):
        assert call(tab(**{member: None}), good) == -1 and "NULL table member" in built.last_error(), built.last_error()
    for member in ("nT", "nD"):
        for n in (1, 0, -4, 513):
            assert call(tab(**{member: n}), good) == -1 and f"{member} must be 2..512" in built.last_error(), built.last_error()
    for member in ("LT", "LD"):
        for value in (np.nan, np.inf, -np.inf):
            assert call(tab(**{member: poke(2, value)}), good) == -1 and f"{member}[2] is not finite" in built.last_error(), built.last_error()
        assert call(tab(**{member: lambda a: a[::-1].copy()}), good) == -1 and f"{member} is not strictly increasing" in built.last_error()
        assert call(tab(**{member: lambda a: np.r_[a[:2], a[1:-1]]}), good) == -1 and f"{member} is not strictly increasing at 2" in built.last_error()
    for member in ("LA", "LE"):
        for value in (np.nan, np.inf):
            assert call(tab(**{member: poke((1, 2, 3), value)}), good) == -1 and f"{member} has a non-finite entry (band 1)" in built.last_error()
    for m_ion in (0.0, -1e-23, np.nan, np.inf):
        assert call(tab(m_ion=m_ion), good) == -1 and "m_ion" in built.last_error()
    for toward in (0, 2, -3):
        assert call(tab(), engine.emission_params(om, 2, toward)) == -1 and "toward" in built.last_error()
    for axis in (3, -1):
        assert call(tab(), engine.emission_params(om, axis)) == -1 and "axis" in built.last_error()
    assert call(tab(), good) == -1 and "NULL ne" in built.last_error()  # every other argument was in order
    assert call(tab(LE=None), good) == -1 and "NULL ne" in built.last_error()  # LTE: a NULL LE is in order
    assert "sr_field_emission_table" in built.last_error()

    with pytest.raises(ValueError, match="Field"):
        engine.emission_table(np.zeros((2, 2, 2)), 1.0, 1.0, table, 2)
    dom = ScalarDomain(2e-3, 4, ne_type="test_slab")
    with pytest.raises(ValueError, match=r"needs external_Te\(\) and external_Z\(\)"):
        dom.table_emission(table)
    dom.external_Te(50.0)
    dom.external_Z(2.0)
    with pytest.raises(ValueError, match="OpacityTable"):
        emission.table_emission(dom, {"temperatures": [1.0, 2.0]})
    for toward in (0, "z", None):
        with pytest.raises(ValueError, match="toward"):
            dom.table_emission(table, toward=toward)
    dom.probing_direction = "w"
    with pytest.raises(ValueError, match="probing_direction"):
        dom.table_emission(table)


def test_table_emission_object_without_a_device(built):
    """4: TableEmission: wavelengths from the photon energies, edges, band_radiance; Emission's after, sample and transmission."""
    from synthpy_amd.emission import Emission, TableEmission

    gu, gv = np.array([0.0, 1.0, 3.0]), np.array([-1.0, 0.0, 2.0, 3.0])
    U, V = np.meshgrid(gu, gv, indexing="ij")
    I1, t1 = np.stack([1 + U + 2 * V, 5 - U * V]), np.stack([0.5 + 0 * U, 0.1 * (U + 1)])
    I2, t2 = np.stack([2 + 0 * U, 1 + U]), np.stack([1.0 + V * 0, 2.0 + V])
    e_ph, edges = [12.0, 90.0], [[10.0, 15.0], [80.0, 100.0]]
    near, far = TableEmission(I1, t1, ("x", "z"), (gu, gv), e_ph, edges), TableEmission(I2, t2, ("x", "z"), (gu, gv), e_ph, edges)
    assert isinstance(near, Emission) and near.intensity.shape == (2, 3, 4)
    assert np.allclose(near.wavelengths, 2 * np.pi * HBAR * LIGHT / (E_CHARGE * np.float64(e_ph)), rtol=1e-15)
    assert abs(near.wavelengths[0] * 12.0 / 1.2398419843320026e-6 - 1) < 1e-12  # hc/e = 1.2398 eV um
    assert np.array_equal(near.photon_energy, e_ph) and np.array_equal(near.edges, edges)
    d_omega = np.float64([5.0, 20.0]) * E_CHARGE / HBAR
    assert np.allclose(near.band_radiance, I1 * d_omega[:, None, None], rtol=1e-15)
    assert np.array_equal(near.transmission, np.exp(-t1))
    both = near.after(far)
    assert np.array_equal(both.intensity, I2 * np.exp(-t1) + I1) and np.array_equal(both.optical_depth, t2 + t1)
    p, q = np.array([0.0, 0.5, 2.0, 3.1]), np.array([-1.0, 1.0, 2.5, 0.0])
    got = near.sample(p, q, "intensity")
    assert got.shape == (2, 4) and np.all(np.isnan(got[:, 3])) and np.allclose(got[0, :3], 1 + p[:3] + 2 * q[:3], rtol=1e-15)
    bare = TableEmission(I1, t1, ("x", "z"), (gu, gv), e_ph)
    assert bare.edges is None
    with pytest.raises(ValueError, match="edges"):
        bare.band_radiance
    with pytest.raises(ValueError, match="differ"):
        near.after(TableEmission(I2, t2, ("x", "z"), (gu, gv), [12.0, 91.0], edges))


def test_table_of_the_nrl_coefficient_gives_self_emission_s_image(built):
    """5: physical cross-check, restatement against restatement: with uniform Z = 6 at 100 nm, a table that holds
    kappa(Z ni, T, Z, omega)/(c rho) at its lattice nodes (10 per decade over 1-500 eV x 1e17-1e21 cm^-3) gives the image
    self_emission's rule gives, up to the error of interpolating ln(kappa) bilinearly in (ln T, ln ni) -- kappa's max() kinks make
    it irregular.  The distance is interpolation error, not rounding, so the bound is a measured number: on these inputs the two
    NumPy restatements differ by at most 1.394e-5 relative in tau and 7.186e-4 in I (measured with this very test; ln(kappa) is
    linear in ln T and ln ni but for the Coulomb logarithm, whose floor of 2 ends near 92 eV here); asserted is twice that."""
    import test_emission as nrl
    from synthpy_amd.utils.eos_opacity import OpacityTable

    Zu, lam = 6.0, 100e-9
    bands = nrl._bands([lam])
    T = np.geomspace(1.0, 500.0, 28)
    D = np.geomspace(1e17, 1e21, 41)
    TT, DD = np.meshgrid(T, D, indexing="ij")
    alpha, _, _ = nrl._node(Zu * DD * 1e6, TT, Zu, bands[0][0], bands[1][0], bands[2][0])  # [1/m]
    A = 12.011
    kappa = alpha / 100.0 / (DD * (A * 1.66053906660e-24))  # [cm^2/g]
    table = OpacityTable(T, D, kappa, bands[1][0], A)
    rng = np.random.default_rng(11)
    shape = (6, 5, 65)
    per_col = 10.0 ** (-3 * rng.permutation(30) / 29).reshape(6, 5, 1)
    ni = 1e21 * 10.0 ** (-rng.random(shape)) * per_col
    Te = 500.0 ** rng.random(shape)
    g = _coords(65, 12)
    ne = ni * Zu * 1e6
    H = host_arrays(table)
    assert abs(H["e_ph"][0] / bands[1][0] - 1) < 4 * EPS
    want = nrl.restate(ne, Te, Zu, g, bands, 2)
    got = restate(ne, Te, Zu, g, H, 2)
    assert not np.any(_node(ne, Te, np.float64(Zu), H, 0)[4]), "a node outside the table"
    d_tau = float(np.max(np.abs(got[1] - want[1]) / want[1]))
    d_I = float(np.max(np.abs(got[0] - want[0]) / want[0]))
    print(f"table of the NRL coefficient, 10 lattice points per decade: tau {want[1].min():.2e} .. {want[1].max():.2e}; "
          f"max relative distance tau {d_tau:.3e}, I {d_I:.3e}")
    assert d_tau <= 2 * 1.394e-5 and d_I <= 2 * 7.186e-4
    assert d_tau > 1e-6, "the table's image equals the formula's to rounding: the test compares a thing with itself"


# ================================================================ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("lateral", LATERAL, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("n", AXIS_N)
@pytest.mark.parametrize("toward", [+1, -1], ids=["plus", "minus"])
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_kernel_against_restatement(eng, axis, toward, n, lateral):
    """6: I and tau within budget, equal NaN sets, finite outputs: 4 bands with an emission table and a backlight, and band 0
    alone in LTE without a backlight (10x10 tables: the LDS branch)."""
    K = _case(axis, n, lateral)
    ref = K["refs"][toward]
    what = f"axis {'xyz'[axis]} toward {toward:+d} n {n} lateral {lateral}"
    assert packed_bytes(K["table"]) <= LDS_BUDGET
    _assert_inputs(ref, what)
    I, tau = _run(eng, K["ne"], K["Te"], K["Z"], K["co"], K["table"], axis, toward, K["back"])
    assert I.shape == (4,) + lateral and np.all(np.isfinite(I)) and np.all(np.isfinite(tau))
    _assert_close(I, tau, ref, what + " 4 bands")
    I1, tau1 = _run(eng, K["ne"], K["Te"], K["Z"], K["co"], K["lte"], axis, toward)
    _assert_inputs(K["refs1"][toward], what)
    _assert_close(I1, tau1, K["refs1"][toward], what + " 1 band LTE")


def _other_tables():
    """The tables besides the 10x10: the smallest, an odd-sized one, and two on the far side of the LDS budget."""
    return {"2x2 2 bands": make_table(2, 2, 2, 31), "37x23 3 bands": make_table(37, 23, 3, 32),
            "37x23 1 band LTE": make_table(37, 23, 1, 33, lte=True), "48x48 4 bands (global)": make_table(48, 48, 4, 34),
            "100x90 1 band LTE (global)": make_table(100, 90, 1, 35, lte=True), "64x63 2 bands LTE (LDS, full)": make_table(64, 63, 2, 36, lte=True)}


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_table_sizes_and_both_branches(eng, axis):
    """7: tables 2x2, 37x23, and tables whose packed size is beyond the 64 KiB LDS budget (read from global memory) and just
    inside it; 1 to 4 bands, with and without an emission table."""
    K = _case(axis, 65, (5, 7))
    tables = _other_tables()
    sizes = {name: packed_bytes(t) for name, t in tables.items()}
    assert sizes["48x48 4 bands (global)"] > LDS_BUDGET and sizes["100x90 1 band LTE (global)"] > LDS_BUDGET
    assert LDS_BUDGET - 1024 < sizes["64x63 2 bands LTE (LDS, full)"] <= LDS_BUDGET and sizes["37x23 3 bands"] <= LDS_BUDGET
    for name, table in tables.items():
        H = host_arrays(table)
        back = K["back"][:table.n_band]
        for toward in (+1, -1):
            ref = restate(K["ne"], K["Te"], K["Z"], K["co"][axis], H, axis, toward, back)
            I, tau = _run(eng, K["ne"], K["Te"], K["Z"], K["co"], table, axis, toward, back)
            _assert_close(I, tau, ref, f"table {name} ({sizes[name]} B) axis {'xyz'[axis]} toward {toward:+d}")


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 2], ids=["x", "z"])
def test_input_kinds(eng, axis):
    """8: float32 fields against the restatement on their widened values; Te / Z as uniform values give the bits of constant-filled
    fields, in every combination and on both table branches; a repeated call gives identical bits; sr_field_emission and
    sr_field_emission_table called alternately on one set of fields each return what they return alone; mismatched fields are refused."""
    lateral, n = (5, 7), 65
    K = _case(axis, n, lateral)
    table2 = make_table(10, 10, 2, 41)
    ne32, Te32, Z32 = (np.float32(K[k]) for k in ("ne", "Te", "Z"))
    ref = restate(np.float64(ne32), np.float64(Te32), np.float64(Z32), K["co"][axis], host_arrays(table2), axis, -1)
    I, tau = _run(eng, ne32, Te32, Z32, K["co"], table2, axis, -1)
    _assert_close(I, tau, ref, f"axis {'xyz'[axis]} float32 fields")
    I64, tau64 = _run(eng, np.float64(ne32), np.float64(Te32), np.float64(Z32), K["co"], table2, axis, -1)
    assert np.array_equal(I, I64) and np.array_equal(tau, tau64), "float32 fields and their float64 widening differ"

    shape = K["ne"].shape
    om = 2 * np.pi * LIGHT / np.float64([1064e-9, 100e-9])
    for dtype in (np.float32, np.float64):
        f_ne = eng.Field(K["ne"].astype(dtype), *K["co"])
        f_Te, f_Z = eng.Field(np.full(shape, 37.5, dtype), *K["co"]), eng.Field(np.full(shape, 4.0, dtype), *K["co"])
        v_Te = eng.Field(K["Te"].astype(dtype), *K["co"])
        try:
            for table in (K["table"], make_table(48, 48, 3, 42)):
                back = K["back"][:table.n_band]
                full = eng.emission_table(f_ne, f_Te, f_Z, table, axis, +1, back)
                assert f_ne.last_kernel_ms > 0
                want = restate(np.float64(K["ne"].astype(dtype)), 37.5, 4.0, K["co"][axis], host_arrays(table), axis, +1, back)
                _assert_close(*full, want, f"axis {'xyz'[axis]} {np.dtype(dtype).name} constant Te, Z, {table.absorption.shape} table")
                for Te, Z in ((37.5, f_Z), (f_Te, 4.0), (37.5, 4.0)):
                    part = eng.emission_table(f_ne, Te, Z, table, axis, +1, back)
                    assert np.array_equal(full[0], part[0]) and np.array_equal(full[1], part[1]), (dtype, type(Te), type(Z))
                again = eng.emission_table(f_ne, f_Te, f_Z, table, axis, +1, back)
                assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1]), "a repeated call returned other bits"
                a, b = eng.emission_table(f_ne, v_Te, 4.0, table, axis, -1), eng.emission_table(f_ne, v_Te, 4.0, table, axis, -1)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "a repeated call returned other bits"
            # the two entries alternately on the same handles
            alone_nrl, alone_tab = eng.emission(f_ne, v_Te, f_Z, om, axis), eng.emission_table(f_ne, v_Te, f_Z, table2, axis)
            for _ in range(2):
                x, y = eng.emission(f_ne, v_Te, f_Z, om, axis), eng.emission_table(f_ne, v_Te, f_Z, table2, axis)
                assert np.array_equal(x[0], alone_nrl[0]) and np.array_equal(x[1], alone_nrl[1]), "sr_field_emission changed after a table call"
                assert np.array_equal(y[0], alone_tab[0]) and np.array_equal(y[1], alone_tab[1]), "sr_field_emission_table changed after an NRL call"
        finally:
            for f in (f_ne, f_Te, f_Z, v_Te):
                f.close()

    from synthpy_amd._ffi import SynthrayError

    co2 = [c.copy() for c in K["co"]]
    co2[1][2] = np.nextafter(co2[1][2], np.float32(1))
    fields = dict(ne=eng.Field(K["ne"], *K["co"]), vec=eng.Field(np.zeros(shape + (3,)), *K["co"]),
                  f32=eng.Field(np.float32(K["Te"]), *K["co"]), moved=eng.Field(K["Te"], *co2))
    try:
        for Te, text in ((fields["vec"], "vector"), (fields["f32"], "dtype"), (fields["moved"], "grids")):
            with pytest.raises(SynthrayError, match=text):
                eng.emission_table(fields["ne"], Te, 3.0, table2, axis)
        with pytest.raises(ValueError, match="backlight"):
            eng.emission_table(fields["ne"], 10.0, 3.0, table2, axis, backlight=K["back"][:3])
    finally:
        for f in fields.values():
            f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("big", [False, True], ids=["lds", "global"])
@pytest.mark.parametrize("axis", [0, 2], ids=["x", "z"])
def test_edge_columns(eng, axis, big):
    """9: dark columns (ne = 0, Te = 0, Te < 0, Z = 0, Z < 0), dark nodes inside a bright column, a NaN node, and columns that lie
    entirely outside the table beyond each of its four edges -- one column each among ordinary ones, 70 planes."""
    n, lateral = 70, (4, 4)
    rng = np.random.default_rng(80 + axis)
    shape = list(lateral)
    shape.insert(axis, n)
    ni = 10.0 ** rng.uniform(18.0, 20.5, shape)
    Te = 10.0 ** rng.uniform(0.5, 2.5, shape)
    Z = rng.uniform(1.0, 10.0, shape)
    col = lambda i, j: tuple(slice(None) if d == axis else (i, j)[d - (d > axis)] for d in range(3))
    node = lambda i, j, k: tuple(k if d == axis else (i, j)[d - (d > axis)] for d in range(3))
    Te[col(2, 0)] = rng.uniform(0.05, 0.9, n)      # below the table in temperature
    Te[col(2, 1)] = rng.uniform(600.0, 5e3, n)     # above
    ni[col(2, 2)] = 10.0 ** rng.uniform(13.0, 16.9, n)  # below in density
    ni[col(2, 3)] = 10.0 ** rng.uniform(21.1, 23.0, n)  # above
    ne = ni * Z * 1e6
    ne[col(0, 0)] = 0.0
    Te[col(0, 1)] = 0.0
    Te[col(0, 2)] = -5.0
    Z[col(0, 3)] = 0.0
    Z[col(1, 0)] = -2.0
    ne[node(1, 1, 37)] = np.nan
    for k, (a, v) in enumerate(((ne, 0.0), (Te, -1.0), (Z, 0.0), (Z, -3.0))):
        a[node(1, 2, 10 + 12 * k)] = v  # dark nodes inside a bright column
    co = [_coords(m, 50 + d) for d, m in enumerate(shape)]
    table = make_table(48, 48, 3, 51) if big else make_table(10, 10, 3, 51)
    assert (packed_bytes(table) > LDS_BUDGET) == big
    H = host_arrays(table)
    back = rng.uniform(1e-8, 2e-7, (3,) + lateral)
    dark = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0)]
    for t in (+1, -1):
        ref = restate(ne, Te, Z, co[axis], H, axis, t, back)
        I, tau = _run(eng, ne, Te, Z, co, table, axis, t, back)
        _assert_close(I, tau, ref, f"edge columns axis {'xyz'[axis]} toward {t:+d}")
        for i, j in dark:
            assert np.array_equal(I[:, i, j], back[:, i, j]) and np.all(tau[:, i, j] == 0), f"the dark column {(i, j)} emitted or absorbed"
        nan = np.zeros(lateral, bool)
        nan[1, 1] = True
        assert np.array_equal(np.isnan(I), np.broadcast_to(nan, I.shape)) and np.array_equal(np.isnan(tau), np.isnan(I))
        assert np.all(tau[:, 2:] > 0) and np.all(tau[:, 1, 2] > 0)
        # outside the table the edge value holds: the columns beyond an edge equal those of fields moved ONTO that edge
        Tc = np.clip(Te, 1.0, 500.0)
        held = restate(ne, np.where(Te > 0, Tc, Te), Z, co[axis], H, axis, t, back)
        assert np.all(np.abs(held[1][:, 2, :2] - ref[1][:, 2, :2]) <= 2 * ref[3][:, 2, :2]), "Te beyond the table is not held at its edge"


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [1, 2], ids=["y", "z"])
def test_slabs_chain(eng, axis):
    """10: 65 planes cut at plane 40 into two fields that share it; chained by backlight and by TableEmission.after, both marches."""
    from synthpy_amd.emission import TableEmission

    K = _case(axis, 65, (5, 7))
    table, H = K["table"], K["H"]
    part = lambda a, lo, hi: np.ascontiguousarray(np.take(a, np.arange(lo, hi + 1), axis=axis))
    slabs = []
    for lo, hi in ((0, 40), (40, 64)):
        co = list(K["co"])
        co[axis] = K["co"][axis][lo:hi + 1]
        slabs.append(tuple(part(K[k], lo, hi) for k in ("ne", "Te", "Z")) + (co,))
    names = [n for k, n in enumerate("xyz") if k != axis]
    lat = [np.float64(K["co"][k]) for k in range(3) if k != axis]
    for t in (+1, -1):
        whole = K["refs"][t]
        far, near = (slabs[0], slabs[1]) if t > 0 else (slabs[1], slabs[0])
        ref_far = restate(*far[:3], far[3][axis], H, axis, t, K["back"])
        ref_near = restate(*near[:3], near[3][axis], H, axis, t, ref_far[0])
        I_far, tau_far = _run(eng, *far, table, axis, t, K["back"])
        I_chain, tau_near = _run(eng, *near, table, axis, t, I_far)
        I_near0, tau_near0 = _run(eng, *near, table, axis, t)
        assert np.array_equal(tau_near, tau_near0)
        mk = lambda I, tau: TableEmission(I, tau, names, lat, table.photon_energy, table.edges)
        em = mk(I_near0, tau_near0).after(mk(I_far, tau_far))
        bud_I = ref_near[2] + ref_far[2] + whole[2] + 4 * EPS * whole[0]  # the slabs', the whole's, and after()'s three roundings
        bud_t = ref_near[3] + ref_far[3] + whole[3] + 2 * EPS * whole[1]
        for name, I, tau in (("backlight", I_chain, tau_far + tau_near), ("after", em.intensity, em.optical_depth)):
            dI, dt = np.abs(I - whole[0]) / bud_I, np.abs(tau - whole[1]) / bud_t
            print(f"slabs by {name}, axis {'xyz'[axis]} toward {t:+d}: max |d| / summed budgets: I {float(dI.max()):.3f}, tau {float(dt.max()):.3f}")
            assert np.all(dI <= 1.0) and np.all(dt <= 1.0)


@pytest.mark.gpu
def test_end_to_end_from_a_propaceos_file(eng):
    """11: a domain of each generation, and a rotated() one, through
    domain.table_emission(OpacityTable.from_propaceos(read_propaceos(<synthetic file>), A=12.011)).  external_Te floors the
    temperature at Te_min = 1 eV by default, the table's lowest temperature here; Te_min=0.0 keeps the nodes below the table."""
    from synthpy_amd.emission import TableEmission
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy import full_solver as fs
    from synthpy_amd.utils.eos_opacity import OpacityTable, read_propaceos

    data = read_propaceos(os.path.join(GOLDEN, "g16_opac.prp"), need_ross_opacity=True, need_emiss_opacity=True, need_abs_opacity=True)
    table = OpacityTable.from_propaceos(data, A=12.011)
    assert table.n_band == 1 and table.absorption.shape == (1, 20, 10) and table.emission is not None
    H = host_arrays(table)
    dims = (12, 10, 14)
    rng = np.random.default_rng(90)
    ni = 10.0 ** rng.uniform(16.5, 21.5, dims)
    Te = np.float32(10.0 ** rng.uniform(-0.2, 3.0, dims))
    ne = np.float32(ni * 3.0 * 1e6)
    for direction in "xyz":
        a = "xyz".index(direction)
        new = NewDomain((4e-3, 3e-3, 5e-3), dims, probing_direction=direction)
        new.external_ne(ne)
        new.external_Te(Te, Te_min=0.0)
        new.external_Z(np.broadcast_to(np.float64(3.0), dims))
        co = [np.linspace(-h, h, m) for h, m in zip((2e-3, 1.5e-3, 2.5e-3), dims)]
        old = fs.ScalarDomain(*co, 2.5e-3, probing_direction=direction)
        old.external_ne(ne)
        old.external_Te(Te, Te_min=0.0)
        old.external_Z(3.0)
        old.calc_dndr(1064e-9)
        ref = restate(np.float64(ne), np.float64(Te), 3.0, (new.x, new.y, new.z)[a], H, a)
        for dom in (new, old):
            em, proj = dom.table_emission(table), dom.line_integrals()
            assert isinstance(em, TableEmission) and em.axes == proj.axes and em.intensity.shape == (1,) + proj.shape
            assert all(np.array_equal(u, v) for u, v in zip(em.coords, proj.coords))
            assert np.array_equal(em.edges, table.edges) and em.band_radiance.shape == em.intensity.shape
            assert np.allclose(em.wavelengths, 1.2398419843320026e-6 / table.photon_energy, rtol=1e-14)
            _assert_close(em.intensity, em.optical_depth, ref, f"{type(dom).__module__.split('.')[-1]} probing {direction}")
            assert np.all(em.optical_depth > 0) and np.all(em.intensity > 0)

    # turned by 90 degrees about y and probed along z, the domain is the original probed along x (tests/test_emission.py, test 11)
    n = 24
    x = np.float32((np.arange(n) - (n - 1) / 2) * 2.0 ** -12)
    rng = np.random.default_rng(91)
    ne, Te = 4.0e6 * 10.0 ** rng.uniform(16.5, 21.5, (n, n, n)), 10.0 ** rng.uniform(-0.2, 3.0, (n, n, n))
    doms = {}
    for direction in "xz":
        doms[direction] = fs.ScalarDomain(x, x, x, float(x[-1]), probing_direction=direction)
        doms[direction].external_ne(ne)
        doms[direction].external_Te(Te, Te_min=0.0)
        doms[direction].external_Z(4.0)
    view = doms["z"].rotated(90, about="y")
    for toward, t in (("+", +1), ("-", -1)):
        ref = restate(ne, Te, 4.0, x, H, 0, t)
        A, B = doms["x"].table_emission(table, toward=toward), view.table_emission(table, toward=toward)
        assert A.axes == ("y", "z") and B.axes == ("x", "y")
        _assert_close(A.intensity, A.optical_depth, ref, f"probing x toward {toward}")
        for name, bud in (("intensity", ref[2]), ("optical_depth", ref[3])):
            want = np.flip(np.transpose(getattr(A, name), (0, 2, 1)), axis=1)
            d = np.abs(getattr(B, name) - want) / (2 * np.flip(np.transpose(bud, (0, 2, 1)), axis=1))
            print(f"turned domain toward {toward} {name}: bit-equal {np.array_equal(getattr(B, name), want)}, max |d| / (2 budgets) = {float(d.max()):.3f}")
            assert np.all(d <= 1.0)
