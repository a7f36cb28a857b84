"""Self-emission images: sr_field_emission (emission.hip), engine.emission, emission.self_emission / Emission and
ScalarDomain.self_emission of both API generations.

THE REFERENCE for values is `restate` below: include/synthray.h's rule in NumPy float64, operation for operation, marching the
cells sequentially (NumPy's elementwise products and sums are separate calls and cannot fuse; the kernel is compiled with
-ffp-contract=off).  The kernel may compose the cells of a column in another fixed order (the header says so; along z it uses a
tree), and its exp / expm1 / log are another library's, so bit equality is NOT expected.  What is ASSERTED are bounds derived from
the operation count, not measured; every test prints the worst observed error as a fraction of its bound.

Units: u = 2^-53.  A correctly rounded operation (+, *, /, sqrt) errs by at most 1 u relative; a library function by its ulp
bound, 1 ulp = 2 u at most.  exp, expm1 and log are budgeted at 1 ulp per side (2 ulp = 4 u for the two sides): for HIP's float64
device functions that figure is from memory of the HIP math API documentation ("maximum ULP error" tables) -- no copy of that
documentation is installed under the ROCm tree this was written against, so it could not be confirmed there -- and for NumPy's
libm it is glibc's documented bound.  One side's error against the exact value of the rule on the same inputs:

* alpha: r = (ne*1e-6)/omega 2 u, r*r 5 u, (3.1e-5*Z)*c 2 u, their product 8 u; the argument of the log carries 8.5 u (2.5 u from
  omega_max, 2 u from L_max, 1 u their product, 2 u the numerator, 1 u the division), an absolute error of the log that the
  Coulomb logarithm's floor of 2 turns into at most 4.25 u relative, + 2 u the library: 6.25 u; times lnL 15.25 u; 1/(Te*sqrt(Te)) 3 u,
  the product 19.25 u, the division by c: E_ALPHA = 21 u (rounded up).
* S = C / expm1(x), x = e_ph/Te (1 u): expm1's condition number x / (1 - exp(-x)) <= x + 1, the library 2 u, the division 1 u:
  (4 + x) u.  x is the same bits on both sides of a kernel comparison but not against np.longdouble, so it stays in the budget.
* a cell: dtau = (0.5*(alpha+alpha'))*h: E_ALPHA + 2 = 23 u (h is a difference of float32 values, exact); a = exp(-dtau): (2 + 23 dtau) u;
  -expm1(-dtau), condition number <= 1: 25 u; the mean of the S: (5 + x) u; b: (31 + x) u.
* a column: I = sum_k term_k with term_k = b_k * prod_{j after k} a_j, all terms >= 0, so a bound relative to each term holds for
  any composition order.  With N_k cells after k, any order multiplies the term's coefficient together in N_k roundings and puts
  the term through at most N_k + 7 additions (N_k + 1 sequentially; the tree's 6 levels + the carry); its factors carry
  sum_j (2 + 23 dtau_j) u.  One side: (38 + x + 4 N_k + 23 tau_after_k) u; the backlight is term 0 with b exact.
  Both sides: budget_I = u * sum_k term_k * (C0 + 2 x_k + C1 N_k + C2 tau_after_k),  C0 = 76, C1 = 8, C2 = 46,
  + a floor of (4 * cells) * 2^-1074 for products that underflow (each loses at most one subnormal spacing, and every later
  factor is <= 1).
* tau = sum_j dtau_j, any order: each dtau carries 23 u a side and passes through fewer additions than there are cells:
  budget_tau = u * (CT0 + CT1 * cells) * tau, CT0 = 46, CT1 = 2, + the same floor.

The budgets are checked against np.longdouble (test 1) so that the yardstick itself is honest.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

EPS = 2.0 ** -53
C0, C1, C2, CT0, CT1 = 76.0, 8.0, 46.0, 46.0, 2.0
TINY = 2.0 ** -1074
LIGHT = 299792458.0
WAVELENGTHS = (1064e-9, 532e-9, 266e-9, 100e-9)


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
def _bands(wavelengths):
    """(omega, e_ph, c_omega) per band: the bits the host hands the kernel (engine.emission_params)."""
    from synthpy_amd import engine

    om = 2 * np.pi * LIGHT / np.atleast_1d(np.float64(wavelengths))
    p = engine.emission_params(om, 2)
    n = p.n_band
    return list(p.omega)[:n], list(p.e_ph)[:n], list(p.c_omega)[:n]


def _node(ne, Te, Z, omega, e_ph, c_omega):
    """alpha and S per node for one band, in the dtype of the inputs (float64: the rule; np.longdouble: the same formulas wide).
    The constants are the float64 constants of the rule in either case."""
    dark = (Te <= 0) | (ne <= 0)
    with np.errstate(all="ignore"):
        n = ne * 1e-6
        wp = 5.64e4 * np.sqrt(n)
        q = np.sqrt(Te)
        L = np.maximum(Z * 1.602176634e-19 / Te, 2.760428269727312e-10 / q)
        w = np.maximum(wp, omega)
        lnL = np.maximum(2.0, np.log(4.19e5 * q / (w * L)))
        r = n / omega
        al = (((((3.1e-5 * Z) * LIGHT) * (r * r)) * lnL) * (1.0 / (Te * q))) / LIGHT
        x = e_ph / Te
        S = c_omega / np.expm1(x)
    zero = np.zeros((), al.dtype)
    return np.where(dark, zero, al), np.where(dark, zero, S), np.where(dark, 0.0, np.float64(x))


def restate(ne, Te, Z, g, bands, axis, toward=+1, backlight=None, dtype=np.float64):
    """include/synthray.h's rule, sequentially.  ne, Te, Z: (nx, ny, nz) arrays or scalars (uniform); g: the float32 node
    coordinates of `axis`; bands = (omega, e_ph, c_omega) lists.  Returns (I, tau, budget_I, budget_tau), each (n_band, n_u, n_v);
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
    for b, (omega, e_ph, c_omega) in enumerate(zip(*bands)):
        al, S, x = _node(ne, Te, Z, omega, e_ph, c_omega)
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
                cells.append((np.float64(a), np.float64(bb), np.float64(dt), np.maximum(x[k], x[k + 1])))
            # the budget, from the last cell back: P = the product of the later factors, N their number, ta their optical depth
            P, ta, bud = np.ones(I.shape), np.zeros(I.shape), np.zeros(I.shape)
            for N, (a, bb, dt, xk) in enumerate(reversed(cells)):
                bud = bud + bb * P * (C0 + 2 * xk + C1 * N + C2 * ta)
                P, ta = P * a, ta + dt
            bud = bud + np.float64(I0) * P * (2 + C1 * (n - 1) + C2 * ta)
        out.append((I, tau, EPS * bud + 4 * (n - 1) * TINY, EPS * (CT0 + CT1 * (n - 1)) * np.float64(tau) + 4 * (n - 1) * TINY))
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
    """The conditions on tested inputs: every column non-empty, every budget below 1e-9 of its value, a thin and a thick column."""
    I, tau, bI, bt = ref
    assert np.all(tau > 0) and np.all(I > 0), f"{what}: an empty column"
    assert np.all(bI < 1e-9 * I) and np.all(bt < 1e-9 * tau), f"{what}: a budget above 1e-9 of its value"
    assert np.any(tau < 1e-3) and np.any((tau > 1) & (tau < 30)), f"{what}: tau spans {tau.min():.2e} .. {tau.max():.2e}"


# ---------------------------------------------------------------- inputs
def _coords(n, seed, half=4e-3):
    """Non-uniform float32 node coordinates inside +-half, no two nodes closer than a fifth of the widest gap."""
    g = np.cumsum(np.random.default_rng(seed).uniform(0.2, 1.0, n))
    return np.float32(-half + (g - g[0]) * (2 * half / (g[-1] - g[0])))


AXIS_N = (2, 3, 63, 64, 65, 129)
LATERAL = ((5, 7), (67, 3))
_CASES = {}


def _case(axis, n, lateral):
    """Fields of one shape, made once (toward only changes the march): ne log-uniform over four decades -- one decade node by
    node times a factor per column spread over three -- scaled so that the thickest column has tau ~ 10 at 1064 nm; Te in
    [1, 500] eV, Z in [1, 30]; the restatement for both marches, 4 bands."""
    key = (axis, n, lateral)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * axis + 10 * n + lateral[0])
        shape = list(lateral)
        shape.insert(axis, n)
        col = list(lateral)
        col.insert(axis, 1)
        per_col = 10.0 ** (-3 * rng.permutation(lateral[0] * lateral[1]) / (lateral[0] * lateral[1] - 1)).reshape(col)
        ne = 1e26 * 10.0 ** (-rng.random(shape)) * per_col
        Te = rng.uniform(1.0, 500.0, shape)
        Z = rng.uniform(1.0, 30.0, shape)
        co = [_coords(m, 7 + k) for k, m in enumerate(shape)]
        bands = _bands(WAVELENGTHS)
        one = tuple(v[:1] for v in bands)
        tau_max = restate(ne, Te, Z, co[axis], one, axis)[1].max()
        ne = ne * np.sqrt(10.0 / tau_max)
        back = rng.uniform(0.0, 2e-7, (4,) + tuple(lateral))
        refs = {t: restate(ne, Te, Z, co[axis], bands, axis, t, back) for t in (+1, -1)}
        for a in (ne, Te, Z, back) + tuple(v for r in refs.values() for v in r):
            a.setflags(write=False)
        _CASES[key] = dict(ne=ne, Te=Te, Z=Z, co=co, bands=bands, back=back, refs=refs)
    return _CASES[key]


def _run(eng, ne, Te, Z, co, wavelengths, axis, toward, backlight=None):
    """engine.emission on freshly uploaded fields; Te, Z arrays or floats."""
    om = 2 * np.pi * LIGHT / np.atleast_1d(np.float64(wavelengths))
    fields = [eng.Field(a, *co) if np.ndim(a) else float(a) for a in (ne, Te, Z)]
    try:
        return eng.emission(*fields, om, axis, toward, backlight)
    finally:
        for f in fields:
            if not isinstance(f, float):
                f.close()


# ================================================================ CPU tests
def test_restatement_against_longdouble(built):
    """1: the yardstick against the same recurrence in np.longdouble (64-bit mantissa here), within its own budget."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    for axis, n, lateral in ((2, 65, (5, 7)), (0, 129, (5, 7)), (1, 3, (67, 3))):
        K = _case(axis, n, lateral)
        for t in (+1, -1):
            wide = restate(K["ne"], K["Te"], K["Z"], K["co"][axis], K["bands"], axis, t, K["back"], dtype=np.longdouble)
            _assert_close(np.float64(wide[0]), np.float64(wide[1]), K["refs"][t], f"restatement vs longdouble axis {axis} n {n} toward {t:+d}")


def test_tested_inputs_meet_the_conditions(built):
    """Every parametrisation of the kernel test: non-empty columns, budgets below 1e-9, a thin and a thick column -- for the
    four bands together and for the one-band call (1064 nm)."""
    for axis in range(3):
        for n in AXIS_N:
            for lateral in LATERAL:
                K = _case(axis, n, lateral)
                for t in (+1, -1):
                    _assert_inputs(K["refs"][t], f"axis {axis} n {n} lateral {lateral} toward {t:+d}")
                    _assert_inputs(tuple(v[:1] for v in K["refs"][t]), f"axis {axis} n {n} lateral {lateral} toward {t:+d} one band")


def test_telescoping_identities(built):
    """2: a uniform slab gives S (1 - exp(-alpha L)); constant Te with random ne gives B(Te) (1 - exp(-tau)): exact for this
    discretisation (the differences telescope), checked within the budget against np.longdouble."""
    Lw = np.longdouble
    bands = _bands(WAVELENGTHS)
    g = _coords(40, 3)
    shape = (3, 4, 40)
    rng = np.random.default_rng(2)
    length = Lw(np.float64(g[-1])) - Lw(np.float64(g[0]))
    for ne0, Te0, Z0 in ((3e25, 80.0, 6.0), (2e24, 3.0, 1.0), (4e26, 450.0, 29.0)):
        I, tau, bI, bt = restate(np.full(shape, ne0), Te0, Z0, g, bands, 2)
        for b in range(4):
            al, S, _ = _node(Lw(ne0), Lw(Te0), Lw(Z0), bands[0][b], bands[1][b], bands[2][b])
            want = S * (-np.expm1(-al * length))
            d = np.abs(Lw(I[b]) - want)
            print(f"uniform slab ne {ne0:g} Te {Te0:g} band {b}: tau {float(al * length):.3e}, max |d| / budget {float(np.max(d / bI[b])):.3f}")
            assert np.all(d <= bI[b]) and np.all(np.abs(Lw(tau[b]) - al * length) <= bt[b])
    ne = 1e26 * 10.0 ** (-4 * rng.random(shape))
    for Te0 in (2.0, 60.0, 500.0):
        I, tau, bI, bt = restate(ne, Te0, 5.0, g, bands, 2)
        wide = restate(ne, Te0, 5.0, g, bands, 2, dtype=Lw)
        for b in range(4):
            _, S, _ = _node(Lw(1e25), Lw(Te0), Lw(5.0), bands[0][b], bands[1][b], bands[2][b])
            want = S * (-np.expm1(-wide[1][b]))
            d = np.abs(Lw(I[b]) - want)
            print(f"constant Te {Te0:g} band {b}: tau {float(tau[b].min()):.3e} .. {float(tau[b].max()):.3e}, max |d| / budget {float(np.max(d / bI[b])):.3f}")
            assert np.all(d <= bI[b])


def test_header_ctypes_and_python_signatures(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "synthray.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sr_field_emission\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 8
    assert re.search(r"#define\s+SR_MAX_BANDS\s+4", text) and built.MAX_BANDS == 4
    assert C.sizeof(built.EmissionParams) == 4 * 4 + 8 * (3 * 4 + 2)
    assert built.SYMBOLS["sr_field_emission"][0] is C.c_int and len(built.SYMBOLS["sr_field_emission"][1]) == 8
    assert "emission.hip" in open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()

    from synthpy_amd import emission, engine
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.emission) == ["ne", "Te", "Z", "omegas", "axis", "toward", "backlight"]
    assert names(emission.self_emission) == ["domain", "wavelengths", "toward", "backlight", "fields"]
    assert names(NewDomain.self_emission) == names(OldDomain.self_emission) == ["self", "wavelengths", "toward", "backlight"]
    # the host's band constants against their definitions in np.longdouble: a few roundings each
    Lw = np.longdouble
    om = 2 * np.pi * LIGHT / np.float64(WAVELENGTHS)
    p = engine.emission_params(om, 1, -1, Te=12.5, Z=3.0)
    assert (p.axis, p.toward, p.n_band, p.Te, p.Z) == (1, -1, 4, 12.5, 3.0)
    hbar = Lw(6.62607015e-34) / (2 * Lw(np.pi))
    for b in range(4):
        assert p.omega[b] == om[b]
        assert abs(p.e_ph[b] - hbar * Lw(om[b]) / Lw(1.602176634e-19)) <= 8 * EPS * p.e_ph[b]
        assert abs(p.c_omega[b] - hbar * Lw(om[b]) ** 3 / (4 * Lw(np.pi) ** 3 * Lw(LIGHT) ** 2)) <= 16 * EPS * p.c_omega[b]
    assert 1.16 < p.e_ph[0] < 1.17 and 12.3 < p.e_ph[3] < 12.5  # eV at 1064 nm and at 100 nm


def test_argument_checks_come_before_the_device(built):
    """3: every rejected argument is SR_ERR_INVALID with its own text, on a machine with or without a GPU (the checks that need a
    live sr_field -- vector fields, dtypes, grids -- are exercised on the GPU)."""
    from synthpy_amd import emission, engine
    from synthpy_amd.simulator.domain import ScalarDomain

    lib, ptr = built.lib, built.ptr
    out = np.zeros((1, 2, 2))
    om = 2 * np.pi * LIGHT / 532e-9

    def call(p, I=out, tau=out):
        return lib.sr_field_emission(None, None, None, None if p is None else C.byref(p), None, ptr(I), ptr(tau), None)

    good = engine.emission_params([om], 2)
    assert call(None) == -1 and "NULL" in built.last_error()
    assert call(good, I=None) == -1 and "NULL" in built.last_error()
    assert call(good, tau=None) == -1 and "NULL" in built.last_error()
    for omegas in ([], [om] * 5):
        assert call(engine.emission_params(omegas, 2)) == -1 and "n_band" in built.last_error(), built.last_error()
    for bad in (0.0, -om, np.nan, np.inf):
        assert call(engine.emission_params([om, bad], 2)) == -1 and "omega of band 1" in built.last_error(), built.last_error()
    for toward in (0, 2, -3):
        assert call(engine.emission_params([om], 2, toward)) == -1 and "toward" in built.last_error()
    for axis in (3, -1):
        assert call(engine.emission_params([om], axis)) == -1 and "axis" in built.last_error()
    assert call(good) == -1 and "NULL ne" in built.last_error()  # every other argument was in order
    assert "sr_field_emission" in built.last_error()

    with pytest.raises(ValueError, match="Field"):
        engine.emission(np.zeros((2, 2, 2)), 1.0, 1.0, [om], 2)
    dom = ScalarDomain(2e-3, 4, ne_type="test_slab")
    with pytest.raises(ValueError, match=r"needs external_Te\(\) and external_Z\(\)"):
        dom.self_emission(532e-9)
    dom.external_Te(50.0)
    with pytest.raises(ValueError, match=r"needs external_Te\(\) and external_Z\(\)"):
        emission.self_emission(dom, 532e-9)
    dom.external_Z(2.0)
    for lam in ([], [532e-9] * 5, 0.0, -1e-7, np.nan, [532e-9, np.inf]):
        with pytest.raises(ValueError, match="wavelengths"):
            dom.self_emission(lam)
    for toward in (0, "z", None):
        with pytest.raises(ValueError, match="toward"):
            dom.self_emission(532e-9, toward=toward)
    dom.probing_direction = "w"
    with pytest.raises(ValueError, match="probing_direction"):
        dom.self_emission(532e-9)


def test_emission_object_without_a_device(built):
    """4: Emission.after, sample and transmission on hand-made maps."""
    from synthpy_amd.emission import Emission
    from synthpy_amd.projection import Projection, bilinear

    gu, gv = np.array([0.0, 1.0, 3.0]), np.array([-1.0, 0.0, 2.0, 3.0])
    U, V = np.meshgrid(gu, gv, indexing="ij")
    I1, t1 = np.stack([1 + U + 2 * V, 5 - U * V]), np.stack([0.5 + 0 * U, 0.1 * (U + 1)])
    I2, t2 = np.stack([2 + 0 * U, 1 + U]), np.stack([1.0 + V * 0, 2.0 + V])
    lam = [532e-9, 100e-9]
    near, far = Emission(I1, t1, ("x", "z"), (gu, gv), lam), Emission(I2, t2, ("x", "z"), (gu, gv), lam)
    assert near.axes == ("x", "z") and near.intensity.shape == (2, 3, 4) and np.array_equal(near.wavelengths, lam)
    assert np.array_equal(near.transmission, np.exp(-t1))
    both = near.after(far)
    assert np.array_equal(both.intensity, I2 * np.exp(-t1) + I1) and np.array_equal(both.optical_depth, t2 + t1)
    assert np.allclose(both.transmission, near.transmission * far.transmission, rtol=1e-15, atol=0)
    # the bilinear rule is Projection.sample's: a bilinear map comes back exactly, outside is NaN
    p, q = np.array([0.0, 0.5, 2.0, 3.0, 3.1, 1.0]), np.array([-1.0, 1.0, 2.5, 3.0, 0.0, -1.5])
    got = near.sample(p, q, "intensity")
    assert got.shape == (2, 6) and np.all(np.isnan(got[:, 4:])) and np.allclose(got[0, :4], 1 + p[:4] + 2 * q[:4], rtol=1e-15)
    proj = Projection.from_integrals((gu, gv), omega=1.0, axes=("x", "z"), ne=I1[1])
    assert np.array_equal(near.sample(p, q)[1], proj.sample(p, q, "areal_density"), equal_nan=True)
    assert np.array_equal(near.sample(p, q, "transmission"), bilinear((gu, gv), np.exp(-t1), p, q), equal_nan=True)
    with pytest.raises(ValueError, match="what"):
        near.sample(p, q, "phase")
    with pytest.raises(ValueError, match="shape"):
        Emission(I1[:1], t1, ("x", "z"), (gu, gv), lam)
    with pytest.raises(ValueError, match="differ"):
        near.after(Emission(I2, t2, ("x", "y"), (gu, gv), lam))
    with pytest.raises(ValueError, match="differ"):
        near.after(Emission(I2, t2, ("x", "z"), (gu, gv), [532e-9, 266e-9]))


# ================================================================ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("lateral", LATERAL, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("n", AXIS_N)
@pytest.mark.parametrize("toward", [+1, -1], ids=["plus", "minus"])
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_kernel_against_restatement(eng, axis, toward, n, lateral):
    """5: I and tau within budget, equal NaN sets, finite outputs; 4 bands and 1 band (whose restatement is band 0 of the four)."""
    K = _case(axis, n, lateral)
    ref = K["refs"][toward]
    what = f"axis {'xyz'[axis]} toward {toward:+d} n {n} lateral {lateral}"
    _assert_inputs(ref, what)
    I, tau = _run(eng, K["ne"], K["Te"], K["Z"], K["co"], WAVELENGTHS, axis, toward, K["back"])
    assert I.shape == (4,) + lateral and np.all(np.isfinite(I)) and np.all(np.isfinite(tau))
    _assert_close(I, tau, ref, what + " 4 bands")
    I1, tau1 = _run(eng, K["ne"], K["Te"], K["Z"], K["co"], WAVELENGTHS[:1], axis, toward, K["back"][:1])
    one = tuple(v[:1] for v in ref)
    _assert_inputs(one, what)
    _assert_close(I1, tau1, one, what + " 1 band")


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 2], ids=["x", "z"])
def test_input_kinds(eng, axis):
    """6: float32 fields against the restatement on their widened values; Te / Z as uniform values give the bits of
    constant-filled fields, in every combination; a repeated call gives identical bits; mismatched fields are refused."""
    lateral, n = (5, 7), 65
    K = _case(axis, n, lateral)
    bands = tuple(v[:2] for v in K["bands"])
    ne32, Te32, Z32 = (np.float32(K[k]) for k in ("ne", "Te", "Z"))
    ref = restate(np.float64(ne32), np.float64(Te32), np.float64(Z32), K["co"][axis], bands, axis, -1)
    _assert_inputs(ref, "float32 fields")
    I, tau = _run(eng, ne32, Te32, Z32, K["co"], WAVELENGTHS[:2], axis, -1)
    _assert_close(I, tau, ref, f"axis {'xyz'[axis]} float32 fields")
    I64, tau64 = _run(eng, np.float64(ne32), np.float64(Te32), np.float64(Z32), K["co"], WAVELENGTHS[:2], axis, -1)
    assert np.array_equal(I, I64) and np.array_equal(tau, tau64), "float32 fields and their float64 widening differ"

    shape = K["ne"].shape
    om = 2 * np.pi * LIGHT / np.float64(WAVELENGTHS[:3])
    for dtype in (np.float32, np.float64):
        f_ne = eng.Field(K["ne"].astype(dtype), *K["co"])
        f_Te, f_Z = eng.Field(np.full(shape, 37.5, dtype), *K["co"]), eng.Field(np.full(shape, 4.0, dtype), *K["co"])
        v_Te = eng.Field(K["Te"].astype(dtype), *K["co"])
        try:
            full = eng.emission(f_ne, f_Te, f_Z, om, axis, +1, K["back"][:3])
            assert f_ne.last_kernel_ms > 0
            for Te, Z in ((37.5, f_Z), (f_Te, 4.0), (37.5, 4.0)):
                part = eng.emission(f_ne, Te, Z, om, axis, +1, K["back"][:3])
                assert np.array_equal(full[0], part[0]) and np.array_equal(full[1], part[1]), (dtype, type(Te), type(Z))
            again = eng.emission(f_ne, f_Te, f_Z, om, axis, +1, K["back"][:3])
            assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1]), "a repeated call returned other bits"
            a, b = eng.emission(f_ne, v_Te, 4.0, om, axis, -1), eng.emission(f_ne, v_Te, 4.0, om, axis, -1)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "a repeated call returned other bits"
        finally:
            for f in (f_ne, f_Te, f_Z, v_Te):
                f.close()

    # the checks that need live handles
    from synthpy_amd._ffi import SynthrayError

    co2 = [c.copy() for c in K["co"]]
    co2[1][2] = np.nextafter(co2[1][2], np.float32(1))
    fields = dict(ne=eng.Field(K["ne"], *K["co"]), vec=eng.Field(np.zeros(shape + (3,)), *K["co"]),
                  f32=eng.Field(np.float32(K["Te"]), *K["co"]), moved=eng.Field(K["Te"], *co2),
                  short=eng.Field(K["Te"][:, :-1], K["co"][0], K["co"][1][:-1], K["co"][2]))
    try:
        for Te, text in ((fields["vec"], "vector"), (fields["f32"], "dtype"), (fields["moved"], "grids"), (fields["short"], "grids")):
            with pytest.raises(SynthrayError, match=text):
                eng.emission(fields["ne"], Te, 3.0, om, axis)
        with pytest.raises(SynthrayError, match="vector"):
            eng.emission(fields["vec"], 10.0, 3.0, om, axis)
        with pytest.raises(ValueError, match="backlight"):
            eng.emission(fields["ne"], 10.0, 3.0, om, axis, backlight=K["back"][:2])
    finally:
        for f in fields.values():
            f.close()


def _layers(axis, n=40, lateral=(4, 3)):
    """A column that is hot and thin in its first half of planes and cold and thick in the second, with a little noise."""
    rng = np.random.default_rng(70 + axis)
    shape = list(lateral)
    shape.insert(axis, n)
    k = np.arange(n).reshape([n if d == axis else 1 for d in range(3)])
    front = k < n // 2
    ne = np.where(front, 2e24, 2.5e25) * rng.uniform(0.8, 1.2, shape)
    Te = np.where(front, 400.0, 5.0) * rng.uniform(0.9, 1.1, shape)
    co = [_coords(m, 40 + d) for d, m in enumerate(shape)]
    return ne, Te, 4.0, co


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 2], ids=["x", "z"])
def test_order_matters(eng, axis):
    """7: the two detector sides see different images (by more than 100 budgets), and marching backwards equals marching forwards
    through the fields flipped along the axis."""
    ne, Te, Z, co = _layers(axis)
    lam = WAVELENGTHS[:2]
    bands = _bands(lam)
    ref = {t: restate(ne, Te, Z, co[axis], bands, axis, t) for t in (+1, -1)}
    for t in (+1, -1):
        assert np.all(ref[t][1] > 1) and np.all(ref[t][1] < 30)
    assert np.all(np.abs(ref[+1][0] - ref[-1][0]) > 100 * (ref[+1][2] + ref[-1][2])), "the restatement's two sides do not differ"
    got = {t: _run(eng, ne, Te, Z, co, lam, axis, t) for t in (+1, -1)}
    for t in (+1, -1):
        _assert_close(*got[t], ref[t], f"layers axis {'xyz'[axis]} toward {t:+d}")
    gap = np.abs(got[+1][0] - got[-1][0]) / (ref[+1][2] + ref[-1][2])
    print(f"hot thin front, cold thick back: the two sides differ by {float(gap.min()):.3e} budgets at least; "
          f"I+ / I- = {float(np.median(got[+1][0] / got[-1][0])):.3e}")
    assert np.all(gap > 100)
    flip = lambda a: np.ascontiguousarray(np.flip(a, axis=axis))
    co_f = list(co)
    co_f[axis] = np.float32(-co[axis][::-1])
    I_f, tau_f = _run(eng, flip(ne), flip(Te), Z, co_f, lam, axis, +1)
    _assert_close(I_f, tau_f, ref[-1], f"flipped fields forwards against the backward march, axis {'xyz'[axis]}")
    d = np.abs(I_f - got[-1][0]) / (2 * ref[-1][2])
    print(f"backward march against the flipped fields forwards: bit-equal {np.array_equal(I_f, got[-1][0])}, max |d| / (2 budgets) = {float(d.max()):.3f}")
    assert np.all(d <= 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 2], ids=["x", "z"])
def test_edge_columns(eng, axis):
    """8: vacuum, an opaque column, a NaN node, Te = 0 and Te < 0 -- one column each among ordinary ones, 70 planes."""
    n, lateral = 70, (3, 4)
    rng = np.random.default_rng(80 + axis)
    shape = list(lateral)
    shape.insert(axis, n)
    ne = 3e25 * 10.0 ** (-rng.random(shape))
    Te = rng.uniform(20.0, 300.0, shape)
    Z = rng.uniform(1.0, 10.0, shape)
    col = lambda i, j: tuple(slice(None) if d == axis else (i, j)[d - (d > axis)] for d in range(3))
    node = lambda i, j, k: tuple(k if d == axis else (i, j)[d - (d > axis)] for d in range(3))
    ne[col(0, 0)] = 0.0
    ne[col(0, 1)] = 4e27
    Te[col(0, 1)] = rng.uniform(2.0, 4.0, n)
    ne[node(1, 0, 37)] = np.nan
    Te[col(1, 1)] = 0.0
    Te[col(1, 2)] = -5.0
    co = [_coords(m, 50 + d) for d, m in enumerate(shape)]
    lam = WAVELENGTHS[1:3]
    bands = _bands(lam)
    back = rng.uniform(1e-8, 2e-7, (2,) + lateral)
    for t in (+1, -1):
        ref = restate(ne, Te, Z, co[axis], bands, axis, t, back)
        assert np.all(ref[1][:, 0, 1] > 800) and np.all(np.isfinite(ref[0][:, 0, 1])) and np.all(ref[0][:, 0, 1] > 0)
        I, tau = _run(eng, ne, Te, Z, co, lam, axis, t, back)
        _assert_close(I, tau, ref, f"edge columns axis {'xyz'[axis]} toward {t:+d}")
        assert np.array_equal(I[:, 0, 0], back[:, 0, 0]) and np.all(tau[:, 0, 0] == 0), "vacuum column"
        nan = np.zeros(lateral, bool)
        nan[1, 0] = True
        assert np.array_equal(np.isnan(I), np.broadcast_to(nan, I.shape)) and np.array_equal(np.isnan(tau), np.isnan(I))
        for j in (1, 2):
            assert np.array_equal(I[:, 1, j], back[:, 1, j]) and np.all(tau[:, 1, j] == 0), "a column without temperature emitted"
        # the opaque column: the backlight is gone exactly -- another backlight, the same bits
        I2, _ = _run(eng, ne, Te, Z, co, lam, axis, t, 3.0 * back)
        assert np.array_equal(I2[:, 0, 1], I[:, 0, 1]) and np.all(np.isfinite(I[:, 0, 1])) and np.all(tau[:, 0, 1] > 800)
        dark, _ = _run(eng, ne, Te, Z, co, lam, axis, t)
        assert np.array_equal(dark[:, 0, 1], I[:, 0, 1]) and np.all(dark[:, 0, 0] == 0) and np.all(dark[:, 1, 1:3] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [1, 2], ids=["y", "z"])
def test_slabs_chain(eng, axis):
    """9: 65 planes cut at plane 40 into two fields that share it; chained by backlight and by Emission.after, for both marches."""
    from synthpy_amd.emission import Emission

    K = _case(axis, 65, (5, 7))
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
        ref_far = restate(*far[:3], far[3][axis], K["bands"], axis, t, K["back"])
        ref_near = restate(*near[:3], near[3][axis], K["bands"], axis, t, ref_far[0])
        I_far, tau_far = _run(eng, *far, WAVELENGTHS, axis, t, K["back"])
        I_chain, tau_near = _run(eng, *near, WAVELENGTHS, axis, t, I_far)
        I_near0, tau_near0 = _run(eng, *near, WAVELENGTHS, axis, t)
        assert np.array_equal(tau_near, tau_near0)
        em = Emission(I_near0, tau_near0, names, lat, WAVELENGTHS).after(Emission(I_far, tau_far, names, lat, WAVELENGTHS))
        bud_I = ref_near[2] + ref_far[2] + whole[2] + 4 * EPS * whole[0]  # the slabs', the whole's, and after()'s three roundings
        bud_t = ref_near[3] + ref_far[3] + whole[3] + 2 * EPS * whole[1]
        for name, I, tau in (("backlight", I_chain, tau_far + tau_near), ("after", em.intensity, em.optical_depth)):
            dI, dt = np.abs(I - whole[0]) / bud_I, np.abs(tau - whole[1]) / bud_t
            print(f"slabs by {name}, axis {'xyz'[axis]} toward {t:+d}: max |d| / summed budgets: I {float(dI.max()):.3f}, tau {float(dt.max()):.3f}")
            assert np.all(dI <= 1.0) and np.all(dt <= 1.0)


def _domain_fields(n=(12, 10, 14)):
    rng = np.random.default_rng(90)
    return 2e25 * 10.0 ** (-2 * rng.random(n)), rng.uniform(5.0, 200.0, n), rng.uniform(1.0, 8.0, n)


@pytest.mark.gpu
def test_against_line_integrals(eng):
    """10: the optical depth at lwl is the absorption line integral / c.  The projection side: tests/test_projection.py's bound
    (n_a + 8) u sum |w f|; this side: budget_tau; between the two formulations 24 u more -- np.power(Te, -1.5) (1 ulp) against
    1/(Te*sqrt(Te)) (3 roundings): 5 u; the division by c per node against once per column: 2 u; trapezoid weights
    (g[k+1] - g[k-1])/2 per node against 0.5*(f + f')*h per cell: 4 u; omega = 2 pi c / lwl formed twice: 1 u, squared: 4 u;
    float64 kappa attached as computed: 0; the rest second order and slack.  With constant Te the image is
    B(Te) (-expm1(-tau)) of its own optical depth."""
    from synthpy_amd.simulator.domain import ScalarDomain

    lwl = 1064e-9
    dims = (12, 10, 14)
    ne, Te, Z = _domain_fields(dims)
    for direction in "xyz":
        a = "xyz".index(direction)
        dom = ScalarDomain((4e-3, 3e-3, 5e-3), dims, inv_brems=True, probing_direction=direction)
        dom.external_ne(ne)
        dom.external_Te(Te)
        dom.external_Z(Z)
        proj, em = dom.line_integrals(lwl), dom.self_emission(lwl)
        assert em.axes == proj.axes and em.optical_depth.shape == (1,) + proj.shape
        assert all(np.array_equal(u, v) for u, v in zip(em.coords, proj.coords))
        want = proj.integrals["kappa"] / LIGHT
        ref = restate(ne, Te, Z, (dom.x, dom.y, dom.z)[a], _bands([lwl]), a)
        bound = (dims[a] + 8 + 24) * EPS * want + ref[3][0]
        d = np.abs(em.optical_depth[0] - want)
        print(f"probing {direction}: tau {want.min():.3e} .. {want.max():.3e}, max |d| / bound = {float(np.max(d / bound)):.3f}")
        assert np.all(want > 0) and np.all(d <= bound)
        _assert_close(em.intensity, em.optical_depth, ref, f"domain probing {direction}")
        # constant Te (a scalar: not uploaded)
        dom.external_Te(60.0)
        em = dom.self_emission([lwl, 266e-9], toward="-")
        bands = _bands([lwl, 266e-9])
        ref = restate(ne, 60.0, Z, (dom.x, dom.y, dom.z)[a], bands, a, -1)
        for b in range(2):
            S = bands[2][b] / np.expm1(bands[1][b] / 60.0)
            want = S * (-np.expm1(-em.optical_depth[b]))
            bound = ref[2][b] + S * ref[3][b] + 8 * EPS * want  # the budget, tau's budget through dI/dtau <= S, and this line's own roundings
            d = np.abs(em.intensity[b] - want)
            print(f"probing {direction} constant Te band {b}: max |d| / bound = {float(np.max(d / bound)):.3f}")
            assert np.all(d <= bound)


@pytest.mark.gpu
def test_domain_api(eng):
    """11: ScalarDomain.self_emission of both generations for the three probing directions; map shapes and axis names are
    line_integrals'; float32 arrays stay float32 and a broadcast Te goes as a value; the turned domain."""
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy import full_solver as fs

    dims = (12, 10, 14)
    ne, Te, Z = _domain_fields(dims)
    lam = [1064e-9, 100e-9]
    for direction in "xyz":
        a = "xyz".index(direction)
        new = NewDomain((4e-3, 3e-3, 5e-3), dims, probing_direction=direction)
        new.external_ne(np.float32(ne))
        new.external_Te(np.float32(Te))
        new.external_Z(np.broadcast_to(np.float64(3.0), dims))
        co = [np.linspace(-h, h, m) for h, m in zip((2e-3, 1.5e-3, 2.5e-3), dims)]
        old = fs.ScalarDomain(*co, 2.5e-3, probing_direction=direction)
        old.external_ne(np.float32(ne))
        old.external_Te(np.float32(Te))
        old.external_Z(3.0)
        old.calc_dndr(1064e-9)
        ref = restate(np.float64(np.float32(ne)), np.float64(np.float32(Te)), 3.0, (new.x, new.y, new.z)[a], _bands(lam), a)
        for dom in (new, old):
            em, proj = dom.self_emission(lam), dom.line_integrals()
            assert em.axes == proj.axes and em.intensity.shape == (2,) + proj.shape == em.optical_depth.shape
            assert all(np.array_equal(u, v) for u, v in zip(em.coords, proj.coords))
            assert np.array_equal(em.wavelengths, lam) and np.array_equal(em.transmission, np.exp(-em.optical_depth))
            _assert_close(em.intensity, em.optical_depth, ref, f"{type(dom).__module__.split('.')[-1]} probing {direction}")
        del old.Te
        with pytest.raises(ValueError, match=r"needs external_Te\(\) and external_Z\(\)"):
            old.self_emission(lam)

    # turned by 90 degrees about y and probed along z, the domain is the original probed along x: view axes x' = -z, y' = y,
    # z' = x, so a map over (x', y') is the original's (y, z) map transposed, then reversed along its first axis
    n = 24
    x = np.float32((np.arange(n) - (n - 1) / 2) * 2.0 ** -12)  # dyadic and symmetric: the 90 degree resample is a transposition
    rng = np.random.default_rng(91)
    ne, Te = 2e25 * 10.0 ** (-2 * rng.random((n, n, n))), rng.uniform(5.0, 200.0, (n, n, n))
    doms = {}
    for direction in "xz":
        doms[direction] = fs.ScalarDomain(x, x, x, float(x[-1]), probing_direction=direction)
        doms[direction].external_ne(ne)
        doms[direction].external_Te(Te)
        doms[direction].external_Z(4.0)
    view = doms["z"].rotated(90, about="y")
    assert np.array_equal(view.Te, np.flip(np.transpose(Te, (2, 1, 0)), axis=0)) and view.Z == 4.0
    for toward, t in (("+", +1), ("-", -1)):
        ref = restate(ne, Te, 4.0, x, _bands(lam), 0, t)
        A, B = doms["x"].self_emission(lam, toward=toward), view.self_emission(lam, toward=toward)
        assert A.axes == ("y", "z") and B.axes == ("x", "y")
        _assert_close(A.intensity, A.optical_depth, ref, f"probing x toward {toward}")
        for name, bud in (("intensity", ref[2]), ("optical_depth", ref[3])):
            want = np.flip(np.transpose(getattr(A, name), (0, 2, 1)), axis=1)
            d = np.abs(getattr(B, name) - want) / (2 * np.flip(np.transpose(bud, (0, 2, 1)), axis=1))
            print(f"turned domain toward {toward} {name}: bit-equal {np.array_equal(getattr(B, name), want)}, max |d| / (2 budgets) = {float(d.max()):.3f}")
            assert np.all(d <= 1.0)
