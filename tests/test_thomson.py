"""Optical Thomson scattering: sr_field_thomson (thomson.hip), engine.thomson, thomson.Probe / Collection / spectra,
ScalarDomain.thomson_scattering, external_Ti and external_V of both API generations, and Ti / V carried by orientation.rotated.

THE REFERENCE for values is `restate` below: include/synthray.h's rule in NumPy float64, operation for operation (NumPy's
elementwise products and sums are separate calls and cannot fuse; the kernel is compiled with -ffp-contract=off).  The
per-wavelength and per-point lines of the rule use +, *, / and sqrt only, correctly rounded on the host and on the device, so
they are expected to agree bit for bit; the per-sample lines call exp (three times per plasma-dispersion value), whose last bit
is the library's own.  restate(dtype=np.longdouble) keeps the first two stages in float64 and runs every sample's arithmetic in
x87 extended precision (exp included, and the Dawson coefficients C[n] = exp(-(n h)^2) formed there instead of read as rounded
constants): the error of the float64 sample against it is what the bounds are made from.

The error measure of a sample (tests 1 and 5): a relative error u of the plasma-dispersion values W(xi_e), W(xi_i) -- of their
size O(1), not of their possibly tiny real part -- moves chi_e and chi_i by u*alpha^2 and u*alpha^2*Z*Te/Ti, so S by about
u*S*(1 + alpha^2 (1 + Z Te/Ti))/|eps|; exp(-xi_e^2) carries xi_e^2 roundings of its argument (it underflows past 745).  Hence
    test 1   |S - S_ref| / (S_ref * amp),     amp = (1 + |chi_e| + |chi_i|)/|eps|
    test 5   |P - P_ref| <= K u f_l sum_q |term_q| A_q,   A_q = (1 + alpha^2 (1 + Z Te/Ti))/|eps| + min(xi_e^2, 745) + 1
with term_q = w_q ne_q S_q and u = 2^-53.
"""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

U = 2.0 ** -53
LIGHT = 299792458.0
QE, ME, MP, EPS0 = 1.602176634e-19, 9.1093837015e-31, 1.67262192369e-27, 8.8541878128e-12
SP, TSP, ISP = 1.7724538509055159, 3.5449077018110318, 0.5641895835477563
C_N = (0.9394130628134758, 0.569782824730923, 0.2096113871510978, 0.04677062238395898, 0.006329715427485747,
       0.0005195746821548384, 2.586810022265412e-05, 7.811489408304491e-07, 1.4307241918567688e-08, 1.5893910094516368e-10,
       1.0709232382508077e-12, 4.37661850287085e-15, 1.0848552640429378e-17)
LAM_I = 532e-9
# 8 x the largest float64-against-longdouble ratio on test 5's inputs (test_sample_error_constant measures and prints it: 28.2)
K_MEASURED = 28.2
K_SAMPLE = 8 * K_MEASURED
# 8 x the largest of test 1's three measured values against scipy.special.wofz (1.84e-14, the electron-plasma-wave case)
WOFZ_BOUND = 8 * 1.84e-14


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
def _dawson(x, dtype):
    """D(x) of the rule: (F, E)."""
    wide = dtype is not np.float64
    one, two, quarter, half = dtype(1.0), dtype(2.0), dtype(0.25), dtype(0.5)
    isp = one / np.sqrt(dtype(4.0) * np.arctan(one)) if wide else ISP
    n0 = two * np.rint(two * x)
    xp = x - quarter * n0
    g = np.exp(-(xp * xp))
    p = np.exp(half * xp)
    m = one / p
    p2, m2, d0 = p * p, m * m, n0 * n0
    s = np.zeros_like(x)
    for j in range(13):
        n = dtype(2 * j + 1)
        cn = np.exp(-(n * quarter) ** 2) if wide else C_N[j]
        s = s + cn * ((p * (n0 - n) + m * (n0 + n)) / (d0 - n * n))
        p = p * p2
        m = m * m2
    return (g * s) * isp, np.exp(-(x * x))


def wavelength_stage(lam, lam_i, cth):
    """The `volume` and `wavelength` lines: a dict of (n_lambda) arrays, float64."""
    tpc = (2.0 * 3.141592653589793) * LIGHT
    wi = tpc / lam_i
    kin = wi / LIGHT
    ws = tpc / lam
    w = ws - wi
    ksc = ws / LIGHT
    k2 = (ksc * ksc + kin * kin) - ((2.0 * ksc) * kin) * cth
    k = np.sqrt(k2)
    return dict(w=w, ksc=ksc, kin=kin, k=k, rk=1.0 / k, rk2=1.0 / k2, f=(1.0 + (2.0 * w) / wi) * (LIGHT / (lam * lam)), wi=wi)


def point_stage(ne, Te, Ti, Z, vs, vi, wq, A):
    """The `point` line on gathered values (n_q each): a dict of (n_q) arrays and the kept flags, float64."""
    with np.errstate(all="ignore"):
        keep = (ne > 0) & (Te > 0) & (Ti > 0) & ~np.isnan(Z) & ~np.isnan(vs) & ~np.isnan(vi)
        ce, ci, ee0 = (2.0 * QE) / ME, (2.0 * QE) / (A * MP), QE / EPS0
        return dict(keep=keep, wn=wq * ne, ivte=1.0 / np.sqrt(ce * Te), ivti=1.0 / np.sqrt(ci * Ti), pe=(ne * ee0) / Te,
                    zt=(Z * Te) / Ti, Z=Z * np.ones_like(ne), vs=vs * np.ones_like(ne), vi=vi * np.ones_like(ne))


def sample_stage(L, Q, has_v=True, dtype=np.float64):
    """The `sample` lines for every (point, wavelength): a dict of (n_q, n_lambda) arrays -- S, chi_e, chi_i, eps (complex parts),
    xe -- in `dtype`.  L: wavelength_stage, Q: point_stage (the dropped points give whatever their numbers give: mask with keep)."""
    wide = dtype is not np.float64
    one, two = dtype(1.0), dtype(2.0)
    sp = np.sqrt(dtype(4.0) * np.arctan(one)) if wide else SP
    tsp = two * sp if wide else TSP
    q = {k: v.astype(dtype)[:, None] for k, v in Q.items() if k != "keep"}
    l = {k: np.asarray(v, np.float64).astype(dtype)[None, :] for k, v in L.items() if k != "wi" and k != "kin"}
    kin = dtype(L["kin"])
    with np.errstate(all="ignore"):
        wp = l["w"] - (l["ksc"] * q["vs"] - kin * q["vi"]) if has_v else l["w"] + dtype(0.0) * q["vs"]
        a = wp * l["rk"]
        xe, xi = a * q["ivte"], a * q["ivti"]
        al = q["pe"] * l["rk2"]
        az = al * q["zt"]
        Fe, Ee = _dawson(xe, dtype)
        Fi, Ei = _dawson(xi, dtype)
        cer, cei = al * (one - (two * xe) * Fe), al * ((sp * xe) * Ee)
        cir, cii = az * (one - (two * xi) * Fi), az * ((sp * xi) * Ei)
        er, ei = (one + cer) + cir, cei + cii
        ie2 = one / (er * er + ei * ei)
        n1 = (one + cir) * (one + cir) + cii * cii
        n2 = cer * cer + cei * cei
        S = (tsp * l["rk"]) * (((n1 * ie2) * Ee) * q["ivte"] + ((q["Z"] * (n2 * ie2)) * Ei) * q["ivti"])
    return dict(S=S, cer=cer, cei=cei, cir=cir, cii=cii, er=er, ei=ei, xe=xe, al=al, az=az)


def restate_volume(ne, Te, Ti, Z, vs, vi, wq, cth, lam, lam_i, A, has_v=True, dtype=np.float64, parts=False):
    """One volume from gathered point values: (P (n_lambda), weight), and with parts the bound's sum_q |term_q| A_q (n_lambda)."""
    L = wavelength_stage(np.asarray(lam, np.float64), lam_i, cth)
    Q = point_stage(*(np.atleast_1d(np.asarray(v, np.float64)) for v in (ne, Te, Ti, Z, vs, vi, wq)), A)
    s = sample_stage(L, Q, has_v, dtype)
    keep = Q["keep"]
    acc, wsum = np.zeros(len(L["w"]), dtype), 0.0
    scale = np.zeros(len(L["w"]), dtype)
    for j in np.nonzero(keep)[0]:  # ascending
        term = dtype(Q["wn"][j]) * s["S"][j]
        acc = acc + term
        wsum = wsum + Q["wn"][j]
        if parts:
            mod_eps = np.sqrt(s["er"][j] ** 2 + s["ei"][j] ** 2)
            Aq = (1 + s["al"][j] + np.abs(s["az"][j])) / mod_eps + np.minimum(s["xe"][j] ** 2, 745.0) + 1
            scale = scale + np.abs(term) * Aq
    P = acc * L["f"].astype(dtype)
    return (P, wsum, scale * np.abs(L["f"]).astype(dtype)) if parts else (P, wsum)


def _locate(g, p):
    n = len(g)
    with np.errstate(invalid="ignore"):
        inside = (p >= g[0]) & (p <= g[-1])
    q = np.where(inside, p, g[0])
    i = np.clip(np.searchsorted(g, q, side="right") - 1, 0, n - 2)
    return i, (q - g[i]) / (g[i + 1] - g[i]), inside


def gather(F, axes, pts):
    """sr_field_resample's cell / outside / blend rule at pts (N, 3): (values (N[, 3]) float64, inside (N)); F (nx, ny, nz[, 3])."""
    (ci, wx, ix), (cj, wy, iy), (ck, wz, iz) = (_locate(axes[a], pts[:, a]) for a in range(3))
    ux, uy, uz = 1.0 - wx, 1.0 - wy, 1.0 - wz
    w00, w01, w10, w11 = uy * uz, uy * wz, wy * uz, wy * wz
    sel = (lambda di, dj, dk: F[ci + di, cj + dj, ck + dk].astype(np.float64))
    ex = (lambda v: v[:, None]) if F.ndim == 4 else (lambda v: v)
    with np.errstate(invalid="ignore"):
        s = [((sel(di, 0, 0) * ex(w00) + sel(di, 0, 1) * ex(w01)) + sel(di, 1, 0) * ex(w10)) + sel(di, 1, 1) * ex(w11) for di in (0, 1)]
        return ex(ux) * s[0] + ex(wx) * s[1], ix & iy & iz


def restate(fields, axes, pts, wts, ki, ks, lam, lam_i, A, Zu=None, dtype=np.float64, parts=False):
    """The whole rule.  fields: dict with ne, Te and optionally Ti, Z, V arrays.  (P (M, n_lambda), weight (M)[, scale])."""
    M, nq = wts.shape
    out = []
    for m in range(M):
        p = pts[m]
        ne, inside = gather(fields["ne"], axes, p)
        Te = gather(fields["Te"], axes, p)[0]
        Ti = gather(fields["Ti"], axes, p)[0] if fields.get("Ti") is not None else Te
        Z = gather(fields["Z"], axes, p)[0] if fields.get("Z") is not None else np.full(nq, float(Zu))
        has_v = fields.get("V") is not None
        if has_v:
            V = gather(fields["V"], axes, p)[0]
            with np.errstate(invalid="ignore"):
                vs = (V[:, 0] * ks[m, 0] + V[:, 1] * ks[m, 1]) + V[:, 2] * ks[m, 2]
                vi = (V[:, 0] * ki[m, 0] + V[:, 1] * ki[m, 1]) + V[:, 2] * ki[m, 2]
        else:
            vs = vi = np.zeros(nq)
        ne = np.where(inside, ne, 0.0)  # outside: dropped, as ne <= 0 is
        cth = (ki[m, 0] * ks[m, 0] + ki[m, 1] * ks[m, 1]) + ki[m, 2] * ks[m, 2]
        out.append(restate_volume(ne, Te, Ti, Z, vs, vi, wts[m], cth, lam, lam_i, A, has_v, dtype, parts))
    return tuple(np.array([o[k] for o in out]) for k in range(3 if parts else 2))


def wofz_volume(ne, Te, Ti, Z, vs, vi, cth, lam, lam_i, A):
    """The same physics written independently with the Faddeeva function, W = 1 + xi i sqrt(pi) w(xi), at one point with the
    flow components vs = V.ks and vi = V.ki: (S, amp), each (n_lambda)."""
    from scipy.special import wofz

    w_s, w_i = 2 * np.pi * LIGHT / lam, 2 * np.pi * LIGHT / lam_i
    k_s, k_i = w_s / LIGHT, w_i / LIGHT
    k = np.sqrt(k_s ** 2 + k_i ** 2 - 2 * k_s * k_i * cth)
    w = (w_s - w_i) - (k_s * vs - k_i * vi)
    vte, vti = np.sqrt(2 * QE * Te / ME), np.sqrt(2 * QE * Ti / (A * MP))
    xe, xi = w / (k * vte), w / (k * vti)
    al2 = ne * QE / (EPS0 * Te) / k ** 2
    W = lambda x: 1 + x * 1j * np.sqrt(np.pi) * wofz(x)
    che, chi = al2 * W(xe), al2 * (Z * Te / Ti) * W(xi)
    eps = 1 + che + chi
    S = 2 * np.sqrt(np.pi) / k * (np.abs(1 + chi) ** 2 / np.abs(eps) ** 2 * np.exp(-xe ** 2) / vte
                                  + Z * np.abs(che) ** 2 / np.abs(eps) ** 2 * np.exp(-xi ** 2) / vti)
    return S, (1 + np.abs(che) + np.abs(chi)) / np.abs(eps)


# ---------------------------------------------------------------- inputs of the CPU tests
KI90, KS90 = np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0])
CASES = {  # ne, Te, Ti, Z, A, half span [m]
    "collective": (1e24, 100.0, 50.0, 4.0, 12.0, 3e-9),
    "electron-plasma-wave": (1e25, 300.0, 100.0, 1.0, 1.0, 60e-9),
    "non-collective": (1e22, 500.0, 500.0, 1.0, 1.0, 60e-9),
}


# ================================================================ tests without a device
@pytest.mark.parametrize("case", list(CASES))
def test_restatement_against_wofz_and_longdouble(case):
    """restate() against the same physics through scipy.special.wofz and against its own sample arithmetic in longdouble, on
    the issue's three plasmas at 90 degrees, 532 nm, 4097 wavelengths, a flow of 3e4 m/s along the scattering wavevector.
    Measured max |S - S_ref|/(S_ref amp) on the build machine: against wofz 1.00e-14 (collective), 1.84e-14
    (electron-plasma-wave), 1.8e-15 (non-collective); against longdouble 4.1e-15, 7.1e-15, 1.5e-15.  Asserted: 8 x the largest
    against wofz, 1.47e-13, for both references (the margin covers libm differences between hosts)."""
    ne, Te, Ti, Z, A, span = CASES[case]
    lam = np.linspace(LAM_I - span, LAM_I + span, 4097)
    V = 3e4 * (KS90 - KI90) / np.sqrt(2.0)  # along the scattering wavevector of the probe's own wavelength
    vs, vi = float(V @ KS90), float(V @ KI90)
    L = wavelength_stage(lam, LAM_I, 0.0)
    Q = point_stage(*(np.array([v]) for v in (ne, Te, Ti, Z, vs, vi, 1.0)), A)
    S = sample_stage(L, Q)["S"][0]
    P, weight = restate_volume(ne, Te, Ti, Z, vs, vi, 1.0, 0.0, lam, LAM_I, A)
    assert weight == ne and np.array_equal(P, (ne * S) * L["f"])
    S_w, amp = wofz_volume(ne, Te, Ti, Z, vs, vi, 0.0, lam, LAM_I, A)
    r_w = float(np.max(np.abs(S - S_w) / (S_w * amp)))
    S_l = sample_stage(L, Q, dtype=np.longdouble)["S"][0]
    r_l = float(np.max(np.abs(S - S_l) / (S_l * amp)))
    print(f"{case}: max |S - S_ref|/(S_ref amp): wofz {r_w:.2e}, longdouble {r_l:.2e}; amp up to {amp.max():.1f}")
    assert np.all(np.isfinite(S)) and np.all(S > 0)
    assert r_w <= WOFZ_BOUND and r_l <= WOFZ_BOUND


@pytest.mark.parametrize("ne,Te,Ti,Z,A", [(1e24, 100.0, 50.0, 4.0, 12.0), (5e24, 200.0, 40.0, 4.0, 12.0), (1e25, 300.0, 30.0, 6.0, 27.0)])
def test_ion_acoustic_peaks(ne, Te, Ti, Z, A):
    """The red and the blue ion-acoustic peak lie within 5 % of k sqrt(e (Z Te/(1 + 1/alpha^2) + 3 Ti)/(A m_p))."""
    k = np.sqrt(2.0) * 2 * np.pi / LAM_I
    al2 = ne * QE / (EPS0 * Te) / k ** 2
    w_ia = k * np.sqrt(QE * (Z * Te / (1 + 1 / al2) + 3 * Ti) / (A * MP))
    w_i = 2 * np.pi * LIGHT / LAM_I
    w = np.linspace(-2 * w_ia, 2 * w_ia, 4097)
    lam = 2 * np.pi * LIGHT / (w_i + w)
    P, _ = restate_volume(ne, Te, Ti, Z, 0.0, 0.0, 1.0, 0.0, lam, LAM_I, A, has_v=False)
    S = P / wavelength_stage(lam, LAM_I, 0.0)["f"]
    blue, red = w > 0, w < 0
    w_blue, w_red = w[blue][np.argmax(S[blue])], w[red][np.argmax(S[red])]
    print(f"ne {ne:g} Te {Te:g} Ti {Ti:g} Z {Z:g} A {A:g}: alpha {np.sqrt(al2):.2f}, peaks at {w_blue / w_ia:.3f}, {w_red / w_ia:.3f} of the fluid value")
    assert abs(w_blue / w_ia - 1) <= 0.05 and abs(-w_red / w_ia - 1) <= 0.05
    assert S[blue].max() > 3 * S[np.argmin(np.abs(w))]  # resolved peaks, not a single hump


def test_doppler_shift_moves_the_argument_only():
    """S(w; V) is S at w - k.V without flow: the restatement with a flow against the restatement without one whose `w` line is
    shifted by hand -- identical bits, because the shifted argument is formed by the same operations."""
    ne, Te, Ti, Z, A, span = CASES["collective"]
    lam = np.linspace(LAM_I - span / 3, LAM_I + span / 3, 2049)
    V = np.array([2e4, 1e4, -1.5e4])
    vs, vi = float(V @ KS90), float(V @ KI90)
    L = wavelength_stage(lam, LAM_I, 0.0)
    Q1 = point_stage(*(np.array([v]) for v in (ne, Te, Ti, Z, vs, vi, 1.0)), A)
    Q0 = point_stage(*(np.array([v]) for v in (ne, Te, Ti, Z, 0.0, 0.0, 1.0)), A)
    S_flow = sample_stage(L, Q1, True)["S"][0]
    shifted = dict(L, w=L["w"] - (L["ksc"] * vs - L["kin"] * vi))
    S_shift = sample_stage(shifted, Q0, False)["S"][0]
    assert np.array_equal(S_flow, S_shift)
    # and the flow is visible: the two ion-acoustic peaks move by k.V = k (V.khat), to the grid's resolution
    S_rest = sample_stage(L, Q0, False)["S"][0]
    kv = float(np.sqrt(2.0) * 2 * np.pi / LAM_I * (V @ (KS90 - KI90)) / np.sqrt(2.0))
    dw = abs(L["w"][1] - L["w"][0])
    for side in (L["w"] > 0, L["w"] < 0):  # |k.V| is less than half the ion-acoustic frequency: each peak stays on its side
        moved = L["w"][side][np.argmax(S_flow[side])] - L["w"][side][np.argmax(S_rest[side])]
        assert abs(moved - kv) <= 2 * dw and abs(kv) > 20 * dw, (moved, kv, dw)


def test_dawson_against_scipy():
    """D(x) of the rule on [-40, 40] against the same form in longdouble and against scipy.special.dawsn, absolute (F <= 0.55)
    and, beyond |x| = 0.5, relative; exp(-x^2) against numpy.  Measured: 4.5 u absolute and 9.9 u relative against longdouble
    (asserted: 8 x); scipy's own dawsn is 17.5 u from the longdouble form, so against it 8 x (9.9 + 17.5) u is asserted."""
    from scipy.special import dawsn

    x = np.concatenate([np.linspace(-40, 40, 200001), [0.0, 0.125, 0.25, 0.375, -0.25, 1e-9, 1e-300]])
    F, E = _dawson(x, np.float64)
    F_l = _dawson(x.astype(np.longdouble), np.longdouble)[0]
    far = np.abs(x) > 0.5
    err, rel = float(np.max(np.abs(F - F_l))), float(np.max(np.abs(F - F_l)[far] / np.abs(F_l)[far]))
    rel_s = float(np.max(np.abs(F - dawsn(x))[far] / np.abs(F_l)[far]))
    print(f"Dawson: against longdouble {err / U:.1f} u absolute, {rel / U:.1f} u relative beyond 0.5; against scipy {rel_s / U:.1f} u")
    assert err <= 8 * 4.5 * U and rel <= 8 * 9.9 * U and rel_s <= 8 * 27.4 * U
    assert np.max(np.abs(F - dawsn(x))) <= 16 * U
    assert np.array_equal(E, np.exp(-(x * x)))


def test_header_ctypes_and_python_signatures(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "synthray.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sr_field_thomson\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 17
    p = re.search(r"typedef struct \{([^}]*)\}\s*sr_thomson_params;", text).group(1)
    assert re.findall(r"(\w+);", p) == [n for n, _ in built.ThomsonParams._fields_] == ["lambda_i", "A", "Z"]
    assert C.sizeof(built.ThomsonParams) == 24
    res, args = built.SYMBOLS["sr_field_thomson"]
    assert res is C.c_int and len(args) == 17 and args[6] is C.c_int64 and args[7] is C.c_int32 and args[12] is C.c_int32
    assert hasattr(built.lib, "sr_field_thomson")
    mk = open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()
    assert "thomson.hip" in mk and "-ffp-contract=off" in mk
    # the constants the header states are the ones this file restates
    header = open(os.path.join(ROOT, "include", "synthray.h")).read()
    for v in C_N + (SP, TSP, ISP, QE, ME, MP, EPS0):
        assert repr(v) in header, v
    assert [repr(float(np.exp(-((2 * j + 1) * 0.25) ** 2))) for j in range(13)] == [repr(v) for v in C_N]
    assert (SP, TSP, ISP) == (float(np.sqrt(np.pi)), float(2 * np.sqrt(np.pi)), float(1 / np.sqrt(np.pi)))

    from synthpy_amd import engine, thomson
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.thomson) == ["ne", "Te", "Ti", "Z", "V", "lambda_i", "ion_mass", "points", "weights", "ki", "ks", "wavelengths"]
    assert names(thomson.spectra) == ["domain", "probe", "collection", "wavelengths", "ion_mass", "instrument_fwhm", "fields"]
    assert names(thomson.Probe.__init__) == ["self", "wavelength", "origin", "direction", "polarisation"]
    assert names(thomson.Collection.__init__)[:6] == ["self", "points", "direction", "length", "n_quad", "beam_radius"]
    for name in ("thomson_scattering", "external_Ti", "external_V", "external_Te", "external_B"):
        assert names(getattr(NewDomain, name)) == names(getattr(OldDomain, name)), name
    assert names(NewDomain.external_Ti) == ["self", "Ti", "Ti_min"] and names(NewDomain.external_V) == ["self", "V"]
    assert names(NewDomain.thomson_scattering) == ["self", "probe", "collection", "wavelengths", "ion_mass", "kw"]
    assert (thomson.R_E, thomson.EPS0, thomson.E_CHARGE) == (2.8179403262e-15, EPS0, QE)


def test_argument_checks_come_before_the_device(built):
    """Every rejected argument is SR_ERR_INVALID with its own text, on a machine with or without a GPU (the checks that need a
    live sr_field -- n_comp, dtypes, grids -- are exercised on the GPU)."""
    from synthpy_amd import engine

    lib, ptr = built.lib, built.ptr
    base = dict(lambda_i=LAM_I, A=12.0, Z=4.0, n_vol=2, n_quad=3, n_lambda=4, pts=np.zeros((2, 3, 3)), wts=np.ones((2, 3)),
                ki=np.tile(KI90, (2, 1)), ks=np.tile(KS90, (2, 1)), lam=np.linspace(531e-9, 533e-9, 4), P=np.zeros((2, 4)),
                weight=np.zeros(2), p=True)

    def call(**kw):
        a = {**base, **kw}
        p = built.ThomsonParams()
        p.lambda_i, p.A, p.Z = a["lambda_i"], a["A"], a["Z"]
        arr = lambda k: None if a[k] is None else ptr(np.ascontiguousarray(a[k], dtype=np.float64))
        rc = lib.sr_field_thomson(None, None, None, None, None, C.byref(p) if a["p"] else None, a["n_vol"], a["n_quad"], arr("pts"),
                                  arr("wts"), arr("ki"), arr("ks"), a["n_lambda"], arr("lam"), arr("P"), arr("weight"), None)
        return rc, built.last_error()

    for name in ("p", "pts", "wts", "ki", "ks", "lam", "P", "weight"):
        rc, err = call(**{name: None})
        assert rc == -1 and "NULL argument" in err, (name, err)
    for name in ("n_vol", "n_quad", "n_lambda"):
        rc, err = call(**{name: -1})
        assert rc == -1 and "must not be negative" in err, (name, err)
    for name in ("lambda_i", "A"):
        for bad in (0.0, -1.0, np.nan, np.inf):
            rc, err = call(**{name: bad})
            assert rc == -1 and name in err, (name, bad, err)
    for bad in (np.nan, np.inf):
        rc, err = call(Z=bad)
        assert rc == -1 and "uniform Z" in err, err
    for bad in (0.0, -532e-9, np.nan, np.inf):
        lam = base["lam"].copy()
        lam[2] = bad
        rc, err = call(lam=lam)
        assert rc == -1 and "lambda[2]" in err, (bad, err)
    for name in ("ki", "ks"):
        for bad in ((0.0, 0.0, 1.1), (0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (np.inf, 0.0, 0.0)):
            d = base[name].copy()
            d[1] = bad
            rc, err = call(**{name: d})
            assert rc == -1 and f"{name} of volume 1" in err, (name, bad, err)
    rc, err = call(ks=np.tile(KI90, (2, 1)))
    assert rc == -1 and "ki equals ks in volume 0" in err, err
    rc, err = call()  # every other argument was in order
    assert rc == -1 and "NULL field" in err and "sr_field_thomson" in err, err
    # n_vol == 0 or n_lambda == 0 succeeds, but not before the fields were looked at
    assert call(n_vol=0)[0] == -1 and call(n_lambda=0)[0] == -1

    z = np.zeros((2, 2, 2))
    with pytest.raises(ValueError, match="ne must be an open engine.Field"):
        engine.thomson(z, z, None, 1.0, None, LAM_I, 12.0, base["pts"], base["wts"], KI90, KS90, base["lam"])


def test_python_argument_checks(built):
    from synthpy_amd import thomson
    from synthpy_amd.simulator.domain import ScalarDomain

    with pytest.raises(ValueError, match="wavelength"):
        thomson.Probe(-1.0, (0, 0, 0), (0, 0, 1))
    with pytest.raises(ValueError, match="zero length"):
        thomson.Probe(LAM_I, (0, 0, 0), (0, 0, 0))
    with pytest.raises(ValueError, match="perpendicular"):
        thomson.Probe(LAM_I, (0, 0, 0), (0, 0, 1), polarisation=(0, 1, 1))
    pr = thomson.Probe(LAM_I, (0, 0, 0), (0, 0, 3.0), polarisation=(2.0, 0, 0))
    assert np.array_equal(pr.direction, (0, 0, 1)) and np.array_equal(pr.polarisation, (1, 0, 0))
    pts = np.zeros((4, 3))
    for kw, msg in ((dict(length=-1.0, n_quad=3), "length"), (dict(length=1e-4, n_quad=0), "n_quad"), (dict(length=1e-4), "needed"),
                    (dict(length=1e-4, n_quad=2, beam_radius=-1.0), "beam_radius"),
                    (dict(quadrature=(np.zeros((4, 2, 3)), np.zeros((4, 3)))), "quadrature"),
                    (dict(length=1e-4, n_quad=2, quadrature=(np.zeros((4, 2, 3)), np.zeros((4, 2)))), "either")):
        with pytest.raises(ValueError, match=msg):
            thomson.Collection(pts, (0, 1, 0), **kw)
    with pytest.raises(ValueError, match="direction must have shape"):
        thomson.Collection(pts, np.ones((3, 3)), length=1e-4, n_quad=2)
    dom = ScalarDomain(4e-3, 5)
    dom.external_ne(np.full((5, 5, 5), 1e24))
    coll = thomson.Collection(pts, (0, 1, 0), length=1e-4, n_quad=2)
    lam = np.linspace(531e-9, 533e-9, 8)
    with pytest.raises(ValueError, match="external_Te"):
        dom.thomson_scattering(pr, coll, lam, 12.0)
    dom.external_Te(np.full((5, 5, 5), 100.0))
    dom.external_Z(4.0)
    for bad_lam in (lam.reshape(2, 4), -lam, np.array([np.nan])):
        with pytest.raises(ValueError, match="wavelengths"):
            dom.thomson_scattering(pr, coll, bad_lam, 12.0)
    with pytest.raises(ValueError, match="ion_mass"):
        dom.thomson_scattering(pr, coll, lam, 0.0)
    with pytest.raises(ValueError, match="no scattering wavevector"):
        dom.thomson_scattering(pr, thomson.Collection(pts, (0, 0, 1), length=1e-4, n_quad=2), lam, 12.0)
    with pytest.raises(ValueError, match="thomson.Probe"):
        dom.thomson_scattering(None, coll, lam, 12.0)


def test_quadrature(built):
    """Gauss-Legendre along the probe, centred on the point, weights summing to the length; the 7-point disc rule integrates the
    polynomials of degree <= 5 over the beam's cross-section exactly; a given (points, weights) passes through."""
    from synthpy_amd import thomson

    d = np.array([1.0, 2.0, -2.0]) / 3.0
    pr = thomson.Probe(LAM_I, (0, 0, 0), d)
    centres = np.array([[1e-3, 0.0, -1e-3], [0.0, 2e-3, 0.0]])
    pts, wts = thomson.Collection(centres, (0, 1, 0), length=2e-4, n_quad=5).quadrature(pr)
    assert pts.shape == (2, 5, 3) and wts.shape == (2, 5)
    t = (pts - centres[:, None, :]) @ d
    assert np.allclose(pts - centres[:, None, :], t[..., None] * d, atol=1e-18)
    assert np.allclose(t, 1e-4 * np.polynomial.legendre.leggauss(5)[0][None, :], rtol=1e-13, atol=0)
    assert np.allclose(wts.sum(axis=1), 2e-4, rtol=1e-14)
    assert np.allclose(np.sum(wts * t ** 8, axis=1), 2 * 1e-4 ** 9 / 9, rtol=1e-12)  # degree 2n - 1 = 9
    R = 5e-5
    pts7, wts7 = thomson.Collection(centres, (0, 1, 0), length=2e-4, n_quad=5, beam_radius=R).quadrature(pr)
    assert pts7.shape == (2, 35, 3) and np.allclose(wts7.sum(axis=1), 2e-4, rtol=1e-14)
    rel = pts7[0] - centres[0]
    along = rel @ d
    perp = rel - along[:, None] * d
    first = perp[:7]  # the disc about the first Gauss node
    assert np.allclose(np.sort(np.sqrt(np.sum(first ** 2, axis=1))), [0.0] + [R * np.sqrt(2 / 3)] * 6, atol=1e-19)
    e1 = first[1] / np.sqrt(first[1] @ first[1])
    e2 = np.cross(d, e1)
    x, y, wd = first @ e1 / R, first @ e2 / R, wts7[0, :7] / wts7[0, :7].sum()
    for (a, b), exact in {(0, 0): 1.0, (2, 0): 0.25, (0, 2): 0.25, (4, 0): 0.125, (0, 4): 0.125, (2, 2): 1 / 24, (1, 0): 0.0,
                          (1, 1): 0.0, (3, 0): 0.0, (2, 1): 0.0, (5, 0): 0.0, (3, 2): 0.0, (1, 4): 0.0}.items():
        assert abs(np.sum(wd * x ** a * y ** b) - exact) <= 1e-15, (a, b)
    given = (np.arange(2 * 3 * 3, dtype=float).reshape(2, 3, 3), np.ones((2, 3)))
    q = thomson.Collection(centres, (0, 1, 0), quadrature=given).quadrature(pr)
    assert np.array_equal(q[0], given[0]) and np.array_equal(q[1], given[1])


def test_instrument_convolution_keeps_the_sum(built):
    from synthpy_amd import thomson

    lam = np.linspace(530e-9, 534e-9, 401)
    rng = np.random.default_rng(1)
    power = rng.random((3, 401))
    power[1] = 0.0
    power[1, 0] = 1.0    # a line on the grid's first sample
    power[2] = 0.0
    power[2, 200] = 1.0  # a line in the middle: the kernel itself
    out = thomson.instrument_convolve(power, lam, 0.2e-9)
    assert out.shape == power.shape and np.all(out >= 0)
    assert np.allclose(out.sum(axis=1), power.sum(axis=1), rtol=1e-13)
    sigma = 0.2e-9 / (2 * np.sqrt(2 * np.log(2)))
    g = np.exp(-0.5 * ((lam - lam[200]) / sigma) ** 2)
    assert np.allclose(out[2], g / g.sum(), atol=1e-15)
    half = out[2] >= 0.5 * out[2].max()
    assert abs((lam[half][-1] - lam[half][0]) - 0.2e-9) <= 2 * (lam[1] - lam[0])
    bent = lam.copy()
    bent[7] += 0.3 * (lam[1] - lam[0])
    for bad in (bent, lam ** 2, np.geomspace(530e-9, 534e-9, 401)):
        with pytest.raises(ValueError, match="uniform"):
            thomson.instrument_convolve(power, bad, 0.2e-9)
    with pytest.raises(ValueError, match="instrument_fwhm"):
        thomson.instrument_convolve(power, lam, 0.0)


def test_external_Ti_and_V_mirror_their_models(built):
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    new = NewDomain((6e-3, 5e-3, 4e-3), (6, 5, 4))
    old = OldDomain(np.linspace(-3e-3, 3e-3, 6), np.linspace(-2e-3, 2e-3, 5), np.linspace(-2e-3, 2e-3, 4), 3e-3)
    assert new.Ti is None and new.V is None and getattr(old, "Ti", None) is None and getattr(old, "V", None) is None
    T = np.linspace(-3.0, 40.0, 6 * 5 * 4).reshape(6, 5, 4)
    V = np.arange(6 * 5 * 4 * 3, dtype=np.float64).reshape(6, 5, 4, 3)
    for dom in (new, old):
        dom.external_Te(T)
        dom.external_Ti(T)
        assert np.array_equal(dom.Ti, dom.Te) and dom.Ti.min() == 1.0  # the same floor as Te's
        dom.external_Te(T, 5.0)
        dom.external_Ti(T, Ti_min=5.0)
        assert np.array_equal(dom.Ti, dom.Te) and dom.Ti.min() == 5.0
        dom.external_B(V)
        dom.external_V(V)
        assert dom.V is V and dom.B is V  # kept as given, as B is


# ---------------------------------------------------------------- inputs of the GPU tests
def _axes():
    """9 x 8 x 7 nodes, every axis non-uniform; float32 node coordinates and their float64 values."""
    x = np.float32(np.cumsum([0.0, 0.5, 0.3, 0.8, 0.4, 0.6, 0.7, 0.35, 0.55]) * 1e-3 - 2.1e-3)
    y = np.float32(np.cumsum([0.0, 0.3, 0.5, 0.9, 0.4, 0.6, 1.0, 0.35]) * 1e-3 - 2.0e-3)
    z = np.float32(np.cumsum([0.0, 0.6, 0.45, 0.7, 0.5, 0.65, 0.4]) * 1e-3 - 1.6e-3)
    return (x, y, z), tuple(np.float64(a) for a in (x, y, z))


AX32, AX = _axes()
A_ION = 12.0
NQ_ALL, NL_ALL = (1, 3, 64, 65), (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def _plasma(dtype_name):
    rng = np.random.default_rng(11)
    shape = tuple(len(a) for a in AX)
    dt = np.dtype(dtype_name)
    ne = (1e24 * (0.5 + rng.random(shape))).astype(dt)
    ne[:2, :2, :2] = 0.0  # the first cell holds no plasma
    f = dict(ne=ne, Te=(50 + 100 * rng.random(shape)).astype(dt), Ti=(20 + 60 * rng.random(shape)).astype(dt),
             Z=(2 + 3 * rng.random(shape)).astype(dt), V=(1e5 * rng.standard_normal(shape + (3,))).astype(dt))
    for a in f.values():
        a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _geometry():
    """5 volumes x 65 points, distinct collection directions, and 257 wavelengths about the probe's (the ion feature and some
    of the electron feature).  The first point of volume 0 lies exactly on two faces of the box, of volume 1 outside it, of
    volume 2 in the cell without plasma; every point of volume 4 lies outside (one of them a NaN)."""
    rng = np.random.default_rng(7)
    lo, hi = np.array([a[0] for a in AX]), np.array([a[-1] for a in AX])
    pts = lo + rng.random((5, 65, 3)) * (hi - lo)
    pts[0, 0] = (lo[0], hi[1], 0.1e-3)
    pts[0, 1] = (hi[0], hi[1], hi[2])
    pts[1, 0] = (lo[0] - 1e-9, 0.0, 0.0)
    pts[1, 1] = (0.0, 0.0, np.nextafter(hi[2], np.inf))
    pts[2, 0] = (AX[0][0] + 1e-4, AX[1][0] + 1e-4, AX[2][0] + 1e-4)
    pts[3, 2] = (AX[0][3], AX[1][4], AX[2][5])  # exactly on a node
    pts[4] = hi + (0.1e-3 + rng.random((65, 3)) * 1e-3)
    pts[4, 5, 1] = np.nan
    wts = 1e-5 * (0.5 + rng.random((5, 65)))
    ki = np.tile(np.array([0.0, 0.0, 1.0]), (5, 1))
    ks = np.array([[0, 1, 0], [1, 0, 0], [0.6, 0, 0.8], [0, -0.8, -0.6], [1, 2, 2]], dtype=float)
    ks /= np.sqrt(np.sum(ks * ks, axis=1, keepdims=True))
    lam = np.concatenate([LAM_I + np.linspace(-2e-9, 2e-9, 201), LAM_I + np.linspace(-40e-9, 40e-9, 56)])
    for a in (pts, wts, ki, ks, lam):
        a.setflags(write=False)
    return pts, wts, ki, ks, lam


VARIANTS = {"all fields": ("ne", "Te", "Ti", "Z", "V"), "no V": ("ne", "Te", "Ti", "Z"), "Ti NULL": ("ne", "Te", "Z", "V"),
            "uniform Z": ("ne", "Te", "Ti", "V")}
Z_UNIFORM = 3.5


@functools.lru_cache(maxsize=None)
def _reference(dtype_name, variant, nq, parts=False, wide=False):
    """restate on the first nq points and all 257 wavelengths (a shorter list is its prefix: wavelengths do not interact)."""
    pts, wts, ki, ks, lam = _geometry()
    f = {k: v for k, v in _plasma(dtype_name).items() if k in VARIANTS[variant]}
    out = restate(f, AX, pts[:, :nq], wts[:, :nq], ki, ks, lam, LAM_I, A_ION, Zu=Z_UNIFORM,
                  dtype=np.longdouble if wide else np.float64, parts=parts)
    for a in out:
        a.setflags(write=False)
    return out


def test_sample_error_constant():
    """K of test 5: the float64 restatement against the one whose sample arithmetic runs in longdouble, on test 5's own inputs,
    in units of u f_l sum_q |term_q| A_q.  Measured on the build machine: 28.12 at most over both dtypes, the four variants and
    the four point counts (float32 fields, uniform Z, 3 points, volume 2 at 0.16 nm from the probe: the ion-acoustic resonance,
    where exp(-xi_i^2) carries xi_i^2 roundings that A_q does not count); above 15 only there.  K_SAMPLE = 8 x 28.2 covers two
    sides and an exp that errs by one ulp where libm's is nearly correctly rounded.  This test holds the measurement itself to
    twice the recorded value (another libm)."""
    worst = 0.0
    for dtype_name in ("float32", "float64"):
        for variant in VARIANTS:
            for nq in NQ_ALL:
                P, w, scale = _reference(dtype_name, variant, nq, True)
                P_l, w_l = _reference(dtype_name, variant, nq, False, True)
                assert np.array_equal(w, w_l) and np.array_equal(P == 0, P_l == 0)
                nz = scale > 0
                worst = max(worst, float(np.max(np.abs(P - P_l)[nz] / (U * scale[nz]))))
    print(f"float64 against longdouble samples: at most {worst:.2f} u f_l sum |term| A_q")
    assert worst <= 2 * K_MEASURED


# ================================================================ tests on the GPU
def _fields(eng, dtype_name, variant, override=None):
    f = dict(_plasma(dtype_name))
    f.update(override or {})
    return {k: eng.Field(f[k], *AX32) for k in VARIANTS[variant]}


def _run(eng, F, nq, nl):
    pts, wts, ki, ks, lam = _geometry()
    return eng.thomson(F["ne"], F["Te"], F.get("Ti"), F.get("Z", Z_UNIFORM), F.get("V"), LAM_I, A_ION,
                       np.ascontiguousarray(pts[:, :nq]), np.ascontiguousarray(wts[:, :nq]), ki, ks, lam[:nl])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_kernel_against_the_restatement(eng, dtype_name, variant):
    """Every instantiation of k_thomson on the 9 x 8 x 7 grid, 5 volumes, 1 / 3 / 64 / 65 points (the LDS chunk is 64) and 1 /
    255 / 256 / 257 wavelengths (the tile is 256).  The decisions are asserted equal: where the restatement gives an exact zero
    (every point outside, or without plasma) the kernel does, and nowhere else; the point on the box's faces counts.  The values
    are asserted within K_SAMPLE u f_l sum_q |term_q| A_q per sample and the weights within 2 (Nq + 8) u sum_q |w_q| max|ne|
    (per side the blend's 7 roundings, the product and the Nq - 1 additions).  Printed: the largest ratio reached.
    On an MI355X: at most 15.8 of the allowed 225.6 (float32 fields, no V; 7.0 to 11.3 elsewhere); the weights equal bit for bit."""
    F = _fields(eng, dtype_name, variant)
    pts, wts, ki, ks, lam = _geometry()
    ne_max = float(np.max(_plasma(dtype_name)["ne"]))
    worst, weights_equal = 0.0, True
    try:
        for nq in NQ_ALL:
            P_ref, w_ref, scale = _reference(dtype_name, variant, nq, True)
            for nl in NL_ALL:
                P, w = _run(eng, F, nq, nl)
                assert P.shape == (5, nl) and w.shape == (5,)
                ref, sc = P_ref[:, :nl], scale[:, :nl]
                assert np.array_equal(P == 0, ref == 0), (nq, nl)
                assert np.array_equal(w == 0, w_ref == 0), (nq, nl)
                assert np.all(P[4] == 0) and w[4] == 0 and w[0] > 0
                if nq == 1:
                    assert np.all(P[1] == 0) and np.all(P[2] == 0) and np.all(P[0] > 0)
                assert np.all(np.isfinite(P))
                nz = sc > 0
                ratio = float(np.max(np.abs(P - ref)[nz] / (U * sc[nz]))) if nz.any() else 0.0
                worst = max(worst, ratio)
                assert ratio <= K_SAMPLE, (nq, nl, ratio)
                w_bound = 2 * (nq + 8) * U * np.sum(np.abs(wts[:, :nq]), axis=1) * ne_max
                assert np.all(np.abs(w - w_ref) <= w_bound), (nq, nl)
                weights_equal &= bool(np.array_equal(w, w_ref))
    finally:
        for f in F.values():
            f.close()
    print(f"{dtype_name}, {variant}: largest |P - P_ref| = {worst:.2f} u f_l sum |term| A_q (allowed {K_SAMPLE:g}); "
          f"weights equal bit for bit: {weights_equal}")


@pytest.mark.gpu
def test_repeated_call_returns_identical_bits(eng):
    F = _fields(eng, "float64", "all fields")
    try:
        first = _run(eng, F, 65, 257)
        again = _run(eng, F, 65, 257)
        other = _run(eng, F, 3, 255)   # the scratch block is reused at another size in between
        third = _run(eng, F, 65, 257)
    finally:
        for f in F.values():
            f.close()
    for a, b, c in zip(first, again, third):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert other[0].shape == (5, 255)


@pytest.mark.gpu
def test_nan_node_touches_only_its_own_cells(eng):
    """A NaN node of Te: by the rule a point whose cell holds it gathers NaN (zero weights included) and is dropped, so a volume
    changes exactly when one of its points lies in one of the node's cells -- it loses those points, as the restatement does --
    and every other volume keeps its bits.  Nothing becomes NaN."""
    pts, wts, ki, ks, lam = _geometry()
    node = (4, 3, 3)
    Te = np.array(_plasma("float64")["Te"])
    Te[node] = np.nan
    cells = [np.clip(np.searchsorted(AX[a], pts[:, :, a], side="right") - 1, 0, len(AX[a]) - 2) for a in range(3)]
    with np.errstate(invalid="ignore"):
        inside = np.all([(pts[:, :, a] >= AX[a][0]) & (pts[:, :, a] <= AX[a][-1]) for a in range(3)], axis=0)
    touched = inside & np.all([(cells[a] == node[a]) | (cells[a] == node[a] - 1) for a in range(3)], axis=0)
    hit = np.any(touched, axis=1)
    assert hit.any() and not hit.all(), "the layout must have volumes of both kinds"
    clean = _fields(eng, "float64", "all fields")
    dirty = _fields(eng, "float64", "all fields", {"Te": Te})
    try:
        P0, w0 = _run(eng, clean, 65, 257)
        P1, w1 = _run(eng, dirty, 65, 257)
    finally:
        for f in list(clean.values()) + list(dirty.values()):
            f.close()
    assert np.all(np.isfinite(P1)) and np.all(np.isfinite(w1))
    for m in range(5):
        if hit[m]:
            assert w1[m] < w0[m] and not np.array_equal(P1[m], P0[m])
        else:
            assert P1[m].tobytes() == P0[m].tobytes() and w1[m] == w0[m]
    f = dict(_plasma("float64"), Te=Te)
    P_ref, w_ref, scale = restate(f, AX, pts, wts, ki, ks, lam, LAM_I, A_ION, parts=True)
    ne = np.array(_plasma("float64")["ne"])
    lost = np.array([np.sum((wts * gather(ne, AX, pts.reshape(-1, 3))[0].reshape(5, 65))[m][touched[m]]) for m in range(5)])
    assert np.allclose(w0 - w1, lost, rtol=1e-12, atol=0)
    assert np.all(np.abs(w1 - w_ref) <= 2 * 73 * U * np.sum(wts, axis=1) * ne.max())
    nz = scale > 0
    assert np.max(np.abs(P1 - P_ref)[nz] / (U * scale[nz])) <= K_SAMPLE


@pytest.mark.gpu
def test_field_checks_need_live_fields(eng):
    from synthpy_amd import _ffi as built

    pts, wts, ki, ks, lam = _geometry()
    p = _plasma("float64")
    call = lambda ne, Te, Ti=None, Z=3.0, V=None: eng.thomson(ne, Te, Ti, Z, V, LAM_I, A_ION, np.ascontiguousarray(pts[:, :3]),
                                                              np.ascontiguousarray(wts[:, :3]), ki, ks, lam[:4])
    ne, Te, V = eng.Field(p["ne"], *AX32), eng.Field(p["Te"], *AX32), eng.Field(p["V"], *AX32)
    Te32 = eng.Field(np.float32(p["Te"]), *AX32)
    moved = eng.Field(p["Te"], AX32[0], AX32[1], AX32[2] + np.float32(1e-6))
    small = eng.Field(p["Te"][:-1], AX32[0][:-1], AX32[1], AX32[2])
    try:
        for args, msg in (((ne, V), "Te must have n_comp == 1"), ((ne, Te, None, 3.0, Te), "V must have n_comp == 3"),
                          ((ne, Te32), "ne and Te differ in dtype"), ((ne, Te, moved), "grids of ne and Ti differ on axis 2"),
                          ((ne, Te, None, small), "grids of ne and Z differ on axis 0")):
            with pytest.raises(built.SynthrayError, match=msg):
                call(*args)
        P, w = call(ne, Te)
        assert P.shape == (5, 4) and np.all(P[0] > 0)
        # nothing to do is no error
        P0, w0 = eng.thomson(ne, Te, None, 3.0, None, LAM_I, A_ION, np.zeros((0, 3, 3)), np.zeros((0, 3)), KI90, KS90, lam[:4])
        assert P0.shape == (0, 4) and w0.shape == (0,)
        P1, w1 = eng.thomson(ne, Te, None, 3.0, None, LAM_I, A_ION, np.ascontiguousarray(pts[:, :3]), np.ascontiguousarray(wts[:, :3]),
                             ki, ks, lam[:0])
        assert P1.shape == (5, 0)
        P2, w2 = eng.thomson(ne, Te, None, 3.0, None, LAM_I, A_ION, np.zeros((5, 0, 3)), np.zeros((5, 0)), ki, ks, lam[:4])
        assert np.all(P2 == 0) and np.all(w2 == 0)
        closed = eng.Field(p["Te"], *AX32)
        closed.close()
        with pytest.raises(ValueError, match="closed"):
            call(ne, closed)
    finally:
        for f in (ne, Te, V, Te32, moved, small):
            f.close()


def _domains():
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    new = NewDomain((4e-3, 3e-3, 3.5e-3), (9, 8, 7))
    old = OldDomain(np.linspace(-2e-3, 2e-3, 9), np.linspace(-1.5e-3, 1.5e-3, 8), np.linspace(-1.75e-3, 1.75e-3, 7), 2e-3)
    p = _plasma("float64")
    for d in (new, old):
        d.external_ne(np.array(p["ne"]) + 1e23)
        d.external_Te(np.array(p["Te"]))
        d.external_Z(np.array(p["Z"]))
        d.external_Ti(np.array(p["Ti"]))
        d.external_V(np.array(p["V"]))
    return new, old


@pytest.mark.gpu
def test_public_path_equals_the_engine_call(eng):
    """domain.thomson_scattering of both generations: r_e^2 (1 - (ks.e)^2) times engine.thomson on the collection's own
    quadrature, bit for bit; the same bits with a reused SourceFields; theta and alpha from the host; the instrument function
    applied after."""
    from synthpy_amd import orientation, thomson

    probe = thomson.Probe(LAM_I, (0, 0, -3e-3), (0, 0, 1), polarisation=(1, 0, 0))
    centres = np.array([[0.0, 0.0, 0.0], [0.5e-3, -0.4e-3, 0.3e-3], [-1.0e-3, 0.7e-3, -0.9e-3], [5e-3, 0.0, 0.0]])
    ks = np.array([[0, 1, 0], [0.6, 0.8, 0], [1, 0, 0], [0, 1, 0]], dtype=float)
    coll = thomson.Collection(centres, ks, length=3e-4, n_quad=4, beam_radius=5e-5)
    lam = np.linspace(LAM_I - 2e-9, LAM_I + 2e-9, 300)
    pts, wts = coll.quadrature(probe)
    assert pts.shape == (4, 28, 3)
    for dom in _domains():
        sp = dom.thomson_scattering(probe, coll, lam, A_ION)
        F = {k: eng.Field(getattr(dom, k), dom.x, dom.y, dom.z) for k in ("ne", "Te", "Ti", "Z", "V")}
        try:
            P, w = eng.thomson(F["ne"], F["Te"], F["Ti"], F["Z"], F["V"], LAM_I, A_ION, pts, wts, probe.direction, ks, lam)
        finally:
            for f in F.values():
                f.close()
        pol = 1.0 - ks[:, 0] ** 2
        assert np.array_equal(sp.power, (thomson.R_E * thomson.R_E * pol)[:, None] * P) and np.array_equal(sp.weight, w)
        assert np.all(sp.power[0] > 0) and np.all(sp.power[2] == 0) and np.all(P[2] > 0)  # ks along the polarisation: nothing
        assert np.all(sp.power[3] == 0) and sp.weight[3] == 0 and np.isnan(sp.alpha[3])   # a volume outside the plasma
        assert np.allclose(sp.theta, [np.pi / 2] * 4) and sp.kernel_ms > 0
        ne_c, Te_c = (gather(np.asarray(getattr(dom, k), np.float64), [np.float64(np.float32(a)) for a in (dom.x, dom.y, dom.z)],
                             centres[:3])[0] for k in ("ne", "Te"))
        k = np.sqrt(2.0) * 2 * np.pi / LAM_I
        assert np.allclose(sp.alpha[:3], np.sqrt(ne_c * QE / (EPS0 * Te_c)) / k, rtol=1e-12)
        src = orientation.SourceFields(dom)
        try:
            a = dom.thomson_scattering(probe, coll, lam, A_ION, fields=src)
            uploads = dict(src.fields)
            b = thomson.spectra(dom, probe, coll, lam, A_ION, fields=src)
            assert set(src.fields) == {"ne", "Te", "Ti", "Z", "V"} and all(src.fields[k] is uploads[k] for k in uploads)
            c = thomson.spectra(dom, probe, coll, lam, A_ION, instrument_fwhm=0.1e-9, fields=src)
        finally:
            src.close()
        assert a.power.tobytes() == b.power.tobytes() == sp.power.tobytes()
        assert np.array_equal(c.power, thomson.instrument_convolve(sp.power, lam, 0.1e-9))
        assert np.allclose(c.power.sum(axis=1), sp.power.sum(axis=1), rtol=1e-12)
        # no polarisation: the factor is 1; a scalar Z and an absent Ti and V go as the uniform value and NULL
        dom.Z, dom.Ti, dom.V = 3.0, None, None
        sp1 = dom.thomson_scattering(thomson.Probe(LAM_I, (0, 0, -3e-3), (0, 0, 1)), coll, lam, A_ION)
        F = {k: eng.Field(getattr(dom, k), dom.x, dom.y, dom.z) for k in ("ne", "Te")}
        try:
            P1, w1 = eng.thomson(F["ne"], F["Te"], None, 3.0, None, LAM_I, A_ION, pts, wts, probe.direction, ks, lam)
        finally:
            for f in F.values():
                f.close()
        assert np.array_equal(sp1.power, (thomson.R_E * thomson.R_E) * P1) and np.all(sp1.power[2] > 0)


@pytest.mark.gpu
def test_rotated_carries_Ti_and_V(eng):
    """rotated() carries Ti as it carries Te and V as it carries B: a domain whose Ti holds Te's values and whose V holds B's comes
    back with Ti == Te and V == B bit for bit at a generic angle (same kernel, same fill), its own fills are honoured, and a
    domain without them comes back without them."""
    p = _plasma("float64")
    for dom in _domains():
        dom.B = np.array(p["V"]) * 1e-5
        dom.V = np.array(dom.B)
        dom.Ti = np.array(dom.Te)
        rot = dom.rotated(33.0, about="y")
        assert rot.Ti.shape == rot.Te.shape and np.array_equal(rot.Ti, rot.Te)
        assert rot.V.shape == rot.B.shape and np.array_equal(rot.V, rot.B)
        assert not np.array_equal(rot.Te, dom.Te) and np.any(rot.Ti == 1.0) and np.any(np.all(rot.V == 0.0, axis=-1))
        # and against sr_field_resample's rule restated on the host: Ti'(q) = Ti(R q), V'(q) = R^T V(R q), the fills outside
        from synthpy_amd import orientation

        R = orientation.rotation_matrix(33.0, "y")
        src_axes = [np.float64(np.float32(a)) for a in (dom.x, dom.y, dom.z)]
        q = np.stack(np.meshgrid(*[np.float64(np.float32(a)) for a in (rot.x, rot.y, rot.z)], indexing="ij"), axis=-1).reshape(-1, 3)
        pos = np.stack([((R[a, 0] * q[:, 0] + R[a, 1] * q[:, 1]) + R[a, 2] * q[:, 2]) + 0.0 for a in range(3)], axis=1)
        Ti_h, inside = gather(np.asarray(dom.Ti, np.float64), src_axes, pos)
        Ti_ref = np.where(inside, Ti_h, 1.0)
        assert np.array_equal(rot.Ti.ravel() == 1.0, ~inside)
        assert np.all(np.abs(rot.Ti.ravel() - Ti_ref) <= 32 * U * np.max(np.abs(dom.Ti)))  # the blend's 7 roundings, both sides, x 2
        b = gather(np.asarray(dom.V, np.float64), src_axes, pos)[0]
        V_h = np.stack([(R.T[r, 0] * b[:, 0] + R.T[r, 1] * b[:, 1]) + R.T[r, 2] * b[:, 2] for r in range(3)], axis=1)
        V_ref = np.where(inside[:, None], V_h, 0.0)
        assert np.all(np.abs(rot.V.reshape(-1, 3) - V_ref) <= 3 * 32 * U * np.max(np.abs(dom.V)))  # three components mix
        print(f"rotated Ti, V equal to the host restatement bit for bit: {np.array_equal(rot.Ti.ravel(), Ti_ref)}, "
              f"{np.array_equal(rot.V.reshape(-1, 3), V_ref)}")
        assert 0.2 < inside.mean() < 0.95
        rot2 = dom.rotated(33.0, about="y", fill={"Ti": 7.0, "V": 2.0})
        assert np.array_equal(rot2.Te, rot.Te) and np.array_equal(rot2.B, rot.B)
        out = rot.Ti == 1.0  # the nodes outside the source box (Te >= 50 inside)
        assert np.all(rot2.Ti[out] == 7.0) and np.array_equal(rot2.Ti[~out], rot.Ti[~out])
        assert np.all(rot2.V[out] == 2.0) and np.array_equal(rot2.V[~out], rot.V[~out])
        dom.Ti = dom.V = None
        bare = dom.rotated(33.0, about="y")
        assert getattr(bare, "Ti", None) is None and getattr(bare, "V", None) is None
        assert np.array_equal(bare.Te, rot.Te) and np.array_equal(bare.B, rot.B)
        with pytest.raises(ValueError, match="fill names"):
            dom.rotated(33.0, fill={"Tion": 1.0})
