"""Thomson scattering from super-Gaussian (Langdon) electrons: sr_field_thomson_sg (thomson_sg.hip), engine.thomson_sg,
thomson.spectra_sg / langdon_order, ScalarDomain.external_order / thomson_scattering_sg of both API generations, and the order
carried by orientation.rotated.  Every test here fails on the commit before this entry existed (the library has no
sr_field_thomson_sg, _ffi no ThomsonSgParams, thomson no spectra_sg): the module-level lookups below already raise there.

THE REFERENCE for values is `restate_sg` below: include/synthray.h's rule in NumPy float64, operation for operation, built from
tests/test_thomson.py's and tests/test_thomson_multi.py's helpers.  The quadrature constants S2, V and the gamma function's
Chebyshev coefficients GC are read from thomson_sg.hip (kS2, kV, kGC) and checked here against numpy's Gauss-Legendre rule and
scipy's gamma.  The error measure of the kernel test is test_thomson_multi.py's with A_q extended by what the new terms enter:
    |P - P_ref| <= K u f_l sum_q |term_q| A_q,
    A_q = (1 + alpha^2 (c N_R + sum_j g_j Te/Ti))/|eps| + (m + 2) min(y, 745) + N_Q + 1          (a super-Gaussian point)
with y = |xs|^m, N_R the sum of the magnitudes of R's terms, each exp(-t^m) counted (1 + t^m) times (the roundings its argument
carries), N_Q = (GAM(2/m) + gamma(2/m, y))/Gamma(2/m, y) below the series' limit and 1 above it; a Maxwellian point keeps
test_thomson_multi.py's A_q.  u = 2^-53.
"""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_thomson import (AX, AX32, EPS0, KI90, KS90, LAM_I, LIGHT, ME, QE, SP, TSP, U, _dawson, _geometry, _plasma, built, eng, gather,
                          wavelength_stage)
from test_thomson_multi import A_SPECIES, _Fields, _all, point_stage_multi, restate_multi, sample_stage_multi

PI = 3.141592653589793
ORDER_EPS = 2.0 ** -30
IT_MAX = 100
M_LIST = (2.0, 2.05, 2.5, 3.3, 4.0, 5.0)
# test 1: the largest |R - R_ref| (1 + xs^2) against mpmath.quad at 34 digits, measured on the build machine (m = 2.05, xs = 1.61,
# 2e-6 beside a node); asserted: 8 x.  The issue's condition on the measured value itself: <= 1e-10.
R_MEASURED = 1.46e-11
# test 2: the largest relative error of the incomplete gamma function against scipy, measured on the build machine; asserted: 8 x.
# The issue's condition on the measured value itself: <= 1e-12.
Q_MEASURED = 1.09e-13
# test 5: the largest float64-against-longdouble ratio on test 6's inputs, measured on the build machine (test_sample_error_constant
# prints it: 6.20, one species with the charge a field; 3.4 to 5.9 elsewhere); the GPU bound is 8 x
K_MEASURED = 6.2
K_SAMPLE = 8 * K_MEASURED
# exp(-|xs|^m) underflows where |xs|^m passes 708 (gradually, to 745), which the +-70 nm wavelengths reach for the larger orders,
# and the ions' exp(-xi^2) with it: there a sample is an exact zero or a denormal number whose absolute error is the denormal
# spacing 5e-324, times wn f_l <= 1e45 in P.  Values below this floor count as zero in the decisions and in the bound.
UNDERFLOW = 1e-250


def _constants():
    text = open(os.path.join(ROOT, "synthpy_amd", "csrc", "thomson_sg.hip")).read()
    out = []
    for name, n in (("kS2", 48), ("kV", 48), ("kGC", 24)):
        body = re.search(r"const double " + name + r"\[(\d+)\] = \{([^}]*)\}", text)
        assert body and int(body.group(1)) == n, name
        vals = np.array([float(v) for v in body.group(2).replace("\n", " ").split(",")])
        assert len(vals) == n
        out.append(vals)
    return out


S2, V, GC = _constants()
NN = len(S2)


# ---------------------------------------------------------------- the restatement
def gam(z):
    """GAM(z) of the rule, 0.2 <= z <= 2.5, float64."""
    z = np.asarray(z, np.float64)
    w = np.where(z < 1.0, z + 1.0, np.where(z > 2.0, z - 1.0, z))
    tau = 2.0 * w - 3.0
    t2 = 2.0 * tau
    b1, b2 = np.zeros_like(w), np.zeros_like(w)
    for k in range(len(GC) - 1, 0, -1):
        b1, b2 = (GC[k] + t2 * b1) - b2, b1
    P = (GC[0] + tau * b1) - b2
    return np.where(z < 1.0, P / z, np.where(z > 2.0, (z - 1.0) * P, P))


def order_stage(m):
    """The `point` constants of the clamped order m (float64 array)."""
    m = np.asarray(m, np.float64)
    im = 1.0 / m
    z2 = 2.0 * im
    G1, G2, G3, G5 = gam(im), gam(z2), gam(3.0 * im), gam(5.0 * im)
    r = np.sqrt((2.0 * G5) / (3.0 * G3))
    b = m / (2.0 * G1)
    return dict(m=m, im=im, z2=z2, G2=G2, r=r, b=b, c=(G1 * G5) / ((3.0 * G3) * G3), fe=(SP * r) / (2.0 * G3), pib=PI * b)


def table(m, im, dtype=np.float64):
    """T (...), t_i and g_i (..., 48) of the points' m and 1/m, in dtype (the wide reference forms pow and exp there)."""
    m, im = np.asarray(m).astype(dtype), np.asarray(im).astype(dtype)
    T = np.power(dtype(40.0), im)
    t = T[..., None] * S2.astype(dtype)
    with np.errstate(under="ignore"):
        return T, t, np.exp(-np.power(t, m[..., None]))


def r_m(xs, m, b, T, t, g, dtype=np.float64):
    """The `R` lines: (R, gx, x, y, N_R).  Every argument broadcasts against xs; t and g carry a trailing axis of 48."""
    one, two, half = dtype(1.0), dtype(2.0), dtype(0.5)
    x = np.abs(xs)
    with np.errstate(all="ignore"):
        y = np.power(x, m)
        gx = np.exp(-y)
        x2 = x * x
        tx = two * x
        L = np.log((T - x) / (T + x))
        s, s_out = np.zeros_like(x), np.zeros_like(x)
        n_in, n_out = np.zeros_like(x), np.zeros_like(x)
        pm1 = m * np.power(x, m - one)
        g1 = -(pm1 * gx)
        g2 = gx * (pm1 * pm1 - (m * (m - one)) * np.power(x, m - two))
        wx_ = gx * (one + y)  # exp(-y) with the roundings of its argument
        for i in range(NN):
            ti, gi = t[..., i], g[..., i]
            tt = ti * ti
            e = ti - x
            dg = gi - gx
            near = np.abs(e) < dtype(1e-6)
            coll = (g1 + (half * g2) * e) - dg / (ti + x)
            normal = (dg * tx) / (tt - x2)
            s = s + dtype(V[i]) * np.where(near, coll, normal)
            s_out = s_out + dtype(V[i]) * ((gi * (two * tt)) / (tt - x2))
            wi_ = gi * (one + np.power(ti, m))
            n_in = n_in + dtype(V[i]) * np.where(near, np.abs(g1) + np.abs(g2 * e) + (wi_ + wx_) / (ti + x), (wi_ + wx_) * np.abs(tx / (tt - x2)))
            n_out = n_out + dtype(V[i]) * np.abs((wi_ * (two * tt)) / (tt - x2))
        R_in = one + (x * b) * (T * s + gx * L)
        R_out = (b * T) * s_out
        N_in = one + (x * b) * (T * n_in + wx_ * np.abs(L))
        N_out = (b * T) * n_out
    inner = x < T
    return np.where(inner, R_in, R_out), gx, x, y, np.where(inner, N_in, N_out)


def upper_gamma(y, xg, z2, G2, dtype=np.float64):
    """The `Q` lines: Gamma(z2, y) with y^z2 exp(-y) given as xg.  (Q, trip counts, N_Q)."""
    one, two = dtype(1.0), dtype(2.0)
    eps, tiny = dtype(1e-16), dtype(1e-300)
    y, xg, z2, G2 = (np.array(a, dtype) for a in np.broadcast_arrays(y, xg, z2, G2))
    low = y < z2 + one
    with np.errstate(all="ignore"):
        ap, de = z2.copy(), one / z2
        sm = de.copy()
        act = low.copy()
        its = np.zeros(y.shape, int)
        for _ in range(IT_MAX):
            if not act.any():
                break
            ap = np.where(act, ap + one, ap)
            de = np.where(act, de * (y / ap), de)
            sm = np.where(act, sm + de, sm)
            its = its + act
            act = act & ~(np.abs(de) < np.abs(sm) * eps)
        Q_lo = G2 - sm * xg
        bb = (y + one) - z2
        cc = (one / tiny) * np.ones_like(bb)
        d = one / bb
        h = d.copy()
        act = ~low & np.isfinite(y)
        for i in range(1, IT_MAX + 1):
            if not act.any():
                break
            an = -dtype(i) * (dtype(i) - z2)
            bb = np.where(act, bb + two, bb)
            dn = an * d + bb
            dn = np.where(np.abs(dn) < tiny, tiny, dn)
            cn = bb + an / cc
            cn = np.where(np.abs(cn) < tiny, tiny, cn)
            dn = one / dn
            de = dn * cn
            d, cc = np.where(act, dn, d), np.where(act, cn, cc)
            h = np.where(act, h * de, h)
            its = its + act
            act = act & ~(np.abs(de - one) < eps)
        Q_hi = xg * h
        N_Q = np.where(low, (G2 + sm * xg) / Q_lo, one)
    return np.where(low, Q_lo, Q_hi), its, N_Q


def point_stage_sg(ne, Te, Ti, Zs, fs, As, vs, vi, ds, di, wq, mo):
    """The `point` lines: test_thomson_multi.py's dict and, per point, sg (the super-Gaussian lines are taken) and order_stage."""
    Q = point_stage_multi(ne, Te, Ti, Zs, fs, As, vs, vi, ds, di, wq)
    mo = mo * np.ones_like(ne)
    Q["keep"] = Q["keep"] & ~np.isnan(mo)
    with np.errstate(invalid="ignore"):
        m = np.minimum(np.maximum(mo, 2.0), 5.0)
        sg = Q["keep"] & (m - 2.0 > ORDER_EPS)
    Q.update(order_stage(np.where(sg, m, 3.0)))  # a point that does not take them gets numbers that are not read
    Q["sg"] = sg
    return Q


def sample_stage_sg(L, Q, has_v=True, has_vd=True, dtype=np.float64):
    """The `sample` lines for every (point, wavelength): (n_q, n_lambda) arrays in dtype.  The point stage stays float64; the
    wide reference forms the tables g_i, pow, exp and log in dtype."""
    wide = dtype is not np.float64
    one, two = dtype(1.0), dtype(2.0)
    sp = np.sqrt(dtype(4.0) * np.arctan(one)) if wide else SP
    tsp = two * sp if wide else TSP
    ns = sum(1 for k in Q if re.fullmatch(r"g\d", k))
    q = {k: v.astype(dtype)[:, None] for k, v in Q.items() if k not in ("keep", "sg")}
    l = {k: np.asarray(v, np.float64).astype(dtype)[None, :] for k, v in L.items() if k != "wi" and k != "kin"}
    kin = dtype(L["kin"])
    sg = Q["sg"][:, None]
    with np.errstate(all="ignore"):
        wp = l["w"] - (l["ksc"] * q["vs"] - kin * q["vi"]) if has_v else l["w"] + dtype(0.0) * q["vs"]
        a = wp * l["rk"]
        ae = (wp - (l["ksc"] * q["ds"] - kin * q["di"])) * l["rk"] if has_vd else a
        xe = ae * q["ivte"]
        al = q["pe"] * l["rk2"]
        Fe, Em = _dawson(xe, dtype)
        cer_m, cei_m = al * (one - (two * xe) * Fe), al * ((sp * xe) * Em)
        T, t, g = table(Q["m"], Q["im"], dtype)
        xs = xe * q["r"]
        R, gx, x, y, N_R = r_m(xs, q["m"], q["b"], T[:, None], t[:, None, :], g[:, None, :], dtype)
        ac = al * q["c"]
        cer_s, cei_s = ac * R, ac * ((q["pib"] * xs) * gx)
        Qg, its, N_Q = upper_gamma(y, (x * x) * gx, q["z2"] * np.ones_like(y), q["G2"] * np.ones_like(y), dtype)
        Es = q["fe"] * Qg
        cer, cei, Ee = np.where(sg, cer_s, cer_m), np.where(sg, cei_s, cei_m), np.where(sg, Es, Em)
        er, ei, sr, si = one + cer, cei, one, dtype(0.0)
        Ei, saz = [], dtype(0.0)
        for j in range(ns):  # ascending
            xi = a * q[f"ivti{j}"]
            az = al * q[f"zt{j}"]
            Fi, E = _dawson(xi, dtype)
            Ei.append(E)
            cir, cii = az * (one - (two * xi) * Fi), az * ((sp * xi) * E)
            er, ei, sr, si = er + cir, ei + cii, sr + cir, si + cii
            saz = saz + np.abs(az)
        ie2 = one / (er * er + ei * ei)
        n1 = sr * sr + si * si
        n2 = cer * cer + cei * cei
        tt = n2 * ie2
        ion = dtype(0.0)
        for j in range(ns):
            ion = ion + ((q[f"g{j}"] * tt) * Ei[j]) * q[f"ivti{j}"]
        S = (tsp * l["rk"]) * (((n1 * ie2) * Ee) * q["ivte"] + ion)
        mod_eps = np.sqrt(er * er + ei * ei)
        A_m = (1 + al + saz) / mod_eps + np.minimum(xe * xe, 745.0) + 1
        A_s = (1 + ac * N_R + saz) / mod_eps + (q["m"] + two) * np.minimum(y, 745.0) + N_Q + 1
    return dict(S=S, A=np.where(sg, A_s, A_m), xs=np.where(sg, xs, np.nan), cer=cer, cei=cei, Ee=Ee, its=np.where(sg, its, 0),
                T=np.where(Q["sg"], T.astype(np.float64), np.nan), t=t, R=R)


def restate_sg(fields, species, order, axes, pts, wts, ki, ks, lam, lam_i, dtype=np.float64, nqs=None):
    """The whole rule.  fields: dict with ne, Te and optionally Ti, V, Vd arrays; species: (A, Z, f) with Z and f a 3-D array or a
    number; order: a 3-D array or a number.  {nq: (P (M, n_lambda), weight (M), keep (M, nq), scale (M, n_lambda))} for the first
    nq points of every volume, nq in nqs (default: all)."""
    M, nq_all = wts.shape
    nqs = (nq_all,) if nqs is None else tuple(nqs)
    out = {n: [] for n in nqs}
    for m in range(M):
        p = pts[m]
        ne, inside = gather(fields["ne"], axes, p)
        Te = gather(fields["Te"], axes, p)[0]
        Ti = gather(fields["Ti"], axes, p)[0] if fields.get("Ti") is not None else Te
        proj = []
        for name in ("V", "Vd"):
            if fields.get(name) is not None:
                v = gather(fields[name], axes, p)[0]
                with np.errstate(invalid="ignore"):
                    proj += [(v[:, 0] * ks[m, 0] + v[:, 1] * ks[m, 1]) + v[:, 2] * ks[m, 2],
                             (v[:, 0] * ki[m, 0] + v[:, 1] * ki[m, 1]) + v[:, 2] * ki[m, 2]]
            else:
                proj += [np.zeros(nq_all), np.zeros(nq_all)]
        val = lambda a: gather(a, axes, p)[0] if np.ndim(a) == 3 else np.full(nq_all, float(a))
        Zs, fs, As = [val(Z) for _, Z, _ in species], [val(f) for _, _, f in species], [A for A, _, _ in species]
        ne = np.where(inside, ne, 0.0)  # outside: dropped, as ne <= 0 is
        cth = (ki[m, 0] * ks[m, 0] + ki[m, 1] * ks[m, 1]) + ki[m, 2] * ks[m, 2]
        L = wavelength_stage(np.asarray(lam, np.float64), lam_i, cth)
        Q = point_stage_sg(ne, Te, Ti, Zs, fs, As, *proj, np.asarray(wts[m], np.float64), val(order))
        kept = np.nonzero(Q["keep"])[0]  # the sample lines of the kept points only (a dropped point adds nothing)
        s = sample_stage_sg(L, {k: v[kept] for k, v in Q.items()}, fields.get("V") is not None, fields.get("Vd") is not None, dtype)
        row = {int(j): i for i, j in enumerate(kept)}
        acc, wsum, scale = np.zeros(len(L["w"]), dtype), 0.0, np.zeros(len(L["w"]), dtype)
        for j in range(nq_all):  # ascending
            if Q["keep"][j]:
                term = dtype(Q["wn"][j]) * s["S"][row[j]]
                acc = acc + term
                wsum = wsum + Q["wn"][j]
                scale = scale + np.abs(term) * s["A"][row[j]]
            if j + 1 in out:
                out[j + 1].append((acc * L["f"].astype(dtype), wsum, Q["keep"][:j + 1].copy(), scale * np.abs(L["f"]).astype(dtype)))
        for n in nqs:
            if n == 0:
                out[n].append((acc * 0, 0.0, Q["keep"][:0], scale * 0))
    return {n: tuple(np.array([o[k] for o in rows]) for k in range(4)) for n, rows in out.items()}


def _one_point(ne, Te, Ti, species, order, lam, V=None, Vd=None, dtype=np.float64):
    """sample_stage_sg at one point of uniform numbers at 90 degrees: the dict of (n_lambda) arrays."""
    proj = [float(v @ d) if v is not None else 0.0 for v in (V, Vd) for d in (KS90, KI90)]
    one = lambda v: np.array([float(v)])
    Q = point_stage_sg(one(ne), one(Te), one(Ti), [one(Z) for _, Z, _ in species], [one(f) for _, _, f in species],
                       [A for A, _, _ in species], *(one(v) for v in proj), one(1.0), one(order))
    assert Q["keep"][0]
    s = sample_stage_sg(wavelength_stage(lam, LAM_I, 0.0), Q, V is not None, Vd is not None, dtype)
    return {k: v[0] for k, v in s.items()}, Q


def _R(m, xs):
    """R_m and the electron factor's Q at the numbers xs for one order m: (R, Q, x, y, gx, consts)."""
    o = order_stage(np.array([float(m)]))
    T, t, g = table(o["m"], o["im"])
    xs = np.asarray(xs, np.float64)
    R, gx, x, y, _ = r_m(xs, o["m"][0], o["b"][0], T[0], t, g)
    Q, its, _ = upper_gamma(y, (x * x) * gx, o["z2"][0] * np.ones_like(y), o["G2"][0] * np.ones_like(y))
    return R, Q, x, y, gx, {k: float(v[0]) for k, v in o.items()}, float(T[0]), t[0], its


# ================================================================ tests without a device
def test_constants_are_the_rule_s():
    """kS2, kV of thomson_sg.hip are s_i^2 and 2 w_i s_i of numpy's 48-point Gauss-Legendre rule on [0, 1] (to 1e-14: numpy's own nodes and weights are Newton-
    polished float64 and differ from the 40-digit ones the constants were rounded from by up to 3.3e-15),
    and GAM agrees with scipy's gamma on [0.2, 2.5] to 8 u: measured 5.7e-16 relative."""
    from scipy.special import gamma

    x, w = np.polynomial.legendre.leggauss(48)
    s, ws = (x + 1) / 2, w / 2
    assert NN == 48 and np.all(np.diff(S2) > 0)
    assert np.max(np.abs(S2 - s * s)) <= 1e-14 and np.max(np.abs(V - 2 * ws * s)) <= 1e-14
    z = np.linspace(0.2, 2.5, 2301)
    err = float(np.max(np.abs(gam(z) - gamma(z)) / gamma(z)))
    print(f"GAM against scipy.special.gamma on [0.2, 2.5]: {err:.2e} relative")
    assert err <= 8 * 5.7e-16


def _r_ref(m, xi):
    import mpmath as mp

    mp.mp.dps = 34
    mm, xi = mp.mpf(m), mp.mpf(float(xi))
    if xi == 0:
        return mp.mpf(1)
    b = mm / (2 * mp.gamma(1 / mm))
    g = lambda t: mp.e ** (-abs(t) ** mm)
    Tc = mp.mpf(100) ** (1 / mm)  # exp(-100): nothing at 34 digits scaled by (1 + xi^2) <= 2501
    # P int t g/(t - xi) dt = int g + xi int_0^inf (g(xi + s) - g(xi - s))/s ds; the integrand lives where |xi +- s| < Tc
    f = lambda s_: (g(xi + s_) - g(xi - s_)) / s_
    lo = max(mp.mpf(0), xi - Tc)
    grid = sorted({lo, xi + Tc, *[lo + mp.mpf(k) / 2 for k in range(int(2 * (xi + Tc - lo)) + 1)]} | ({xi} if xi > lo else set()))
    return 1 + xi * b * mp.quad(f, grid)


def _xi_list(m):
    """The issue's xs list for one m: 0 to 50, on a node, 1e-12, 1e-9, 3e-7 and 2e-6 beside one, T -+ 1e-3, T itself, and the first
    and last node (the first lies within 1e-6 of 0)."""
    *_, T, t, _ = _R(m, [0.0])
    return [0.0, 1e-3, 0.3, 0.9, 1.0, 1.59, 1.61, 1.7, 2.5, T - 1e-3, T, T + 1e-3, T + 0.3, 9.0, 50.0, t[NN // 3], t[NN // 3] + 1e-9,
            t[NN // 2] - 3e-7, t[NN // 2] + 2e-6, t[5] + 1e-12, t[0], t[NN - 1] - 1e-9]


def test_R_against_mpmath():
    """The restated R_m against mpmath.quad at 34 digits for m in {2, 2.05, 2.5, 3.3, 4, 5} and xs from 0 to 50 with xs on a node,
    1e-12, 1e-9, 3e-7 and 2e-6 beside one, at T and T -+ 1e-3.  Measure: |R - R_ref| (1 + xs^2).  Measured on the build machine:
    1.46e-11 (m = 2.05, xs = 1.611 = a node + 2e-6; 3.9e-13 at m = 2).  Asserted: 8 x that; the measured value itself meets the
    issue's condition <= 1e-10."""
    import mpmath as mp

    assert R_MEASURED <= 1e-10
    worst, where = 0.0, None
    for m in M_LIST:
        xs = _xi_list(m)
        R = _R(m, xs)[0]
        for xi, Rv in zip(xs, R):
            e = float(abs(mp.mpf(float(Rv)) - _r_ref(m, xi)) * (1 + xi * xi))
            if e > worst:
                worst, where = e, (m, xi)
    print(f"max |R - R_ref| (1 + xs^2) = {worst:.3e} at m, xs = {where}")
    assert worst <= 8 * R_MEASURED


def test_incomplete_gamma_against_scipy():
    """The restated Gamma(2/m, y) against scipy.special.gammaincc * gamma, relative, for 61 orders in [2, 5] and y = x^m, x from 0
    to 6 (4003 values, both sides of the series' limit y = 2/m + 1), wherever the reference exceeds 1e-300.  Measured on the build
    machine: 1.09e-13 at most, 85 terms at most.  Asserted: 8 x; the measured value meets the issue's condition <= 1e-12."""
    from scipy.special import gamma, gammaincc

    assert Q_MEASURED <= 1e-12
    worst, most = 0.0, 0
    for m in np.linspace(2, 5, 61):
        x = np.concatenate([np.linspace(0, 6, 4001), [1e-9, 1e-3]])
        _, Q, _, y, _, o, _, _, its = _R(m, x)
        ref = gammaincc(2 / m, y) * gamma(2 / m)
        ok = ref > 1e-300
        worst, most = max(worst, float(np.max(np.abs(Q - ref)[ok] / ref[ok]))), max(most, int(its.max()))
    print(f"incomplete gamma: {worst:.3e} relative at most, {most} terms at most")
    assert worst <= 8 * Q_MEASURED and most < IT_MAX


CH = [(12.0, 6.0, 0.5), (1.0, 1.0, 0.5)]


def test_limits_and_identities():
    """3a: m = 2 through the rule (the threshold taken) reproduces test_thomson_multi.py's sample bit for bit, and forced through the
    super-Gaussian lines (the threshold bypassed) its electron numbers to rounding: R against 1 - 2 x F(x) within test 1's bound,
    fe Gamma(1, x^2) against exp(-x^2) and the imaginary part within 64 u.  3b: R_m(0) = 1 exactly, so chi_e(0) =
    al c.  3c: c = 1, r = 1, b = 1/sqrt(pi), fe Gamma(1, 0) = 1 at m = 2 to 4 u.  3d: int f1 du = 1 by quadrature of the electron
    factor, to 1e-10.  3e: R even and cei odd in xs, bit for bit.  (3f is test_langdon_order.)"""
    lam = np.linspace(LAM_I - 60e-9, LAM_I + 60e-9, 2049)
    # 3a through the rule: identical bits
    s2, Q = _one_point(1e25, 300.0, 100.0, CH, 2.0, lam, 3e4 * KS90, 4e5 * KS90)
    assert not Q["sg"][0]
    Qm = point_stage_multi(*(np.array([v]) for v in (1e25, 300.0, 100.0)), [np.array([6.0]), np.array([1.0])], [np.array([0.5])] * 2,
                           [12.0, 1.0], *(np.array([float(v @ d)]) for v in (3e4 * KS90, 4e5 * KS90) for d in (KS90, KI90)), np.array([1.0]))
    Sm = sample_stage_multi(wavelength_stage(lam, LAM_I, 0.0), Qm)["S"][0]
    assert s2["S"].tobytes() == Sm.tobytes()
    # 3a forced through the super-Gaussian lines: the electron numbers agree to rounding with the Maxwellian ones
    xs = np.linspace(-7.5, 7.5, 3001)
    R, Qg, x, y, gx, o, T, t, _ = _R(2.0, xs)
    F, E = _dawson(xs, np.float64)
    assert np.max(np.abs(R - (1.0 - (2.0 * xs) * F)) * (1 + xs * xs)) <= 8 * R_MEASURED
    assert np.max(np.abs(o["fe"] * Qg - E)) <= 64 * U and np.max(np.abs((o["pib"] * xs) * gx - (SP * xs) * E)) <= 64 * U
    # 3c
    assert abs(o["c"] - 1) <= 4 * U and abs(o["r"] - 1) <= 4 * U and abs(o["b"] * np.sqrt(np.pi) - 1) <= 4 * U and abs(o["fe"] - 1) <= 4 * U
    for m in M_LIST[1:]:
        s, Q = _one_point(1e25, 300.0, 100.0, CH, m, np.array([LAM_I]))
        # 3b: at the probe's own wavelength without flow xs = 0: R = 1 exactly
        assert Q["sg"][0] and s["R"][0] == 1.0 and s["cer"][0] == (Q["pe"][0] * wavelength_stage(np.array([LAM_I]), LAM_I, 0.0)["rk2"][0]) * Q["c"][0]
        assert s["cei"][0] == 0.0
        # 3e
        xs = np.concatenate([np.linspace(0, 8, 801), _xi_list(m)])
        Rp, Qp, _, _, gp, o, *_ = _R(m, xs)
        Rn, Qn, _, _, gn, *_ = _R(m, -xs)
        assert Rp.tobytes() == Rn.tobytes() and Qp.tobytes() == Qn.tobytes()
        assert ((o["pib"] * xs) * gp).tobytes() == (-((o["pib"] * -xs) * gn)).tobytes()
        # 3d: f1(u) du with u = v_m xs: int fe Q r / sqrt(pi) dxe = 1, xe = xs / r
        xg, wg = np.polynomial.legendre.leggauss(400)
        Tm = 40.0 ** (1 / m) * 1.3
        u = 0.5 * Tm * (xg + 1)
        Qu = _R(m, u)[1]
        total = 2 * np.sum(0.5 * Tm * wg * o["fe"] * Qu) / (np.sqrt(np.pi) * o["r"])
        assert abs(total - 1) <= 1e-10, (m, total)


def test_langdon_order(built):
    """3f: langdon_order gives 2 at alpha = 0 and 5 as alpha -> infinity, is monotone in the intensity, and takes numbers or arrays."""
    from synthpy_amd import thomson

    assert thomson.langdon_order(10.0, 0.0, 100.0, 351e-9) == 2.0
    assert thomson.langdon_order(0.0, 1e19, 100.0, 351e-9) == 2.0
    assert abs(thomson.langdon_order(10.0, 1e40, 100.0, 351e-9) - 5.0) <= 1e-9
    I = np.logspace(14, 24, 101)
    m = thomson.langdon_order(10.0, I, 500.0, 351e-9)
    assert m.shape == (101,) and np.all(np.diff(m) > 0) and np.all((m > 2) & (m < 5))
    # alpha by hand at one point: Z v_osc^2 / v_t^2
    E2 = 2 * 1e19 / (EPS0 * LIGHT)
    alpha = 10.0 * E2 * (QE / (ME * 2 * np.pi * LIGHT / 351e-9)) ** 2 / (QE * 500.0 / ME)
    assert np.isclose(thomson.langdon_order(10.0, 1e19, 500.0, 351e-9), 2 + 3 / (1 + 1.66 / alpha ** 0.724), rtol=1e-12)
    grid = thomson.langdon_order(np.full((3, 4, 5), 6.0), 1e19, np.full((3, 4, 5), 300.0), 351e-9)
    assert grid.shape == (3, 4, 5) and np.all(grid == grid[0, 0, 0])


def test_restated_physics():
    """The signs test 8 asserts on the device, on the restatement: at m = 4 against m = 2 the electron-plasma-wave peak is higher
    and narrower, and the ion-acoustic peaks are narrower (less electron Landau damping)."""
    out = {}
    for m in (2.0, 4.0):
        out[m] = _physics_numbers(lambda lam, m=m: _one_point(*PHYS_PLASMA, m, lam)[0]["S"])
    print("restatement, m = 2 / 4: " + ", ".join(f"{k} {out[2.0][k]:.4g} / {out[4.0][k]:.4g}" for k in out[2.0]))
    _assert_physics(out[2.0], out[4.0])


# ne, Te, Ti, species: carbon, alpha about 3.3 at 90 degrees and 532 nm -- the wave's phase velocity lies in the tail, which a
# super-Gaussian depletes (with light ions or alpha near 2 the orderings are not these)
PHYS_PLASMA = (2e25, 200.0, 50.0, [(12.0, 6.0, 1.0)])
PHYS_EPW = np.linspace(LAM_I + 40e-9, LAM_I + 65e-9, 2001)      # the red electron-plasma-wave peak
PHYS_IAW = np.linspace(LAM_I + 0.15e-9, LAM_I + 0.40e-9, 2001)  # the red ion-acoustic peak


def _fwhm(lam, s):
    k = int(np.argmax(s))
    assert 0 < k < len(s) - 1, "the peak must lie inside the window"
    above = np.nonzero(s >= 0.5 * s[k])[0]
    assert above[0] > 0 and above[-1] < len(s) - 1, "the half-maximum points must lie inside the window"
    return lam[above[-1]] - lam[above[0]]


def _physics_numbers(spectrum):
    e, i = spectrum(PHYS_EPW), spectrum(PHYS_IAW)
    return dict(epw_peak=float(e.max()), epw_width=float(_fwhm(PHYS_EPW, e)), iaw_width=float(_fwhm(PHYS_IAW, i)))


def _assert_physics(maxwell, sg):
    assert sg["epw_peak"] > maxwell["epw_peak"] and sg["epw_width"] < maxwell["epw_width"] and sg["iaw_width"] < maxwell["iaw_width"]


def test_header_ctypes_and_python_signatures(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "synthray.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sr_field_thomson_sg\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 20
    p = re.search(r"typedef struct \{([^}]*)\}\s*sr_thomson_sg_params;", text).group(1)
    assert re.findall(r"(\w+)(?:\[SR_MAX_SPECIES\])?;", p) == [n for n, _ in built.ThomsonSgParams._fields_] == \
        ["lambda_i", "n_species", "reserved", "A", "Z", "frac", "order"]
    assert C.sizeof(built.ThomsonSgParams) == 120 and built.ThomsonSgParams.order.offset == 112
    res, args = built.SYMBOLS["sr_field_thomson_sg"]
    assert res is C.c_int and len(args) == 20 and args[9] is C.c_int64 and args[10] is C.c_int32 and args[15] is C.c_int32
    assert hasattr(built.lib, "sr_field_thomson_sg")
    mk = open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()
    assert "thomson_sg.hip" in mk and "thomson_multi.hip" in mk and "-ffp-contract=off" in mk
    header = open(os.path.join(ROOT, "include", "synthray.h")).read()
    for word in ("kS2", "kV", "kGC", "pow(40.0, im)", "2^-30"):
        assert word in header, word

    from synthpy_amd import engine, thomson
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.thomson_sg) == ["ne", "Te", "Ti", "V", "Vd", "species", "order", "lambda_i", "points", "weights", "ki", "ks", "wavelengths"]
    assert names(thomson.spectra_sg) == ["domain", "probe", "collection", "wavelengths", "species", "order", "instrument_fwhm", "fields"]
    assert inspect.signature(thomson.spectra_sg).parameters["order"].default is None
    assert names(thomson.langdon_order) == ["Z", "intensity", "Te", "wavelength"]
    for name in ("thomson_scattering_sg", "external_order"):
        assert names(getattr(NewDomain, name)) == names(getattr(OldDomain, name)), name
    assert names(NewDomain.external_order) == ["self", "m"]
    assert names(NewDomain.thomson_scattering_sg) == ["self", "probe", "collection", "wavelengths", "species", "order", "kw"]
    # the entries before this one keep their signatures
    assert names(engine.thomson_multi) == ["ne", "Te", "Ti", "V", "Vd", "species", "lambda_i", "points", "weights", "ki", "ks", "wavelengths"]
    assert names(thomson.spectra_multi) == ["domain", "probe", "collection", "wavelengths", "species", "instrument_fwhm", "fields"]


def test_argument_checks_come_before_the_device(built):
    """Test 4.  A uniform order outside [2, 5] or NaN is SR_ERR_INVALID with its own text on a machine with or without a GPU, as is
    everything sr_field_thomson_multi rejects; an order in range gets as far as the NULL fields.  An sr_field exists only on a
    device (sr_field_create uploads it), so the order FIELD's cases -- n_comp, dtype, grid -- are in
    test_field_checks_need_live_fields, marked gpu."""
    from synthpy_amd import engine

    lib, ptr = built.lib, built.ptr
    base = dict(lambda_i=LAM_I, n_species=2, A=(12.0, 1.0), Z=(6.0, 1.0), frac=(0.5, 0.5), order=3.0, n_vol=2, n_quad=3, n_lambda=4,
                pts=np.zeros((2, 3, 3)), wts=np.ones((2, 3)), ki=np.tile(KI90, (2, 1)), ks=np.tile(KS90, (2, 1)),
                lam=np.linspace(531e-9, 533e-9, 4), P=np.zeros((2, 4)), weight=np.zeros(2), p=True)

    def call(**kw):
        a = {**base, **kw}
        p = built.ThomsonSgParams()
        p.lambda_i, p.n_species, p.order = a["lambda_i"], a["n_species"], a["order"]
        for j in range(len(a["A"])):
            p.A[j], p.Z[j], p.frac[j] = a["A"][j], a["Z"][j], a["frac"][j]
        arr = lambda k: None if a[k] is None else ptr(np.ascontiguousarray(a[k], dtype=np.float64))
        rc = lib.sr_field_thomson_sg(None, None, None, None, None, None, None, None, C.byref(p) if a["p"] else None, a["n_vol"],
                                     a["n_quad"], arr("pts"), arr("wts"), arr("ki"), arr("ks"), a["n_lambda"], arr("lam"), arr("P"),
                                     arr("weight"), None)
        return rc, built.last_error()

    for bad in (1.999, 5.001, 0.0, -3.0, np.inf, -np.inf, np.nan):
        rc, err = call(order=bad)
        assert rc == -1 and "the uniform order must lie in [2, 5]" in err and "sr_field_thomson_sg" in err, (bad, err)
    for good in (2.0, 2.0 + 2.0 ** -40, 3.3, 5.0):
        rc, err = call(order=good)
        assert rc == -1 and "NULL field" in err, (good, err)
    for name in ("p", "pts", "wts", "ki", "ks", "lam", "P", "weight"):
        rc, err = call(**{name: None})
        assert rc == -1 and "NULL argument" in err, (name, err)
    for name in ("n_vol", "n_quad", "n_lambda"):
        rc, err = call(**{name: -1})
        assert rc == -1 and "must not be negative" in err, (name, err)
    for kw, text in ((dict(lambda_i=np.nan), "lambda_i"), (dict(n_species=5), "n_species must be 1..4, got 5"), (dict(A=(12.0, 0.0)), "A[1]"),
                     (dict(Z=(-1.0, 1.0)), "uniform Z[0]"), (dict(frac=(0.5, np.nan)), "uniform frac[1]"),
                     (dict(ks=np.tile(KI90, (2, 1))), "ki equals ks in volume 0")):
        rc, err = call(**kw)
        assert rc == -1 and text in err, (kw, err)
    lam = base["lam"].copy()
    lam[2] = -1.0
    rc, err = call(lam=lam)
    assert rc == -1 and "lambda[2]" in err, err
    assert call(n_vol=0)[0] == -1 and call(n_lambda=0)[0] == -1  # not before the fields were looked at
    z = np.zeros((2, 2, 2))
    with pytest.raises(ValueError, match="ne must be an open engine.Field"):
        engine.thomson_sg(z, z, None, None, None, [(12.0, 6.0, 1.0)], 3.0, LAM_I, base["pts"], base["wts"], KI90, KS90, base["lam"])


def test_python_argument_checks(built):
    from synthpy_amd import thomson
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    pr = thomson.Probe(LAM_I, (0, 0, 0), (0, 0, 1))
    coll = thomson.Collection(np.zeros((4, 3)), (0, 1, 0), length=1e-4, n_quad=2)
    lam = np.linspace(531e-9, 533e-9, 8)
    ch = [thomson.Species(12, 6, 0.5), thomson.Species(1, 1, 0.5)]
    new = NewDomain(4e-3, 5)
    old = OldDomain(np.linspace(-2e-3, 2e-3, 5), np.linspace(-2e-3, 2e-3, 5), np.linspace(-2e-3, 2e-3, 5), 2e-3)
    for dom in (new, old):
        assert getattr(dom, "order", None) is None
        dom.external_ne(np.full((5, 5, 5), 1e24))
        with pytest.raises(ValueError, match="external_Te"):
            dom.thomson_scattering_sg(pr, coll, lam, ch, order=3.0)
        dom.external_Te(np.full((5, 5, 5), 100.0))
        with pytest.raises(ValueError, match="holds no order"):
            dom.thomson_scattering_sg(pr, coll, lam, ch)
        for bad in (1.9, 5.1, np.nan, np.inf):
            with pytest.raises(ValueError, match=r"a uniform order must lie in \[2, 5\]"):
                dom.thomson_scattering_sg(pr, coll, lam, ch, order=bad)
        with pytest.raises(ValueError, match=r"order has shape \(5, 5, 4\)"):
            dom.thomson_scattering_sg(pr, coll, lam, ch, order=np.full((5, 5, 4), 3.0))
        with pytest.raises(ValueError, match="species must be 1 to 4"):
            dom.thomson_scattering_sg(pr, coll, lam, [], order=3.0)
        m = np.full((5, 5, 5), 3.0)
        dom.external_order(m)
        assert dom.order is m  # kept as given, as V is
        with pytest.raises(ValueError, match=r"order has shape"):
            dom.thomson_scattering_sg(pr, coll, lam, ch, order=np.full((4, 5, 5), 3.0))


# ---------------------------------------------------------------- inputs of the GPU tests
NQ_SG, NL_SG = (1, 64, 65, 130), (1, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def _order_field(dtype_name):
    """The order on test_thomson.py's grid: 2 + 3 x random, with a block of exact 2.0 nodes (its inner cells give m = 2 among
    super-Gaussian neighbours), a block of 1.5 (clamped to 2), a block of 6.5 (clamped to 5), one infinite node and one NaN node."""
    rng = np.random.default_rng(31)
    shape = tuple(len(a) for a in AX)
    m = 2.0 + 3.0 * rng.random(shape)
    m[0:3, 4:8, 0:4] = 2.0
    m[5:8, 0:3, 3:6] = 1.5
    m[3:6, 5:8, 4:7] = 6.5
    m[8, 7, 0] = np.inf
    m[6, 4, 2] = np.nan
    m = m.astype(np.dtype(dtype_name))
    m.setflags(write=False)
    return m


def _first_point(config):
    """The gathered numbers of volume 0's point 2 (a generic interior point) for `config`: what the special wavelengths are made for."""
    pts, wts, ki, ks, lam = _geometry_sg()
    dtype_name, given, spec, order = CONFIGS[config]
    f = _all(dtype_name)
    p = pts[0, 2:3]
    Te = gather(f["Te"], AX, p)[0][0]
    m = float(np.clip(gather(_order_field(dtype_name), AX, p)[0][0], 2, 5)) if order == "field" else float(order)
    return Te, m


def _special_wavelengths():
    """Wavelengths at which xs of volume 0's point 2 in the configuration SPECIAL (no flow, no drift, so xs = xe r depends on the
    wavelength alone) falls on quadrature nodes (nearest float64 wavelength: |xs - t_i| of a few 1e-15, and exactly on it where
    the search finds such a wavelength), 1e-9, 3e-7 and 2e-6 beside a node, and at T -+ 1e-3: (wavelengths, the targets)."""
    Te, m = _first_point(SPECIAL)
    o = order_stage(np.array([m]))
    T, t, _ = table(o["m"], o["im"])
    ivte = 1.0 / np.sqrt(((2.0 * QE) / ME) * Te)
    ks = _geometry()[3]
    cth = float(ks[0, 2])

    def xs_of(lam):
        L = wavelength_stage(np.asarray(lam, np.float64), LAM_I, cth)
        return ((L["w"] * L["rk"]) * ivte) * o["r"][0]

    targets = [t[0][i] for i in (8, 12, 16, 20, 24)] + [t[0][14] + 1e-9, t[0][18] - 3e-7, t[0][22] + 2e-6, T[0] - 1e-3, T[0] + 1e-3]
    out = []
    for target in targets:
        lo, hi = LAM_I - 100e-9, LAM_I  # xs falls with the wavelength; the blue side
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if xs_of(mid) > target:
                lo = mid
            else:
                hi = mid
        near = lo + np.arange(-8, 9) * np.spacing(lo)
        out.append(near[np.argmin(np.abs(xs_of(near) - target))])
    return np.array(out), np.array(targets)


@functools.lru_cache(maxsize=None)
def _geometry_sg():
    """test_thomson.py's 5 volumes with 130 points each (its 65 and 65 more inside the box) and 513 wavelengths: its 257, the
    special ones in places 1.., and the electron feature out to +-70 nm, where |xs| passes T for the larger orders."""
    pts0, wts0, ki, ks, lam0 = _geometry()
    rng = np.random.default_rng(41)
    lo, hi = np.array([a[0] for a in AX]), np.array([a[-1] for a in AX])
    more = lo + rng.random((5, 65, 3)) * (hi - lo)
    more[4] = hi + 1e-4  # volume 4 stays outside
    pts = np.concatenate([pts0, more], axis=1)
    wts = np.concatenate([wts0, 1e-5 * (0.5 + rng.random((5, 65)))], axis=1)
    lam = np.concatenate([lam0, LAM_I + np.linspace(-70e-9, 70e-9, 256)])
    for a in (pts, wts, lam):
        a.setflags(write=False)
    return np.ascontiguousarray(pts), np.ascontiguousarray(wts), ki, ks, lam


@functools.lru_cache(maxsize=None)
def _lam_sg():
    lam = np.array(_geometry_sg()[4])
    special, _ = _special_wavelengths()
    lam[1:1 + len(special)] = special
    lam.setflags(write=False)
    return lam


# name -> (dtype, the optional fields given, per species (Z, f): the name of a field or a number, the order: "field" or a number).
# Every instantiation (V x Vd x dtype), 1 and 4 species (Z1 and f2 are 0 on blocks: g = 0 at some points), Ti NULL, the order as a
# field and uniform.
CONFIGS = {
    "f64 V Vd 4 fields": ("float64", ("Ti", "V", "Vd"), (("Z0", "f0"), ("Z1", "f1"), ("Z2", "f2"), ("Z3", "f3")), "field"),
    "f64 V 1 uniform": ("float64", ("Ti", "V"), ((3.5, 1.0),), "field"),
    "f64 Vd 2 mixed, Ti NULL, m = 3.5": ("float64", ("Vd",), ((6.0, "f0"), ("Z1", 0.5)), 3.5),
    "f64 1 field Z": ("float64", ("Ti",), (("Z0", 1.0),), "field"),
    "f32 V Vd 1 uniform, Ti NULL": ("float32", ("V", "Vd"), ((3.5, 2.0),), "field"),
    "f32 V 4 mixed": ("float32", ("Ti", "V"), (("Z0", 0.4), ("Z1", "f1"), (2.0, "f2"), ("Z3", "f3")), "field"),
    "f32 Vd 1 field Z, m = 5": ("float32", ("Ti", "Vd"), (("Z0", 1.0),), 5.0),
    "f32 4 fields": ("float32", ("Ti",), (("Z0", "f0"), ("Z1", "f1"), ("Z2", "f2"), ("Z3", "f3")), "field"),
}
SPECIAL = "f64 1 field Z"


def _host_inputs(config):
    dtype_name, given, spec, order = CONFIGS[config]
    f = _all(dtype_name)
    fields = {k: f[k] for k in ("ne", "Te") + given}
    species = [(A_SPECIES[j], f[Z] if isinstance(Z, str) else Z, f[fr] if isinstance(fr, str) else fr) for j, (Z, fr) in enumerate(spec)]
    return fields, species, _order_field(dtype_name) if order == "field" else order


WIDE_LAMBDAS = np.array(sorted(set(range(16)) | set(range(0, 513, 4))))  # what the longdouble reference is formed at


@functools.lru_cache(maxsize=None)
def _reference(config, wide=False):
    """restate_sg for the first 1, 64, 65 and 130 points: {nq: (P, weight, keep, scale)} -- on all 513 wavelengths, or, in
    longdouble, on the special ones and every fourth (WIDE_LAMBDAS; wavelengths do not interact)."""
    pts, wts, ki, ks, _ = _geometry_sg()
    fields, species, order = _host_inputs(config)
    lam = _lam_sg()[WIDE_LAMBDAS] if wide else _lam_sg()
    out = restate_sg(fields, species, order, AX, pts, wts, ki, ks, lam, LAM_I, np.longdouble if wide else np.float64, NQ_SG)
    for tup in out.values():
        for a in tup:
            a.setflags(write=False)
    return out


def test_sample_error_constant():
    """Test 5: K of test 6 -- the float64 restatement against the one whose sample arithmetic (the tables g_i, pow, exp, log, the
    quadrature sums, the incomplete gamma function's loops) runs in longdouble, on test 6's own inputs (every point; the special wavelengths and every
    fourth of the others), in units of u f_l sum_q |term_q| A_q.  A_q counts the roundings the new lines add to test_thomson_multi.py's: the relative error of chi_e
    is that of R, a sum of 48 terms of which each exp(-t^m) carries (1 + t^m) roundings of its argument and is divided by
    t^2 - x^2 (N_R sums those magnitudes; beside a node the divisor is small and N_R grows accordingly); exp(-y) of the
    imaginary part and of the electron factor carries m roundings of y = pow(x, m)'s argument xs = xe r and y of its own, hence
    (m + 2) min(y, 745); Gamma(2/m, y) below the series' limit is a difference, hence N_Q = (GAM + gamma)/Gamma.  GAM and the
    point constants are +, *, / and sqrt only and agree bit for bit on both sides.  K_SAMPLE = 8 x the measurement covers two
    sides and a pow, exp or log that errs by an ulp.  This test holds the measurement itself to twice the recorded value (another
    libm).  Measured on the build machine: 6.20 over all 513 wavelengths (one species whose charge is a field; 3.4 to 5.9
    elsewhere) and 5.38 on the wavelengths this test forms the longdouble reference at."""
    worst = {}
    for config in CONFIGS:
        ref, ref_l = _reference(config), _reference(config, True)
        for nq in NQ_SG:
            P, w, keep, scale = ref[nq]
            P, scale = P[:, WIDE_LAMBDAS], scale[:, WIDE_LAMBDAS]
            P_l, w_l, keep_l, _ = ref_l[nq]
            assert np.array_equal(w, w_l) and np.array_equal(keep, keep_l)
            assert not np.any((P_l == 0) & (P != 0)) and np.all(np.abs(P_l[P == 0]) <= UNDERFLOW)  # see UNDERFLOW
            nz = np.abs(P) > UNDERFLOW
            worst[config] = max(worst.get(config, 0.0), float(np.max(np.abs(P - P_l)[nz] / (U * scale[nz]))))
    print("float64 against longdouble samples, in u f_l sum |term| A_q: " + "; ".join(f"{k}: {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) <= 2 * K_MEASURED


def test_the_inputs_visit_every_path():
    """The configurations cover every instantiation, 1 and 4 species and both kinds of order; the layout has, inside the first
    chunk of 64 points, points of exactly m = 2 (and of a blend within 2^-30 of it), clamped points on both sides, a dropped NaN
    point, and super-Gaussian points; the special wavelengths put xs of the chosen point on a node (|xs - t_i| <= 1e-13, the
    Taylor branch), 1e-9 beside one, and |xs| on both sides of T; the continued fraction and the series both run."""
    seen = {(CONFIGS[c][0], "V" in CONFIGS[c][1], "Vd" in CONFIGS[c][1]) for c in CONFIGS}
    assert len(seen) == 8 and {len(CONFIGS[c][2]) for c in CONFIGS} >= {1, 4} and {CONFIGS[c][3] == "field" for c in CONFIGS} == {True, False}
    pts = _geometry_sg()[0]
    mo, inside = gather(np.float64(_order_field("float64")), AX, pts[:4, :64].reshape(-1, 3))
    with np.errstate(invalid="ignore"):
        assert np.sum(inside & (mo == 2.0)) >= 2 and np.sum(inside & (mo < 2.0)) >= 2 and np.sum(inside & (mo > 5.0)) >= 2
        assert np.sum(inside & np.isnan(mo)) >= 1 and np.sum(inside & (mo > 2.1) & (mo < 4.9)) >= 100
    # the special wavelengths, on the configuration they were made for
    Te, m = _first_point(SPECIAL)
    special, targets = _special_wavelengths()
    fields, species, order = _host_inputs(SPECIAL)
    p, w = pts[0:1, 2:3], np.ones((1, 1))
    ne, ins = gather(fields["ne"], AX, p[0])
    assert ins[0] and ne[0] > 0 and 2.1 < m < 4.9
    ks = _geometry()[3]
    L = wavelength_stage(special, LAM_I, float(ks[0, 2]))
    val = lambda a: gather(a, AX, p[0])[0] if np.ndim(a) == 3 else np.full(1, float(a))
    Q = point_stage_sg(ne, val(fields["Te"]), val(fields["Ti"]), [val(Z) for _, Z, _ in species], [val(f) for _, _, f in species],
                       [A for A, _, _ in species], np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1), np.ones(1), val(order))
    s = sample_stage_sg(L, Q, False, False)
    xs, T = s["xs"][0], s["T"][0]
    assert Q["sg"][0] and np.max(np.abs(xs[:5] - targets[:5])) <= 1e-13
    print(f"special wavelengths: |xs - node| = {np.abs(xs[:5] - targets[:5])}; exactly on a node: {int(np.sum(xs[:5] == targets[:5]))}")
    assert np.all(np.abs(xs[5:8] - targets[5:8]) <= 1e-13)
    assert xs[8] < T < xs[9] and abs(xs[8] - (T - 1e-3)) <= 1e-12 and abs(xs[9] - (T + 1e-3)) <= 1e-12
    # over all 513 wavelengths the same point has |xs| on both sides of T and takes both evaluations of Gamma(2/m, y)
    s = sample_stage_sg(wavelength_stage(_lam_sg(), LAM_I, float(ks[0, 2])), Q, False, False)
    y = np.abs(s["xs"][0]) ** Q["m"][0]
    assert np.any(np.abs(s["xs"][0]) < T) and np.any(np.abs(s["xs"][0]) >= T) and np.any(y < Q["z2"][0] + 1) and np.any(y >= Q["z2"][0] + 1)


# ================================================================ tests on the GPU
def _upload(eng, config, override=None):
    dtype_name, given, spec, order = CONFIGS[config]
    f = dict(_all(dtype_name), order=_order_field(dtype_name))
    f.update(override or {})
    names = {"ne", "Te", *given} | {v for pair in spec for v in pair if isinstance(v, str)} | ({"order"} if order == "field" else set())
    return _Fields(eng, {k: f[k] for k in sorted(names)})


def _run(eng, F, config, nq, nl, order=None, multi=False, vols=slice(None)):
    pts, wts, ki, ks, _ = _geometry_sg()
    lam = _lam_sg()
    spec = CONFIGS[config][2]
    species = [(A_SPECIES[j], *(F[v] if isinstance(v, str) else v for v in s)) for j, s in enumerate(spec)]
    if order is None:
        order = F["order"] if CONFIGS[config][3] == "field" else CONFIGS[config][3]
    args = (LAM_I, np.ascontiguousarray(pts[vols, :nq]), np.ascontiguousarray(wts[vols, :nq]), np.ascontiguousarray(ki[vols]),
            np.ascontiguousarray(ks[vols]), lam[:nl])
    if multi:
        return eng.thomson_multi(F["ne"], F["Te"], F.get("Ti"), F.get("V"), F.get("Vd"), species, *args)
    return eng.thomson_sg(F["ne"], F["Te"], F.get("Ti"), F.get("V"), F.get("Vd"), species, order, *args)


def _w_bound(dtype_name, nq):
    wts = _geometry_sg()[1]
    return 2 * (nq + 8) * U * np.sum(np.abs(wts[:, :nq]), axis=1) * float(np.max(_plasma(dtype_name)["ne"]))


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_kernel_against_the_restatement(eng, config):
    """Test 6.  Every instantiation of k_thomson_sg on test_thomson.py's 9 x 8 x 7 grid and 5 volumes, 1 / 64 / 65 / 130 points (the
    LDS chunk is 64) and 1 / 256 / 257 / 513 wavelengths (the tile is 256); the order a field spanning 2..5 with exact 2.0 nodes,
    values below 2 and above 5 (clamped), an infinite and a NaN node (dropped: the weight shows it, as the restatement's does),
    or uniform; points outside the box; wavelengths on, and 1e-9 beside, quadrature nodes and on both sides of T.  The decisions
    are asserted equal: where the restatement gives a zero (an exact one, or an underflowed sample: UNDERFLOW) the kernel does, and
    nowhere else; a volume without kept points gives exact zeros.  The values are asserted
    within K_SAMPLE u f_l sum_q |term_q| A_q per sample and the weights within 2 (Nq + 8) u sum_q |w_q| max|ne|.  Printed: the
    largest ratio.  On an MI355X: at most 4.07 of the allowed 49.6 (float64, one species whose charge is a field; 1.40 to 2.93
    elsewhere); the weights equal bit for bit.  Fails before this entry existed: engine.thomson_sg is missing."""
    F = _upload(eng, config)
    worst, weights_equal = 0.0, True
    try:
        for nq in NQ_SG:
            P_ref, w_ref, keep, scale = _reference(config)[nq]
            for nl in NL_SG:
                P, w = _run(eng, F, config, nq, nl)
                assert P.shape == (5, nl) and w.shape == (5,)
                ref, sc = P_ref[:, :nl], scale[:, :nl]
                assert np.array_equal(np.abs(P) <= UNDERFLOW, np.abs(ref) <= UNDERFLOW), (nq, nl)
                assert np.all(P[w_ref == 0] == 0), (nq, nl)  # a volume whose points are all dropped: exact zeros
                assert np.array_equal(w == 0, w_ref == 0), (nq, nl)
                assert np.all(P[4] == 0) and w[4] == 0 and w[0] > 0
                assert np.all(np.isfinite(P)) and np.all(np.isfinite(w))
                nz = np.abs(ref) > UNDERFLOW
                ratio = float(np.max(np.abs(P - ref)[nz] / (U * sc[nz]))) if nz.any() else 0.0
                print(f"  nq {nq} nl {nl}: {ratio:.2f}")
                worst = max(worst, ratio)
                assert ratio <= K_SAMPLE, (nq, nl, ratio)
                assert np.all(np.abs(w - w_ref) <= _w_bound(CONFIGS[config][0], nq)), (nq, nl)
                weights_equal &= bool(np.array_equal(w, w_ref))
    finally:
        F.close()
    print(f"{config}: largest |P - P_ref| = {worst:.2f} u f_l sum |term| A_q (allowed {K_SAMPLE:g}); "
          f"weights equal bit for bit: {weights_equal}")


@pytest.mark.gpu
def test_nan_order_drops_the_points_that_read_it(eng):
    """The NaN node of the order field drops exactly the kept points whose cell holds it: against the same field with the NaN
    replaced by 3.0 the weight falls by theirs, and a volume with no such point keeps its bits."""
    config = "f64 V Vd 4 fields"
    pts, wts, ki, ks, _ = _geometry_sg()
    mended = np.array(_order_field("float64"))
    mended[6, 4, 2] = 3.0
    fields, species, order = _host_inputs(config)
    keep_bad = _reference(config)[130][2]
    keep_ok = restate_sg(fields, species, mended, AX, pts, wts, ki, ks, _lam_sg()[:2], LAM_I)[130][2]
    lost = keep_ok & ~keep_bad
    assert lost.any() and not np.any(keep_bad & ~keep_ok)
    hit = lost.any(axis=1)
    assert hit.any() and not hit.all()
    bad, ok = _upload(eng, config), _upload(eng, config, {"order": mended})
    try:
        P1, w1 = _run(eng, bad, config, 130, 257)
        P0, w0 = _run(eng, ok, config, 130, 257)
    finally:
        bad.close()
        ok.close()
    ne_q = gather(np.array(_plasma("float64")["ne"]), AX, pts.reshape(-1, 3))[0].reshape(5, 130)
    assert np.allclose(w0 - w1, np.sum(np.where(lost, wts * ne_q, 0.0), axis=1), rtol=1e-12, atol=1e-12 * w0.max())
    for m in range(5):
        if hit[m]:
            assert w1[m] < w0[m] and not np.array_equal(P1[m], P0[m])
        else:
            assert P1[m].tobytes() == P0[m].tobytes() and w1[m] == w0[m]


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["f64 V Vd 4 fields", "f32 V Vd 1 uniform, Ti NULL", "f64 1 field Z", "f32 4 fields"])
def test_bit_identities(eng, config):
    """Test 7.  A uniform order of 2, and an order field of 2.0 everywhere, return engine.thomson_multi's P and weight bit for bit;
    a repeated call returns identical bits, with a call of another size in between; permuting the volumes permutes the rows."""
    dtype_name = CONFIGS[config][0]
    twos = np.full(tuple(len(a) for a in AX), 2.0, np.dtype(dtype_name))
    F = _upload(eng, config)
    extra = _Fields(eng, {"twos": twos})
    try:
        Pm, wm = _run(eng, F, config, 130, 513, multi=True)
        assert np.all(Pm[0] > 0)
        for order in (2.0, extra["twos"]):
            P, w = _run(eng, F, config, 130, 513, order=order)
            assert P.tobytes() == Pm.tobytes() and w.tobytes() == wm.tobytes(), type(order)
        first = _run(eng, F, config, 130, 513)
        again = _run(eng, F, config, 130, 513)
        other = _run(eng, F, config, 3, 255)  # the scratch block is reused at another size in between
        third = _run(eng, F, config, 130, 513)
        for a, b, c in zip(first, again, third):
            assert a.tobytes() == b.tobytes() == c.tobytes()
        assert other[0].shape == (5, 255) and not np.array_equal(first[0], Pm)
        perm = np.array([3, 0, 4, 2, 1])
        Pp, wp = _run(eng, F, config, 130, 513, vols=perm)
        assert Pp.tobytes() == first[0][perm].tobytes() and wp.tobytes() == first[1][perm].tobytes()
    finally:
        F.close()
        extra.close()


@pytest.mark.gpu
def test_field_checks_need_live_fields(eng):
    """Test 4's field cases (an sr_field exists only on a device): an order field with the wrong n_comp, dtype or grid is rejected
    with its own text, a closed one by Python; nothing to do is no error."""
    from synthpy_amd import _ffi as built

    pts, wts, ki, ks, _ = _geometry_sg()
    lam = _lam_sg()
    p = _plasma("float64")
    geo = (LAM_I, np.ascontiguousarray(pts[:, :3]), np.ascontiguousarray(wts[:, :3]), ki, ks, lam[:4])
    m64 = np.array(_order_field("float64"))
    ne, Te, V, order = (eng.Field(a, *AX32) for a in (p["ne"], p["Te"], p["V"], m64))
    order32 = eng.Field(np.float32(m64), *AX32)
    moved = eng.Field(m64, AX32[0], AX32[1], AX32[2] + np.float32(1e-6))
    small = eng.Field(m64[:-1], AX32[0][:-1], AX32[1], AX32[2])
    call = lambda o: eng.thomson_sg(ne, Te, None, None, None, [(12.0, 6.0, 1.0)], o, *geo)
    try:
        for o, msg in ((V, "order must have n_comp == 1"), (order32, "ne and order differ in dtype"),
                       (moved, "grids of ne and order differ on axis 2"), (small, "grids of ne and order differ on axis 0")):
            with pytest.raises(built.SynthrayError, match=msg):
                call(o)
        for bad in (1.5, 5.5, np.nan):
            with pytest.raises(built.SynthrayError, match="the uniform order must lie in"):
                call(bad)
        with pytest.raises(ValueError, match="order must be an open engine.Field or a number"):
            call(None)
        P, w = call(order)
        assert P.shape == (5, 4) and np.all(P[0] > 0) and ne.last_kernel_ms > 0
        P0, w0 = eng.thomson_sg(ne, Te, None, None, None, [(12.0, 6.0, 1.0)], order, LAM_I, np.zeros((0, 3, 3)), np.zeros((0, 3)), KI90, KS90, lam[:4])
        assert P0.shape == (0, 4) and w0.shape == (0,)
        P2, w2 = eng.thomson_sg(ne, Te, None, None, None, [(12.0, 6.0, 1.0)], 3.0, LAM_I, np.zeros((5, 0, 3)), np.zeros((5, 0)), ki, ks, lam[:4])
        assert np.all(P2 == 0) and np.all(w2 == 0)
        closed = eng.Field(m64, *AX32)
        closed.close()
        with pytest.raises(ValueError, match="closed"):
            call(closed)
    finally:
        for f in (ne, Te, V, order, order32, moved, small):
            f.close()


def _uniform_domains():
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    ne, Te, Ti, _ = PHYS_PLASMA
    new = NewDomain((4e-3, 4e-3, 4e-3), (9, 9, 9))
    old = OldDomain(*(np.linspace(-2e-3, 2e-3, 9),) * 3, 2e-3)
    for d in (new, old):
        d.external_ne(np.full((9, 9, 9), ne))
        d.external_Te(np.full((9, 9, 9), Te))
        d.external_Ti(np.full((9, 9, 9), Ti))
    return new, old


@pytest.mark.gpu
def test_physics_through_the_public_api(eng):
    """Test 8.  A uniform carbon plasma through thomson_scattering_sg of both API generations and through a rotated() domain that
    carries the order: at m = 4 against m = 2 the red electron-plasma-wave peak is higher and narrower and the ion-acoustic peak
    narrower (signs and orderings only).  order=2 equals thomson_scattering_multi bit for bit; order=None reads external_order;
    the public path equals r_e^2 engine.thomson_sg on the collection's quadrature; rotated() carries the order as it carries Ti,
    with fill 2.0."""
    from synthpy_amd import thomson

    probe = thomson.Probe(LAM_I, (0, 0, -3e-3), (0, 0, 1))
    coll = thomson.Collection(np.array([[0.0, 0.0, 0.0]]), (0, 1, 0), length=2e-4, n_quad=3)
    species = [thomson.Species(A, Z, f) for A, Z, f in PHYS_PLASMA[3]]
    for dom in _uniform_domains():
        spectrum = lambda d, **kw: (lambda lam: d.thomson_scattering_sg(probe, coll, lam, species, **kw).power[0])
        maxwell = _physics_numbers(spectrum(dom, order=2.0))
        dom.external_order(np.full((9, 9, 9), 4.0))
        sg = _physics_numbers(spectrum(dom))  # order=None: the domain's field
        print(f"{type(dom).__module__}: m = 2 / 4: " + ", ".join(f"{k} {maxwell[k]:.4g} / {sg[k]:.4g}" for k in sg))
        _assert_physics(maxwell, sg)
        a = dom.thomson_scattering_sg(probe, coll, PHYS_IAW, species, order=2.0)
        b = dom.thomson_scattering_multi(probe, coll, PHYS_IAW, species)
        assert a.power.tobytes() == b.power.tobytes() and a.weight.tobytes() == b.weight.tobytes() and np.all(a.power > 0)
        by_field = dom.thomson_scattering_sg(probe, coll, PHYS_EPW, species)
        by_number = dom.thomson_scattering_sg(probe, coll, PHYS_EPW, species, order=4.0)
        assert by_field.power.tobytes() == by_number.power.tobytes() and by_field.kernel_ms > 0
        pts, wts = coll.quadrature(probe)
        F = {k: eng.Field(v, dom.x, dom.y, dom.z) for k, v in dict(ne=dom.ne, Te=dom.Te, Ti=dom.Ti, order=dom.order).items()}
        try:
            P, w = eng.thomson_sg(F["ne"], F["Te"], F["Ti"], None, None, PHYS_PLASMA[3], F["order"], LAM_I, pts, wts, probe.direction,
                                  coll.direction, PHYS_EPW)
        finally:
            for f in F.values():
                f.close()
        assert np.array_equal(by_field.power, (thomson.R_E * thomson.R_E) * P) and np.array_equal(by_field.weight, w)
        rot = dom.rotated(33.0, about="y")
        assert rot.order.shape == (9, 9, 9) and np.any(rot.order == 2.0) and abs(rot.order[4, 4, 4] - 4.0) <= 1e-12
        assert np.all((rot.order == 2.0) == (rot.ne == 0.0))  # outside the source box: vacuum, Maxwellian
        _assert_physics(maxwell, _physics_numbers(spectrum(rot)))
        dom.order = None
        assert getattr(dom.rotated(33.0, about="y"), "order", None) is None
