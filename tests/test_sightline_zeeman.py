"""Zeeman-split lines along sightlines: sr_field_sightline_zeeman (sightline_zeeman.hip, zeeman_node.inc), engine.sightline_zeeman,
utils.eos_opacity.ZeemanLineTable, sightlines.sightline_zeeman / StokesSpectra and ScalarDomain.sightline_zeeman of both generations.

THE REFERENCE for the kernel is `restate_zeeman` below: include/synthray.h's rule in NumPy float64, operation for operation, with
tests/test_sightline_voigt.py's `voigt_restated` as its V(a, x).  The grid, the fields, the chords, `geometry`, `gather` and the
lattice interpolant are tests/test_sightline_lines.py's, test_sightlines.py's and test_table_emission.py's, imported.  chord, steps,
column and the set of missed chords are held BIT-EQUAL; I, Q, U, Vs and tau within budgets counted as follows (u = 2^-53).

* Everything B gives a sample -- Bn, Bu, Bv, T, B2, wL, sP, cS, cQ, cU, cV -- and the chord's frame are +, -, *, / and sqrt of gathered
  values, correctly rounded on either side: the same bits.  So sh = g*wL, x = ((omega - wc) - sh)*iw, x*x and the branch x*x > cut
  are the same bits too, as in the siblings.
* phi = V(a, x): E_phi = E_Vw + E_a, with E_Vw = MEASURED_WORST/u (1.62e-13 relative to H: tests/test_sightline_voigt.py's measured
  worst of V against scipy.special.wofz) and E_a = E_l(LG) + 3 as there (|d ln H / d ln a| <= 1); E_a = 0 where the table has no
  widths (a = 0 exactly).
* P_q = sum of s_k*phi_k, all positive: E_P = max_k E_phi + 1 + nk, nk the counted components of the line (product, sums).
* Ps = Pp + Pm (+1); eI = 0.5*(sP*P0) + (0.5*cS)*Ps, all positive: E_P + 3.  eP and eV cancel, so their error is taken against the
  ABSOLUTE sums AP = 0.5*(P0 + 0.5*Ps) and AV = 0.5*Ps: (E_P + 2) u AP and (E_P + 1) u AV.
* aJ = exp(l(LJ))*g: E_l(LJ) + 3 (the line tests').  A line's term aJ*eI: E_l(LJ) + 3 + E_P + 3 + 1; aJ*(eP*cQ): E_l(LJ) + 3 + E_P + 2 + 2
  against aJ*AP*|cQ|; jV the same against aJ*AV*|cV|.  Summed over nlc counted lines, each partial sum at most the absolute sum:
      E_j = max_l(E_l(LJ_l) + E_P_l) + 7 + nlc          for jI relative to itself and for jQ, jU, jV relative to
      AQ = sum_l aJ*AP*|cQ|,  AU = sum_l aJ*AP*|cU|,  AW = sum_l aJ*AV*|cV|;       E_aL the same from LK.
* The update is the line tests' recurrence with the same counts (exp, expm1: 2 u each, the division, the products and the sum: the
  constants 4 below), run once for I with its own magnitude T_I and once for each of Q, U, Vs with the running ABSOLUTE sum
  T <- T*E + (A/a)*F in place of the parameter's magnitude: the budgets of Q, U, Vs are relative to the sum of the absolute values
  of the terms that entered them, attenuated as the march attenuates them, not to Q, U, Vs themselves, which cancel.

Test 4 holds the float64 restatement to a second formulation -- V from scipy.special.wofz, every sum, exp, log and the recurrence
in np.longdouble -- within HALF of each budget.

The issue's n_freq are 70 and 300.  70 runs as two tiles of the 64-lane build with idle lanes in the last.  The library's own choice
for 300 is five tiles of the 64-lane build (256 lanes are chosen where 193..256 of every 256 are used); the cases with 300
frequencies set SYNTHRAY_SPECTRA_FL=256, the library's documented override, so that they run as two tiles of the 256-lane build.

MEASURED on the CPU and written into the tests below: the quadrature errors of tests 9 and 10.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import test_emission as nrl
import test_sightline_lines as gl
import test_sightline_voigt as vt
import test_table_emission as tab
from test_sightlines import EPS, TINY, _assert_exact, _poisoned, gather, geometry

LIGHT, ISP = gl.LIGHT, gl.ISP
SHAPE = gl.SHAPE
MEASURED_WORST = vt.MEASURED_WORST
E_VW = MEASURED_WORST / EPS
KL = 1.602176634e-19 / (2.0 * 9.1093837015e-31)
WING = 6.0
STOKES = ("I", "Q", "U", "V")
_CACHE = {}

built, eng = gl.built, gl.eng


# ---------------------------------------------------------------- the restatement
def frames(d, ref, toward):
    """The header's chord frame: (n^, e1, e2), each (3, N)."""
    d, r = np.asarray(d, np.float64), np.asarray(ref, np.float64)
    su = toward / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    n = [d[k] * su for k in range(3)]
    p = (r[0] * n[0] + r[1] * n[1]) + r[2] * n[2]
    t = [r[k] - p * n[k] for k in range(3)]
    tn = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    e1 = [t[k] / tn for k in range(3)]
    e2 = [n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]]
    return np.array(n), np.array(e1), np.array(e2)


def host_zeeman(lines):
    if lines.lorentz_width is not None:
        H = vt.host_voigt(lines)
    else:
        H = gl.host_lines(lines)
        H["LG"], H["GG"] = None, None
    H["patterns"] = [np.array(p, np.float64) for p in lines.patterns]
    return H


def restate_zeeman(F, co, o, d, ref, H, omegas, toward, step, max_steps, continuum, wing, backlight=None, second=False):
    """include/synthray.h's rule for sr_field_sightline_zeeman.  F: tests/test_sightline_lines.py's dict of fields plus B
    ((nx, ny, nz, 3)); ref: (3, N).  second=True: the second formulation -- V from scipy.special.wofz and every sum, exp, log and the
    recurrence in np.longdouble.  Returns I, Q, U, V, tau and their budgets bI, bQ, bU, bV, bt (N, n_freq), column, chord, steps,
    miss (N), and what the companion test asks about."""
    from scipy.special import wofz
    from synthpy_amd import engine

    g = [np.float64(np.float32(a)) for a in co]
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    om, e_ph, c_om = engine.spectrum_constants(omegas)
    G = geometry(g, o, d, step, max_steps)
    hit, n, h = G["hit"], G["n"], G["h"]
    N, NF, NL = o.shape[1], len(om), len(H["w0"])
    wt = np.longdouble if second else np.float64
    cut = np.float64(wing) * np.float64(wing)
    fr = frames(d, ref, toward)
    S = {k: np.zeros((N, NF), wt) for k in STOKES}
    if backlight is not None:
        S["I"] = np.array(backlight, wt)
    tau = np.zeros((N, NF), wt)
    T = {k: np.asarray(S[k], np.float64).copy() for k in STOKES}  # magnitudes: I's own, the absolute sums of Q, U, V
    Bd = {k: np.zeros((N, NF)) for k in STOKES}
    Bt = np.zeros((N, NF))
    column = np.zeros(N)
    with np.errstate(all="ignore"):
        su = toward / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    fields = [np.float64(F["ne"])] + [np.float64(F[k]) if np.ndim(F[k]) else float(F[k]) for k in ("Te", "Z")]
    has_ti, has_v = F.get("Ti") is not None, F.get("V") is not None
    if has_ti:
        fields.append(np.float64(F["Ti"]))
    if has_v:
        fields += [np.float64(F["V"][..., a]) for a in range(3)]
    fields += [np.float64(F["B"][..., a]) for a in range(3)]
    terms = counted_terms = 0
    nearcut, cases, ncount = np.inf, [0, 0, 0], np.zeros((N, NF), np.int64)
    drop, split = np.zeros(N, np.int64), [np.inf, 0.0]
    f64 = lambda v: np.asarray(v, np.float64)
    for m in range(int(n.max()) if N else 0):
        act = hit & (m < n)
        k = np.where(act, m if toward > 0 else n - 1 - m, 0)
        t = G["t0"] + (k + 0.5) * G["dt"]
        p = [o[a] + d[a] * t for a in range(3)]
        vals, inside = gather(fields, g, p, act)
        ne_s = np.where(inside, vals[0], 0.0)
        Te_s = np.where(inside, vals[1], 1.0) if np.ndim(vals[1]) else np.full(N, vals[1])
        Z_s = np.where(inside, vals[2], 1.0) if np.ndim(vals[2]) else np.full(N, vals[2])
        Ti_s = np.where(inside, vals[3], 1.0) if has_ti else Te_s
        with np.errstate(all="ignore"):
            column = np.where(act, column + ne_s * h, column)
            beta = np.zeros(N)
            if has_v:
                V = [np.where(inside, v, 0.0) for v in vals[-6:-3]]
                beta = (((V[0] * d[0] + V[1] * d[1]) + V[2] * d[2]) * su) / LIGHT
            Bs = [np.where(inside, v, 0.0) for v in vals[-3:]]
            Bn, Bu, Bv = [(Bs[0] * e[0] + Bs[1] * e[1]) + Bs[2] * e[2] for e in fr]
            Tt = Bu * Bu + Bv * Bv
            B2 = Tt + Bn * Bn
            zero = B2 == 0.0
            r = np.sqrt(B2)
            wL = np.where(zero, 0.0, KL * r)
            sP = np.where(zero, 1.0, Tt / B2)
            cS = np.where(zero, 0.5, 0.5 * (1.0 + (Bn * Bn) / B2))
            cQ = np.where(zero, 0.0, (Bu * Bu - Bv * Bv) / B2)
            cU = np.where(zero, 0.0, ((2.0 * Bu) * Bv) / B2)
            cV = np.where(zero, 0.0, Bn / r)
            dark = (Te_s <= 0) | (ne_s <= 0) | (Z_s <= 0) | (Ti_s <= 0) | ~inside
            live = act & ~dark
            a_ne, a_Te, a_Z, hw = ne_s.astype(wt), Te_s.astype(wt), Z_s.astype(wt), h.astype(wt)[:, None]
            ni = (a_ne * 1e-6) / a_Z
            lt, ld = np.log(a_Te), np.log(ni)
            i, ft = tab._locate(H["LT"].astype(wt), lt)
            j, fd = tab._locate(H["LD"].astype(wt), ld)

            def E_l(Gs, l):
                return (Gs[0][l] * (2 + 2 * np.abs(f64(ld)) + 5 * H["dD_max"]) + Gs[1][l] * (2 * np.abs(f64(lt)) + 5 * H["dT_max"]) + 2 * Gs[2][l])

            col = lambda v: v.astype(wt)[:, None]
            jS = {k_: np.zeros((N, NF), wt) for k_ in STOKES}
            aL = np.zeros((N, NF), wt)
            AA = {k_: np.zeros((N, NF)) for k_ in "QUV"}  # the absolute sums AQ, AU, AW
            counted, nlc = np.zeros((N, NF), bool), np.zeros((N, NF))
            EJ, EK = np.zeros((N, NF)), np.zeros((N, NF))
            for l in range(NL):
                wc = H["w0"][l] * (1.0 + beta)
                wd = H["w0"][l] * (np.sqrt(H["ci"][l] * Ti_s) / LIGHT)
                iw = 1.0 / wd
                gg = ISP * iw
                aJ = np.exp(tab._interp(H["LJ"][l].astype(wt), i, j, ft, fd)) * gg.astype(wt)
                if H["LG"] is not None:
                    av = np.exp(tab._interp(H["LG"][l].astype(wt), i, j, ft, fd)) * iw.astype(wt)
                    Ea = E_l(H["GG"], l)[:, None] + 3
                else:
                    av, Ea = np.zeros(N, wt), 0.0
                a64 = np.broadcast_to(f64(av)[:, None], (N, NF))
                P = {-1.0: np.zeros((N, NF), wt), 0.0: np.zeros((N, NF), wt), 1.0: np.zeros((N, NF), wt)}
                any_, nk = np.zeros((N, NF), bool), np.zeros((N, NF))
                for q, gk, sk in H["patterns"][l]:
                    sh = gk * wL
                    x = ((om[None, :] - wc[:, None]) - sh[:, None]) * iw[:, None]
                    x2 = x * x
                    keep = ~(x2 > cut) & live[:, None]
                    phi = np.zeros((N, NF), wt)
                    if keep.any():
                        if second:
                            phi[keep] = wofz(x[keep] + 1j * a64[keep]).real
                        else:
                            phi[keep] = vt.voigt_restated(a64[keep], x[keep])[0]
                    P[q] = np.where(keep, P[q] + wt(sk) * phi, P[q])
                    any_ |= keep
                    nk += keep
                    terms += int(live.sum()) * NF
                    counted_terms += int(keep.sum())
                    drop += (live[:, None] & ~keep).sum(axis=1)
                    if live.any() and NF and np.isfinite(cut):
                        nearcut = min(nearcut, float(np.nanmin(np.abs(x2[live] / cut - 1.0))))
                if live.any():
                    s_ = (np.abs(wL) * iw)[live]
                    split = [min(split[0], float(np.nanmin(s_))), max(split[1], float(np.nanmax(s_)))]
                Ps = P[1.0] + P[-1.0]
                eI = 0.5 * (col(sP) * P[0.0]) + (0.5 * col(cS)) * Ps
                eP = 0.5 * (P[0.0] - 0.5 * Ps)
                eV = 0.5 * (P[1.0] - P[-1.0])
                AP, AV = f64(0.5 * (P[0.0] + 0.5 * Ps)), f64(0.5 * Ps)
                aJc = aJ[:, None]
                jS["I"] = np.where(any_, jS["I"] + aJc * eI, jS["I"])
                jS["Q"] = np.where(any_, jS["Q"] + aJc * (eP * col(cQ)), jS["Q"])
                jS["U"] = np.where(any_, jS["U"] + aJc * (eP * col(cU)), jS["U"])
                jS["V"] = np.where(any_, jS["V"] + aJc * (eV * col(cV)), jS["V"])
                for k_, A_, c_ in (("Q", AP, cQ), ("U", AP, cU), ("V", AV, cV)):
                    AA[k_] = np.where(any_, AA[k_] + f64(aJc) * A_ * np.abs(c_)[:, None], AA[k_])
                EP = E_VW + Ea + 1 + nk
                EJ = np.where(any_, np.maximum(EJ, E_l(H["GJ"], l)[:, None] + EP), EJ)
                if H["LK"] is not None:
                    aK = np.exp(tab._interp(H["LK"][l].astype(wt), i, j, ft, fd)) * gg.astype(wt)
                    aL = np.where(any_, aL + aK[:, None] * eI, aL)
                    EK = np.where(any_, np.maximum(EK, E_l(H["GK"], l)[:, None] + EP), EK)
                else:  # the rule as written: aK = 0 and aL = aL + 0*eI, which a NaN eI makes NaN (and tau with it)
                    aL = np.where(any_, aL + wt(0.0) * eI, aL)
                counted |= any_
                nlc += any_
            ncount += counted
            Ej = np.where(counted, EJ + 7 + nlc, 0.0)
            EaL = np.where(counted & (H["LK"] is not None), EK + 7 + nlc, 0.0)
            if continuum:
                ac, Sc, xc = nrl._node(a_ne[:, None], a_Te[:, None], a_Z[:, None], om[None, :], e_ph[None, :], c_om[None, :])
                Eac, Esc = np.where(ac != 0, gl.E_AC, 0.0), np.where(ac != 0, 4 + xc, 0.0)
            else:
                ac, Sc, Eac, Esc = np.zeros((N, NF), wt), np.zeros((N, NF), wt), np.zeros((N, NF)), np.zeros((N, NF))
            act2 = act[:, None] & np.ones((1, NF), bool)
            d0 = ac * hw
            a0, F0 = np.exp(-d0), -np.expm1(-d0)
            a_ = ac + aL
            d1 = a_ * hw
            thin = counted & act2 & (d1 == 0)
            gen = counted & act2 & ~thin
            quiet = act2 & ~counted
            a1, F1 = np.exp(-d1), -np.expm1(-d1)
            Ea_ = np.maximum(Eac, EaL) + 1
            ea1, ea0 = Ea_ + 1, Eac + 1
            for k_ in STOKES:
                if k_ == "I":
                    b1, b0, b2 = ((ac * Sc + jS["I"]) / a_) * F1, Sc * F0, jS["I"] * hw
                    m1, m0, m2 = f64(b1), f64(b0), f64(b2)
                    es1 = np.maximum(Eac + Esc + 1, Ej) + 1 + Ea_ + 1
                    es0 = Esc
                else:
                    b1, b0, b2 = (jS[k_] / a_) * F1, np.zeros((N, NF), wt), jS[k_] * hw
                    m1, m0, m2 = f64((AA[k_] / f64(a_)) * f64(F1)), np.zeros((N, NF)), AA[k_] * f64(hw)
                    es1 = Ej + 1 + Ea_ + 1
                    es0 = 0.0
                if continuum:
                    new = np.where(gen, S[k_] * a1 + b1, np.where(thin, S[k_] + b2, np.where(quiet, S[k_] * a0 + b0, S[k_])))
                else:
                    new = np.where(gen, S[k_] * a1 + b1, np.where(thin, S[k_] + b2, np.where(quiet, S[k_] + wt(0.0), S[k_])))
                Bg = f64(a1) * (Bd[k_] + (4 + ea1 * f64(d1)) * T[k_]) + m1 * (es1 + ea1 + 4)
                Bn_ = f64(a0) * (Bd[k_] + (4 + ea0 * f64(d0)) * T[k_]) + m0 * (es0 + ea0 + 4)
                Bh = Bd[k_] + T[k_] + m2 * (Ej + 2)
                Bd[k_] = np.where(gen, Bg, np.where(thin, Bh, np.where(quiet, Bn_, Bd[k_])))
                T[k_] = np.where(gen, T[k_] * f64(a1) + m1, np.where(thin, T[k_] + m2, np.where(quiet, T[k_] * f64(a0) + m0, T[k_])))
                S[k_] = new
            tau = np.where(gen, tau + d1, np.where(thin, tau, np.where(act2, tau + d0, tau)))
            Bt = np.where(gen, Bt + ea1 * f64(d1), np.where(act2 & ~thin, Bt + ea0 * f64(d0), Bt))
            cases[0] += int(quiet.sum())
            cases[1] += int(gen.sum())
            cases[2] += int(thin.sum())
    floor = (4 * n * TINY)[:, None]
    out = dict(tau=tau, column=column, chord=G["chord"], steps=n.astype(np.int32), miss=~hit, terms=terms, counted=counted_terms,
               nearcut=nearcut, cases=cases, ncount=ncount, drop=drop, split=split, frames=fr)
    with np.errstate(all="ignore"):
        for k_ in STOKES:
            out[k_] = S[k_]
            out["b" + k_] = 2 * EPS * Bd[k_] + floor
            out["T" + k_] = T[k_]
        out["bt"] = EPS * (2 * Bt + 2 * n[:, None] * f64(tau)) + floor
    return out


def _assert_close(got, ref, what, names=STOKES + ("tau",), scale=1.0):
    """tests/test_sightlines.py's _assert_close on the five maps: NaN sets equal, finite where the reference is, within budget."""
    worst = {}
    for name in names:
        have, want, lim = np.asarray(got[name]), np.asarray(ref[name]).astype(np.float64), scale * ref["bt" if name == "tau" else "b" + name]
        assert have.shape == want.shape, (what, name, have.shape, want.shape)
        assert np.array_equal(np.isnan(have), np.isnan(want)), f"{what}: the NaN set of {name} differs from the restatement's"
        fin = np.isfinite(want)
        assert np.all(np.isfinite(have[fin])), f"{what}: {name} is not finite where the restatement is"
        dist = np.abs(have[fin] - want[fin])
        assert np.all(dist <= lim[fin]), f"{what}: {name} is off by up to {np.max(dist / np.maximum(lim[fin], TINY)):.3f} budgets"
        pos = lim[fin] > 0
        worst[name] = float(np.max(dist[pos] / lim[fin][pos])) if np.any(pos) else 0.0
    print(f"{what}: max |d| / budget: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


def _assert_cone(got, ref, what):
    """I^2 >= Q^2 + U^2 + V^2 up to the budgets of the four."""
    I, Q, U, V = (np.asarray(got[k], np.float64) for k in STOKES)
    fin = np.isfinite(I) & np.isfinite(Q) & np.isfinite(U) & np.isfinite(V)
    p = np.sqrt(Q * Q + U * U + V * V)
    slack = ref["bI"] + ref["bQ"] + ref["bU"] + ref["bV"]
    assert np.all(p[fin] <= I[fin] + slack[fin]), f"{what}: outside the cone by up to {np.max((p - I)[fin] / np.maximum(slack[fin], TINY)):.3f} budgets"


# ---------------------------------------------------------------- inputs
def max_steps():
    from synthpy_amd import _ffi

    return 2 * _ffi.ZEEMAN_CHUNK + 2


def d2_pattern():
    from synthpy_amd.utils.eos_opacity import lande_pattern

    return lande_pattern(1.5, 4.0 / 3.0, 0.5, 2.0)


def make_zeeman(n_line, lk, lg, pattern, strength=1.0):
    """tests/test_sightline_voigt.py's make_voigt (lg) or tests/test_sightline_lines.py's make_lines with a pattern per line:
    "triplet", "d2", or "mixed" (line l takes the triplet, D2, D1 in turn)."""
    from synthpy_amd.utils.eos_opacity import ZeemanLineTable, lande_pattern, normal_triplet

    base = vt.make_voigt(n_line, lk, strength=strength) if lg else gl.make_lines(n_line, lk, strength=strength)
    pats = {"triplet": [normal_triplet()], "d2": [d2_pattern()], "mixed": [normal_triplet(), d2_pattern(), lande_pattern(0.5, 2.0 / 3.0, 0.5, 2.0)]}[pattern]
    return ZeemanLineTable.from_lines(base, [pats[l % len(pats)] for l in range(n_line)])


def field_B(dt=np.float64, seed=31, scale=60.0):
    """B on the tests' grid: every component uniform in +-scale tesla, so that the splitting kL|B|/wd runs from a fraction of a
    thermal width to several."""
    return np.random.default_rng(seed).uniform(-scale, scale, SHAPE + (3,)).astype(dt)


def default_ref(d):
    ref = np.zeros(d.shape)
    ref[np.argmin(np.abs(d), axis=0), np.arange(d.shape[1])] = 1.0
    return ref


NFREQS, NLINES = (70, 300), (1, 2, 3)
_BITS = np.random.default_rng(13).integers(0, 2, (12, 6))
CASES = tuple(dict(f64=bool(b[0]), toward=+1 if b[1] else -1, ti=bool(b[2]), v=bool(b[3]), lk=bool(b[4]), cont=bool(b[5]), nf=NFREQS[k % 2],
                   nl=NLINES[(k // 2) % 3], te_f=k % 4 != 3, z_f=k % 5 < 3, view="pinhole" if k == 6 else "six", k=k, lg=k % 6 != 5,
                   pattern=("triplet", "d2", "mixed")[k % 3], wing=WING if k % 2 == 1 else np.inf)
              for k, b in enumerate(_BITS))


def _id(c):
    return gl._id(c) + f"-LG{int(c['lg'])}-{c['pattern']}-wing{c['wing']:g}"


def _inputs(c, **over):
    c = dict(c, **over)
    R = gl._inputs(c)
    lines = make_zeeman(c["nl"], c["lk"], c["lg"], c["pattern"])
    om = gl.make_freqs(lines, c["nf"], 40 + c["k"], sort=c["k"] % 2 == 0)
    back = np.random.default_rng(60 + c["k"]).uniform(0.0, 2e-6, (R["o"].shape[1], len(om)))
    dt = np.float64 if c["f64"] else np.float32
    R["F"] = dict(R["F"], B=field_B(dt))
    rng = np.random.default_rng(90 + c["k"])
    ref = default_ref(R["d"]) + 0.3 * rng.uniform(-1, 1, R["d"].shape)  # oblique to every chord, of any length
    R.update(c=c, lines=lines, om=om, back=back, step=R["K"]["step"] / 3, max_steps=max_steps(), refdir=ref)
    return R


def _restate(R, second=False, **kw):
    c = R["c"]
    F = dict(R["F"], B=kw.pop("B", R["F"]["B"]))
    return restate_zeeman(F, R["K"]["co"], R["o"], R["d"], kw.pop("refdir", R["refdir"]), host_zeeman(kw.pop("lines", R["lines"])), kw.pop("om", R["om"]),
                          c["toward"], R["step"], R["max_steps"], c["cont"], c["wing"], backlight=kw.pop("backlight", R["back"]), second=second, **kw)


def _case(c):
    key = ("case", c["k"])
    if key not in _CACHE:
        R = _inputs(c)
        R["ref"] = _restate(R)
        _CACHE[key] = R
    return _CACHE[key]


def _upload(eng, R, B="own"):
    f = gl._upload(eng, R)
    b = R["F"]["B"] if isinstance(B, str) else B
    return f + [None if b is None else eng.Field(b, *R["K"]["co"])]


def _run(eng, R, fields=None, timed=True, **kw):
    """engine.sightline_zeeman on freshly uploaded fields (unless given); I, Q, U, V, tau (n, n_freq) as the restatement's.  Cases of
    300 frequencies run on the 256-lane build (the module docstring)."""
    own = fields is None
    fields = _upload(eng, R) if own else fields
    c = R["c"]
    old = os.environ.get("SYNTHRAY_SPECTRA_FL")
    om = kw.pop("om", R["om"])
    if len(om) == 300:
        os.environ["SYNTHRAY_SPECTRA_FL"] = "256"
    try:
        out = eng.sightline_zeeman(*fields, R["o"], R["d"], kw.pop("refdir", R["refdir"]), lines=kw.pop("lines", R["lines"]), omegas=om,
                                   continuum=c["cont"], wing=c["wing"], toward=c["toward"], step=R["step"], max_steps=R["max_steps"],
                                   backlight=kw.pop("backlight", R["back"]), **kw)
        if "intensity" in out:
            assert not timed or fields[0].last_kernel_ms > 0
            assert out["intensity"].shape == out["optical_depth"].shape == out["Q"].shape == (R["o"].shape[1], len(om))
            out["I"], out["tau"] = out["intensity"], out["optical_depth"]
        return out
    finally:
        if len(om) == 300:
            if old is None:
                del os.environ["SYNTHRAY_SPECTRA_FL"]
            else:
                os.environ["SYNTHRAY_SPECTRA_FL"] = old
        if own:
            gl._close(fields)


def _chunk_case(fl, N, chunk):
    R = gl._chunk_case(fl, N, chunk)
    c = dict(R["c"], wing=WING if N % 2 else np.inf, lg=True, pattern="mixed", nf={64: 70, 256: 300}[fl])
    lines = make_zeeman(3, True, True, "mixed")
    om = gl.make_freqs(lines, c["nf"], 40 + c["k"], sort=True)
    R["F"] = dict(R["F"], B=field_B(np.float64))
    R.update(c=c, lines=lines, om=om, back=np.random.default_rng(5).uniform(0.0, 2e-6, (3, len(om))), refdir=np.array([[0.1, 1.0, 0.3]] * 3).T.copy())
    return R


# ================================================================ CPU tests
def test_header_ctypes_and_python_signatures(built):
    """1: the header's prototype and struct, the ctypes binding, the chunk and its LDS bound, the Python signatures; the library
    exports the new symbols."""
    raw = open(os.path.join(ROOT, "include", "synthray.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+sr_field_sightline_zeeman\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 26
    names = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["ne", "Te", "Ti", "Z", "V", "B", "lines", "p", "n", "origin", "dir", "ref", "n_freq", "omega", "e_ph", "c_omega", "backlight",
                     "I", "Q", "U", "Vs", "tau", "column", "chord", "steps", "kernel_ms"]
    kinds = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]
    assert kinds[6] == "const sr_zeeman_table *" and kinds[7] == "const sr_voigt_params *" and kinds[5] == "const sr_field *"
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*sr_zeeman_table\s*;", text)
    fields = ["voigt", "n_comp", "comp"]
    assert m and re.findall(r"\b(" + "|".join(fields) + r")\b", m.group(1)) == fields
    Z = built.ZeemanTable
    assert [f[0] for f in Z._fields_] == fields and C.sizeof(Z) == 88 and Z.voigt.offset == 0 and Z.n_comp.offset == 72 and Z.comp.offset == 80
    assert dict(Z._fields_)["voigt"] is built.VoigtTable
    assert re.search(r"#define\s+SR_MAX_ZEEMAN\s+24\b", raw) and built.MAX_ZEEMAN == 24
    res, args = built.SYMBOLS["sr_field_sightline_zeeman"]
    assert res is C.c_int and len(args) == 26 and args[8] is C.c_int64 and args[12] is C.c_int32
    assert hasattr(built.lib, "sr_field_sightline_zeeman") and built.SYMBOLS["sr_zeeman_chunk"] == (C.c_int, [])
    from synthpy_amd import engine, sightlines
    from synthpy_amd._domain import DomainExtras
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain
    from synthpy_amd.utils.eos_opacity import VoigtLineTable, ZeemanLineTable

    chunk = built.lib.sr_zeeman_chunk()
    assert built.ZEEMAN_CHUNK == engine.ZEEMAN_CHUNK == chunk and 2 * chunk <= 64
    assert 2 * chunk * (16 + 6 * 32) * 8 + 8192 <= 64 * 1024 < 2 * (chunk + 2) * (16 + 6 * 32) * 8 + 8192
    assert engine.LARMOR == KL
    mk = open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()
    assert "sightline_zeeman.hip" in mk and "zeeman_node.inc" in mk and "-ffp-contract=off" in mk
    a, b, c = raw.index("/* ---- Voigt lines along sightlines"), raw.index("/* ---- Zeeman-split lines along sightlines"), raw.index("/* ---- proton radiography")
    assert a < b < c
    mine = raw[b:c]
    for word in ("sr_field_sightline_voigt's, word for word", "1.602176634e-19", "9.1093837015e-31", "B NULL", "dichroism", "Faraday rotation",
                 "Paschen-Back", "hyperfine", "positive helicity", "along e1", "no trigonometry", "1e-9", "1e-6", "does NOT delegate"):
        assert word in mine, word

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.sightline_zeeman) == ["ne", "Te", "Ti", "Z", "V", "B", "origins", "directions", "reference", "lines", "omegas", "continuum",
                                              "wing", "toward", "step", "max_steps", "backlight", "want"]
    par = inspect.signature(engine.sightline_zeeman).parameters
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names(engine.sightline_zeeman)[9:])
    assert par["wing"].default == np.inf and par["continuum"].default is False and par["backlight"].default is None
    assert names(sightlines.sightline_zeeman) == ["domain", "view", "lines", "wavelengths", "photon_energies", "continuum", "wing", "step",
                                                  "max_steps", "fields", "reference"]
    assert names(NewDomain.sightline_zeeman) == names(OldDomain.sightline_zeeman) == ["self", "view", "lines", "wavelengths", "photon_energies",
                                                                                       "continuum", "wing", "step", "max_steps", "reference"]
    assert NewDomain.sightline_zeeman is DomainExtras.sightline_zeeman is OldDomain.sightline_zeeman
    assert issubclass(ZeemanLineTable, VoigtLineTable) and issubclass(sightlines.StokesSpectra, sightlines.LineSpectra)
    assert names(ZeemanLineTable.from_lande) == ["table", "J_upper", "g_upper", "J_lower", "g_lower"]
    assert names(sightlines.StokesSpectra.analysed) == ["self", "angle", "circular"] and names(sightlines.StokesSpectra.b_parallel) == ["self", "window", "g_eff"]
    for doc in (engine.sightline_zeeman.__doc__, sightlines.sightline_zeeman.__doc__, DomainExtras.sightline_zeeman.__doc__):
        for word in ("dichroism", "Faraday rotation", "Paschen-Back", "hyperfine"):
            assert word in doc, word


def test_argument_checks_come_before_the_device(built):
    """2: a rejected argument is SR_ERR_INVALID with a text that names sr_field_sightline_zeeman, and the device is never
    initialised: the calls carry a B that is no field (it is never dereferenced before ne's check) and NULL for the other fields, so
    a call that passes every other check ends at 'NULL ne'.  The checks of B's grid, dtype and n_comp need live fields: they are
    in test_nan_edges_and_field_checks."""
    from synthpy_amd import engine

    lib, ptr = built.lib, built.ptr
    o0, d0 = np.zeros((3, 2)), np.ones((3, 2))
    r0 = np.array([[0.0, 1.0], [1.0, 0.0], [0.0, 0.0]])
    out = [np.zeros((2, 5)) for _ in range(5)]
    om0, e0, c0 = engine.spectrum_constants(np.linspace(7.5e15, 7.6e15, 5))
    fakeB = C.c_void_p(C.addressof(C.create_string_buffer(256)))  # not NULL: the Zeeman path

    def params(wing=np.inf, toward=1, step=1e-4, max_steps=10, continuum=0):
        p = built.VoigtParams()
        p.march.toward, p.march.max_steps, p.march.continuum, p.march.step, p.wing = toward, max_steps, continuum, step, wing
        return p

    def table(pattern="mixed", lg=True):
        return engine.zeeman_table_params(make_zeeman(3, True, lg, pattern))

    t0, keep0 = table()

    def call(p, n=2, o=o0, d=d0, r=r0, t=t0, nf=5, B=fakeB, I=out[0], Q=out[1], U=out[2], V=out[3], tau=out[4]):
        return lib.sr_field_sightline_zeeman(None, None, None, None, None, B, None if t is None else C.byref(t), None if p is None else C.byref(p), n,
                                             ptr(o), ptr(d), ptr(r), nf, ptr(om0), ptr(e0), ptr(c0), None, ptr(I), ptr(Q), ptr(U), ptr(V), ptr(tau),
                                             None, None, None, None)

    def err(text, *a, **kw):
        assert call(*a, **kw) == -1, text
        msg = built.last_error()
        assert text in msg and "sr_field_sightline_zeeman" in msg, (text, msg)

    err("NULL line table", params(), t=None)
    for name in ("r", "Q", "U", "V"):
        err("NULL ref, Q, U or Vs", params(), **{name: None})
    for name in ("o", "d", "I", "tau"):
        err("NULL argument", params(), **{name: None})
    err("NULL argument", None)
    for member in ("n_comp", "comp"):
        t, keep = table()
        setattr(t, member, None)
        err("NULL component table", params(), t=t)
    for q in (2.0, -2.0, 0.5, np.nan):
        t, keep = table()
        keep[-1][4, 0] = q
        err("q of component 1 of line 1 must be -1, 0 or +1", params(), t=t)
    for g in (np.nan, np.inf, -np.inf):
        t, keep = table()
        keep[-1][0, 1] = g
        err("non-finite g of component 0 of line 0", params(), t=t)
    for s in (0.0, -0.5, np.nan, np.inf):
        t, keep = table()
        keep[-1][2, 2] = s
        err("s of component 2 of line 0 must be finite and positive", params(), t=t)
    t, keep = table()
    keep[-1][3, 2] = 0.25 + 1e-8  # the first sigma- component of the D2 line: its group no longer sums to 1
    err("the strengths of the q = -1 group of line 1 sum to", params(), t=t)
    t, keep = table()
    keep[-1][3, 2] = 0.25 + 1e-11  # within the stated 1e-9
    err("NULL ne", params(), t=t)
    for nc in (0, -1, 25):
        t, keep = table()
        keep[-2][2] = nc
        err("n_comp of line 2 must be 1..24", params(), t=t)
    for v in (np.nan, np.inf):
        r = r0.copy()
        r[2, 1] = v
        err("non-finite ref of line 1", params(), r=r)
    r = r0.copy()
    r[:, 0] = (2.0, 2.0, 2.0 + 1e-6)  # d = (1, 1, 1): within 1e-6 rad of the chord
    err("ref of line 0 is parallel to the chord", params(), r=r)
    r[:, 0] = 0.0
    err("ref of line 0 is parallel to the chord", params(), r=r)
    r[:, 0] = (-3.0, -3.0, -3.0)
    err("ref of line 0 is parallel to the chord", params(), r=r)
    for wing in (np.nan, 0.0, -3.0):
        err("wing must be positive", params(wing=wing))
    t, keep = table(lg=False)  # LG NULL does not delegate: wing is read
    assert t.voigt.LG is None
    err("wing must be positive", params(wing=0.0), t=t)
    err("NULL ne", params(), t=t)
    err("toward", params(toward=0))
    err("step must be finite and positive", params(step=0.0))
    err("n x frequency tiles exceeds 2^31 - 1 workgroups", params(), n=2 ** 31)
    a = np.ones((3, 2))
    a[2, 1] = np.nan
    err("non-finite direction of line 1", params(), d=a)
    # in order: every other argument was fine; n == 0 and n_freq == 0 do not skip the checks
    err("NULL ne", params())
    err("NULL ne", params(wing=WING, continuum=1))
    err("NULL ne", params(), n=0)
    err("NULL ne", params(), nf=0)
    # B NULL: sr_field_sightline_voigt's checks under its own name; the component table, ref, Q, U and Vs may be NULL
    t, keep = table()
    t.n_comp = t.comp = None
    assert call(params(), B=None, t=t, r=None, Q=None, U=None, V=None) == -1
    assert "NULL ne" in built.last_error() and "sr_field_sightline_voigt" in built.last_error()
    assert keep0 is not None
    with pytest.raises(ValueError, match="patterns"):
        from synthpy_amd import sightlines

        sightlines.sightline_zeeman(object(), sightlines.Chords(np.zeros((3, 1)), np.ones((3, 1)), -1), vt.make_voigt(1, True), wavelengths=[5e-7])


def test_from_lande_and_the_table_by_hand(built):
    """3: from_lande against patterns worked out by hand; g_eff against the closed form; every group sums to 1 to rounding for all
    J <= 7/2; the table's checks; with_lte_absorption keeps the patterns."""
    from synthpy_amd.utils.eos_opacity import ZeemanLineTable, lande_pattern, normal_triplet

    tri = normal_triplet()
    assert tri.tolist() == [[-1, -1, 1], [0, 0, 1], [1, 1, 1]]
    assert np.array_equal(lande_pattern(1, 1.0, 0, 1.0), tri) and np.array_equal(lande_pattern(1, 1.0, 0, 7.0), tri)
    for Ju, Jl in ((2.5, 1.5), (2, 2), (2.5, 3.5), (0.5, 0.5), (1, 2)):
        assert np.array_equal(lande_pattern(Ju, 1.0, Jl, 1.0), tri), (Ju, Jl)
    d1 = lande_pattern(0.5, 2.0 / 3.0, 0.5, 2.0)
    assert np.allclose(d1, [[-1, -4 / 3, 1], [0, -2 / 3, 0.5], [0, 2 / 3, 0.5], [1, 4 / 3, 1]], rtol=0, atol=4 * EPS)
    d2 = lande_pattern(1.5, 4.0 / 3.0, 0.5, 2.0)
    assert np.allclose(d2, [[-1, -5 / 3, 0.25], [-1, -1, 0.75], [0, -1 / 3, 0.5], [0, 1 / 3, 0.5], [1, 1, 0.75], [1, 5 / 3, 0.25]], rtol=0, atol=4 * EPS)
    base = gl.make_lines(2, True)
    z = ZeemanLineTable.from_lande(base, [0.5, 1.5], [2.0 / 3.0, 4.0 / 3.0], 0.5, 2.0)
    assert np.allclose(z.g_eff, [4.0 / 3.0, 7.0 / 6.0], rtol=4 * EPS, atol=0) and z.lorentz_width is None
    assert np.array_equal(z.patterns[0], d1) and np.array_equal(z.patterns[1], d2) and np.array_equal(z.omega0, base.omega0)
    worst, most = 0.0, 0
    for Ju in np.arange(0.0, 4.0, 0.5):
        for dJ in (-1, 0, 1):
            Jl = Ju - dJ
            if Jl < 0 or Jl > 3.5 or (Ju == 0 and Jl == 0):
                continue
            gu, gl_ = 1.37, 0.71
            p = lande_pattern(Ju, gu, Jl, gl_)
            most = max(most, len(p))
            for q in (-1.0, 0.0, 1.0):
                sel = p[:, 0] == q
                if sel.any():
                    worst = max(worst, abs(float(np.sum(p[sel, 2])) - 1.0))
            sel = p[:, 0] == 1.0
            want = 0.5 * (gu + gl_) + 0.25 * (gu - gl_) * (Ju * (Ju + 1) - Jl * (Jl + 1))
            assert abs(float(np.sum(p[sel, 1] * p[sel, 2])) - want) <= 16 * EPS * abs(want), (Ju, Jl)
            minus = p[p[:, 0] == -1.0]
            assert np.allclose(np.sort(-minus[:, 1]), np.sort(p[sel, 1]), rtol=0, atol=8 * EPS)  # sigma- mirrors sigma+
    print(f"from_lande over J <= 7/2: a group's strengths sum to 1 within {worst / EPS:.1f} u; at most {most} components")
    assert worst <= 8 * EPS and most == 22 <= 24
    assert len(lande_pattern(3.5, 1.2, 2.5, 0.9)) == 18
    for args, word in (((0, 1, 0, 1), "dipole"), ((2, 1, 0, 1), "dipole"), ((1.5, 1, 1, 1), "dipole"), ((0.3, 1, 0.3, 1), "J_upper"), ((1, np.nan, 0, 1), "finite")):
        with pytest.raises(ValueError, match=word):
            lande_pattern(*args)
    for bad, word in (([[2, 0, 1]], "q must be"), ([[0, np.inf, 1]], "g must be"), ([[0, 0, -1]], "s must be"), ([[0, 0, 0.5]], "sum to"),
                      (np.zeros((25, 3)), r"1\.\.24"), (None, "patterns must be given")):
        with pytest.raises(ValueError, match=word):
            ZeemanLineTable.from_lines(base, None if bad is None else [np.array(bad, np.float64)] * 2)
    with pytest.raises(ValueError, match="one array per line"):
        ZeemanLineTable.from_lines(base, [tri])
    v = ZeemanLineTable.from_lines(vt.make_voigt(2, False), tri)
    assert v.lorentz_width is not None and len(v.patterns) == 2 and v.absorption is None
    lte = v.with_lte_absorption()
    assert isinstance(lte, ZeemanLineTable) and lte.patterns is v.patterns and lte.lorentz_width is v.lorentz_width and lte.absorption is not None
    n_comp, comp = z.packed_patterns()
    assert n_comp.tolist() == [4, 6] and n_comp.dtype == np.int32 and comp.shape == (10, 3)


def test_restatement_against_the_second_formulation(built):
    """4: the float64 restatement (voigt_restated for V) against the same rule with V from scipy.special.wofz and every sum, exp, log
    and the recurrence in np.longdouble: I, Q, U, Vs and tau agree within HALF of the budgets the GPU tests use."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    worst = dict.fromkeys(STOKES + ("tau",), 0.0)
    for k in (0, 3, 5, 10):
        R = _case(CASES[k])
        w = _assert_close(_restate(R, second=True), R["ref"], f"second formulation, {_id(CASES[k])}", scale=0.5)
        worst = {n: max(worst[n], w[n]) for n in worst}
    print("float64 restatement against wofz + np.longdouble: worst fraction of the one-sided budget used: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert worst["I"] > 0 and worst["Q"] > 0 and worst["V"] > 0


def test_tested_inputs_meet_the_conditions(built):
    """5b: on the restatement alone: no x*x within 1e-9 of the cut; with the finite wing every chord that hits drops a term and counts
    one; the splitting spans from under one thermal width to several; every update case occurs; Q, U, Vs are not small beside
    their absolute sums everywhere (the budgets bind) and cancel somewhere (they are needed); flags and sizes are covered."""
    total = np.zeros(3, np.int64)
    lo, hi = np.inf, 0.0
    for c in CASES:
        ref = _case(c)["ref"]
        print(f"{_id(c)}: {ref['terms']} terms, {ref['counted'] / max(ref['terms'], 1):.3f} counted, least |x2/cut - 1| {ref['nearcut']:.2e}, "
              f"updates {ref['cases']}, splitting {ref['split'][0]:.2f} .. {ref['split'][1]:.2f} widths")
        assert ref["nearcut"] > 1e-9, _id(c)
        for k in STOKES + ("tau",):
            assert np.all(np.isfinite(ref[k])), (k, _id(c))
        hitc = ~ref["miss"]
        assert np.any(ref["miss"]) and hitc.any()
        if np.isfinite(c["wing"]):
            assert np.all(ref["drop"][hitc] > 0) and np.all(ref["ncount"][hitc].sum(axis=1) > 0), _id(c)
        else:
            assert ref["counted"] == ref["terms"] and np.all(ref["drop"] == 0)
        assert c["view"] == "pinhole" or (np.any(ref["steps"] == 1) and np.any(ref["steps"] == max_steps()))
        for k in "QUV":
            ratio = np.abs(ref[k][hitc]) / np.maximum(ref["T" + k][hitc], TINY)
            assert np.all(ratio <= 1 + 1e-9) and ratio.max() > 0.05 and np.median(ratio) < 0.9, (k, _id(c))
        total += ref["cases"]
        lo, hi = min(lo, ref["split"][0]), max(hi, ref["split"][1])
    assert lo < 1.0 and hi > 3.0
    assert np.all(total > 0), f"update cases not counted / counted / counted with dtau == 0: {total}"
    for name in ("f64", "ti", "v", "lk", "cont", "te_f", "z_f", "lg"):
        assert {c[name] for c in CASES} == {True, False}, name
    assert {c["toward"] for c in CASES} == {1, -1} and {c["view"] for c in CASES} == {"six", "pinhole"}
    assert {(c["nf"], c["nl"]) for c in CASES} == {(a, b) for a in NFREQS for b in NLINES}
    assert {c["pattern"] for c in CASES} == {"triplet", "d2", "mixed"} and {np.isfinite(c["wing"]) for c in CASES} == {True, False}
    assert {(c["lk"], c["cont"]) for c in CASES} == {(a, b) for a in (True, False) for b in (True, False)}


def test_stokes_spectra_by_hand(built):
    """10b: analysed on three analysers and b_parallel on a spectrum made by hand; the default reference."""
    from synthpy_amd import sightlines
    from synthpy_amd.utils.eos_opacity import ZeemanLineTable, normal_triplet

    lines = ZeemanLineTable.from_lines(gl.make_lines(1, False), normal_triplet())
    w0 = lines.omega0[0]
    wd, Bpar = 2e12, 7.5
    om = w0 + wd * np.linspace(-12, 12, 481)
    sig = lambda s: np.exp(-(((om - w0) - s * KL * Bpar) / wd) ** 2)
    I = np.stack([0.5 * (sig(1) + sig(-1)), 3.0 * sig(1)])
    V = np.stack([0.5 * (sig(1) - sig(-1)), 3.0 * sig(1)])
    Q, U = 0.3 * I, -0.2 * I
    ch = sightlines.Chords(np.zeros((3, 2)), np.ones((3, 2)), -1)
    sp = sightlines.StokesSpectra(ch, I, np.zeros_like(I), np.zeros(2), np.zeros(2), np.zeros(2, np.int32), om, lines, Q, U, V)
    assert np.array_equal(sp.analysed(angle=0.0), 0.5 * (I + Q)) and np.array_equal(sp.analysed(circular=-1), 0.5 * (I - V))
    assert np.allclose(sp.analysed(angle=np.pi / 2), 0.5 * (I - Q), rtol=0, atol=2 * EPS * np.abs(I).max())
    assert np.allclose(sp.analysed(angle=np.pi / 4), 0.5 * (I + U), rtol=0, atol=2 * EPS * np.abs(I).max())
    assert np.array_equal(sp.analysed(circular=+1), 0.5 * (I + V))
    for kw in (dict(), dict(angle=0.0, circular=1), dict(circular=2)):
        with pytest.raises(ValueError):
            sp.analysed(**kw)
    got = sp.b_parallel(11 * wd)
    # chord 0: Gaussians sampled 20 times a width over +-12 widths: the trapezoid's error is far below rounding; chord 1 has no
    # negative-helicity light: NaN
    assert got.shape == (2, 1) and abs(got[0, 0] / Bpar - 1.0) < 1e-12 and np.isnan(got[1, 0])
    assert abs(sp.b_parallel(11 * wd, g_eff=2.0)[0, 0] / (Bpar / 2) - 1.0) < 1e-12
    with pytest.raises(ValueError, match="window"):
        sp.b_parallel(-1.0)
    ch = sightlines.Chords(np.zeros((3, 3)), np.array([[1.0, 0.2, 0.3], [0.0, 1.0, -0.3], [0.5, 0.5, 0.1]]).T.copy().T.reshape(3, 3), -1)
    ref = sightlines.default_reference(ch)
    assert ref.shape == (3, 3) and np.all(ref.sum(axis=0) == 1) and np.array_equal(np.argmax(ref, axis=0), np.argmin(np.abs(ch.directions), axis=0))
    cam = sightlines.PinholeCamera((0, 0, 1.0), (0, 0.1, -1.0), (0, 1, 0), 0.05, (2, 3), 1e-3)
    assert np.array_equal(sightlines.default_reference(cam), np.broadcast_to(cam.y[:, None], (3, 6)))


# ================================================================ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_kernel_against_restatement(eng, c):
    """5: chord, steps, column and the missed chords bit-equal, the NaN sets equal (none), I, Q, U, Vs and tau within the counted
    budgets; 10a: the cone."""
    R = _case(c)
    got = _run(eng, R)
    _assert_exact(got, R["ref"], _id(c))
    _assert_close(got, R["ref"], _id(c))
    _assert_cone(got, R["ref"], _id(c))
    miss = R["ref"]["miss"]
    assert np.array_equal(got["I"][miss], R["back"][miss]) and all(np.all(got[k][miss] == 0) for k in ("Q", "U", "V", "tau"))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 3, 7])
def test_b_null_is_sightline_voigt(eng, k):
    """6: B = None: I, tau, column, chord and steps carry engine.sightline_voigt's bits and Q, U, Vs are exact zeros (the patterns
    and the reference are not read); a B field of zeros with any pattern gives exact zeros in Q, U, Vs too, and I and tau within
    the two budgets of the Voigt entry's."""
    R = _case(CASES[k if CASES[k]["lg"] else k + 1])
    c = R["c"]
    assert c["lg"]
    fields = _upload(eng, R, B=np.zeros_like(R["F"]["B"]))
    try:
        kw = dict(lines=R["lines"], omegas=R["om"], continuum=c["cont"], wing=c["wing"], toward=c["toward"], step=R["step"], max_steps=R["max_steps"],
                  backlight=R["back"])
        old = eng.sightline_voigt(*fields[:5], R["o"], R["d"], **kw)
        new = eng.sightline_zeeman(*fields[:5], None, R["o"], R["d"], None, **kw)
        assert list(new) == list(old) + ["Q", "U", "V"]
        for name in old:
            assert new[name].dtype == old[name].dtype and np.array_equal(new[name], old[name], equal_nan=True), name
        for name in ("Q", "U", "V"):
            assert new[name].shape == old["intensity"].shape and not np.any(new[name]) and not np.any(np.signbit(new[name])), name
        zero = _run(eng, R, fields=fields)
        ref0 = _restate(R, B=np.zeros_like(R["F"]["B"]))
        for name in ("Q", "U", "V"):
            assert not np.any(zero[name]), name
        for name in ("column", "chord", "steps"):
            assert np.array_equal(zero[name], old[name]), name
        refv = vt.restate_voigt(R["F"], R["K"]["co"], R["o"], R["d"], vt.host_voigt(R["lines"]), R["om"], c["toward"], R["step"], R["max_steps"],
                                c["cont"], c["wing"], backlight=R["back"])
        assert np.all(np.abs(zero["I"] - old["intensity"]) <= ref0["bI"] + refv["bI"])
        assert np.all(np.abs(zero["tau"] - old["optical_depth"]) <= ref0["bt"] + refv["bt"])
        assert fields[0].last_kernel_ms > 0 and np.any(old["steps"] > 0)
    finally:
        gl._close(fields)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 4, 8])
def test_exact_symmetries(eng, k):
    """7: bit for bit: B -> -B leaves I, Q, U, tau and flips Vs; swapping the shifts (and strengths) of the q = +1 and q = -1 groups
    does the same; a permutation of the frequencies permutes the results; a repeated call repeats its bits.  Within budget: ref
    turned by psi about the chord turns (Q, U) by 2 psi."""
    from synthpy_amd.utils.eos_opacity import ZeemanLineTable

    R = _case(CASES[k])
    fields = _upload(eng, R)
    minus = eng.Field(-R["F"]["B"], *R["K"]["co"])
    try:
        got = _run(eng, R, fields=fields)
        again = _run(eng, R, fields=fields)
        for name in STOKES + ("tau", "column", "chord", "steps"):
            assert np.array_equal(got[name], again[name], equal_nan=True), name
        assert np.any(got["V"] != 0) and np.any(got["Q"] != 0) and np.any(got["U"] != 0)
        flipped = _run(eng, R, fields=fields[:5] + [minus])
        swapped_patterns = []
        for p in R["lines"].patterns:
            q = p.copy()
            q[:, 0] = np.where(p[:, 0] == 0, 0.0, -p[:, 0])  # the q = +1 group takes the q = -1 group's (g, s), in its order
            swapped_patterns.append(q)
        swapped = _run(eng, R, fields=fields, lines=ZeemanLineTable.from_lines(R["lines"], swapped_patterns))
        for other, what in ((flipped, "B -> -B"), (swapped, "q -> -q")):
            for name in ("I", "Q", "U", "tau"):
                assert np.array_equal(other[name], got[name]), (what, name)
            assert np.array_equal(other["V"], -got["V"]), what
        order = np.random.default_rng(3).permutation(len(R["om"]))
        s = _run(eng, R, fields=fields, om=R["om"][order], backlight=np.ascontiguousarray(R["back"][:, order]))
        for name in STOKES + ("tau",):
            assert np.array_equal(s[name], got[name][:, order]), name
        # ref turned by psi about the chord: e1' = e1 cos psi + e2 sin psi
        psi = 0.7
        n_, e1, e2 = R["ref"]["frames"]
        turned = _run(eng, R, fields=fields, refdir=np.ascontiguousarray(2.5 * (e1 * np.cos(psi) + e2 * np.sin(psi)) + 0.4 * n_))
        c2, s2 = np.cos(2 * psi), np.sin(2 * psi)
        # both sides within their budgets, the rotation's own roundings (3) and the turned frame's (e1' is e1 cos + e2 sin to 8 u)
        lim = 2 * (R["ref"]["bQ"] + R["ref"]["bU"]) + 32 * EPS * (R["ref"]["TQ"] + R["ref"]["TU"])
        assert np.all(np.abs(turned["Q"] - (got["Q"] * c2 + got["U"] * s2)) <= lim) and np.all(np.abs(turned["U"] - (-got["Q"] * s2 + got["U"] * c2)) <= lim)
        for name in ("I", "V", "tau"):
            assert np.all(np.abs(turned[name] - got[name]) <= 2 * R["ref"]["bt" if name == "tau" else "b" + name]), name
    finally:
        gl._close(fields + [minus])


@pytest.mark.gpu
@pytest.mark.parametrize("fl", [64, 256])
@pytest.mark.parametrize("which", range(6))
def test_chunk_boundaries_of_the_sample_staging(eng, fl, which):
    """8: chords of ZEEMAN_CHUNK*k + {-1, 0, 1} samples, k = 1, 2, at both lane widths (70 frequencies: the 64-lane build, 300 with
    the override: the 256-lane build), against the restatement."""
    chunk = eng.ZEEMAN_CHUNK
    N = [chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1][which]
    R = _chunk_case(fl, N, chunk)
    ref = _restate(R)
    assert ref["steps"].tolist() == [N] * 3 and ref["cases"][1] > 0
    got = _run(eng, R)
    _assert_exact(got, ref, f"{N} samples, tiles of {fl}")
    _assert_close(got, ref, f"{N} samples, tiles of {fl}")
    _assert_cone(got, ref, f"{N} samples, tiles of {fl}")


def _uniform_inputs(Bvec, om, toward=+1, lk=False, n_steps=20):
    """A uniform plasma with a uniform field on the tests' grid, one chord along +x through the box; Gaussian triplet, thin lines."""
    from synthpy_amd.utils.eos_opacity import ZeemanLineTable, normal_triplet

    K = gl._grid()
    g = K["g"]
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    c = dict(CASES[0], f64=True, toward=toward, ti=True, v=False, lk=lk, cont=False, nf=len(om), nl=1, te_f=True, z_f=True, view="six", k=500,
             lg=False, pattern="triplet", wing=np.inf)
    F = dict(ne=np.full(SHAPE, 2e24), Te=np.full(SHAPE, 25.0), Z=np.full(SHAPE, 2.0), Ti=np.full(SHAPE, 200.0), V=None,
             B=np.broadcast_to(np.asarray(Bvec, np.float64), SHAPE + (3,)).copy())
    o = np.array([[lo[0] - 2.0 ** -10, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])]]).T.copy()
    d = np.array([[1.0, 0.0, 0.0]]).T.copy()
    lines = ZeemanLineTable.from_lines(gl.make_lines(1, lk, strength=1e-6), normal_triplet())
    return dict(c=c, K=K, F=F, o=o, d=d, lines=lines, om=om, back=None, step=(hi[0] - lo[0]) / (n_steps - 0.5), max_steps=4 * n_steps,
                refdir=np.array([[0.0, 1.0, 0.0]]).T.copy())


@pytest.mark.gpu
def test_uniform_plasma_closed_forms(eng):
    """9: thin Gaussian triplet in a uniform plasma, splitting 5 thermal widths.  The light travels along +x (toward = +1), e1 = y,
    e2 = x cross y = z.  B along the light: Vs/I = +1 at the q = +1 peak and -1 at the q = -1 peak, with the sign of B.n^; no pi
    component; Q = U = 0 within budget.  B along e1: Q/I = +1 at the pi peak, -1 at the sigma peaks; Vs = 0 exactly.  Any angle:
    the frequency integral of I is exp(l(LJ))*chord and those of Q, U, Vs vanish, within the quadrature error of this grid of
    frequencies, 561 of them 0.05 widths apart over +-14 widths.  MEASURED on the restatement on the CPU: I's integral is off by
    less than 1 u of itself (0 in float64), Q's and U's by 3.1e-17 of I's, Vs's is 0 exactly (the grid is symmetric about omega0
    and Vs antisymmetric bit for bit).  A Gaussian's trapezoid error at this spacing, ~exp(-(pi/0.05)^2), and the tails beyond 9
    widths of the outermost component, exp(-81), are far below rounding; what is left is the rounding of the trapezoid's sum of 561
    positive terms, at most 561 u = 6.2e-14 of the integral of I, which is the bound asserted (beside the budgets' integral)."""
    base = _uniform_inputs((1.0, 0.0, 0.0), np.zeros(1))
    w0 = base["lines"].omega0[0]
    wd = base["lines"].thermal_width(200.0)[0]
    Bmag = 5.0 * wd / KL
    om = w0 + wd * np.linspace(-14.0, 14.0, 561)  # 0.05 widths apart; index 280 is the centre, 280 +- 100 the sigma peaks
    ctr, up, dn = 280, 380, 180
    for sign in (+1, -1):
        R = _uniform_inputs((sign * Bmag, 0.0, 0.0), om)
        got, ref = _run(eng, R), _restate(R)
        _assert_close(got, ref, f"B along the light, sign {sign:+d}")
        I, Q, U, V = (got[k][0] for k in STOKES)
        assert V[up] == sign * I[up] or abs(V[up] / I[up] - sign) < 1e-12
        assert abs(V[dn] / I[dn] + sign) < 1e-12
        assert I[ctr] < 1e-9 * I[up]  # no pi component: only the sigma components' tails, exp(-25) each
        assert np.all(np.abs(Q) <= ref["bQ"][0]) and np.all(np.abs(U) <= ref["bU"][0])
    R = _uniform_inputs((0.0, Bmag, 0.0), om)
    got, ref = _run(eng, R), _restate(R)
    _assert_close(got, ref, "B along e1")
    I, Q, U, V = (got[k][0] for k in STOKES)
    assert not np.any(V) and np.all(np.abs(U) <= ref["bU"][0])
    assert abs(Q[ctr] / I[ctr] - 1.0) < 1e-9 and abs(Q[up] / I[up] + 1.0) < 1e-9 and abs(Q[dn] / I[dn] + 1.0) < 1e-9  # the others' tails: exp(-25)
    # any angle
    R = _uniform_inputs((0.5 * Bmag, -0.6 * Bmag, 0.62 * Bmag), om)
    got, ref = _run(eng, R), _restate(R)
    _assert_close(got, ref, "B oblique")
    _assert_cone(got, ref, "B oblique")
    dw = np.diff(om)
    integral = lambda y: float(np.sum(0.5 * (y[1:] + y[:-1]) * dw))
    H = gl.host_lines(R["lines"])
    i, ft = tab._locate(H["LT"], np.log(25.0))
    j, fd = tab._locate(H["LD"], np.log(2e24 * 1e-6 / 2.0))
    want = float(np.exp(tab._interp(H["LJ"][0], i, j, ft, fd))) * float(got["chord"][0])
    quad = 561 * EPS
    tol = quad * want + integral(ref["bI"][0])
    print(f"integrals over frequency / (exp(l(LJ)) chord): I {integral(got['I'][0]) / want - 1:.3e} + 1, "
          + ", ".join(f"{k} {integral(got[k][0]) / want:.3e}" for k in "QUV") + f"; tolerance {tol / want:.3e}")
    assert abs(integral(got["I"][0]) - want) <= tol
    assert abs(integral(ref["I"][0]) - want) <= tol
    for k in "QUV":
        assert abs(integral(got[k][0])) <= quad * want + integral(ref["b" + k][0]), k


@pytest.mark.gpu
def test_b_parallel_read_out(eng):
    """10c: StokesSpectra.b_parallel on the kernel's spectra equals the same method on the restatement's within the propagated
    budget, and the restatement's equals the true B.n^ of a uniform oblique field within the grid's quadrature error (thin Gaussian
    triplet, splitting 2 widths, 561 frequencies 0.05 widths apart over +-14 widths, the window +-13.5 widths: MEASURED on the CPU,
    3.3e-16 relative.  The bound asserted is the rounding of the four trapezoid sums of 561 terms each, whose first moments weigh
    |omega - omega0| up to 13.5 widths against a centroid difference of 2.2 widths: 4 * 561 u = 2.5e-13)."""
    from synthpy_amd import sightlines

    base = _uniform_inputs((1.0, 0.0, 0.0), np.zeros(1))
    w0, wd = base["lines"].omega0[0], base["lines"].thermal_width(200.0)[0]
    Bmag = 2.0 * wd / KL
    om = w0 + wd * np.linspace(-14.0, 14.0, 561)
    Bvec = np.array([0.55, -0.6, 0.58]) * Bmag
    R = _uniform_inputs(Bvec, om)
    got, ref = _run(eng, R), _restate(R)
    _assert_close(got, ref, "oblique field for b_parallel")
    ch = sightlines.Chords(R["o"], R["d"], +1)
    mk = lambda S: sightlines.StokesSpectra(ch, np.float64(S["I"]), np.float64(S["tau"]), S["column"], S["chord"], S["steps"], om, R["lines"],
                                            np.float64(S["Q"]), np.float64(S["U"]), np.float64(S["V"]))
    b_got, b_ref = mk(got).b_parallel(13.5 * wd)[0, 0], mk(ref).b_parallel(13.5 * wd)[0, 0]
    true = Bvec[0]  # the light travels along +x
    # propagated: a centroid m1/m0 of y = 0.5(I +- V) moves by at most (|x|max * sum(b) dw + |cen| sum(b) dw) / m0
    dw = np.diff(om)
    trap = lambda y: float(np.sum(0.5 * (y[1:] + y[:-1]) * dw))
    bsum = trap(0.5 * (ref["bI"][0] + ref["bV"][0]))
    m0 = min(trap(0.5 * (np.float64(ref["I"][0]) + s * np.float64(ref["V"][0]))) for s in (1, -1))
    lim = 2 * (2 * 14.0 * wd * bsum / m0) / (2 * KL)
    print(f"b_parallel: kernel {b_got:.9e}, restatement {b_ref:.9e}, true {true:.9e} T; |kernel - restatement| / limit {abs(b_got - b_ref) / lim:.3f}")
    assert abs(b_got - b_ref) <= lim
    assert abs(b_ref / true - 1.0) <= 4 * 561 * EPS


@pytest.mark.gpu
def test_nan_edges_and_field_checks(eng, built):
    """11: a NaN in one corner of B poisons exactly the chords and frequencies the restatement says (those whose samples fall in its
    cells), and no other; a dark sample counts nothing (a chord through ne = 0 returns the backlight); the checks of B that need live
    fields: n_comp, grid, dtype."""
    R = _inputs(CASES[2])
    B = R["F"]["B"].copy()
    B[4, 3, 3, 1] = np.nan
    ref = _restate(R, B=B)
    bad = np.isnan(ref["V"])
    # a NaN shift is never dropped: whole chords, and never a chord that misses the box
    assert bad.any() and not bad.all() and np.array_equal(bad, np.repeat(bad.any(axis=1)[:, None], bad.shape[1], axis=1)) and not np.any(bad[ref["miss"]])
    fields = _upload(eng, R, B=B)
    try:
        got = _run(eng, R, fields=fields)
        for name in STOKES + ("tau",):
            assert np.array_equal(np.isnan(got[name]), np.isnan(ref[name])), name
        clean = ~bad.any(axis=1)
        assert clean.any()
        # dark: ne = 0 everywhere
        dark = dict(R, F=dict(R["F"], ne=np.zeros_like(R["F"]["ne"])))
        f2 = _upload(eng, dark)
        try:
            d = _run(eng, dict(dark, c=dict(dark["c"], cont=False)), fields=f2)
            assert np.array_equal(d["I"], R["back"]) and not np.any(d["Q"]) and not np.any(d["U"]) and not np.any(d["V"]) and not np.any(d["tau"])
        finally:
            gl._close(f2)
        # B must be a 3-vector field on ne's grid and of its dtype
        co = R["K"]["co"]
        wrong = [eng.Field(R["F"]["ne"], *co), eng.Field(B.astype(np.float32 if R["c"]["f64"] else np.float64), *co),
                 eng.Field(B[:-1], co[0][:-1], co[1], co[2])]
        try:
            for w in wrong:
                with pytest.raises(Exception, match="B"):
                    _run(eng, R, fields=fields[:5] + [w])
        finally:
            gl._close(wrong)
    finally:
        gl._close(fields)
    # the clean chords of the poisoned run carry the bits of the run without the NaN
    fields = _upload(eng, R)
    try:
        base = _run(eng, R, fields=fields)
        for name in STOKES + ("tau",):
            assert np.array_equal(got[name][clean], base[name][clean]), name
        # n == 0 and n_freq == 0 succeed and write nothing
        e0 = eng.sightline_zeeman(*fields, np.zeros((3, 0)), np.zeros((3, 0)), np.zeros((3, 0)), lines=R["lines"], omegas=R["om"], toward=1,
                                  step=R["step"], max_steps=5)
        assert e0["Q"].shape == (0, len(R["om"])) and e0["steps"].shape == (0,)
    finally:
        gl._close(fields)


@pytest.mark.gpu
def test_both_generations_return_the_engines_bits(eng):
    """11c: ScalarDomain.sightline_zeeman of both generations returns the bits of engine.sightline_zeeman on the same fields, in a
    StokesSpectra whose moments, fwhm and signal work on intensity; the default reference of Chords is the lab axis least aligned
    with each chord, a pinhole view's its up; a rotated() domain works unchanged."""
    from synthpy_amd import sightlines
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy import full_solver as fs
    from synthpy_amd.utils.eos_opacity import LineTable, VoigtLineTable, ZeemanLineTable

    dims, cell = (12, 9, 10), 5e-4
    lengths = tuple(cell * (m - 1) for m in dims)
    base = LineTable([1.0, 500.0], [1e17, 1e21], np.full((2, 2), 4.0e9), wavelengths=250e-9, mass_number=12.011)
    voigt = VoigtLineTable.power_law(base, 3e11, 1e24, zbar=2.0).with_lte_absorption()
    lines = ZeemanLineTable.from_lande(voigt, 1.5, 4.0 / 3.0, 0.5, 2.0)
    w0, wd = lines.omega0[0], lines.thermal_width(40.0)[0]
    om = w0 + wd * np.linspace(-12.0, 12.0, 70)
    rng = np.random.default_rng(5)
    ne = np.float32(10.0 ** rng.uniform(23.5, 24.5, dims))
    Ti = np.float32(rng.uniform(20.0, 60.0, dims))
    V = np.float32(rng.uniform(-2e5, 2e5, dims + (3,)))
    B = np.float32(rng.uniform(-40.0, 40.0, dims + (3,)))
    new = NewDomain(lengths, dims)
    old = fs.ScalarDomain(*[np.linspace(-L / 2, L / 2, m) for L, m in zip(lengths, dims)], lengths[2] / 2)
    for dom in (new, old):
        dom.external_ne(ne)
        dom.external_Te(30.0)
        dom.external_Z(2.0)
        dom.external_Ti(Ti)
        dom.external_V(V)
        dom.external_B(B)
    ch = sightlines.Chords([[-8e-3, 1e-4], [1e-4, -8e-3], [2e-4, 3e-4]], [[1.0, 0.1], [0.0, 1.0], [0.1, 0.0]], -1)
    lam = 2 * np.pi * LIGHT / om
    got = [dom.sightline_zeeman(ch, lines, wavelengths=lam, continuum=True, wing=8.0, step=cell, max_steps=60) for dom in (new, old)]
    ref = sightlines.default_reference(ch)
    assert ref.T.tolist() == [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for sp in got:
        assert isinstance(sp, sightlines.StokesSpectra) and sp.lines is lines and sp.intensity.shape == sp.Q.shape == (2, 70) and np.all(sp.steps > 0)
        assert np.all(np.isfinite(sp.intensity)) and np.all(sp.optical_depth > 0) and np.any(sp.V != 0) and np.any(sp.Q != 0)
        assert np.all(sp.intensity ** 2 * (1 + 1e-9) >= sp.Q ** 2 + sp.U ** 2 + sp.V ** 2)
        assert sp.moments(10 * wd)["radiance"].shape == (2, 1) and sp.fwhm(10 * wd).shape == (2, 1) and sp.signal().shape == (2,)
        assert np.all(np.isfinite(sp.b_parallel(11 * wd)))
    f = [eng.Field(a, new.x, new.y, new.z) for a in (ne, Ti, V, B)]
    try:
        o, d = ch.lines()
        raw = eng.sightline_zeeman(f[0], 30.0, f[1], 2.0, f[2], f[3], np.float64(o), np.float64(d), ref, lines=lines, omegas=got[0].omega,
                                   continuum=True, wing=8.0, toward=-1, step=cell, max_steps=60)
    finally:
        for h in f:
            h.close()
    for sp in got:
        for name in ("intensity", "optical_depth", "column", "chord", "steps", "Q", "U", "V"):
            assert np.array_equal(getattr(sp, name), raw[name]), name
    # a pinhole view: the maps come back in pixel order and shape; its reference is the camera's up
    cam = sightlines.PinholeCamera((1e-3, -2e-3, 25e-3), (0.05, 0.1, -1.0), (0, 1, 0), 50e-3, (3, 2), 2e-3)
    sp = new.sightline_zeeman(cam, lines, wavelengths=lam, step=cell, max_steps=60)
    assert sp.Q.shape == sp.V.shape == sp.intensity.shape == (3, 2, 70) and np.any(sp.V != 0)
    o, d = cam.lines()
    flat = sightlines.sightline_zeeman(new, sightlines.Chords(o, d, -1), lines, wavelengths=lam, step=cell, max_steps=60,
                                       reference=sightlines.default_reference(cam))
    for name in ("intensity", "Q", "U", "V", "optical_depth"):
        assert np.array_equal(getattr(sp, name).reshape(6, 70), getattr(flat, name)), name
    rot = new.rotated(25.0, about="y")
    assert rot.B is not None and np.shape(rot.B)[-1] == 3
    spr = rot.sightline_zeeman(ch, lines, wavelengths=lam, step=cell, max_steps=60)
    assert isinstance(spr, sightlines.StokesSpectra) and np.all(np.isfinite(spr.intensity)) and np.any(spr.V != 0)
    with pytest.raises(ValueError, match="exactly one"):
        new.sightline_zeeman(ch, lines)
    with pytest.raises(ValueError, match="ZeemanLineTable"):
        new.sightline_zeeman(ch, voigt, wavelengths=[250e-9])
    with pytest.raises(ValueError, match="reference"):
        new.sightline_zeeman(ch, lines, wavelengths=[250e-9], reference=np.zeros((3, 5)))
    new.B = None
    with pytest.raises(ValueError, match="external_B"):
        new.sightline_zeeman(ch, lines, wavelengths=[250e-9])
