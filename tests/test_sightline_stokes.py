"""Polarised transfer along sightlines: sr_field_sightline_stokes (sightline_stokes.hip, stokes_node.inc, voigt_node.inc's voigt_w),
engine.sightline_stokes, sightlines.sightline_stokes / StokesSpectra.polarisation_angle and degree, and ScalarDomain.sightline_stokes
of both generations.

THE REFERENCE for the kernel is `restate_stokes` below: include/synthray.h's rule in NumPy float64, operation for operation, built
from tests/test_sightline_zeeman.py's pieces (frames, host_zeeman, make_zeeman, field_B, the cases' inputs), with `voigt_w_restated`
(both parts of w(x + i a); its real part is tests/test_sightline_voigt.py's voigt_restated bit for bit) and `cell_update` (the
scaling-and-squaring update) stated here.  chord, steps, column and the set of missed chords are held BIT-EQUAL; I, Q, U, Vs and tau
within budgets counted as follows (u = 2^-53).

* Everything B gives a sample, the chord's frame, x, x*x and the branch x*x > cut are the same bits on either side, as in the
  siblings; so are neh/h, Bn and the faraday term's five operations (six roundings with the sum: 6 u of the term).
* (H, L) = W(a, x): E_W = MEASURED_WORST_W/u relative to |w| (test 2), plus COND_W*E_a for a's own error, E_a = E_l(LG) + 3 as in the
  Voigt tests (0 without widths); COND_W bounds |dw/d ln a|/|w| on the grid (test 2).  P_q and R_q are sums of s_k*H_k and s_k*L_k:
  both within (E_W + COND_W*E_a + 1 + nk) u of W_q = sum_k s_k*|w_k|, nk the line's counted components.
* A line's contribution to every one of the eleven coefficients is at most a*(W0 + Wp + Wm) in magnitude (the angular factors and
  the halves are at most 1), a = aJ or aK with E_l(LJ or LK) + 3 of its own, at most 5 further roundings, and one per line summed:
      E_j = max_l(E_l(LJ_l) + E_P_l) + 8 + nlc   relative to AJ = sum_l aJ*(W0 + Wp + Wm),   E_k the same from LK relative to AK.
  The continuum's ac and Sc carry the line tests' E_AC and 4 + x_c.
* The update.  The evolution over a sample is a contraction in the 2-norm (the symmetric part of K has the eigenvalues eI +-
  |(hQ, hU, hV)| >= 0), so a perturbation dK of the matrix and d eps of the source move the result by at most
  h*(|dK|*M + |d eps|), M = |X| + h*|eps| bounding the vector anywhere in the sample (1-norms), and what was there before is not
  amplified.  To that comes the update's own rounding, (C0 + C1*s + C2*nrm*h) u M, with the constants MEASURED in test 3 against
  mpmath.expm at 50 digits and a factor 4 of margin.  So along the chord
      b <- b + h*(|dK|*M + |d eps|) + (C0 + C1*s + C2*nrm*h) u M
  with |dK| = u*((E_AC + 2)*ac + 4*(E_k + 1)*AK + 6*|rV_faraday|) and |d eps| = u*((E_AC + E_Sc + 2)*ac*Sc + 4*(E_j + 1)*AJ).  One
  budget b serves I, Q, U and Vs: it is relative to the running norm of the Stokes vector, not to Q, U, Vs themselves.  The scalar
  shortcut's samples take the same formula with s = 0 (its exp and expm1 are within C0).  Both sides round, so 2 b is held.
* tau: the Zeeman tests' budget with hI's error against AK.

The issue's n_freq are 70 and 300: 70 runs as two tiles of the 64-lane build, 300 with SYNTHRAY_SPECTRA_FL=256 as two tiles of the
256-lane build (tests/test_sightline_zeeman.py's _run convention).

MEASURED on the CPU and written into the tests below: W's worst error and condition (test 2), the update's constants (test 3), the
remainders of the closed forms (test 8).
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
import test_sightline_zeeman as zt
import test_table_emission as tab
from test_sightlines import EPS, TINY, _assert_exact, gather, geometry

LIGHT, ISP, KL = gl.LIGHT, gl.ISP, zt.KL
SHAPE = gl.SHAPE
STOKES = zt.STOKES
WING = zt.WING
KF = ((1.602176634e-19 * 1.602176634e-19) * 1.602176634e-19) / ((((2.0 * 8.8541878128e-12) * 9.1093837015e-31) * 9.1093837015e-31) * LIGHT)
MEASURED_WORST_W = 1.59e-13  # L (and H: 1.57e-13) against wofz on the grid of test 2, relative to |w|
COND_W = 2.0                 # |dw / d ln a| / |w| on that grid is at most 1 (measured 1.000); held with a margin of 2
E_WW = MEASURED_WORST_W / EPS
THETA, ORDER = 0.25, 13
MEASURED_C = (4.0, 2.0, 4.2)  # the update against mpmath.expm on the grid of test 3: error <= (c0 + c1*s + c2*nrm*h) u
C0, C1, C2 = (4.0 * c for c in MEASURED_C)
_CACHE = {}

built, eng = gl.built, gl.eng


# ---------------------------------------------------------------- W(a, x) = (Re w, Im w), the header's algorithm
def _cf_w(a, x, K):
    Nr, Ni, Dr, Di = x.copy(), a.copy(), np.ones_like(x), np.zeros_like(x)
    for k in range(K, 0, -1):
        c = 0.5 * k
        tr = (Nr * x - Ni * a) - c * Dr
        ti = (Nr * a + Ni * x) - c * Di
        Dr, Di, Nr, Ni = Nr, Ni, tr, ti
    den = Nr * Nr + Ni * Ni
    return (ISP * (Dr * Ni - Di * Nr)) / den, (ISP * (Dr * Nr + Di * Ni)) / den


def _sampled_w(a, x, h, ih2, h2, Cn):
    n0 = 2.0 * np.rint(ih2 * x)
    xp = x - h * n0
    a2 = a * a
    g = np.exp(a2 - xp * xp)
    th = (2.0 * a) * xp
    Gr, Gi = g * np.cos(th), -(g * np.sin(th))
    pe = np.exp(h2 * xp)
    me = 1.0 / pe
    ca, sa = np.cos(h2 * a), np.sin(h2 * a)
    pr, pi, mr, mi = pe * ca, pe * sa, me * ca, -(me * sa)
    p2r, p2i = pr * pr - pi * pi, (2.0 * pr) * pi
    m2r, m2i = mr * mr - mi * mi, (2.0 * mr) * mi
    d0 = n0 * n0
    Sr, Si = np.zeros_like(x), np.zeros_like(x)
    for k, c in enumerate(Cn):
        n = 2 * k + 1
        q = c / (d0 - n * n)
        Sr = Sr + q * (pr * (n0 - n) + mr * (n0 + n))
        Si = Si + q * (pi * (n0 - n) + mi * (n0 + n))
        pr, pi = pr * p2r - pi * p2i, pr * p2i + pi * p2r
        mr, mi = mr * m2r - mi * m2i, mr * m2i + mi * m2r
    imF = (Gr * Si + Gi * Sr) * ISP
    reF = (Gr * Sr - Gi * Si) * ISP
    e, t2 = np.exp(a2 - x * x), (2.0 * a) * x
    return e * np.cos(t2) - (2.0 * ISP) * imF, (2.0 * ISP) * reF - e * np.sin(t2)


def voigt_w_restated(a, x):
    """(H, L, region): voigt_w of voigt_node.inc in float64; region indexes vt.REGIONS."""
    a, x = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(x, np.float64))
    H, L = np.empty(a.shape), np.empty(a.shape)
    with np.errstate(all="ignore"):
        z2 = x * x + a * a
        r0 = ~(z2 < 1e17)
        r1 = ~r0 & (z2 >= 100.0)
        r2 = ~r0 & ~r1 & (a >= 2.0)
        r3 = ~r0 & ~r1 & ~r2 & (a <= 0.5)
        r4 = ~(r0 | r1 | r2 | r3)
        H[r0], L[r0] = (ISP * a[r0]) / z2[r0], (ISP * x[r0]) / z2[r0]
        H[r1], L[r1] = _cf_w(a[r1], x[r1], 10)
        H[r2], L[r2] = _cf_w(a[r2], x[r2], 40)
        H[r3], L[r3] = _sampled_w(a[r3], x[r3], 0.25, 2.0, 0.5, vt.CA)
        H[r4], L[r4] = _sampled_w(a[r4], x[r4], 0.1875, 2.6666666666666665, 0.375, vt.CB)
    return H, L, r1 * 1 + r2 * 2 + r3 * 3 + r4 * 4


# ---------------------------------------------------------------- the update of one sample
def _row(A, i, v):
    return ((A[i][0] * v[0] + A[i][1] * v[1]) + A[i][2] * v[2]) + A[i][3] * v[3]


def cell_update(ac, Sc, j, hI, hq, r, h, X):
    """stokes_update of stokes_node.inc, elementwise on arrays of one shape.  j = (jI, jQ, jU, jV), hq = (hQ, hU, hV),
    r = (rQ, rU, rV), X = (I, Q, U, Vs).  Returns the new X (four arrays), s and nrm*h."""
    with np.errstate(all="ignore"):
        eI = ac + hI
        hQ, hU, hV = hq
        rQ, rU, rV = r
        K = [[eI, hQ, hU, hV], [hQ, eI, rV, -rU], [hU, -rV, eI, rQ], [hV, rU, -rQ, eI]]
        nrm = None
        for i in range(4):
            ri = ((np.abs(K[i][0]) + np.abs(K[i][1])) + np.abs(K[i][2])) + np.abs(K[i][3])
            nrm = ri if nrm is None else np.where(ri > nrm, ri, nrm)
        t = nrm * h
        t0 = t.copy()
        hs = np.broadcast_to(np.asarray(h, np.float64), t.shape).copy()
        s = np.zeros(t.shape, np.int64)
        live = t <= np.finfo(np.float64).max
        while True:
            m = live & (t > THETA)
            if not m.any():
                break
            t = np.where(m, 0.5 * t, t)
            hs = np.where(m, 0.5 * hs, hs)
            s += m
        g0, gQ, gU, gV = -(eI * hs), -(hQ * hs), -(hU * hs), -(hV * hs)
        fQ, fU, fV = -(rQ * hs), -(rU * hs), -(rV * hs)
        b = [(ac * Sc + j[0]) * hs, j[1] * hs, j[2] * hs, j[3] * hs]
        one, zero = np.ones(t.shape), np.zeros(t.shape)
        O = [[one if i == k else zero for k in range(4)] for i in range(4)]
        p = [zero, zero, zero, zero]
        for k in range(ORDER, 0, -1):
            c = float(k)
            a0, aQ, aU, aV, cQ, cU, cV = g0 / c, gQ / c, gU / c, gV / c, fQ / c, fU / c, fV / c
            A = [[a0, aQ, aU, aV], [aQ, a0, cV, -cU], [aU, -cV, a0, cQ], [aV, cU, -cQ, a0]]
            N = [[_row(A, i, [O[0][k2], O[1][k2], O[2][k2], O[3][k2]]) for k2 in range(4)] for i in range(4)]
            q = [_row(A, i, p) + b[i] / c for i in range(4)]
            O = [[1.0 + N[i][k2] if i == k2 else N[i][k2] for k2 in range(4)] for i in range(4)]
            p = q
        for m_ in range(int(s.max()) if s.size else 0):
            on = m_ < s
            q = [p[i] + _row(O, i, p) for i in range(4)]
            N = [[_row(O, i, [O[0][k2], O[1][k2], O[2][k2], O[3][k2]]) for k2 in range(4)] for i in range(4)]
            p = [np.where(on, q[i], p[i]) for i in range(4)]
            O = [[np.where(on, N[i][k2], O[i][k2]) for k2 in range(4)] for i in range(4)]
        Y = [_row(O, i, X) + p[i] for i in range(4)]
    return Y, s, t0


# ---------------------------------------------------------------- the restatement of the chord
def restate_stokes(F, co, o, d, ref, H, omegas, toward, step, max_steps, continuum, wing, backlight=None, pol=None, faraday=False):
    """include/synthray.h's rule for sr_field_sightline_stokes.  F: tests/test_sightline_lines.py's dict of fields plus B
    ((nx, ny, nz, 3)); ref: (3, N).  Returns I, Q, U, V, tau, the budgets b (for each of I, Q, U, V) and bt, (N, n_freq), column,
    chord, steps, miss (N), and the counters the companion test asks about."""
    from synthpy_amd import engine

    g = [np.float64(np.float32(a)) for a in co]
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    om, e_ph, c_om = engine.spectrum_constants(omegas)
    G = geometry(g, o, d, step, max_steps)
    hit, n, h = G["hit"], G["n"], G["h"]
    N, NF, NL = o.shape[1], len(om), len(H["w0"])
    cut = np.float64(wing) * np.float64(wing)
    fr = zt.frames(d, ref, toward)
    I0 = np.zeros((N, NF)) if backlight is None else np.array(backlight, np.float64)
    X = [I0.copy()] + [np.zeros((N, NF)) if pol is None else I0 * np.float64(pol[k]) for k in range(3)]
    tau, b, Bt, column = np.zeros((N, NF)), np.zeros((N, NF)), np.zeros((N, NF)), np.zeros(N)
    kF2 = 2.0 * KF
    with np.errstate(all="ignore"):
        su = toward / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    fields = [np.float64(F["ne"])] + [np.float64(F[k]) if np.ndim(F[k]) else float(F[k]) for k in ("Te", "Z")]
    has_ti, has_v = F.get("Ti") is not None, F.get("V") is not None
    if has_ti:
        fields.append(np.float64(F["Ti"]))
    if has_v:
        fields += [np.float64(F["V"][..., a]) for a in range(3)]
    fields += [np.float64(F["B"][..., a]) for a in range(3)]
    cnt = dict(shortcut=0, matrix=0, s5=0, smax=0, full=0, drop=np.zeros(N, np.int64), shist=np.zeros(64, np.int64), quiet_matrix=0)
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
            neh = ne_s * h
            column = np.where(act, column + neh, column)
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
            ni = (ne_s * 1e-6) / Z_s
            lt, ld = np.log(Te_s), np.log(ni)
            i, ft = tab._locate(H["LT"], lt)
            j, fd = tab._locate(H["LD"], ld)

            def E_l(Gs, l):
                return (Gs[0][l] * (2 + 2 * np.abs(ld) + 5 * H["dD_max"]) + Gs[1][l] * (2 * np.abs(lt) + 5 * H["dT_max"]) + 2 * Gs[2][l])

            col = lambda v: v[:, None]
            jS = [np.zeros((N, NF)) for _ in range(4)]
            hS = [np.zeros((N, NF)) for _ in range(4)]  # hI, hQ, hU, hV
            rS = [np.zeros((N, NF)) for _ in range(3)]  # rQ, rU, rV
            AJ, AK = np.zeros((N, NF)), np.zeros((N, NF))
            counted, nlc = np.zeros((N, NF), bool), np.zeros((N, NF))
            EJ, EK = np.zeros((N, NF)), np.zeros((N, NF))
            for l in range(NL):
                wc = H["w0"][l] * (1.0 + beta)
                wd = H["w0"][l] * (np.sqrt(H["ci"][l] * Ti_s) / LIGHT)
                iw = 1.0 / wd
                gg = ISP * iw
                aJ = np.exp(tab._interp(H["LJ"][l], i, j, ft, fd)) * gg
                if H["LG"] is not None:
                    av = np.exp(tab._interp(H["LG"][l], i, j, ft, fd)) * iw
                    Ea = E_l(H["GG"], l)[:, None] + 3
                else:
                    av, Ea = np.zeros(N), 0.0
                a64 = np.broadcast_to(av[:, None], (N, NF))
                P = {q: np.zeros((N, NF)) for q in (-1.0, 0.0, 1.0)}
                Rr = {q: np.zeros((N, NF)) for q in (-1.0, 0.0, 1.0)}
                Wa = np.zeros((N, NF))
                any_, nk = np.zeros((N, NF), bool), np.zeros((N, NF))
                for q, gk, sk in H["patterns"][l]:
                    sh = gk * wL
                    x = ((om[None, :] - wc[:, None]) - sh[:, None]) * iw[:, None]
                    x2 = x * x
                    keep = ~(x2 > cut) & live[:, None]
                    Hh, Ll = np.zeros((N, NF)), np.zeros((N, NF))
                    if keep.any():
                        Hh[keep], Ll[keep], _ = voigt_w_restated(a64[keep], x[keep])
                    P[q] = np.where(keep, P[q] + sk * Hh, P[q])
                    Rr[q] = np.where(keep, Rr[q] + sk * Ll, Rr[q])
                    Wa = np.where(keep, Wa + sk * np.sqrt(Hh * Hh + Ll * Ll), Wa)
                    any_ |= keep
                    nk += keep
                    cnt["drop"] += (live[:, None] & ~keep).sum(axis=1)
                Ps = P[1.0] + P[-1.0]
                eI = 0.5 * (col(sP) * P[0.0]) + (0.5 * col(cS)) * Ps
                eP = 0.5 * (P[0.0] - 0.5 * Ps)
                eV = 0.5 * (P[1.0] - P[-1.0])
                Rs = Rr[1.0] + Rr[-1.0]
                fP = 0.5 * (Rr[0.0] - 0.5 * Rs)
                fV = 0.5 * (Rr[1.0] - Rr[-1.0])
                aJc = aJ[:, None]
                if H["LK"] is not None:
                    aKc = (np.exp(tab._interp(H["LK"][l], i, j, ft, fd)) * gg)[:, None]
                else:
                    aKc = np.zeros((N, 1))
                add = lambda acc, v: np.where(any_, acc + v, acc)
                jS = [add(jS[0], aJc * eI), add(jS[1], aJc * (eP * col(cQ))), add(jS[2], aJc * (eP * col(cU))), add(jS[3], aJc * (eV * col(cV)))]
                hS = [add(hS[0], aKc * eI), add(hS[1], aKc * (eP * col(cQ))), add(hS[2], aKc * (eP * col(cU))), add(hS[3], aKc * (eV * col(cV)))]
                rS = [add(rS[0], aKc * (fP * col(cQ))), add(rS[1], aKc * (fP * col(cU))), add(rS[2], aKc * (fV * col(cV)))]
                AJ = np.where(any_, AJ + aJc * Wa, AJ)
                AK = np.where(any_, AK + aKc * Wa, AK)
                EP = E_WW + COND_W * Ea + 1 + nk
                EJ = np.where(any_, np.maximum(EJ, E_l(H["GJ"], l)[:, None] + EP), EJ)
                if H["LK"] is not None:
                    EK = np.where(any_, np.maximum(EK, E_l(H["GK"], l)[:, None] + EP), EK)
                counted |= any_
                nlc += any_
            Ej = np.where(counted, EJ + 8 + nlc, 0.0)
            Ek = np.where(counted & (H["LK"] is not None), EK + 8 + nlc, 0.0)
            rVf = np.zeros((N, NF))
            if faraday:
                rVf = ((kF2 * (neh / h))[:, None] * Bn[:, None]) / (om * om)[None, :]
                rS[2] = rS[2] + rVf
            if continuum:
                ac, Sc, xc = nrl._node(ne_s[:, None], Te_s[:, None], Z_s[:, None], om[None, :], e_ph[None, :], c_om[None, :])
                Eac, Esc = np.where(ac != 0, gl.E_AC, 0.0), np.where(ac != 0, 4 + xc, 0.0)
            else:
                ac, Sc, Eac, Esc = np.zeros((N, NF)), np.zeros((N, NF)), np.zeros((N, NF)), np.zeros((N, NF))
            act2 = act[:, None] & np.ones((1, NF), bool)
            hw = h[:, None]
            scalar = np.ones((N, NF), bool)
            for v in hS[1:] + rS:
                scalar &= v == 0.0
            # the matrix update
            Y, s_, t_ = cell_update(ac, Sc, jS, hS[0], hS[1:], rS, hw, X)
            # sr_field_sightline_zeeman's update
            d0 = ac * hw
            a0, F0 = np.exp(-d0), -np.expm1(-d0)
            a_ = ac + hS[0]
            d1 = a_ * hw
            a1, F1 = np.exp(-d1), -np.expm1(-d1)
            mat = act2 & ~scalar
            thin = act2 & scalar & counted & (d1 == 0)
            gen = act2 & scalar & counted & ~(d1 == 0)
            quiet = act2 & scalar & ~counted
            eps = [ac * Sc + jS[0], jS[1], jS[2], jS[3]]
            M = sum(np.abs(v) for v in X) + hw * sum(np.abs(v) for v in eps)
            new = []
            for k_ in range(4):
                src1 = (eps[0] / a_) * F1 if k_ == 0 else (jS[k_] / a_) * F1
                src0 = Sc * F0 if k_ == 0 else 0.0
                if continuum:
                    q_ = X[k_] * a0 + src0 if k_ == 0 else X[k_] * a0
                else:
                    q_ = X[k_] + 0.0
                new.append(np.where(mat, Y[k_], np.where(gen, X[k_] * a1 + src1, np.where(thin, X[k_] + jS[k_] * hw, np.where(quiet, q_, X[k_])))))
            dK = (Eac + 2) * ac + 4 * (Ek + 1) * AK + 6 * np.abs(rVf)
            de = (Eac + Esc + 2) * np.abs(ac * Sc) + 4 * (Ej + 1) * AJ
            s_eff = np.where(mat, s_, 0)
            nh = np.where(mat, t_, np.abs(d1))
            grow = hw * (dK * M + de) + (C0 + C1 * s_eff + C2 * nh) * M
            b = np.where(act2, b + grow, b)
            tau_new = np.where(mat | gen, tau + d1, np.where(thin, tau, np.where(quiet & continuum, tau + d0, np.where(quiet, tau + 0.0, tau))))
            Bt = np.where(act2, Bt + (Eac + 2) * d0 + (Ek + 2) * AK * hw, Bt)
            X, tau = new, tau_new
            cnt["shortcut"] += int((act2 & scalar).sum())
            cnt["matrix"] += int(mat.sum())
            cnt["quiet_matrix"] += int((mat & ~counted).sum())
            if mat.any():
                cnt["s5"] += int((s_[mat] >= 5).sum())
                cnt["smax"] = max(cnt["smax"], int(s_[mat].max()))
                cnt["shist"] += np.bincount(np.minimum(s_[mat], 63), minlength=64)
                eI_ = ac + hS[0]
                cnt["full"] += int((mat & (eI_ > 0) & (np.abs(np.abs(hS[3]) - eI_) <= 4 * EPS * eI_)).sum())
    floor = (4 * n * TINY)[:, None]
    out = dict(I=X[0], Q=X[1], U=X[2], V=X[3], tau=tau, column=column, chord=G["chord"], steps=n.astype(np.int32), miss=~hit, cnt=cnt, frames=fr)
    with np.errstate(all="ignore"):
        out["b"] = 2 * EPS * b + floor
        for k_ in STOKES:
            out["b" + k_] = out["b"]
        out["bt"] = EPS * (2 * Bt + 2 * n[:, None] * tau) + floor
    return out


# ---------------------------------------------------------------- inputs
def _mk(k, f64, toward, ti, v, lk, cont, far, lg, wing, nf, nl, pattern, pol, strength=1.0, view="six", te_f=True, z_f=True):
    return dict(k=k, f64=f64, toward=toward, ti=ti, v=v, lk=lk, cont=cont, far=far, lg=lg, wing=wing, nf=nf, nl=nl, pattern=pattern, pol=pol,
                strength=strength, view=view, te_f=te_f, z_f=z_f)


# float32 and float64 fields; with and without Ti, V, LG, LK; continuum and faraday on and off; toward = +-1; a finite wing; thin and
# thick tables; 70 frequencies (two tiles of 64 lanes) and 300 (two of 256)
CASES = (
    _mk(0, True, +1, True, True, True, True, True, True, np.inf, 70, 2, "mixed", (0.6, 0.3, -0.2)),
    _mk(1, False, -1, False, False, True, False, False, True, WING, 300, 3, "d2", None, strength=30.0),
    _mk(2, True, -1, True, False, False, True, True, False, np.inf, 70, 1, "triplet", (0.0, 0.0, 1.0)),
    _mk(3, False, +1, False, True, False, False, False, True, WING, 300, 2, "mixed", None),
    _mk(4, True, +1, True, True, True, False, True, False, WING, 70, 3, "mixed", (1.0, 0.0, 0.0), strength=100.0),
    _mk(5, False, -1, True, True, True, True, False, True, np.inf, 300, 1, "triplet", None, strength=10.0, view="pinhole"),
    _mk(6, True, -1, False, True, True, True, True, True, WING, 70, 3, "d2", (-0.5, 0.5, 0.5), strength=3.0, te_f=False, z_f=False),
    _mk(7, False, +1, True, False, True, False, True, False, np.inf, 70, 2, "triplet", (0.0, -1.0, 0.0), strength=300.0),
)


def _id(c):
    return (f"{c['k']}-{'f64' if c['f64'] else 'f32'}-{c['toward']:+d}-Ti{int(c['ti'])}-V{int(c['v'])}-LK{int(c['lk'])}-LG{int(c['lg'])}-cont{int(c['cont'])}"
            f"-far{int(c['far'])}-wing{c['wing']:g}-{c['nf']}f-{c['nl']}l-{c['pattern']}-x{c['strength']:g}-{c['view']}")


def _inputs(c, **over):
    c = dict(c, **over)
    R = zt._inputs(c)
    if c["strength"] != 1.0:
        R["lines"] = zt.make_zeeman(c["nl"], c["lk"], c["lg"], c["pattern"], strength=c["strength"])
    R["c"] = c
    return R


def _restate(R, **kw):
    c = R["c"]
    F = dict(R["F"], B=kw.pop("B", R["F"]["B"]))
    return restate_stokes(F, R["K"]["co"], R["o"], R["d"], kw.pop("refdir", R["refdir"]), zt.host_zeeman(kw.pop("lines", R["lines"])),
                          kw.pop("om", R["om"]), c["toward"], R["step"], R["max_steps"], c["cont"], c["wing"],
                          backlight=kw.pop("backlight", R["back"]), pol=kw.pop("pol", c["pol"]), faraday=kw.pop("faraday", c["far"]), **kw)


def _case(c):
    key = ("case", c["k"])
    if key not in _CACHE:
        R = _inputs(c)
        R["ref"] = _restate(R)
        _CACHE[key] = R
    return _CACHE[key]


def _aligned_case():
    """A uniform plasma with B exactly along the chord, Gaussian triplet, splitting 14 thermal widths, wing 6, a thick table: where
    only one sigma component reaches a frequency it is completely polarised, |hV| = eI to rounding and K is singular to rounding."""
    if "aligned" not in _CACHE:
        base = zt._uniform_inputs((1.0, 0.0, 0.0), np.zeros(1), lk=True)
        w0, wd = base["lines"].omega0[0], base["lines"].thermal_width(200.0)[0]
        om = w0 + wd * np.linspace(-21.0, 21.0, 70)
        R = zt._uniform_inputs((14.0 * wd / KL, 0.0, 0.0), om, lk=True)
        R["lines"] = _triplet(gl.make_lines(1, True, strength=100.0))
        R["c"] = dict(R["c"], wing=WING, pol=(0.3, -0.4, 0.5), far=False, strength=100.0, lk=True)
        R["back"] = np.full((1, len(om)), 1e-6)
        R["ref"] = _restate(R)
        _CACHE["aligned"] = R
    return _CACHE["aligned"]


def _triplet(base):
    from synthpy_amd.utils.eos_opacity import ZeemanLineTable, normal_triplet

    return ZeemanLineTable.from_lines(base, normal_triplet())


def _upload(eng, R, B="own"):
    return zt._upload(eng, R, B=B)


def _run(eng, R, fields=None, timed=True, **kw):
    """engine.sightline_stokes on freshly uploaded fields (unless given); I, Q, U, V, tau (n, n_freq) as the restatement's.  Cases of
    300 frequencies run on the 256-lane build (the module docstring)."""
    own = fields is None
    fields = _upload(eng, R) if own else fields
    c = R["c"]
    old = os.environ.get("SYNTHRAY_SPECTRA_FL")
    om = kw.pop("om", R["om"])
    if len(om) == 300:
        os.environ["SYNTHRAY_SPECTRA_FL"] = "256"
    try:
        call = kw.pop("call", eng.sightline_stokes)
        if call is eng.sightline_stokes:
            kw.setdefault("polarisation", c["pol"])
            kw.setdefault("faraday", c["far"])
        out = call(*fields, R["o"], R["d"], kw.pop("refdir", R["refdir"]), lines=kw.pop("lines", R["lines"]), omegas=om, continuum=c["cont"],
                   wing=c["wing"], toward=c["toward"], step=R["step"], max_steps=R["max_steps"], backlight=kw.pop("backlight", R["back"]), **kw)
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


def _assert_close(got, ref, what):
    return zt._assert_close(got, ref, what)


# ================================================================ CPU tests
def test_header_ctypes_and_python_signatures(built):
    """1a: the header's prototype, the ctypes binding, the chunk and its LDS bound, the Python signatures of every layer; the library
    exports the new symbols; the documents name the entry."""
    raw = open(os.path.join(ROOT, "include", "synthray.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+sr_field_sightline_stokes\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 28
    names = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["ne", "Te", "Ti", "Z", "V", "B", "lines", "p", "n", "origin", "dir", "ref", "n_freq", "omega", "e_ph", "c_omega", "backlight",
                     "pol", "faraday", "I", "Q", "U", "Vs", "tau", "column", "chord", "steps", "kernel_ms"]
    kinds = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]
    assert kinds[6] == "const sr_zeeman_table *" and kinds[7] == "const sr_voigt_params *" and kinds[17] == "const double *" and kinds[18] == "int32_t"
    res, args = built.SYMBOLS["sr_field_sightline_stokes"]
    assert res is C.c_int and len(args) == 28 and args[8] is C.c_int64 and args[12] is C.c_int32 and args[18] is C.c_int32
    assert args[:18] == built.SYMBOLS["sr_field_sightline_zeeman"][1][:17] + [C.c_void_p]
    assert hasattr(built.lib, "sr_field_sightline_stokes") and built.SYMBOLS["sr_stokes_chunk"] == (C.c_int, [])
    from synthpy_amd import engine, sightlines
    from synthpy_amd._domain import DomainExtras
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    chunk = built.lib.sr_stokes_chunk()
    assert built.STOKES_CHUNK == engine.STOKES_CHUNK == chunk and 2 * chunk <= 64
    # a staged sample: 18 + 6*n_line float64; two buffers and the lattices inside 64 KiB at 32 lines
    assert 2 * chunk * (18 + 6 * 32) * 8 + 8192 <= 64 * 1024
    assert engine.FARADAY == KF and abs(KF * (1.0 / (2 * np.pi * LIGHT)) ** 2 / 2.62e-13 - 1.00427) < 1e-5
    mk = open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()
    assert "sightline_stokes.hip" in mk and "stokes_node.inc" in mk and "-ffp-contract=off" in mk
    a, b, c = raw.index("/* ---- Zeeman-split lines along sightlines"), raw.index("/* ---- Polarised transfer along sightlines"), raw.index("/* ---- proton radiography")
    assert a < b < c
    mine = raw[b:c]
    for word in ("the rule is sr_field_sightline_zeeman's", "8.8541878128e-12", "theta = 1/4", "order 13", "B NULL", "Paschen-Back", "hyperfine",
                 "cyclotron dichroism", "scattering polarisation", "Hanle", "(ISP*x)/z2", "Dr*Nr + Di*Ni", "Gr*Sr - Gi*Si", "from e1 towards e2",
                 "1.6e-13"):
        assert word in mine, word
    assert "dichroism" not in mine.split("Not modelled:")[1].split("Arguments are checked")[0].replace("cyclotron dichroism", "")

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.sightline_stokes) == ["ne", "Te", "Ti", "Z", "V", "B", "origins", "directions", "reference", "lines", "omegas", "continuum",
                                              "wing", "toward", "step", "max_steps", "backlight", "polarisation", "faraday", "want"]
    par = inspect.signature(engine.sightline_stokes).parameters
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names(engine.sightline_stokes)[9:])
    assert par["wing"].default == np.inf and par["polarisation"].default is None and par["faraday"].default is False
    assert names(sightlines.sightline_stokes) == names(sightlines.sightline_zeeman) + ["polarisation", "faraday"]
    assert names(NewDomain.sightline_stokes) == names(OldDomain.sightline_stokes) == names(DomainExtras.sightline_zeeman) + ["polarisation", "faraday"]
    assert NewDomain.sightline_stokes is DomainExtras.sightline_stokes is OldDomain.sightline_stokes
    assert names(sightlines.StokesSpectra.polarisation_angle) == ["self"] and names(sightlines.StokesSpectra.degree) == ["self"]
    for doc in (engine.sightline_stokes.__doc__, sightlines.sightline_stokes.__doc__, DomainExtras.sightline_stokes.__doc__):
        for word in ("Paschen-Back", "hyperfine", "cyclotron dichroism", "scattering polarisation", "Hanle"):
            assert word in doc, word
    for name in ("README.md", "DESIGN.md", os.path.join("tools", "README.md")):
        assert "sightline_stokes" in open(os.path.join(ROOT, name)).read(), name
    # StokesSpectra's two read-outs by hand
    ch = sightlines.Chords(np.zeros((3, 1)), np.ones((3, 1)), +1)
    lines = zt.make_zeeman(1, True, True, "triplet")
    I, Q, U, V = np.array([[2.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]), np.array([[1.0, -0.5, 0.0]]), np.array([[0.0, 0.5, 0.0]])
    sp = sightlines.StokesSpectra(ch, I, np.zeros((1, 3)), np.zeros(1), np.zeros(1), np.zeros(1, np.int32), np.array([1.0, 2.0, 3.0]), lines, Q, U, V)
    assert np.allclose(sp.polarisation_angle(), [[np.pi / 8, -np.pi / 4, 0.0]], rtol=0, atol=1e-16)
    d = sp.degree()
    assert np.allclose(d[0, :2], [np.sqrt(0.5), np.sqrt(0.5)], rtol=1e-15) and np.isnan(d[0, 2])


def test_argument_checks_come_before_the_device(built):
    """1b: a rejected argument is SR_ERR_INVALID with a text that names sr_field_sightline_stokes, and the device is never
    initialised: the calls carry a B that is no field and NULL for the other fields, so a call that passes every other check ends at
    'NULL ne' (tests/test_sightline_zeeman.py's device)."""
    from synthpy_amd import engine, sightlines

    lib, ptr = built.lib, built.ptr
    o0, d0 = np.zeros((3, 2)), np.ones((3, 2))
    r0 = np.array([[0.0, 1.0], [1.0, 0.0], [0.0, 0.0]])
    out = [np.zeros((2, 5)) for _ in range(5)]
    om0, e0, c0 = engine.spectrum_constants(np.linspace(7.5e15, 7.6e15, 5))
    fakeB = C.c_void_p(C.addressof(C.create_string_buffer(256)))

    def params(wing=np.inf, toward=1, step=1e-4, max_steps=10, continuum=0):
        p = built.VoigtParams()
        p.march.toward, p.march.max_steps, p.march.continuum, p.march.step, p.wing = toward, max_steps, continuum, step, wing
        return p

    def table(pattern="mixed", lg=True):
        return engine.zeeman_table_params(zt.make_zeeman(3, True, lg, pattern))

    t0, keep0 = table()

    def call(p, n=2, o=o0, d=d0, r=r0, t=t0, nf=5, B=fakeB, pol=None, faraday=0, I=out[0], Q=out[1], U=out[2], V=out[3], tau=out[4]):
        pol = None if pol is None else np.array(pol, np.float64)
        return lib.sr_field_sightline_stokes(None, None, None, None, None, B, None if t is None else C.byref(t), None if p is None else C.byref(p), n,
                                             ptr(o), ptr(d), ptr(r), nf, ptr(om0), ptr(e0), ptr(c0), None, ptr(pol), faraday, ptr(I), ptr(Q), ptr(U),
                                             ptr(V), ptr(tau), None, None, None, None)

    def err(text, *a, **kw):
        assert call(*a, **kw) == -1, text
        msg = built.last_error()
        assert text in msg and "sr_field_sightline_stokes" in msg, (text, msg)

    # what this entry adds
    for pol in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)):
        err("non-finite pol", params(), pol=pol)
    for pol in ((1.0, 1e-5, 0.0), (0.6, 0.6, 0.6), (0.0, 0.0, -1.001)):
        err("outside the unit ball", params(), pol=pol)
    for far in (2, -1):
        err("faraday must be 0 or 1", params(), faraday=far)
    err("faraday needs B", params(), B=None, faraday=1)
    err("pol needs B", params(), B=None, pol=(0.0, 0.0, 0.0))
    for pol in ((1.0, 0.0, 0.0), (0.6, 0.8, 0.0), (0.0, 0.0, 0.0), (-0.5, 0.5, 0.5)):  # inside, or a unit vector as rounded
        err("NULL ne", params(), pol=pol, faraday=1)
    # everything sr_field_sightline_zeeman checks, under this entry's name
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
    t, keep = table()
    keep[-1][4, 0] = 0.5
    err("q of component 1 of line 1 must be -1, 0 or +1", params(), t=t)
    t, keep = table()
    keep[-1][0, 1] = np.nan
    err("non-finite g of component 0 of line 0", params(), t=t)
    t, keep = table()
    keep[-1][2, 2] = 0.0
    err("s of component 2 of line 0 must be finite and positive", params(), t=t)
    t, keep = table()
    keep[-1][3, 2] = 0.25 + 1e-8
    err("the strengths of the q = -1 group of line 1 sum to", params(), t=t)
    t, keep = table()
    keep[-2][2] = 25
    err("n_comp of line 2 must be 1..24", params(), t=t)
    r = r0.copy()
    r[2, 1] = np.nan
    err("non-finite ref of line 1", params(), r=r)
    r = r0.copy()
    r[:, 0] = (2.0, 2.0, 2.0 + 1e-6)
    err("ref of line 0 is parallel to the chord", params(), r=r)
    for wing in (np.nan, 0.0, -3.0):
        err("wing must be positive", params(wing=wing))
    err("toward", params(toward=0))
    err("step must be finite and positive", params(step=0.0))
    err("n x frequency tiles exceeds 2^31 - 1 workgroups", params(), n=2 ** 31)
    a = np.ones((3, 2))
    a[2, 1] = np.nan
    err("non-finite direction of line 1", params(), d=a)
    err("NULL ne", params())
    err("NULL ne", params(wing=WING, continuum=1), n=0)
    err("NULL ne", params(), nf=0)
    # B NULL: sr_field_sightline_voigt's checks under its own name
    t, keep = table()
    t.n_comp = t.comp = None
    assert call(params(), B=None, t=t, r=None, Q=None, U=None, V=None) == -1
    assert "NULL ne" in built.last_error() and "sr_field_sightline_voigt" in built.last_error()
    assert keep0 is not None
    with pytest.raises(ValueError, match="patterns"):
        sightlines.sightline_stokes(object(), sightlines.Chords(np.zeros((3, 1)), np.ones((3, 1)), -1), vt.make_voigt(1, True), wavelengths=[5e-7])
    with pytest.raises(ValueError, match="polarisation must be"):
        engine.sightline_stokes(None, 1.0, None, 1.0, None, None, o0, d0, None, lines=zt.make_zeeman(1, True, True, "triplet"), omegas=om0, toward=1,
                                step=1e-4, max_steps=5, polarisation=(1.0, 0.0))


def test_dispersion_profile_against_wofz(built):
    """2: L = Im w of the restatement against scipy.special.wofz(...).imag on the Voigt test's grid of (a, x), both signs of x, with
    every region boundary straddled; the error is taken relative to |w| (L is odd in x and cancels at the centre).  MEASURED worst:
    1.59e-13 (H on the same footing: 1.57e-13), at a just under 2; the bound held is 8 x that, the Thomson test's margin.  H from
    voigt_w equals voigt_restated bit for bit.  |dw / d ln a| / |w| <= 1 (measured 1.000000007), which COND_W = 2 covers."""
    from scipy.special import wofz

    worst_l = worst_h = cond = 0.0
    seen = set()
    for a, x in vt.accuracy_grid():
        assert np.any(x < 0) and np.any(x > 0)
        ref = wofz(x + 1j * a)
        H, L, reg = voigt_w_restated(a, x)
        Hv, regv = vt.voigt_restated(a, x)
        assert np.array_equal(H, Hv) and np.array_equal(reg, regv) and np.all(np.isfinite(L))
        aw = np.abs(ref)
        worst_l, worst_h = max(worst_l, float(np.max(np.abs(L - ref.imag) / aw))), max(worst_h, float(np.max(np.abs(H - ref.real) / aw)))
        seen |= set(reg.tolist())
        da = a * 1e-4
        cond = max(cond, float(np.max(np.abs(wofz(x + 1j * (a + da)) - wofz(x + 1j * (a - da))) / aw / np.log((a + da) / (a - da)))))
    print(f"L against wofz.imag: worst error relative to |w| {worst_l:.3e} (H: {worst_h:.3e}; bound {8 * MEASURED_WORST_W:.2e}); |dw/dlna|/|w| <= {cond:.9f}")
    assert seen == {0, 1, 2, 3, 4}
    assert worst_l <= 8 * MEASURED_WORST_W and worst_h <= 8 * MEASURED_WORST_W
    assert cond <= COND_W
    # odd in x bit for bit, exactly 0 at the centre in every region, a NaN stays a NaN; at an infinite x the asymptote's L is inf/inf, a NaN (H is 0)
    H, L, _ = voigt_w_restated([0.3, 0.3, 1.0, 3.0, 20.0, np.nan, 1.0, 1.0], [1.7, -1.7, 0.0, 0.0, 0.0, 1.0, np.nan, np.inf])
    assert L[0] == -L[1] and L[0] > 0 and not np.any(L[2:5]) and np.isnan(L[5]) and np.isnan(L[6]) and np.isnan(L[7]) and H[7] == 0.0


def _update_grid():
    """The stated grid of test 3: (eI*h, eta*h, rho*h)."""
    rng = np.random.default_rng(7)
    unit = lambda v: np.asarray(v, np.float64) / np.linalg.norm(v)
    out = []
    for eh in (1e-6, 1e-4, 1e-2, 0.1, 0.25, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0, 1e3):
        for deg in (0.0, 0.5, 1 - 1e-14, 1.0):
            for rr in (0.0, 0.3, 1.0, 3.0, 30.0):
                for geom in ("par", "perp", "rand"):
                    e = unit(rng.normal(size=3)) if geom != "par" else unit([0.3, -0.5, 0.8])
                    rdir = e if geom == "par" else unit(np.cross(e, rng.normal(size=3))) if geom == "perp" else unit(rng.normal(size=3))
                    out.append((eh, deg * eh * e, rr * eh * rdir))
        for deg in (0.5, 1.0):  # the degenerate case of the closed form: |eta| = |rho|, eta . rho = 0
            e = unit(rng.normal(size=3))
            out.append((eh, deg * eh * e, deg * eh * unit(np.cross(e, rng.normal(size=3)))))
        out.append((eh, np.array([0.0, 0.0, eh]), np.array([eh, 0.0, 0.0])))  # exactly orthogonal, exactly equal, completely dichroic
    for rh in (1e-3, 0.2, 1.0, 10.0, 100.0, 1e3):  # rotation alone: modes that do not decay
        out.append((0.0, np.zeros(3), np.array([0.0, 0.0, rh])))
        out.append((0.0, np.zeros(3), rh * unit([1.0, 2.0, -1.5])))
    return out


def test_cell_update_against_mpmath_expm(built):
    """3: the update restated in NumPy against mpmath.expm of the 5 x 5 augmented matrix [[-K h, eps h], [0, 0]] at 50 digits, on
    _update_grid(): eI*h from 1e-6 to 1e3, degree of dichroism 0, 0.5, 1 - 1e-14 and exactly 1, |rho|/eI from 0 to 30 (parallel,
    perpendicular and oblique to eta), the degenerate case |eta| = |rho| with eta . rho = 0, and pure rotations; the vector and the
    source drawn inside the cone, the source once near LTE and once free.  The error of the 2-norm relative to max(|X|, |p|) is held
    under (C0 + C1*s + C2*nrm*h) u with (C0, C1, C2) = 4 x MEASURED_C.  MEASURED (this grid, two draws per point): at most 2.9 u where
    s = 0; (4 + 2*s + 4.2*nrm*h) u covers every point, the last constant set by modes that do not decay (complete dichroism, pure
    rotation), where an error of u in K h is an error of u*nrm*h in exp: 29 430 u at eI*h = 1e3 with |rho| = 30 eI (nrm*h = 4.1e4)."""
    import mpmath

    rng = np.random.default_rng(11)
    unit = lambda v: v / np.linalg.norm(v)
    arr = lambda v: np.array([v], np.float64)
    worst, need, smax = 0.0, 0.0, 0
    with mpmath.workdps(50):
        m = mpmath.mpf
        for eh, eta, rho in _update_grid():
            for trial in range(2):
                X = np.array([1.0, *(rng.uniform(0, 1) * unit(rng.normal(size=3)))]) * 10 ** rng.uniform(-3, 3)
                if trial == 0:
                    eps = 10 ** rng.uniform(-2, 2) * np.array([eh, *eta]) * (1 + 0.3 * rng.uniform(-1, 1, 4))
                else:
                    eps = np.array([1.0, *(rng.uniform(0, 1) * unit(rng.normal(size=3)))]) * max(eh, 1e-3) * 10 ** rng.uniform(-2, 2)
                Y, s, t = cell_update(arr(0.0), arr(0.0), [arr(v) for v in eps], arr(eh), [arr(v) for v in eta], [arr(v) for v in rho], 1.0,
                                      [arr(v) for v in X])
                Y, s, t = np.array([y[0] for y in Y]), int(s[0]), float(t[0])
                assert s == max(0, int(np.ceil(np.log2(t / THETA)))) if t > 0 else s == 0
                (hQ, hU, hV), (rQ, rU, rV), eI = (m(float(v)) for v in eta), (m(float(v)) for v in rho), m(float(eh))
                K = [[eI, hQ, hU, hV], [hQ, eI, rV, -rU], [hU, -rV, eI, rQ], [hV, rU, -rQ, eI]]
                M = mpmath.zeros(5)
                for i in range(4):
                    for k in range(4):
                        M[i, k] = -K[i][k]
                    M[i, 4] = m(float(eps[i]))
                E = mpmath.expm(M)
                p = [E[i, 4] for i in range(4)]
                exact = [sum(E[i, k] * m(float(X[k])) for k in range(4)) + p[i] for i in range(4)]
                err = float(mpmath.sqrt(sum((m(float(Y[i])) - exact[i]) ** 2 for i in range(4))))
                scale = max(float(np.linalg.norm(X)), float(mpmath.sqrt(sum(v * v for v in p))))
                eu = err / scale / EPS
                worst, smax = max(worst, eu), max(smax, s)
                need = max(need, eu / (C0 + C1 * s + C2 * t))
                assert eu <= C0 + C1 * s + C2 * t, (eh, eta, rho, s, t, eu)
    print(f"update against mpmath.expm: worst error {worst:.1f} u, largest s {smax}, worst share of (C0 + C1 s + C2 nrm h) used {need:.3f}")
    assert smax >= 17 and need <= 0.25 + 1e-9  # the margin of 4 is there


def test_tested_inputs_meet_the_conditions(built):
    """4: from the restatement's counters: the GPU cases contain samples with s >= 5, samples on the scalar shortcut, samples that
    only rotate (no line term counted), samples with |hV| = eI to rounding, dropped components, chords that miss the box, and chords
    with fewer and with more samples than sr_stokes_chunk(); every (chord, frequency) pair of every case is compared (no mask)."""
    chunk = built.STOKES_CHUNK
    tot = dict(shortcut=0, matrix=0, s5=0, full=0, quiet_matrix=0, drop=0, miss=0, below=0, above=0)
    for R in [_case(c) for c in CASES] + [_aligned_case()]:
        ref, cn = R["ref"], R["ref"]["cnt"]
        for k in ("shortcut", "matrix", "s5", "full", "quiet_matrix"):
            tot[k] += cn[k]
        tot["drop"] += int(cn["drop"].sum())
        tot["miss"] += int(ref["miss"].sum())
        hit = ref["steps"][~ref["miss"]]
        tot["below"] += int((hit < chunk).sum())
        tot["above"] += int((hit > chunk).sum())
        assert R["max_steps"] > chunk or R is _CACHE.get("aligned")
        for k in STOKES + ("tau", "b", "bt"):
            assert ref[k].shape == (R["o"].shape[1], len(R["om"])) and np.all(np.isfinite(ref[k])), k
        assert np.all(ref["b"][~ref["miss"]] > 0)
    print("conditions met by the GPU cases:", tot)
    assert all(v > 0 for v in tot.values()), tot
    c3 = _case(CASES[3])["ref"]["cnt"]
    assert c3["matrix"] == 0 and c3["shortcut"] > 0  # LK NULL, faraday off: every sample on the shortcut
    assert {c["nf"] for c in CASES} == {70, 300} and {c["f64"] for c in CASES} == {True, False} and {c["toward"] for c in CASES} == {1, -1}
    for key in ("ti", "v", "lk", "lg", "cont", "far"):
        assert {c[key] for c in CASES} == {True, False}, key
    assert any(np.isfinite(c["wing"]) for c in CASES)


# ================================================================ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES + ("aligned",), ids=lambda c: c if isinstance(c, str) else _id(c))
def test_kernel_against_restatement(eng, c):
    """5: chord, steps, column and the missed chords bit-equal, the NaN sets equal (none), I, Q, U, Vs and tau within the budgets of
    the module docstring, over every chord and frequency; a chord that misses the box returns the march's start; 8(v): the cone."""
    R = _aligned_case() if isinstance(c, str) else _case(c)
    what = c if isinstance(c, str) else _id(c)
    got = _run(eng, R)
    _assert_exact(got, R["ref"], what)
    _assert_close(got, R["ref"], what)
    zt._assert_cone(got, R["ref"], what)
    miss, pol = R["ref"]["miss"], R["c"]["pol"]
    assert np.array_equal(got["I"][miss], R["back"][miss]) and not np.any(got["tau"][miss])
    for k, name in enumerate("QUV"):
        assert np.array_equal(got[name][miss], R["back"][miss] * pol[k] if pol is not None else np.zeros_like(got[name][miss])), name


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 1, 5])
def test_bits_of_the_siblings_and_of_a_repeat(eng, k):
    """6: LK NULL with faraday off (and an unpolarised backlight) equals engine.sightline_zeeman bit for bit in all five maps (and
    column, chord, steps) -- case 3 as it is, the others with their table's absorption taken out; B = None equals
    engine.sightline_voigt, with exact zeros in Q, U, V; a repeated call returns identical bits."""
    R = _case(CASES[k])
    c = R["c"]
    lines = R["lines"] if not c["lk"] else zt.make_zeeman(c["nl"], False, c["lg"], c["pattern"], strength=c["strength"])
    fields = _upload(eng, R)
    try:
        old = _run(eng, R, fields=fields, call=eng.sightline_zeeman, lines=lines)
        new = _run(eng, R, fields=fields, lines=lines, polarisation=None, faraday=False)
        assert list(new) == list(old)
        for name in old:
            assert new[name].dtype == old[name].dtype and np.array_equal(new[name], old[name], equal_nan=True), name
        assert np.any(old["Q"] != 0) and np.any(old["V"] != 0)
        full, again = _run(eng, R, fields=fields), _run(eng, R, fields=fields)
        for name in full:
            assert np.array_equal(full[name], again[name], equal_nan=True), name
        if c["lg"]:
            kw = dict(lines=R["lines"], omegas=R["om"], continuum=c["cont"], wing=c["wing"], toward=c["toward"], step=R["step"],
                      max_steps=R["max_steps"], backlight=R["back"])
            if len(R["om"]) == 300:
                os.environ["SYNTHRAY_SPECTRA_FL"] = "256"
            try:
                voigt = eng.sightline_voigt(*fields[:5], R["o"], R["d"], **kw)
                none = eng.sightline_stokes(*fields[:5], None, R["o"], R["d"], None, **kw)
            finally:
                os.environ.pop("SYNTHRAY_SPECTRA_FL", None)
            assert list(none) == list(voigt) + ["Q", "U", "V"]
            for name in voigt:
                assert np.array_equal(none[name], voigt[name], equal_nan=True), name
            for name in "QUV":
                assert none[name].shape == voigt["intensity"].shape and not np.any(none[name]) and not np.any(np.signbit(none[name])), name
            with pytest.raises(Exception, match="faraday needs B"):
                eng.sightline_stokes(*fields[:5], None, R["o"], R["d"], None, faraday=True, **kw)
    finally:
        gl._close(fields)


@pytest.mark.gpu
@pytest.mark.parametrize("fl", [64, 256])
@pytest.mark.parametrize("which", range(5))
def test_chunk_boundaries_of_the_sample_staging(eng, fl, which):
    """7: chords of chunk - 1, chunk, chunk + 1, 2*chunk and 2*chunk + 1 samples at both lane widths (70 frequencies: the 64-lane
    build; 300 with the override: the 256-lane build), with absorption, faraday and a polarised backlight, against the restatement."""
    chunk = eng.STOKES_CHUNK
    N = [chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1][which]
    R = zt._chunk_case(fl, N, chunk)
    R["c"] = dict(R["c"], pol=(0.2, -0.7, 0.4), far=True, strength=1.0)
    ref = _restate(R)
    assert ref["steps"].tolist() == [N] * 3 and ref["cnt"]["matrix"] > 0
    got = _run(eng, R)
    _assert_exact(got, ref, f"{N} samples, tiles of {fl}")
    _assert_close(got, ref, f"{N} samples, tiles of {fl}")
    zt._assert_cone(got, ref, f"{N} samples, tiles of {fl}")


def _uniform(Bvec, om, strength, *, lk=True, wing=np.inf, pol=None, far=False, back=None, cont=False, toward=+1, lte=False, Te=25.0):
    """tests/test_sightline_zeeman.py's uniform plasma (ne = 2e24, Z = 2, Ti = 200, one chord along +x, e1 = y, e2 = z; a Gaussian
    normal triplet) with this entry's options; lte: the table's absorption is its emissivity over the Planck function."""
    R = zt._uniform_inputs(Bvec, om, toward=toward, lk=lk)
    base = gl.make_lines(1, lk, strength=strength)
    R["lines"] = _triplet(base.with_lte_absorption() if lte else base)
    R["F"] = dict(R["F"], Te=np.full(SHAPE, Te))
    R["c"] = dict(R["c"], wing=wing, pol=pol, far=far, cont=cont, strength=strength, lk=lk)
    R["back"] = None if back is None else np.full((1, len(om)), float(back))
    return R


@pytest.mark.gpu
def test_faraday_rotation_alone(eng):
    """8(i): no line reaches (wing 6, the frequencies 0.02 to 0.5 of the line's), continuum off, polarisation (1, 0, 0): I is
    unchanged bit for bit, and Q + iU = I0 exp(i rV L) with rV L / 2 = kF ne (B.n^) L / omega^2, from e1 towards e2 for B along the
    light's travel; the sense reverses with B, and with toward.  The uniform plasma has no quadrature remainder: what is left is
    rounding, the budget and 16 u (1 + 2 phi) for the closed form's own operations.  The angle equals the tracer's rotation map
    (line_integrals().rotation) on an axis-parallel chord after scaling by kF lambda^2 / (4 pi^2 c^2) / (2.62e-13 lambda^2) =
    1.00427: the tracer's rounded constant is 0.43 % low."""
    w0 = zt._uniform_inputs((1.0, 0.0, 0.0), np.zeros(1))["lines"].omega0[0]
    om = w0 * np.array([0.02, 0.05, 0.1, 0.5])
    Bx = 50.0
    angles = {}
    for sign, toward in ((+1, +1), (-1, +1), (+1, -1)):
        R = _uniform((sign * Bx, 3.0, -4.0), om, 1.0, wing=WING, pol=(1.0, 0.0, 0.0), far=True, back=1e-6, toward=toward)
        got, ref = _run(eng, R), _restate(R)
        assert ref["cnt"]["quiet_matrix"] == ref["cnt"]["matrix"] > 0 and ref["cnt"]["shortcut"] == 0
        _assert_close(got, ref, f"faraday alone, B {sign:+d}, toward {toward:+d}")
        L = float(got["chord"][0])
        phi = KF * 2e24 * (sign * Bx * toward) * L / om ** 2  # B.n^ = Bx*toward: the light travels along toward*x
        assert np.array_equal(got["I"][0], R["back"][0]) and not np.any(got["V"]) and not np.any(got["tau"])
        lim = ref["b"][0] + 16 * EPS * (1 + 2 * np.abs(phi)) * 1e-6
        assert np.all(np.abs(got["Q"][0] - 1e-6 * np.cos(2 * phi)) <= lim) and np.all(np.abs(got["U"][0] - 1e-6 * np.sin(2 * phi)) <= lim)
        assert np.all(np.sign(got["U"][0][-1:]) == sign * toward) and abs(phi[0]) > 1.0 and abs(phi[-1]) < 0.1
        angles[(sign, toward)] = phi
    assert np.array_equal(angles[(1, 1)], -angles[(-1, 1)])
    # the tracer's rotation map of the same plasma, along x
    from synthpy_amd import sightlines
    from synthpy_amd.simulator.domain import ScalarDomain

    dims, lengths, lam = (11, 6, 5), (4e-3, 2e-3, 2e-3), 532e-9
    dom = ScalarDomain(lengths, dims, B_on=True, probing_direction="x", auto_batching=False)
    B = np.zeros(dims + (3,))
    B[..., 0], B[..., 1] = 20.0, 7.0
    dom.external_ne(np.full(dims, 3e25)), dom.external_Te(30.0), dom.external_Z(2.0), dom.external_B(B)
    rot = dom.line_integrals(lwl=lam).rotation
    assert rot.shape == dims[1:] and np.all(rot > 0)
    ch = sightlines.Chords([[-1.0], [float(dom.y[2])], [float(dom.z[1])]], [[1.0], [0.0], [0.0]], +1, backlight=1.0)
    lines = _triplet(gl.make_lines(1, True))
    sp = dom.sightline_stokes(ch, lines, wavelengths=[lam], wing=WING, step=lengths[0] / 40, max_steps=100, reference=(0.0, 1.0, 0.0),
                              polarisation=(1.0, 0.0, 0.0), faraday=True)
    ratio = KF * lam ** 2 / (4 * np.pi ** 2 * LIGHT ** 2) / (2.62e-13 * lam ** 2)
    print(f"rotation: sightline_stokes {sp.polarisation_angle()[0, 0]:.9e} rad, tracer {rot[2, 1]:.9e} rad, ratio {sp.polarisation_angle()[0, 0] / rot[2, 1]:.6f} (constants: {ratio:.6f})")
    assert abs(ratio - 1.00427) < 1e-5
    # float32 volumes on the tracer's side (2^-24 each for ne and B) and 40 samples against 10 cells of a uniform plasma: 1e-6
    assert abs(sp.polarisation_angle()[0, 0] / (rot[2, 1] * ratio) - 1.0) < 1e-6 and sp.degree()[0, 0] == pytest.approx(1.0, abs=1e-12)


@pytest.mark.gpu
def test_lte_and_thin_absorption(eng):
    """8(ii): one line with aJ = S aK (with_lte_absorption; Te on a node of the table's lattice, so that S is the Planck function
    there) plus the continuum, whose source function Sc(omega) is the same Planck function up to its variation over +-12 thermal
    widths (MEASURED on the restatement: |Sc/S - 1| <= 3.96e-3; held: 8e-3): a backlight S stays (S, 0, 0, 0) at every thickness
    (strength 1e-3 to 1e3), and no backlight saturates to it where every mode is thick (a splitting of half a width keeps
    |eta| <= eI/2, so the slowest mode has at least tau/2 > 40) -- within the budget plus that variation, for I (a convex
    combination of S and Sc) and for Q, U, V (driven by ac*(Sc - S) alone).
    8(iii): thin absorption of an unpolarised backlight: (X(I0) - X(0))/I0 = -(hQ, hU, hV) L to first order, the opposite signs to
    the emission case, (jQ, jU, jV) L = X(0) to first order, with h = j aK/aJ = j/S.  In LTE the two sides are tied exactly, not
    only to first order, (X(I0) - X(0))/I0 = -X(0)/S (MEASURED on the restatement: they differ by 4.4e-15 of the signal), and
    -hV L and -hQ L themselves, from Gaussians worked out here by hand, are met within the second-order remainder -- every entry of
    (K L)^2 / 2 is at most (nrm L)^2 / 2 <= 8 tau_max^2, nrm <= 4 eI being K's row-sum norm (tau_max = 3.3e-6; MEASURED: 0.59
    tau_max^2) -- the hand formula's own rounding (x up to 15 widths: 1e-9 of the signal) and the budgets."""
    probe = _uniform((1.0, 0.0, 0.0), np.zeros(1), 1.0, lte=True)
    H = zt.host_zeeman(probe["lines"])
    Te = float(np.exp(H["LT"][2]))
    w0, wd = probe["lines"].omega0[0], probe["lines"].thermal_width(200.0)[0]
    om = w0 + wd * np.linspace(-12.0, 12.0, 70)
    Bvec = np.array([0.5, -0.6, 0.62]) * (3.0 * wd / KL)
    i, ft = tab._locate(H["LT"], np.log(Te))
    j, fd = tab._locate(H["LD"], np.log(2e24 * 1e-6 / 2.0))
    S = float(np.exp(tab._interp(H["LJ"][0], i, j, ft, fd) - tab._interp(H["LK"][0], i, j, ft, fd)))
    from synthpy_amd import engine

    _, e_ph, c_om = engine.spectrum_constants(om)
    _, Sc, _ = nrl._node(np.float64(2e24), np.float64(Te), np.float64(2.0), om, e_ph, c_om)
    var = float(np.max(np.abs(Sc / S - 1.0)))
    print(f"LTE: S = {S:.6e}, |Sc/S - 1| <= {var:.3e}")
    assert var <= 8e-3
    for strength in (1e-3, 1.0, 30.0, 1e3):
        R = _uniform(Bvec, om, strength, cont=True, lte=True, back=S, Te=Te, pol=None)
        got, ref = _run(eng, R), _restate(R)
        _assert_close(got, ref, f"LTE, backlight S, strength {strength:g}")
        lim = ref["b"][0] + var * S
        assert np.all(np.abs(got["I"][0] - S) <= lim) and all(np.all(np.abs(got[k][0]) <= lim) for k in "QUV"), strength
    R = _uniform(Bvec / 6.0, om, 1e3, cont=True, lte=True, back=None, Te=Te)
    got, ref = _run(eng, R), _restate(R)
    _assert_close(got, ref, "LTE, no backlight, thick")
    thick = got["tau"][0] > 80.0
    assert thick.sum() >= 10 and np.all(np.abs(got["I"][0][thick] - S) <= ref["b"][0][thick] + var * S)
    assert all(np.all(np.abs(got[k][0][thick]) <= ref["b"][0][thick] + var * S) for k in "QUV")
    # (iii)
    I0 = 1e3 * S
    runs = {}
    for back in (None, I0):
        R = _uniform(Bvec, om, 1e-6, lte=True, back=back, Te=Te)
        H1 = zt.host_zeeman(R["lines"])
        runs[back], ref = _run(eng, R), _restate(R)
        _assert_close(runs[back], ref, f"thin, backlight {back}")
        runs[back]["b"] = ref["b"]
    em, ab = runs[None], runs[I0]
    tau_max = float(ab["tau"].max())
    assert 0 < tau_max < 1e-5
    worst = 0.0
    for k in "QUV":
        signal = (ab[k][0] - em[k][0]) / I0
        want = -em[k][0] / S
        lim = 2 * tau_max * np.abs(want) + (ab["b"][0] + em["b"][0]) / I0 + em["b"][0] / S
        assert np.all(np.abs(signal - want) <= lim), k
        worst = max(worst, float(np.max(np.abs(signal - want)) / np.max(np.abs(want))))
        big = np.abs(want) > 0.05 * np.abs(want).max()
        assert big.sum() > 5 and np.all(np.sign(signal[big]) == -np.sign(em[k][0][big])), k
    # -hV L and -hQ L by hand: n^ = x, e1 = y, e2 = z
    aK = float(np.exp(tab._interp(H1["LK"][0], i, j, ft, fd))) * ISP / wd
    Bm = float(np.linalg.norm(Bvec))
    P = {q: np.exp(-(((om - w0) - q * KL * Bm) / wd) ** 2) for q in (-1, 0, 1)}
    L = float(ab["chord"][0])
    byhand = {"V": aK * 0.5 * (P[1] - P[-1]) * (Bvec[0] / Bm), "Q": aK * 0.5 * (P[0] - 0.5 * (P[1] + P[-1])) * ((Bvec[1] ** 2 - Bvec[2] ** 2) / Bm ** 2)}
    second = 0.0
    for k, hk in byhand.items():
        signal, want = (ab[k][0] - em[k][0]) / I0, -hk * L
        lim = 8 * tau_max ** 2 + 1e-9 * np.max(np.abs(want)) + (ab["b"][0] + em["b"][0]) / I0
        assert np.all(np.abs(signal - want) <= lim), k
        second = max(second, float(np.max(np.abs(signal - want))) / tau_max ** 2)
    print(f"thin absorption against -h L by hand: remainder {second:.3f} tau_max^2")
    print(f"thin absorption: tau_max {tau_max:.3e}, worst |signal - first order| / max|first order| {worst:.3e}")


@pytest.mark.gpu
def test_sign_anchor_far_to_the_blue(eng):
    """8(iv): anchor (b).  Far to the blue of a normal triplet (8 to 20 thermal widths above the centre, Gaussian components: the
    absorption there is below exp(-36) of the centre's, the dispersion profile falls as 1/x), faraday off, B along the light: a
    backlight polarised along e1 comes out turned from e1 towards e2 (U > 0 for Q > 0), the sense of the continuum's Faraday
    rotation for the same B, and the other way for B reversed; far to the red the sense is the same (rV is even about the centre:
    the Macaluso-Corbino rotation).  The angles run from 0.42 rad at 8 widths to 0.06 rad at 20 (MEASURED on the restatement)."""
    probe = _uniform((1.0, 0.0, 0.0), np.zeros(1), 1.0)
    w0, wd = probe["lines"].omega0[0], probe["lines"].thermal_width(200.0)[0]
    off = np.linspace(8.0, 20.0, 35)
    om = w0 + wd * np.concatenate([off, -off])
    for sign in (+1, -1):
        R = _uniform((sign * 2.0 * wd / KL, 0.0, 0.0), om, 10.0, pol=(1.0, 0.0, 0.0), back=1e-6)
        got, ref = _run(eng, R), _restate(R)
        _assert_close(got, ref, f"anchor (b), B {sign:+d}")
        ang = 0.5 * np.arctan2(got["U"][0], got["Q"][0])
        assert np.all(np.abs(ang) > 100 * ref["b"][0] / 1e-6) and np.all(np.abs(ang) < 0.7)
        assert np.all(np.sign(ang) == sign) and 0.3 < abs(ang[0]) < 0.5 and 0.04 < abs(ang[34]) < 0.08
        far = _uniform((sign * 2.0 * wd / KL, 0.0, 0.0), om[:35], 10.0, wing=WING, far=True, pol=(1.0, 0.0, 0.0), back=1e-6)
        assert np.all(np.sign(_run(eng, far)["U"][0]) == sign)


def _reversing_domain(Domain):
    """A slab whose field along z reverses along x, Bz = B0 tanh(x / 0.4 mm), cold and dense enough to absorb, not to emit."""
    dims, cell = (16, 12, 10), 2.5e-4
    lengths = tuple(cell * (m - 1) for m in dims)
    if isinstance(Domain, type) and Domain.__module__.endswith("simulator.domain"):
        dom = Domain(lengths, dims)
    else:
        dom = Domain(*[np.linspace(-L / 2, L / 2, m) for L, m in zip(lengths, dims)], lengths[2] / 2)
    x = np.linspace(-lengths[0] / 2, lengths[0] / 2, dims[0])
    B = np.zeros(dims + (3,), np.float32)
    B[..., 2] = (30.0 * np.tanh(x / 4e-4))[:, None, None]
    B[..., 1] = 4.0
    rng = np.random.default_rng(8)
    dom.external_ne(np.float32(10.0 ** rng.uniform(23.8, 24.2, dims)))
    dom.external_Te(30.0)
    dom.external_Z(2.0)
    dom.external_Ti(np.float32(rng.uniform(30.0, 50.0, dims)))
    dom.external_B(B)
    return dom, lengths


def _backlit(dom, lengths, lines, om, **kw):
    from synthpy_amd import sightlines

    from synthpy_amd import engine

    _, e_ph, c_om = engine.spectrum_constants(lines.omega0[:1])
    I0 = 1e4 * float(c_om[0] / np.expm1(e_ph[0] / 30.0))  # 1e4 Planck functions of the plasma's 30 eV: its emission is 1e-4 of the signal
    view = sightlines.PointBacklighter((1e-4, -2e-4, -40e-3), (0.0, 0.0, 1.0), (0, 1, 0), 80e-3, (8, 8), 0.6e-3, radiance=I0)
    return view, I0, dom.sightline_stokes(view, lines, wavelengths=2 * np.pi * LIGHT / om, wing=8.0, step=2.5e-4, max_steps=60, **kw)


def _absorbing_lines():
    from synthpy_amd.utils.eos_opacity import LineTable, VoigtLineTable, ZeemanLineTable, normal_triplet

    base = LineTable([1.0, 500.0], [1e17, 1e21], np.full((2, 2), 4.0e8), wavelengths=250e-9, mass_number=12.011)
    return ZeemanLineTable.from_lines(VoigtLineTable.power_law(base, 3e11, 1e24, zbar=2.0).with_lte_absorption(), [normal_triplet()])


@pytest.mark.gpu
def test_backlit_view_reads_the_reversing_field(eng):
    """9: a PointBacklighter, 8 x 8 pixels, through a field whose component along the view reverses along x.  b_parallel() of the
    absorption spectrum -- what the plasma took out of the backlight, (I0 - I, -Q, -U, -V) -- has the sign of B.n^ on every pixel
    and, the line being thin, the size of the column-weighted B.n^ within 20 %; sightline_zeeman, whose absorption is one scalar,
    leaves Q = U = V = 0 apart from the emission's, 1e-4 of the signal, and reads nothing."""
    from synthpy_amd import sightlines
    from synthpy_amd.simulator.domain import ScalarDomain

    lines = _absorbing_lines()
    dom, lengths = _reversing_domain(ScalarDomain)
    w0, wd = lines.omega0[0], lines.thermal_width(40.0)[0]
    om = w0 + wd * np.linspace(-12.0, 12.0, 70)
    view, I0, sp = _backlit(dom, lengths, lines, om)
    assert isinstance(sp, sightlines.StokesSpectra) and sp.intensity.shape == (8, 8, 70) and np.all(sp.steps > 0)
    depth = I0 - sp.intensity
    assert np.all(depth.max(axis=-1) > 1e-3 * I0) and np.all(sp.optical_depth.max(axis=-1) < 0.5)
    absorbed = sightlines.StokesSpectra(view, depth, sp.optical_depth, sp.column, sp.chord, sp.steps, sp.omega, lines, -sp.Q, -sp.U, -sp.V)
    b = absorbed.b_parallel(11 * wd)[..., 0]
    # B.n^ along each pixel's chord at the slab's mid-plane: n^ is nearly z, Bz = 30 tanh(x / 0.4 mm)
    o, d = view.lines()
    n = d / np.linalg.norm(d, axis=0)
    xm = (o[0] + d[0] * (0.0 - o[2]) / d[2]).reshape(8, 8)
    want = (30.0 * np.tanh(xm / 4e-4)) * n[2].reshape(8, 8) + 4.0 * n[1].reshape(8, 8)
    assert np.all(np.isfinite(b)) and np.array_equal(np.sign(b), np.sign(want)) and (want > 0).any() and (want < 0).any()
    strong = np.abs(want) > 10.0
    assert strong.sum() >= 24 and np.all(np.abs(b[strong] / want[strong] - 1.0) < 0.2)
    zee = dom.sightline_zeeman(view, lines, wavelengths=2 * np.pi * LIGHT / om, wing=8.0, step=2.5e-4, max_steps=60)
    assert np.max(np.abs(zee.V)) < 1e-3 * np.max(np.abs(sp.V))


@pytest.mark.gpu
def test_nan_edges(eng):
    """10: a NaN in one corner of B poisons exactly the chords the restatement says (those with a sample in its cells; a NaN shift is
    never dropped, so all their frequencies) and no other: the clean chords carry the bits of the run without it, and a chord that
    misses the box is never poisoned; a NaN in the polarisation is an argument error before the device."""
    R = _inputs(CASES[0])
    B = R["F"]["B"].copy()
    B[4, 3, 3, 1] = np.nan
    ref = _restate(R, B=B)
    bad = np.isnan(ref["V"])
    assert bad.any() and not bad.all() and np.array_equal(bad, np.repeat(bad.any(axis=1)[:, None], bad.shape[1], axis=1)) and not np.any(bad[ref["miss"]])
    fields = _upload(eng, R, B=B)
    try:
        got = _run(eng, R, fields=fields)
        for name in STOKES + ("tau",):
            assert np.array_equal(np.isnan(got[name]), np.isnan(ref[name])), name
        with pytest.raises(Exception, match="non-finite pol"):
            _run(eng, R, fields=fields, polarisation=(0.1, np.nan, 0.0))
    finally:
        gl._close(fields)
    clean = ~bad.any(axis=1)
    base = _run(eng, R)
    for name in STOKES + ("tau",):
        assert clean.any() and np.array_equal(got[name][clean], base[name][clean]), name


@pytest.mark.gpu
def test_both_generations_return_the_engines_bits(eng):
    """11: ScalarDomain.sightline_stokes of both generations returns the bits of engine.sightline_stokes on the same fields, in a
    StokesSpectra on which analysed, b_parallel, moments, fwhm, signal, polarisation_angle and degree work; a rotated() domain works
    unchanged."""
    from synthpy_amd import sightlines
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy import full_solver as fs

    lines = _absorbing_lines()
    w0, wd = lines.omega0[0], lines.thermal_width(40.0)[0]
    om = w0 + wd * np.linspace(-12.0, 12.0, 70)
    got = []
    for Domain in (NewDomain, fs.ScalarDomain):
        dom, lengths = _reversing_domain(Domain)
        got.append(_backlit(dom, lengths, lines, om, continuum=True, polarisation=(0.3, 0.2, -0.1), faraday=True)[2])
    view = got[0].view
    for sp in got:
        assert isinstance(sp, sightlines.StokesSpectra) and sp.lines is lines and sp.intensity.shape == sp.Q.shape == (8, 8, 70)
        assert np.all(np.isfinite(sp.intensity)) and np.all(sp.optical_depth > 0) and np.any(sp.V != 0)
        assert np.all(sp.intensity ** 2 * (1 + 1e-9) >= sp.Q ** 2 + sp.U ** 2 + sp.V ** 2)
        assert sp.moments(10 * wd)["radiance"].shape == (8, 8, 1) and sp.fwhm(10 * wd).shape == (8, 8, 1) and sp.signal().shape == (8, 8)
        assert sp.analysed(angle=0.3).shape == sp.analysed(circular=-1).shape == (8, 8, 70) and sp.b_parallel(11 * wd).shape == (8, 8, 1)
        assert sp.polarisation_angle().shape == (8, 8, 70) and np.all(sp.degree() <= 1 + 1e-9) and np.all(sp.degree() > 0.3)
    for name in ("intensity", "Q", "U", "V", "optical_depth", "column", "chord", "steps"):
        assert np.array_equal(getattr(got[0], name), getattr(got[1], name)), name
    dom, lengths = _reversing_domain(NewDomain)
    f = [eng.Field(np.asarray(a), dom.x, dom.y, dom.z) for a in (dom.ne, dom.Ti, dom.B)]
    try:
        o, d = view.lines()
        perm = view.order()
        ref = sightlines.default_reference(view)
        raw = eng.sightline_stokes(f[0], 30.0, f[1], 2.0, None, f[2], np.ascontiguousarray(o[:, perm]), np.ascontiguousarray(d[:, perm]),
                                   np.ascontiguousarray(ref[:, perm]), lines=lines, omegas=got[0].omega, continuum=True, wing=8.0, toward=+1,
                                   step=2.5e-4, max_steps=60, backlight=np.full((64, 70), float(np.ravel(view.radiance)[0])),
                                   polarisation=(0.3, 0.2, -0.1), faraday=True)
    finally:
        for h in f:
            h.close()
    for name, key in (("intensity", "intensity"), ("Q", "Q"), ("U", "U"), ("V", "V"), ("optical_depth", "optical_depth")):
        flat = getattr(got[0], name).reshape(64, 70)
        assert np.array_equal(flat[perm], raw[key]), name
    turned = dom.rotated(25.0, about="y")
    sp = turned.sightline_stokes(view, lines, wavelengths=2 * np.pi * LIGHT / om, wing=8.0, step=2.5e-4, max_steps=60, polarisation=(0.0, 0.0, 1.0))
    assert isinstance(sp, sightlines.StokesSpectra) and np.all(np.isfinite(sp.intensity)) and np.any(sp.Q != 0)
