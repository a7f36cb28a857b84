"""Line spectra along sightlines: sr_field_sightline_lines (sightline_lines.hip), engine.sightline_lines, utils.eos_opacity.LineTable,
sightlines.LineSpectra / sightline_lines and ScalarDomain.sightline_lines of both API generations.

THE REFERENCE for values is `restate_lines` below: include/synthray.h's rule in NumPy float64, operation for operation.  Its clip,
steps, sample positions and gather are tests/test_sightlines.py's (`geometry`, `gather`, imported), held to that file's standard:
chord, steps, column and the set of missed chords BIT-EQUAL.  What is new is held to a BUDGET derived from the operation count, in
tests/test_sightlines.py's units (u = 2^-53; a correctly rounded operation errs by at most 1 u relative, a library function by 2 u),
one side against the exact value of the rule on the same inputs, first order:

* SAME BITS on every side, because only +, -, *, /, sqrt and comparisons make them: beta, wc, wd, iw, g = ISP*iw, x, x2 and so the
  branch x2 > 40 (tested inputs keep x2 1e-9 away from 40 all the same).  The wide restatement (np.longdouble) keeps them float64:
  they are the rule itself, as the geometry and the gather are.
* the lattice search and the interpolant l(T) of a table T: tests/test_table_emission.py's E_l [u, ABSOLUTE],
      E_l = G_d (2 + 2|ld| + 5 dD_max) + G_t (2|lt| + 5 dT_max) + 2 M
  with the whole-table slopes G_d, G_t and M = max|T| per line (an lt within rounding of a lattice node may land on either side).
* aJ = exp(l(LJ))*g: E_l(LJ) + 2 (the library) + 1 (the product) = E_l(LJ) + 3; aK the same with LK.  phi = exp(-x2): 2 (x2 is
  exact).  aJ*phi: E_l + 6.  j is a sum of nc non-negative counted terms in ascending order: E_j = max_l E_l(LJ_l) + 6 + nc; E_aL the
  same from LK (0 where LK is NULL: aL = 0 exactly).
* the continuum: E_ac = 21, E_Sc = 4 + xc, xc = e_ph/Te (tests/test_emission.py); 0 where the node is dark or the continuum off.
* a counted sample with dtau != 0:  a = ac + aL (non-negative parts): E_a = max(E_ac, E_aL) + 1;  dtau = a*h: ea = E_a + 1;
  exp(-dtau): (2 + ea dtau) u;  -expm1(-dtau), condition number <= 1: (ea + 2) u;  ac*Sc + j: max(E_ac + E_Sc + 1, E_j) + 1;
  the quotient by a: es = that + E_a + 1;  b = quotient * (-expm1): (es + ea + 3) u.
* a counted sample with dtau == 0 (thin lines, no continuum: a == 0 exactly on every side):  b = j*h: (E_j + 1) u, and the sum
  I + b one more on everything: B <- B + T + b (E_j + 2), T <- T + b in the recurrence below.
* a sample without a counted term is tests/test_sightlines.py's sample with the continuum as its node: ea = E_ac + 1, es = E_Sc.
* a chord, marched sequentially: tests/test_sightlines.py's recurrence, B <- a (B + (4 + ea dtau) T) + b (es + ea + 4), T <- T a + b,
      budget_I = 2 u B + a floor of 4 n 2^-1074,      budget_tau = u (2 sum_j ea_j dtau_j + 2 n tau) + the same floor.
Test 1 checks the budgets against np.longdouble and prints the worst fraction used.

Tested inputs.  A (9, 8, 7)-node grid over +-4 mm with unequal spacing (tests/test_emission.py's `_coords`); ne log-uniform over
10^24 .. 10^25.5 m^-3, Te over 3 .. 300 eV, Z in [1, 8], Ti over 30 .. 1600 eV, |V_a| <= 3e5 m/s, node by node; a 6 x 5 lattice over
1 .. 500 eV x 1e17 .. 1e21 cm^-3.  Lines sit 1.2e-4 w0 apart from 250 nm on (thermal 1/e widths 0.7 .. 5e-4 w0, Doppler shifts up to
1e-3 w0: neighbours blend), every third one of helium's mass instead of carbon's; ln K is spread over a decade about the value that
makes a chord's line centre a few optical depths thick, ln J = ln K + ln B(T) + U(-1, 1).  Frequencies: most of them uniform over the
lines' span +- 2e-3 w0, the others 20 % below and above it, where every term is dropped (the ties of test 7); sorted in even cases,
in random order in odd ones.  Six chords -- oblique, along an axis through a node column, beside the box (a miss), a corner graze
of one sample, from inside the box, with one zero direction component -- or a 4 x 4 pinhole view.  step = a tenth of the x extent,
max_steps = 12.  The conditions (test 2) are asserted on the restatement alone.
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
from test_sightlines import EPS, TINY, _assert_close, _assert_exact, _planted, _poisoned, gather, geometry

LIGHT = 299792458.0
E_CH, M_P, ISP = 1.602176634e-19, 1.67262192369e-27, 0.5641895835477563
E_AC = 21.0  # tests/test_emission.py's E_ALPHA
SHAPE = (9, 8, 7)
MAX_STEPS = 12
NFREQS, NLINES = (5, 70, 257), (1, 3, 32)
_CACHE = {}


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
def host_lines(lines):
    """The bits the host hands the kernel (engine.line_table_params) + the slopes of the budget, per line."""
    from synthpy_amd import engine

    t, (LT, LD, w0, A, LJ, LK) = engine.line_table_params(lines)
    dT, dD = np.diff(LT), np.diff(LD)

    def slopes(T):
        return (np.max(np.abs(np.diff(T, axis=2)) / dD, axis=(1, 2)), np.max(np.abs(np.diff(T, axis=1)) / dT[:, None], axis=(1, 2)),
                np.max(np.abs(T), axis=(1, 2)))

    return dict(LT=LT, LD=LD, w0=w0, ci=(2.0 * E_CH) / (A * M_P), LJ=LJ, LK=LK, GJ=slopes(LJ), GK=None if LK is None else slopes(LK),
                dT_max=dT.max(), dD_max=dD.max())


def restate_lines(F, co, o, d, H, omegas, toward, step, max_steps, continuum, backlight=None, wide=False):
    """include/synthray.h's rule for sr_field_sightline_lines.  F: dict of ne, Te, Z (arrays (nx, ny, nz) or scalars for Te, Z), Ti
    (array or None) and V ((nx, ny, nz, 3) or None); co: the float32 coordinates; o, d: (3, N); H: host_lines(table); omegas: (n_freq).
    Returns I, tau, bI, bt (N, n_freq), column, chord, steps, miss (N), and what test 2 asks about: terms, counted (numbers of
    (sample, frequency, line) terms of samples that are not dark), near40 (the least |x2/40 - 1|), cases (samples x frequencies that
    took each update: not counted, counted with dtau != 0, counted with dtau == 0), ncount (N, n_freq): counted terms per element.
    wide: exp, expm1, log, the interpolant, the sums and the recurrence in np.longdouble."""
    from synthpy_amd import engine

    g = [np.float64(np.float32(a)) for a in co]
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    om, e_ph, c_om = engine.spectrum_constants(omegas)
    G = geometry(g, o, d, step, max_steps)
    hit, n, h = G["hit"], G["n"], G["h"]
    N, NF, NL = o.shape[1], len(om), len(H["w0"])
    wt = np.longdouble if wide else np.float64
    I = np.zeros((N, NF), wt) if backlight is None else np.array(backlight, wt)
    tau = np.zeros((N, NF), wt)
    T1, B, Bt = I.astype(np.float64), np.zeros((N, NF)), np.zeros((N, NF))
    column = np.zeros(N)
    with np.errstate(all="ignore"):
        su = toward / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    fields = [np.float64(F["ne"])] + [np.float64(F[k]) if np.ndim(F[k]) else float(F[k]) for k in ("Te", "Z")]
    has_ti, has_v = F.get("Ti") is not None, F.get("V") is not None
    if has_ti:
        fields.append(np.float64(F["Ti"]))
    if has_v:
        fields += [np.float64(F["V"][..., a]) for a in range(3)]
    terms = counted_terms = 0
    near40, cases, ncount = np.inf, [0, 0, 0], np.zeros((N, NF), np.int64)
    for m in range(int(n.max()) if N else 0):
        act = hit & (m < n)
        k = np.where(act, m if toward > 0 else n - 1 - m, 0)
        t = G["t0"] + (k + 0.5) * G["dt"]
        p = [o[a] + d[a] * t for a in range(3)]
        vals, inside = gather(fields, g, p, act)
        ne_s = np.where(inside, vals[0], 0.0)  # outside: dark, and ne counts as 0
        Te_s = np.where(inside, vals[1], 1.0) if np.ndim(vals[1]) else np.full(N, vals[1])
        Z_s = np.where(inside, vals[2], 1.0) if np.ndim(vals[2]) else np.full(N, vals[2])
        Ti_s = np.where(inside, vals[3], 1.0) if has_ti else Te_s
        with np.errstate(all="ignore"):
            column = np.where(act, column + ne_s * h, column)
            beta = np.zeros(N)
            if has_v:
                V = [np.where(inside, v, 0.0) for v in vals[-3:]]
                beta = (((V[0] * d[0] + V[1] * d[1]) + V[2] * d[2]) * su) / LIGHT
            dark = (Te_s <= 0) | (ne_s <= 0) | (Z_s <= 0) | (Ti_s <= 0) | ~inside
            live = act & ~dark
            a_ne, a_Te, a_Z, hw = ne_s.astype(wt), Te_s.astype(wt), Z_s.astype(wt), h.astype(wt)[:, None]
            ni = (a_ne * 1e-6) / a_Z
            lt, ld = np.log(a_Te), np.log(ni)
            i, ft = tab._locate(H["LT"].astype(wt), lt)
            j, fd = tab._locate(H["LD"].astype(wt), ld)

            def E_l(Gs, l):
                return (Gs[0][l] * (2 + 2 * np.abs(np.asarray(ld, np.float64)) + 5 * H["dD_max"])
                        + Gs[1][l] * (2 * np.abs(np.asarray(lt, np.float64)) + 5 * H["dT_max"]) + 2 * Gs[2][l])

            jj, aL = np.zeros((N, NF), wt), np.zeros((N, NF), wt)
            counted, nc = np.zeros((N, NF), bool), np.zeros((N, NF))
            EJ, EK = np.zeros((N, NF)), np.zeros((N, NF))
            for l in range(NL):
                wc = H["w0"][l] * (1.0 + beta)
                wd = H["w0"][l] * (np.sqrt(H["ci"][l] * Ti_s) / LIGHT)
                iw = 1.0 / wd
                gg = ISP * iw
                aJ = np.exp(tab._interp(H["LJ"][l].astype(wt), i, j, ft, fd)) * gg.astype(wt)
                x = (om[None, :] - wc[:, None]) * iw[:, None]
                x2 = x * x
                keep = ~(x2 > 40.0) & live[:, None]
                phi = np.exp(-x2.astype(wt))
                jj = np.where(keep, jj + aJ[:, None] * phi, jj)
                EJ = np.where(keep, np.maximum(EJ, E_l(H["GJ"], l)[:, None]), EJ)
                if H["LK"] is not None:
                    aK = np.exp(tab._interp(H["LK"][l].astype(wt), i, j, ft, fd)) * gg.astype(wt)
                    aL = np.where(keep, aL + aK[:, None] * phi, aL)
                    EK = np.where(keep, np.maximum(EK, E_l(H["GK"], l)[:, None]), EK)
                counted |= keep
                nc += keep
                terms += int(live.sum()) * NF
                counted_terms += int(keep.sum())
                if live.any() and NF:
                    near40 = min(near40, float(np.nanmin(np.abs(x2[live] / 40.0 - 1.0))))
            ncount += counted * nc.astype(np.int64)
            Ej = np.where(counted, EJ + 6 + nc, 0.0)
            EaL = np.where(counted & (H["LK"] is not None), EK + 6 + nc, 0.0)
            if continuum:
                ac, Sc, xc = nrl._node(a_ne[:, None], a_Te[:, None], a_Z[:, None], om[None, :], e_ph[None, :], c_om[None, :])
                Eac, Esc = np.where(ac != 0, E_AC, 0.0), np.where(ac != 0, 4 + xc, 0.0)
            else:
                ac, Sc, Eac, Esc = np.zeros((N, NF), wt), np.zeros((N, NF), wt), np.zeros((N, NF)), np.zeros((N, NF))
            act2 = act[:, None] & np.ones((1, NF), bool)
            # not counted: sr_field_sightlines' update with the continuum
            d0 = ac * hw
            a0, b0 = np.exp(-d0), Sc * (-np.expm1(-d0))
            # counted
            a_ = ac + aL
            d1 = a_ * hw
            thin = counted & act2 & (d1 == 0)
            gen = counted & act2 & ~thin
            a1, b1 = np.exp(-d1), ((ac * Sc + jj) / a_) * (-np.expm1(-d1))
            b2 = jj * hw
            I = np.where(gen, I * a1 + b1, np.where(thin, I + b2, np.where(act2, I * a0 + b0, I)))
            tau = np.where(gen, tau + d1, np.where(thin, tau, np.where(act2, tau + d0, tau)))
            cases[0] += int((act2 & ~counted).sum())
            cases[1] += int(gen.sum())
            cases[2] += int(thin.sum())
            # the budget's recurrence, float64
            f = lambda v: np.asarray(v, np.float64)
            Ea = np.maximum(Eac, EaL) + 1
            ea1 = Ea + 1
            es1 = np.maximum(Eac + Esc + 1, Ej) + 1 + Ea + 1
            ea0 = Eac + 1
            Bg = f(a1) * (B + (4 + ea1 * f(d1)) * T1) + f(b1) * (es1 + ea1 + 4)
            Bn = f(a0) * (B + (4 + ea0 * f(d0)) * T1) + f(b0) * (Esc + ea0 + 4)
            Bh = B + T1 + f(b2) * (Ej + 2)
            B = np.where(gen, Bg, np.where(thin, Bh, np.where(act2, Bn, B)))
            T1 = np.where(gen, T1 * f(a1) + f(b1), np.where(thin, T1 + f(b2), np.where(act2, T1 * f(a0) + f(b0), T1)))
            Bt = np.where(gen, Bt + ea1 * f(d1), np.where(act2 & ~thin, Bt + ea0 * f(d0), Bt))
    floor = (4 * n * TINY)[:, None]
    with np.errstate(all="ignore"):
        bI, bt = 2 * EPS * B + floor, EPS * (2 * Bt + 2 * n[:, None] * tau.astype(np.float64)) + floor
    return dict(I=I, tau=tau, bI=bI, bt=bt, column=column, chord=G["chord"], steps=n.astype(np.int32), miss=~hit, terms=terms,
                counted=counted_terms, near40=near40, cases=cases, ncount=ncount)


# ---------------------------------------------------------------- inputs
def _grid():
    """The grid and the float64 fields, made once and read-only."""
    if "grid" not in _CACHE:
        rng = np.random.default_rng(2024)
        co = [nrl._coords(m, 300 + k) for k, m in enumerate(SHAPE)]
        K = dict(co=co, g=[np.float64(a) for a in co], ne=10.0 ** rng.uniform(24.0, 25.5, SHAPE), Te=10.0 ** rng.uniform(0.5, 2.5, SHAPE),
                 Z=rng.uniform(1.0, 8.0, SHAPE), Ti=10.0 ** rng.uniform(1.5, 3.2, SHAPE), V=rng.uniform(-3e5, 3e5, SHAPE + (3,)))
        K["step"] = float(K["g"][0][-1] - K["g"][0][0]) / 10
        for a in (K["ne"], K["Te"], K["Z"], K["Ti"], K["V"]):
            a.setflags(write=False)
        _CACHE["grid"] = K
    return _CACHE["grid"]


def make_lines(n_line, lk, seed=5, strength=1.0):
    """A LineTable of n_line lines 1.2e-4 w0 apart from 250 nm on, on a jittered 6 x 5 lattice (the module docstring)."""
    from synthpy_amd.utils.eos_opacity import LineTable

    rng = np.random.default_rng(seed + n_line)
    T, D = tab._lattice(1.0, 500.0, 6, rng), tab._lattice(1e17, 1e21, 5, rng)
    w0 = (2 * np.pi * LIGHT / 250e-9) * (1.0 + 1.2e-4 * np.arange(n_line))
    A = np.where(np.arange(n_line) % 3 == 2, 4.0026, 12.011)
    lnK = np.log(strength * 1.3e15 / max(1.0, n_line / 4)) + rng.uniform(-1.15, 1.15, (n_line, 6, 5))
    thin = LineTable(T, D, np.ones((n_line, 6, 5)), wavelengths=2 * np.pi * LIGHT / w0, mass_number=A)
    lnJ = lnK + np.log(thin.planck())[:, :, None] + rng.uniform(-1.0, 1.0, lnK.shape)
    return LineTable(T, D, np.exp(lnJ), wavelengths=2 * np.pi * LIGHT / w0, mass_number=A, absorption=np.exp(lnK) if lk else None)


def make_freqs(lines, n_freq, seed, sort):
    w0 = lines.omega0
    rng = np.random.default_rng(seed)
    n_far = 1 if n_freq < 10 else max(2, n_freq // 16)
    near = rng.uniform(w0.min() * (1 - 2e-3), w0.max() * (1 + 2e-3), n_freq - n_far)
    far = np.where(np.arange(n_far) % 2 == 0, 0.8 * w0.min(), 1.2 * w0.max()) * rng.uniform(0.99, 1.01, n_far)
    om = np.concatenate([near, far])
    return np.sort(om) if sort else rng.permutation(om)


def six_chords(g):
    P = _planted(g)
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    mid, ext = 0.5 * (lo + hi), hi - lo
    src = lo - 0.3 * ext * np.array([1.0, 0.8, 0.6])
    L = [(src, 1.3 * (mid - src)), P["column"], P["beside"], P["graze"], P["inside"],
         ((lo[0] - 2.0 ** -10, mid[1] - 0.2 * ext[1], mid[2] + 0.1 * ext[2]), (1.0, 0.4, 0.0))]
    return np.ascontiguousarray(np.array([p[0] for p in L], np.float64).T), np.ascontiguousarray(np.array([p[1] for p in L], np.float64).T)


def pinhole_chords():
    from synthpy_amd import sightlines

    cam = sightlines.PinholeCamera((1e-3, -2e-3, 25e-3), (0.05, 0.1, -1.0), (0, 1, 0), 50e-3, (4, 4), 5e-3)
    o, d = cam.lines()
    return np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)


# the pruned flag cases of test 6: (f64, toward, Ti given, V given, LK given, continuum) drawn once, n_freq and n_line cycling so that
# all nine pairs occur, Te / Z as fields or uniform, two of them on the pinhole view
_BITS = np.random.default_rng(11).integers(0, 2, (24, 6))
CASES = tuple(dict(f64=bool(b[0]), toward=+1 if b[1] else -1, ti=bool(b[2]), v=bool(b[3]), lk=bool(b[4]), cont=bool(b[5]), nf=NFREQS[k % 3],
                   nl=NLINES[(k // 3) % 3], te_f=k % 4 != 3, z_f=k % 5 < 3, view="pinhole" if k in (5, 14) else "six", k=k)
              for k, b in enumerate(_BITS))


def _id(c):
    return (f"{c['k']}-{'f64' if c['f64'] else 'f32'}-{c['toward']:+d}-Ti{int(c['ti'])}-V{int(c['v'])}-LK{int(c['lk'])}-cont{int(c['cont'])}"
            f"-{c['nf']}f-{c['nl']}l-{c['view']}")


def _inputs(c, **over):
    """The inputs of one case: the fields in its dtype, the chords, the table, the frequencies, the backlight."""
    c = dict(c, **over)
    K = _grid()
    dt = np.float64 if c["f64"] else np.float32
    F = dict(ne=K["ne"].astype(dt), Te=K["Te"].astype(dt) if c["te_f"] else 37.5, Z=K["Z"].astype(dt) if c["z_f"] else 4.0,
             Ti=K["Ti"].astype(dt) if c["ti"] else None, V=K["V"].astype(dt) if c["v"] else None)
    o, d = six_chords(K["g"]) if c["view"] == "six" else pinhole_chords()
    lines = make_lines(c["nl"], c["lk"])
    om = make_freqs(lines, c["nf"], 40 + c["k"], sort=c["k"] % 2 == 0)
    back = np.random.default_rng(60 + c["k"]).uniform(0.0, 2e-6, (o.shape[1], len(om)))
    return dict(c=c, K=K, F=F, o=o, d=d, lines=lines, om=om, back=back, step=K["step"], max_steps=MAX_STEPS)


def _restate(R, wide=False, **kw):
    c = R["c"]
    return restate_lines(R["F"], R["K"]["co"], R["o"], R["d"], host_lines(R["lines"]), R["om"], c["toward"], R["step"], R["max_steps"],
                         c["cont"], backlight=kw.pop("backlight", R["back"]), wide=wide, **kw)


def _case(c):
    key = ("case", c["k"])
    if key not in _CACHE:
        R = _inputs(c)
        R["ref"] = _restate(R)
        _CACHE[key] = R
    return _CACHE[key]


def _upload(eng, R):
    K, F = R["K"], R["F"]
    return [None if F[k] is None else (eng.Field(F[k], *K["co"]) if np.ndim(F[k]) else float(F[k])) for k in ("ne", "Te", "Ti", "Z", "V")]


def _close(fields):
    for f in fields:
        if f is not None and not isinstance(f, float):
            f.close()


def _run(eng, R, fields=None, timed=True, **kw):
    """engine.sightline_lines on freshly uploaded fields (unless given); I, tau (n, n_freq) as the restatement's."""
    own = fields is None
    fields = _upload(eng, R) if own else fields
    c = R["c"]
    try:
        out = eng.sightline_lines(*fields, R["o"], R["d"], lines=R["lines"], omegas=R["om"], continuum=c["cont"], toward=c["toward"],
                                  step=R["step"], max_steps=R["max_steps"], backlight=kw.pop("backlight", R["back"]), **kw)
        if "intensity" in out:
            assert not timed or fields[0].last_kernel_ms > 0
            assert out["intensity"].shape == out["optical_depth"].shape == (R["o"].shape[1], len(R["om"]))
            out["I"], out["tau"] = out["intensity"], out["optical_depth"]
        return out
    finally:
        if own:
            _close(fields)


# chunk boundaries (test 8): three chords along x with exactly N samples, N about the staging's chunk
def _chunk_case(fl, N, chunk):
    c = dict(CASES[0], f64=True, toward=+1 if N % 2 else -1, ti=True, v=True, lk=True, cont=True, nf={64: 5, 256: 200}[fl], nl=3, te_f=True,
             z_f=True, view="six", k=100 + N)
    R = _inputs(c)
    g = R["K"]["g"]
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    far = lo[0] - 2.0 ** -10
    o = np.array([[far, g[1][2], g[2][3]], [far, 0.37 * lo[1] + 0.63 * hi[1], 0.5 * (g[2][1] + g[2][2])], [far, lo[1], 0.5 * (lo[2] + hi[2])]]).T
    d = np.array([[1.0, 0.0, 0.0]] * 3).T
    R.update(o=np.ascontiguousarray(o), d=np.ascontiguousarray(d), back=R["back"][:3], max_steps=4 * chunk, step=(hi[0] - lo[0]) / (N - 0.5))
    return R


def _chunk_counts(chunk):
    return (chunk - 1, chunk, chunk + 1, 2 * chunk + 1)


# ================================================================ CPU tests
def test_restatement_against_longdouble(built):
    """1: the yardstick's budgets against the same rule with its library functions, sums and recurrence in np.longdouble."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    worst = [0.0, 0.0]
    for k in (0, 4, 7, 8, 13, 17, 23):
        R = _case(CASES[k])
        wide = _restate(R, wide=True)
        for m, (name, bud) in enumerate((("I", "bI"), ("tau", "bt"))):
            a, b, lim = R["ref"][name], wide[name].astype(np.float64), R["ref"][bud] / 2  # one side of the two the budget holds
            assert np.all(np.isfinite(a)) and np.all(np.abs(a - b) <= lim), f"{_id(CASES[k])}: {name} off by {np.max(np.abs(a - b) / np.maximum(lim, TINY)):.3f}"
            pos = lim > 0
            worst[m] = max(worst[m], float(np.max(np.abs(a - b)[pos] / lim[pos])))
    print(f"float64 restatement against np.longdouble: worst fraction of the one-sided budget used: I {worst[0]:.3f}, tau {worst[1]:.3f}")
    assert worst[0] > 0  # the two differ: the wide one is wide


def test_tested_inputs_meet_the_conditions(built):
    """2: on the restatement alone: no x2 within 1e-9 of 40; every case counts at least 10 % of its terms and drops at least 10 %;
    the flags, sizes and update cases are covered."""
    from synthpy_amd import engine

    total = np.zeros(3, np.int64)
    everything = list(CASES) + [_chunk_case(fl, N, engine.LINES_CHUNK)["c"] for fl in (64, 256) for N in _chunk_counts(engine.LINES_CHUNK)]
    for c in everything:
        R = _case(c) if c["k"] < 100 else None
        ref = R["ref"] if R else _restate(_chunk_case({5: 64, 200: 256}[c["nf"]], c["k"] - 100, engine.LINES_CHUNK))
        share = ref["counted"] / ref["terms"]
        print(f"{_id(c)}: {ref['terms']} terms, {share:.3f} counted, least |x2/40 - 1| {ref['near40']:.2e}, updates {ref['cases']}")
        assert ref["near40"] > 1e-9, _id(c)
        assert 0.10 <= share <= 0.90, f"{_id(c)}: {share:.3f} of the terms counted"
        assert np.all(np.isfinite(ref["I"])) and np.all(np.isfinite(ref["tau"])) and np.all(ref["I"][~ref["miss"]] > 0)
        if c["k"] < 100:
            assert np.any(ref["miss"]) and len(set(ref["steps"].tolist())) >= 3
            assert c["view"] == "pinhole" or (np.any(ref["steps"] == 1) and np.any(ref["steps"] == MAX_STEPS))
            assert np.any(ref["ncount"][~ref["miss"]] == 0) and np.any(ref["ncount"] > 0)
        total += ref["cases"]
    assert np.all(total > 0), f"update cases not counted / counted / counted with dtau == 0: {total}"
    for name in ("f64", "ti", "v", "lk", "cont", "te_f", "z_f"):
        assert {c[name] for c in CASES} == {True, False}, name
    assert {c["toward"] for c in CASES} == {1, -1} and {c["view"] for c in CASES} == {"six", "pinhole"}
    assert {(c["nf"], c["nl"]) for c in CASES} == {(a, b) for a in NFREQS for b in NLINES}
    for pair in (("lk", "cont"), ("ti", "v"), ("f64", "toward")):
        assert len({(c[pair[0]], c[pair[1]]) for c in CASES}) == 4, pair
    assert 24 <= len(CASES) <= 36


def test_header_ctypes_and_python_signatures(built):
    """3: the header's prototype and structs, the ctypes binding and the Python signatures agree; the library exports the symbol."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "synthray.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sr_field_sightline_lines\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 21
    kinds = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]
    assert kinds[5] == "const sr_line_table *" and kinds[6] == "const sr_lines_params *" and kinds[7] == "int64_t" and kinds[10] == "int32_t"
    for struct, cls, fields, size in (("sr_lines_params", built.LinesParams, ["toward", "max_steps", "continuum", "reserved", "step", "Te", "Z"], 40),
                                      ("sr_line_table", built.LineTable, ["nT", "nD", "n_line", "reserved", "LT", "LD", "w0", "A", "LJ", "LK"], 64)):
        m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", text)
        assert m and re.findall(r"\b(" + "|".join(fields) + r")\b", m.group(1)) == fields
        assert [f[0] for f in cls._fields_] == fields and C.sizeof(cls) == size
    assert [getattr(built.LinesParams, f).offset for f in ("toward", "max_steps", "continuum", "reserved", "step", "Te", "Z")] == [0, 4, 8, 12, 16, 24, 32]
    assert re.search(r"#define\s+SR_MAX_LINES\s+32\b", text) and built.MAX_LINES == 32
    res, args = built.SYMBOLS["sr_field_sightline_lines"]
    assert res is C.c_int and len(args) == 21 and args[7] is C.c_int64 and args[10] is C.c_int32
    assert hasattr(built.lib, "sr_field_sightline_lines") and built.SYMBOLS["sr_lines_chunk"] == (C.c_int, [])
    mk = open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()
    assert "sightline_lines.hip" in mk and "line_node.inc" in mk  # the build id covers both
    raw = open(os.path.join(ROOT, "include", "synthray.h")).read()
    for word in ("Lorentzian", "Zeeman", "exp(-40)", "partial", "instrument function", "one GPU only"):
        assert word in raw, word
    assert raw.count("t0 = max(t0, min(ta, tb))") == 1  # the clip is stated once: this section refers to it

    from synthpy_amd import engine, sightlines
    from synthpy_amd._domain import DomainExtras
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.sightline_lines) == ["ne", "Te", "Ti", "Z", "V", "origins", "directions", "lines", "omegas", "continuum", "toward", "step",
                                             "max_steps", "backlight", "want"]
    par = inspect.signature(engine.sightline_lines).parameters
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names(engine.sightline_lines)[7:])
    assert names(sightlines.sightline_lines) == ["domain", "view", "lines", "wavelengths", "photon_energies", "continuum", "step", "max_steps", "fields"]
    assert names(NewDomain.sightline_lines) == names(OldDomain.sightline_lines) == ["self", "view", "lines", "wavelengths", "photon_energies",
                                                                                     "continuum", "step", "max_steps"]
    assert NewDomain.sightline_lines is DomainExtras.sightline_lines is OldDomain.sightline_lines
    assert issubclass(sightlines.LineSpectra, sightlines.SightlineSpectra)
    assert engine.LINES_CHUNK == built.lib.sr_lines_chunk() and 2 * engine.LINES_CHUNK * (10 + 4 * 32) * 8 <= 64 * 1024
    for doc in (engine.sightline_spectra.__doc__, sightlines.sightline_spectra.__doc__, DomainExtras.sightline_spectra.__doc__):
        assert "Doppler shifts" not in doc.split("Not modelled")[1].split("Spectral lines")[0]


def test_argument_checks_come_before_the_device(built):
    """4: every rejected argument is SR_ERR_INVALID with its own text and the device is never initialised: the calls carry NULL
    fields, so a call that passed every other check ends at 'NULL ne' (the checks that need a live sr_field are test 11's)."""
    from synthpy_amd import engine

    lib, ptr = built.lib, built.ptr
    lines = make_lines(3, True)
    o0, d0 = np.zeros((3, 2)), np.ones((3, 2))
    out = np.zeros((2, 5))
    om0, e0, c0 = engine.spectrum_constants(np.linspace(7.5e15, 7.6e15, 5))

    def params(toward=1, step=1e-4, max_steps=10, continuum=0):
        p = built.LinesParams()
        p.toward, p.max_steps, p.continuum, p.step = toward, max_steps, continuum, step
        return p

    def table(**change):  # a fresh table each time: w0 and A are the LineTable's own arrays, and some checks below spoil them
        t, keep = engine.line_table_params(make_lines(3, True))
        for k, v in change.items():
            setattr(t, k, v)
        return t, keep

    t0, keep0 = table()  # the default table and the arrays it points into

    def call(p, n=2, o=o0, d=d0, I=out, tau=out, t=t0, nf=5, om=om0, e=e0, c=c0):
        return lib.sr_field_sightline_lines(None, None, None, None, None, None if t is None else C.byref(t), None if p is None else C.byref(p), n,
                                            ptr(o), ptr(d), nf, ptr(om), ptr(e), ptr(c), None, ptr(I), ptr(tau), None, None, None, None)

    def err(text, *a, **kw):
        assert call(*a, **kw) == -1 and text in built.last_error(), (text, built.last_error())

    err("NULL argument", None)
    for name in ("o", "d", "I", "tau"):
        err("NULL argument", params(), **{name: None})
    for name in ("om", "e", "c"):
        err("NULL omega, e_ph or c_omega", params(), **{name: None})
    err("n must not be negative", params(), n=-1)
    err("n_freq must not be negative", params(), nf=-3)
    many = np.full(built.MAX_FREQS + 1, 1.0)
    err("n_freq must be 1..16384", params(), nf=built.MAX_FREQS + 1, om=many, e=many, c=many)
    for w in (0.0, -1.0, np.nan, np.inf):
        bad = om0.copy()
        bad[4] = w
        err("omega of frequency 4", params(), om=bad)
    for name in ("e", "c"):
        bad = e0.copy()
        bad[3] = np.nan
        err("e_ph or c_omega of frequency 3", params(), **{name: bad})
    for toward in (0, 2, -3):
        err("toward", params(toward=toward))
    for step in (0.0, -1e-4, np.nan, np.inf):
        err("step must be finite and positive", params(step=step))
    for ms in (0, -5):
        err("max_steps", params(max_steps=ms))
    # the line table
    err("NULL line table", params(), t=None)
    for member in ("LT", "LD", "w0", "A", "LJ"):
        t, keep = table(**{member: None})
        err("NULL line-table member", params(), t=t)
    for nl in (0, -1, built.MAX_LINES + 1):
        t, keep = table(n_line=nl)
        err("n_line must be 1..32", params(), t=t)
    for member in ("nT", "nD"):
        for v in (1, 513):
            t, keep = table(**{member: v})
            err(f"{member} must be 2..512", params(), t=t)
    for at, member in ((2, "w0"), (3, "A")):
        for v in (0.0, -2.0, np.nan, np.inf):
            t, keep = table()
            keep[at][1] = v
            err(f"{member} of line 1 must be finite and positive", params(), t=t)
    t, keep = table()
    keep[0][1] = keep[0][0]
    err("LT is not strictly increasing at 1", params(), t=t)
    t, keep = table()
    keep[1][2] = np.nan
    err("LD[2] is not finite", params(), t=t)
    for at, member in ((4, "LJ"), (5, "LK")):
        t, keep = table()
        keep[at][2, 1, 3] = np.inf
        err(f"{member} has a non-finite entry (line 2)", params(), t=t)
    err("n x frequency tiles exceeds 2^31 - 1 workgroups", params(), n=2 ** 31, nf=5)
    for name, text in (("o", "non-finite origin of line 1"), ("d", "non-finite direction of line 1")):
        for v in (np.nan, np.inf):
            a = np.ones((3, 2))
            a[2, 1] = v
            err(text, params(), **{name: a})
    dz = np.ones((3, 2))
    dz[:, 1] = 0.0
    err("the direction of line 1 is zero", params(), d=dz)
    t, keep = table(LK=None)
    err("NULL ne", params(), t=t)               # thin lines: LK may be NULL
    err("NULL ne", params(continuum=1))         # every other argument was in order
    err("NULL ne", params(), n=0)               # n == 0 and n_freq == 0 do not skip the checks
    err("NULL ne", params(), nf=0)
    assert "sr_field_sightline_lines" in built.last_error() and keep0 is not None

    with pytest.raises(ValueError, match="Field"):
        engine.sightline_lines(np.zeros((2, 2, 2)), 1.0, None, 1.0, None, o0, d0, lines=lines, omegas=om0, toward=1, step=1e-4, max_steps=5)


def test_line_table_and_moments_by_hand(built):
    """5: LineTable validates like SpectralOpacityTable and names the member; with_lte_absorption() against a hand computation;
    LineSpectra.moments() on a synthetic Gaussian, by hand."""
    from synthpy_amd import sightlines
    from synthpy_amd.utils.eos_opacity import LineTable

    T, D = [1.0, 10.0, 100.0], [1e18, 1e20]
    J = np.full((2, 3, 2), 3.0)
    t = LineTable(T, D, J, photon_energy=[2.0, 4.0], mass_number=12.0)
    assert t.n_line == 2 and t.absorption is None and t.mass_number.tolist() == [12.0, 12.0]
    assert np.allclose(t.omega0, np.array([2.0, 4.0]) * tab.E_CHARGE / tab.HBAR, rtol=1e-15) and np.allclose(t.photon_energy, [2.0, 4.0], rtol=1e-15)
    one = LineTable(T, D, J[0], wavelengths=500e-9, mass_number=[4.0])
    assert one.n_line == 1 and np.allclose(one.omega0, 2 * np.pi * LIGHT / 500e-9, rtol=1e-15) and np.allclose(one.wavelengths, 500e-9, rtol=1e-15)
    for kw, word in ((dict(temperatures=[1.0, 1.0, 2.0]), "temperatures"), (dict(ion_densities=[1e18]), "densities"),
                     (dict(emissivity=J[:, :2]), "emissivity"), (dict(emissivity=-J), "emissivity"), (dict(emissivity=np.ones((33, 3, 2))), "1 to 32"),
                     (dict(absorption=J[:1]), "absorption"), (dict(absorption=J * np.nan), "absorption"), (dict(photon_energy=[2.0]), "photon_energy"),
                     (dict(photon_energy=[2.0, -1.0]), "photon_energy"), (dict(wavelengths=[1e-7, 2e-7]), "exactly one"),
                     (dict(photon_energy=None), "exactly one"), (dict(mass_number=None), "mass_number"), (dict(mass_number=[1.0, 2.0, 3.0]), "mass_number"),
                     (dict(mass_number=0.0), "mass_number")):
        args = dict(temperatures=T, ion_densities=D, emissivity=J, photon_energy=[2.0, 4.0], mass_number=12.0)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            LineTable(**args)
    # Kirchhoff by hand: K = J / B_omega(omega0, T), B = hbar w^3 / (4 pi^3 c^2) / expm1(hbar w / (e T))
    lte = t.with_lte_absorption()
    assert t.absorption is None and lte.emissivity is t.emissivity and lte.absorption.shape == (2, 3, 2)
    for l, e_ph in enumerate((2.0, 4.0)):
        w = e_ph * tab.E_CHARGE / tab.HBAR
        for i, Te in enumerate(T):
            B = tab.HBAR * w ** 3 / (4 * np.pi ** 3 * LIGHT ** 2) / np.expm1(e_ph / Te)
            assert np.allclose(lte.absorption[l, i], 3.0 / B, rtol=1e-13)
    # moments of 2 exp(-((w - wc)/wd)^2) about w0: radiance 2 wd sqrt(pi), velocity c (wc - w0)/w0, Ti = A m_p c^2 (wd^2/2) / (e w0^2)
    w0 = t.omega0
    wd, shift = 3e-4 * w0[0], 1.1e-4 * w0[0]
    om = np.concatenate([w0[0] + shift + wd * np.linspace(-8, 8, 257), [w0[1]]])  # one frequency at the other line: NaN there
    inten = np.stack([2.0 * np.exp(-((om - w0[0] - shift) / wd) ** 2), np.zeros_like(om)])
    ch = sightlines.Chords(np.zeros((3, 2)), np.ones((3, 2)), -1)
    sp = sightlines.LineSpectra(ch, inten, np.zeros_like(inten), np.zeros(2), np.zeros(2), np.zeros(2, np.int32), om, t)
    assert sp.lines is t and sp.signal().shape == (2,)
    M = sp.moments(10 * wd)
    assert M["radiance"].shape == M["velocity"].shape == M["Ti"].shape == (2, 2)
    assert np.isclose(M["radiance"][0, 0], 2.0 * wd * np.sqrt(np.pi), rtol=1e-12) and np.isclose(M["velocity"][0, 0], LIGHT * 1.1e-4, rtol=1e-9)
    assert np.isclose(M["Ti"][0, 0], 12.0 * M_P * LIGHT ** 2 * (wd ** 2 / 2) / (E_CH * w0[0] ** 2), rtol=1e-9)
    assert np.isclose(t.thermal_width(M["Ti"][0, 0])[0], wd, rtol=1e-9)
    assert np.all(np.isnan(M["velocity"][:, 1])) and np.all(np.isnan(M["Ti"][1]))  # one frequency in the window; a dark chord
    with pytest.raises(ValueError, match="window"):
        sp.moments(-1.0)


# ================================================================ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_kernel_against_restatement(eng, c):
    """6: chord, steps, column and the missed chords bit-equal, the NaN sets equal (none), I and tau within budget."""
    R = _case(c)
    got = _run(eng, R)
    _assert_exact(got, R["ref"], _id(c))
    _assert_close(got, R["ref"], _id(c))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 9, 14, 20])
def test_ties_to_the_continuum_entries(eng, k):
    """7: at the elements where every term is dropped, continuum=True returns engine.sightline_spectra's bits and continuum=False
    the backlight and tau == 0 exactly; column, chord and steps are engine.sightlines'."""
    base = _case(CASES[k])
    quiet = (base["ref"]["ncount"] == 0)
    assert quiet[~base["ref"]["miss"]].any() and not quiet.all()
    fields = _upload(eng, base)
    try:
        three = [fields[0], fields[1], fields[3]]
        kw = dict(toward=base["c"]["toward"], step=base["step"], max_steps=base["max_steps"])
        spec = eng.sightline_spectra(*three, base["o"], base["d"], omegas=base["om"], backlight=base["back"], **kw)
        four = eng.sightlines(*three, base["o"], base["d"], omegas=base["om"][:4], **kw)
        for cont in (True, False):
            R = dict(base, c=dict(base["c"], cont=cont))
            got = _run(eng, R, fields=fields)
            for name in ("column", "chord", "steps"):
                assert np.array_equal(got[name], spec[name]) and np.array_equal(got[name], four[name]), f"{name} differs from engine.sightlines'"
            if cont:
                assert np.array_equal(got["intensity"][quiet], spec["intensity"][quiet]), "I differs from sightline_spectra's where nothing is counted"
                assert np.array_equal(got["optical_depth"][quiet], spec["optical_depth"][quiet])
                assert np.any(spec["optical_depth"][quiet] > 0)
            else:
                assert np.array_equal(got["intensity"][quiet], base["back"][quiet]) and np.all(got["optical_depth"][quiet] == 0)
            loud = ~quiet & ~base["ref"]["miss"][:, None]
            # the lines are there (a term counted at exp(-40) of its peak may add less than a rounding: most, not all)
            assert np.mean(got["intensity"][loud] != (spec["intensity"] if cont else base["back"])[loud]) > 0.5
    finally:
        _close(fields)


@pytest.mark.gpu
@pytest.mark.parametrize("fl", [64, 256])
@pytest.mark.parametrize("which", range(4))
def test_chunk_boundaries_of_the_sample_staging(eng, fl, which):
    """8: chords of LINES_CHUNK - 1, LINES_CHUNK, LINES_CHUNK + 1 and 2 LINES_CHUNK + 1 samples, at both tile widths."""
    N = _chunk_counts(eng.LINES_CHUNK)[which]
    R = _chunk_case(fl, N, eng.LINES_CHUNK)
    ref = _restate(R)
    assert ref["steps"].tolist() == [N] * 3 and ref["cases"][0] > 0 and ref["cases"][1] > 0
    got = _run(eng, R)
    _assert_exact(got, ref, f"{N} samples, tiles of {fl}")
    _assert_close(got, ref, f"{N} samples, tiles of {fl}")


def _uniform(eng, lines, om, V, Ti, toward, Te=25.0, ne=2e24, Z=2.0, continuum=False, n_steps=20):
    """One chord along +x through a uniform plasma on the grid: (the engine's dict, the restatement, the chord's length)."""
    K = _grid()
    F = dict(ne=np.full(SHAPE, ne), Te=Te, Z=Z, Ti=np.full(SHAPE, Ti), V=np.broadcast_to(np.float64(V), SHAPE + (3,)).copy())
    g = K["g"]
    o, d = np.array([[g[0][0] - 1e-3, 0.1e-3, -0.2e-3]]).T, np.array([[2.0, 0.0, 0.0]]).T
    length = g[0][-1] - g[0][0]
    c = dict(toward=toward, cont=continuum)
    R = dict(c=c, K=K, F=F, o=o, d=d, lines=lines, om=om, back=None, step=length / (n_steps - 0.5), max_steps=100)
    ref = _restate(R, backlight=None)
    assert ref["steps"].tolist() == [n_steps]
    return _run(eng, R, backlight=None), ref, ref["chord"][0]


@pytest.mark.gpu
def test_uniform_plasma_closed_forms(eng):
    """9: a uniform plasma.  Thin single line: I(w) = J L phi(w), phi = ISP/wd exp(-((w - wc)/wd)^2), within the restatement's budget
    + 8 u for the closed form's own roundings (exp 2, the quotient, the square and four products, rounded up).  Uniform V: the
    centroid sits at w0 vpar/c, blue when the plasma moves towards the observer, for toward = +1 and -1; the width returns Ti.
    An LTE-thick line: I(w0) is the Planck radiance within e^-tau."""
    from synthpy_amd import sightlines
    from synthpy_amd.utils.eos_opacity import LineTable

    T, D = [1.0, 25.0, 400.0], [1e17, 1e21]
    J0, A, Ti = 4.0e9, 12.011, 300.0
    thin = LineTable(T, D, np.full((3, 2), J0), wavelengths=250e-9, mass_number=A)
    w0 = thin.omega0[0]
    wd = w0 * (np.sqrt(((2.0 * E_CH) / (A * M_P)) * Ti) / LIGHT)
    assert np.isclose(thin.thermal_width(Ti)[0], wd, rtol=1e-14)
    v_th = LIGHT * wd / w0
    n_steps = 20
    for toward, V in ((+1, (1.5e5, 7e4, -3e4)), (-1, (1.5e5, 7e4, -3e4)), (+1, (0.0, 0.0, 0.0))):
        vpar = V[0] * toward  # the chord runs along +x; the light travels along toward * d
        wc = w0 * (1.0 + vpar / LIGHT)
        om = wc + wd * np.linspace(-8.0, 8.0, 257)
        got, ref, L = _uniform(eng, thin, om, V, Ti, toward, n_steps=n_steps)
        _assert_close(got, ref, f"uniform thin line, toward {toward:+d}")
        x2 = ((om - wc) * (1.0 / wd)) ** 2
        closed = np.where(x2 > 40.0, 0.0, (np.exp(np.log(J0)) * (ISP * (1.0 / wd))) * np.exp(-x2) * L)
        assert np.all(np.abs(got["I"][0] - closed) <= ref["bI"][0] + 8 * EPS * closed), "I differs from J L phi"
        assert np.all(got["tau"] == 0) and got["I"][0].max() > 0 and np.any(closed == 0)
        # moments: each I carries (n + 20) u, a moment is a ratio of trapezoid sums of 257 terms ((n + 300) u a side, the integrand of
        # the first moment reaching 6.4 wd, of the second 40 wd^2 against wd^2 / 2); the frequencies are rounded to u w0, which moves a
        # trapezoid sum of a Gaussian by that over wd.  The trapezoid itself is exact to exp(-(16 pi)^2) at this spacing, wd / 16.
        ch = sightlines.Chords([[0.0], [0.0], [0.0]], [[1.0], [0.0], [0.0]], toward)
        sp = sightlines.LineSpectra(ch, got["I"], got["tau"], got["column"], got["chord"], got["steps"], om, thin)
        M = sp.moments(9 * wd)
        rel = 2 * (n_steps + 300) * EPS + 4 * EPS * w0 / wd
        assert abs(M["velocity"][0, 0] - vpar) <= 6.4 * rel * v_th, (M["velocity"][0, 0], vpar)
        assert abs(M["Ti"][0, 0] / Ti - 1.0) <= 80 * rel + 2 * (6.4 * rel) ** 2, M["Ti"][0, 0]
        assert abs(M["radiance"][0, 0] / (J0 * L) - 1.0) <= rel + 8 * EPS + (n_steps + 20) * EPS
        if V[0]:
            assert (M["velocity"][0, 0] > 0) == (toward > 0)  # +x flow: towards the observer of toward = +1, a blue shift
    # LTE, thick: tau(w0) about 40; Te on a lattice node, so that the table's Planck function is B(w0, Te) but for E_l
    thick = LineTable(T, D, np.full((3, 2), 3.0e11), wavelengths=250e-9, mass_number=A).with_lte_absorption()
    om = w0 + wd * np.array([0.0, 0.5, -1.0, 30.0])
    got, ref, L = _uniform(eng, thick, om, (0.0, 0.0, 0.0), Ti, -1)
    _assert_close(got, ref, "uniform LTE line")
    e_ph = tab.HBAR * w0 / tab.E_CHARGE
    planck = tab.HBAR * w0 ** 3 / (4 * np.pi ** 3 * LIGHT ** 2) / np.expm1(e_ph / 25.0)
    t0 = got["tau"][0, 0]
    assert 20 < t0 < 80 and got["tau"][0, 3] == 0 and got["I"][0, 3] == 0
    assert abs(got["I"][0, 0] / planck - 1.0) <= np.exp(-t0) * (1 + 1e-6) + ref["bI"][0, 0] / planck
    assert abs(got["I"][0, 2] / planck - 1.0) <= np.exp(-got["tau"][0, 2]) * (1 + 1e-6) + ref["bI"][0, 2] / planck


@pytest.mark.gpu
def test_counter_streaming_halves_on_both_generations(eng):
    """10: a domain whose x < 0 half flows at +v along x and whose x > 0 half at -v shows two peaks 2 w0 v / c apart along an x
    chord, through ScalarDomain.sightline_lines() of both generations, and along the turned chord through rotated()."""
    from synthpy_amd import sightlines
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy import full_solver as fs
    from synthpy_amd.utils.eos_opacity import LineTable

    dims, cell, v = (16, 9, 11), 5e-4, 2.0e5
    lengths = tuple(cell * (m - 1) for m in dims)
    lines = LineTable([1.0, 500.0], [1e17, 1e21], np.full((2, 2), 4.0e9), wavelengths=250e-9, mass_number=12.011)
    w0 = lines.omega0[0]
    wd = lines.thermal_width(40.0)[0]
    assert w0 * v / LIGHT > 3 * wd  # the peaks are resolved
    om = w0 + wd * np.linspace(-12.0, 12.0, 193)
    x = np.linspace(-lengths[0] / 2, lengths[0] / 2, dims[0])
    V = np.zeros(dims + (3,), np.float32)
    V[..., 0] = np.where(x < 0, v, -v)[:, None, None]
    new = NewDomain(lengths, dims)
    old = fs.ScalarDomain(*[np.linspace(-L / 2, L / 2, m) for L, m in zip(lengths, dims)], lengths[2] / 2)
    for dom in (new, old):
        dom.external_ne(np.full(dims, 2e24, np.float32))
        dom.external_Te(30.0)
        dom.external_Z(2.0)
        dom.external_Ti(np.full(dims, 40.0, np.float32))
        dom.external_V(V)
    ch = sightlines.Chords([[-8e-3], [1e-4], [2e-4]], [[1.0], [0.0], [0.0]], -1)

    def peaks(sp):
        y = sp.intensity[0]
        top = [k for k in range(1, len(y) - 1) if y[k] > y[k - 1] and y[k] >= y[k + 1] and y[k] > 0.2 * y.max()]
        assert len(top) == 2, top
        return om[top[1]] - om[top[0]]

    for dom in (new, old):
        sp = dom.sightline_lines(ch, lines, wavelengths=2 * np.pi * LIGHT / om)
        assert isinstance(sp, sightlines.LineSpectra) and sp.intensity.shape == (1, 193) and sp.steps[0] > 0 and np.all(sp.optical_depth == 0)
        assert abs(peaks(sp) - 2 * w0 * v / LIGHT) <= 2 * (om[1] - om[0])  # a peak is found to within a frequency step
        M = sp.moments(12 * wd)
        assert abs(M["velocity"][0, 0]) < 0.05 * v  # the halves cancel in the centroid (the chord's halves differ by under a cell)
        assert M["Ti"][0, 0] > 5 * 40.0             # and the width is the streams', not the temperature's
        with pytest.raises(ValueError, match="exactly one"):
            dom.sightline_lines(ch, lines)
        with pytest.raises(ValueError, match="LineTable"):
            dom.sightline_lines(ch, object(), wavelengths=[250e-9])
        still = dom.sightline_lines(sightlines.Chords([[0.0], [-8e-3], [0.0]], [[0.0], [1.0], [0.0]], -1), lines, photon_energies=tab.HBAR * om / tab.E_CHARGE,
                                    continuum=True)
        assert np.all(still.optical_depth > 0) and abs(still.moments(12 * wd)["velocity"][0, 0]) < 1e-3 * v  # V is across this chord
    # the same plasma seen from a frame turned by 90 degrees about z: the flow turns with the grid, the turned chord sees the two peaks
    rot = new.rotated(90.0, about="z")
    assert rot.V.shape[-1] == 3 and np.abs(rot.V[..., 1]).max() > 0.9 * v
    sp = rot.sightline_lines(sightlines.Chords([[1e-4, 1e-4], [-8e-3, 8e-3], [2e-4, 2e-4]], [[0.0, 0.0], [1.0, -1.0], [0.0, 0.0]], -1), lines,
                             wavelengths=2 * np.pi * LIGHT / om)
    assert sp.steps.min() > 0
    for k in range(2):
        one = sightlines.LineSpectra(sightlines.Chords(np.zeros((3, 1)), np.ones((3, 1)), -1), sp.intensity[k:k + 1], sp.optical_depth[k:k + 1],
                                     sp.column[k:k + 1], sp.chord[k:k + 1], sp.steps[k:k + 1], sp.omega, lines)
        assert abs(peaks(one) - 2 * w0 * v / LIGHT) <= 2 * (om[1] - om[0])


@pytest.mark.gpu
def test_nan_nodes_poison_what_the_restatement_says(eng):
    """11a: a NaN node in ne, in Ti and in V makes NaN the elements the restatement makes NaN, and no other."""
    base = _case(CASES[next(k for k, c in enumerate(CASES) if c["ti"] and c["v"] and c["view"] == "six" and c["nf"] >= 70)])
    for name, at in (("ne", (4, 3, 3)), ("Ti", (3, 4, 3)), ("V", (4, 4, 3, 1))):
        F = dict(base["F"])
        a = np.array(F[name])
        a[at] = np.nan
        F[name] = a
        R = dict(base, F=F)
        ref = _restate(R)
        bad = np.isnan(ref["I"])
        assert 0 < bad.sum() < bad.size and not np.any(bad[ref["miss"]]), f"NaN in {name}: {bad.sum()} of {bad.size} elements"
        got = _run(eng, R)
        _assert_exact(got, ref, f"NaN node of {name}")
        _assert_close(got, ref, f"NaN node of {name}")
        assert np.array_equal(np.isnan(got["intensity"]), bad)
        assert np.isnan(got["column"]).any() == (name == "ne")
        if name != "ne":  # a NaN width or centre is never dropped: whole chords
            assert np.array_equal(bad, np.repeat(bad.any(axis=1)[:, None], bad.shape[1], axis=1))


@pytest.mark.gpu
def test_repeats_shuffles_optional_outputs_and_empties(eng, built, monkeypatch):
    """11b: a repeated call gives identical bits; a shuffled frequency list the same bits per frequency; each optional output can be
    asked for alone; n == 0 and n_freq == 0 succeed; the checks that need a live field."""
    R = _case(CASES[next(k for k, c in enumerate(CASES) if c["nl"] == 32 and c["nf"] == 257)])
    fields = _upload(eng, R)
    try:
        a, b = _run(eng, R, fields=fields), _run(eng, R, fields=fields)
        names = ("intensity", "optical_depth", "column", "chord", "steps")
        assert all(np.array_equal(a[k], b[k]) for k in names)
        _assert_close(a, R["ref"], "the repeated case")
        for order in (np.argsort(R["om"], kind="stable"), np.random.default_rng(3).permutation(len(R["om"]))):
            S = dict(R, om=R["om"][order], back=np.ascontiguousarray(R["back"][:, order]))
            s = _run(eng, S, fields=fields)
            assert np.array_equal(s["intensity"], a["intensity"][:, order]) and np.array_equal(s["optical_depth"], a["optical_depth"][:, order])
            assert all(np.array_equal(s[k], a[k]) for k in names[2:])
        for name in names[2:]:
            with monkeypatch.context() as m:  # an array the library does not write holds 0xA5 bytes, not a recycled buffer's
                m.setattr(np, "empty", _poisoned(np.empty))
                one = _run(eng, R, fields=fields, want=(name,))
            assert list(one) == [name] and one[name].dtype == a[name].dtype and np.array_equal(one[name], a[name]), name
        E = dict(R, o=np.zeros((3, 0)), d=np.zeros((3, 0)), back=np.zeros((0, len(R["om"]))))
        none = _run(eng, E, fields=fields, timed=False)
        assert none["intensity"].shape == (0, len(R["om"])) and none["steps"].shape == (0,)
        E = dict(R, om=np.zeros(0), back=np.zeros((R["o"].shape[1], 0)))
        none = _run(eng, E, fields=fields, timed=False)
        assert none["intensity"].shape == (R["o"].shape[1], 0) and none["column"].shape == (R["o"].shape[1],)
        # live fields: n_comp, dtype, grid
        ne, Te = fields[0], fields[1] if not isinstance(fields[1], float) else 30.0
        K = R["K"]
        vec = eng.Field(np.zeros(SHAPE + (3,), R["F"]["ne"].dtype), *K["co"])
        other = eng.Field(np.ones(SHAPE, np.float64 if R["F"]["ne"].dtype == np.float32 else np.float32), *K["co"])
        moved = eng.Field(np.ones(SHAPE, R["F"]["ne"].dtype), K["co"][0], K["co"][1], K["co"][2] + np.float32(1e-6))
        kw = dict(lines=R["lines"], omegas=R["om"], toward=1, step=R["step"], max_steps=5)
        try:
            for args, msg in (((ne, Te, vec, 2.0, None), "Ti must have n_comp == 1"), ((ne, Te, None, 2.0, ne), "V must have n_comp == 3"),
                              ((ne, Te, other, 2.0, None), "ne and Ti differ in dtype"), ((ne, Te, moved, 2.0, None), "grids of ne and Ti differ on axis 2")):
                with pytest.raises(built.SynthrayError, match=msg):
                    eng.sightline_lines(*args, R["o"], R["d"], **kw)
        finally:
            for f in (vec, other, moved):
                f.close()
    finally:
        _close(fields)
