"""Proton radiography through matter: sr_particles_push_matter (push_matter.hip), engine.push_particles_matter,
radiography.Material, radiograph(material=...), Radiograph.scatter_sigma / scattered / counts_in, and ScalarDomain.proton_radiograph
of both API generations with a material.

THE REFERENCE for values is `restate` below: include/synthray.h's rule in NumPy float64, operation for operation, on top of
tests/test_radiography.py's restatement of the push (whose helpers and shapes are imported, not copied).  +, *, / and sqrt are
correctly rounded on both sides; log is each side's library's, so bit equality is expected only where no particle meets matter and
is PRINTED everywhere.  What is ASSERTED are bounds counted from the roundings, in that file's units (u = 2^-53; one operation 1 u,
sqrt, / and log budgeted at 2 u), evaluated on the restatement's own magnitudes, never on the kernel's.

One side's error of the matter lines of ONE step, given u with the relative error rel = bu/|u| and xm with the error bx
(Wb = 54 kap + 33: a blended value's relative error in u, test_radiography.py; h the smallest cell width):
* uu 3 u, q 4 u, gn 5 u, un = sqrt(uu) 4 u, v = un/gn 11 u, v*v 23 u, ds 12 u; each also moves by its power of rel.
* the logarithms: aq 5 u; HW*sqrt(ne) carries Wb/2 + 3 u; the quotient 2 u more; log turns a relative error r of its argument into
  the absolute error r and adds 2 u |L|; b2 = q/(gn*gn) 17 u (b2 < 1); the difference 1 u |L|:  dL <= (Wb/2 + 27 + 3 Lmax) u + 2 rel,
  Lmax the largest |log| met.
* nb = (ne*dz+)/Z: dz = Zn - Z errs by (Wb Z + dz) u, so dnb <= nb (2 Wb + 4) u + ne Wb u.
* N = ne*Lf+ + nb*Lb+ (every term positive; clamping at 0 is continuous): with Nscale = (ne + nb) max(Lmax, 1) >= N,
  dN <= [N (2 Wb + 5) + ne Wb Lmax + (ne + nb)(Wb/2 + 27 + 3 Lmax)] u <= Nscale (3.5 Wb + 35) u  (+ 2 rel Nscale from the logs).
* a = ((S/mass)*dt)/un with S = (KS/(v*v))*N: 23 + 2 + 1 + 2 + 1 + 2 + 4 = 35 u relative, and a ~ |u|^-3 moves by 3 rel:
  da <= a_scale [(3.5 Wb + 70) u + 6 rel + P],  a_scale = KS/(v*v) * Nscale / mass * dt / un  (>= a),
  P = 2 sqrt(3) (bx/h) (2 NEmax/ne + 2 Zmax/Z): what the error of xm changes ne and Z by (their largest nodes over the local value:
  near an edge of the matter the relative change is large and the absolute one is not).
* fac = 1 - a: da + 1 u;  u_a*fac: one more.  bu' = bu + |u| (da + 2 u);  the energy (mc2*q)/(gn + 1): 2 rel + 20 u relative.
* Ts = (KT*(ne/Z))/(pv*pv): ne/Z 2 Wb + 2, pv 6 u, squared 13 u, the quotient 2, KT* 1: (2 Wb + 18) u + 4 rel + P/2; t = Ts*ds adds
  13 u + rel:  relT = (2 Wb + 31) u + 5 rel + P/2.  s errs by bs' = bs + ds (12 u + rel) + s u; sm = s + 0.5 ds by bs + 1 u sm.
  M0 += t: t relT + M0 u;  M1 += t*sm: t sm (relT + bs/sm + 2 u) + M1 u;  M2 += (t*sm)*sm: t sm^2 (relT + 2 bs/sm + 4 u) + M2 u.
Two sides: twice these.  Over a path the bounds are carried by the recurrence above next to the restatement itself (`restate`
returns them per particle): bu also takes the push's own one-step du (test_radiography._scales, both sides already in it) and what bx
changes E and B by, hq 2 sqrt(3) (2 FE + 3 U FB) bx/h; bx takes 2 * 18 u X + dt bu per step.  The drag's factor 1 + 6 a_scale per step
is the Bragg peak: a slowing particle's error grows like (u_0/u)^6, which the recurrence follows step by step.
A particle is BORDERLINE when at some step a threshold lies within its bound: the energy after the drag within its bound of
stop_energy, fac within da of 0, a coordinate of x within bx of a face of the box, or a coordinate of xm within bx of a node plane
(the cell, and with it a NaN or zero node, may then differ).  Borderline particles are excused from the equality of decisions,
must still be within the bound up to the step where the restatement decided, and are at most 1 % -- of the restatement alone, so
the seed cannot be chosen by the kernel.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import test_radiography as tr
from conftest import ROOT

EPS, LIGHT, IC2, QM_P = tr.EPS, tr.LIGHT, tr.IC2, tr.QM_P
AX, AX32, DT, N_PART = tr.AX, tr.AX32, tr.DT, tr.N_PART
UNFINISHED, MISSED, STOPPED = 1, 2, 4
M_P = 1.67262192369e-27
E_CH, M_E, EPS0, HBAR, PI = 1.602176634e-19, 9.1093837015e-31, 8.8541878128e-12, 1.054571817e-34, 3.141592653589793
MEV = 1e6 * E_CH
SHAPE = tuple(len(a) for a in AX)
H_MIN = min(float(np.min(np.diff(a))) for a in AX)
AL = dict(Zn=13.0, I=166.0 * E_CH, lnLs=float(np.log(204.0 * 13.0 ** (-1.0 / 3.0))))  # aluminium (radiography.Material.Al)


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
def consts(qm, dt, mass, z, Zn, I, lnLs, Z=0.0, stop=0.0):
    """The host's constants, each formed as the header writes it."""
    e2 = E_CH * E_CH
    ze = (z * e2) / ((4.0 * PI) * EPS0)
    return dict(hq=(qm * dt) * 0.5, hd=dt * 0.5, dt=dt, mass=mass, mc2=mass * (LIGHT * LIGHT), A2=(2.0 * M_E) * (LIGHT * LIGHT),
                HW=HBAR * np.sqrt(e2 / (EPS0 * M_E)), I=I, Zn=Zn, Zu=Z, KS=((z * z) * (e2 * e2)) / ((((4.0 * PI) * EPS0) * EPS0) * M_E),
                KT=(((8.0 * PI) * (Zn * (Zn + 1.0))) * (ze * ze)) * lnLs, stop=stop, qm=qm)


def _gather1(F, axes, xm):
    """(N) float64: a scalar field's blend of sr_field_resample's rule at xm (3, N), fill 0."""
    (ci, wx, ix), (cj, wy, iy), (ck, wz, iz) = (tr._locate(axes[a], xm[a]) for a in range(3))
    inside = ix & iy & iz
    ux, uy, uz = 1.0 - wx, 1.0 - wy, 1.0 - wz
    w00, w01, w10, w11 = uy * uz, uy * wz, wy * uz, wy * wz
    f = lambda di, dj, dk: np.float64(F[ci + di, cj + dj, ck + dk])
    s = [((f(di, 0, 0) * w00 + f(di, 0, 1) * w01) + f(di, 1, 0) * w10) + f(di, 1, 1) * w11 for di in (0, 1)]
    return np.where(inside, ux * s[0] + wx * s[1], 0.0)


def restate_step(s, path, E, B, ne, Z, axes, K, bounds=None):
    """One step of the rule on the states s (6, N) and paths (4, N: M0, M1, M2, s): (states, paths, stopped).  E, B, Z: arrays or
    None.  bounds: a dict with bu, bx, bs, bM (3, N), b_T and `border` (N) that the recurrence of the docstring updates in place,
    and the scales du1, dx1 (the push's one-step bounds), X, kap, fe, fb, U, ne_max, z_max."""
    with np.errstate(all="ignore"):
        x, u = s[:3], s[3:]
        hq, hd, dt = K["hq"], K["hd"], K["dt"]
        g = np.sqrt(1.0 + tr._n2(u) * IC2)
        xm = x + u * (hd / g)
        Ev = None if E is None else tr._gather(E, axes, xm)
        Bv = None if B is None else tr._gather(B, axes, xm)
        nev = _gather1(ne, axes, xm)
        Zv = np.full(s.shape[1], K["Zu"]) if Z is None else _gather1(Z, axes, xm)
        um = u if Ev is None else u + hq * Ev
        if Bv is None:
            up = um
        else:
            gm = np.sqrt(1.0 + tr._n2(um) * IC2)
            t = (hq / gm) * Bv
            sv = t * (2.0 / (1.0 + tr._n2(t)))
            w = um + tr._cross(um, t)
            up = um + tr._cross(w, sv)
        un3 = up if Ev is None else up + hq * Ev
        uu = tr._n2(un3)
        q = uu * IC2
        gn = np.sqrt(1.0 + q)
        un = np.sqrt(uu)
        v = un / gn
        ds = v * dt
        matter = (nev > 0.0) & (Zv > 0.0)
        rest = matter & ~(uu > 0.0)
        sc = matter & ~rest
        M0, M1, M2, sp = path
        pv = (K["mass"] * uu) / gn
        Ts = (K["KT"] * (nev / Zv)) / (pv * pv)
        sm = sp + 0.5 * ds
        tt = Ts * ds
        M0n = np.where(sc, M0 + tt, M0)
        M1n = np.where(sc, M1 + tt * sm, M1)
        M2n = np.where(sc, M2 + (tt * sm) * sm, M2)
        spn = sp + ds
        aq, b2 = K["A2"] * q, q / (gn * gn)
        Lf = np.log(aq / (K["HW"] * np.sqrt(nev))) - b2
        Lb = np.log(aq / K["I"]) - b2
        dz = K["Zn"] - Zv
        nb = (nev * np.where(dz > 0.0, dz, 0.0)) / Zv
        Nn = nev * np.where(Lf > 0.0, Lf, 0.0) + nb * np.where(Lb > 0.0, Lb, 0.0)
        S = (K["KS"] / (v * v)) * Nn
        fac = 1.0 - ((S / K["mass"]) * dt) / un
        moves = fac > 0.0
        ud = np.where(sc, np.where(moves, un3 * fac, 0.0), un3)
        qd = tr._n2(ud) * IC2
        gd = np.sqrt(1.0 + qd)
        Td = (K["mc2"] * qd) / (gd + 1.0)
        stopped = rest | (sc & (~moves | (Td < K["stop"])))
        xn = np.where(stopped, xm, xm + ud * (hd / gd))
        if bounds is not None:
            b = bounds
            Wb = 54.0 * b["kap"] + 33.0
            unorm = np.where(un > 0, un, 1.0)
            bu_f = b["bu"] + b["du1"] + abs(hq) * 2 * np.sqrt(3) * (2 * b["fe"] + 3 * b["U"] * b["fb"]) * b["bx"] / H_MIN
            rel = bu_f / unorm
            P = np.where(sc, 2 * np.sqrt(3) * (b["bx"] / H_MIN) * (2 * b["ne_max"] / nev + 2 * b["z_max"] / Zv), 0.0)
            Lmax = np.where(sc, np.maximum(1.0, np.maximum(np.abs(Lf + b2), np.abs(Lb + b2))), 1.0)
            a_scale = np.where(sc, (K["KS"] / (v * v)) * ((nev + nb) * Lmax) / K["mass"] * dt / unorm, 0.0)
            da = a_scale * (2 * (3.5 * Wb + 70.0) * EPS + 6 * rel + P)
            bu_n = bu_f + np.where(sc, un * (da + 4 * EPS), 0.0)
            nd = np.sqrt(tr._n2(ud))
            bT = np.where(sc, Td * (2 * bu_n / np.where(nd > 0, nd, 1.0) + 40 * EPS), 0.0)
            relT = 2 * (2 * Wb + 31.0) * EPS + 5 * rel + P / 2
            bs = b["bs"]
            smn = np.where(sm > 0, sm, 1.0)
            b["bM"][0] += np.where(sc, tt * relT + 2 * EPS * M0n, 0.0)
            b["bM"][1] += np.where(sc, tt * sm * (relT + bs / smn + 4 * EPS) + 2 * EPS * M1n, 0.0)
            b["bM"][2] += np.where(sc, tt * sm * sm * (relT + 2 * bs / smn + 8 * EPS) + 2 * EPS * M2n, 0.0)
            b["bs"] = bs + ds * (24 * EPS + rel) + 2 * EPS * spn
            bx_m = b["bx"] + 18 * EPS * b["X"] + hd * bu_f  # of xm
            bx_n = bx_m + 18 * EPS * b["X"] + hd * bu_n
            near_node = np.zeros(s.shape[1], bool)
            near_face = np.zeros(s.shape[1], bool)
            for a in range(3):
                near_node |= np.min(np.abs(xm[a][None, :] - axes[a][:, None]), axis=0) <= bx_m
                near_face |= (np.abs(xn[a] - axes[a][0]) <= bx_n) | (np.abs(xn[a] - axes[a][-1]) <= bx_n)
            b["border"] |= near_node | (near_face & ~stopped) | (sc & (np.abs(fac) <= da)) | (sc & moves & (np.abs(Td - K["stop"]) <= bT))
            b["bu"], b["bx"], b["b_T"] = bu_n, np.where(stopped, bx_m, bx_n), bT
    return np.concatenate([xn, ud]), np.stack([M0n, M1n, M2n, spn]), stopped


def start_bounds(n, s0, E, B, ne, Z, K):
    du1, dx1 = tr._scales(s0, E, B, K["qm"], K["dt"]) if (E is not None or B is not None) else (0.0, 0.0)
    X = max(float(np.max(np.abs(a))) for a in AX) + LIGHT * K["dt"]
    hq = abs(K["hq"])
    fe = 0.0 if E is None else float(np.max(np.abs(E)))
    fb = 0.0 if B is None else float(np.max(np.abs(B)))
    U = float(np.nanmax(np.sqrt(np.sum(s0[3:] ** 2, axis=0)))) + 2 * hq * np.sqrt(3) * fe
    return dict(bu=np.zeros(n), bx=np.zeros(n), bs=np.zeros(n), bM=np.zeros((3, n)), b_T=np.zeros(n), border=np.zeros(n, bool),
                du1=du1, X=X, kap=X / H_MIN, fe=fe, fb=fb, U=U, ne_max=float(np.nanmax(ne)),
                z_max=K["Zu"] if Z is None else float(np.nanmax(Z)))


def restate(s0, E, B, ne, Z, axes, K, max_steps, axis, det_pos, hit_scale, with_bounds=True):
    """The whole rule: a dict with sf, hits, steps, flags, energy, moments and, per particle, the bounds of the docstring."""
    s = np.array(s0, np.float64)
    n = s.shape[1]
    path = np.zeros((4, n))
    steps, active, stopped = np.zeros(n, np.int32), np.arange(n), np.zeros(n, bool)
    full = start_bounds(n, s0, E, B, ne, Z, K) if with_bounds else None
    per = ("bu", "bx", "bs", "b_T", "border")
    for _ in range(max_steps):
        b = None
        if with_bounds:
            b = {**full, **{k: full[k][active] for k in per}, "bM": full["bM"][:, active]}
        s[:, active], path[:, active], st = restate_step(s[:, active], path[:, active], E, B, ne, Z, axes, K, b)
        if with_bounds:
            for k in per:
                full[k][active] = b[k]
            full["bM"][:, active] = b["bM"]
        steps[active] += 1
        stopped[active] = st
        active = active[tr._inside(s[:, active], axes) & ~st]
        if not len(active):
            break
    hits, flags = tr._detector(s, axis, det_pos, hit_scale)
    flags[active] |= UNFINISHED
    flags[stopped] |= STOPPED
    with np.errstate(all="ignore"):
        q = tr._n2(s[3:]) * IC2
        energy = (K["mc2"] * q) / (np.sqrt(1.0 + q) + 1.0)
    return dict(sf=s, hits=hits, steps=steps, flags=flags, energy=energy, moments=path, bounds=full)


# ---------------------------------------------------------------- inputs
def _matter(dtype, with_nan=True):
    """ne: 2e30 m^-3 (2.5 x solid aluminium, so that 14.7 MeV protons stop within the box) filling x >= node 5 -- the edge lies
    inside the cell row 4..5, where the blend ramps from 0 -- with a vacuum channel, and one NaN node; Z: 3 with a block of zeros
    (matter skipped) and a block of 15 > Zn (no bound electrons)."""
    ne = np.zeros(SHAPE)
    ne[5:, :, :] = 2e30
    ne[7:9, 2:4, :] = 0.0
    if with_nan:
        ne[9, 6, 4] = np.nan
    Z = np.full(SHAPE, 3.0)
    Z[6:8, 5:8, 2:5] = 0.0
    Z[9:, :4, :] = 15.0
    return ne.astype(dtype), Z.astype(dtype)


def _particles(seed=5):
    """test_radiography's 1037 states (nodes, faces, midpoints outside, starts outside, NaN, slow) with 20 more made slow enough to stop
    on their first step in matter (47 keV) and 20 at 1 MeV."""
    s, k = tr._particles(seed)
    # the ones that sit exactly on nodes and faces are moved off them: on a node plane every one of them would be borderline by
    # the definition above (test 1 keeps them where they are, and there the bits are asserted)
    s[:3, k["nodes"]] += np.array([3e-5, -2e-5, 1.5e-5])[:, None] * np.where(k["nodes"] == 2, -1.0, 1.0)
    s[:3, k["faces"]] *= 1.0 - 1e-3
    k["first"] = np.arange(60, 80)
    s[3:, k["first"]] *= 3e6 / 5.4e7
    k["mev"] = np.arange(80, 100)
    s[3:, k["mev"]] *= 1.38e7 / 5.4e7
    return s, k


def _push(eng, E, B, ne, Z, s0, max_steps, stop=0.0, axis=2, det_pos=0.1, hit_scale=1e3, image=None, dt=DT, mat=AL, uniform_Z=3.0, **kw):
    f = {name: None if a is None else eng.Field(a, *AX32) for name, a in (("E", E), ("B", B), ("ne", ne), ("Z", Z))}
    try:
        return eng.push_particles_matter(f["E"], f["B"], f["ne"], f["Z"] if Z is not None else uniform_Z, s0, QM_P, dt, max_steps, axis,
                                         det_pos, hit_scale, mass=M_P, z=1.0, stop_energy=stop, image=image, **mat, **kw)
    finally:
        for h in f.values():
            if h is not None:
                h.close()


# ================================================================ tests without a device
def test_header_ctypes_and_python_signatures(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "synthray.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sr_particles_push_matter\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 15
    assert re.search(r"#define\s+SR_PUSH_STOPPED\s+4", text) and built.PUSH_STOPPED == 4
    p = re.search(r"typedef struct \{([^}]*)\}\s*sr_push_matter_params;", text).group(1)
    assert re.findall(r"(\w+);", p) == [n for n, _ in built.PushMatterParams._fields_] == ["push", "mass", "z", "Zn", "I", "lnLs", "Z", "stop_energy"]
    assert C.sizeof(built.PushMatterParams) == C.sizeof(built.PushParams) + 7 * 8 and built.PushMatterParams.mass.offset == 40
    st = re.search(r"typedef struct \{([^}]*)\}\s*sr_push_matter_stats;", text).group(1)
    assert re.findall(r"(\w+)[,;]", st) == [n for n, _ in built.PushMatterStats._fields_]
    assert C.sizeof(built.PushMatterStats) == 8 + 5 * 8 and C.sizeof(built.PushStats) == 8 + 4 * 8
    res, args = built.SYMBOLS["sr_particles_push_matter"]
    assert res is C.c_int and len(args) == 15 and args[5] is C.c_int64 and hasattr(built.lib, "sr_particles_push_matter")
    mk = open(os.path.join(ROOT, "synthpy_amd", "csrc", "Makefile")).read()
    assert "push_matter.hip" in mk and "push_blend.inc" in mk

    from synthpy_amd import engine, radiography
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy.full_solver import ScalarDomain as OldDomain

    names = lambda f: list(inspect.signature(f).parameters)
    assert names(engine.push_particles_matter)[:11] == ["E", "B", "ne", "Z", "s0", "qm", "dt", "max_steps", "axis", "det_pos", "hit_scale"]
    assert names(radiography.radiograph)[-3:] == ["material", "stop_energy_MeV", "scatter_seed"]
    assert names(NewDomain.proton_radiograph) == names(OldDomain.proton_radiograph)


def test_argument_checks_come_before_the_device(built):
    from synthpy_amd import engine

    lib, ptr = built.lib, built.ptr
    s0 = np.zeros((6, 4))

    def call(p, n=4, s=s0):
        return lib.sr_particles_push_matter(None, None, None, None, None if p is None else C.byref(p), n, ptr(s), None, None, None, None,
                                            None, None, None, None)

    base = dict(qm=QM_P, dt=1e-12, max_steps=4, axis=2, det_pos=0.1, mass=M_P, z=1.0, Zn=13.0, I=2.7e-17, lnLs=4.0, Z=3.0)
    good = lambda **kw: engine.push_matter_params(**{**base, **kw})
    assert call(None) == -1 and "NULL" in built.last_error()
    assert call(good(), s=None) == -1 and "NULL" in built.last_error()
    assert call(good(), n=-1) == -1 and "n must not be negative" in built.last_error()
    for name, bads in (("dt", (0.0, -1e-12, np.nan, np.inf)), ("qm", (np.nan, np.inf)), ("det_pos", (np.nan,)), ("hit_scale", (np.inf,)),
                       ("max_steps", (0, -3)), ("axis", (3, -1)), ("mass", (0.0, -1.0, np.nan, np.inf)), ("z", (np.nan, np.inf)),
                       ("Zn", (0.0, np.nan)), ("I", (0.0, -1.0, np.inf)), ("lnLs", (-1.0, np.nan)), ("stop_energy", (-1.0, np.nan)),
                       ("Z", (0.0, -2.0, np.nan))):
        for bad in bads:
            assert call(good(**{name: bad})) == -1 and name in built.last_error(), (name, bad, built.last_error())
    assert call(good()) == -1 and "ne is NULL" in built.last_error()  # every other argument was in order; E = B = NULL is allowed
    assert "sr_particles_push_matter" in built.last_error()
    kw = dict(mass=M_P, z=1.0, Zn=13.0, I=2.7e-17, lnLs=4.0)
    with pytest.raises(ValueError, match="Field"):
        engine.push_particles_matter(None, None, np.zeros((2, 2, 2)), 3.0, s0, QM_P, 1e-12, 4, 2, 0.1, **kw)
    with pytest.raises(ValueError, match="want"):
        engine.push_particles_matter(None, None, None, 3.0, s0, QM_P, 1e-12, 4, 2, 0.1, want=("rf",), **kw)


def test_material_defaults(built):
    from synthpy_amd.radiography import AMU, Material

    for Zn in (3.5, 13.0, 74.0):
        m = Material(Zn, 2 * Zn, 100.0)
        assert m.coulomb_log == float(np.log(204.0 * Zn ** (-1.0 / 3.0))) and m.I == 100.0 * E_CH
    assert Material(13, 27, 166, coulomb_log=5.0).coulomb_log == 5.0
    al, ch, cu, w = Material.Al(), Material.CH(), Material.Cu(), Material.W()
    assert (al.Zn, al.I_eV) == (13.0, 166.0) and (cu.Zn, cu.I_eV) == (29.0, 322.0) and (w.Zn, w.I_eV) == (74.0, 727.0)
    assert (ch.Zn, ch.I_eV) == (3.5, 68.7) and (al.Zn, al.I, al.coulomb_log) == (AL["Zn"], AL["I"], AL["lnLs"])
    assert abs(al.electron_density(2699.0) / 7.83e29 - 1) < 2e-3  # solid aluminium: 13 electrons per atom, 6.02e28 atoms/m^3
    assert al.electron_density(2699.0, Z=3.0) == 2699.0 * 3.0 / (al.A * AMU)
    for bad in (dict(Zn=0), dict(A=-1), dict(I_eV=np.nan), dict(coulomb_log=-1.0)):
        with pytest.raises(ValueError):
            Material(**{**dict(Zn=13, A=27, I_eV=166), **bad})


def _slab_radiograph(n, Ts, t, d, seed=0):
    """A hand-made Radiograph: n particles that crossed a uniform slab of thickness t (scattering power Ts, no energy loss) along
    directions inside a cone about z and then drift d along their flight to the plane z = det."""
    from synthpy_amd.radiography import Radiograph

    rng = np.random.default_rng(seed)
    th, ph = 0.3 * rng.random(n), 2 * np.pi * rng.random(n)
    nh = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    det = 0.05
    x = np.stack([1e-3 * rng.standard_normal(n), 1e-3 * rng.standard_normal(n), np.zeros(n)])
    x[2] = det - d * nh[2]  # d along the flight from the exit point to the plane
    sf = np.concatenate([x, 5e7 * nh])
    moments = np.stack([np.full(n, Ts * t), np.full(n, Ts * t * t / 2), np.full(n, Ts * t ** 3 / 3), np.full(n, t)])
    from synthpy_amd import radiography

    hits, missed = radiography.project(sf, 2, det, 1e3)
    edges = (np.linspace(-50, 50, 33), np.linspace(-50, 50, 33))
    return Radiograph(None, edges, hits, np.zeros(n, np.uint8), np.ones(n, np.int32), sf, 1.0, None, hits, 1e-12, 1, energy_MeV=np.full(n, 14.7),
                      moments=moments, axis=2, det_pos=det, hit_scale=1e3), nh


def test_scatter_sigma_against_the_slab(built):
    """A uniform slab of thickness t followed by a drift d: sigma_theta^2 = Ts t/2, sigma_y^2 = Ts (t^3/3 + t^2 d + t d^2)/2.
    scatter_sigma forms L^2 M0 - 2 L M1 + M2 with L = t + d: three terms of magnitude <= Ts t L^2 that cancel down to the closed
    form, >= Ts t L^2/3 -- so 3 * (about 12 roundings) u relative; 64 u is asserted."""
    Ts, t, d = 3.0e-2, 2.0e-3, 0.04
    rad, _ = _slab_radiograph(500, Ts, t, d)
    st, sy = rad.scatter_sigma()
    assert np.all(np.abs(st ** 2 - Ts * t / 2) <= 8 * EPS * Ts * t)
    want = Ts * (t ** 3 / 3 + t * t * d + t * d * d) / 2
    print(f"slab: sigma_theta {st[0]:.4e} rad, sigma_y {sy[0]:.4e} m; max rel error of sigma_y^2 {float(np.max(np.abs(sy ** 2 - want)) / want):.2e}")
    assert np.all(np.abs(sy ** 2 - want) <= 64 * EPS * want)
    from synthpy_amd.radiography import Radiograph

    plain = Radiograph(None, rad.edges, rad.hits, rad.flags, rad.steps, rad.sf, 1.0, None, rad.hits, 1e-12, 1)
    assert plain.moments is None and plain.stopped is None and plain.energy_MeV is None
    with pytest.raises(ValueError, match="material"):
        plain.scatter_sigma()


def test_scattered_hits_are_seeded_normals(built):
    """scattered_hits(seed): reproducible; the displacement perpendicular to the flight has the variance sigma_y^2 in both
    directions.  With n = 20000 draws of a normal the sample variance has the standard error sigma^2 sqrt(2/n) = 1 % of sigma^2;
    5 standard errors (a chance of 6e-7 per direction) are allowed, and the mean is within 5 sigma/sqrt(n)."""
    n = 20000
    Ts, t, d = 3.0e-2, 2.0e-3, 0.04
    rad, nh = _slab_radiograph(n, Ts, t, d, seed=4)
    h1, h2, h3 = rad.scattered_hits(7), rad.scattered_hits(7), rad.scattered_hits(8)
    assert np.array_equal(h1, h2) and not np.array_equal(h1, h3) and h1.shape == (2, n)
    sig = float(np.sqrt(Ts * (t ** 3 / 3 + t * t * d + t * d * d) / 2))
    # the shift in the plane, D = d - n^ d_z/n_z with d perpendicular to n^, gives d back as d = D - n^ (n^ . D) (D_z = 0)
    D = np.concatenate([(h1 - rad.hits) / 1e3, np.zeros((1, n))])
    dperp = D - nh * np.sum(nh * D, axis=0)
    e1 = -nh[0] * nh
    e1[0] += 1.0
    e1 /= np.sqrt(np.sum(e1 * e1, axis=0))
    e2 = np.cross(nh, e1, axis=0)
    for e in (e1, e2):
        comp = np.sum(dperp * e, axis=0)
        print(f"scattered: sample variance / sigma_y^2 = {float(np.var(comp) / sig ** 2):.4f}, mean / sigma_y = {float(np.mean(comp) / sig):+.4f}")
        assert abs(np.var(comp) / sig ** 2 - 1.0) <= 5 * np.sqrt(2.0 / n) and abs(np.mean(comp)) <= 5 * sig / np.sqrt(n)
    assert abs(np.mean(np.sum(dperp * e1, axis=0) * np.sum(dperp * e2, axis=0))) <= 5 * sig ** 2 / np.sqrt(n)  # independent


def test_restatement_borderline_share_on_the_cpu():
    """The seed's choice, made without the kernel: the restatement's own borderline particles are under the 1 % cap, and the
    restatement run again on states perturbed by ten times the one-step bound takes the same decisions outside them."""
    for dtype in (np.float64, np.float32):
        C_ = _whole_case(dtype)
        ref = C_["ref"]
        assert ref["bounds"]["border"].mean() <= 0.01, ref["bounds"]["border"].sum()
        rng = np.random.default_rng(1)
        s1 = C_["s0"] * (1.0 + 10 * 64 * EPS * rng.uniform(-1, 1, C_["s0"].shape))
        pert = restate(s1, C_["E"], C_["B"], C_["ne"], C_["Z"], AX, C_["K"], 64, 2, 0.1, 1e3, with_bounds=False)
        differ = (pert["flags"] != ref["flags"]) | (pert["steps"] != ref["steps"])
        exact = np.zeros(N_PART, bool)  # hand-made particles sitting exactly on faces and nodes are moved off them by the perturbation
        exact[:30] = True
        assert (differ & ~exact).mean() <= 0.01, np.nonzero(differ & ~exact)[0]


_CASES = {}


def _whole_case(dtype):
    """The whole-path case of test 2, restated once per dtype: weak E and B (as test_radiography's test 5c, so that the fields'
    own error growth stays below e), the matter of _matter, stop_energy 0.5 MeV, 64 steps."""
    key = np.dtype(dtype).name
    if key not in _CASES:
        rng = np.random.default_rng(31)
        E = (2e7 * np.clip(rng.standard_normal(SHAPE + (3,)), -4, 4)).astype(dtype)
        B = (0.5 * np.clip(rng.standard_normal(SHAPE + (3,)), -4, 4)).astype(dtype)
        ne, Z = _matter(dtype)
        s0, k = _particles()
        K = consts(QM_P, DT, M_P, 1.0, AL["Zn"], AL["I"], AL["lnLs"], stop=0.5 * MEV)
        _CASES[key] = dict(E=E, B=B, ne=ne, Z=Z, s0=s0, k=k, K=K, ref=restate(s0, E, B, ne, Z, AX, K, 64, 2, 0.1, 1e3))
    return _CASES[key]


# ================================================================ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("which", ["none", "E", "B", "EB"])
def test_no_matter_is_the_plain_push(eng, which, dtype):
    """1: ne = 0 everywhere (Z uniform and a Z field), and ne > 0 with every gather skipped (Z = 0 everywhere; ne NaN everywhere):
    sf, hits, steps, flags are engine.push_particles' bits; nobody stops, the moments stay 0, the path length is the steps' sum.
    Without E and B there is no plain push to compare with: the restatement of the push without fields stands in."""
    E, B = tr._fields(dtype)
    E, B = (E if "E" in which else None), (B if "B" in which else None)
    s0, k = tr._particles()
    if which == "none":
        rs, rh, rsteps, rflags = tr.restate(s0, None, None, AX, QM_P, DT, 64, 2, 0.1, 1e3)
        plain = dict(sf=rs, hits=rh, steps=rsteps, flags=rflags)
    else:
        plain = tr._push(eng, E, B, s0, QM_P, DT, 64)
    zero, full = np.zeros(SHAPE, dtype), np.full(SHAPE, 2e30, dtype)
    for name, ne, Z in (("ne = 0, uniform Z", zero, None), ("ne = 0, Z field", zero, np.full(SHAPE, 3.0, dtype)),
                        ("Z = 0", full, zero), ("ne NaN", np.full(SHAPE, np.nan, dtype), None)):
        out = _push(eng, E, B, ne, Z, s0, 64, stop=0.5 * MEV)
        same = {n: np.array_equal(out[n], plain[n], equal_nan=True) for n in ("sf", "hits", "steps", "flags")}
        print(f"{which} {np.dtype(dtype).name}, {name}: bit-equal to the plain push {same}")
        assert all(same.values()), (name, same)
        assert out["stats"].stopped == 0 and np.all(out["moments"][:3] == 0.0)
        assert np.all(out["moments"][3] >= 0.0)  # every u is finite, so every path length is
        q = np.sum(out["sf"][3:] ** 2, axis=0) * IC2
        want = (M_P * LIGHT * LIGHT * q) / (np.sqrt(1.0 + q) + 1.0)
        assert np.all(np.abs(out["energy"] - want) <= 16 * EPS * want)


def _assert_against(out, ref, n_steps, who):
    """Decisions equal outside the borderline particles; values within the carried bounds (both sides already in them)."""
    b = ref["bounds"]
    border = b["border"]
    sure = ~border
    assert border.mean() <= 0.01, f"{who}: {border.sum()} borderline particles"
    for name in ("steps", "flags"):
        bad = np.nonzero((out[name] != ref[name]) & sure)[0]
        assert not len(bad), (who, name, bad[:10], out[name][bad[:10]], ref[name][bad[:10]])
    assert np.array_equal(np.isnan(out["sf"][:, sure]), np.isnan(ref["sf"][:, sure]))
    same_path = sure | (out["steps"] == ref["steps"])  # a borderline particle that took the same decisions is held to the bound too
    ok = ~np.isnan(ref["sf"]).any(axis=0) & same_path
    fx, fu = 3.0, 3.0  # the fields' own growth over the path (test_radiography's 5c), on top of the recurrence
    d = np.abs(out["sf"] - ref["sf"])[:, ok]
    bx, bu = fx * b["bx"][ok] + 18 * EPS * b["X"], fu * b["bu"][ok] + 8 * EPS * np.sqrt(np.sum(ref["sf"][3:, ok] ** 2, axis=0))
    bT = ref["energy"][ok] * (2 * bu / np.maximum(np.sqrt(np.sum(ref["sf"][3:, ok] ** 2, axis=0)), 1e-300) + 40 * EPS)
    dT = np.abs(out["energy"] - ref["energy"])[ok]
    dM = np.abs(out["moments"] - ref["moments"])[:, ok]
    bM = np.concatenate([fu * b["bM"][:, ok], (fu * b["bs"][ok])[None, :]]) + 8 * EPS * np.abs(ref["moments"][:, ok])
    with np.errstate(all="ignore"):
        ratio = lambda dd, bb: float(np.nanmax(np.where(bb > 0, dd / bb, 0.0)))
        print(f"{who}: {int(border.sum())} borderline of {len(border)}; bit-equal sf {np.array_equal(out['sf'], ref['sf'], equal_nan=True)}, "
              f"energy {np.array_equal(out['energy'], ref['energy'], equal_nan=True)}, moments "
              f"{np.array_equal(out['moments'], ref['moments'], equal_nan=True)}; max |dx| / bound {ratio(d[:3], bx):.3g}, |du| {ratio(d[3:], bu):.3g}, "
              f"|dT| {ratio(dT, bT):.3g}, |dM| {ratio(dM, bM):.3g}; largest bounds: dx {float(bx.max()):.2e} m, du/|u| "
              f"{float(np.max(bu / np.maximum(np.sqrt(np.sum(ref['sf'][3:, ok] ** 2, axis=0)), 1.0))):.2e}")
    assert np.all(d[:3] <= bx) and np.all(d[3:] <= bu) and np.all(dT <= bT) and np.all(dM <= bM)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("which", ["none", "E", "B", "EB"])
def test_one_step_against_restatement(eng, which, dtype):
    """2a: max_steps = 1 for every instantiation with a Z field (and, for EB, with the uniform Z): strong random fields, the edge
    of the matter inside a cell row (wavefronts mix matter and vacuum), a NaN node, Z = 0 and Z > Zn blocks, particles that stop
    on their first step, slow ones, and ones that start outside."""
    E, B = tr._fields(dtype)
    E, B = (E if "E" in which else None), (B if "B" in which else None)
    ne, Z = _matter(dtype)
    s0, k = _particles()
    for Zf in ((Z, None) if which == "EB" else (Z,)):
        K = consts(QM_P, DT, M_P, 1.0, AL["Zn"], AL["I"], AL["lnLs"], Z=3.0, stop=0.5 * MEV)
        ref = restate(s0, E, B, ne, Zf, AX, K, 1, 2, 0.1, 1e3)
        out = _push(eng, E, B, ne, Zf, s0, 1, stop=0.5 * MEV)
        stopped = (ref["flags"] & STOPPED) > 0
        in_matter = ref["moments"][0] > 0
        # the inputs do what they were made for: matter and vacuum inside one wavefront, first-step stops, no matter outside the box
        waves = in_matter[:1024].reshape(16, 64).sum(axis=1)
        assert np.all((waves > 0) & (waves < 64)) and 40 <= stopped.sum() < 400 and in_matter.sum() > 300
        if which in ("none", "B"):
            assert stopped[k["first"]].sum() >= 5 and not in_matter[k["outside"][4:]].any() and not in_matter[k["nan"]].any()
        assert np.all(ref["steps"] == 1) and np.array_equal(out["steps"], ref["steps"])
        assert not np.any(ref["flags"][stopped] & UNFINISHED)
        _assert_against(out, ref, 1, f"one step, {which} {np.dtype(dtype).name}, Z {'field' if Zf is not None else 'uniform'}")
        st = out["stats"]
        assert st.stopped == int(((out["flags"] & STOPPED) > 0).sum()) and st.finished + st.unfinished == N_PART and st.kernel_ms > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_whole_paths_against_restatement(eng, dtype):
    """2b: 64 steps through weak E and B and the matter of _matter with stop_energy = 0.5 MeV: some particles stop inside, some
    leave, some are still inside -- asserted from the restatement -- and the kernel's loop is its own step composed: chained
    max_steps = 1 calls give the 64-step call's states, energies, steps and flags bit for bit."""
    C_ = _whole_case(dtype)
    ref, s0 = C_["ref"], C_["s0"]
    stopped, unfinished = (ref["flags"] & STOPPED) > 0, (ref["flags"] & UNFINISHED) > 0
    left = ~stopped & ~unfinished
    assert stopped.sum() > 200 and left.sum() > 200 and unfinished.sum() >= 5, (stopped.sum(), left.sum(), unfinished.sum())
    assert (stopped & (ref["steps"] > 3)).sum() > 100 and len(np.unique(ref["steps"][stopped])) > 8  # stopped along the way, not only at once
    assert ref["energy"][stopped].max() < 0.5 * MEV and ref["energy"][left & (ref["moments"][0] > 0)].min() >= 0.5 * MEV
    f = {n: eng.Field(C_[n], *AX32) for n in ("E", "B", "ne", "Z")}
    kw = dict(mass=M_P, z=1.0, stop_energy=0.5 * MEV, **AL)
    try:
        whole = eng.push_particles_matter(f["E"], f["B"], f["ne"], f["Z"], s0, QM_P, DT, 64, 2, 0.1, **kw)
        s, steps, active = s0.copy(), np.zeros(N_PART, np.int32), np.arange(N_PART)
        flags, energy = np.zeros(N_PART, np.uint8), np.zeros(N_PART)
        M0, sp = np.zeros(N_PART), np.zeros(N_PART)
        for _ in range(64):
            one = eng.push_particles_matter(f["E"], f["B"], f["ne"], f["Z"], np.ascontiguousarray(s[:, active]), QM_P, DT, 1, 2, 0.1, **kw)
            s[:, active], flags[active], energy[active] = one["sf"], one["flags"], one["energy"]
            M0[active] = M0[active] + one["moments"][0]  # the step's t, added as the kernel adds it
            sp[active] = sp[active] + one["moments"][3]
            steps[active] += 1
            active = active[(one["flags"] & UNFINISHED) > 0]
            if not len(active):
                break
    finally:
        for h in f.values():
            h.close()
    for name, mine in (("sf", s), ("steps", steps), ("flags", flags), ("energy", energy)):
        assert np.array_equal(whole[name], mine, equal_nan=True), f"the 64-step call is not its step composed: {name}"
    assert np.array_equal(whole["moments"][0], M0, equal_nan=True) and np.array_equal(whole["moments"][3], sp, equal_nan=True)
    _assert_against(whole, ref, 64, f"64 steps, {np.dtype(dtype).name}")


def _bethe_S(T, ne, Z, K):
    """S(T) [J/m] of the rule for a proton of kinetic energy T [J], in float64 (the quadrature's integrand)."""
    g = 1.0 + T / K["mc2"]
    q = g * g - 1.0
    b2 = q / (g * g)
    Lf = np.log(K["A2"] * q / (K["HW"] * np.sqrt(ne))) - b2
    Lb = np.log(K["A2"] * q / K["I"]) - b2
    nb = ne * max(0.0, K["Zn"] - Z) / Z
    return K["KS"] / (b2 * LIGHT * LIGHT) * (ne * np.maximum(Lf, 0.0) + nb * np.maximum(Lb, 0.0))


@pytest.mark.gpu
def test_matter_only_slab(eng):
    _slab_check(lambda ne, s0, steps, dt: _push(eng, None, None, ne, None, s0, steps, dt=dt))


def _slab_check(run):
    """3: E = B = NULL in uniform ne (3.5e28 m^-3 of aluminium at Z = 3: 1.5e29 electrons per m^3 in all; float64): straight lines, and the energy after n steps
    against T1 with  integral_{T1}^{T0} dT/S(T) = s_end  (64-point Gauss-Legendre on 8 panels in NumPy, T1 by bisection), s_end the
    path length the kernel returns.
    The scheme is explicit Euler: a step takes ds = v dt and then u <- u (1 - S dt/(m |u|)), i.e. p <- p - S dt.  In energy,
    T(p - dp) = T - v dp + dp^2/(2 m gamma^3) - ..., with v dp = S ds: one step is Euler's step of dT/ds = -S(T) plus
    (S ds)^2/(2 m gamma^3 v^2) <= S^2 ds^2/(4 T) (1 + T/(m c^2)); Euler's local error is ds^2/2 |S S'| (S' = dS/dT).  An error dT made at
    one step grows along the rest of the path as d(dT)/ds = -S' dT, by at most S(T1)/S(T0) (S' < 0 above the Bragg peak).  So
      |T_n - T1| <= n ds^2 max(|S S'|/2 + S^2/(4 T) (1 + T/mc2)) S(T1)/S(T0) =: trunc     (max over [T1, T0], ds = v_0 dt, S' by differences),
    plus the roundings, n steps of the one-step da (below 1e3 u relative here).  Halving dt (2 n steps) halves the bound and must
    not increase the error.  Then the moments with the drag off (ne = 1e18: S s_end/T < 1e-10, which bounds the change of Ts by
    4e-10 relative, Ts ~ (pv)^-2 ~ T^-2 and twice for slack): M0 = Ts L, M1 = Ts L^2/2, and the midpoint rule's M2 = Ts (L^3/3 - L ds^2/12) exactly, L = n ds."""
    K = consts(QM_P, DT, M_P, 1.0, AL["Zn"], AL["I"], AL["lnLs"], Z=3.0)
    ne_v, T0 = 3.5e28, 14.7 * MEV
    g0 = 1.0 + T0 / K["mc2"]
    u0 = LIGHT * np.sqrt(g0 * g0 - 1.0)
    n = 257
    s0 = np.zeros((6, n))
    s0[0], s0[1] = np.linspace(-2.9e-3, 2.9e-3, n), np.linspace(-2.3e-3, 1.8e-3, n)
    s0[2], s0[5] = AX[2][0], u0
    xg, wg = np.polynomial.legendre.leggauss(64)

    def path_to(T1):
        e = np.linspace(T1, T0, 9)
        mid, half = 0.5 * (e[1:] + e[:-1])[:, None], 0.5 * (e[1:] - e[:-1])[:, None]
        return float(np.sum(half * wg / _bethe_S(mid + half * xg, ne_v, 3.0, K)))

    errs = []
    for dt, steps in ((DT, 30), (DT / 2, 60)):
        out = run(np.full(SHAPE, ne_v), s0, steps, dt)
        assert np.all(out["steps"] == steps) and np.all(out["flags"] == UNFINISHED)  # still inside: every midpoint was in the matter
        assert np.array_equal(out["sf"][:2], s0[:2]) and np.all(out["sf"][3:5] == 0.0), "a straight line along z"
        s_end = out["moments"][3]
        # s adds v dt of the speed before each drag, x half a step of the speed before and half of the speed after it: the
        # difference telescopes to (dt/2) (v_0 - v_n)
        v_n = out["sf"][5] / np.sqrt(1.0 + out["sf"][5] ** 2 * IC2)
        assert np.all(np.abs(s_end - (out["sf"][2] - s0[2]) - 0.5 * dt * (u0 / g0 - v_n)) <= 8 * steps * EPS * 5e-3)
        lo, hi = 0.0, T0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if path_to(mid) < s_end[0] else (mid, hi)
        T1 = 0.5 * (lo + hi)
        Tg = np.linspace(T1, T0, 4001)
        Sg = _bethe_S(Tg, ne_v, 3.0, K)
        dS = np.gradient(Sg, Tg)
        ds = u0 / g0 * dt
        trunc = steps * ds * ds * float(np.max(np.abs(Sg * dS) / 2 + Sg * Sg / (4 * Tg) * (1 + Tg / K["mc2"]))) * Sg[0] / Sg[-1]
        err = float(np.max(np.abs(out["energy"] - T1)))
        errs.append(err)
        print(f"slab, dt {dt:.2e}, {steps} steps, {s_end[0] * 1e3:.3f} mm: exit {out['energy'][0] / MEV:.4f} MeV, quadrature {T1 / MEV:.4f} MeV, "
              f"|error| {err / MEV:.3e} MeV, truncation bound {trunc / MEV:.3e} MeV; spread over particles {float(np.ptp(out['energy'])) / MEV:.1e} MeV")
        assert 0.3 * T0 < T1 < 0.9 * T0 and err <= trunc + 1e3 * steps * EPS * T0
    assert errs[1] <= errs[0]
    thin = run(np.full(SHAPE, 1e18), s0, 30, DT)
    M0, M1, M2, L = thin["moments"]
    v0 = u0 / g0
    Ts = K["KT"] * (1e18 / 3.0) / (M_P * u0 * u0 / g0) ** 2
    ds = v0 * DT
    assert np.all(np.abs(thin["energy"] - T0) <= 1e-10 * T0)
    tol = 4e-10 + 200 * 30 * EPS
    print(f"drag off: M0 / (Ts L) - 1 = {float(np.max(np.abs(M0 / (Ts * L) - 1))):.2e}, M1 {float(np.max(np.abs(M1 / (Ts * L * L / 2) - 1))):.2e}, "
          f"M2 {float(np.max(np.abs(M2 / (Ts * (L ** 3 / 3 - L * ds * ds / 12)) - 1))):.2e}; tolerance {tol:.1e}")
    assert np.all(np.abs(L - 30 * ds) <= tol * L)
    assert np.all(np.abs(M0 - Ts * L) <= tol * Ts * L) and np.all(np.abs(M1 - Ts * L * L / 2) <= tol * Ts * L * L / 2)
    assert np.all(np.abs(M2 - Ts * (L ** 3 / 3 - L * ds * ds / 12)) <= tol * Ts * L ** 3 / 3)


@pytest.mark.gpu
def test_counts_image_and_stats(eng):
    """4: the device's counts image is engine.hist2d of the returned hits with flags == 0; stopped particles are absent; the
    stats add up; an image-only call deposits the same; a repeated call returns the same bits."""
    C_ = _whole_case(np.float64)
    s0 = C_["s0"].copy()
    s0[5] = np.abs(s0[5])  # towards the plane z = 0.1 and within 0.3 rad of its normal, so that most of those that leave land on
    s0[3:5] *= 0.2         # the detector
    img, img2 = (eng.DetectorImage(eng.IMG_COUNTS, 32, 24, -40.0, 40.0, -30.0, 30.0) for _ in range(2))
    try:
        out = _push(eng, C_["E"], C_["B"], C_["ne"], C_["Z"], s0, 64, stop=0.5 * MEV, image=img)
        H = img.download()
        only = _push(eng, C_["E"], C_["B"], C_["ne"], C_["Z"], s0, 64, stop=0.5 * MEV, image=img2, want=())
        H2 = img2.download()
        again = _push(eng, C_["E"], C_["B"], C_["ne"], C_["Z"], s0, 64, stop=0.5 * MEV)
    finally:
        img.close()
        img2.close()
    good = out["flags"] == 0
    stopped = (out["flags"] & STOPPED) > 0
    want = eng.hist2d(np.ascontiguousarray(out["hits"][0, good]), np.ascontiguousarray(out["hits"][1, good]), 32, 24, -40.0, 40.0, -30.0, 30.0)
    assert np.array_equal(H, want) and np.array_equal(H2, H) and set(only) == {"stats"}
    st = out["stats"]
    assert st.deposited == int(H.sum()) == only["stats"].deposited and 100 < H.sum() <= good.sum()
    assert stopped.sum() > 200 and not np.any(good & stopped)
    with_stopped = eng.hist2d(np.ascontiguousarray(out["hits"][0, good | stopped]), np.ascontiguousarray(out["hits"][1, good | stopped]), 32, 24,
                              -40.0, 40.0, -30.0, 30.0)
    finite_stopped = stopped & np.all(np.isfinite(out["hits"]), axis=0) & ((out["flags"] & MISSED) == 0)
    assert finite_stopped.sum() > 50 and with_stopped.sum() > H.sum(), "stopped particles with a finite hit exist and are left out"
    assert st.finished + st.unfinished == N_PART and st.unfinished == int(((out["flags"] & UNFINISHED) > 0).sum())
    assert st.stopped == int(stopped.sum()) and st.missed == int(((out["flags"] & MISSED) > 0).sum()) and again["stats"].deposited == 0
    for name in ("sf", "hits", "steps", "flags", "energy", "moments"):
        assert np.array_equal(out[name], again[name], equal_nan=True), f"a repeated call returned other bits in {name}"


@pytest.mark.gpu
def test_api_material(eng):
    """5: ScalarDomain.proton_radiograph(material=...) of both generations and on a rotated() domain is the engine call: the same
    bits as engine.push_particles_matter on radiography.entry's states, with sort=True and sort=False; Z as a grid and as a
    number; energy windows and the scattered image."""
    from synthpy_amd import radiography
    from synthpy_amd.simulator.domain import ScalarDomain as NewDomain
    from synthpy_amd.solvers_legacy import full_solver as fs

    n = 12
    x = np.float32((np.arange(n) - (n - 1) / 2) * 2.0 ** -11)
    ext = float(x[-1])
    rng = np.random.default_rng(3)
    B = 0.5 * np.clip(rng.standard_normal((n, n, n, 3)), -4, 4)
    ne = np.zeros((n, n, n))
    ne[4:7, 2:10, 2:10] = 1.5e29  # a foil across the line of sight x, smaller than the box
    Zg = np.full((n, n, n), 3.0)
    Zg[:, :5] = 11.0
    al = radiography.Material.Al()
    pos = np.array([-9e-3, 0.2e-3, -0.1e-3])
    src = radiography.ProtonSource(14.7, pos, "x", half_angle=0.45, n=N_PART, seed=2)  # a cone wider than the box
    old = fs.ScalarDomain(x, x, x, ext, probing_direction="z")
    new = NewDomain((2 * ext, 2 * ext, 2 * ext), (n, n, n))
    assert np.array_equal(np.float32(new.x), x)
    rads = {}
    for name, dom in (("legacy", old), ("simulator", new)):
        dom.external_ne(ne)
        dom.external_B(B)
        dom.external_Z(Zg)
        rads[name] = dom.proton_radiograph(src, 0.06, bins=(32, 32), material=al, stop_energy_MeV=1.0)
        rads[name + ", sort=False"] = dom.proton_radiograph(src, 0.06, bins=(32, 32), material=al, stop_energy_MeV=1.0, sort=False)
    a = rads["legacy"]
    # the engine call on the host's entry states
    g = [np.float64(x)] * 3
    s_in, meets = radiography.entry(src.states(), [x[0]] * 3, [x[-1]] * 3)
    idx = np.nonzero(meets)[0]
    f = {k: eng.Field(v, x, x, x) for k, v in (("B", B), ("ne", ne), ("Z", Zg))}
    try:
        direct = eng.push_particles_matter(None, f["B"], f["ne"], f["Z"], np.ascontiguousarray(s_in[:, idx]), src.qm, a.dt, a.max_steps, 0, 0.06,
                                           mass=src.mass, z=1.0, Zn=al.Zn, I=al.I, lnLs=al.coulomb_log, stop_energy=1.0 * MEV)
    finally:
        for h in f.values():
            h.close()
    assert 100 < len(idx) < N_PART and a.stats.finished == len(idx)
    for name in ("sf", "hits", "flags", "steps"):
        assert np.array_equal(getattr(a, name)[..., idx], direct[name], equal_nan=True), name
    assert np.array_equal(a.energy_MeV[idx], direct["energy"] / MEV) and np.array_equal(a.moments[:, idx], direct["moments"])
    assert np.all(a.moments[:, ~meets] == 0) and np.all(np.abs(a.energy_MeV[~meets] - 14.7) <= 1e-12)
    for name, r in rads.items():
        for attr in ("hits", "flags", "steps", "sf", "counts", "energy_MeV", "moments", "stopped"):
            assert np.array_equal(getattr(a, attr), getattr(r, attr), equal_nan=True), (name, attr)
        assert r.stats.stopped == a.stats.stopped and r.stats.deposited == a.stats.deposited
    assert a.stats.stopped == int(a.stopped.sum())
    crossed = a.moments[0] > 0
    assert crossed.sum() > 100 and np.all(a.energy_MeV[crossed] < 14.7) and np.all(a.energy_MeV[~crossed & (a.steps > 0)] > 14.69)
    # Z as a number: the uniform-Z instantiation, not the field's bits where Z differs
    old.external_Z(3.0)
    u = old.proton_radiograph(src, 0.06, bins=(32, 32), material=al, stop_energy_MeV=1.0)
    assert np.array_equal(u.steps == 0, a.steps == 0) and not np.array_equal(u.energy_MeV, a.energy_MeV)
    old.external_Z(Zg)
    # energy windows partition the image; the scattered image keeps the particles and moves them by about sigma_y
    lo_w, hi_w = a.counts_in(0.0, 12.0), a.counts_in(12.0, 20.0)
    assert np.array_equal(lo_w + hi_w, a.counts) and lo_w.sum() > 0 and hi_w.sum() > 0
    sc = a.scattered(5)
    sc2 = old.proton_radiograph(src, 0.06, bins=(32, 32), material=al, stop_energy_MeV=1.0, scatter_seed=5)
    assert np.array_equal(sc.hits, sc2.hits) and np.array_equal(sc.counts, sc2.counts) and np.array_equal(sc.hits, a.scattered_hits(5))
    (x0, x1), (y0, y1) = ((e[0], e[-1]) for e in a.edges)
    keep = a.flags == 0
    assert np.array_equal(sc.counts, eng.hist2d(np.ascontiguousarray(sc.hits[0, keep]), np.ascontiguousarray(sc.hits[1, keep]), 32, 32, x0, x1, y0, y1))
    _, sy = a.scatter_sigma()
    moved = np.sqrt(np.sum((sc.hits - a.hits) ** 2, axis=0)) / 1e3
    assert np.all(moved[~crossed] == 0) and 0.5 < np.median(moved[crossed & keep] / sy[crossed & keep]) < 2.5
    # a rotated domain carries ne and Z: probed along z' it is the original probed along x (test_radiography's 5c), decisions equal
    view = old.rotated(90, about="y")
    s0 = src.states()
    s0v = np.array([-s0[2], s0[1], s0[0], -s0[5], s0[4], s0[3]])
    fixed = tr._Fixed(src, 2, (-pos[2], pos[1], pos[0]), s0v)
    fixed.mass, fixed.charge = src.mass, src.charge
    rv = view.proton_radiograph(fixed, 0.06, bins=(32, 32), material=al, stop_energy_MeV=1.0)
    rv2 = view.proton_radiograph(fixed, 0.06, bins=(32, 32), material=al, stop_energy_MeV=1.0, sort=False)
    for attr in ("hits", "flags", "steps", "sf", "energy_MeV", "moments"):
        assert np.array_equal(getattr(rv, attr), getattr(rv2, attr), equal_nan=True), attr
    assert np.array_equal(rv.steps, a.steps) and np.array_equal(rv.flags, a.flags)
    # the two runs sum |u|^2 and the blends in another order: the energies agree to the path's roundings (1e3 u per step is generous
    # for a path without a stop: the loss is 15 % at most)
    assert np.all(np.abs(rv.energy_MeV - a.energy_MeV) <= 1e3 * a.steps.max() * EPS * 14.7)
    with pytest.raises(ValueError, match="material"):
        old.proton_radiograph(src, 0.06, material="Al")
    with pytest.raises(ValueError, match="need a material"):
        old.proton_radiograph(src, 0.06, scatter_seed=1)
