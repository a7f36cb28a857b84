"""CPU-only: the checks the four line-spectra entries share (sr_field_sightline_lines, _voigt, _zeeman, _stokes) are the same
checks in the same order with the same text under every entry -- only the entry's name differs.  The files of the single
entries hold each entry's own checks; this one holds the entries to each other.  2 chords, 3 frequencies, a 2 x 2 lattice with
one line; every call carries NULL fields (and, for the two polarised entries, a B that is no field and is never dereferenced),
so a call that passes every check ends at 'NULL ne field' and nothing reaches the device."""
import ctypes as C
import itertools

import numpy as np
import pytest

ENTRIES = ("lines", "voigt", "zeeman", "stokes")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from synthpy_amd import _ffi

    return _ffi


def _table(built, kind, keep):
    """The entry's table struct on a 2 x 2 lattice with one line (a Lorentzian width, one pi component); keep holds the arrays."""
    LT, LD = np.log([10.0, 100.0]), np.log([1e22, 1e24])
    w0, A = np.array([7.55e15]), np.array([12.0])
    LJ, LK, LG = np.log(np.full((1, 2, 2), 3.0)), np.log(np.full((1, 2, 2), 2.0)), np.log(np.full((1, 2, 2), 1e11))
    n_comp, comp = np.array([1], np.int32), np.array([[0.0, 1.0, 1.0]])
    keep += [LT, LD, w0, A, LJ, LK, LG, n_comp, comp]
    ptr = built.ptr
    t = built.LineTable()
    t.nT, t.nD, t.n_line, t.reserved = 2, 2, 1, 0
    t.LT, t.LD, t.w0, t.A, t.LJ, t.LK = ptr(LT), ptr(LD), ptr(w0), ptr(A), ptr(LJ), ptr(LK)
    if kind == "lines":
        return t
    v = built.VoigtTable()
    v.lines, v.LG = t, ptr(LG)
    if kind == "voigt":
        return v
    z = built.ZeemanTable()
    z.voigt, z.n_comp, z.comp = v, ptr(n_comp), ptr(comp)
    return z


# The family's checks in the family's order: (name, what the call changes, the text after "<entry>: ").  A name in `changes`
# is an argument of call() below; two breaks that change the same argument cannot be combined.
def _breaks(kind):
    nan_origin, zero_dir = np.zeros((3, 2)), np.ones((3, 2))
    nan_origin[1, 1] = np.nan
    zero_dir[:, 0] = 0.0
    bad_omega, bad_c = np.array([7.5e15, 0.0, 7.6e15]), np.array([1.0, 1.0, np.inf])
    rows = [
        ("NULL p", {"p": None}, "NULL argument"),
        ("NULL omega", {"om": None}, "NULL omega, e_ph or c_omega"),
        ("negative n", {"n": -1}, "n must not be negative, got -1"),
        ("negative n_freq", {"nf": -1}, "n_freq must not be negative, got -1"),
        ("non-positive omega", {"om": bad_omega}, "omega of frequency 1 must be finite and positive"),
        ("non-finite c_omega", {"c": bad_c}, "non-finite e_ph or c_omega of frequency 2"),
        ("toward = 0", {"toward": 0}, "toward must be +1 or -1, got 0"),
        ("step = 0", {"step": 0.0}, "step must be finite and positive"),
        ("max_steps = 0", {"max_steps": 0}, "max_steps must be at least 1, got 0"),
        ("NULL table", {"t": None}, "NULL line table"),
        ("wing = 0", {"wing": 0.0}, "wing must be positive (+inf is allowed), got 0"),
        ("workgroup cap", {"n": 2 ** 31}, "n x frequency tiles exceeds 2^31 - 1 workgroups"),
        ("non-finite origin", {"o": nan_origin}, "non-finite origin of line 1"),
        ("zero direction", {"d": zero_dir}, "the direction of line 0 is zero"),
    ]
    if kind == "lines":  # sr_lines_params has no wing
        rows = [r for r in rows if r[0] != "wing = 0"]
    return rows


_IN_P = {"toward", "step", "max_steps", "wing"}  # members of the params struct: a NULL p has none of them


def _conflict(a, b):
    ka, kb = set(a), set(b)
    return bool(ka & kb) or ("p" in ka and kb & _IN_P) or ("p" in kb and ka & _IN_P)


@pytest.fixture(scope="module")
def caller(built):
    lib, ptr = built.lib, built.ptr
    keep = []
    out = [np.zeros((2, 3)) for _ in range(5)]
    ref = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 0.0]])  # across d = (1, 1, 1)
    fakeB = C.c_void_p(C.addressof(C.create_string_buffer(256)))  # not NULL: the polarised path; never dereferenced before ne's check
    keep.append(fakeB)
    defaults = dict(n=2, nf=3, o=np.zeros((3, 2)), d=np.ones((3, 2)), om=np.array([7.5e15, 7.55e15, 7.6e15]), e=np.ones(3),
                    c=np.ones(3), toward=1, step=1e-4, max_steps=10, wing=np.inf, p="built", t="built")
    tables = {kind: _table(built, kind, keep) for kind in ENTRIES}

    def call(kind, **kw):
        """(return code, error text) of the entry `kind` with the defaults but for kw"""
        a = dict(defaults, **kw)
        if kind == "lines":
            p = built.LinesParams()
            m = p
        else:
            p = built.VoigtParams()
            m = p.march
            p.wing = a["wing"]
        m.toward, m.max_steps, m.continuum, m.reserved, m.step, m.Te, m.Z = a["toward"], a["max_steps"], 0, 0, a["step"], 50.0, 1.0
        p = None if a["p"] is None else C.byref(p)
        t = a["t"]
        t = None if t is None else C.byref(tables[kind] if isinstance(t, str) else t)
        chords = (a["n"], ptr(a["o"]), ptr(a["d"]))
        freqs = (a["nf"], ptr(a["om"]), ptr(a["e"]), ptr(a["c"]))
        I, Q, U, V, tau = (ptr(x) for x in out)
        if kind == "lines":
            rc = lib.sr_field_sightline_lines(None, None, None, None, None, t, p, *chords, *freqs, None, I, tau, None, None, None, None)
        elif kind == "voigt":
            rc = lib.sr_field_sightline_voigt(None, None, None, None, None, t, p, *chords, *freqs, None, I, tau, None, None, None, None)
        elif kind == "zeeman":
            rc = lib.sr_field_sightline_zeeman(None, None, None, None, None, fakeB, t, p, *chords, ptr(ref), *freqs, None, I, Q, U, V, tau,
                                               None, None, None, None)
        else:
            rc = lib.sr_field_sightline_stokes(None, None, None, None, None, fakeB, t, p, *chords, ptr(ref), *freqs, None, None, 0, I, Q, U,
                                               V, tau, None, None, None, None)
        return rc, built.last_error()

    call.keep, call.tables = keep, tables
    return call


@pytest.mark.parametrize("kind", ENTRIES)
def test_every_shared_check_alone(caller, kind):
    """A call that breaks one shared check and nothing earlier: SR_ERR_INVALID and the family's text under the entry's name."""
    who = "sr_field_sightline_" + kind
    assert caller(kind) == (-1, who + ": NULL ne field")  # every argument in order: the fields' check, the last one, speaks
    for name, change, text in _breaks(kind):
        assert caller(kind, **change) == (-1, f"{who}: {text}"), name


@pytest.mark.parametrize("kind", ENTRIES)
def test_of_two_broken_checks_the_earlier_one_speaks(caller, kind):
    """Every pair of shared checks that can be broken in one call, in the family's order: the earlier one's text."""
    who = "sr_field_sightline_" + kind
    pairs = 0
    for (na, ca, ta), (nb, cb, _) in itertools.combinations(_breaks(kind), 2):
        if _conflict(ca, cb):
            continue
        assert caller(kind, **ca, **cb) == (-1, f"{who}: {ta}"), (na, nb)
        pairs += 1
    assert pairs >= 60


def test_wing_is_read_only_where_the_entry_reads_it(built, caller):
    """sr_field_sightline_voigt reads wing only with LG given (LG NULL is sr_field_sightline_lines' rule, delegated after voigt's
    own checks); the polarised entries always read it."""
    keep = []
    gauss_v = _table(built, "voigt", keep)
    gauss_v.LG = None
    assert caller("voigt", t=gauss_v, wing=0.0) == (-1, "sr_field_sightline_voigt: NULL ne field")
    for kind in ("zeeman", "stokes"):
        gauss_z = _table(built, kind, keep)
        gauss_z.voigt.LG = None
        assert caller(kind, t=gauss_z, wing=0.0) == (-1, f"sr_field_sightline_{kind}: wing must be positive (+inf is allowed), got 0")
        assert caller(kind, t=gauss_z) == (-1, f"sr_field_sightline_{kind}: NULL ne field")
