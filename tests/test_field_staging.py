"""The host staging the field diagnostics share (synthpy_amd/fields.py) and the one wording of their entry points' field checks.

The CPU tests replace engine.Field by a recorder, so what is uploaded, under which name and in which dtype, and what is closed,
is read off without a device.  The host cell search (fields.locate) is tested against a brute-force search, and its three users
against values recorded before they shared it (tests/golden/field_staging_host.npz).  The GPU tests run the five entry points
that take several sr_field handles on fields that must be refused, and self_emission / table_emission on kept uploads."""
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import golden

SHAPE = (4, 5, 6)


def _axes():
    """4 x 5 x 6 non-uniform node coordinates [m], float64 values that float32 does not hold."""
    rng = np.random.default_rng(41)
    return [np.cumsum(rng.uniform(0.4, 1.6, n)) * 1e-3 - 2e-3 for n in SHAPE]


def _domain(dtype=np.float64, **extra):
    rng = np.random.default_rng(43)
    x, y, z = _axes()
    d = SimpleNamespace(x=x, y=y, z=z, probing_direction="z", ne=(1e24 * (0.5 + rng.random(SHAPE))).astype(dtype),
                        Te=(50.0 + 100.0 * rng.random(SHAPE)).astype(dtype), Z=(1.0 + 5.0 * rng.random(SHAPE)).astype(dtype))
    for k, v in extra.items():
        setattr(d, k, v)
    return d


class Recorder:
    """Stands in for engine.Field: keeps what it was given and counts close()."""
    made = []

    def __init__(self, data, x, y, z):
        self.array = np.asarray(data)
        self.shape, self.dtype = self.array.shape, self.array.dtype
        self.closed = 0
        self.last_kernel_ms = 0.0
        self.nbytes = self.array.nbytes
        Recorder.made.append(self)

    def close(self):
        self.closed += 1


@pytest.fixture
def rec(monkeypatch):
    from synthpy_amd import engine

    Recorder.made = []
    monkeypatch.setattr(engine, "Field", Recorder)
    return Recorder


# ---------------------------------------------------------------- SourceFields.get_all, staged
def test_get_all_uploads_in_one_dtype(rec):
    from synthpy_amd import fields, orientation

    assert orientation.SourceFields is fields.SourceFields
    d = _domain(np.float32)
    src = fields.SourceFields(d)
    got = src.get_all({"ne": d.ne, "Te": d.Te, "Z": None})
    assert got["Z"] is None and len(rec.made) == 2 and sorted(src.fields) == ["Te", "ne"]
    assert got["ne"].dtype == np.float32 and got["Te"].dtype == np.float32
    again = src.get_all({"ne": d.ne, "Te": d.Te, "Z": None})
    assert again["ne"] is got["ne"] and again["Te"] is got["Te"] and len(rec.made) == 2
    # one float64 among float32: the float32 ones are widened under a name of their own, the float64 one keeps its name
    Z64 = np.float64(d.Z)
    mixed = src.get_all({"ne": d.ne, "Te": d.Te, "Z": Z64})
    assert len(rec.made) == 5 and sorted(src.fields) == ["Te", "Te:float64", "Z", "ne", "ne:float64"]
    assert all(f.dtype == np.float64 for f in mixed.values())
    assert mixed["ne"] is src.fields["ne:float64"] and mixed["Z"] is src.fields["Z"]
    assert np.array_equal(mixed["ne"].array, np.float64(d.ne)) and mixed["Z"].array is Z64
    assert src.get_all({"ne": d.ne, "Te": d.Te, "Z": Z64})["Te"] is mixed["Te"] and len(rec.made) == 5
    assert src.nbytes == sum(f.nbytes for f in rec.made)
    src.close()
    assert all(f.closed == 1 for f in rec.made) and src.fields == {}


def test_staged_owns_or_borrows(rec):
    from synthpy_amd import fields

    d, other = _domain(), _domain()
    with pytest.raises(ValueError, match="fields holds the fields of another domain"):
        with fields.staged(d, fields.SourceFields(other)):
            pass
    with pytest.raises(ValueError, match="source holds the fields of another domain"):
        with fields.staged(d, fields.SourceFields(other), "source"):
            pass
    with fields.staged(d, None) as src:
        f = src.get("ne", d.ne)
        assert src.domain is d and f.closed == 0
    assert f.closed == 1
    with pytest.raises(KeyError):
        with fields.staged(d, None) as src:
            g = src.get("ne", d.ne)
            raise KeyError("the body fails")
    assert g.closed == 1
    mine = fields.SourceFields(d)
    with fields.staged(d, mine) as src:
        assert src is mine
        h = src.get("ne", d.ne)
    assert h.closed == 0 and mine.fields == {"ne": h}
    with pytest.raises(KeyError):
        with fields.staged(d, mine) as src:
            raise KeyError("the body fails")
    assert h.closed == 0


def test_uniform():
    from synthpy_amd import fields

    assert fields.uniform(3) == 3.0 and fields.uniform(np.float32(2.5)) == 2.5 and fields.uniform(np.array([7.0])) == 7.0
    assert fields.uniform(np.broadcast_to(np.float64(4.0), SHAPE)) == 4.0
    assert fields.uniform(np.full(SHAPE, 4.0)) is None


# ---------------------------------------------------------------- the host cell search
def test_locate_against_brute_force():
    from synthpy_amd import fields

    g = np.array([-1.0, -0.25, 0.5, 0.75, 2.0])
    n = len(g)
    rng = np.random.default_rng(47)
    p = np.r_[g, np.nextafter(g, np.inf), np.nextafter(g, -np.inf), rng.uniform(-1.5, 2.5, 40), np.nan, -np.inf, np.inf]
    cell, w, inside = fields.locate(g, p)
    for k in range(len(p)):
        ok = bool(p[k] >= g[0] and p[k] <= g[-1])
        assert inside[k] == ok, p[k]
        if ok:
            c = max(i for i in range(n - 1) if g[i] <= p[k])  # the largest cell whose lower node is not above p
            assert cell[k] == c and w[k] == (p[k] - g[c]) / (g[c + 1] - g[c]), p[k]
        assert 0 <= cell[k] <= n - 2
    # a point on every node: weight 0 in the node's own cell, the last node weight 1 in the last cell
    assert cell[:n].tolist() == [0, 1, 2, 3, n - 2] and w[:n].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    # outside on both sides (one ulp, and infinitely far) and a NaN
    assert not inside[2 * n - 1] and not inside[2 * n] and not inside[-3:].any() and np.isnan(w[-3])
    assert inside[:2 * n - 1].all() and inside[2 * n + 1:3 * n].all()


def host_cases():
    """Seeded inputs on the 4 x 5 x 6 grid for thomson._at, radiography.entry_cell_order and projection.bilinear."""
    from synthpy_amd import fields

    rng = np.random.default_rng(53)
    d = _domain()
    d.Te = np.float32(d.Te)
    g = fields.grid_f64(d)
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    span = hi - lo
    points = lo + (rng.random((60, 3)) * 1.3 - 0.15) * span          # some outside, on every side
    points[:4] = [[g[0][i], g[1][i + 1], g[2][i + 2]] for i in range(4)]  # on nodes, the last ones included
    points[4] = [np.nan, g[1][2], g[2][2]]
    states = np.empty((6, 80))
    states[:3] = (lo + (rng.random((80, 3)) * 1.2 - 0.1) * span).T
    states[:3, :4] = points[:4].T
    states[3:] = rng.standard_normal((3, 80))
    maps = rng.standard_normal((2, SHAPE[1], SHAPE[2]))
    p = lo[1] + (rng.random(50) * 1.2 - 0.1) * span[1]
    q = lo[2] + (rng.random(50) * 1.2 - 0.1) * span[2]
    p[:3], q[:3] = [g[1][0], g[1][-1], g[1][2]], [g[2][-1], g[2][0], g[2][3]]
    p[3], q[4] = np.nan, np.nan
    return dict(domain=d, ne=d.ne, Te=d.Te, g=g, points=points, states=states, maps=maps, p=p, q=q)


def test_cell_search_users_keep_their_bits():
    from synthpy_amd import projection, radiography, thomson

    c, want = host_cases(), golden("field_staging_host")
    ne_c, Te_c = thomson._at(c["domain"], (c["ne"], c["Te"]), c["points"])
    assert ne_c.tobytes() == want["at_ne"].tobytes() and Te_c.tobytes() == want["at_Te"].tobytes()
    assert np.isnan(ne_c).sum() > 5 and np.isfinite(ne_c).sum() > 20
    assert np.array_equal(radiography.entry_cell_order(c["states"], c["g"]), want["order"])
    out = projection.bilinear((c["g"][1], c["g"][2]), c["maps"], c["p"], c["q"])
    assert out.tobytes() == want["bilinear"].tobytes() and np.isnan(out[0]).sum() > 2


# ---------------------------------------------------------------- what each diagnostic uploads
def test_upload_counts(rec, monkeypatch):
    """The Fields each diagnostic constructs -- the same numbers as before they shared SourceFields.get_all: thomson.spectra
    5 for ne, Te, Ti, Z, V arrays and 2 for a scalar Z without Ti and V; wave.propagate 1 without absorb; self_emission 1 for a
    scalar Te and Z; radiograph 2 for E and B.  Everything is closed once when the call owns the uploads."""
    from synthpy_amd import emission, engine, radiography, thomson, wave

    rng = np.random.default_rng(59)
    monkeypatch.setattr(engine, "thomson", lambda ne, Te, Ti, Z, V, li, A, pts, wts, ki, ks, lam: (np.zeros((len(pts), len(lam))), np.zeros(len(pts))))
    probe = thomson.Probe(532e-9, (0, 0, -5e-3), (0, 0, 1))
    coll = thomson.Collection(np.zeros((2, 3)), (0, 1, 0), length=1e-4, n_quad=2)
    lam = np.linspace(530e-9, 534e-9, 3)
    d = _domain(Ti=20.0 + rng.random(SHAPE), V=rng.standard_normal(SHAPE + (3,)))
    thomson.spectra(d, probe, coll, lam, 12.0)
    assert len(rec.made) == 5 and all(f.closed == 1 and f.dtype == np.float64 for f in rec.made)
    rec.made.clear()
    d = _domain(np.float32)
    d.Z = 3.0
    thomson.spectra(d, probe, coll, lam, 12.0)
    assert len(rec.made) == 2 and all(f.closed == 1 and f.dtype == np.float32 for f in rec.made)

    rec.made.clear()
    monkeypatch.setattr(engine, "wave", lambda ne, Te, Z, U, *a, **k: (U, None))
    wave.propagate(_domain(), wave.Source.plane((4, 4), 1e-4, 532e-9))
    assert len(rec.made) == 1 and rec.made[0].closed == 1

    rec.made.clear()
    seen = []

    def fake_emission(ne, Te, Z, omegas, axis, toward=+1, backlight=None):
        seen.append((ne, Te, Z))
        return np.zeros((len(omegas),) + SHAPE[:2]), np.zeros((len(omegas),) + SHAPE[:2])

    monkeypatch.setattr(engine, "emission", fake_emission)
    d = _domain()
    d.Te, d.Z = 80.0, np.broadcast_to(np.float64(2.0), SHAPE)
    emission.self_emission(d, [532e-9])
    assert len(rec.made) == 1 and rec.made[0].closed == 1 and seen[0] == (rec.made[0], 80.0, 2.0)
    # an array broadcast along an axis is uploaded in full
    rec.made.clear()
    d.Te = np.float32(50.0 + rng.random((1, 5, 6)))
    emission.self_emission(d, [532e-9])
    assert sorted((f.shape, str(f.dtype)) for f in rec.made) == [(SHAPE, "float64")] * 2
    assert np.array_equal(seen[1][1].array, np.broadcast_to(np.float64(d.Te), SHAPE))

    rec.made.clear()
    image = SimpleNamespace(kind=engine.IMG_COUNTS, nx=4, ny=4, range=(-1.0, 1.0, -1.0, 1.0), counts_f64=lambda: np.zeros((4, 4)),
                            close=lambda: None)
    monkeypatch.setattr(engine, "DetectorImage", lambda *a, **k: image)
    n_pushed = []

    def fake_push(E, B, s0, *a, **k):
        n = s0.shape[1]
        n_pushed.append((E, B))
        return dict(sf=s0, hits=np.zeros((2, n)), flags=np.zeros(n, np.uint8), steps=np.ones(n, np.int32), stats=engine.PushStats(0.0, n, 0, 0, n))

    monkeypatch.setattr(engine, "push_particles", fake_push)
    d = _domain(E=np.float32(rng.standard_normal(SHAPE + (3,))), B=rng.standard_normal(SHAPE + (3,)))
    src = radiography.ProtonSource(14.7, (0.0, 0.0, -10e-3), "z", half_angle=0.05, n=16, pattern="lattice")
    radiography.radiograph(d, src, det_pos=0.1)
    assert len(rec.made) == 2 and all(f.closed == 1 and f.dtype == np.float64 for f in rec.made)
    assert n_pushed[0][0].array.shape == SHAPE + (3,) and np.array_equal(n_pushed[0][0].array, np.float64(d.E))


# ---------------------------------------------------------------- GPU: the entry points' field checks, kept uploads
@pytest.fixture(scope="module")
def eng():
    from synthpy_amd import engine

    engine.init(0)
    return engine


ENTRIES = ("sr_field_emission", "sr_field_emission_table", "sr_field_wave", "sr_field_thomson", "sr_particles_push")


def _entry_call(eng, entry):
    """(n_comp of the entry's first two fields, their names, call(first, second))."""
    from test_table_emission import make_table

    if entry == "sr_field_emission":
        return 1, ("ne", "Te"), lambda a, b: eng.emission(a, b, 1.0, [3.5e15], 2)
    if entry == "sr_field_emission_table":
        table = make_table(3, 4, 2, seed=5)
        return 1, ("ne", "Te"), lambda a, b: eng.emission_table(a, b, 1.0, table, 2)
    if entry == "sr_field_wave":
        U = np.ones((4, 4), np.complex128)
        return 1, ("ne", "Te"), lambda a, b: eng.wave(a, b, 1.0, U, (-2e-4, 1e-4, -2e-4, 1e-4), 532e-9, 2)
    if entry == "sr_field_thomson":
        return 1, ("ne", "Te"), lambda a, b: eng.thomson(a, b, None, 3.0, None, 532e-9, 12.0, np.zeros((1, 1, 3)), np.ones((1, 1)),
                                                        (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), [531e-9, 533e-9])
    s0 = np.array([[0.0], [0.0], [0.0], [0.0], [0.0], [5e7]])
    return 3, ("E", "B"), lambda a, b: eng.push_particles(a, b, s0, 9.58e7, 1e-12, 4, 2, 0.1)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_refuse_fields_in_one_wording(eng, entry):
    from synthpy_amd import _ffi as built

    nc, (first, second), call = _entry_call(eng, entry)
    x, y, z = (np.float32(a) for a in _axes())
    rng = np.random.default_rng(61)
    tail = (3,) if nc == 3 else ()
    data = rng.random(SHAPE + tail) + 1.0
    made = dict(ref=eng.Field(data, x, y, z), other_comp=eng.Field(rng.random(SHAPE + ((3,) if nc == 1 else ())) + 1.0, x, y, z),
                single=eng.Field(np.float32(data), x, y, z), moved=eng.Field(data, x, y, z + np.float32(1e-6)),
                small=eng.Field(data[:-1], x[:-1], y, z))
    try:
        for b, text in ((made["other_comp"], f"{second} must have n_comp == {nc}"),
                        (made["single"], f"{first} and {second} differ in dtype"),
                        (made["moved"], f"the grids of {first} and {second} differ on axis 2"),
                        (made["small"], f"the grids of {first} and {second} differ on axis 0")):
            with pytest.raises(built.SynthrayError, match=re.escape(f"{entry}: {text}")):
                call(made["ref"], b)
        with pytest.raises(built.SynthrayError, match=re.escape(f"{entry}: {first} must have n_comp == {nc}")):
            call(made["other_comp"], made["ref"])
    finally:
        for f in made.values():
            f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("self_emission", "table_emission"))
def test_emission_keeps_uploads(eng, which):
    from synthpy_amd import emission, fields
    from test_table_emission import make_table

    d = _domain()
    d.ne = d.ne * 1e-3
    d.Z = 2.0
    if which == "self_emission":
        run = lambda **kw: emission.self_emission(d, [532e-9, 200e-9], **kw)
    else:
        table = make_table(3, 4, 2, seed=5)
        d.ne = d.ne * 1e-3  # ion densities inside the table's lattice
        run = lambda **kw: emission.table_emission(d, table, **kw)
    alone = run()
    assert np.all(np.isfinite(alone.intensity)) and np.all(alone.intensity > 0) and np.all(alone.optical_depth > 0)
    src = fields.SourceFields(d)
    try:
        first = run(fields=src)
        kept = dict(src.fields)
        second = run(fields=src)
        assert sorted(kept) == ["Te", "ne"] and src.fields == kept and all(src.fields[k] is kept[k] for k in kept)
        for em in (first, second):
            assert em.intensity.tobytes() == alone.intensity.tobytes() and em.optical_depth.tobytes() == alone.optical_depth.tobytes()
        with pytest.raises(ValueError, match="fields holds the fields of another domain"):
            emission.self_emission(_domain(), [532e-9], fields=src)
    finally:
        src.close()
