"""utils/eos_opacity.py: read_propaceos against what the reference's reader returned for the synthetic files under tests/golden
(g16_*.prp, g16_propaceos.npz; tests/golden/make_g16_propaceos.py wrote both) -- bit for bit, key for key, Nones included -- and
OpacityTable: from_propaceos round-trips and every validation error names its member.  No GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_g16_propaceos as g16  # noqa: E402  (the cases' names, flags and file paths; it reads the reference only in main())


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "g16_propaceos.npz"))


@pytest.mark.parametrize("tag", list(g16.CASES))
def test_reader_equals_the_reference(golden, tag):
    """all flags on / opacities only / nT = 10, nD = 20 / one group (an edge block of one line with two values)."""
    from synthpy_amd.utils.eos_opacity import read_propaceos

    got = read_propaceos(g16.path(tag), **g16.flags(tag))
    assert list(got) == golden[f"{tag}/keys"].tolist()
    none = set(golden[f"{tag}/none"].tolist())
    assert none == {k for k in g16.ALL if k not in g16.CASES[tag][4]}
    _, n_t, n_d, n_g, _ = g16.CASES[tag]
    for key, value in got.items():
        if key in none:
            assert value is None, (tag, key)
            continue
        want = golden[f"{tag}/{key}"]
        assert isinstance(value, np.ndarray) and value.dtype == want.dtype == np.float64 and value.shape == want.shape, (tag, key)
        assert np.array_equal(value, want), (tag, key)
    assert got["temperatures"].shape == (n_t,) and got["densities"].shape == (n_d,) and got["rad_groups"].shape == (n_g + 1,)
    assert got["abs_opacity"].shape == (n_t, n_d)
    # the default call reads the grids alone
    bare = read_propaceos(g16.path(tag))
    assert all(bare[k] is None for k in g16.ALL) and np.array_equal(bare["temperatures"], got["temperatures"])


def test_reader_quirks_are_the_reference_s(tmp_path):
    """A later table asked for without the earlier ones is read from the earlier block; counts that are no multiple of ten lose
    their short line; a count <= 0 is refused with the reference's words."""
    from synthpy_amd.utils.eos_opacity import read_propaceos

    full = read_propaceos(g16.path("all"), **g16.flags("all"))
    only_abs = read_propaceos(g16.path("all"), need_abs_opacity=True)
    assert np.array_equal(only_abs["abs_opacity"], full["zf_table"]) and only_abs["zf_table"] is None
    lines = open(g16.path("all")).read().split("\n")
    bad = tmp_path / "zero.prp"
    bad.write_text("\n".join(lines[:38] + ["0"] + lines[39:]))
    with pytest.raises(ValueError, match="No temperature grid"):
        read_propaceos(str(bad))
    bad.write_text("\n".join(lines[:41] + ["-3"] + lines[42:]))
    with pytest.raises(ValueError, match="No density grid"):
        read_propaceos(str(bad))
    # 25 temperatures in three rows: 25 // 10 = 2 rows are read, the third is taken for the density count
    t = np.geomspace(1.0, 100.0, 25)
    rows = [" ".join(f"{v:.8E}" for v in t[k:k + 10]) for k in range(0, 25, 10)]
    bad.write_text("\n".join(lines[:38] + ["25"] + rows + lines[41:]))
    with pytest.raises(ValueError):
        read_propaceos(str(bad))
    short = tmp_path / "short.prp"
    short.write_text("\n".join(lines[:20]))
    with pytest.raises(StopIteration):
        read_propaceos(str(short))


def test_from_propaceos_round_trips():
    from synthpy_amd.utils.eos_opacity import ATOMIC_MASS_G, OpacityTable, read_propaceos

    for tag in g16.CASES:
        d = read_propaceos(g16.path(tag), **g16.flags(tag))
        t = OpacityTable.from_propaceos(d, A=12.011)
        assert t.n_band == 1 and t.A == 12.011 and t.m_ion == 12.011 * ATOMIC_MASS_G
        assert np.array_equal(t.temperatures, d["temperatures"]) and np.array_equal(t.densities, d["densities"])
        assert np.array_equal(t.absorption, d["abs_opacity"][None]) and np.array_equal(t.emission, d["emiss_opacity"][None])
        assert np.array_equal(t.edges, [[d["rad_groups"][0], d["rad_groups"][-1]]])
        assert np.array_equal(t.photon_energy, [np.sqrt(d["rad_groups"][0] * d["rad_groups"][-1])])
        LT, LD, LA, LE = t.logs()
        assert np.array_equal(LT, np.log(d["temperatures"])) and np.array_equal(LD, np.log(d["densities"]))
        assert np.array_equal(LA[0], np.log(d["abs_opacity"])) and np.array_equal(LE[0], np.log(d["emiss_opacity"]))
        assert all(a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] for a in (LT, LD, LA, LE))
    d = read_propaceos(g16.path("all"), need_zf_table=True, need_ross_opacity=True, need_emiss_opacity=True, need_abs_opacity=True)
    lte = dict(d, emiss_opacity=None)
    t = OpacityTable.from_propaceos(lte, A=1.008, photon_energy=12.4)
    assert t.emission is None and t.logs()[3] is None and np.array_equal(t.photon_energy, [12.4])
    with pytest.raises(ValueError, match="abs_opacity"):
        OpacityTable.from_propaceos(read_propaceos(g16.path("all")), A=12.0)


def test_opacity_table_validation_names_the_member():
    from synthpy_amd.utils.eos_opacity import OpacityTable

    T, D = np.geomspace(1.0, 500.0, 5), np.geomspace(1e17, 1e21, 4)
    k = np.full((2, 5, 4), 3.0)
    good = dict(temperatures=T, densities=D, absorption=k, photon_energy=[10.0, 90.0], A=12.0, emission=2 * k, edges=[[8, 12], [80, 100]])
    t = OpacityTable(**good)
    assert t.n_band == 2 and t.absorption.shape == (2, 5, 4) and t.edges.shape == (2, 2)
    assert OpacityTable(T, D, k[0], 10.0, 12.0).absorption.shape == (1, 5, 4)  # a 2-D table is one band

    def bad(member, **change):
        with pytest.raises(ValueError, match=member):
            OpacityTable(**dict(good, **change))

    for name, grid in (("temperatures", T), ("densities", D)):
        bad(name, **{name: grid[:1]})
        bad(name, **{name: np.geomspace(1.0, 2.0, 513)})
        bad(name, **{name: grid[::-1]})
        bad(name, **{name: np.r_[grid[:2], grid[1:]]})  # a repeated node: not strictly increasing
        bad(name, **{name: np.r_[-1.0, grid[1:]]})
        bad(name, **{name: np.r_[grid[:-1], np.inf]})
        bad(name, **{name: np.r_[grid[:-1], np.nan]})
        bad(name, **{name: grid.reshape(1, -1)})
    for name in ("absorption", "emission"):
        bad(name, **{name: k[:, :4]})
        bad(name, **{name: np.where(np.arange(4) == 2, 0.0, k)})
        bad(name, **{name: np.where(np.arange(4) == 1, np.nan, k)})
        bad(name, **{name: -k})
    bad("absorption", absorption=np.full((5, 5, 4), 3.0), emission=None, photon_energy=[1.0] * 5, edges=None)
    bad("emission", emission=k[:1])
    bad("photon_energy", photon_energy=[10.0])
    bad("photon_energy", photon_energy=[10.0, -1.0])
    bad("photon_energy", photon_energy=[10.0, np.nan])
    bad("edges", edges=[[8, 12]])
    bad("edges", edges=[[8, 12], [100, 80]])
    bad("edges", edges=[[8, 12], [80, np.inf]])
    for A in (0.0, -1.0, np.nan, np.inf):
        bad("A must", A=A)
