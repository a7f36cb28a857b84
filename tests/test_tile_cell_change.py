"""The tile kernels' cell-change regions (relocate2, trace_tile.inc): a ray that leaves its cell steps to the neighbour its weight
points at -- integer arithmetic on the weight's high word, no clamp of the index -- and the tile's node tables end in sentinel
entries that must reject a step off the tile.  A wrong step, a wrong table entry or a sentinel that accepts keeps a ray in the
wrong cell: its result differs from k_trace_f64's, which searches the volume's own node arrays.  So every test here compares sf,
rf, Jf bit for bit (NaN for NaN) and ray_steps between a tile kernel forced (SYNTHRAY_F64_TILE=1, tile_segments and
tile_records asserted) and the per-ray kernel (SYNTHRAY_F64_TILE=0) on the same rays, on the smallest grids at which a region
can go wrong: 9 x 8 lateral nodes (the records kernel's minimum, 8 x 7 cells: ONE tile, clamped on all four sides) and 24 x 20,
each uniform and with cell widths that alternate 1 : 3.5; 33 node planes, three lateral cells apart, so that a divergent beam
(0.035 rad) crosses a cell face every ten planes.  That every kind of cell change occurs (+b, -b, +c, -c, both axes between two
planes) is counted from the per-ray kernel's own plane-by-plane states (two-plane slabs chained by the hand-off records) and
asserted.  Needs an MI355X: -m gpu.
"""
import os

import numpy as np
import pytest

LWL = 1064e-9
NA = 33  # node planes along z
DX = 1e-4  # mean lateral cell width; the node planes are 3 * DX apart
DIV = 0.035

GRIDS = {"min uniform": (9, 8, False), "min stretched": (9, 8, True), "wide uniform": (24, 20, False), "wide stretched": (24, 20, True)}


def _axis(n, stretched):
    """n nodes centred on 0: equal cells, or cell widths alternating 1 : 3.5 (neighbours differ by more than 3 x)."""
    w = np.where(np.arange(n - 1) % 2 == 0, 1.0, 3.5) if stretched else np.ones(n - 1)
    w = w * (DX * (n - 1) / w.sum())
    x = np.concatenate([[0.0], np.cumsum(w)])
    return x - 0.5 * x[-1]


def _grid(nx, ny, stretched):
    axes = (_axis(nx, stretched), _axis(ny, stretched), np.linspace(-0.5 * (NA - 1) * 3 * DX, 0.5 * (NA - 1) * 3 * DX, NA))
    half = [a[-1] for a in axes]
    X, Y, Z = np.meshgrid(*axes, indexing="ij", sparse=True)
    r2 = ((X - 0.1 * half[0]) / (0.5 * half[0])) ** 2 + ((Y + 0.07 * half[1]) / (0.5 * half[1])) ** 2 + (Z / (0.45 * half[2])) ** 2
    ne = 1e25 * np.exp(-r2) * (1.0 + 0.15 * np.sin(5.0 * X / half[0] + 3.0 * Y / half[1]) * np.cos(4.0 * Z / half[2]))
    return axes, half, ne


def _beam(axes, half, n, seed):
    """A divergent square beam over 1.15 x the lateral faces, started before the first node plane -- and the rays a cell search
    can trip over: on interior nodes (weight exactly 0), on the volume's first and last lateral nodes, a NaN position, a slow
    ray the density hill turns around; the overfill and the divergence make rays leave sideways."""
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    np.random.seed(seed)
    s0 = init_beam(n, 1.0, DIV, half[2] * 1.01, "square", "z")
    s0[0] *= 1.15 * half[0]
    s0[1] *= 1.15 * half[1]
    x, y, z = axes
    c = float(np.max(np.abs(s0[5])))
    q = 0
    for ix in range(1, len(x) - 1, 2):  # on interior nodes, parallel to the axis: w = 0 exactly in every stage until deflected
        for iy in range(1, len(y) - 1, 3):
            s0[0, q], s0[1, q], s0[3, q], s0[4, q] = x[ix], y[iy], 0.0, 0.0
            q += 1
    for ix, iy in ((0, 0), (0, len(y) - 1), (len(x) - 1, 0), (len(x) - 1, len(y) - 1), (0, 3), (len(x) - 1, 4), (3, 0), (4, len(y) - 1)):
        s0[0, q], s0[1, q], s0[3, q], s0[4, q] = x[ix], y[iy], 0.0, 0.0  # the volume's first and last lateral nodes
        q += 1
    for ix in (2, 5):  # on a node along b, moving along c (and the other way round): one weight exactly 0, the other changing
        s0[0, q], s0[3, q] = x[ix], 0.0
        s0[1, q + 1], s0[4, q + 1] = y[ix], 0.0
        q += 2
    s0[0, q] = np.nan  # a NaN position
    q += 1
    # on the first node plane, creeping up the density hill: its axial velocity turns negative inside the volume
    s0[0, q], s0[1, q], s0[2, q] = 0.1 * half[0], -0.07 * half[1], z[0]
    s0[3, q], s0[4, q], s0[5, q] = 1e-4 * c, -1e-4 * c, 2e-3 * c
    assert q < n // 4
    return np.ascontiguousarray(s0)


class _env:
    """Environment variables for the traces inside the block; what was there before comes back."""

    def __init__(self, **kv):
        self.set = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.set}
        for k, v in self.set.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _trace(eng, vol, s0, ext, **env):
    with _env(**env):
        rays = eng.RayBundle(s0.shape[1]).upload(s0)
        st = rays.trace(vol, eng.default_t_end(ext), ext, precision="f64")
        out = rays.download()
        info = (rays.tile_segments, rays.tile_records)
        rays.close()
    return out, st, info


def _same(got, ref, what):
    for u, w, name in zip(got, ref, ("sf", "rf", "Jf")):
        assert np.array_equal(u, w, equal_nan=True), (what, name, int((~((u == w) | ((u != u) & (w != w)))).sum()))


def _plane_cells(eng, axes, ne, s0, ext):
    """(NA, 2, N) lateral cell indices of every ray on every node plane (-1: not a plane-form ray there, or outside the grid),
    from the per-ray kernel through two-plane slabs chained by the hand-off records (bit-equal to the whole trace)."""
    n = s0.shape[1]
    cells = np.full((NA, 2, n), -1)
    with _env(SYNTHRAY_F64_TILE="0"):
        rays = eng.RayBundle(n).upload(s0)
        for lo in range(NA - 2):  # the state on plane lo + 1 as slab (lo, lo + 1) hands it on
            vol = eng.Volume.from_ne_slab(eng.slab_source(ne, 2, lo, lo + 1), *axes, LWL, "z", lo, lo + 1, phaseshift=True)
            rays.trace(vol, eng.default_t_end(ext), ext, precision="f64", handoff=(eng.HANDOFF_ENTER if lo else 0) | eng.HANDOFF_EXIT)
            rec = rays.handoff_download()
            vol.close()
            ok = np.isfinite(rec[0]) & np.isfinite(rec[1]) & np.isfinite(rec[2]) & np.isfinite(rec[9])
            idx = rec[9, ok].astype(np.int64)
            for q in (0, 1):
                g = axes[q]
                p = rec[q, ok]
                ci = np.searchsorted(g, p, side="right") - 1
                cells[lo + 1, q, idx] = np.where((p >= g[0]) & (p < g[-1]), ci, -1)
        rays.close()
    return cells


def _changes(cells):
    """How often a ray is in another cell on the next node plane, by kind."""
    a, b = cells[1:-1], cells[2:]  # plane 0 is not recorded
    both = (a >= 0).all(axis=1) & (b >= 0).all(axis=1)
    db, dc = (b[:, 0] - a[:, 0])[both], (b[:, 1] - a[:, 1])[both]
    return {"+b": int((db > 0).sum()), "-b": int((db < 0).sum()), "+c": int((dc > 0).sum()), "-c": int((dc < 0).sum()),
            "both": int(((db != 0) & (dc != 0)).sum())}


@pytest.fixture(scope="module")
def eng():
    from synthpy_amd import engine

    engine.init(0)
    return engine


@pytest.fixture(scope="module")
def cases(eng):
    """Per grid: the volume, the bundle and the per-ray kernel's result, formed once, shared by the tests, never changed."""
    out = {}
    for seed, (tag, (nx, ny, stretched)) in enumerate(GRIDS.items()):
        axes, half, ne = _grid(nx, ny, stretched)
        ext = half[2] * 1.01
        s0 = _beam(axes, half, 6_007 if nx < 12 else 20_011, 11 + seed)
        vol = eng.Volume.from_ne(ne, *axes, LWL, "z", phaseshift=True)
        ref, st, info = _trace(eng, vol, s0, ext, SYNTHRAY_F64_TILE="0")
        assert info[0] == 0
        out[tag] = {"axes": axes, "half": half, "ne": ne, "ext": ext, "s0": s0, "vol": vol, "ref": ref, "steps": st.ray_steps}
    yield out
    for c in out.values():
        c["vol"].close()


def test_the_grids_are_what_the_header_says():
    for nx, ny, stretched in GRIDS.values():
        for n in (nx, ny):
            w = np.diff(_axis(n, stretched))
            assert np.all(w > 0) and abs(w.sum() - DX * (n - 1)) < 1e-18
            if stretched:
                assert np.all(np.maximum(w[1:] / w[:-1], w[:-1] / w[1:]) >= 3.0)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_every_kind_of_cell_change_occurs(eng, cases, grid):
    """A condition of the tests below, not a measurement: between two node planes rays step up and down along either axis, and
    along both at once, ten times at the very least; and the special rays are what they are meant to be."""
    c = cases[grid]
    n = _changes(_plane_cells(eng, c["axes"], c["ne"], c["s0"], c["ext"]))
    print(grid, n)
    assert all(v >= 10 for v in n.values()), n
    sf = c["ref"][0]
    assert np.isnan(sf).any() and np.isfinite(sf).all(axis=0).sum() > 0.5 * sf.shape[1]


@pytest.mark.gpu
@pytest.mark.parametrize("records", ["1", "0"], ids=["records", "producers"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_cell_changes_bit_for_bit(eng, cases, grid, records):
    """One segment over all 33 planes, 8 x 7 tiles: on the 9 x 8 grid the tile is the whole volume and every step off it is a
    step out of the volume; on the wide grid tiles sit inside and at the edges."""
    c = cases[grid]
    out, st, (segs, recs) = _trace(eng, c["vol"], c["s0"], c["ext"], SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS=records,
                                   SYNTHRAY_TILE="8,7,2,4,32", SYNTHRAY_TILE_CUTS=None)
    assert segs == 1 and recs == (records == "1"), (segs, recs)
    _same(out, c["ref"], (grid, records))
    assert st.ray_steps == c["steps"], (st.ray_steps, c["steps"])


@pytest.mark.gpu
@pytest.mark.parametrize("records", ["1", "0"], ids=["records", "producers"])
@pytest.mark.parametrize("grid", ["wide uniform", "wide stretched"])
def test_tiles_smaller_than_the_cloud_lose_rays_on_every_side(eng, cases, grid, records):
    """8 x 5 tiles with a halo of one cell under a divergent beam: rays step off their tile on all four sides -- the sentinel
    entries below node 0 and from node T on -- and are carried by k_trace_f64."""
    c = cases[grid]
    out, st, (segs, recs) = _trace(eng, c["vol"], c["s0"], c["ext"], SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS=records,
                                   SYNTHRAY_TILE="8,5,1,3,7", SYNTHRAY_TILE_CUTS=None)
    assert segs == 5 and recs == (records == "1"), (segs, recs)
    assert st.fallback_rays > 0
    _same(out, c["ref"], (grid, records))
    assert st.ray_steps == c["steps"], (st.ray_steps, c["steps"])


@pytest.mark.gpu
@pytest.mark.parametrize("records", ["1", "0"], ids=["records", "producers"])
@pytest.mark.parametrize("grid", ["min stretched", "wide stretched"])
def test_short_segments(eng, cases, grid, records):
    """Segments of five planes: cell changes in the first and the last step of a segment, the cell found again from the
    hand-off record at every start."""
    c = cases[grid]
    out, st, (segs, recs) = _trace(eng, c["vol"], c["s0"], c["ext"], SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS=records,
                                   SYNTHRAY_TILE="8,7,2,4,5", SYNTHRAY_TILE_CUTS=None)
    assert segs == 7 and recs == (records == "1"), (segs, recs)
    _same(out, c["ref"], (grid, records))
    assert st.ray_steps == c["steps"], (st.ray_steps, c["steps"])


@pytest.mark.gpu
def test_optional_terms_kernel(eng, cases):
    """The optional-terms tile kernel (a volume with kappa and B; 6 x 7 tiles) shares relocate2 with its own record layout."""
    c = cases["wide stretched"]
    axes, ne = c["axes"], c["ne"]
    X, Y, Z = np.meshgrid(*axes, indexing="ij", sparse=True)
    kappa = 3e9 * ne / ne.max() * (1.0 + 0.2 * np.cos(2e4 * X))
    B = np.stack([5.0 + 0 * ne, 2.0 * np.sin(1e4 * Y) + 0 * ne, 8.0 * np.cos(3e3 * Z) + 0 * ne], axis=-1)
    vol = eng.Volume.from_ne(ne, *axes, LWL, "z", phaseshift=True)
    vol.attach_aux(np.ascontiguousarray(kappa), np.ascontiguousarray(ne), np.ascontiguousarray(B), 2.6e-13)
    try:
        ref, st0, info = _trace(eng, vol, c["s0"], c["ext"], SYNTHRAY_F64_TILE="0")
        assert info[0] == 0
        for tile, n_seg in ((None, 1), ("6,5,1,3,7", 5)):
            out, st, (segs, recs) = _trace(eng, vol, c["s0"], c["ext"], SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE=tile, SYNTHRAY_TILE_CUTS=None)
            assert segs == n_seg and not recs, (tile, segs, recs)
            _same(out, ref, ("aux", tile))
            assert st.ray_steps == st0.ray_steps, (tile, st.ray_steps, st0.ray_steps)
    finally:
        vol.close()
