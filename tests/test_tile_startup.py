"""What a tile kernel does before its first RK4 step (trace_tile.inc): the entry cell comes from the binning (the packed cells of
k_keys_band / k_keys_band_rec, read through the launch order), the predicted exit cell from the cell's own reciprocal width, the
workgroup's box from a reduction in registers, and the node tables are filled while the first node planes are on their way.  None
of it may decide a ray's result: the tile's place only decides which rays a launch loses, and k_trace_f64 carries those to the same
bits.  So every GPU test here forces a tile kernel (SYNTHRAY_F64_TILE=1, tile_segments / tile_records asserted) against the
per-ray kernel (SYNTHRAY_F64_TILE=0) on the same rays and compares sf, rf, Jf bit for bit (NaN for NaN) and ray_steps: 33 node
planes in three segments (SYNTHRAY_TILE=...,11), the grids and the beam of tests/test_tile_cell_change.py plus the rays a start-up
can trip over.  The packed cells themselves are read back (RayBundle.binned_cells) and compared with numpy.searchsorted.
Needs an MI355X: -m gpu.
"""
import numpy as np
import pytest

from test_tile_cell_change import GRIDS, LWL, NA, _beam, _env, _grid, _same

TILE3 = "8,7,2,4,11"  # 32 steps in segments of 11 planes: three launches, two re-binnings
KERNELS = pytest.mark.parametrize("records", ["1", "0"], ids=["records", "producers"])


def _special(s0, axes, half, t_end):
    """The last rays of the bundle become the ones a start-up can trip over (the first ones are _beam's: rays on interior nodes,
    on the volume's first and last lateral nodes, a NaN position, a ray that turns around).  Nodes: the float32 numbers stored."""
    x, y, z = (np.asarray(g, np.float32).astype(np.float64) for g in axes)
    c = float(np.max(np.abs(s0[5])))
    q = s0.shape[1] - 1

    def put(px, py, pz, vx, vy, vz):
        nonlocal q
        s0[0:6, q] = (px, py, pz, vx, vy, vz)
        q -= 1

    for px, py in ((np.nextafter(x[0], -np.inf), 0.0), (np.nextafter(x[-1], np.inf), 0.0), (0.0, np.nextafter(y[0], -np.inf)),
                   (0.0, np.nextafter(y[-1], np.inf)), (np.nextafter(x[0], np.inf), np.nextafter(y[-1], -np.inf))):
        put(px, py, -1.01 * half[2], 0.0, 0.0, c)  # just outside the first / last lateral node (and just inside two of them)
    put(0.2 * half[0], 0.1 * half[1], -1.01 * half[2], 0.0, 0.0, 0.0)          # v_a = 0
    put(0.2 * half[0], 0.1 * half[1], -1.01 * half[2], 1e-3 * c, 0.0, -c)      # v_a < 0
    put(0.3 * half[0], -0.2 * half[1], 0.0, 1e-3 * c, 1e-3 * c, c)             # starts inside the volume
    put(0.3 * half[0], -0.2 * half[1], float(z[0]), 1e-3 * c, 1e-3 * c, c)     # starts ON the entry plane: no drift
    for f in (1.0 - 1e-12, 1.0, 1.0 + 1e-12):  # the vacuum drift takes tau just under, at and just over t_end
        put(0.1 * half[0], 0.1 * half[1], float(z[0]) - c * t_end * f, 0.0, 0.0, c)
    put(-0.4 * half[0], 0.3 * half[1], float(z[0]) - 0.5 * c * t_end, 2e-4 * c, -1e-4 * c, c)  # a long drift that arrives
    assert q > s0.shape[1] // 2
    return s0


def _run(eng, vol, s0, ext, keep=False, **env):
    with _env(**env):
        rays = eng.RayBundle(s0.shape[1]).upload(s0)
        st = rays.trace(vol, eng.default_t_end(ext), ext, precision="f64")
        out = rays.download()
        info = (rays.tile_segments, rays.tile_records)
        if keep:
            return out, st, info, rays
        rays.close()
    return out, st, info


@pytest.fixture(scope="module")
def eng():
    from synthpy_amd import engine

    engine.init(0)
    return engine


@pytest.fixture(scope="module")
def cases(eng):
    """Per grid: the volume, the bundle with the special rays and the per-ray kernel's result, formed once, shared, never changed."""
    out = {}
    for seed, tag in enumerate(("min uniform", "wide uniform", "wide stretched")):
        nx, ny, stretched = GRIDS[tag]
        axes, half, ne = _grid(nx, ny, stretched)
        ext = half[2] * 1.01
        s0 = _special(_beam(axes, half, 6_007 if nx < 12 else 20_011, 31 + seed), axes, half, eng.default_t_end(ext))
        vol = eng.Volume.from_ne(ne, *axes, LWL, "z", phaseshift=True)
        ref, st, info = _run(eng, vol, s0, ext, SYNTHRAY_F64_TILE="0")
        assert info[0] == 0
        out[tag] = {"axes": axes, "half": half, "ne": ne, "ext": ext, "s0": s0, "vol": vol, "ref": ref, "steps": st.ray_steps}
    yield out
    for c in out.values():
        c["vol"].close()


def _entry_cells(axes, s0):
    """(2, N) cells of the rays where they meet the entry plane, by the key kernel's rule restated in NumPy: the drift's
    arithmetic (p + v * tau, no fused multiply-add), a ray inside the closed lateral grid has the cell searchsorted finds (the
    last node belongs to the last cell), any other ray -1.  The nodes are the float32 numbers the library stores."""
    x, y, z = (np.asarray(g, np.float32).astype(np.float64) for g in axes)
    with np.errstate(all="ignore"):
        tau = (z[0] - s0[2]) / s0[5]
        drift = (s0[5] > 0) & (s0[2] < z[0])
        p = [np.where(drift, s0[0] + s0[3] * tau, s0[0]), np.where(drift, s0[1] + s0[4] * tau, s0[1])]
        inside = (p[0] >= x[0]) & (p[0] <= x[-1]) & (p[1] >= y[0]) & (p[1] <= y[-1])
    cells = np.full((2, s0.shape[1]), -1, np.int64)
    for q, g in enumerate((x, y)):
        ci = np.clip(np.searchsorted(g, p[q], side="right") - 1, 0, len(g) - 2)
        cells[q] = np.where(inside, ci, -1)
    return cells


def test_entry_cells_restated_on_hand_written_rays():
    """The NumPy restatement itself, on rays whose cells are known."""
    axes = (np.array([0.0, 1.0, 2.0, 4.0]), np.array([-1.0, 0.0, 3.0]), np.array([0.0, 1.0, 2.0]))
    s0 = np.zeros((9, 6))
    s0[5] = 1.0
    s0[2] = -1.0
    s0[0] = [0.0, 1.0, 3.9, 4.0, 4.1, np.nan]
    s0[1] = [-1.0, -0.5, 0.0, 3.0, 0.0, 0.0]
    s0[3, 1] = 0.5  # drifts from x = 1.0 to 1.5 on the entry plane: still cell 1
    assert _entry_cells(axes, s0).tolist() == [[0, 1, 2, 2, -1, -1], [0, 0, 1, 1, -1, -1]]


def test_binned_cells_refuses_null_arguments():
    """No device needed: the entry checks its arguments before anything else."""
    from synthpy_amd._ffi import lib

    assert lib.sr_rays_binned_cells(None, None) != 0


@pytest.mark.gpu
@KERNELS
@pytest.mark.parametrize("grid", ["min uniform", "wide uniform", "wide stretched"])
def test_three_segments_bit_for_bit(eng, cases, grid, records):
    """9 x 8 nodes: one tile, clamped on all four sides; 24 x 20 uniform; 24 x 20 with cell widths 1 : 3.5, where the cell handed
    down must be the non-uniform search's.  With the special rays: on and just outside the first and last lateral nodes, NaN,
    v_a <= 0, inside the volume, the vacuum drift with tau around t_end."""
    c = cases[grid]
    out, st, (segs, recs) = _run(eng, c["vol"], c["s0"], c["ext"], SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS=records,
                                 SYNTHRAY_TILE=TILE3, SYNTHRAY_TILE_CUTS=None)
    assert segs == 3 and recs == (records == "1"), (segs, recs)
    _same(out, c["ref"], (grid, records))
    assert st.ray_steps == c["steps"], (st.ray_steps, c["steps"])


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["min uniform", "wide uniform", "wide stretched"])
def test_packed_cells_are_the_search_sorted_cells(eng, cases, grid):
    """One segment from s0: the packed cells are by ray index, and equal the cells of the entry positions -- for every ray inside
    the lateral grid; every other ray has none."""
    c = cases[grid]
    out, st, (segs, recs), rays = _run(eng, c["vol"], c["s0"], c["ext"], keep=True, SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS="1",
                                       SYNTHRAY_TILE="8,7,2,4,32", SYNTHRAY_TILE_CUTS=None)
    try:
        got = rays.binned_cells()
    finally:
        rays.close()
    assert segs == 1 and recs
    want = _entry_cells(c["axes"], c["s0"])
    assert (want[0] >= 0).sum() > 0.5 * want.shape[1] and (want[0] < 0).sum() >= 5
    assert np.array_equal(got, want), int((got != want).any(axis=0).sum())
    _same(out, c["ref"], grid)


@pytest.mark.gpu
@KERNELS
def test_a_sparse_stripe_inside_a_dense_bundle(eng, cases, records):
    """Nine rays in ten sit in the first four cell columns, the rest is spread over the whole face: the workgroups of the sparse
    part have entry cells that span more than a tile, and lose the rays beyond it at the start."""
    c = cases["wide uniform"]
    x, y, _ = c["axes"]
    s0 = c["s0"].copy()
    n = s0.shape[1]
    rng = np.random.default_rng(5)
    dense = rng.random(n) < 0.9
    dense[:200] = dense[-20:] = False  # the special rays (80 at the front, 13 at the back) stay
    s0[1, dense] = y[0] + (y[4] - y[0]) * rng.random(int(dense.sum()))
    ref, st0, info = _run(eng, c["vol"], s0, c["ext"], SYNTHRAY_F64_TILE="0")
    assert info[0] == 0
    out, st, (segs, recs) = _run(eng, c["vol"], s0, c["ext"], SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS=records,
                                 SYNTHRAY_TILE=TILE3, SYNTHRAY_TILE_CUTS=None)
    assert segs == 3 and recs == (records == "1") and st.fallback_rays > 0, (segs, recs, st.fallback_rays)
    _same(out, ref, ("stripe", records))
    assert st.ray_steps == st0.ray_steps


@pytest.mark.gpu
@KERNELS
@pytest.mark.parametrize("n", [1, 255, 257, 3 * 256 + 1])
def test_bundle_sizes(eng, cases, records, n):
    """One ray, one short of a workgroup, one over, three workgroups and a ray: padding lanes and padding wavefronts take part in
    the box's reduction with the identity."""
    c = cases["min uniform"]
    s0 = np.ascontiguousarray(np.concatenate([c["s0"][:, : n - n // 2], c["s0"][:, c["s0"].shape[1] - n // 2:]], axis=1))
    assert s0.shape[1] == n
    ref, st0, info = _run(eng, c["vol"], s0, c["ext"], SYNTHRAY_F64_TILE="0")
    assert info[0] == 0
    out, st, (segs, recs) = _run(eng, c["vol"], s0, c["ext"], SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS=records,
                                 SYNTHRAY_TILE=TILE3, SYNTHRAY_TILE_CUTS=None)
    assert segs == 3 and recs == (records == "1"), (segs, recs)
    _same(out, ref, (n, records))
    assert st.ray_steps == st0.ray_steps


def _chain(eng, c, cuts, envs):
    """The bundle through a chain of slabs, slab q traced under envs[q]; the exit state, the steps, and the segments of each
    slab's trace."""
    s0, ext = c["s0"], c["ext"]
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    steps, segs, vols = 0, [], []
    for q, (lo, hi) in enumerate(cuts):
        vol = eng.Volume.from_ne_slab(eng.slab_source(c["ne"], 2, lo, hi), *c["axes"], LWL, "z", lo, hi, phaseshift=True)
        vols.append(vol)
        with _env(**envs[q]):
            st = rays.trace(vol, eng.default_t_end(ext), ext, precision="f64",
                            handoff=(eng.HANDOFF_ENTER if q else 0) | (eng.HANDOFF_EXIT if q + 1 < len(cuts) else 0))
        steps += st.ray_steps
        segs.append((rays.tile_segments, rays.tile_records))
    out = rays.download()
    rays.close()
    for vol in vols:
        vol.close()
    return out, steps, segs


@pytest.mark.gpu
@KERNELS
@pytest.mark.parametrize("first_tiled", [True, False], ids=["tile then tile", "per-ray then tile"])
def test_two_slabs_with_handoff_enter(eng, cases, records, first_tiled):
    """Two slabs of 17 node planes, three segments each: the second slab's first launch reads ARRIVALS through k_keys_band_rec's
    cells -- also when the first slab ran the per-ray kernel and the bundle has never been binned by band before.  Against the
    per-ray kernel through the same chain."""
    c = cases["wide stretched"]
    cuts = [(0, 16), (16, NA - 1)]
    per_ray = dict(SYNTHRAY_F64_TILE="0")
    tile = dict(SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS=records, SYNTHRAY_TILE="8,7,2,4,6", SYNTHRAY_TILE_CUTS=None)
    ref, steps0, segs0 = _chain(eng, c, cuts, [per_ray, per_ray])
    assert all(s == 0 for s, _ in segs0)
    out, steps, segs = _chain(eng, c, cuts, [tile if first_tiled else per_ray, tile])
    assert segs == [(3, records == "1") if first_tiled else (0, False), (3, records == "1")], segs
    _same(out, ref, ("slabs", records, first_tiled))
    assert steps == steps0


@pytest.mark.gpu
@KERNELS
@pytest.mark.parametrize("direction", ["x", "y", "z"])
def test_each_probing_axis(eng, cases, records, direction):
    """The same volume and beam turned so that the rays probe along x, y and z: the lateral axes b, c = (axis + 1, axis + 2) % 3
    take every pair of physical axes."""
    c = cases["wide stretched"]
    a = "xyz".index(direction)
    # the z-beam's axes (x, y, z) become the physical axes ((a + 1) % 3, (a + 2) % 3, a)
    order = [(a + 1) % 3, (a + 2) % 3, a]
    axes, s0 = [None] * 3, c["s0"].copy()
    for src, dst in enumerate(order):
        axes[dst] = c["axes"][src]
        s0[dst], s0[3 + dst] = c["s0"][src], c["s0"][3 + src]
    ne = np.ascontiguousarray(np.transpose(c["ne"], np.argsort(order)))
    assert ne.shape == tuple(len(g) for g in axes)
    ext = c["ext"]
    vol = eng.Volume.from_ne(ne, *axes, LWL, direction, phaseshift=True)
    try:
        ref, st0, info = _run(eng, vol, s0, ext, SYNTHRAY_F64_TILE="0")
        assert info[0] == 0 and np.isfinite(ref[0]).all(axis=0).sum() > 0.5 * s0.shape[1]
        out, st, (segs, recs) = _run(eng, vol, s0, ext, SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS=records, SYNTHRAY_TILE=TILE3,
                                     SYNTHRAY_TILE_CUTS=None)
        assert segs == 3 and recs == (records == "1"), (segs, recs)
        _same(out, ref, (direction, records))
        assert st.ray_steps == st0.ray_steps
    finally:
        vol.close()
