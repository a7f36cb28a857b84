"""The launch order of the ray binning, checked by itself: k_keys / k_keys_band / k_keys_band_rec, k_bin_count, k_scan_blocks /
k_scan / k_scan_add, k_bin_coarse and k_bin_fine (trace.hip: bin_rays, bin_by_band; the head of trace_tile.inc).

Every other test sees that chain only through "a sorted trace returns the bits of an unsorted one", which any permutation
passes.  Here the order is read back (RayBundle.launch_order, sr_rays_launch_order) and compared with a NumPy restatement of
the keys, written from the comments in the sources: the entry-plane projection, the cell rule, the Morton key, the band key and
the host's choice of shift, lo_bits and the key of the dead rays.  The library is built without fused multiply-adds, so the
restatement's arithmetic is the kernels' operation for operation and the comparison is exact:

  (a) np.sort(order) == arange(N);
  (b) key_ref[order] is non-decreasing; hence (c) the dead rays -- outside the lateral grid, NaN, v_a <= 0 between segments --
      are one run at the tail, as long as the restatement's count of them.

The per-ray float64 kernel also gives the same sf, bit for bit, with and without the sort, in every case.  The volumes are thin
(3 node planes along the probing axis unless a case says otherwise) and the shapes the smallest at which each path of the sort
exists.  The CPU tests check the restatement against cases written out by hand; the rest needs an MI355X (-m gpu).
"""
from collections import namedtuple

import numpy as np
import pytest

from test_tile_step_loop import _cuts, _env

LWL = 1064e-9
C_LIGHT = 299792458.0
CELL = 2.0 ** -12   # [m] 0.244 mm; a node is an integer (< 2^24) times 2^-13 m: a float32 number, as the library stores them
K_BIN_TILE = 4096   # rays per workgroup of the sort (trace.hip: kBinTile)
K_SCAN_BLOCK = 2048  # counts per workgroup of k_scan_blocks, and the LDS counters of a sort level (kScanPerBlock, kBinMaxDigits)
K_SCAN_CHUNK = 1024  # block totals per pass of k_scan


# ================================================================ the restatement (NumPy, from the comments in the sources)
def cell_of(g, p):
    """The cell rule: the largest i with g[i] <= p, clipped to n - 2 (the last node belongs to the last cell); -1 for p outside
    [g[0], g[n-1]] and for NaN -- such a ray goes behind every cell."""
    g = np.asarray(g, np.float64)
    p = np.asarray(p, np.float64)
    inside = (p >= g[0]) & (p <= g[-1])
    i = np.searchsorted(g, np.where(inside, p, g[0]), side="right") - 1
    return np.where(inside, np.minimum(i, len(g) - 2), -1)


def entry_point(s0, a, ga0):
    """Where a ray meets the entry plane: only for v_a > 0 and p_a < g_a[0] (tau = (g_a[0] - p_a) / v_a, p + v * tau); every other
    ray -- started inside, flying backwards, NaN in p_a or v_a -- is taken where it is."""
    b, c = (a + 1) % 3, (a + 2) % 3
    pa, pb, pc, va, vb, vc = s0[a], s0[b], s0[c], s0[3 + a], s0[3 + b], s0[3 + c]
    with np.errstate(all="ignore"):
        hit = (va > 0) & (pa < ga0)
        tau = (ga0 - pa) / va
        return np.where(hit, pb + vb * tau, pb), np.where(hit, pc + vc * tau, pc)


def spread_bits(v):
    """bit k of v on position 2k"""
    v = np.asarray(v, np.uint64)
    out = np.zeros_like(v)
    for k in range(16):
        out |= ((v >> np.uint64(k)) & np.uint64(1)) << np.uint64(2 * k)
    return out


def morton_plan(ncb, ncc):
    """sr_rays_trace's choice for ncb x ncc lateral cells: (shift, lo_bits, key of the dead rays).  `bits` holds the longer axis;
    past 11 bits (2048 cells, the LDS counters of a sort level) the key is that of the coarser cell, 2^shift cells a side; the
    sort's fine digit is the low lo_bits = bits key bits, and 2^(2 bits) is one more coarse group behind all cells."""
    bits = 1
    while (1 << bits) < max(ncb, ncc):
        bits += 1
    shift = max(0, bits - 11)
    bits -= shift
    return shift, bits, 1 << (2 * bits)


def morton_key(ib, ic, shift=0):
    """Morton key of (ib >> shift, ic >> shift), ib's bits on the odd positions"""
    return ((spread_bits(np.asarray(ib) >> shift) << np.uint64(1)) | spread_bits(np.asarray(ic) >> shift)).astype(np.int64)


def band_plan(ncb, ncc, band):
    """bin_by_band's choice: (shift, lo_bits, key of the dead rays).  Bands of `band` cell rows: n_keys = bands * ncc * band keys;
    more than 2^22 of them drop low key bits; the dead key is one past the last cell's; lo_bits: half of its bits, rounded up,
    11 at most."""
    n_keys = -(-ncb // band) * ncc * band
    bits = 1
    while (1 << bits) < n_keys:
        bits += 1
    shift = max(0, bits - 22)
    dead = ((n_keys - 1) >> shift) + 1
    bits = 1
    while (1 << bits) <= dead:
        bits += 1
    return shift, min(11, (bits + 1) // 2), dead


def band_key(ib, ic, ncc, band, shift=0):
    """((bnd * ncc + col) * band + row) >> shift: bands of `band` rows along b, inside a band by column -- reversed in odd bands
    --, inside a column by row"""
    ib, ic = np.asarray(ib, np.int64), np.asarray(ic, np.int64)
    bnd, row = ib // band, ib % band
    col = np.where(bnd % 2 == 1, ncc - 1 - ic, ic)
    return ((bnd * ncc + col) * band + row) >> shift


def keys_at(gb, gc, qb, qc, alive=None, band=None):
    """(key_ref, dead key) of rays at lateral positions (qb, qc): the Morton key (band None) or the band key of their cells;
    rays outside the grid, NaN rays and rays that are not `alive` get the dead key."""
    ncb, ncc = len(gb) - 1, len(gc) - 1
    ib, ic = cell_of(gb, qb), cell_of(gc, qc)
    live = (ib >= 0) & (ic >= 0)
    if alive is not None:
        live &= alive
    ib, ic = np.where(live, ib, 0), np.where(live, ic, 0)
    if band is None:
        shift, _, dead = morton_plan(ncb, ncc)
        key = morton_key(ib, ic, shift)
    else:
        shift, _, dead = band_plan(ncb, ncc, band)
        key = band_key(ib, ic, ncc, band, shift)
    return np.where(live, key, dead).astype(np.int64), dead


def near_a_node(gb, gc, qb, qc, tol=1e-12):
    """rays whose position lies within tol of a lateral node: a rounding of the stepped position could change their cell"""
    out = np.zeros(np.shape(qb), bool)
    for g, q in ((gb, qb), (gc, qc)):
        g = np.asarray(g, np.float64)
        with np.errstate(invalid="ignore"):
            j = np.clip(np.searchsorted(g, np.nan_to_num(q)), 1, len(g) - 1)
            out |= np.minimum(np.abs(q - g[j - 1]), np.abs(q - g[j])) <= tol
    return out


# ================================================================ grids and rays
Grid = namedtuple("Grid", "axes a b c ga gb gc ext ne")


def _axis(n, rng=None, scale=1.0):
    """n nodes, float32 numbers all: uniform cells of CELL * scale, or (rng) widths of 1 to 5 half cells -- where find_cell's
    first guess is wrong and it walks"""
    w = np.ones(n - 1) * 2.0 if rng is None else rng.integers(1, 6, n - 1).astype(np.float64)
    g = np.concatenate([[0.0], np.cumsum(w)])
    g = (g - g[(n - 1) // 2]) * (0.5 * CELL * scale)
    assert np.array_equal(g, g.astype(np.float32).astype(np.float64))
    return g


def make_grid(na, nb, nc, pdir="z", rng=None, a_scale=1.0, vacuum=False):
    """(na, nb, nc) nodes along the probing axis and the lateral axes b = (a+1)%3, c = (a+2)%3; ne: a smooth blob, or zero"""
    a = "xyz".index(pdir)
    b, c = (a + 1) % 3, (a + 2) % 3
    axes = [None] * 3
    axes[a], axes[b], axes[c] = _axis(na, scale=a_scale), _axis(nb, rng), _axis(nc, rng)
    X = np.meshgrid(*axes, indexing="ij", sparse=True)
    w = [max(0.4 * (g[-1] - g[0]), CELL) for g in axes]
    ne = 1e25 * np.exp(-sum(((X[k] - 0.1 * w[k]) / w[k]) ** 2 for k in range(3)))
    ne = np.ascontiguousarray(np.broadcast_to(ne, tuple(len(g) for g in axes))) * (0.0 if vacuum else 1.0)
    return Grid(tuple(axes), a, b, c, axes[a], axes[b], axes[c], float(-axes[a][0] * 1.25), ne)


def make_rays(G, n, seed, fill=1.0, div=0.0, dead=True):
    """n rays uniform over `fill` of the lateral faces, started before the entry plane, lateral angles N(0, div); dead: every
    37th ray NaN and every 41st outside the lateral grid, spread over every tile of the sort"""
    rng = np.random.default_rng(seed)
    s0 = np.zeros((9, n))
    for ax, g in ((G.b, G.gb), (G.c, G.gc)):
        mid, half = 0.5 * (g[0] + g[-1]), 0.5 * (g[-1] - g[0])
        s0[ax] = mid + fill * half * (2.0 * rng.random(n) - 1.0)
        s0[3 + ax] = C_LIGHT * div * rng.standard_normal(n)
    s0[G.a] = -G.ext
    s0[3 + G.a] = C_LIGHT
    s0[6] = 1.0
    if dead:
        i = np.arange(n)
        s0[:6, i % 37 == 5] = np.nan
        out = i % 41 == 7
        s0[G.b, out] = G.gb[-1] + CELL
        s0[3 + G.b, out] = s0[3 + G.c, out] = 0.0  # they stay outside
    return s0


def entry_keys(G, s0, band=None):
    qb, qc = entry_point(s0, G.a, G.ga[0])
    return keys_at(G.gb, G.gc, qb, qc, band=band)


# ================================================================ CPU: the restatement against cases written out by hand
def test_morton_keys_of_a_4x4_grid():
    want = [[0, 1, 4, 5], [2, 3, 6, 7], [8, 9, 12, 13], [10, 11, 14, 15]]  # [ib][ic]: ib's bits on the odd positions
    ib, ic = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    assert morton_key(ib, ic).tolist() == want
    assert morton_key(ib * 2 + 1, ic * 2, 1).tolist() == want  # the coarser cell
    assert morton_plan(4, 4) == (0, 2, 16) and morton_plan(3, 4) == (0, 2, 16) and morton_plan(5, 2) == (0, 3, 64)
    assert morton_key(2047, 2047) == (1 << 22) - 1 and morton_key(1024, 1) == (1 << 21) + 1


def test_band_order_of_a_5x3_grid_at_band_2():
    """bands {0, 1}, {2, 3}, {4}: band 0 by column 0 1 2, band 1 by column 2 1 0 (boustrophedon), the last band one row"""
    want = [[0, 2, 4], [1, 3, 5], [10, 8, 6], [11, 9, 7], [12, 14, 16]]  # [ib][ic]
    ib, ic = np.meshgrid(np.arange(5), np.arange(3), indexing="ij")
    assert band_key(ib, ic, 3, 2).tolist() == want
    assert band_plan(5, 3, 2) == (0, 3, 18)  # 18 keys; the dead key 18 has 5 bits: 3 low ones
    walk = sorted((k, r, q) for r, row in enumerate(want) for q, k in enumerate(row))  # neighbours in the order are neighbours
    steps = [abs(r1 - r0) + abs(q1 - q0) for (_, r0, q0), (_, r1, q1) in zip(walk[:-1], walk[1:])]
    assert max(steps[:11]) <= 2 and steps[5] == 1, steps  # band 0 ends in column 2, band 1 begins there
    assert band_plan(8, 8, 1) == (0, 4, 64) and band_plan(9, 8, 8) == (0, 4, 128)
    assert band_plan(4096, 1099, 2)[0] == 1  # 4.5e6 keys: one low bit dropped


def test_cell_rule_and_last_node():
    g = np.array([0.0, 1.0, 2.0, 4.0])
    p = [0.0, np.nextafter(1.0, 0.0), 1.0, 2.0, 3.9, 4.0, np.nextafter(4.0, 5.0), -5e-324, np.nan, np.inf]
    assert cell_of(g, p).tolist() == [0, 0, 1, 2, 2, 2, -1, -1, -1, -1]
    assert cell_of([0.0, 1.0], [0.0, 0.5, 1.0, 1.5]).tolist() == [0, 0, 0, -1]  # one cell
    key, dead = keys_at(g, g, np.array([4.0, 4.0, 5.0, np.nan]), np.array([0.0, 4.0, 1.0, 1.0]))
    assert dead == 16 and key.tolist() == [int(morton_key(2, 0)), int(morton_key(2, 2)), 16, 16]


def test_host_choices_of_shift_and_digits():
    assert morton_plan(8, 4099) == (2, 11, 1 << 22)   # 4099 cells: 13 bits, the key of a 4 x 4 block of cells
    assert morton_plan(2049, 8) == (1, 11, 1 << 22)
    assert morton_plan(2048, 2048) == (0, 11, 1 << 22)
    assert morton_plan(1025, 2) == (0, 11, 1 << 22)   # 1025 to 2048 cells: 2^11 + 1 = 2049 coarse groups
    assert morton_plan(1024, 2) == (0, 10, 1 << 20)
    assert morton_plan(31, 33) == (0, 6, 1 << 12) and morton_plan(31, 32) == (0, 5, 1 << 10)  # bits crosses 5 to 6
    assert morton_plan(1, 1) == (0, 1, 4)             # one lateral cell: bits = 1, three coarse groups
    assert morton_key(4098, 7, 2) == morton_key(1024, 1) and morton_key(4095, 3, 2) == morton_key(1023, 0)


def test_entry_projection_only_before_the_plane():
    """v_a > 0 and p_a < g_a[0], nothing else: a ray on the plane, inside, flying backwards or with a NaN is taken where it is"""
    s0 = np.zeros((9, 6))
    s0[2] = [-2.0, -1.0, 0.0, -2.0, np.nan, -2.0]   # p_a; the entry plane is at -1
    s0[5] = [2.0, 2.0, 2.0, -2.0, 2.0, np.nan]      # v_a
    s0[0], s0[3] = 0.25, 1.0                        # p_b, v_b
    s0[1], s0[4] = -0.5, -3.0                       # p_c, v_c
    qb, qc = entry_point(s0, 2, -1.0)
    assert qb.tolist() == [0.75, 0.25, 0.25, 0.25, 0.25, 0.25] and qc.tolist() == [-2.0, -0.5, -0.5, -0.5, -0.5, -0.5]


def _rebin_case():
    """The re-binning case: 13 node planes four cells apart, vacuum, 32 x 25 lateral cells, a beam whose rays cross about a
    cell per segment; SYNTHRAY_TILE = 8,8,2,2,4 cuts the 12 steps into 5 + 4 + 3.  (grid, s0, last cut plane, positions there)"""
    G = make_grid(13, 33, 26, a_scale=4.0, vacuum=True)
    s0 = make_rays(G, 40_003, seed=11, fill=0.75, div=0.06)
    cut = _cuts(len(G.ga) - 1, 4, [])
    with np.errstate(all="ignore"):
        tau = (G.ga[cut[-2]] - s0[G.a]) / s0[3 + G.a]
        qb, qc = s0[G.b] + s0[3 + G.b] * tau, s0[G.c] + s0[3 + G.c] * tau
    return G, s0, cut, qb, qc


def test_rebinning_case_is_well_posed():
    G, s0, cut, qb, qc = _rebin_case()
    assert cut == [0, 5, 9, 12]
    assert not near_a_node(G.gb, G.gc, qb, qc).any()  # the seed leaves no ray within 1e-12 m of a node on the last cut plane
    eb, ec = entry_point(s0, G.a, G.ga[0])
    live = (cell_of(G.gb, eb) >= 0) & (cell_of(G.gc, qc) >= 0) & (cell_of(G.gb, qb) >= 0) & (cell_of(G.gc, ec) >= 0)
    moved = (cell_of(G.gb, eb) != cell_of(G.gb, qb)) | (cell_of(G.gc, ec) != cell_of(G.gc, qc))
    assert moved[live].mean() > 0.5  # most rays are in another cell by the last cut
    for G2, s2, p2 in _handoff_cases():
        assert not near_a_node(G2.gb, G2.gc, *p2).any()


def _handoff_cases():
    """The tile path's slab chain: 5 node planes four cells apart in vacuum, slabs of planes 0..2 and 2..4.  (grid, s0,
    positions on the shared plane)"""
    G = make_grid(5, 33, 26, a_scale=4.0, vacuum=True)
    s0 = make_rays(G, 40_003, seed=12, fill=0.75, div=0.06)
    with np.errstate(all="ignore"):
        tau = (G.ga[2] - s0[G.a]) / s0[3 + G.a]
        pos = s0[G.b] + s0[3 + G.b] * tau, s0[G.c] + s0[3 + G.c] * tau
    return [(G, s0, pos)]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from synthpy_amd import _ffi

    return _ffi


def test_launch_order_checks_its_arguments_before_the_device(built):
    buf = np.zeros(4, np.uint32)
    for r, order in ((None, built.ptr(buf)), (None, None)):
        assert built.lib.sr_rays_launch_order(r, order) == -1 and "sr_rays_launch_order: NULL" in built.last_error()
    assert built.lib.sr_rays_set_count(None, 1) == -1 and "sr_rays_set_count: NULL" in built.last_error()
    assert not buf.any()


# ================================================================ GPU
@pytest.fixture(scope="module")
def eng():
    from synthpy_amd import engine

    if engine.device_count() == 0:
        pytest.skip("no MI355X visible")
    engine.init(0)
    return engine


_PER_RAY = dict(SYNTHRAY_F64_TILE="0", SYNTHRAY_TILE=None, SYNTHRAY_TILE_CUTS=None, SYNTHRAY_TILE_RECORDS=None)


def _volume(eng, G, **kw):
    return eng.Volume.from_ne(G.ne, *G.axes, LWL, "xyz"[G.a], phaseshift=False, **kw)


def assert_order(order, key, dead, what, skip=None):
    """(a), (b) and (c) of the module's docstring; skip: rays left out of (b) and (c)"""
    n = len(key)
    assert order.dtype == np.uint32 and order.shape == (n,), what
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)), f"{what}: the order is no permutation of the rays"
    if skip is not None:
        order = order[~skip[order]]
    ks = key[order]
    down = np.flatnonzero(ks[1:] < ks[:-1])
    assert down.size == 0, f"{what}: {down.size} descents of the key, the first at launch slot {down[:1]}: keys {ks[down[:1]]} -> {ks[down[:1] + 1]}"
    n_dead = int((ks == dead).sum())
    assert np.all(ks[len(ks) - n_dead:] == dead) and np.all(ks[:len(ks) - n_dead] < dead), f"{what}: the dead rays are not the tail"


def _trace_order(eng, vol, G, s0, sort, rays=None, sf=True, **env):
    """one trace: (launch order, sf or None, stats, bundle)"""
    with _env(**env):
        if rays is None:
            rays = eng.RayBundle(s0.shape[1])
        rays.upload(s0)
        st = rays.trace(vol, eng.default_t_end(G.ext), G.ext, precision="f64", sort_rays=sort)
        order = rays.launch_order()
        out = np.array(rays.download(rf=False, Jf=False)[0]) if sf else None
    return order, out, st, rays


def check_morton(eng, vol, G, s0, what, rays=None):
    """The Morton path (the per-ray float64 kernel): the order against the restatement, the identity without the sort, and the
    same sf either way"""
    key, dead = entry_keys(G, s0)
    order, sf, _, rays = _trace_order(eng, vol, G, s0, True, rays, **_PER_RAY)
    assert rays.tile_segments == 0, what
    ident, sf0, _, _ = _trace_order(eng, vol, G, s0, False, rays, **_PER_RAY)
    assert np.array_equal(ident, np.arange(s0.shape[1], dtype=np.uint32)), f"{what}: sort_rays=False is not the identity"
    assert_order(order, key, dead, what)
    assert np.array_equal(sf, sf0, equal_nan=True), f"{what}: sf depends on the ray order"
    return rays


@pytest.fixture(scope="module")
def base(eng):
    """the 33 x 26 node lateral grid, three node planes: shared, never changed"""
    G = make_grid(3, 33, 26)
    vol = _volume(eng, G)
    yield G, vol
    vol.close()


@pytest.mark.gpu
def test_launch_order_state(eng, base):
    """SR_ERR_STATE until a trace has been queued, and again after the bundle is resized"""
    from synthpy_amd import _ffi as built

    G, vol = base
    rays = eng.RayBundle(300)
    buf = np.full(300, 7, np.uint32)
    assert built.lib.sr_rays_launch_order(rays._h, built.ptr(buf)) == -4 and "no trace" in built.last_error()
    assert built.lib.sr_rays_launch_order(rays._h, None) == -1
    rays.upload(make_rays(G, 300, 1))
    with pytest.raises(built.SynthrayError, match="no trace"):
        rays.launch_order()
    assert np.all(buf == 7)
    check_morton(eng, vol, G, make_rays(G, 300, 1), "state", rays)
    with pytest.raises(built.SynthrayError, match="made for 300"):
        rays.resize(301)
    rays.resize(200)
    with pytest.raises(built.SynthrayError, match="no trace"):
        rays.launch_order()
    with pytest.raises(built.SynthrayError):
        rays.download()
    rays.close()
    empty = eng.RayBundle(0).upload(np.zeros((9, 0)))
    empty.trace(vol, eng.default_t_end(G.ext), G.ext, precision="f64")
    assert empty.launch_order().shape == (0,)
    empty.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_tile_boundaries_of_the_sort(eng, base, n):
    """ray counts around the 256 threads of a sort workgroup and its tile of kBinTile = 4096 rays"""
    G, vol = base
    check_morton(eng, vol, G, make_rays(G, n, seed=n), f"N = {n}").close()


def _population(G, tag, n=20_003):
    s0 = make_rays(G, n, seed=3, dead=False)
    b, c = G.b, G.c
    i = np.arange(n)
    if tag == "one cell":
        s0[b] = G.gb[7] + CELL * np.linspace(0.0, 0.999, n)
        s0[c] = G.gc[20] + 0.5 * CELL
    elif tag == "one column":
        s0[c] = G.gc[3] + 0.25 * CELL
    elif tag == "all outside":
        s0[c] = np.where(i % 2 == 0, G.gc[0] - CELL, G.gc[-1] + 0.5 * CELL)
    elif tag == "all nan":
        s0[:6] = np.nan
    elif tag == "half dead":
        s0[b, 0::4] = np.nan
        s0[c, 2::4] = G.gc[-1] * 2.0
    elif tag == "two corners":
        s0[b] = np.where(i % 3 == 0, G.gb[0], G.gb[-1])
        s0[c] = np.where(i % 3 == 0, G.gc[0], G.gc[-1])
    else:
        raise KeyError(tag)
    return s0


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["one cell", "one column", "all outside", "all nan", "half dead", "two corners"])
def test_degenerate_populations(eng, base, tag):
    """every ray in one digit of a level, or in none: one run of a coarse group, empty groups, the dead group alone"""
    G, vol = base
    s0 = _population(G, tag)
    key, dead = entry_keys(G, s0)
    n_dead = {"all outside": len(key), "all nan": len(key), "half dead": (len(key) + 1) // 2}.get(tag, 0)
    assert int((key == dead).sum()) == n_dead and len(np.unique(key)) == {"one cell": 1, "two corners": 2}.get(tag, len(np.unique(key)))
    check_morton(eng, vol, G, s0, tag).close()


@pytest.mark.gpu
def test_one_lateral_cell(eng):
    """2 x 2 lateral nodes: bits = 1, three coarse groups, every live ray key 0"""
    G = make_grid(3, 2, 2)
    vol = _volume(eng, G)
    s0 = make_rays(G, 20_003, seed=4)
    key, dead = entry_keys(G, s0)
    assert dead == 4 and set(np.unique(key)) == {0, 4}
    check_morton(eng, vol, G, s0, "one lateral cell").close()
    vol.close()


def _edge_rays(G, rng):
    """Rays exactly on lateral nodes (first, inner, last of each axis, the four corners) with no projection arithmetic -- started
    ON the entry plane, or before it with v_b = v_c = 0 --, oblique rays from before the plane that the projection moves to
    another cell, rays that start inside the volume, rays with v_a <= 0 -- and a few thousand ordinary ones around them."""
    s0 = make_rays(G, 6_007, seed=5, div=0.3)
    a, b, c = G.a, G.b, G.c
    nb, nc = len(G.gb), len(G.gc)
    ib = np.array([0, 1, nb // 2, nb - 2, nb - 1])
    ic = np.array([0, 1, nc // 3, nc - 2, nc - 1])
    on_b, on_c = np.meshgrid(G.gb[ib], G.gc[ic], indexing="ij")  # 25 node pairs, the four corners among them
    k = on_b.size
    for q, (pa, vlat) in enumerate(((G.ga[0], 0.3), (-G.ext, 0.0))):  # on the plane, obliquely; before it, straight
        sl = slice(100 + q * k, 100 + (q + 1) * k)
        s0[b, sl], s0[c, sl], s0[a, sl] = on_b.ravel(), on_c.ravel(), pa
        s0[3 + b, sl] = s0[3 + c, sl] = C_LIGHT * vlat
    sl = slice(200, 200 + k)  # one axis on a node, the other inside a cell
    s0[b, sl], s0[a, sl], s0[3 + b, sl], s0[3 + c, sl] = on_b.ravel(), -G.ext, 0.0, 0.0
    inside = slice(1000, 1400)  # start inside the volume: taken where they are, whatever their direction
    s0[a, inside] = G.ga[0] + (G.ga[-1] - G.ga[0]) * rng.random(400)
    back = slice(1400, 1800)    # v_a <= 0 before the plane: no projection either
    s0[3 + a, back] = np.where(np.arange(400) % 2 == 0, -C_LIGHT, 0.0)
    return s0


@pytest.mark.gpu
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "non-uniform"])
def test_edges_of_the_cell_rule(eng, uniform):
    rng = np.random.default_rng(6)
    G = make_grid(3, 33, 26, rng=None if uniform else rng)._replace(ext=10.0 * CELL)  # nine cells before the entry plane
    assert uniform == bool(np.ptp(np.diff(G.gb)) == 0)
    vol = _volume(eng, G)
    s0 = _edge_rays(G, rng)
    qb, qc = entry_point(s0, G.a, G.ga[0])
    sl = slice(100, 150)  # the 50 node rays of the first two groups: exactly on nodes after the (absent) projection
    assert np.all(np.isin(qb[sl], G.gb)) and np.all(np.isin(qc[sl], G.gc))
    assert cell_of(G.gb, qb[sl]).max() == len(G.gb) - 2 and cell_of(G.gc, qc[sl]).max() == len(G.gc) - 2  # the last node: the last cell
    ordinary = slice(2000, 6007)
    moved = (cell_of(G.gb, qb[ordinary]) != cell_of(G.gb, s0[G.b, ordinary])) & (cell_of(G.gb, qb[ordinary]) >= 0)
    assert moved.mean() > 0.3  # the projection decides the cell of the oblique rays
    check_morton(eng, vol, G, s0, "cell-rule edges").close()
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cells", [(8, 7), (31, 33), (256, 9), (9, 256), (2049, 8), (8, 4099)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_key_widths(eng, cells):
    """bits from 3 to 11, unequal axes, and the coarsened key of axes past 2048 cells (shift 1 and 2), where the order is by the
    coarser cell only -- as the restatement's shift says"""
    G = make_grid(3, cells[0] + 1, cells[1] + 1, pdir="x" if cells[1] > cells[0] else "z")
    shift, bits, dead = morton_plan(*cells)
    assert (shift, bits) == {(8, 7): (0, 3), (31, 33): (0, 6), (256, 9): (0, 8), (9, 256): (0, 8), (2049, 8): (1, 11), (8, 4099): (2, 11)}[cells]
    vol = _volume(eng, G)
    s0 = make_rays(G, 60_001 if shift else 20_003, seed=7, div=0.05)
    check_morton(eng, vol, G, s0, f"{cells} cells").close()
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_wg", [63, 100])
def test_scan_across_two_blocks(eng, base, n_wg):
    """33 coarse groups x 63 sort tiles = 2079 counts: a second k_scan_blocks workgroup, whose counts -- the dead group's runs
    of tiles 32 to 62 -- get the first one's total from k_scan_add; x 100 tiles the boundary falls inside a group of cells"""
    G, vol = base
    n = (n_wg - 1) * K_BIN_TILE + 1
    n_coarse = (1 << morton_plan(32, 25)[1]) + 1
    assert n_coarse == 33 and -(-n // K_BIN_TILE) == n_wg and K_SCAN_BLOCK < n_coarse * n_wg <= 2 * K_SCAN_BLOCK
    check_morton(eng, vol, G, make_rays(G, n, seed=8), f"{n_wg} tiles").close()


@pytest.mark.gpu
def test_scan_of_more_than_1024_block_totals(eng):
    """3 x 1026 x 3 nodes: 1025 cells along b give 2^11 + 1 = 2049 coarse groups; 4 194 305 rays are 1025 sort tiles; 2 100 225
    counts are 1026 block totals, so k_scan (one workgroup, 1024 totals a pass, a carry between passes) runs a second pass, as
    on the headline.  Totals 1024 and 1025 cover the coarse groups from 2046 on: the cells' keys end at 2^21 + 1 (group 1024),
    so what the second pass places is the DEAD group, 2048 -- the NaN and outside rays that make_rays spreads over every tile.
    The one large case of the file: two traces of two steps."""
    G = make_grid(3, 1026, 3)
    n = 1024 * K_BIN_TILE + 1
    n_wg = -(-n // K_BIN_TILE)
    n_coarse = (1 << morton_plan(1025, 2)[1]) + 1
    totals = -(-n_coarse * n_wg // K_SCAN_BLOCK)
    assert (n, n_wg, n_coarse, totals) == (4_194_305, 1025, 2049, 1026) and totals > K_SCAN_CHUNK
    vol = _volume(eng, G)
    s0 = make_rays(G, n, seed=9)
    key, dead = entry_keys(G, s0)
    assert (dead >> 11) * n_wg // K_SCAN_BLOCK >= K_SCAN_CHUNK and int((key == dead).sum()) > 200_000
    check_morton(eng, vol, G, s0, "1026 block totals").close()
    vol.close()


def _tile_env(band, planes, records):
    return dict(SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE=f"8,8,2,{band},{planes}", SYNTHRAY_TILE_RECORDS="1" if records else "0",
                SYNTHRAY_TILE_CUTS=None)


@pytest.fixture(scope="module")
def band_grids(eng):
    out = {}
    for cells in ((8, 8), (9, 8), (33, 26)):
        G = make_grid(3, cells[0] + 1, cells[1] + 1)
        s0 = make_rays(G, 40_003, seed=10, div=0.01)
        out[cells] = (G, _volume(eng, G), s0)
    yield out
    for _, vol, _ in out.values():
        vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("records", [True, False], ids=["records", "producers"])
@pytest.mark.parametrize("band", [1, 2, 3, 8])
@pytest.mark.parametrize("cells", [(8, 8), (9, 8), (33, 26)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_band_order(eng, band_grids, cells, band, records):
    """The tile path's first binning, one segment: bands of 1, 2, 3 and 8 cell rows (9 and 33 rows: a last band of fewer rows),
    columns forth and back.  The per-ray kernel on the same rays: the Morton order, and sf whatever the order."""
    G, vol, s0 = band_grids[cells]
    key, dead = entry_keys(G, s0, band=band)
    order, sf, st, rays = _trace_order(eng, vol, G, s0, True, **_tile_env(band, len(G.ga) - 1, records))
    assert rays.tile_segments == 1 and rays.tile_records == records, (rays.tile_segments, rays.tile_records)
    assert_order(order, key, dead, f"band {band}, {cells} cells")
    if band == 2 and records:  # once per grid
        rays = check_morton(eng, vol, G, s0, f"{cells} cells, per-ray kernel", rays)
        assert np.array_equal(sf, np.array(rays.download(rf=False, Jf=False)[0]), equal_nan=True), "tile path: sf differs from the per-ray kernel's"
    rays.close()


def _sorted_prefix(ks):
    down = np.flatnonzero(ks[1:] < ks[:-1])
    return len(ks) if down.size == 0 else int(down[0]) + 1


@pytest.mark.gpu
@pytest.mark.parametrize("records", [True, False], ids=["records", "producers"])
def test_rebinning_between_segments(eng, records):
    """Three segments in vacuum: after the trace the order is that of the LAST re-binning, by the band key of the cell a ray is
    in on node plane 9 -- p + v * tau in NumPy.  Rays the tiles lost before that plane carry the dead key on the device and sit
    at the tail among the dead: the sorted prefix is at least N - fallback_rays - (the restatement's dead) long."""
    G, s0, cut, qb, qc = _rebin_case()
    vol = _volume(eng, G)
    skip = near_a_node(G.gb, G.gc, qb, qc)
    assert skip.mean() <= 1e-3
    key, dead = keys_at(G.gb, G.gc, qb, qc, alive=s0[3 + G.a] > 0, band=2)
    order, sf, st, rays = _trace_order(eng, vol, G, s0, True, **_tile_env(2, 4, records))
    assert rays.tile_segments == 3 and rays.tile_records == records, (rays.tile_segments, rays.tile_records)
    n = len(key)
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)), "the order is no permutation of the rays"
    ks = key[order[~skip[order]]]
    n_dead = int((key == dead).sum())
    need = n - int(skip.sum()) - st.fallback_rays - n_dead
    print(f"re-binning: {st.fallback_rays} rays lost by the tiles, {n_dead} dead, sorted prefix {_sorted_prefix(ks)} of {len(ks)}, needed {need}")
    assert st.fallback_rays < n // 2 and need > n // 3, (st.fallback_rays, need)
    assert _sorted_prefix(ks) >= need, (_sorted_prefix(ks), need)
    ident, sf0, _, _ = _trace_order(eng, vol, G, s0, False, rays, **_PER_RAY)
    assert rays.tile_segments == 0 and np.array_equal(ident, np.arange(n, dtype=np.uint32))
    assert np.array_equal(sf, sf0, equal_nan=True), "sf of the segmented tile path differs from the unsorted per-ray kernel's"
    rays.close()
    vol.close()


def _slab_chain(eng, G, s0, env2, env1=None):
    """two slabs (node planes 0..2 and 2..4) chained by the hand-off records in one bundle: (first order, second order, bundle info)"""
    vols, orders, info = [], [], []
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    for q, (lo, hi) in enumerate(((0, 2), (2, 4))):
        vol = eng.Volume.from_ne_slab(eng.slab_source(G.ne, G.a, lo, hi), *G.axes, LWL, "xyz"[G.a], lo, hi, phaseshift=False)
        vols.append(vol)
        with _env(**((env1 or env2) if q == 0 else env2)):
            rays.trace(vol, eng.default_t_end(G.ext), G.ext, precision="f64", handoff=eng.HANDOFF_EXIT if q == 0 else eng.HANDOFF_ENTER)
            orders.append(rays.launch_order())
            info.append((rays.tile_segments, rays.tile_records))
    sf = np.array(rays.download(rf=False, Jf=False)[0])
    rays.close()
    for vol in vols:
        vol.close()
    return orders, info, sf


@pytest.mark.gpu
def test_handoff_keeps_the_senders_order_on_the_per_ray_kernel(eng):
    """k_perm_from_rec: the second slab launches the rays in the order they arrive in, the first slab's Morton order"""
    G, s0, _ = _handoff_cases()[0]
    (first, second), info, _ = _slab_chain(eng, G, s0, _PER_RAY)
    assert info == [(0, False), (0, False)]
    key, dead = entry_keys(G, s0)
    assert_order(first, key, dead, "first slab")
    assert np.array_equal(second, first)


@pytest.mark.gpu
@pytest.mark.parametrize("first_tiled", [False, True], ids=["from the per-ray kernel", "from the tile path"])
def test_handoff_bins_the_arrivals_on_the_tile_path(eng, first_tiled):
    """the second slab's tile path bins the arrivals by the band key of the cell they arrive in (k_keys_band_rec on the records
    as they came), whatever order the sender had"""
    G, s0, (qb, qc) = _handoff_cases()[0]
    tile = _tile_env(2, 2, True)
    (first, second), info, sf = _slab_chain(eng, G, s0, tile, tile if first_tiled else _PER_RAY)
    assert info == [(1 if first_tiled else 0, first_tiled), (1, True)], info
    key1, dead1 = entry_keys(G, s0, band=2 if first_tiled else None)
    assert_order(first, key1, dead1, "first slab")
    skip = near_a_node(G.gb, G.gc, qb, qc)
    assert skip.mean() <= 1e-3
    key, dead = keys_at(G.gb, G.gc, qb, qc, alive=s0[3 + G.a] > 0, band=2)
    assert_order(second, key, dead, "second slab", skip)
    assert not np.array_equal(second, first)
    _, _, sf0 = _slab_chain(eng, G, s0, _PER_RAY)
    assert np.array_equal(sf, sf0, equal_nan=True), "the slab chain's sf depends on the kernels and orders"


@pytest.mark.gpu
def test_one_bundle_traced_with_changing_counts(eng, base):
    """One bundle made for 8193 rays, traced with 8193, 257, 4097 and 1: bins_cap and sort_tmp are sized once, by the first
    trace and the capacity; every order is right whatever the trace before it left in them."""
    G, vol = base
    rays = eng.RayBundle(8193)
    for n in (8193, 257, 4097, 1):
        rays.resize(n)
        assert rays.n == n
        check_morton(eng, vol, G, make_rays(G, n, seed=100 + n, div=0.05), f"capacity 8193, N = {n}", rays)
    rays.close()
