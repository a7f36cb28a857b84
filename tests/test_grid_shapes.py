"""Every trace kernel on grids that are not cubes: node counts that differ on every axis, probing axes whose length sits on an
octet edge of the packed node planes, lateral grids exactly one tile wide or one cell short of it, skewed and very wide
lateral grids.  On a cube a swap of the probing axis a and the lateral axes b = (a+1)%3, c = (a+2)%3 gives the same numbers;
here it does not.  Needs an MI355X: run with -m gpu.

For every case of SHAPES and every probing axis it lists: the gradient volumes against the oracle bit for bit, the gathers at
nodes / faces / interiors / out of bounds / NaN, each float64 kernel forced by name (k_trace_f64, the tile path's records
and producers' kernels) and the mixed build against the oracle, the kernels against each other and the two ray orders bit
for bit, and the counts images.  Where the library declines the tile path (fewer than three node planes, a lateral grid
under the tile) the test asserts that it declined.  SLAB_CASES chain slabs of unequal thickness through the same grids."""
from collections import namedtuple

import numpy as np
import pytest

from conftest import golden
from test_gpu_parity import _forced_kernel

pytestmark = pytest.mark.gpu

LWL = 1064e-9
Case = namedtuple("Case", "tag abc pdir cell n_dense why")


def _octets(pd):
    return [Case(f"na{na}_{pd}", (na, 33, 26), pd, 2.5e-4, 40_003, f"na = {na}: " + why) for na, why in (
        (2, "one cell along the probing axis, where the tile path must decline"),
        (3, "the tile path's smallest volume, one octet of node planes partly filled"),
        (8, "exactly one octet of node planes"),
        (9, "one node plane past an octet"),
        (17, "one node plane past two octets"))]


# (na, nb, nc): node counts along the probing axis a and the lateral axes b = (a+1)%3, c = (a+2)%3; cell: the mean cell width
# (each axis a little different, see _grid); n_dense: rays of the dense beam
SHAPES = [
    # the distinct-count grid of g14 (41 x 29 x 23 as x, y, z), so probing along x, y and z gives (na, nb, nc) = (41, 29, 23),
    # (29, 23, 41), (23, 41, 29)
    Case("distinct_x", (41, 29, 23), "x", 2.5e-4, 60_001, "every count differs: a/b/c permutation, records index, tile tb / tc"),
    Case("distinct_y", (29, 23, 41), "y", 2.5e-4, 60_001, "as distinct_x, and the y-probing row order"),
    Case("distinct_z", (23, 41, 29), "z", 2.5e-4, 60_001, "as distinct_x, probing along z"),
    *_octets("z"), *_octets("x"), *_octets("y"),
    Case("tile_rec_exact", (12, 9, 8), "z", 2.5e-4, 40_003, "8 x 7 lateral cells: the records kernel's tile exactly; producers decline"),
    Case("tile_prod_exact", (12, 9, 9), "x", 2.5e-4, 40_003, "8 x 8 lateral cells: the producers' tile exactly"),
    Case("tile_short", (12, 8, 8), "y", 2.5e-4, 40_003, "7 x 7 lateral cells: one short of every tile, the planner declines"),
    Case("one_lateral_cell", (12, 2, 2), "z", 2.5e-4, 40_003, "a single lateral cell"),
    Case("skew_b", (12, 257, 10), "z", 2.5e-4, 40_003, "256 x 9 cells: Morton and band keys on unequal axes, density estimate"),
    Case("skew_c", (12, 10, 257), "x", 2.5e-4, 40_003, "9 x 256 cells: the same with the long axis second"),
    Case("wide_b", (9, 2050, 9), "z", 5e-5, 200_003, "2049 cells along b: past the 2048 x 2048 LDS counters of the ray binning"),
    Case("wide_c", (9, 9, 4100), "x", 5e-5, 300_001, "4099 cells along c: past the counters and the 4096-cell Morton digits"),
    Case("wide_both", (9, 4097, 1100), "z", 5e-5, 300_001, "4.5e6 lateral cells (> 2^22): the band key of the forced tile path"),
]
SLAB_CASES = ["distinct_x", "distinct_y", "distinct_z"]


def _grid(case):
    """Physical coordinates (x, y, z), ne and the probing axis of a case: the (na, nb, nc) counts placed on axes a, b, c; every
    axis gets its own cell width (0.9, 1.0, 1.1 times `cell` in x, y, z) and an off-centre blob sized to that axis."""
    a = "xyz".index(case.pdir)
    n = [0, 0, 0]
    for q in range(3):
        n[(a + q) % 3] = case.abc[q]
    half = [0.5 * (n[k] - 1) * case.cell * (0.9, 1.0, 1.1)[k] for k in range(3)]
    if case.tag.startswith("distinct"):  # g14's grid: +-5, +-4, +-3 mm
        half = [5e-3, 4e-3, 3e-3]
    x, y, z = (np.linspace(-h, h, m) for h, m in zip(half, n))
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij", sparse=True)
    w = [max(0.45 * h, 1e-4) for h in half]
    r2 = ((X - 0.06 * half[0]) / w[0]) ** 2 + ((Y + 0.04 * half[1]) / w[1]) ** 2 + (Z / w[2]) ** 2
    ne = 1e25 * np.exp(-r2) * (1.0 + 0.1 * np.sin(2.6 * X / w[0] + 1.7 * Y / w[1]) * np.cos(2.1 * Z / w[2]))
    return (x, y, z), half, ne, a


def _beams(axes, half, a, n_dense):
    """dense: a near-collimated square beam over 80 % of the lateral faces (dense enough for the tile path wherever the count
    of lateral cells allows) with 5 NaN rays; overfill: a divergent beam 1.3 times the lateral faces,
    rays that start outside them, leave and come in through them, 3 NaN rays.  Neither count is a multiple of 256."""
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    ext = half[a] * 1.01  # the rays start before the first node plane
    b, c = (a + 1) % 3, (a + 2) % 3
    out = {}
    for tag, n, fill, div, seed in (("dense", n_dense, 0.8, 5e-5, 7), ("overfill", 5_003, 1.3, 2e-3, 8)):
        np.random.seed(seed)
        s0 = init_beam(n, 1.0, div, ext, "square", "xyz"[a])
        s0[b] *= fill * half[b]
        s0[c] *= fill * half[c]
        s0[:, 1:4 if tag == "overfill" else 6] = np.nan
        out[tag] = np.ascontiguousarray(s0)
    return out, ext


def _admits(tile, na, nb, nc):
    """Whether the tile path can take this grid (tile_plan): three node planes at least and a lateral grid of at least one tile
    -- 8 x 7 cells for the records kernel (tile 1), 8 x 8 for the producers' kernel (tile 2)."""
    if not tile:
        return False
    return na >= 3 and nb - 1 >= 8 and nc - 1 >= (7 if tile == 1 else 8)


def _trace(eng, vol, s0, t_end, ext, tile, expect_tile, **kw):
    """RayBundle.trace with the kernel forced by _forced_kernel; asserts that the library ran it, or declined the tile path
    where the grid does not admit it.  (sf, rf, Jf, stats, bundle)."""
    with _forced_kernel(tile) as fk:
        rays = eng.RayBundle(s0.shape[1]).upload(s0)
        st = rays.trace(vol, t_end, ext, **kw)
        if tile and not expect_tile:
            assert rays.tile_segments == 0, f"tile {tile}: tile_segments = {rays.tile_segments} on a grid the tile path cannot take"
        else:
            fk.check(rays)
        return (*rays.download(), st, rays)


def _same(u, w):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(u, w))


def _close(got, ref, tol, what):
    """NaN where the reference has NaN, and max |got - ref| <= tol over the rest."""
    bad = np.isnan(ref)
    assert np.array_equal(np.isnan(got), bad), f"{what}: NaN pattern differs"
    err = float(np.max(np.abs(got[~bad] - ref[~bad]))) if (~bad).any() else 0.0
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def _vs_oracle(sf, rf, Jf, st, so, ro, Jo, steps_o, f64, what):
    assert st.ray_steps == steps_o, (what, st.ray_steps, steps_o)
    tx, ta = (1e-13, 1e-11) if f64 else (5e-11, 2e-8)
    _close(rf[0::2], ro[0::2], tx, what + " exit position")
    _close(rf[1::2], ro[1::2], ta, what + " exit angle")
    # phase: test_trace_vs_oracle's 1e-10 of the largest phase in float64.  The mixed build forms each step's phase increment
    # as a float32 RK4 sum of float32 slopes (trace_mx.inc); on a volume of a few node planes nothing averages those roundings
    # out, and they reach 11 * 2^-24 (6.8e-7) of a ray's phase on 2 to 12 planes -- beyond test_trace_mixed_vs_oracle's 1e-7 of
    # the largest phase, which held on 16 to 32 planes.  1e-6 of the largest phase here: an axis or stride mix-up is of order 1.
    _close(sf[7], so[7], (1e-10 if f64 else 1e-6) * max(1.0, float(np.nanmax(np.abs(so[7])))), what + " phase")
    if f64:  # test_trace_vs_oracle's terms for the state at t_end and the Jones vector
        _close(sf[:3], so[:3], 1e-12, what + " position at t_end")
        _close(sf[3:6], so[3:6], 1e-3, what + " velocity at t_end")
        assert np.array_equal(sf[6], so[6], equal_nan=True) and np.array_equal(sf[8], so[8], equal_nan=True), what
        _close(Jf, Jo, 1e-9, what + " Jones vector")


def _gather_points(axes, rng):
    """nodes, points on cell faces, cell interiors, points out of bounds on each side of each axis, NaN points"""
    g32 = [np.float64(np.float32(v)) for v in axes]
    lo, hi = [v[0] for v in g32], [v[-1] for v in g32]
    m = 400
    nodes = np.stack([v[rng.integers(0, len(v), m)] for v in g32], 1)
    faces = np.stack([rng.uniform(lo[k], hi[k], m) for k in range(3)], 1)
    for k in range(3):
        faces[k::3, k] = g32[k][rng.integers(0, len(g32[k]), len(faces[k::3]))]
    faces[:6] = [[lo[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], lo[2]], [hi[0], lo[1], hi[2]],
                 [hi[0], hi[1], lo[2]], [lo[0], lo[1], hi[2]]]  # corners
    inner = np.stack([rng.uniform(lo[k], hi[k], m) for k in range(3)], 1)
    outside = np.stack([rng.uniform(lo[k], hi[k], 12) for k in range(3)], 1)
    for q in range(6):
        k, side = q // 2, q % 2
        outside[2 * q:2 * q + 2, k] = (hi[k] + 1e-6, hi[k] * 1.5) if side else (lo[k] - 1e-6, lo[k] * 1.5)
    nan = np.array([[np.nan, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, np.nan]])
    return np.concatenate([nodes, faces, inner, outside, nan])


def _counts(eng, orc, rays, rf, bin_scale):
    img = eng.DetectorImage.counts(bin_scale=bin_scale)
    rays.deposit(img, eng.chain_shadow_two())
    r_o, _ = orc.optics(orc.m_to_mm(rf), orc.chain_shadow_two())
    return img.download(), orc.histogram(r_o, bin_scale=bin_scale)


@pytest.fixture(scope="module")
def eng():
    from synthpy_amd import engine

    engine.init(0)
    return engine


@pytest.mark.parametrize("case", SHAPES, ids=[c.tag for c in SHAPES])
def test_grid_shape(eng, orc, case):
    axes, half, ne, a = _grid(case)
    pd = "xyz"[a]
    na, nb, nc = case.abc
    assert (len(axes[a]), len(axes[(a + 1) % 3]), len(axes[(a + 2) % 3])) == case.abc
    vol = eng.Volume.from_ne(ne, *axes, LWL, pd, phaseshift=True)

    # 1. gradients bit for bit, n - 1 within 2e-15 of its largest value
    om, gx, gy, gz = orc.calc_dndr(ne, *axes, LWL)
    fx, fy, fz, nm1 = vol.fields(phase=True)
    assert np.array_equal(fx, gx) and np.array_equal(fy, gy) and np.array_equal(fz, gz)
    nref1 = orc.n_refrac(ne, om) - 1.0
    assert np.max(np.abs(nm1 - nref1)) <= 2e-15 * np.max(np.abs(nref1))

    # 2. gathers against scipy's rule (the oracle), out of bounds exactly the fill value
    pts = _gather_points(axes, np.random.default_rng(3))
    F = vol.sample(pts)
    g32 = [np.float32(v) for v in axes]
    for k, fld in enumerate((gx, gy, gz)):
        ref = orc.interp(*g32, fld, pts, 0.0)
        _close(F[k], ref, 1e-15 * np.nanmax(np.abs(ref)), f"gather d n/d{'xyz'[k]}")
    ref = orc.interp(*g32, nref1, pts, 0.0)
    _close(F[3], ref, 1e-12 * np.nanmax(np.abs(ref)), "gather n - 1")
    out = np.zeros(len(pts), bool)
    for k in range(3):
        out |= (pts[:, k] < g32[k][0]) | (pts[:, k] > g32[k][-1])
    assert out.sum() == 12 and np.all(F[:, out] == 0)
    del fx, fy, fz, nm1, F

    # 3.-5. traces
    beams, ext = _beams(axes, half, a, case.n_dense)
    t_end = eng.default_t_end(ext)
    dt = float(g32[a][1] - g32[a][0]) / orc.c
    dom = orc.Domain.from_ne(ne, *axes, LWL, phaseshift=True)
    vol_np = eng.Volume.from_ne(ne, *axes, LWL, pd)  # no phase integral: what the default counts path traces in the mixed build
    assert eng.resolve_precision("auto", vol_np) == "mixed"
    for tag, s0 in beams.items():
        so, steps_o = orc.trace_rk4(dom, s0, dt, t_end, pd, "planes", 1)
        ro, Jo = orc.ray_to_jones(so, ext, pd)
        res = {}
        for tile in (0, 1, 2):
            *r, st, rays = _trace(eng, vol, s0, t_end, ext, tile, _admits(tile, na, nb, nc), precision="f64", dt=dt)
            _vs_oracle(*r, st, so, ro, Jo, steps_o, True, f"{tag}, tile {tile}")
            res[tile] = (r, st.ray_steps)
            if tile == 0:
                rays0 = rays
        for tile in (1, 2):  # 4. the tile kernels are the per-ray kernel, bit for bit
            assert _same(res[tile][0], res[0][0]) and res[tile][1] == res[0][1], (tag, tile)
        *r, st, _ = _trace(eng, vol, s0, t_end, ext, 0, False, precision="f64", dt=dt, sort_rays=False)
        assert _same(r, res[0][0]) and st.ray_steps == res[0][1], (tag, "f64 unsorted")
        *r, st, _ = _trace(eng, vol, s0, t_end, ext, None, False, precision="f64", dt=dt)  # the library's own choice
        assert _same(r, res[0][0]) and st.ray_steps == res[0][1], (tag, "f64, the library's choice")
        *rm, st, _ = _trace(eng, vol, s0, t_end, ext, None, False, precision="mixed", dt=dt)
        _vs_oracle(*rm, st, so, ro, Jo, steps_o, False, f"{tag}, mixed")
        *r, st_u, _ = _trace(eng, vol, s0, t_end, ext, None, False, precision="mixed", dt=dt, sort_rays=False)
        assert _same(r, rm) and st_u.ray_steps == st.ray_steps, (tag, "mixed unsorted")

        # 5. counts: the float64 trace's image is the oracle's histogram of the same rays; the default path's image is the float64 one
        rf0 = res[0][0][1]
        for bs in (1, 10):
            H, H_o = _counts(eng, orc, rays0, rf0, bs)
            assert np.array_equal(H, H_o.astype(np.uint32)), (tag, bs)
        rays_d = eng.RayBundle(s0.shape[1]).upload(s0)
        rays_d.trace(vol_np, t_end, ext, dt=dt)
        rays_f = eng.RayBundle(s0.shape[1]).upload(s0)
        rays_f.trace(vol_np, t_end, ext, dt=dt, precision="f64")
        rf_f = rays_f.download()[1]
        for bs in (1, 10):
            Hd, _ = _counts(eng, orc, rays_d, rf_f, bs)
            Hf, Hf_o = _counts(eng, orc, rays_f, rf_f, bs)
            assert np.array_equal(Hf, Hf_o.astype(np.uint32)) and np.array_equal(Hd, Hf), (tag, "default path", bs)
        for rr in (rays0, rays_d, rays_f):
            rr.close()
    vol.close()
    vol_np.close()


def _slab_chain(eng, ne, axes, a, cuts, s0, t_end, ext, dt, precision, tile=None):
    """The rays through the slabs of `cuts` in turn, handed over on the shared node planes through the host (odd slabs) or in
    place; (sf, rf, Jf), total steps, each slab's tile_segments."""
    pd = "xyz"[a]
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    steps, tiles = 0, []
    with _forced_kernel(tile):
        for q, (lo, hi) in enumerate(cuts):
            vol = eng.Volume.from_ne_slab(eng.slab_source(ne, a, lo, hi), *axes, LWL, pd, lo, hi, phaseshift=True)
            flags = (eng.HANDOFF_ENTER if q > 0 else 0) | (eng.HANDOFF_EXIT if q + 1 < len(cuts) else 0)
            st = rays.trace(vol, t_end, ext, precision=precision, handoff=flags, dt=dt)
            steps += st.ray_steps
            tiles.append(rays.tile_segments)
            if q % 2 == 0 and q + 1 < len(cuts):
                rec = rays.handoff_download()
                rays = eng.RayBundle(s0.shape[1]).handoff_upload(rec)
    return rays.download(), steps, tiles


@pytest.mark.parametrize("tag", SLAB_CASES)
def test_slab_chain_non_cubic(eng, orc, tag):
    """6. The (41, 29, 23) grid cut into three slabs of unequal thickness along the probing axis, one of them two node planes
    thick: each slab's gradients are the whole volume's planes; the chain is the whole-volume trace bit for bit -- float64
    through the per-ray kernel and through the tile kernel (the two-plane slab falls to the per-ray kernel), and mixed."""
    case = next(c for c in SHAPES if c.tag == tag)
    axes, half, ne, a = _grid(case)
    pd, na = "xyz"[a], case.abc[0]
    m = 1 + 2 * (na - 2) // 3
    cuts = [(0, m), (m, m + 1), (m + 1, na - 1)]  # about 2/3, two planes, 1/3
    whole = eng.Volume.from_ne(ne, *axes, LWL, pd, phaseshift=True)
    wf = whole.fields(phase=True)
    for lo, hi in cuts:
        part = eng.Volume.from_ne_slab(eng.slab_source(ne, a, lo, hi), *axes, LWL, pd, lo, hi, phaseshift=True)
        sl = [slice(None)] * 3
        sl[a] = slice(lo, hi + 1)
        for u, w in zip(part.fields(phase=True), wf):
            assert np.array_equal(u, w[tuple(sl)]), (lo, hi)
        part.close()
    beams, ext = _beams(axes, half, a, case.n_dense)
    s0 = np.ascontiguousarray(beams["dense"][:, 6:])  # no NaN rays: the whole volume would count their time-stepping steps
    t_end = eng.default_t_end(ext)
    dt = float(np.float32(axes[a])[1] - np.float32(axes[a])[0]) / orc.c
    for precision in ("f64", "mixed"):
        with _forced_kernel(0 if precision == "f64" else None):
            sf, rf, Jf, st = eng.trace(whole, s0, t_end, ext, precision=precision, dt=dt)
        for tile in ((0, 1) if precision == "f64" else (None,)):
            out, steps, tiles = _slab_chain(eng, ne, axes, a, cuts, s0, t_end, ext, dt, precision, tile)
            assert _same(out, (sf, rf, Jf)) and steps == st.ray_steps, (precision, tile, steps, st.ray_steps)
            if tile is not None:
                assert [t > 0 for t in tiles] == [bool(tile) and hi - lo >= 2 for lo, hi in cuts], (tile, tiles)
    whole.close()


@pytest.mark.parametrize("pdir", ["x", "y", "z"])
@pytest.mark.parametrize("precision,tile", [("f64", 0), ("f64", 1), ("f64", 2), ("mixed", None)])
def test_g14_vs_reference_tight(eng, pdir, precision, tile):
    """g14 (the reference's own solve on 41 x 29 x 23 nodes over +-5, +-4, +-3 mm): the device gradients are the reference's
    bit for bit, and every plane kernel by name is within test_trace_vs_reference_tight's terms of the reference RHS
    integrated at rtol 1e-10."""
    g = golden("g14_shapes")
    ext = float(g[f"extent_{pdir}"])
    vol = eng.Volume.from_ne(g["ne"], g["x"], g["y"], g["z"], float(g["lwl"]), pdir, phaseshift=True)
    gx, gy, gz = vol.fields()
    assert np.array_equal(gx, g["dndx"]) and np.array_equal(gy, g["dndy"]) and np.array_equal(gz, g["dndz"])
    s0 = np.ascontiguousarray(g[f"s0_{pdir}"])
    with _forced_kernel(tile) as fk:
        rays = eng.RayBundle(s0.shape[1]).upload(s0)
        rays.trace(vol, eng.default_t_end(ext), ext, precision=precision)
        fk.check(rays)
        sf, rf, Jf = rays.download()
    rt, st = g[f"rf_tight_{pdir}"], g[f"sf_tight_{pdir}"]
    assert np.max(np.abs(rf[0::2] - rt[0::2])) <= 1e-8
    assert np.max(np.abs(rf[1::2] - rt[1::2])) <= 1e-6
    assert np.max(np.abs(sf[:3] - st[:3])) <= 2e-8
    phmax = max(1.0, np.max(np.abs(st[7])))
    assert np.max(np.abs(sf[7] - st[7])) <= 1e-5 * phmax
    assert np.max(np.abs(Jf - g[f"Jf_tight_{pdir}"])) <= 1e-5 * phmax
    vol.close()
