"""The deposit kernels (csrc/deposit.hip) on ray layouts that real traces never produce.

k_deposit and k_deposit_intensity privatise a TW x TH patch of the detector in LDS whose origin is the workgroup's minimum
(bx, by); hits outside the patch go straight to HBM and the patch is flushed under a guard against the detector's right and
bottom edge.  Rays from an imaging chain leave the out-of-tile branch, the overhanging flush, the empty workgroup and the
exact-edge compares of walk / bin_hist / bin_digitize all but unused, so the layouts here are built to use them:

1. SCATTER   4*256 + 37 rays uniform over +-9.5 mm x +-7.5 mm: every workgroup's hits cover the whole detector (most are out
             of tile), some rays miss it, some are killed by the mask [(OP_CIRC_AP, 8.0)].
2. EDGES     positions k * 2^-20 m, zero angle, on the detector [-8192u, 8192u] x [-4096u, 4096u], u = 1000 * 2^-20 mm: rays
             on every edge of both axes (lo and hi included), one lattice unit either side of each, and on bin corners.  All
             of it is exact in float64 (test_dyadic_lattice_is_exact).  Further rays sit, bit for bit, on inner edges of the
             63 x 31, 65 x 33 and 344 x 257 detectors of the same range, which are no lattice points: there (v - lo) / step can
             round below the edge's index, and walk()'s second loop has to move the ray on (rounded_edges).
3. ANCHORED  consecutive workgroups of one bundle: (a) one ray in bin (0, 0) + 255 at the far corner, (b) a cluster whose
             minimum bin is (nx-3, ny-2), (c) 256 misses (half off the detector, half NaN from the mask), (d) one hit among 255
             misses, (e) a full workgroup inside one tile, (f) a last workgroup of one ray.
4. ONE BIN   66 000 rays with distinct positions and fields in a single bin: 256-way LDS contention, a count above 65535.

The rays are launched through an empty 16^3 volume with sort_rays=False (launch slot j is ray j: rays 256 b .. 256 b + 255
share workgroup b) in float64; every GPU test asserts on the GPU's own coordinates what its layout claims before it compares
an image, and the CPU tests assert the same claims on the straight-line prediction.

THE BOUNDS are derived, none is measured.  Counts: np.histogram2d of the post-chain coordinates (RayBundle.optics: the
deposit's own front end), np.array_equal.  Complex sums: binned with np.digitize(v, np.linspace(lo, hi, n_edges)) - 1 (right
edge open, rtm_solver.py:436-448), summed in np.longdouble; per pixel and component |d| <= (n + 16) 2^-53 sum|e_i| -- n - 1
roundings for a float64 sum in ANY order (LDS tile, then HBM), the 16 for the second-order terms.  Intensities: test_polarimetry's
_numpy_images and _assert_within_bound, unchanged.  An empty pixel must be exactly 0.0.
"""
import numpy as np
import pytest

from test_polarimetry import EPS, _assert_within_bound, _numpy_images

EXT = 10e-3                # half-length of the empty volume [m]
C0 = 299792458.0           # engine.c
OP_DIST, OP_CIRC_AP = 0, 2  # engine.OP_DIST, engine.OP_CIRC_AP (asserted in the eng fixture)
WG = 256                   # rays per workgroup of k_deposit / k_deposit_intensity
TILE_COUNTS, TILE_COMPLEX = (64, 32), (32, 16)  # kTileW x kTileH, kCTileW x kCTileH = kITileW x kITileH

DET = (-9.0, 9.0, -6.75, 6.75)   # layouts 1 and 4: the default detector's range [mm]
DET3 = (-6.0, 6.0, -4.5, 4.5)    # layout 3: inside the mask's radius (corner at 7.5 mm < 8 mm)
U = 1000.0 * 2.0 ** -20          # layout 2: the lattice unit [mm]
DET2 = (-8192 * U, 8192 * U, -4096 * U, 4096 * U)
MASK = [(OP_CIRC_AP, 8.0)]
BINS = [(1, 1), (8, 4), (63, 31), (64, 32), (65, 33), (344, 257)]
BINS2 = BINS + [(32, 16), (33, 17)]  # complex and intensity tiles are 32 x 16
ANALYSERS = {1: (None,), 2: (0.7, None), 3: (np.pi / 4, -np.pi / 4, None), 4: (0.3, -0.3, 1.0, None)}
KWAVE = 2 * np.pi / 532e-9


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
    assert (engine.c, engine.OP_DIST, engine.OP_CIRC_AP) == (C0, OP_DIST, OP_CIRC_AP)
    return engine


# ---------------------------------------------------------------- the layouts (numpy only)
def _launch_state(x_m, y_m, th, ph, rng):
    """s0 (9, N) on the volume's entry plane: position [m], angles [rad], and a field of its own for every ray."""
    N = x_m.size
    s0 = np.zeros((9, N))
    t, p = np.tan(th), np.tan(ph)
    norm = np.sqrt(1 + t ** 2 + p ** 2)
    s0[0], s0[1], s0[2] = x_m, y_m, -EXT
    s0[3], s0[4], s0[5] = C0 * t / norm, C0 * p / norm, C0 / norm
    s0[6], s0[7], s0[8] = rng.uniform(0.2, 1.5, N), rng.uniform(0, 6, N), rng.uniform(-1.5, 1.5, N)
    return s0


def layout_scatter():
    rng = np.random.default_rng(101)
    N = 4 * WG + 37
    return _launch_state(rng.uniform(-9.5e-3, 9.5e-3, N), rng.uniform(-7.5e-3, 7.5e-3, N), rng.normal(0, 1e-3, N),
                         rng.normal(0, 1e-3, N), rng)


def rounded_edges(lo, hi, ns):
    """(metres, n, short): coordinates m whose mm value m * 1e3 is, bit for bit, an inner edge of the n-bin detector on
    [lo, hi] that is NO lattice point.  Where (v - lo) / step rounds below the edge's index (`short`), walk()'s first guess is
    one bin low and its second loop has to move the ray on; all of those are taken, and a dozen of the others per n."""
    ms, nn, short = [], [], []
    for n in ns:
        e, i = np.linspace(lo, hi, n + 1), np.arange(n + 1)
        m, found = np.full(n + 1, np.nan), np.zeros(n + 1, bool)
        for c in (e / 1e3, np.nextafter(e / 1e3, np.inf), np.nextafter(e / 1e3, -np.inf)):
            ok = (c * 1e3 == e) & ~found & (i > 0) & (i < n) & (e / U != np.round(e / U))
            m[ok], found = c[ok], found | ok
        low = found & (((e - lo) / ((hi - lo) / n)).astype(int) < i)
        take = low | (found & (np.cumsum(found & ~low) <= 12))
        ms.append(m[take]), nn.append(np.full(take.sum(), n)), short.append(low[take])
    return np.concatenate(ms), np.concatenate(nn), np.concatenate(short)


ROUNDED_BINS = ((63, 65, 344), (31, 33, 257))  # the detectors of BINS2 on DET2 whose inner edges are no lattice points


def edges_rays():
    """Layout 2, shuffled: x_m, y_m [m]; kx, ky: the lattice coordinates of the lattice rays (`lattice`); nx_edge, ny_edge: for
    the other rays the bin count of the detector whose rounded edge the coordinate sits on (0: none); short_x, short_y."""
    rng = np.random.default_rng(202)
    xe, ye = -8192 + 256 * np.arange(65), -4096 + 256 * np.arange(33)

    def mid(n, half):  # inside the detector, never on an edge of the 64 x 32 detector
        return 256 * rng.integers(-half, half, n) + rng.integers(1, 256, n)

    ax = np.concatenate([xe - 1, xe, xe + 1])                # every x edge and one unit either side
    by = np.concatenate([ye - 1, ye, ye + 1])                # every y edge and one unit either side
    i = np.arange(65)
    cx = np.concatenate([xe, xe])                            # bin corners: both coordinates on an edge
    cy = np.concatenate([ye[i % 33], ye[32 - i % 33]])
    dx, dy = np.meshgrid([-1, 0, 1], [-1, 0, 1])
    qx = np.concatenate([c + dx.ravel() for c in (xe[0], xe[0], xe[-1], xe[-1])])  # the detector's corners and around them
    qy = np.concatenate([c + dy.ravel() for c in (ye[0], ye[-1], ye[0], ye[-1])])
    rx, rnx, rsx = rounded_edges(DET2[0], DET2[1], ROUNDED_BINS[0])
    ry, rny, rsy = rounded_edges(DET2[2], DET2[3], ROUNDED_BINS[1])
    n_fill = 4 * WG + 5 - (ax.size + by.size + cx.size + qx.size + rx.size + ry.size)
    assert n_fill >= 100
    kx = np.concatenate([ax, mid(by.size, 32), cx, qx, rng.integers(-8400, 8401, n_fill), np.zeros(rx.size, int), mid(ry.size, 32)])
    ky = np.concatenate([mid(ax.size, 16), by, cy, qy, rng.integers(-4300, 4301, n_fill), mid(rx.size, 16), np.zeros(ry.size, int)])
    n_lat = kx.size - rx.size - ry.size
    x_m, y_m = kx * 2.0 ** -20, ky * 2.0 ** -20
    x_m[n_lat:n_lat + rx.size], y_m[n_lat + rx.size:] = rx, ry
    z, fx, fy = np.zeros(n_lat, int), np.zeros(rx.size, int), np.zeros(ry.size, int)
    out = dict(x_m=x_m, y_m=y_m, kx=kx, ky=ky, nx_edge=np.concatenate([z, rnx, fy]), ny_edge=np.concatenate([z, fx, rny]),
               short_x=np.concatenate([z > 0, rsx, fy > 0]), short_y=np.concatenate([z > 0, fx > 0, rsy]))
    out["lat_x"], out["lat_y"] = out["nx_edge"] == 0, out["ny_edge"] == 0  # a rounded-edge ray's other coordinate is a lattice point
    order = rng.permutation(kx.size)
    return {k: v[order] for k, v in out.items()}


def layout_edges():
    q = edges_rays()
    z = np.zeros(q["x_m"].size)
    return _launch_state(q["x_m"], q["y_m"], z, z, np.random.default_rng(203))


NX3, NY3 = 344, 257  # the detector layout 3's claims are made on (range DET3, chain MASK)


def layout_anchored():
    rng = np.random.default_rng(303)
    wx, wy = (DET3[1] - DET3[0]) / NX3, (DET3[3] - DET3[2]) / NY3
    ex, ey = lambda i: DET3[0] + i * wx, lambda j: DET3[2] + j * wy  # bin edges [mm]; rays keep 5 % of a bin away from them

    def box(n, i0, i1, j0, j1):  # n rays inside bins [i0, i1) x [j0, j1)
        return (rng.uniform(ex(i0) + 0.05 * wx, ex(i1) - 0.05 * wx, n), rng.uniform(ey(j0) + 0.05 * wy, ey(j1) - 0.05 * wy, n))

    def off(n):  # alive, but right of the detector (radius < 7.6 mm)
        return rng.uniform(6.2, 7.0, n), rng.uniform(-3.0, 3.0, n)

    def masked(n):  # radius > 8 mm
        return rng.uniform(8.5, 9.4, n), rng.uniform(-2.0, 2.0, n)

    def cat(*parts):
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    groups = [
        cat(box(1, 0, 1, 0, 1), box(255, NX3 - 10, NX3, NY3 - 8, NY3)),                    # (a)
        cat(box(1, NX3 - 3, NX3 - 2, NY3 - 2, NY3 - 1), box(255, NX3 - 3, NX3, NY3 - 2, NY3)),  # (b)
        cat(off(128), masked(128)),                                                         # (c)
        cat(off(100), box(1, 170, 171, 120, 121), masked(100), off(55)),                    # (d)
        box(256, 150, 179, 130, 144),                                                       # (e): 29 x 14 bins
        box(1, 230, 231, 40, 41),                                                           # (f)
    ]
    x, y = cat(*groups)
    assert x.size == 5 * WG + 1
    z = np.zeros(x.size)
    return _launch_state(x * 1e-3, y * 1e-3, z, z, rng)


N_ONE = 66_000


def layout_one_bin():
    rng = np.random.default_rng(404)
    x = 1.1 + 0.01 * (rng.permutation(N_ONE) + 0.5) / N_ONE  # distinct, inside one bin of every detector of BINS on DET
    y = 2.0 + 0.01 * (rng.permutation(N_ONE) + 0.5) / N_ONE
    z = np.zeros(N_ONE)
    return _launch_state(x * 1e-3, y * 1e-3, z, z, rng)


LAYOUTS = {"scatter": layout_scatter, "edges": layout_edges, "anchored": layout_anchored, "one_bin": layout_one_bin}


def straight_line(s0):
    """rf (4, N) of a ray that is not deflected: the entry state carried to the exit plane (what the empty volume does)."""
    tx, ty = s0[3] / s0[5], s0[4] / s0[5]
    return np.stack([s0[0] + tx * 2 * EXT, np.arctan(tx), s0[1] + ty * 2 * EXT, np.arctan(ty)])


def host_front_end(rf, ops):
    """m_to_mm and a chain of OP_DIST / OP_CIRC_AP in plain numpy (the CPU tests' stand-in for RayBundle.optics)."""
    r = rf * np.array([1e3, 1.0, 1e3, 1.0])[:, None]
    for o in ops:
        if o[0] == OP_DIST:
            r[0], r[2] = r[0] + o[1] * r[1], r[2] + o[1] * r[3]
        elif o[0] == OP_CIRC_AP:
            r[:, r[0] ** 2 + r[2] ** 2 > o[1] ** 2] = np.nan
        else:
            raise ValueError(o)
    return r


# ---------------------------------------------------------------- what a layout claims, on post-chain coordinates r [mm]
def hist_bins(v, lo, hi, n):
    """np.histogramdd's bin of v: searchsorted(edges, v, 'right') - 1, the last edge closed, -1 for outliers and NaN."""
    e = np.linspace(lo, hi, n + 1)
    with np.errstate(invalid="ignore"):
        j = np.where(v == hi, n - 1, np.searchsorted(e, v, "right") - 1)
        return np.where((v >= lo) & (v <= hi), j, -1)


def workgroups(r, nx, ny, rng, tile):
    """Per workgroup of 256 consecutive rays: hits, the patch origin, how many hits fall outside the tile, whether the
    tile overhangs the detector."""
    bx, by = hist_bins(r[0], rng[0], rng[1], nx), hist_bins(r[2], rng[2], rng[3], ny)
    hit = (bx >= 0) & (by >= 0)
    out = []
    for s in range(0, r.shape[1], WG):
        h = hit[s:s + WG]
        hx, hy = bx[s:s + WG][h], by[s:s + WG][h]
        g = dict(rays=h.size, hits=int(h.sum()), nan=int(np.isnan(r[0, s:s + WG]).sum()), org=None, out_of_tile=0, overhang=False,
                 bins=len(set(zip(hx.tolist(), hy.tolist()))))
        if g["hits"]:
            ox, oy = int(hx.min()), int(hy.min())
            g.update(org=(ox, oy), out_of_tile=int(((hx - ox >= tile[0]) | (hy - oy >= tile[1])).sum()),
                     overhang=ox + tile[0] > nx or oy + tile[1] > ny)
        out.append(g)
    return out


def claims_scatter(r_plain, r_mask):
    """Layout 1 on the 344 x 257 detector: in every workgroup at least half of the hits lie outside even the counts tile,
    rays miss the detector, and the mask kills some."""
    for r in (r_plain, r_mask):
        gs = workgroups(r, 344, 257, DET, TILE_COUNTS)
        assert [g["rays"] for g in gs] == [256, 256, 256, 256, 37]
        for g in gs:
            assert g["hits"] >= 20 and 2 * g["out_of_tile"] >= g["hits"] and 10 * g["bins"] >= 9 * g["hits"], g
    alive = ~np.isnan(r_plain[0])
    assert alive.all() and np.isnan(r_mask[0]).sum() >= 20
    miss = (np.abs(r_plain[0]) > 9) | (np.abs(r_plain[2]) > 6.75)
    assert miss.sum() >= 20 and (~miss).sum() >= 800


def claims_edges(r):
    """Layout 2 on the 64 x 32 detector of DET2: the lattice rays' coordinates ARE the lattice, and their on-edge counts are
    those of the integers; the rounded-edge rays sit, bit for bit, on an inner edge of their own detector."""
    q = edges_rays()
    kx, ky, lx, ly = q["kx"], q["ky"], q["lat_x"], q["lat_y"]
    assert np.array_equal(r[0], q["x_m"] * 1e3) and np.array_equal(r[2], q["y_m"] * 1e3)
    assert np.array_equal(r[0][lx], 1000 * kx[lx] * 2.0 ** -20) and np.array_equal(r[2][ly], 1000 * ky[ly] * 2.0 ** -20)
    xe, ye = np.linspace(DET2[0], DET2[1], 65), np.linspace(DET2[2], DET2[3], 33)
    on_x, on_y = np.isin(r[0], xe), np.isin(r[2], ye)
    assert np.array_equal(on_x, lx & (kx % 256 == 0) & (np.abs(kx) <= 8192)) and np.array_equal(on_y, ly & (ky % 256 == 0) & (np.abs(ky) <= 4096))
    # every edge of both axes carries a ray, and so does the lattice point either side of it
    for d in (-1, 0, 1):
        assert np.isin(xe + d * U, r[0]).all() and np.isin(ye + d * U, r[2]).all()
    assert on_x.sum() >= 65 + 130 and on_y.sum() >= 33 + 130 and (on_x & on_y).sum() >= 130
    assert ((r[0] == DET2[1]) & (r[2] == DET2[3])).any() and ((r[0] == DET2[0]) & (r[2] == DET2[2])).any()
    # the rounded edges: on an edge of np.linspace, between two lattice points, and the kernel's first guess one bin low on some
    n_short = 0
    for v, (lo, hi), n_edge, short, bins in ((r[0], DET2[:2], q["nx_edge"], q["short_x"], ROUNDED_BINS[0]),
                                             (r[2], DET2[2:], q["ny_edge"], q["short_y"], ROUNDED_BINS[1])):
        for n in bins:
            sel = n_edge == n
            e = np.linspace(lo, hi, n + 1)
            idx = np.searchsorted(e, v[sel])
            assert sel.sum() >= 12 and np.array_equal(e[idx], v[sel]) and np.all(v[sel] / U != np.round(v[sel] / U)), (n, int(sel.sum()))
            guess = ((v[sel] - lo) / ((hi - lo) / n)).astype(int)
            assert np.array_equal(guess < idx, short[sel]) and np.all(guess <= idx)
            assert (guess < idx).sum() >= 5, (n, int((guess < idx).sum()))
            n_short += int((guess < idx).sum())
    gs = workgroups(r, 64, 32, DET2, TILE_COMPLEX)
    assert len(gs) == 5 and all(g["out_of_tile"] > 0 for g in gs[:4])  # shuffled: a complex / intensity tile cannot hold a workgroup
    return int(on_x.sum()), int(on_y.sum()), int((on_x & on_y).sum()), n_short


def claims_anchored(r):
    """Layout 3 on the 344 x 257 detector of DET3 behind the mask, for the counts tile and the complex / intensity tile."""
    for tile in (TILE_COUNTS, TILE_COMPLEX):
        a, b, c, d, e, f = workgroups(r, NX3, NY3, DET3, tile)
        assert a["hits"] == 256 and a["org"] == (0, 0) and a["out_of_tile"] == 255, a
        assert b["hits"] == 256 and b["org"] == (NX3 - 3, NY3 - 2) and b["overhang"] and b["out_of_tile"] == 0, b
        assert c["rays"] == 256 and c["hits"] == 0 and c["nan"] == 128, c
        assert d["rays"] == 256 and d["hits"] == 1 and d["nan"] == 100, d
        assert e["hits"] == 256 and e["out_of_tile"] == 0 and not e["overhang"] and e["bins"] > 100, e
        assert f["rays"] == 1 and f["hits"] == 1, f


def claims_one_bin(r):
    """Layout 4: distinct positions, one bin on every detector of BINS."""
    assert np.unique(r[0]).size == N_ONE and np.unique(r[2]).size == N_ONE and N_ONE > 65535
    for nx, ny in BINS:
        g = workgroups(r[:, :WG], nx, ny, DET, TILE_COMPLEX)[0]
        assert g["hits"] == 256 and g["bins"] == 1, (nx, ny, g)
        bx, by = hist_bins(r[0], DET[0], DET[1], nx), hist_bins(r[2], DET[2], DET[3], ny)
        assert bx.min() == bx.max() >= 0 and by.min() == by.max() >= 0


# ---------------------------------------------------------------- the independent results
def complex_reference(x, y, E, nxe, nye, rng):
    """(sums (4, nye-1, nxe-1) longdouble: Re Ex, Im Ex, Re Ey, Im Ey; sums of the moduli; rays per pixel) binned as
    rtm_solver.py:436-448 bins: np.digitize - 1, right edge open, everything outside dropped (NaN sorts past the last edge)."""
    ix = np.digitize(x, np.linspace(rng[0], rng[1], nxe)) - 1
    iy = np.digitize(y, np.linspace(rng[2], rng[3], nye)) - 1
    ok = (ix >= 0) & (ix < nxe - 1) & (iy >= 0) & (iy < nye - 1)
    E = np.asarray(E)
    comps = np.stack([E[0].real, E[0].imag, E[1].real, E[1].imag])[:, ok].astype(np.longdouble)
    assert not np.isnan(comps).any()
    sums, mods = np.zeros((2, 4, (nye - 1) * (nxe - 1)), np.longdouble)
    flat = iy[ok] * (nxe - 1) + ix[ok]
    order = np.argsort(flat, kind="stable")
    pix, start, count = np.unique(flat[order], return_index=True, return_counts=True)
    if pix.size:  # longdouble sums of each pixel's rays: their own rounding (n 2^-64) is far below the bound
        sums[:, pix] = np.add.reduceat(comps[:, order], start, axis=1)
        mods[:, pix] = np.add.reduceat(np.abs(comps[:, order]), start, axis=1)
    n = np.zeros((nye - 1) * (nxe - 1))
    n[pix] = count
    shape = (nye - 1, nxe - 1)
    sums, mods, n = sums.reshape((4,) + shape), mods.reshape((4,) + shape), n.reshape(shape)
    return sums, mods, n


def assert_complex_within_bound(amp, ref, what, factor=1.0):
    sums, mods, n = ref
    assert amp.shape == (2,) + n.shape and amp.dtype == np.complex128, (what, amp.shape)
    got = np.stack([amp[0].real, amp[0].imag, amp[1].real, amp[1].imag])
    assert not np.isnan(got).any(), what
    d = np.abs(got.astype(np.longdouble) - sums)
    bound = factor * (n + 16) * EPS * mods
    lit = mods > 0
    worst = float(np.max(d[lit] / bound[lit])) if lit.any() else 0.0
    assert np.all(d <= bound), (what, worst)
    assert np.all(got[:, n == 0] == 0.0), (what, "an empty pixel is not exactly 0.0")
    return worst


def counts_reference(r, nx, ny, rng):
    ok = ~(np.isnan(r[0]) | np.isnan(r[2]))
    return np.histogram2d(r[0][ok], r[2][ok], bins=[nx, ny], range=[[rng[0], rng[1]], [rng[2], rng[3]]])[0].T


def assert_amplitude(img, amp, what):
    """DetectorImage.amplitude() = sqrt(Re(Ax)^2 + Re(Ay)^2) of the sums the image holds: two products and a sum of
    non-negative terms (2^-53 each, halved by the root) and a root good to one ulp: 4 * 2^-53 relative."""
    want = np.sqrt(amp[0].real ** 2 + amp[1].real ** 2)
    assert np.all(np.abs(img.amplitude() - want) <= 4 * EPS * want), what


# ================================================================ CPU tests
def test_layout_builders_hold_their_claims():
    """Every layout claims on the straight-line prediction of rf what its GPU test asserts on the GPU's own rf: the on-edge
    ray counts, a workgroup with no hit, one with exactly one hit, the overhanging cluster's minimum bin, the scatter's
    out-of-tile share (at least half of every workgroup's hits), a single bin for 66 000 distinct rays."""
    rf = straight_line(layout_scatter())
    claims_scatter(host_front_end(rf, []), host_front_end(rf, MASK))
    s0 = layout_edges()
    assert s0.shape == (9, 4 * WG + 5) and not s0[3].any() and not s0[4].any()
    on_x, on_y, corners, short = claims_edges(host_front_end(straight_line(s0), []))
    print(f"layout 2: {on_x} rays on an x edge, {on_y} on a y edge, {corners} on a corner, {short} on a rounded edge the first guess misses, of {s0.shape[1]}")
    s0 = layout_anchored()
    claims_anchored(host_front_end(straight_line(s0), MASK))
    # without the mask the masked rays are off the detector: workgroup (c) still holds no hit
    assert workgroups(host_front_end(straight_line(s0), []), NX3, NY3, DET3, TILE_COUNTS)[2]["hits"] == 0
    claims_one_bin(host_front_end(straight_line(layout_one_bin()), []))
    for name, make in LAYOUTS.items():  # seeded: the same rays every time, a field of its own per ray
        a, b = make(), make()
        assert np.array_equal(a, b) and np.unique(a[6]).size == a.shape[1], name
        assert np.abs(a[0]).max() < 9.6e-3 and np.abs(a[1]).max() < 9.6e-3  # inside the +-10 mm volume


def test_constants_are_the_library_s(built):
    """The tile sizes, op codes and c this file's claims are worked out with are those of deposit.hip and the engine."""
    import os
    import re

    from conftest import ROOT
    from synthpy_amd import engine

    assert (engine.c, engine.OP_DIST, engine.OP_CIRC_AP) == (C0, OP_DIST, OP_CIRC_AP)
    text = open(os.path.join(ROOT, "synthpy_amd", "csrc", "deposit.hip")).read()
    tiles = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"constexpr int k(\w*)TileW = (\d+), k\w*TileH = (\d+);", text)}
    assert tiles == {"": TILE_COUNTS, "C": TILE_COMPLEX, "I": TILE_COMPLEX}, tiles
    assert "__launch_bounds__(256) void k_deposit(" in text and "__launch_bounds__(256) void k_deposit_intensity(" in text
    assert built.MAX_ANALYSERS >= 3


def test_dyadic_lattice_is_exact():
    """Layout 2's exactness claims: k 2^-20 m times 1e3 is 1000 k 2^-20 mm without rounding, np.linspace's edges of the
    256 u detector are lattice points, and the kernel's edge formula i*step + lo (last edge = hi) gives the same doubles."""
    k = np.arange(-8500, 8501)
    assert np.array_equal((k * 2.0 ** -20) * 1e3, (1000 * k) * 2.0 ** -20)
    assert all(float(v).as_integer_ratio()[1] <= 2 ** 20 for v in ((k[::97] * 2.0 ** -20) * 1e3))
    for lo, hi, n in ((DET2[0], DET2[1], 64), (DET2[2], DET2[3], 32)):
        step = (hi - lo) / n
        assert step == 256 * U
        kernel = np.arange(n + 1) * step + lo
        kernel[-1] = hi
        lattice = lo + 256 * U * np.arange(n + 1)
        assert np.array_equal(np.linspace(lo, hi, n + 1), kernel) and np.array_equal(kernel, lattice)
        assert np.array_equal(lattice / U, np.round(lattice / U))


# the host-array kernels' cases: (lo, hi, bins); for each the kernel's edge formula reproduces np.linspace bit for bit
RANGES = [(0.1, 0.7, 3), (-7.0, 6.0, 255), (-6.75, 6.75, 257), (-1.0, 1.0, 7), (1e15, 1e15 + 64, 64), (0.3, 0.3000001, 5)]
SIZES = [0, 1, 255, 256, 257]


def axis_values(lo, hi, n):
    """Every edge (lo and hi among them), the doubles either side of each, +-inf, +-0.0 and a subnormal."""
    e = np.linspace(lo, hi, n + 1)
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [np.inf, -np.inf, 0.0, -0.0, 5e-324]])


def host_points(rx, ry, seed):
    """(x, y, E): each special value of one axis against interior values of the other and against the other's own special
    values, NaN in x only and in y only; shuffled."""
    rng = np.random.default_rng(seed)
    vx, vy = axis_values(*rx), axis_values(*ry)
    inx, iny = rng.uniform(rx[0], rx[1], vy.size + 8), rng.uniform(ry[0], ry[1], vx.size + 8)
    m = max(vx.size, vy.size)
    x = np.concatenate([vx, inx[:vy.size], np.resize(vx, m), np.full(4, np.nan), inx[-8:-4], np.full(4, np.nan)])
    y = np.concatenate([iny[:vx.size], vy, np.resize(np.roll(vy, 1), m), iny[-8:-4], np.full(4, np.nan), np.full(4, np.nan)])
    order = rng.permutation(x.size)
    E = rng.uniform(-1.5, 1.5, (2, x.size)) + 1j * rng.uniform(-1.5, 1.5, (2, x.size))
    return x[order], y[order], E


def test_host_cases_hold_their_claims():
    """The edge formula of deposit.hip (make_edges, edge_at) equals np.linspace on every range used here, and the point sets
    hold what they say: every edge, its neighbours, lo, hi, infinities, zeros of both signs, a subnormal, one-sided NaN."""
    for q, (lo, hi, n) in enumerate(RANGES):
        step = (hi - lo) / n
        kernel = np.arange(n + 1) * step + lo
        kernel[-1] = hi
        e = np.linspace(lo, hi, n + 1)
        assert np.array_equal(kernel, e) and np.all(np.diff(e) > 0), (lo, hi, n)
        x, y, E = host_points(RANGES[q], RANGES[(q + 1) % len(RANGES)], q)
        assert x.shape == y.shape and E.shape == (2, x.size) and x.size >= 3 * (n + 1)
        for v in (e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [np.inf, -np.inf, 5e-324]):
            assert np.isin(v, x).all()
        assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
        assert (np.isnan(x) & ~np.isnan(y)).sum() == 4 and (np.isnan(y) & ~np.isnan(x)).sum() == 4
        assert (np.isin(x, e) & np.isin(y, np.linspace(*RANGES[(q + 1) % len(RANGES)][:2], RANGES[(q + 1) % len(RANGES)][2] + 1))).sum() >= 3


def test_complex_reference_binning():
    """complex_reference's binning on a case small enough to write out: the right edge is open, the left closed, NaN and
    outliers are dropped, and the sums are those of the rays of the pixel."""
    x = np.array([0.0, 1.0, 1.0, 2.0, np.nan, -0.1, 0.5, np.nextafter(2.0, 0)])
    y = np.array([0.0, 0.0, 1.0, 0.5, 0.5, 0.5, 1.0, np.nextafter(1.0, 0)])
    E = np.stack([np.arange(1.0, 9.0) + 0j, 1j * np.arange(1.0, 9.0)])
    sums, mods, n = complex_reference(x, y, E, 3, 2, (0.0, 2.0, 0.0, 1.0))  # 2 x 1 pixels: [0, 1) and [1, 2) by [0, 1)
    assert n.tolist() == [[1, 2]] and sums[0].tolist() == [[1.0, 10.0]] and sums[3].tolist() == [[1.0, 10.0]]
    assert not sums[1].any() and not sums[2].any() and mods[0].tolist() == [[1.0, 10.0]]


# ================================================================ GPU tests
_TRACED = {}


def traced(eng, name, precision="f64"):
    """(rays, s0, rf, Jf) of a layout traced through the empty volume, once per module."""
    key = (name, precision)
    if key not in _TRACED:
        s0 = LAYOUTS[name]()
        x = np.linspace(-EXT, EXT, 16)
        vol = eng.Volume.from_ne(np.zeros((16, 16, 16)), x, x, x, 1064e-9, "z", phaseshift=True)
        rays = eng.RayBundle(s0.shape[1]).upload(s0)
        rays.trace(vol, eng.default_t_end(EXT), EXT, sort_rays=False, precision=precision)
        _, rf, Jf = rays.download()
        _TRACED[key] = (rays, s0, np.array(rf), np.array(Jf))
    return _TRACED[key]


def assert_claims(name, rays, s0, rf):
    """What the layout claims, on the GPU's own rays (no test passes on rays that are not where it thinks they are)."""
    front = lambda ops: np.array(rays.optics(ops)[0])
    assert not np.isnan(rf).any() and np.array_equal(front([]), rf * np.array([1e3, 1.0, 1e3, 1.0])[:, None])
    if name != "scatter":  # zero angle: the exit position IS the launch position
        assert np.array_equal(rf[0], s0[0]) and np.array_equal(rf[2], s0[1]) and not rf[1].any() and not rf[3].any()
    if name == "scatter":
        claims_scatter(front([]), front(MASK))
    elif name == "edges":
        claims_edges(front([]))
    elif name == "anchored":
        claims_anchored(front(MASK))
    else:
        claims_one_bin(front([]))


def cases(eng, name):
    """(range, [(nx, ny) bins], {chain name: ops}) of a layout."""
    chains = {"empty": [], "dist": [(eng.OP_DIST, 400.0)], "shadow_two": eng.chain_shadow_two()}
    if name in ("scatter", "anchored"):
        chains["mask"] = MASK
    return {"scatter": DET, "edges": DET2, "anchored": DET3, "one_bin": DET}[name], BINS2 if name == "edges" else BINS, chains


def make_image(eng, kind, nx, ny, rng, n_ch=0):
    if kind == "counts":
        return eng.DetectorImage(eng.IMG_COUNTS, nx, ny, *rng)
    if kind == "complex":
        return eng.DetectorImage(eng.IMG_COMPLEX, nx + 1, ny + 1, *rng)
    return eng.DetectorImage(eng.IMG_INTENSITY, nx, ny, *rng, n_channels=n_ch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_counts_on_layout(eng, name):
    """k_deposit<COUNTS> with and without the LDS tile against np.histogram2d: equal integers, `deposited` equal to their
    sum, two deposits exactly twice one, zero() all zeros."""
    rays, s0, rf, Jf = traced(eng, name)
    assert_claims(name, rays, s0, rf)
    rng, bins, chains = cases(eng, name)
    for cname, ops in chains.items():
        r = np.array(rays.optics(ops)[0])
        for nx, ny in bins:
            H_ref = counts_reference(r, nx, ny, rng)
            what = f"counts {name} {cname} {nx}x{ny}"
            assert H_ref.sum() > 0, what
            got = []
            for tiles in (True, False):
                img = make_image(eng, "counts", nx, ny, rng)
                _, deposited = rays.deposit(img, ops, lds_tiles=tiles)
                H = img.download()
                assert H.shape == (ny, nx) and np.array_equal(H, H_ref), (what, tiles, int(np.abs(H - H_ref).sum()))
                assert deposited == int(H_ref.sum()), (what, tiles)
                rays.deposit(img, ops, lds_tiles=tiles)
                assert np.array_equal(img.download(), 2 * H_ref), (what, tiles, "two deposits")
                img.zero()
                assert not img.download().any()
                img.close()
                got.append(H)
            assert np.array_equal(got[0], got[1]), what
    if name == "one_bin":
        assert H_ref.max() == N_ONE > 65535


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_complex_on_layout(eng, name):
    """k_deposit<COMPLEX> with and without the LDS tile against the longdouble sums of the same E (RayBundle.optics with
    with_E), with and without field propagation and a reference beam; amplitude() against the downloaded sums."""
    rays, s0, rf, Jf = traced(eng, name)
    assert_claims(name, rays, s0, rf)
    rng, bins, chains = cases(eng, name)
    runs = [(c, ops, {}) for c, ops in chains.items()]
    runs += [("dist+k", chains["dist"], dict(kwave=KWAVE)), ("shadow_two+k+ref", chains["shadow_two"], dict(kwave=KWAVE, ref_beam=(10, 20)))]
    worst = 0.0
    for cname, ops, kw in runs:
        r, E = rays.optics(ops, with_E=True, **kw)
        r, E = np.array(r), np.array(E)
        for nx, ny in bins:
            ref = complex_reference(r[0], r[2], E, nx + 1, ny + 1, rng)
            what = f"complex {name} {cname} {nx + 1}x{ny + 1} edges"
            for tiles in (True, False):
                img = make_image(eng, "complex", nx, ny, rng)
                _, deposited = rays.deposit(img, ops, lds_tiles=tiles, **kw)
                amp = img.download()
                worst = max(worst, assert_complex_within_bound(amp, ref, (what, tiles)))
                assert deposited == int(ref[2].sum()), (what, tiles)
                assert_amplitude(img, amp, (what, tiles))
                img.zero()
                assert not img.download().any()
                img.close()
    print(f"complex {name}: max |d| / bound = {worst:.3g}")
    if name == "one_bin":
        assert ref[2].max() == N_ONE


@pytest.mark.gpu
@pytest.mark.parametrize("name, n_ch", [(name, n_ch) for name in LAYOUTS for n_ch in ((1, 2, 3, 4) if name == "scatter" else (1, 3))])
def test_intensity_on_layout(eng, name, n_ch):
    """k_deposit_intensity<1> and <3> (a None analyser among them) with and without the LDS tile against np.histogram2d with
    weights, under test_polarimetry's bound; <2> and <4> on the scattered rays, so that every instantiation runs here."""
    rays, s0, rf, Jf = traced(eng, name)
    assert_claims(name, rays, s0, rf)
    rng, bins, chains = cases(eng, name)
    if n_ch in (2, 4):
        bins = BINS2  # with the detectors around the 32 x 16 tile
    an = ANALYSERS[n_ch]
    for cname, ops in chains.items():
        r = np.array(rays.optics(ops)[0])
        for nx, ny in bins:
            I_ref, n, S = _numpy_images(r[0], r[2], Jf, an, nx, ny, rng)
            for tiles in (True, False):
                img = make_image(eng, "intensity", nx, ny, rng, n_ch)
                _, deposited = rays.deposit_intensity(img, ops, an, lds_tiles=tiles)
                _assert_within_bound(img.download(), I_ref, n, S, f"intensity {name} {cname} {n_ch}ch {nx}x{ny} tiles={int(tiles)}")
                assert deposited == int(n.sum())
                img.zero()
                assert not img.download().any()
                img.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scatter", "edges", "anchored"])
def test_two_halves_in_two_bundles(eng, name):
    """The two halves of a layout, traced as two bundles and deposited into ONE image, against the one-bundle result: equal
    counts, and sums within the same bound of the same reference (a sum in another order).  The split is no multiple of 256,
    so the second half's workgroups hold other rays than before.  The chunked driver rests on this."""
    rays, s0, rf, Jf = traced(eng, name)
    rng, bins, chains = cases(eng, name)
    cname = "mask" if "mask" in chains else "shadow_two"
    ops, an = chains[cname], ANALYSERS[3]
    h = s0.shape[1] // 2 + 3
    x = np.linspace(-EXT, EXT, 16)
    vol = eng.Volume.from_ne(np.zeros((16, 16, 16)), x, x, x, 1064e-9, "z", phaseshift=True)
    parts = []
    for part in (s0[:, :h], s0[:, h:]):
        b = eng.RayBundle(part.shape[1]).upload(np.ascontiguousarray(part))
        b.trace(vol, eng.default_t_end(EXT), EXT, sort_rays=False, precision="f64")
        parts.append(b)
    r, E = rays.optics(ops, with_E=True)
    r, E = np.array(r), np.array(E)
    worst = 0.0
    for nx, ny in ((65, 33), (344, 257)):
        for tiles in (True, False):
            one, two = make_image(eng, "counts", nx, ny, rng), make_image(eng, "counts", nx, ny, rng)
            _, d1 = rays.deposit(one, ops, lds_tiles=tiles)
            d2 = sum(b.deposit(two, ops, lds_tiles=tiles)[1] for b in parts)
            assert d1 == d2 > 0 and np.array_equal(one.download(), two.download())
            assert np.array_equal(two.download(), counts_reference(r, nx, ny, rng))
            two = make_image(eng, "complex", nx, ny, rng)
            for b in parts:
                b.deposit(two, ops, lds_tiles=tiles)
            worst = max(worst, assert_complex_within_bound(two.download(), complex_reference(r[0], r[2], E, nx + 1, ny + 1, rng),
                                                           ("halves complex", name, nx, ny, tiles)))
            two = make_image(eng, "intensity", nx, ny, rng, 3)
            for b in parts:
                b.deposit_intensity(two, ops, an, lds_tiles=tiles)
            I_ref, n, S = _numpy_images(r[0], r[2], Jf, an, nx, ny, rng)
            _assert_within_bound(two.download(), I_ref, n, S, f"halves intensity {name} {nx}x{ny} tiles={int(tiles)}")
    print(f"halves complex {name}: max |d| / bound = {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scatter", "edges"])
def test_mixed_trace_exact_counts(eng, name):
    """The same layout traced by the mixed build and deposited with exact counts (k_deposit<COUNTS, *, true>, then
    k_deposit_list for the rays the edge guard traced again), with and without tiles: the float64 bundle's image and
    `deposited`, integer for integer, with rays exactly on bin edges."""
    rays, s0, rf, Jf = traced(eng, name)
    mixed = traced(eng, name, "mixed")[0]
    rng, bins, chains = cases(eng, name)
    for cname, ops in chains.items():
        r = np.array(rays.optics(ops)[0])
        for nx, ny in bins:
            H_ref = counts_reference(r, nx, ny, rng)
            ref_img = make_image(eng, "counts", nx, ny, rng)
            _, want = rays.deposit(ref_img, ops)
            H64 = ref_img.download()
            assert np.array_equal(H64, H_ref)
            for tiles in (True, False):
                img = make_image(eng, "counts", nx, ny, rng)
                _, deposited = mixed.deposit(img, ops, lds_tiles=tiles, exact_counts=True)
                print(f"mixed {name} {cname} {nx}x{ny} tiles={int(tiles)}: retraced {mixed.retraced} of {mixed.n}")
                H = img.download()
                assert np.array_equal(H, H64), (name, cname, nx, ny, tiles, int(np.abs(H.astype(np.int64) - H64).sum()))
                assert deposited == want
                img.close()
            ref_img.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", range(len(RANGES)))
def test_host_array_kernels(eng, q):
    """sr_hist2d, sr_interferogram (sums) and sr_intensity2d on direct inputs: every edge of both axes, the doubles either
    side of it, lo, hi, +-inf, one-sided NaN, +-0.0, a subnormal; N in {0, 1, 255, 256, 257} and the whole set."""
    (xlo, xhi, nx), (ylo, yhi, ny) = RANGES[q], RANGES[(q + 1) % len(RANGES)]
    rng = (xlo, xhi, ylo, yhi)
    X, Y, EE = host_points(RANGES[q], RANGES[(q + 1) % len(RANGES)], q)
    worst = 0.0
    for N in SIZES + [X.size]:
        x, y, E = X[:N], Y[:N], np.ascontiguousarray(EE[:, :N])
        H_ref = counts_reference(np.stack([x, x, y, y]), nx, ny, rng)
        H = eng.hist2d(x, y, nx, ny, *rng)
        assert H.shape == (ny, nx) and np.array_equal(H, H_ref), (RANGES[q], N, int(np.abs(H - H_ref).sum()))
        Hc, amp = eng.interferogram(x, y, E, nx + 1, ny + 1, *rng, sums=True)
        ref = complex_reference(x, y, E, nx + 1, ny + 1, rng)
        worst = max(worst, assert_complex_within_bound(amp, ref, ("interferogram", RANGES[q], N)))
        want = np.sqrt(amp[0].real ** 2 + amp[1].real ** 2)
        assert np.all(np.abs(Hc - want) <= 4 * EPS * want)
        for an in ANALYSERS.values():
            I_ref, n, S = _numpy_images(x, y, E, an, nx, ny, rng)
            assert np.array_equal(n, H_ref)
            _assert_within_bound(eng.intensity2d(x, y, E, an, nx, ny, *rng), I_ref, n, S, f"intensity2d {RANGES[q]} N={N} {len(an)}ch")
    assert H_ref.sum() >= nx + ny and ref[2].sum() >= nx + ny - 2  # the whole set: the edges' rays were counted
    print(f"interferogram {RANGES[q]}: max |d| / bound = {worst:.3g}")
