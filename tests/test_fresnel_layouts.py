"""The gridding of the rays (grid_rays / propagate, sr_fresnel_grid / sr_fresnel_rays, synthpy_amd/csrc/fresnel.hip) on
rays that are NOT in general position: lattices, rays at one position, co-circular rays, rays along hull edges, rays on
one line, and nodes exactly on rays, on triangle edges, on the hull's edges and on its vertices.  tests/test_fresnel.py
draws its rays from continuous distributions, where no orientation or in-circle predicate is ever exactly zero; every
tie-break of the search (nearest, mate, the team reduction's comparator, the >= tests of locate, in_hull) is reached
only by layouts like these.

Exact layouts.  Every ray and node coordinate is origin + integer * unit with unit a power of two, and the integers
are small enough that the float64 orientation and in-circle expressions of fresnel.hip are exact (and that the reference
below fits int64): test_layouts_are_exact asserts the bounds.  So there is no rounding to argue about: the kernel's
inside / outside decision and its triangle must be exactly right, and the checker has no tolerance.  Ray indices are
shuffled with a fixed seed, so index order and position order are unrelated.

The exact reference is plain numpy on the integers and independent of the kernel's search:
  * closed-hull membership of a node from an exact monotone chain (a node on the hull's boundary is inside, as scipy's
    LinearNDInterpolator treats it: test_scipy_fills_the_closed_hull);
  * check(): the three indices of a node's triangle are distinct, ascending and not collinear, the node is in the closed
    triangle, no ray is strictly inside the circumcircle (every triangle against every ray), and each vertex is the
    lowest index among the rays at its position;
  * the value: the barycentric interpolation of the triangle's vertex values at the node, formed in integers and rounded
    once.
Values are compared to 1e-12 of the field's maximum (the tolerance tests/test_fresnel.py uses for the gridded fields)
and the propagated field to 1e-10 (the tolerance of its test_propagate_equals_reference); everything else is exact.
"""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from synthpy_amd.simulator import fresnel_integral as fi

LWL, Z = 1064e-9, 0.05
VAL_BITS = 10  # ray values are integers / 2^10


# ---------------------------------------------------------------- the layouts
class Layout:
    """rays at (x0 + xi * unit, y0 + yi * unit), nodes at np.meshgrid(x0 + gxi * unit, y0 + gyi * unit); xi, yi, gxi, gyi
    int64, unit a power of two.  The rays are shuffled by RandomState(seed)."""

    def __init__(self, name, pts, gxi, gyi, seed, unit=2.0 ** -16, x0=0.0, y0=0.0):
        pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
        pts = pts[np.random.RandomState(seed).permutation(len(pts))]
        self.name, self.seed, self.unit, self.x0, self.y0 = name, seed, unit, x0, y0
        self.xi, self.yi = np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])
        self.gxi, self.gyi = np.asarray(gxi, dtype=np.int64), np.asarray(gyi, dtype=np.int64)
        self.n = len(pts)

    x = property(lambda s: s.x0 + s.xi * s.unit)
    y = property(lambda s: s.y0 + s.yi * s.unit)
    gx = property(lambda s: s.x0 + s.gxi * s.unit)
    gy = property(lambda s: s.y0 + s.gyi * s.unit)
    shape = property(lambda s: (len(s.gyi), len(s.gxi)))

    def jones(self):
        j = np.zeros((4, self.n))
        j[0], j[2] = self.x, self.y
        return j

    def reshuffled(self, seed):
        """the same rays in another index order, and the permutation: ray k of the result is ray perm[k] of self"""
        perm = np.random.RandomState(seed).permutation(self.n)
        other = Layout(self.name, np.c_[self.xi, self.yi], self.gxi, self.gyi, 0, self.unit, self.x0, self.y0)
        other.xi, other.yi = np.ascontiguousarray(self.xi[perm]), np.ascontiguousarray(self.yi[perm])
        return other, perm


def lattice(nx, ny, sx, sy, ox=0, oy=0):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    return np.c_[ox + sx * i.ravel(), oy + sy * j.ravel()]


def ring_points(r=65):
    return np.array([(a, b) for a in range(-r, r + 1) for b in range(-r, r + 1) if a * a + b * b == r * r])


LATTICE17 = lattice(17, 17, 4, 4)  # quarter steps are the unit
Q17 = np.arange(-4, 69)  # 73 nodes at quarter steps, one step outside the lattice on either side


def _layouts():
    L = {}

    def add(name, *a, **k):
        L[name] = Layout(name, *a, seed=1000 + len(L), **k)

    add("lattice17", LATTICE17, Q17, Q17)
    # 64 x 64 rays, the unit is half a step: 129 x 129 nodes at half steps, one outside on either side.  ~1400 bins with the
    # rays on their boundaries; more rays than the first pass's budget
    add("lattice64", lattice(64, 64, 2, 2), np.arange(-1, 128), np.arange(-1, 128))
    # far from the origin: 1 m, -2 m, a step of 2^-14 m
    add("offset", LATTICE17, Q17, Q17, x0=1.0, y0=-2.0)
    # 256 x 4 rays, the x step 64 times the y step (the unit is half a y step); nodes at half steps: bins far from square
    strip = lattice(256, 4, 128, 2)
    sgx, sgy = np.arange(-64, 255 * 128 + 65, 64), np.arange(-1, 8)
    add("strip", strip, sgx, sgy)
    add("strip_t", strip[:, ::-1], sgy, sgx)
    # every position twice
    add("doubled", np.r_[LATTICE17, LATTICE17], Q17, Q17)
    # 200 further rays at one interior lattice position: one bin far above the mean
    add("pile", np.r_[LATTICE17, np.tile([[20, 36]], (200, 1))], Q17, Q17)
    # the 36 integer points of x^2 + y^2 = 65^2; nodes at every integer of the bounding square
    ring, rq = ring_points(), np.arange(-65, 66)
    add("ring", ring, rq, rq)
    add("ring_centre", np.r_[ring, [[0, 0]]], rq, rq)
    add("ring_lattice", np.r_[ring, lattice(17, 17, 4, 4, -32, -32)], rq, rq)
    # lattice64 (the unit is half a step) and four rays at the corners of a square 16 times wider; 127 x 127 nodes every
    # 8 steps: on lattice edges inside, in triangles whose circles hold the whole lattice outside, on the hull's edges
    w = 16 * 126
    add("far_corners", np.r_[lattice(64, 64, 2, 2, 944, 945), [[0, 0], [w, 0], [0, w], [w, w]]], np.arange(0, w + 1, 16),
        np.arange(0, w + 1, 16))
    # 33 rays on y = 0 and an apex: a hull of 3 vertices with 31 rays on one edge; the slanted edges hold a node every (4, 3)
    add("fan", np.r_[np.c_[4 * np.arange(33), np.zeros(33, int)], [[64, 48]]], np.arange(-4, 133), np.arange(-4, 53))
    add("minimal3", [[0, 0], [8, 0], [0, 8]], np.arange(-1, 10), np.arange(-1, 10))
    add("square4", [[0, 0], [8, 0], [0, 8], [8, 8]], np.arange(-1, 10), np.arange(-1, 10))
    k = np.arange(20)
    add("line_h", np.c_[4 * k, 0 * k + 5], np.arange(-4, 81, 2), np.arange(0, 11))
    add("line_v", np.c_[0 * k + 5, 4 * k], np.arange(0, 11), np.arange(-4, 81, 2))
    add("line_d", np.c_[4 * k, 2 * k], np.arange(-4, 81, 2), np.arange(-4, 43))
    return L


LAYOUTS = _layouts()
NAMES = list(LAYOUTS)
LINES = ("line_h", "line_v", "line_d")

# what each layout is there for: rays, distinct positions, strict hull vertices, nodes inside the closed hull, nodes exactly
# on the hull's boundary, nodes exactly on a ray
CLAIMS = {
    "lattice17": (289, 289, 4, 65 * 65, 4 * 64, 17 * 17),
    "lattice64": (4096, 4096, 4, 127 * 127, 4 * 126, 64 * 64),
    "offset": (289, 289, 4, 65 * 65, 4 * 64, 17 * 17),
    "strip": (1024, 1024, 4, 511 * 7, 2 * 510 + 2 * 6, 1024),
    "strip_t": (1024, 1024, 4, 511 * 7, 2 * 510 + 2 * 6, 1024),
    "doubled": (578, 289, 4, 65 * 65, 4 * 64, 17 * 17),
    "pile": (489, 289, 4, 65 * 65, 4 * 64, 17 * 17),
    "ring": (36, 36, 36, None, 140, 36),
    "ring_centre": (37, 37, 36, None, 140, 37),
    "ring_lattice": (36 + 289, 36 + 289, 36, None, 140, 36 + 289),
    "far_corners": (4100, 4100, 4, 127 * 127, 4 * 126, 4),
    "fan": (34, 34, 3, None, 129 + 2 * 15 + 1, 34),
    "minimal3": (3, 3, 3, 45, 24, 3),
    "square4": (4, 4, 4, 81, 32, 4),
    "line_h": (20, 20, 0, 0, 0, None),
    "line_v": (20, 20, 0, 0, 0, None),
    "line_d": (20, 20, 0, 0, 0, None),
}


# ---------------------------------------------------------------- the exact reference
def cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def strict_hull(xi, yi):
    """the strict convex hull (no collinear, no repeated point), counter-clockwise, by a monotone chain in Python
    integers; [] when the points span no area"""
    pts = sorted(set(zip(xi.tolist(), yi.tolist())))
    if len(pts) < 3:
        return []
    chains = []
    for seq in (pts, pts[::-1]):
        h = []
        for p in seq:
            while len(h) >= 2 and cross(h[-2], h[-1], p) <= 0:
                h.pop()
            h.append(p)
        chains.append(h[:-1])
    h = chains[0] + chains[1]
    return h if len(h) >= 3 else []


@functools.lru_cache(maxsize=None)
def hull_masks(name):
    """(strict hull, nodes in the closed hull, nodes on its boundary), the masks of shape (ny, nx)"""
    L = LAYOUTS[name]
    h = strict_hull(L.xi, L.yi)
    GX, GY = np.meshgrid(L.gxi, L.gyi)
    inside, on = np.full(GX.shape, bool(h)), np.zeros(GX.shape, bool)
    for (ax, ay), (bx, by) in zip(h, h[1:] + h[:1]):
        o = (bx - ax) * (GY - ay) - (by - ay) * (GX - ax)
        inside &= o >= 0
        on |= o == 0
    inside.setflags(write=False)
    return h, inside, on & inside


def lowest_at_position(L):
    """for every ray the lowest index among the rays at its position"""
    _, inv = np.unique(np.c_[L.xi, L.yi], axis=0, return_inverse=True)
    inv = inv.ravel()
    low = np.full(inv.max() + 1, L.n, dtype=np.int64)
    np.minimum.at(low, inv, np.arange(L.n))
    return low[inv]


OK, MASK, ORDER, FLAT, MISSES, CIRCLE, DUPLICATE = range(7)
REASON = ["ok", "inside / outside wrong", "indices not distinct and ascending", "collinear vertices", "node not in the triangle",
          "a ray strictly inside the circumcircle", "a vertex that is not the lowest index at its position"]


def holds_a_ray(xi, yi, ut):
    """for every triangle of ut (T, 3): is a ray strictly inside its circumcircle?  With B, C, D relative to A and
    cr = B x C > 0, D is strictly inside iff |D|^2 cr - D . (C_y |B|^2 - B_y |C|^2, B_x |C|^2 - C_x |B|^2) < 0, which is
    linear in (X^2 + Y^2, X, Y, 1) of D: one integer matrix product, every triangle against every ray"""
    ax, ay, bx, by, cx, cy = (v[ut[:, k]] for k in range(3) for v in (xi, yi))
    bx, by, cx, cy = bx - ax, by - ay, cx - ax, cy - ay
    cr = bx * cy - by * cx
    s = np.sign(cr)
    b2, c2 = bx * bx + by * by, cx * cx + cy * cy
    ux, uy, cr = (cy * b2 - by * c2) * s, (bx * c2 - cx * b2) * s, cr * s
    D = np.stack([xi * xi + yi * yi, xi, yi, np.ones(len(xi), dtype=np.int64)])
    full = np.zeros(len(ut), bool)
    for lo in range(0, len(ut), 1024):
        q = slice(lo, lo + 1024)
        # cr (|D|^2 - 2 A.D + |A|^2) - u . (D - A)
        coef = np.stack([cr[q], -2 * cr[q] * ax[q] - ux[q], -2 * cr[q] * ay[q] - uy[q],
                         cr[q] * (ax[q] * ax[q] + ay[q] * ay[q]) + ux[q] * ax[q] + uy[q] * ay[q]], axis=1)
        full[q] = ((coef @ D) < 0).any(axis=1)
    return full


def check(L, tri):
    """a code of REASON for every node, (ny, nx): tri (ny, nx, 3) holds the node's triangle or -1 where it is outside"""
    _, inside, _ = hull_masks(L.name)
    code = np.zeros(L.shape, dtype=np.int64)
    got = tri[..., 0] >= 0
    code[got != inside] = MASK
    jj, ii = np.nonzero(got & inside)
    if not len(jj):
        return code
    t = tri[jj, ii]
    px, py = L.gxi[ii], L.gyi[jj]
    c = np.zeros(len(jj), dtype=np.int64)

    def mark(bad, what):
        c[(c == OK) & bad] = what

    mark(~((t[:, 0] < t[:, 1]) & (t[:, 1] < t[:, 2])) | (t.min(axis=1) < 0) | (t.max(axis=1) >= L.n), ORDER)
    t = np.clip(t, 0, L.n - 1)
    ax, ay, bx, by, cx, cy = (v[t[:, k]] for k in range(3) for v in (L.xi, L.yi))
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    mark(area == 0, FLAT)
    s = np.sign(area)
    la = ((bx - px) * (cy - py) - (by - py) * (cx - px)) * s
    lb = ((cx - px) * (ay - py) - (cy - py) * (ax - px)) * s
    lc = ((ax - px) * (by - py) - (ay - py) * (bx - px)) * s
    mark((la < 0) | (lb < 0) | (lc < 0), MISSES)
    mark((lowest_at_position(L)[t] != t).any(axis=1), DUPLICATE)
    ut, back = np.unique(t, axis=0, return_inverse=True)  # the empty circle, once per distinct triangle
    mark(holds_a_ray(L.xi, L.yi, ut)[back.ravel()] & (area != 0), CIRCLE)
    code[jj, ii] = c
    return code


def ray_values(L, seed=5):
    """amplitude and phase numerators (integers over 2^VAL_BITS), unrelated from ray to ray: rays at one position differ"""
    rng = np.random.RandomState(seed)
    return rng.randint(512, 1536, L.n).astype(np.int64), rng.randint(-4096, 4097, L.n).astype(np.int64)


def affine_values(xi, yi):
    """numerators of an affine amplitude and phase with dyadic coefficients: exact at every ray and every node"""
    return (1 << 18) + 3 * xi - 2 * yi, -1000 + 5 * xi + 7 * yi


def interpolate(L, tri, num):
    """the barycentric interpolation of num / 2^VAL_BITS in each node's triangle, formed in integers and rounded once;
    0 where tri is -1"""
    out = np.zeros(L.shape)
    jj, ii = np.nonzero(tri[..., 0] >= 0)
    t = tri[jj, ii]
    px, py = L.gxi[ii], L.gyi[jj]
    ax, ay, bx, by, cx, cy = (v[t[:, k]] for k in range(3) for v in (L.xi - 0, L.yi - 0))
    la = (bx - px) * (cy - py) - (by - py) * (cx - px)
    lb = (cx - px) * (ay - py) - (cy - py) * (ax - px)
    lc = (ax - px) * (by - py) - (ay - py) * (bx - px)
    top = la * num[t[:, 0]] + lb * num[t[:, 1]] + lc * num[t[:, 2]]
    out[jj, ii] = top / ((la + lb + lc) << VAL_BITS)
    return out


def assert_close(a, ref, rel, what):
    scale = np.abs(ref).max()
    err = np.abs(a - ref).max()
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    assert err <= rel * scale, f"{what}: max |diff| {err:.3e} > {rel:g} * {scale:.3e}"


# ---------------------------------------------------------------- host: no GPU needed
@pytest.mark.parametrize("name", NAMES)
def test_layouts_are_exact(name):
    """coordinates are exactly origin + integer * unit in float64; with Dx, Dy the extents of rays and nodes together, every
    difference the kernel forms is an integer (in units) of at most Dx or Dy, a squared distance at most Dx^2 + Dy^2, a
    2 x 2 determinant at most 2 Dx Dy and an in-circle sum at most 6 Dx Dy (Dx^2 + Dy^2): below 2^53 each is exact in
    float64 (and in int64); so are the reference's interpolation sums"""
    L = LAYOUTS[name]
    assert L.unit == 2.0 ** round(np.log2(L.unit))
    for f, o, i in ((L.x, L.x0, L.xi), (L.y, L.y0, L.yi), (L.gx, L.x0, L.gxi), (L.gy, L.y0, L.gyi)):
        assert all(Fraction(v) == Fraction(o) + int(k) * Fraction(L.unit) for v, k in zip(f.tolist(), i.tolist()))
    Dx = int(max(L.xi.max(), L.gxi.max()) - min(L.xi.min(), L.gxi.min()))
    Dy = int(max(L.yi.max(), L.gyi.max()) - min(L.yi.min(), L.gyi.min()))
    assert 6 * Dx * Dy * (Dx * Dx + Dy * Dy) < 2 ** 53
    big = max(int(np.abs(v).max()) for pair in (ray_values(L), affine_values(L.xi, L.yi)) for v in pair)
    assert 6 * Dx * Dy * big < 2 ** 53 and (2 * Dx * Dy) << VAL_BITS < 2 ** 53
    # the checker's expanded in-circle form uses absolute integers
    m = int(max(np.abs(L.xi).max(), np.abs(L.yi).max()))
    assert 64 * max(Dx, Dy, m) ** 4 < 2 ** 63 or 16 * Dx * Dy * (Dx * Dx + Dy * Dy + 2 * m * m) < 2 ** 63


@pytest.mark.parametrize("name", NAMES)
def test_layouts_hold_their_claims(name):
    L = LAYOUTS[name]
    rays, positions, hull_size, n_inside, n_boundary, n_on_ray = CLAIMS[name]
    h, inside, on = hull_masks(name)
    assert L.n == rays
    assert len(set(zip(L.xi.tolist(), L.yi.tolist()))) == positions
    assert len(h) == hull_size
    if n_inside is not None:
        assert int(inside.sum()) == n_inside
    assert int(on.sum()) == n_boundary
    if n_on_ray is not None:
        rays_at = set(zip(L.xi.tolist(), L.yi.tolist()))
        assert sum((int(a), int(b)) in rays_at for b in L.gyi for a in L.gxi) == n_on_ray
    # index order and position order are unrelated
    assert L.n <= 4 or not np.array_equal(np.lexsort((L.xi, L.yi)), np.arange(L.n))


def test_layout_particulars():
    low = lowest_at_position(LAYOUTS["doubled"])
    assert np.array_equal(np.bincount(low, minlength=578)[np.unique(low)], np.full(289, 2))
    P = LAYOUTS["pile"]
    at = (P.xi == 20) & (P.yi == 36)
    assert at.sum() == 201 and (lowest_at_position(P)[at] == np.flatnonzero(at)[0]).all()
    for name in ("doubled", "pile"):  # rays at one position carry different values
        L = LAYOUTS[name]
        amp, ph = ray_values(L)
        low = lowest_at_position(L)
        other = low != np.arange(L.n)
        assert other.sum() >= 200 and (amp[other] != amp[low[other]]).mean() > 0.99 and (ph[other] != ph[low[other]]).mean() > 0.99
    for name in ("ring", "ring_centre", "ring_lattice"):
        L = LAYOUTS[name]
        assert int((L.xi ** 2 + L.yi ** 2 == 65 ** 2).sum()) == 36 and int((L.xi ** 2 + L.yi ** 2 > 65 ** 2).sum()) == 0
        h = strict_hull(L.xi, L.yi)  # the integer points of a lattice polygon's boundary: gcd(dx, dy) per edge
        assert sum(math.gcd(b[0] - a[0], b[1] - a[1]) for a, b in zip(h, h[1:] + h[:1])) == 140
    F = LAYOUTS["fan"]
    assert int((F.yi == 0).sum()) == 33 and len(strict_hull(F.xi, F.yi)) == 3
    gx, gy = set(F.gxi.tolist()), set(F.gyi.tolist())
    assert all(v in gx for v in (0, 64, 128)) and all(v in gy for v in (0, 48))  # the hull's vertices are nodes
    S = LAYOUTS["square4"]
    GX, GY = np.meshgrid(S.gxi, S.gyi)
    assert int(((GX == GY) & (GX >= 0) & (GX <= 8)).sum()) == 9 and int(((GX + GY == 8) & (GX >= 0) & (GX <= 8)).sum()) == 9
    O = LAYOUTS["offset"]
    assert O.x.min() == 1.0 and O.y.min() == -2.0 and np.unique(O.x)[1] - 1.0 == 2.0 ** -14


def index_at(L):
    low = lowest_at_position(L)
    return {(int(L.xi[k]), int(L.yi[k])): int(k) for k in np.unique(low)}


def one_node(L, node, corners, at=None):
    """a tri array that is -1 everywhere but at `node` (integer coordinates), where it holds the rays at `corners`"""
    at = at or index_at(L)
    tri = np.full(L.shape + (3,), -1, dtype=np.int64)
    i, j = int(np.flatnonzero(L.gxi == node[0])[0]), int(np.flatnonzero(L.gyi == node[1])[0])
    tri[j, i] = sorted(at[c] for c in corners)
    return tri, (j, i)


def test_checker_rejects_wrong_answers():
    L = LAYOUTS["lattice17"]
    node = (5, 6)  # in the cell (4..8)^2, above its diagonal
    for corners, want in ((((4, 4), (8, 8), (4, 8)), OK), (((4, 4), (8, 4), (4, 8)), OK),  # either diagonal: co-circular
                          (((4, 4), (8, 4), (8, 8)), MISSES),
                          (((0, 0), (16, 0), (0, 16)), CIRCLE),
                          (((4, 8), (4, 4), (12, 8)), CIRCLE),
                          (((4, 4), (8, 8), (12, 12)), FLAT)):
        tri, q = one_node(L, node, corners)
        assert check(L, tri)[q] == want, (corners, REASON[check(L, tri)[q]])
    for at_node, corners in (((4, 6), ((4, 4), (4, 8), (8, 8))), ((4, 6), ((4, 4), (4, 8), (0, 4))),  # on an edge: either neighbour
                          ((6, 6), ((4, 4), (8, 8), (4, 8))), ((8, 8), ((4, 4), (8, 8), (4, 8))),  # on a diagonal, on a ray
                          ((0, 0), ((0, 0), (4, 0), (0, 4))), ((2, 0), ((0, 0), (4, 0), (4, 4)))):  # hull corner, hull edge
        tri, q = one_node(L, at_node, corners)
        assert check(L, tri)[q] == OK, (at_node, corners)
    tri, q = one_node(L, node, ((4, 4), (8, 8), (4, 8)))
    code = check(L, tri)
    assert code[q] == OK and (code[hull_masks(L.name)[1]] == MASK).sum() == 65 * 65 - 1  # inside nodes marked outside
    tri, q = one_node(L, (-4, -4), ((0, 0), (4, 0), (0, 4)))
    assert check(L, tri)[q] == MASK  # an outside node given a triangle
    tri, q = one_node(L, node, ((4, 4), (8, 8), (4, 8)))
    tri[q] = tri[q][[1, 0, 2]]
    assert check(L, tri)[q] == ORDER
    tri[q] = tri[q][[0, 0, 2]]
    assert check(L, tri)[q] == ORDER
    # a duplicate that is not the lowest index at its position
    L = LAYOUTS["doubled"]
    at = index_at(L)
    tri, q = one_node(L, node, ((4, 4), (8, 8), (4, 8)), at)
    assert check(L, tri)[q] == OK
    twin = [k for k in np.flatnonzero((L.xi == 8) & (L.yi == 8)) if k != at[(8, 8)]][0]
    tri[q] = sorted([at[(4, 4)], at[(4, 8)], int(twin)])
    assert check(L, tri)[q] == DUPLICATE
    # the ring: any three of the co-circular rays around the node pass; with the centre added the same triangle fails
    L = LAYOUTS["ring"]
    tri, q = one_node(L, (1, 2), ((65, 0), (-33, 56), (-16, -63)))
    assert check(L, tri)[q] == OK
    assert check(LAYOUTS["ring_centre"], one_node(LAYOUTS["ring_centre"], (1, 2), ((65, 0), (-33, 56), (-16, -63)))[0])[q] == CIRCLE


def test_checker_in_circle_form_equals_the_determinant():
    """the expanded form holds_a_ray() evaluates against the 3 x 3 in-circle determinant in Python integers, on the layout
    with the largest coordinates"""
    L = LAYOUTS["far_corners"]
    rng = np.random.RandomState(3)
    seen = set()
    for _ in range(400):
        k = rng.choice(L.n, 4, replace=False)
        k[3] = k[3] if rng.randint(2) else L.n - 1 - rng.randint(4)  # often one of the far corners
        (ax, ay), (bx, by), (cx, cy), (dx, dy) = ((int(L.xi[i]), int(L.yi[i])) for i in k)
        area = cross((ax, ay), (bx, by), (cx, cy))
        if area == 0 or len(set(k.tolist())) < 4:
            continue
        ax, ay, bx, by, cx, cy = ax - dx, ay - dy, bx - dx, by - dy, cx - dx, cy - dy
        det = ((ax * ax + ay * ay) * (bx * cy - cx * by) + (bx * bx + by * by) * (cx * ay - ax * cy)
               + (cx * cx + cy * cy) * (ax * by - bx * ay))
        inside = det * area > 0
        seen.add(inside)
        assert bool(holds_a_ray(L.xi[k], L.yi[k], np.array([[0, 1, 2]]))[0]) == inside, k
    assert seen == {True, False}


@pytest.mark.parametrize("name", ["lattice17", "fan"])
def test_scipy_fills_the_closed_hull(name):
    """"on the hull is inside" is scipy's behaviour, and so the reference's: LinearNDInterpolator(..., fill_value=0) has a
    value at exactly the nodes of the closed hull; its triangles pass check(), and the affine field is reproduced"""
    interp = pytest.importorskip("scipy.interpolate")
    spatial = pytest.importorskip("scipy.spatial")
    L = LAYOUTS[name]
    _, inside, on = hull_masks(name)
    GX, GY = np.meshgrid(L.gxi, L.gyi)
    pts = np.c_[L.xi, L.yi].astype(float)
    v = interp.LinearNDInterpolator(pts, np.ones(L.n), fill_value=0.0)((GX.astype(float), GY.astype(float)))
    assert np.array_equal(v != 0.0, inside) and on.sum() > 100
    d = spatial.Delaunay(pts)
    s = d.find_simplex(np.c_[GX.ravel(), GY.ravel()].astype(float)).reshape(GX.shape)
    tri = np.where((s >= 0)[..., None], np.sort(d.simplices[s], axis=-1), -1).astype(np.int64)
    assert not check(L, tri).any()
    num = affine_values(L.xi, L.yi)[0]
    assert_close(interpolate(L, tri, num), np.where(inside, affine_values(GX, GY)[0] / 2.0 ** VAL_BITS, 0.0), 1e-15, name)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    from synthpy_amd import engine

    engine.init(0)
    return engine


@pytest.fixture(scope="module")
def gridded(dev):
    """grid_rays of a layout with the unrelated ray values, once per module: (amplitude, phase, triangles, stats)"""
    @functools.lru_cache(maxsize=None)
    def run(name):
        L = LAYOUTS[name]
        amp, ph = ray_values(L)
        out = fi.grid_rays(L.gx, L.gy, L.jones(), amp / 2.0 ** VAL_BITS, ph / 2.0 ** VAL_BITS, return_triangles=True)
        for a in out[:3]:
            a.setflags(write=False)
        return out
    return run


def grid_affine(L):
    amp, ph = affine_values(L.xi, L.yi)
    return fi.grid_rays(L.gx, L.gy, L.jones(), amp / 2.0 ** VAL_BITS, ph / 2.0 ** VAL_BITS, return_triangles=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_inside_is_the_closed_hull(gridded, name):
    """a node gets a triangle exactly where it lies in the closed hull of the rays, its boundary and vertices included"""
    h, inside, on = hull_masks(name)
    a, p, tri, stats = gridded(name)
    got = tri[..., 0] >= 0
    wrong = np.argwhere(got != inside)
    assert not len(wrong), (f"{name}: {len(wrong)} nodes of {inside.size} differ, {int((on & ~got).sum())} of them among the "
                            f"{int(on.sum())} on the hull's boundary; first (row, column): {wrong[:5].tolist()}")
    assert np.array_equal(tri[..., 1] >= 0, got) and np.array_equal(tri[..., 2] >= 0, got)
    assert stats.outside == int((~inside).sum())
    assert stats.hull_vertices == len(h)
    if name in LINES:
        assert stats.outside == inside.size and stats.hull_vertices == 0 and (tri == -1).all() and not a.any() and not p.any()
    if name == "far_corners":
        assert stats.second_pass > 0, stats
    if name == "lattice64":
        assert stats.bins_x * stats.bins_y > 1300 and 200 <= stats.filter_survivors <= 300, stats
    if name in ("strip", "strip_t"):
        assert max(stats.bins_x, stats.bins_y) > 300 and min(stats.bins_x, stats.bins_y) == 1, stats


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_every_triangle_is_a_delaunay_triangle_that_holds_its_node(gridded, name):
    """at every node that got a triangle: distinct ascending indices, not collinear, the node in the closed triangle, no ray
    strictly inside the circumcircle, every vertex the lowest index at its position.  Exact, every node, every ray."""
    L = LAYOUTS[name]
    tri = gridded(name)[2]
    code = check(L, tri)
    code[code == MASK] = OK  # test_inside_is_the_closed_hull's subject
    bad = np.argwhere(code != OK)
    assert not len(bad), (f"{name}: {len(bad)} nodes; first (row, column, triangle, why): "
                          f"{[(int(j), int(i), tri[j, i].tolist(), REASON[code[j, i]]) for j, i in bad[:5]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_values_are_the_triangles_interpolation(gridded, name):
    L = LAYOUTS[name]
    a, p, tri, stats = gridded(name)
    amp, ph = ray_values(L)
    outside = tri[..., 0] < 0
    assert np.all(a[outside] == 0.0) and np.all(p[outside] == 0.0)
    if name in LINES:
        return
    assert_close(a, interpolate(L, tri, amp), 1e-12, f"{name} amplitude")
    assert_close(p, interpolate(L, tri, ph), 1e-12, f"{name} phase")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_affine_field_is_reproduced_whatever_the_triangle(dev, name):
    """linear interpolation reproduces an affine function in any triangle: the one statement that does not depend on the
    triangulation, so it is scipy's interpolant too.  Rays at one position carry the same value here.  Also: another order
    of the ray indices changes neither the inside mask nor these values, and a second call returns identical arrays."""
    L = LAYOUTS[name]
    _, inside, _ = hull_masks(name)
    GX, GY = np.meshgrid(L.gxi, L.gyi)
    want = [np.where(inside, v / 2.0 ** VAL_BITS, 0.0) for v in affine_values(GX, GY)]
    a, p, tri, stats = grid_affine(L)
    again = grid_affine(L)
    for u, w in zip((a, p, tri), again[:3]):
        assert np.array_equal(u, w)
    assert again[3] == stats
    other, perm = L.reshuffled(77)
    a2, p2, tri2, _ = grid_affine(other)
    assert np.array_equal(tri2[..., 0] >= 0, tri[..., 0] >= 0), f"{name}: the inside mask depends on the ray order"
    for got, what in ((a, "amplitude"), (p, "phase"), (a2, "amplitude, reshuffled"), (p2, "phase, reshuffled")):
        ref = want[0] if what.startswith("amp") else want[1]
        assert np.all(got[~inside] == 0.0)
        if name not in LINES:
            assert_close(np.where(inside, got, 0.0), ref, 1e-12, f"{name} {what}")
    if name in ("lattice17", "fan", "ring_lattice"):
        interp = pytest.importorskip("scipy.interpolate")
        pts = np.c_[L.xi, L.yi].astype(float)
        for got, num in ((a, affine_values(L.xi, L.yi)[0]), (p, affine_values(L.xi, L.yi)[1])):
            ref = interp.LinearNDInterpolator(pts, num / 2.0 ** VAL_BITS, fill_value=0.0)((GX.astype(float), GY.astype(float)))
            assert_close(np.where(inside, got, 0.0), np.where(inside, ref, 0.0), 1e-12, f"{name} against scipy")


@pytest.mark.gpu
def test_propagate_of_a_lattice_beam_keeps_its_border(dev, gridded):
    """propagate on lattice17 over a grid equal to the lattice's extent: the one-call path equals fresnel_propagate of the
    prepared field built from the exact gridding, and the border row and column are not zeroed"""
    L = LAYOUTS["lattice17"]
    amp, ph = ray_values(L)
    q = np.arange(0, 65)
    G = Layout("lattice17", np.c_[L.xi, L.yi], q, q, 0)
    G.xi, G.yi = L.xi, L.yi
    a, p, tri, stats = fi.grid_rays(G.gx, G.gy, G.jones(), amp / 2.0 ** VAL_BITS, ph / 2.0 ** VAL_BITS, return_triangles=True)
    assert (tri[..., 0] >= 0).all() and stats.outside == 0
    ea, ep = interpolate(G, tri, amp), interpolate(G, tri, ph)
    U0 = ea * np.exp(-1j * ep)
    border = np.r_[U0[0], U0[-1], U0[:, 0], U0[:, -1]]
    assert np.abs(border).min() >= 0.5
    ext = float(G.gx[-1] - G.gx[0])
    ref = fi.fresnel_propagate(fi.prepare_field_for_propagation(U0), (ext, ext), LWL, Z, U0.shape)
    out = fi.propagate(LWL, G.gx, G.gy, ext, ext, G.jones(), amp / 2.0 ** VAL_BITS, ph / 2.0 ** VAL_BITS, Z)
    assert out.dtype == np.complex128 and out.shape == (65, 65)
    assert_close(out, ref, 1e-10, "propagate on lattice17")
