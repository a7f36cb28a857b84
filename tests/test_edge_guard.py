"""The exact-counts edge guard on inputs that stress it (needs an MI355X: run with -m gpu).

The default counts path traces with the mixed build (k_trace_mx: float32 stage arithmetic) and the deposit traces again in
float64 every ray whose pixel or mask decision could differ from the float64 build's within the per-ray bound the mixed
kernel writes (trace_mx.inc, header; deposit.hip, apply_chain).  Two things are checked here, away from the comfortable
inputs of test_gpu_parity.py::test_edge_guard_bound_holds (divergent beams through smooth or turbulent fields):

* the bound itself, GPU against GPU: the same uploaded bundle traced with precision "f64" and "mixed"; on every finite ray
  |d angle| <= bound and |d position| <= guard_len * bound (sr_rays.guard_len: the volume's length plus the distance from its
  last node plane to the plane `extent`), a bound of 0 meaning no difference at all.  The volumes are chosen where the
  float32 blend rounds relative to the cell's corner values while the interpolated lateral field is small: collimated beams
  (no entry term) near the symmetry planes of a blob, fields that vary along one lateral axis only, white noise per node, a
  sharp step, stretched grids on every probing axis, rays entering through the lateral faces;
* the guard's contract: the image of the default path equals the image of the float64 GPU trace of the same s0, bit for
  bit, for every counts chain of the two APIs (focal_plane != 0, light field, knife edges on both axes and both directions,
  OP_SCALE), at bin_scale 1 and 10, through single deposits and through one sr_rays_refine call of four diagnostics.
"""
import functools

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

EXT, LWL = 5e-3, 1064e-9
L = 400.0


@pytest.fixture(scope="module")
def eng():
    from synthpy_amd import engine

    engine.init(0)
    return engine


# ---------------------------------------------------------------- volumes and beams
def _collimated(p1, p2, pd="z"):
    """s0 of rays along the probing axis (divergence 0: no entry term in the bound) at lateral positions (p1, p2)."""
    from synthpy_amd import _beam

    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    return _beam.assemble(p1, p2, np.zeros(p1.size), np.zeros(p1.size), EXT, pd)


def _near(x0, h, rng, spread):
    """Offsets from x0 of h/100 ... h/4 (both signs), and for each a second coordinate drawn from +-spread."""
    d = h * np.geomspace(1e-2, 0.25, 16)
    d = np.concatenate([d, -d])
    return x0 + np.repeat(d, 64), rng.uniform(-spread, spread, d.size * 64)


def _near_both(x0, y0, h):
    """Every pair of offsets h/100 ... h/4 (both signs) from (x0, y0)."""
    d = h * np.geomspace(1e-2, 0.25, 16)
    d = np.concatenate([d, -d])
    a, b = np.meshgrid(d, d, indexing="ij")
    return x0 + a.ravel(), y0 + b.ravel()


def _blob64():
    """The C1 blob on 64^3 nodes (even: the symmetry planes x = 0, y = 0 lie in the middle of a cell), a collimated beam,
    rays within h/100 ... h/4 of either plane and of both."""
    rng = np.random.default_rng(101)
    x = np.linspace(-EXT, EXT, 64)
    h = float(x[1] - x[0])
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij", sparse=True)
    ne = 1e25 * np.exp(-(X ** 2 + Y ** 2 + Z ** 2) / (1.5e-3) ** 2)
    ax, ay = _near(0.0, h, rng, 4e-3)
    bx, by = _near(0.0, h, rng, 4e-3)
    cx, cy = _near_both(0.0, 0.0, h)
    ux, uy = rng.uniform(-4e-3, 4e-3, (2, 40_000))
    s0 = _collimated(np.concatenate([ax, by, cx, ux]), np.concatenate([ay, bx, cy, uy]))
    return ne, (x, x, x), "z", s0


def _cos(axis):
    """n_e = 1e25 (1 + 0.5 cos(2 pi q / lam)) along ONE lateral axis q (x: axis 0, y: axis 1), 5.3 cells per period (the
    zero crossings of the node gradient fall inside cells); a collimated beam, rays within h/100 ... h/4 of every crossing
    of the interpolated gradient."""
    rng = np.random.default_rng(202 + axis)
    x = np.linspace(-EXT, EXT, 64)
    h = float(x[1] - x[0])
    prof = 1.0 + 0.5 * np.cos(2 * np.pi * (x - 0.3 * h) / (5.3 * h))
    shape = [1, 1, 1]
    shape[axis] = 64
    ne = 1e25 * np.broadcast_to(prof.reshape(shape), (64, 64, 64)).copy()
    # node gradient (the sign is that of -d prof / dq whatever the factor): the crossings of its linear interpolation
    g = np.gradient(prof, x)
    i = np.nonzero((np.sign(g[:-1]) * np.sign(g[1:]) < 0) & (np.abs(x[:-1]) < 4e-3))[0]
    xs = x[i] + h * g[i] / (g[i] - g[i + 1])
    q, o = [], []
    for x0 in xs:
        a, b = _near(x0, h, rng, 4e-3)
        q.append(a[::4])
        o.append(b[::4])
    ux, uy = rng.uniform(-4e-3, 4e-3, (2, 40_000))
    q, o = np.concatenate(q + [ux]), np.concatenate(o + [uy])
    s0 = _collimated(q, o) if axis == 0 else _collimated(o, q)
    return ne, (x, x, x), "z", s0


def _noise():
    """Zero-mean white noise per node on 64^3 (the gradient changes sign from node to node), a collimated beam."""
    rng = np.random.default_rng(303)
    x = np.linspace(-EXT, EXT, 64)
    ne = 1e25 * (1.0 + 0.05 * rng.standard_normal((64, 64, 64)))
    p = rng.uniform(-4e-3, 4e-3, (2, 60_000))
    return ne, (x, x, x), "z", _collimated(p[0], p[1])


def _slab():
    """The reference's slab / step fixture (a sharp interface): its 128 rays and a collimated beam over the cross-section."""
    g = golden("g2_trace_slab16_z_s0")
    x = g["x"]
    rng = np.random.default_rng(404)
    p = rng.uniform(0.95 * x[0], 0.95 * x[-1], (2, 60_000))
    return g["ne"], (x, x, x), "z", np.concatenate([g["s0"], _collimated(p[0], p[1])], axis=1)


def _stretched(pd):
    """test_non_uniform_grid_vs_oracle's stretched grid (cell widths varying by up to 60 %, guard_h6 = the largest h/6) and
    field, probed along pd with a collimated beam and a slightly divergent one."""
    from synthpy_amd import _beam

    rng = np.random.default_rng(12)
    n = (30, 26, 34)
    axes = []
    for m in n:
        w = 1.0 + 0.6 * rng.random(m - 1)
        c = np.concatenate([[0.0], np.cumsum(w)])
        axes.append((2 * c / c[-1] - 1) * EXT)
    X, Y, Z = np.meshgrid(*axes, indexing="ij", sparse=True)
    ne = 1e25 * np.exp(-(X ** 2 + 1.3 * Y ** 2 + 0.8 * Z ** 2) / (2e-3) ** 2) * (1 + 0.2 * np.sin(3e3 * X + 2e3 * Y) * np.cos(2.5e3 * Z))
    rng = np.random.default_rng(505)
    p = rng.uniform(-3.5e-3, 3.5e-3, (2, 40_000))
    s_col = _collimated(p[0], p[1], pd)
    q = rng.uniform(-3.5e-3, 3.5e-3, (2, 20_000))
    s_div = _beam.assemble(q[0], q[1], 1e-3 * rng.standard_normal(q.shape[1]), np.pi * rng.random(q.shape[1]), EXT, pd)
    return ne, tuple(axes), pd, np.concatenate([s_col, s_div], axis=1)


def _overfill():
    """test_rays_crossing_lateral_faces's overfilling square beam (+-7.5 mm on a +-5 mm volume, 0.08 rad): rays that enter
    and leave through the lateral faces, and rays in the virtual cells outside the volume; with it a collimated overfilling
    beam (rays that never enter) and a mildly divergent one (2e-3 rad: rays that graze the faces)."""
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    g = golden("g2_trace_blob32_z_s0")
    x = g["x"]
    np.random.seed(11)
    s0 = [init_beam(6000, 1.5 * EXT, 0.08, EXT, "square", "z"), init_beam(20_000, 1.5 * EXT, 2e-3, EXT, "square", "z")]
    p = np.random.default_rng(606).uniform(-1.5 * EXT, 1.5 * EXT, (2, 20_000))
    s0.append(_collimated(p[0], p[1]))
    return g["ne"], (x, x, x), "z", np.concatenate(s0, axis=1)


CASES = {
    "blob64 collimated, near x=0 / y=0": _blob64,
    "cos along x": functools.partial(_cos, 0),
    "cos along y": functools.partial(_cos, 1),
    "white noise 64^3": _noise,
    "slab16 step": _slab,
    "stretched grid, z": functools.partial(_stretched, "z"),
    "stretched grid, x": functools.partial(_stretched, "x"),
    "stretched grid, y": functools.partial(_stretched, "y"),
    "overfilling, lateral faces": _overfill,
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


def _volume(eng, ne, axes, pd):
    vol = eng.Volume.from_ne(ne, *axes, LWL, pd)
    assert eng.resolve_precision("auto", vol) == "mixed"
    return vol


def _guard_len(axes, pd):
    """sr_rays.guard_len as the trace forms it (trace.hip): the volume's length along the probing axis plus the distance from
    its last node plane to the plane `extent`."""
    g = np.asarray(axes["xyz".index(pd)], np.float64)
    return float(g[-1] - g[0]) + abs(EXT - float(g[-1]))


# ---------------------------------------------------------------- 1. the bound, GPU against GPU
@pytest.mark.parametrize("name", list(CASES))
def test_mixed_error_within_its_bound(eng, name):
    """On every finite ray: |d angle| <= bound and |d position| <= guard_len * bound between the mixed and the float64
    build of the same bundle; a ray whose bound is 0 differs by nothing.  Prints the worst ratios."""
    ne, axes, pd, s0 = _case(name)
    vol = _volume(eng, ne, axes, pd)
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    t_end = eng.default_t_end(EXT)
    rays.trace(vol, t_end, EXT, precision="f64")
    _, r64, _ = rays.download(sf=False, Jf=False)
    r64 = np.array(r64)
    assert not rays.error_bound().any()
    rays.trace(vol, t_end, EXT, precision="mixed")
    _, rmx, _ = rays.download(sf=False, Jf=False)
    b = rays.error_bound().astype(np.float64)
    fin = np.isfinite(rmx).all(axis=0)
    assert np.array_equal(fin, np.isfinite(r64).all(axis=0)), "a ray finite in one build only"
    assert fin.sum() > 0.9 * fin.size and np.all(b[fin] >= 0)
    d_ang = np.maximum(np.abs(rmx[1] - r64[1]), np.abs(rmx[3] - r64[3]))[fin]
    d_pos = np.maximum(np.abs(rmx[0] - r64[0]), np.abs(rmx[2] - r64[2]))[fin]
    bb, gl = b[fin], _guard_len(axes, pd)
    pos = bb > 0
    ra, rp = d_ang[pos] / bb[pos], d_pos[pos] / (gl * bb[pos])
    print(f"{name}: {fin.sum()} rays, {int((~pos).sum())} with bound 0; max |d angle| / bound {ra.max():.3f}, "
          f"max |d pos| / (guard_len * bound) {rp.max():.3f}; rays beyond: {int((ra > 1).sum())} / {int((rp > 1).sum())}; "
          f"median bound {np.median(bb[pos]):.2e} rad")
    assert not np.any(d_ang[~pos]) and not np.any(d_pos[~pos]), "a ray with bound 0 differs from the float64 build"
    assert np.all(d_ang <= bb), (name, float(ra.max()), int((ra > 1).sum()))
    assert np.all(d_pos <= gl * bb), (name, float(rp.max()), int((rp > 1).sum()))


def test_mixed_build_never_runs_the_tile_path(eng, monkeypatch):
    """k_trace_mx's recovery branch (A.recover: the error sum carried in guard[] from segment to segment) belonged to the
    mixed tile kernel, which is gone: sr_rays_trace launches the mixed build per ray (launch_mx) before it looks at the tile
    plan, and no launch sets `recover`.  So the branch cannot run and no segment hand-off of the bound can be tested; this
    pins down that a dense bundle traced "mixed", with the tile path forced on, still takes the per-ray kernel and gets the
    same bound."""
    import bench

    ne, x = bench.make_volume(64)
    s0 = bench.make_rays(100_000, EXT, 3)
    vol = eng.Volume.from_ne(ne, x, x, x, LWL, "z")
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    rays.trace(vol, eng.default_t_end(EXT), EXT, precision="mixed")
    assert rays.tile_segments == 0
    b0, r0 = rays.error_bound(), np.array(rays.download(sf=False, Jf=False)[1])
    monkeypatch.setenv("SYNTHRAY_F64_TILE", "1")
    rays.trace(vol, eng.default_t_end(EXT), EXT, precision="mixed")
    assert rays.tile_segments == 0
    assert np.array_equal(rays.error_bound(), b0) and np.array_equal(rays.download(sf=False, Jf=False)[1], r0, equal_nan=True)
    assert (b0 > 0).mean() > 0.99


# ---------------------------------------------------------------- 2. the guard's contract: images
def _knife(offset, axis, direction):
    """A knife edge as simulator/diagnostics.py's knife_edge builds it."""
    from synthpy_amd.engine import OP_KNIFE

    return (OP_KNIFE, offset, direction, 0 if axis == "x" else 2)


def _chains(eng):
    """Every counts chain of the two APIs, each also with focal_plane != 0, and chains with knife edges (x and y, both
    directions, in the schlieren focal plane) and with OP_SCALE (inside the chain and just before the detector)."""
    fp = 7.5
    knife_head = [(eng.OP_DIST, L), (eng.OP_CIRC_AP, 25.0), (eng.OP_LENS, L, L), (eng.OP_DIST, L)]
    knife_tail = [(eng.OP_DIST, L), (eng.OP_CIRC_AP, 25.0), (eng.OP_LENS, L, L), (eng.OP_DIST, L)]
    ch = {
        "shadow single": eng.chain_shadow_single(),
        "shadow single fp": eng.chain_shadow_single(focal_plane=fp),
        "shadow two": eng.chain_shadow_two(),
        "shadow two fp": eng.chain_shadow_two(focal_plane=-fp),
        "shadow exp": eng.chain_shadow_exp(),
        "shadow exp detL": eng.chain_shadow_exp(detL=300.0),
        "schlieren DF": eng.chain_schlieren(),
        "schlieren DF fp": eng.chain_schlieren(focal_plane=fp),
        "schlieren LF": eng.chain_schlieren(dark_field=False),
        "schlieren LF fp": eng.chain_schlieren(focal_plane=fp, dark_field=False),
        "refractometry": eng.chain_refractometry(),
        "refractometry fp": eng.chain_refractometry(focal_plane=fp),
        "shadow single, scale 2.5 at the detector": eng.chain_shadow_single() + [(eng.OP_SCALE, 2.5)],
        "shadow two, scale 0.5 inside": [(eng.OP_SCALE, 0.5)] + eng.chain_shadow_two()[:4] + [(eng.OP_SCALE, 2.0)] + eng.chain_shadow_two()[4:],
    }
    for axis in ("x", "y"):
        for direction in (1, -1):
            ch[f"knife {axis} {'+' if direction > 0 else '-'}"] = knife_head + [_knife(0.002 * direction, axis, direction)] + knife_tail
    return ch


def _images(eng, rays, chains, img, **kw):
    out, again = {}, 0
    for name, ops in chains.items():
        img.zero()
        rays.deposit(img, ops, **kw)
        out[name] = img.download()
        again += rays.retraced
    return out, again


# the smooth volumes, where the existing counts tests' rule holds: the float64 GPU build's image is the oracle's from s0
ORACLE_CASES = ("blob64 collimated, near x=0 / y=0", "cos along x", "cos along y", "stretched grid, z")


@pytest.mark.parametrize("name", list(CASES))
def test_default_counts_equal_f64_images(eng, orc, name):
    """image(default path: mixed trace + edge guard) == image(float64 GPU trace of the same s0), bit for bit, for every
    chain, at bin_scale 1 and 10; on the smooth volumes also == the oracle's image from s0.  Prints how many rays the guard
    traced again (no cap on these inputs)."""
    ne, axes, pd, s0 = _case(name)
    N = s0.shape[1]
    assert N <= 200_000
    vol = _volume(eng, ne, axes, pd)
    rays = eng.RayBundle(N).upload(s0)
    t_end = eng.default_t_end(EXT)
    chains = _chains(eng)
    ro = None
    if name in ORACLE_CASES:
        dom = orc.Domain.from_ne(ne, *axes, LWL)
        dt = float(np.float32(axes[2])[1] - np.float32(axes[2])[0]) / orc.c
        so, _ = orc.trace_rk4(dom, s0, dt, orc.default_t_end(EXT), pd, "planes", 1)
        ro, _ = orc.ray_to_jones(so, EXT, pd)
    for bs in (1, 10):
        img = eng.DetectorImage.counts(bin_scale=bs)
        rays.trace(vol, t_end, EXT, precision="f64")
        ref, _ = _images(eng, rays, chains, img)
        rays.trace(vol, t_end, EXT)
        got, again = _images(eng, rays, chains, img)
        bad = [(c, int(np.abs(got[c].astype(np.int64) - ref[c].astype(np.int64)).sum())) for c in chains if not np.array_equal(got[c], ref[c])]
        print(f"{name}, bin_scale {bs}: {again} rays traced again over {len(chains)} chains ({100.0 * again / (N * len(chains)):.3f} % per chain)")
        assert not bad, (name, bs, bad)
        assert sum(int(H.sum()) for H in ref.values()) > 0
        if ro is not None:
            for c, ops in chains.items():
                r_o, _ = orc.optics(orc.m_to_mm(ro), ops)
                assert np.array_equal(ref[c], orc.histogram(r_o, bin_scale=bs).astype(np.uint32)), (name, bs, c)
        img.close()


def _refine_four(eng, vol, s0, cap):
    """One sr_rays_refine of four diagnostics (a knife chain among them), then deposits without the guard: the images of
    single exact-counts deposits and of the float64 trace."""
    ch = _chains(eng)
    names = ["shadow two", "schlieren DF fp", "refractometry", "knife y -"]
    N = s0.shape[1]
    rays = eng.RayBundle(N).upload(s0)
    t_end = eng.default_t_end(EXT)
    rays.trace(vol, t_end, EXT, precision="f64")
    ref = {}
    for c in names:
        im = eng.DetectorImage.counts()
        rays.deposit(im, ch[c])
        ref[c] = im.download()
    rays.trace(vol, t_end, EXT)
    single = 0
    for c in names:
        im = eng.DetectorImage.counts()
        rays.deposit(im, ch[c])
        assert np.array_equal(im.download(), ref[c]), c
        if cap:
            assert rays.retraced <= 0.05 * N, (c, rays.retraced)
        single += rays.retraced
    rays.trace(vol, t_end, EXT)
    imgs = [eng.DetectorImage.counts() for _ in names]
    n_all = rays.refine([(im, ch[c]) for im, c in zip(imgs, names)])
    assert n_all <= single and (n_all > 0 or single == 0)
    for im, c in zip(imgs, names):
        rays.deposit(im, ch[c], exact_counts=False)
        assert np.array_equal(im.download(), ref[c]), c
    return n_all, single


def test_refine_four_diagnostics_with_a_knife(eng):
    """sr_rays_refine with SR_MAX_REFINE (4) diagnostics in one call, a knife chain among them, followed by deposits with
    exact_counts=False: the images of the float64 trace.  On BASELINE's turbulence (2e5 rays of C2's 256^3) every single
    exact-counts deposit keeps the cap of 5 % re-traced rays; on the collimated blob the count is printed."""
    import bench

    ne, x = bench.make_volume(256)
    s0 = bench.make_rays(200_000, EXT, 0)
    n_all, single = _refine_four(eng, _volume(eng, ne, (x, x, x), "z"), s0, cap=True)
    print(f"turbulence 256^3: one refine traced {n_all} rays again, the four single deposits {single}")
    ne, axes, pd, s0 = _case("blob64 collimated, near x=0 / y=0")
    n_all, single = _refine_four(eng, _volume(eng, ne, axes, pd), s0, cap=False)
    print(f"blob64 collimated: one refine traced {n_all} rays again, the four single deposits {single}")
