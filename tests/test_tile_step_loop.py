"""The records kernel's step loop (k_trace_tile<., false, true>, trace_tile.inc) keeps its addresses as running values: five
slot byte addresses rotated in scalar registers, one LDS byte offset per ray for its cell, a running HBM pointer for the
LDS-DMA of node plane k + 2 and a running pointer into the step table.  An address that is wrong by one slot, one column or
one plane reads another record: the result differs from k_trace_f64's, which forms every address from scratch.  So every
test here compares sf, rf, Jf bit for bit (NaN for NaN) and ray_steps between the records kernel forced
(SYNTHRAY_F64_TILE=1, tile_records asserted) and the per-ray kernel (SYNTHRAY_F64_TILE=0), on the smallest shapes at which
an address can go wrong: a 24 x 40 x 33 node grid (non-cubic: the bytes per tile column, 23 * 128, and per node plane,
39 * 23 * 128, cannot be swapped unnoticed; the lateral grid is wider than a tile on both axes).  Needs an MI355X: -m gpu.
"""
import math
import os

import numpy as np
import pytest

LWL = 1064e-9
N_NODES = (24, 40, 33)  # x, y, z; probing along z: 33 node planes = 32 steps, 23 x 39 lateral cells
STEPS = N_NODES[2] - 1


@pytest.fixture(scope="module")
def eng():
    from synthpy_amd import engine

    engine.init(0)
    return engine


def _grid():
    half = [0.5 * (n - 1) * 1e-4 * f for n, f in zip(N_NODES, (0.9, 1.0, 1.1))]
    axes = tuple(np.linspace(-h, h, n) for h, n in zip(half, N_NODES))
    X, Y, Z = np.meshgrid(*axes, indexing="ij", sparse=True)
    w = [0.45 * h for h in half]
    r2 = ((X - 0.06 * half[0]) / w[0]) ** 2 + ((Y + 0.04 * half[1]) / w[1]) ** 2 + (Z / w[2]) ** 2
    ne = 1e25 * np.exp(-r2) * (1.0 + 0.1 * np.sin(2.6 * X / w[0] + 1.7 * Y / w[1]) * np.cos(2.1 * Z / w[2]))
    return axes, half, ne


def _beam(n, fill, div, half, seed):
    """A square beam over `fill` times the lateral faces, started before the first node plane."""
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    np.random.seed(seed)
    s0 = init_beam(n, 1.0, div, half[2] * 1.01, "square", "z")
    s0[0] *= fill * half[0]
    s0[1] *= fill * half[1]
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


@pytest.fixture(scope="module")
def case(eng):
    """The grid, its two volumes (with and without the phase integral), the two bundles and the per-ray kernel's results: formed
    once, shared by the tests, never changed."""
    axes, half, ne = _grid()
    ext = half[2] * 1.01
    beams = {"collimated": _beam(30_011, 0.8, 5e-5, half, 7), "overfill": _beam(20_003, 1.3, 2e-2, half, 8)}
    beams["overfill"][:, 1:6] = np.nan  # NaN rays and a ray flying backwards: not plane-form rays
    beams["overfill"][5, 9] *= -1
    vols = {ph: eng.Volume.from_ne(ne, *axes, LWL, "z", phaseshift=ph) for ph in (True, False)}
    ref = {}
    for ph, vol in vols.items():
        for tag, s0 in beams.items():
            out, st, info = _trace(eng, vol, s0, ext, SYNTHRAY_F64_TILE="0")
            assert info[0] == 0
            ref[ph, tag] = (out, st.ray_steps)
    yield {"axes": axes, "half": half, "ne": ne, "ext": ext, "beams": beams, "vols": vols, "ref": ref}
    for vol in vols.values():
        vol.close()


def _cuts(steps, seg, weights):
    """The library's segment boundaries (trace.hip, tile_cuts): ceil(steps / seg) segments; their shares are `weights` when there
    is one per segment, else a ramp from 1.3 down to 0.7."""
    n_seg = -(-steps // seg)
    w = list(weights) if len(weights) == n_seg else [1.3 - 0.6 * q / (n_seg - 1) if n_seg > 1 else 1.0 for q in range(n_seg)]
    cut, acc = [0], 0.0
    for q in range(n_seg):
        acc += w[q]
        cut.append(steps if q + 1 == n_seg else min(steps - (n_seg - 1 - q), max(cut[-1] + 1, math.floor(steps * acc / sum(w) + 0.5))))
    return cut


# (SYNTHRAY_TILE = rows, columns, halo, rows per band, planes per segment; SYNTHRAY_TILE_CUTS).  The ring of three node-plane
# slots and two mid slots comes round every six planes: the segments' first planes below are 0 5 9 14 18 23 27, then (the
# seven shares do not fit five segments: the ramp) 0 8 16 22 28, then 0 1 7 13 19 25 31 -- every residue modulo 6, and in the
# last case a first and a last segment of one step.
RING_CASES = [("8,7,2,4,5", "1,1,1,1,1,1,1"), ("8,7,2,4,7", "1,1,1,1,1,1,1"), ("8,7,2,4,5", "1,6,6,6,6,6,1")]


def test_the_cases_start_segments_at_every_ring_phase():
    cuts = [_cuts(STEPS, int(t.split(",")[-1]), [float(x) for x in c.split(",")]) for t, c in RING_CASES]
    assert {k0 % 6 for cut in cuts for k0 in cut[:-1]} == set(range(6)), cuts
    assert cuts[2][-1] - cuts[2][-2] == 1 and cuts[2][1] == 1, cuts[2]


@pytest.mark.gpu
@pytest.mark.parametrize("phase", [True, False], ids=["phase", "no phase"])
def test_every_ring_phase(eng, case, phase):
    """Segments that start at every residue of the slot ring's period, one of them a single step long: where the five slot
    addresses start, how they rotate, where the running record and step-table pointers start."""
    ref, steps = case["ref"][phase, "collimated"]
    for tile, cuts in RING_CASES:
        out, st, (segs, recs) = _trace(eng, case["vols"][phase], case["beams"]["collimated"], case["ext"],
                                       SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS="1", SYNTHRAY_TILE=tile, SYNTHRAY_TILE_CUTS=cuts)
        assert recs and segs == len(_cuts(STEPS, int(tile.split(",")[-1]), [float(x) for x in cuts.split(",")])) - 1, (tile, cuts, segs, recs)
        _same(out, ref, (tile, cuts))
        assert st.ray_steps == steps, (tile, cuts, st.ray_steps, steps)


@pytest.mark.gpu
@pytest.mark.parametrize("phase", [True, False], ids=["phase", "no phase"])
def test_clamped_tiles_and_lost_rays(eng, case, phase):
    """A divergent beam that overfills the volume, NaN rays and a backward ray in it, five-column tiles (the last wavefront
    brings one column, or none): tiles clamped at the volume's edges, rays that change their cell in every stage, rays the
    tiles lose to k_trace_f64."""
    ref, steps = case["ref"][phase, "overfill"]
    out, st, (segs, recs) = _trace(eng, case["vols"][phase], case["beams"]["overfill"], case["ext"],
                                   SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS="1", SYNTHRAY_TILE="8,5,1,3,7", SYNTHRAY_TILE_CUTS=None)
    assert recs and segs == 5, (segs, recs)
    assert st.fallback_rays > 0  # some rays went through k_trace_f64
    _same(out, ref, "overfill")
    assert st.ray_steps == steps, (st.ray_steps, steps)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [None, "8,7,2,4,4"], ids=["one segment per slab", "short segments"])
def test_slabs(eng, case, tile):
    """The 33 planes in three slabs (cuts at planes 11 and 21: no multiples of six), chained by the hand-off records, the
    records kernel on every slab: a slab's records are its OWN planes, counted from its first one -- where the running pointer
    of the DMA starts."""
    ref, steps = case["ref"][True, "collimated"]
    cuts = eng.slab_cuts(N_NODES[2], 3)
    assert len(cuts) == 3 and all(lo % 6 for lo, _ in cuts[1:]), cuts
    s0, ext = case["beams"]["collimated"], case["ext"]
    with _env(SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS="1", SYNTHRAY_TILE=tile, SYNTHRAY_TILE_CUTS=None):
        rays = eng.RayBundle(s0.shape[1]).upload(s0)
        total, vols = 0, []
        for q, (lo, hi) in enumerate(cuts):
            vol = eng.Volume.from_ne_slab(eng.slab_source(case["ne"], 2, lo, hi), *case["axes"], LWL, "z", lo, hi, phaseshift=True)
            vols.append(vol)
            flags = (eng.HANDOFF_ENTER if q > 0 else 0) | (eng.HANDOFF_EXIT if q + 1 < len(cuts) else 0)
            st = rays.trace(vol, eng.default_t_end(ext), ext, precision="f64", handoff=flags)
            assert rays.tile_segments == (1 if tile is None else -(-(hi - lo) // 4)) and rays.tile_records, (lo, hi, rays.tile_segments, rays.tile_records)
            total += st.ray_steps
        out = rays.download()
        rays.close()
        for vol in vols:
            vol.close()
    _same(out, ref, ("slabs", tile))
    assert total == steps, (total, steps)


@pytest.mark.gpu
def test_producers_kernel_shares_the_loop(eng, case):
    """The producers' kernel (SYNTHRAY_TILE_RECORDS=0) runs the same step loop with slot indices for handles."""
    ref, steps = case["ref"][True, "collimated"]
    tile, cuts = RING_CASES[0]
    out, st, (segs, recs) = _trace(eng, case["vols"][True], case["beams"]["collimated"], case["ext"],
                                   SYNTHRAY_F64_TILE="1", SYNTHRAY_TILE_RECORDS="0", SYNTHRAY_TILE=tile, SYNTHRAY_TILE_CUTS=cuts)
    assert segs == 7 and not recs, (segs, recs)
    _same(out, ref, "producers")
    assert st.ray_steps == steps, (st.ray_steps, steps)
