"""GPU parity: libsynthray.so (through the C ABI / ctypes) against the oracle and against the
reference's own outputs in tests/golden/.  Needs an MI355X: run with -m gpu.

Bar: bit-exact for the float32 gradient volumes, the optics coordinates and every integer count;
for the float64 trace the tolerance is written in each test (GPU and oracle run the same algorithm;
they differ only by fused multiply-adds and the reciprocal cell widths).
"""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

FIELDS = ["g1_fields_a", "g1_fields_b", "g1_fields_c", "g1_fields_u"]
TRACES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "g2_trace_*.npz")))


@pytest.fixture(scope="module")
def eng():
    from synthpy_amd import engine

    engine.init(0)
    return engine


# ---------------------------------------------------------------- A1 / A5 / A4 / A3
@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("pdir", ["x", "y", "z"])
def test_calc_dndr_bit_exact_vs_reference(eng, name, pdir):
    """Device gradient volumes == the reference's float32 calc_dndr output, bit for bit, for every layout."""
    g = golden(name)
    vol = eng.Volume.from_ne(g["ne"], g["x"], g["y"], g["z"], float(g["lwl"]), pdir, phaseshift=True)
    assert vol.omega == float(g["omega"])
    gx, gy, gz, nm1 = vol.fields(phase=True)
    assert np.array_equal(gx, g["dndx"]) and np.array_equal(gy, g["dndy"]) and np.array_equal(gz, g["dndz"])
    # n-1 is kept as hi+lo float32 pair: 48 bits of n-1
    assert np.max(np.abs(nm1 - (g["nref"] - 1.0))) <= 2e-15 * np.max(np.abs(g["nref"] - 1.0))


def test_calc_dndr_float32_ne(eng, orc):
    g = golden("g1_fields_a")
    ne32 = np.float32(g["ne"])
    vol = eng.Volume.from_ne(ne32, g["x"], g["y"], g["z"], float(g["lwl"]), "z")
    _, ox, oy, oz = orc.calc_dndr(ne32, g["x"], g["y"], g["z"], float(g["lwl"]))
    gx, gy, gz = vol.fields()
    assert np.array_equal(gx, ox) and np.array_equal(gy, oy) and np.array_equal(gz, oz)


def _small_domain():
    """A 16 x 12 x 10 domain on stretched axes: the optional arguments of the volume's host-array entry points, each at a size
    that takes no time."""
    rng = np.random.default_rng(41)
    x, y, z = (np.float32(1e-4 * np.cumsum(1.0 + 0.3 * rng.random(m))) for m in (16, 12, 10))
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij", sparse=True)
    ne = 1e25 * (1.0 + 0.3 * np.sin(4e3 * X) * np.cos(3e3 * Y) + 0.2 * np.sin(5e3 * Z))
    return x, y, z, ne


@pytest.mark.parametrize("phase", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("pdir", ["x", "z"])
def test_from_ne_dtypes_phase_and_field_subsets(eng, orc, pdir, dtype, phase):
    """Volume.from_ne for float32 / float64 ne, with and without the phase field, against the oracle (gradients bit for bit,
    n-1 to the 48 bits it is kept with); then sr_volume_fields asked for every subset of its outputs: what is asked for equals
    the full read, what is not asked for is not written."""
    from synthpy_amd import _ffi

    x, y, z, ne = _small_domain()
    ne = dtype(ne)
    lwl = 1064e-9
    vol = eng.Volume.from_ne(ne, x, y, z, lwl, pdir, phaseshift=phase)
    om, *grads = orc.calc_dndr(ne, x, y, z, lwl)
    full = vol.fields(phase=phase)
    for a, b in zip(full[:3], grads):
        assert np.array_equal(a, b)
    if phase:
        nm1 = orc.n_refrac(np.float64(ne), om) - 1.0
        assert np.max(np.abs(full[3] - nm1)) <= 2e-15 * np.max(np.abs(nm1))
    for mask in range(1, 16 if phase else 8):
        outs = [np.full(vol.shape, -7.0, np.float32 if k < 3 else np.float64) for k in range(4)]
        args = [_ffi.ptr(outs[k]) if mask >> k & 1 else None for k in range(4)]
        assert _ffi.lib.sr_volume_fields(vol._h, *args) == 0, _ffi.last_error()
        for k in range(4):
            assert np.array_equal(outs[k], full[k]) if mask >> k & 1 else np.all(outs[k] == -7.0), (mask, k)
    if not phase:  # n-1 of a volume without it: an argument error, after the outputs before it were written
        out = np.empty(vol.shape)
        assert _ffi.lib.sr_volume_fields(vol._h, None, None, None, _ffi.ptr(out)) == -1 and "SR_VOL_PHASE" in _ffi.last_error()
    vol.close()


@pytest.mark.parametrize("with_nref", [False, True])
def test_from_fields_with_and_without_nref(eng, orc, with_nref):
    """Volume.from_fields returns what it was given: the gradients bit for bit, n-1 to the 48 bits it is kept with."""
    x, y, z, ne = _small_domain()
    om, gx, gy, gz = orc.calc_dndr(ne, x, y, z, 1064e-9)
    nref = orc.n_refrac(ne, om) if with_nref else None
    for pdir in "xyz":
        vol = eng.Volume.from_fields(gx, gy, gz, x, y, z, om, pdir, nref=nref)
        assert vol.phase == with_nref
        back = vol.fields(phase=with_nref)
        assert np.array_equal(back[0], gx) and np.array_equal(back[1], gy) and np.array_equal(back[2], gz)
        if with_nref:
            assert np.max(np.abs(back[3] - (nref - 1.0))) <= 2e-15 * np.max(np.abs(nref - 1.0))
        vol.close()


def test_attach_aux_subsets_and_replacement(eng):
    """attach_aux with kappa only, with ne and B only, with both, and a second time on the same volume (the fields of the first
    call are replaced or dropped): which fields the volume holds (its size says so), and their values at the nodes that open a
    cell on every axis -- the gathers' weights are 0 and 1 there, so the node values come back, to the bound of
    test_aux_gathers_vs_reference."""
    x, y, z, ne = _small_domain()
    rng = np.random.default_rng(42)
    kappa = [1e9 * (1.0 + rng.random(ne.shape)) for _ in range(2)]
    nes = [ne * (1.0 + 0.5 * k) for k in range(2)]
    B = [rng.standard_normal(ne.shape + (3,)) for _ in range(2)]
    pts = np.stack(np.meshgrid(*(np.float64(a[:-1]) for a in (x, y, z)), indexing="ij"), axis=-1).reshape(-1, 3)
    at_pts = lambda f: f[:-1, :-1, :-1].ravel()
    for pdir in "xz":
        vol = eng.Volume.from_ne(ne, x, y, z, 1064e-9, pdir)
        na = vol.shape["xyz".index(pdir)]
        packed = (na + 7) // 8 * 8 * (ne.size // na)
        bare = vol.nbytes
        # (kappa, ne + B) of each call, by index into the two sets above; None: not given.  Every call after the first replaces
        calls = [(0, None), (None, 0), (1, 1), (None, 1), (0, None), (1, 0)]
        for ik, iq in calls:
            vol.attach_aux(None if ik is None else kappa[ik], None if iq is None else nes[iq], None if iq is None else B[iq], 2.5e-13)
            assert vol.nbytes == bare + packed * 8 * ((ik is not None) + 4 * (iq is not None)), (pdir, ik, iq)
            X = vol.sample_aux(pts)
            ref = []
            if ik is not None:
                ref.append((X[0], at_pts(kappa[ik])))
            if iq is not None:
                ref += [(X[1], at_pts(nes[iq]))] + [(X[2 + c], at_pts(B[iq][..., c])) for c in range(3)]
            for got, want in ref:
                assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want)), (pdir, ik, iq)
        vol.close()


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("pdir", ["x", "y", "z"])
def test_gather_vs_reference(eng, name, pdir):
    """A4/A3: the trilinear gathers at the reference's query points (on nodes, on faces, out of bounds, NaN)
    against the reference's dndr / dsdt: <= 4 ulp of the field's magnitude (fma and reciprocal widths)."""
    g = golden(name)
    vol = eng.Volume.from_fields(g["dndx"], g["dndy"], g["dndz"], g["x"], g["y"], g["z"], float(g["omega"]), pdir, nref=g["nref"])
    F = vol.sample(g["pts"])
    ref = g["grad"]
    assert np.array_equal(np.isnan(F[:3]), np.isnan(ref))
    scale = np.nanmax(np.abs(ref))
    assert np.nanmax(np.abs(F[:3] - ref)) <= 1e-15 * scale
    # out-of-bounds points: exactly the fill value
    oob = (ref[0] == 0) & (ref[1] == 0) & (ref[2] == 0)
    assert np.all(F[:3, oob] == 0)
    dphase = float(g["omega"]) * F[3]
    rp = g["dsdt"][7]
    assert np.nanmax(np.abs(dphase - rp)) <= 1e-12 * np.nanmax(np.abs(rp))


# ---------------------------------------------------------------- A2 + A6
def _oracle_trace(orc, g, sub=1, mode="planes"):
    x = g["x"]
    dom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), phaseshift=bool(g["phaseshift"]))
    ext = float(g["extent"])
    sf, steps = orc.trace_rk4(dom, g["s0"], float(x[1] - x[0]) / orc.c, orc.default_t_end(ext), str(g["pdir"]), mode, sub)
    rf, Jf = orc.ray_to_jones(sf, ext, str(g["pdir"]), "legacy")
    return sf, rf, Jf, steps


class _forced_kernel:
    """Environment for one trace: tile = 0 the per-ray kernel k_trace_f64 alone; 1 the tile path as the library runs it (round 5:
    the RECORDS kernel, k_trace_tile<., false, true>, + k_trace_f64 for the stragglers); 2 the tile path with the PRODUCERS' kernel
    (SYNTHRAY_TILE_RECORDS=0: what runs when the records do not fit in HBM); None: the library's own choice.  check(rays) asserts
    that the library ran what was asked."""

    def __init__(self, tile):
        self.tile = tile
        self.set = {} if tile is None else {"SYNTHRAY_F64_TILE": "1" if tile else "0", "SYNTHRAY_TILE_RECORDS": "0" if tile == 2 else "1"}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.set}
        os.environ.update(self.set)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def check(self, rays, aux=False):
        if self.tile is None:
            return
        assert (rays.tile_segments > 0) == bool(self.tile), f"tile_segments = {rays.tile_segments} with tile = {self.tile}"
        if self.tile and not aux:
            assert rays.tile_records == (self.tile == 1), f"tile_records = {rays.tile_records} with tile = {self.tile}"


def _forced_kernel_trace(eng, vol, s0, t_end, ext, tile, aux=False, **kw):
    """RayBundle.trace with the kernel forced (_forced_kernel), asserting that the library ran what was asked: (sf, rf, Jf, stats).
    aux: the volume carries the optional terms (their tile kernel has producers, never ready-made records)."""
    with _forced_kernel(tile) as fk:
        rays = eng.RayBundle(s0.shape[1]).upload(s0)
        st = rays.trace(vol, t_end, ext, **kw)
        fk.check(rays, aux)
        return (*rays.download(), st)


def _gpu_trace(eng, g, sub=1, sort=True, precision="f64", tile=None):
    """tile None: sr_trace on host arrays, the library's own choice of kernel; 0 / 1: the per-ray / the tile kernel forced."""
    x = g["x"]
    pdir = str(g["pdir"])
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), pdir, phaseshift=bool(g["phaseshift"]))
    ext = float(g["extent"])
    if tile is None:
        return eng.trace(vol, g["s0"], eng.default_t_end(ext), ext, substeps=sub, sort_rays=sort, precision=precision)
    return _forced_kernel_trace(eng, vol, np.ascontiguousarray(g["s0"], np.float64), eng.default_t_end(ext), ext, tile,
                                substeps=sub, sort_rays=sort, precision=precision)


# (sub-steps, kernel): the per-ray kernel with 1 and 2 RK4 steps per cell, the tile kernel (one step per cell is all it takes)
KERNELS = [(1, 0), (2, 0), (1, 1), (1, 2)]  # tile 1: the records kernel, 2: the producers' kernel (_forced_kernel)


@pytest.mark.parametrize("name", TRACES)
@pytest.mark.parametrize("sub,tile", KERNELS)
def test_trace_vs_oracle(eng, orc, name, sub, tile):
    """precision "f64": same algorithm on GPU and CPU: exit position <=1e-13 m, angle <=1e-11 rad, state at t_end
    <=1e-12 m / 1e-3 m/s, phase <=1e-10 rad (relative ~1e-12), Jones vector <=1e-9; identical step counts.  Each float64
    plane kernel by name: k_trace_f64 (tile 0) and the headline's k_trace_tile (tile 1), directly against the oracle."""
    g = golden(name)
    sf_o, rf_o, Jf_o, steps_o = _oracle_trace(orc, g, sub)
    sf, rf, Jf, st = _gpu_trace(eng, g, sub, tile=tile)
    assert st.ray_steps == steps_o and (tile or st.fallback_rays == 0)  # tile path: fallback_rays = rays a tile lost to k_trace_f64
    assert np.max(np.abs(rf[0::2] - rf_o[0::2])) <= 1e-13
    assert np.max(np.abs(rf[1::2] - rf_o[1::2])) <= 1e-11
    assert np.max(np.abs(sf[:3] - sf_o[:3])) <= 1e-12
    assert np.max(np.abs(sf[3:6] - sf_o[3:6])) <= 1e-3
    assert np.max(np.abs(sf[7] - sf_o[7])) <= 1e-10 * max(1.0, np.max(np.abs(sf_o[7])))
    assert np.array_equal(sf[6], sf_o[6]) and np.array_equal(sf[8], sf_o[8])
    assert np.max(np.abs(Jf - Jf_o)) <= 1e-9


@pytest.mark.parametrize("name", TRACES)
@pytest.mark.parametrize("sub", [1, 2])
def test_trace_mixed_vs_oracle(eng, orc, name, sub):
    """precision "mixed": float32 stage arithmetic on float64 state and accumulation (k_trace_mx; with sub-steps the library
    runs its float64 kernel instead -- the mixed build has none for them since round 4 -- well inside these bounds).  Against the
    float64 oracle: exit position <=2e-11 m, angle <=5e-9 rad, state at t_end <=1e-9 m (its along-ray part carries the float32 time integral) / 1 m/s (of 3e8),
    phase <=1e-7 of its magnitude, Jones vector <=1e-4 (phase of up to 320 rad); identical step counts."""
    g = golden(name)
    sf_o, rf_o, Jf_o, steps_o = _oracle_trace(orc, g, sub)
    sf, rf, Jf, st = _gpu_trace(eng, g, sub, precision="mixed")
    assert st.ray_steps == steps_o and st.fallback_rays == 0
    assert np.max(np.abs(rf[0::2] - rf_o[0::2])) <= 2e-11
    assert np.max(np.abs(rf[1::2] - rf_o[1::2])) <= 5e-9
    assert np.max(np.abs(sf[:3] - sf_o[:3])) <= 1e-9
    assert np.max(np.abs(sf[3:6] - sf_o[3:6])) <= 1.0
    phmax = max(1.0, np.max(np.abs(sf_o[7])))
    assert np.max(np.abs(sf[7] - sf_o[7])) <= 1e-7 * phmax
    assert np.max(np.abs(Jf - Jf_o)) <= 1e-4


@pytest.mark.parametrize("name", TRACES)
@pytest.mark.parametrize("precision,tile", [("f64", 0), ("f64", 1), ("f64", 2), ("mixed", None)])
def test_trace_vs_reference_tight(eng, name, precision, tile):
    """Against the reference RHS integrated at rtol=1e-10 (fixtures written by the reference's own dsdt,
    full_solver.py:516-544), every plane kernel by name -- k_trace_f64, k_trace_tile, k_trace_mx: <=1e-8 m, <=1e-6 rad,
    state at t_end <=2e-8 m, phase <=1e-5 of its magnitude."""
    g = golden(name)
    sf, rf, Jf, _ = _gpu_trace(eng, g, precision=precision, tile=tile)
    rt, st = g["rf_tight"], g["sf_tight"]
    assert np.max(np.abs(rf[0::2] - rt[0::2])) <= 1e-8
    assert np.max(np.abs(rf[1::2] - rt[1::2])) <= 1e-6
    assert np.max(np.abs(sf[:3] - st[:3])) <= 2e-8
    phmax = max(1.0, np.max(np.abs(st[7])))
    assert np.max(np.abs(sf[7] - st[7])) <= 1e-5 * phmax
    assert np.max(np.abs(Jf - g["Jf_tight"])) <= 1e-5 * phmax


@pytest.mark.parametrize("name", [t for t in TRACES if "blob32" in t or "turb" in t])
def test_trace_order_independent(eng, name):
    """Binning the rays by cell changes nothing (rays are independent): bit-identical outputs, both precisions."""
    g = golden(name)
    for precision in ("f64", "mixed"):
        a = _gpu_trace(eng, g, sort=True, precision=precision)
        b = _gpu_trace(eng, g, sort=False, precision=precision)
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u, v)
    with pytest.raises(ValueError):
        _gpu_trace(eng, g, precision="f16")


def _block_in_pool(eng, where):
    import gc

    gc.collect()
    return any(where in blocks for blocks in eng._pinned_free.values())


def test_host_buffer_trace_in_pipelined_chunks_is_bit_identical(eng, monkeypatch):
    """sr_trace on host arrays sends a large bundle through in chunks that alternate between the two streams (upload and
    download of one chunk under the trace of another, the traces themselves in a row): same arrays as the single pass, bit for bit, the same totals;
    a shorter last chunk, return_sf / return_E off, both builds."""
    g = golden("g2_trace_turb32_z_s0")
    s0 = np.tile(g["s0"], (1, 6))[:, :5500]
    s0[0] += np.linspace(0, 1e-5, s0.shape[1])  # distinct rays
    x = g["x"]
    ext = float(g["extent"])
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    for precision in ("f64", "mixed"):
        monkeypatch.setenv("SYNTHRAY_TRACE_CHUNK", "0")
        one = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision=precision)
        monkeypatch.setenv("SYNTHRAY_TRACE_CHUNK", "1000")  # at most 1000 rays a chunk: five of 917 and one of 915
        for serial in ("1", "0"):  # the chunks' traces one after the other (the default), or side by side on the two streams
            monkeypatch.setenv("SYNTHRAY_TRACE_SERIAL", serial)
            many = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision=precision)
            for u, v in zip(one[:3], many[:3]):
                assert np.array_equal(u, v, equal_nan=True)
            assert many[3].ray_steps == one[3].ray_steps and many[3].fallback_rays == one[3].fallback_rays
        monkeypatch.delenv("SYNTHRAY_TRACE_SERIAL")
        _, rf, none, _ = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision=precision, return_sf=False, return_E=False)
        assert none is None and np.array_equal(rf, one[1], equal_nan=True)
    # result arrays over page-locked blocks: ordinary writeable arrays, same values; the block is recycled once collected
    monkeypatch.setattr(eng, "PINNED_MIN_BYTES", 1024)
    first = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="mixed")  # "auto": a size is page-locked from its second use
    assert first[1].base is None or type(first[1].base).__name__ != "_PinnedBlock"
    pinned = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="mixed")
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(many[:3], pinned[:3]))
    assert type(pinned[1].base).__name__ == "_PinnedBlock" and pinned[1].flags.writeable and pinned[1].flags.c_contiguous
    where = pinned[1].base.ptr
    pinned[1][:] = 0.0
    view = pinned[1][:, ::2]
    del pinned
    assert view.base is not None and not _block_in_pool(eng, where)  # a view keeps the block out of the pool
    del view
    assert _block_in_pool(eng, where)
    again = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="mixed", return_sf=False, return_E=False)[1]
    assert again.base.ptr == where and np.array_equal(again, many[1], equal_nan=True)
    del again
    monkeypatch.setattr(eng, "PINNED_MIN_BYTES", 8 << 20)
    monkeypatch.setenv("SYNTHRAY_TRACE_CHUNK", "2750")  # exactly two full chunks
    two = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="f64")
    monkeypatch.setenv("SYNTHRAY_TRACE_CHUNK", "0")
    one = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="f64")
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(one[:3], two[:3]))
    # the pipeline's device-side working set is kept between calls (same chunk size: reused; another: replaced) and can be given back
    monkeypatch.setenv("SYNTHRAY_TRACE_CHUNK", "2750")
    again = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="f64")
    eng.release_caches()
    once_more = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="f64")
    monkeypatch.setenv("SYNTHRAY_TRACE_CACHE", "0")
    uncached = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="f64")
    for other in (again, once_more, uncached):
        assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(one[:3], other[:3]))
    eng.release_caches()
    eng.select_stream(0)


@pytest.mark.parametrize("tile", ["0", "1"])
def test_pipeline_ring_slot_first_used_by_a_short_chunk(eng, monkeypatch, tile):
    """sr_trace keeps its three ring bundles between calls.  When 2*chunk < N <= 3*chunk the third slot is first used by the SHORT
    last chunk; its lazily allocated buffers (the sort's pairs, the tile path's records) must be sized by the bundle's capacity,
    not by that chunk's ray count, or the next call with N >= 3*chunk -- the slot at full size -- writes past their end.  Both
    kernels (the tile path allocates the records), against the single pass."""
    g = golden("g2_trace_turb32_z_s0")
    x, ext = g["x"], float(g["extent"])
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    big = np.tile(g["s0"], (1, 40))[:, :9000]
    big[0] += np.linspace(0, 2e-5, big.shape[1])
    monkeypatch.setenv("SYNTHRAY_F64_TILE", tile)
    eng.release_caches()
    for n in (4100, 9000, 4100, 8000):  # at most 2000 rays a chunk: the bundles first see 1367 / 1366 rays, then 1800, 1367, 2000
        s0 = np.ascontiguousarray(big[:, :n])
        monkeypatch.setenv("SYNTHRAY_TRACE_CHUNK", "0")
        one = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="f64")
        monkeypatch.setenv("SYNTHRAY_TRACE_CHUNK", "2000")
        many = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="f64")
        for u, v in zip(one[:3], many[:3]):
            assert np.array_equal(u, v, equal_nan=True), n
        assert many[3].ray_steps == one[3].ray_steps
    eng.release_caches()
    eng.select_stream(0)


def test_fallback_rays_time_stepping(eng, orc):
    """Rays the plane form cannot take: started inside the volume, flying backwards, or too slow to reach
    the exit plane by t_end.  They go through the time-stepping kernel; same rule as the oracle."""
    g = golden("g2_trace_blob32_z_s0")
    s0 = g["s0"][:, :64].copy()
    s0[2, :16] = 0.0                 # start inside the volume
    s0[5, 16:24] *= -1.0             # flying away from the volume
    s0[3:6, 24:32] *= 0.5            # half speed: still inside at t_end
    s0[0, 32:36] = 6e-3              # outside laterally
    x = g["x"]
    ext = float(g["extent"])
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    dt = float(x[1] - x[0]) / orc.c  # same fallback time step on both sides (time steps see the field's kinks)
    sf, rf, Jf, st = eng.trace(vol, s0, eng.default_t_end(ext), ext, dt=dt, precision="f64")
    dom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), phaseshift=True)
    sf_o, steps_o = orc.trace_rk4(dom, s0, dt, orc.default_t_end(ext), "z", "planes", 1)
    assert st.fallback_rays == 32 and st.ray_steps == steps_o
    # time steps straddle the field's kinks, so fma-level differences grow a little more than in the plane form
    assert np.max(np.abs(sf[:3] - sf_o[:3])) <= 1e-10
    assert np.max(np.abs(sf[3:6] - sf_o[3:6])) <= 1e-1
    assert np.max(np.abs(sf[7] - sf_o[7])) <= 1e-8


def test_trace_edge_cases(eng):
    """Empty bundle, a single ray, NaN rays (stay NaN, no error), ray count not a multiple of the block."""
    g = golden("g2_trace_blob32_z_s0")
    x = g["x"]
    ext = float(g["extent"])
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z")
    sf, rf, Jf, st = eng.trace(vol, np.zeros((9, 0)), eng.default_t_end(ext), ext)
    assert rf.shape == (4, 0) and st.ray_steps == 0
    s0 = g["s0"][:, :200].copy()
    s0[0, 5] = np.nan
    s0[4, 7] = np.nan
    sf, rf, Jf, st = eng.trace(vol, s0, eng.default_t_end(ext), ext)
    assert np.all(np.isnan(rf[:, 5])) and np.all(np.isnan(rf[:, 7]))
    ok = np.ones(200, bool)
    ok[[5, 7]] = False
    assert np.all(np.isfinite(rf[:, ok]))
    one = eng.trace(vol, s0[:, :1], eng.default_t_end(ext), ext)[1]
    assert np.array_equal(one[:, 0], rf[:, 0])
    with pytest.raises(ValueError):
        eng.trace(vol, np.zeros((8, 4)), 1e-10, ext)


def test_ray_to_jones_vs_reference(eng):
    """A6 alone on the reference's own final states: positions bit-exact, angles/Jones within 2 ulp."""
    for name in TRACES:
        g = golden(name)
        rf, Jf = eng.ray_to_jones(g["sf_default"], float(g["extent"]), str(g["pdir"]))
        assert np.array_equal(rf[0::2], g["rf_default"][0::2])
        assert np.allclose(rf[1::2], g["rf_default"][1::2], rtol=4e-16, atol=0)
        assert np.allclose(Jf, g["Jf_default"], rtol=0, atol=4e-16)


# ---------------------------------------------------------------- A7 - A11
def _chains(eng):
    return {
        "shadow_single": eng.chain_shadow_single(),
        "shadow_two": eng.chain_shadow_two(),
        "shadow_two_fp": eng.chain_shadow_two(L=350, R=20, focal_plane=3.0),
        "schlieren_df": eng.chain_schlieren(),
        "schlieren_lf": eng.chain_schlieren(stop_R=2, dark_field=False),
        "refracto": eng.chain_refractometry(),
    }


def test_optics_bit_exact_vs_reference(eng):
    g = golden("g3_optics")
    for name, ops in _chains(eng).items():
        r, _ = eng.optics(g["rf"], [(eng.OP_SCALE, 1e3)] + ops)
        assert np.array_equal(r, g[name + "_rf"], equal_nan=True), name


def test_histogram_counts_exact_vs_reference(eng):
    g = golden("g3_optics")
    for name in _chains(eng):
        rf = g[name + "_rf"]
        H = eng.hist2d(rf[0], rf[2], 344, 257, -9, 9, -6.75, 6.75)
        assert np.array_equal(H, g[name + "_H10"]), name
        H = eng.hist2d(rf[0], rf[2], 64, 48, -9, 9, -6.75, 6.75)
        assert np.array_equal(H, g[name + "_H64x48"]), name
    e = g["edge_pts"]
    assert np.array_equal(eng.hist2d(e[0], e[2], 344, 257, -9, 9, -6.75, 6.75), g["edge_H10"])
    assert eng.hist2d(np.zeros(0), np.zeros(0), 8, 4, -1, 1, -1, 1).sum() == 0


def test_interferometry_vs_reference(eng):
    g = golden("g3_optics")
    k = 2 * np.pi / 532e-9
    r, E = eng.optics(g["rf"], [(eng.OP_SCALE, 1e3)] + eng.chain_shadow_two(), E=g["E"], kwave=k)
    assert np.array_equal(r, g["interf_rf"], equal_nan=True)
    ok = ~np.isnan(g["interf_rE"][0])
    assert np.array_equal(ok, ~np.isnan(E[0]))
    assert np.max(np.abs(E[:, ok] - g["interf_rE"][:, ok])) <= 1e-6  # k*|dr| ~ 3e8 rad amplifies 1-ulp differences
    for (nxe, nye), key in (((344, 257), "interf_H10"), ((40, 30), "interf_H40x30")):
        H = eng.interferogram(g["interf_rf"][0], g["interf_rf"][2], g["interf_rE"], nxe, nye, -9, 9, -7, 6)
        assert H.shape == g[key].shape
        assert np.max(np.abs(H - g[key])) <= 1e-12 * max(1.0, g[key].max())
    p = g["interf_edge_pts"]
    H = eng.interferogram(p[0], p[2], g["E"][:, :400], 344, 257, -9, 9, -7, 6)
    assert np.allclose(H, g["interf_edge_H10"], rtol=0, atol=1e-12)


def test_interfere_ref_beam(eng, orc):
    g = golden("g3_optics")
    ok = ~np.isnan(g["rf"][0])
    for nf, deg in ((10, 20), (120, -20), (7, 60)):
        a = eng.interfere_ref_beam(g["rf"][0], g["rf"][2], g["E"], nf, deg)
        b = orc.interfere_ref_beam(g["rf"], g["E"], nf, deg)
        assert np.allclose(a[:, ok], b[:, ok], rtol=0, atol=5e-16)


# ---------------------------------------------------------------- fused device-resident pipeline
@pytest.mark.parametrize("name", ["g2_trace_blob32_z_s0", "g2_trace_turb32_z_s1", "g2_trace_blob24_y_s0"])
def test_fused_trace_deposit(eng, orc, name):
    """Rays stay in HBM from upload to image.  The counts equal the oracle's binning of the GPU's own exit
    rays exactly, and the complex image matches the oracle's within 1e-9 of its maximum."""
    g = golden(name)
    x = g["x"]
    pdir = str(g["pdir"])
    ext = float(g["extent"])
    N = g["s0"].shape[1]
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), pdir, phaseshift=True)
    rays = eng.RayBundle(N).upload(g["s0"])
    rays.trace(vol, eng.default_t_end(ext), ext)
    _, rf, Jf = rays.download()
    for ops, bs in ((eng.chain_shadow_two(), 10), (eng.chain_schlieren(), 10), (eng.chain_refractometry(), 20)):
        img = eng.DetectorImage.counts(bin_scale=bs)
        _, n_in = rays.deposit(img, ops)
        H = img.download()
        r_o, _ = orc.optics(orc.m_to_mm(rf), ops)
        H_o = orc.histogram(r_o, bin_scale=bs)
        assert np.array_equal(H, H_o)
        assert n_in == int(H_o.sum())
        img2 = eng.DetectorImage.counts(bin_scale=bs)  # without the LDS-privatised tiles: same integers
        rays.deposit(img2, ops, lds_tiles=False)
        assert np.array_equal(img2.download(), H)
    k = 2 * np.pi / 532e-9
    img = eng.DetectorImage.complex_field(bin_scale=10)
    rays.deposit(img, eng.chain_shadow_two(), kwave=k, ref_beam=(10, 20))
    amp = img.download()
    E_o = orc.interfere_ref_beam(rf, Jf, 10, 20)
    r_o, E_o = orc.optics(orc.m_to_mm(rf), orc.chain_shadow_two(), E=E_o, kwave=k)
    amp_o = orc.interferogram_sums(r_o, E_o, bin_scale=10)
    assert amp.shape == amp_o.shape
    assert np.max(np.abs(amp - amp_o)) <= 1e-6 * max(1.0, np.max(np.abs(amp_o)))
    Hc = img.amplitude()
    assert np.max(np.abs(Hc - np.sqrt(amp.real[0] ** 2 + amp.real[1] ** 2))) <= 1e-12


# ---------------------------------------------------------------- interferometry end to end, from s0
def _interf_case(name):
    """(ne, x, s0, ext, lwl) of a fixture: the 32^3 trace fixtures or the 64^3 Gaussian blob of BASELINE configs[0]."""
    if name == "c1_blob64":
        from test_oracle_golden import _c1_inputs

        g = golden("g8_config1")
        x, ne, s0 = _c1_inputs(g)
        return ne, x, s0[:, :4000], float(g["extent"]), float(g["lwl"])
    g = golden(name)
    return g["ne"], g["x"], g["s0"], float(g["extent"]), float(g["lwl"])


def _oracle_interferogram_from_s0(orc, ne, x, s0, ext, lwl, bin_scale, sums=False):
    """The reference's interferometry flow on the CPU, from the launch state: solve (phaseshift) -> ray_to_Jonesvector
    -> interfere_ref_beam(10, 10) -> Interferometry.two_lens_solve -> interferogram
    (full_solver.py:376-403, 838-894; diagnostics.py:559-581; rtm_solver.py:376-453)."""
    dom = orc.Domain.from_ne(ne, x, x, x, lwl, phaseshift=True)
    sf, _ = orc.trace_rk4(dom, s0, float(x[1] - x[0]) / orc.c, orc.default_t_end(ext), "z", "planes", 1)
    rf, Jf = orc.ray_to_jones(sf, ext, "z", "legacy")
    E = orc.interfere_ref_beam(rf, Jf, 10, 10)
    r, E = orc.optics(orc.m_to_mm(rf), orc.chain_shadow_two(), E=E, kwave=2 * np.pi / lwl)
    return (orc.interferogram_sums(r, E, bin_scale=bin_scale) if sums else orc.interferogram(r, E, bin_scale=bin_scale)), rf


def _gpu_interferogram_from_s0(eng, ne, x, s0, ext, lwl, bin_scale, precision, tile=None):
    vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    with _forced_kernel(tile) as fk:
        rays.trace(vol, eng.default_t_end(ext), ext, precision=precision)
        fk.check(rays)
    img = eng.DetectorImage.complex_field(bin_scale=bin_scale)
    rays.deposit(img, eng.chain_shadow_two(), kwave=2 * np.pi / lwl, ref_beam=(10, 10))
    return img.amplitude(), rays.download()[1]


INTERF_CASES = ["g2_trace_blob32_z_s0", "g2_trace_turb32_z_s1", "c1_blob64"]


@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("bin_scale", [10, 1])
@pytest.mark.parametrize("name", INTERF_CASES)
def test_interferometry_end_to_end_from_s0_f64(eng, orc, name, bin_scale, tile):
    """The headline diagnostic of BASELINE configs[2], whole flow, both sides starting from the SAME s0: the float64
    build's interferogram equals the oracle's to 1e-5 of its maximum.  (The field propagation exp(i*k*|dr|) carries
    k = 2*pi/lambda[m] against |dr| in mm, rtm_solver.py:380-384: 2.4e9 rad per radian of exit angle over a 400 mm leg,
    so the image tolerance is the trace's angle agreement, ~4e-15 rad, times that.)"""
    ne, x, s0, ext, lwl = _interf_case(name)
    Ho, rf_o = _oracle_interferogram_from_s0(orc, ne, x, s0, ext, lwl, bin_scale)
    Hg, rf_g = _gpu_interferogram_from_s0(eng, ne, x, s0, ext, lwl, bin_scale, "f64", tile)  # each float64 kernel by name
    assert Hg.shape == Ho.shape and Ho.max() > 0
    assert np.max(np.abs(rf_g[1::2] - rf_o[1::2])) <= 1e-13
    err = np.max(np.abs(Hg - Ho)) / Ho.max()
    assert err <= 1e-5, f"{name} bin_scale {bin_scale}: max|dH|/max H = {err:.3g}"
    assert np.array_equal(Hg > 0, Ho > 0)  # the same pixels are lit


@pytest.mark.parametrize("name", INTERF_CASES)
def test_interferometry_end_to_end_from_s0_mixed_is_another_realisation(eng, orc, name):
    """The mixed build (float32 stage arithmetic) stays within its stated ray tolerance (5e-9 rad) -- and that is NOT
    enough for this diagnostic: 5e-9 rad x 2.4e9 rad/rad = 12 rad of field phase, so its interferogram from the same s0
    is a different realisation of the same speckle (measured here: the per-pixel amplitude differs by O(1) of the
    maximum), as is the reference's own default run against its tight run (6e-5 rad apart).  What
    does agree: which pixels are lit (ray positions, 2e-11 m) and the image's mean amplitude.  This is why
    engine.resolve_precision("auto") traces phase-integrating volumes in float64 and why bench.py quotes the
    interferometry headline on that build."""
    ne, x, s0, ext, lwl = _interf_case(name)
    Ho, rf_o = _oracle_interferogram_from_s0(orc, ne, x, s0, ext, lwl, 10)
    Hm, rf_m = _gpu_interferogram_from_s0(eng, ne, x, s0, ext, lwl, 10, "mixed")
    assert np.max(np.abs(rf_m[0::2] - rf_o[0::2])) <= 2e-11 and np.max(np.abs(rf_m[1::2] - rf_o[1::2])) <= 5e-9
    lit_o, lit_m = Ho > 0, Hm > 0
    assert np.sum(lit_o != lit_m) <= 4          # a ray 2e-11 m from a pixel edge may change pixel
    assert abs(Hm.sum() - Ho.sum()) <= 0.2 * Ho.sum()
    err = np.max(np.abs(Hm - Ho)) / Ho.max()
    assert err > 1e-3, "the mixed build reproduced the interferogram: revisit engine.resolve_precision"
    # and the rule that follows from it
    vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)
    assert eng.resolve_precision("auto", vol) == "f64" and eng.resolve_precision(None, vol) == "f64"
    assert eng.resolve_precision("auto", eng.Volume.from_ne(ne, x, x, x, lwl, "z")) == "mixed"
    assert eng.resolve_precision("mixed", vol) == "mixed"


def test_interferometry_end_to_end_sums_and_api_mirror(eng, orc):
    """The complex per-pixel sums behind the image (before sqrt(Re^2 + Re^2)) from s0, and the same flow through the
    legacy API mirror (ScalarDomain.solve(return_E=True) -> rtm.Interferometry): float64 by the auto rule."""
    from synthpy_amd.solvers_legacy import full_solver as fs
    from synthpy_amd.solvers_legacy import rtm_solver as rtm

    ne, x, s0, ext, lwl = _interf_case("g2_trace_turb32_z_s1")
    So, _ = _oracle_interferogram_from_s0(orc, ne, x, s0, ext, lwl, 10, sums=True)
    vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    rays.trace(vol, eng.default_t_end(ext), ext)  # precision "auto" -> f64
    img = eng.DetectorImage.complex_field(bin_scale=10)
    rays.deposit(img, eng.chain_shadow_two(), kwave=2 * np.pi / lwl, ref_beam=(10, 10))
    Sg = img.download()
    assert np.max(np.abs(Sg - So)) <= 2e-5 * np.max(np.abs(So))
    dom = fs.ScalarDomain(x, x, x, ext, phaseshift=True)
    dom.external_ne(ne)
    dom.calc_dndr(lwl)
    rf, Jf = dom.solve(s0, return_E=True)
    it = rtm.Interferometry(rf, E=eng.interfere_ref_beam(rf[0], rf[2], Jf, 10, 10))  # on rf in metres (diagnostics.py:579-581)
    it.two_lens_solve(wl=lwl)
    it.interferogram(bin_scale=10)
    Ho, _ = _oracle_interferogram_from_s0(orc, ne, x, s0, ext, lwl, 10)
    assert np.max(np.abs(it.H - Ho)) <= 1e-5 * Ho.max()


# ---------------------------------------------------------------- the reference's API surface
def test_legacy_api_end_to_end(eng, orc):
    """The reference's documented flow (full_solver.py:13-82) through the mirror classes."""
    from synthpy_amd.solvers_legacy import full_solver as fs
    from synthpy_amd.solvers_legacy import rtm_solver as rtm

    g = golden("g2_trace_blob32_z_s0")
    x = g["x"]
    ext = float(g["extent"])
    dom = fs.ScalarDomain(x, x, x, ext, phaseshift=True)
    dom.external_ne(g["ne"])
    dom.calc_dndr(float(g["lwl"]))
    rf, Jf = dom.solve(g["s0"], return_E=True)
    assert np.max(np.abs(rf[0::2] - g["rf_tight"][0::2])) <= 1e-8
    assert np.max(np.abs(rf[1::2] - g["rf_tight"][1::2])) <= 1e-6
    sh = rtm.Shadowgraphy(rf)
    sh.two_lens_solve()
    sh.histogram(bin_scale=10)
    r_o, _ = orc.optics(orc.m_to_mm(rf), orc.chain_shadow_two())
    assert np.array_equal(sh.rf, r_o, equal_nan=True)
    assert sh.H.dtype == np.float64 and np.array_equal(sh.H, orc.histogram(r_o, bin_scale=10))
    assert np.array_equal(sh.xedges, np.linspace(-9, 9, 345))
    it = rtm.Interferometry(rf, E=Jf)
    it.two_lens_solve(wl=532e-9)
    it.interferogram(bin_scale=10)
    assert it.H.shape == (256, 343)
    # dsdt through the mirror against the reference's RHS fixture
    f = golden("g1_fields_a")
    d2 = fs.ScalarDomain(f["x"], f["y"], f["z"], float(f["extent"]), phaseshift=True)
    d2.external_ne(f["ne"])
    d2.calc_dndr(float(f["lwl"]))
    ds = fs.dsdt(0.0, f["s"].flatten(), d2).reshape(9, -1)
    ok = ~np.isnan(f["dsdt"][3])
    assert np.max(np.abs(ds[:, ok] - f["dsdt"][:, ok])) <= 1e-12 * np.max(np.abs(f["dsdt"][:, ok]))
    assert np.array_equal(d2.dndx, f["dndx"])


@pytest.mark.parametrize("name", ["g9_solve_at_depth_z", "g9_solve_at_depth_x"])
def test_legacy_solve_at_depth(eng, orc, name):
    """ScalarDomain.solve_at_depth (full_solver.py:405-425): the rays are stopped after a flight of length z, inside the
    volume -- none of them is a plane-form ray, the whole bundle goes through the levels to the time-stepping kernel.
    Against the oracle's same route, the reference's RHS integrated tightly, and the reference's own default run."""
    from synthpy_amd.solvers_legacy import full_solver as fs

    g = golden(name)
    x, ext, pdir, depth = g["x"], float(g["extent"]), str(g["pdir"]), float(g["depth"])
    dom = fs.ScalarDomain(x, x, x, ext, phaseshift=True, probing_direction=pdir)
    dom.external_ne(g["ne"])
    dom.calc_dndr(float(g["lwl"]))
    rf = dom.solve_at_depth(g["s0"], depth)
    sf = dom.sf
    st = g["sf_tight"]
    assert np.max(np.abs(sf[:3] - st[:3])) <= 1e-8 and np.max(np.abs(sf[3:6] - st[3:6])) / orc.c <= 2e-5
    assert np.max(np.abs(sf[7] - st[7])) <= 2e-4 * max(1.0, np.max(np.abs(st[7])))
    own = np.max(np.abs(g["rf_default"][0::2] - g["rf_tight"][0::2]))
    assert np.max(np.abs(rf[0::2] - g["rf_tight"][0::2])) <= max(1e-8, own)
    odom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), phaseshift=True)
    dt = float(np.float32(x)[1] - np.float32(x)[0]) / orc.c  # the engine's default time step: one float32 cell of the probing axis
    so, _ = orc.trace_rk4(odom, g["s0"], dt, depth / orc.c, pdir, "planes", 1)
    assert np.max(np.abs(sf[:3] - so[:3])) <= 1e-10 and np.max(np.abs(sf[7] - so[7])) <= 1e-8


def test_simulator_api_end_to_end(eng):
    """The JAX-generation flow (examples/notebooks/test_SynthRayTracer.ipynb cells 4-15) through the mirror: shapes, the
    (rf, Jf, duration) return, and the error behaviour."""
    from synthpy_amd.simulator import beam, diagnostics as diag, domain as d, propagator as p

    ext = 5e-3
    dom = d.ScalarDomain(2 * ext, 48, ne_type="test_exponential_cos", phaseshift=True)
    b = beam.Beam(5000, 4e-3, 5e-5, ext, probing_direction="z", wavelength=1064e-9, seeded=True)
    rf, Jf, duration = p.solve(b.s0, dom, ext, return_E=True)
    assert rf.shape == (4, 5000) and Jf.shape == (2, 5000) and duration > 0
    rf2, Jf2, _ = p.solve(b.s0, dom, ext)
    assert Jf2 is None and np.array_equal(rf, rf2)
    sh = diag.Shadowgraphy(1064e-9, rf)
    sh.single_lens_solve()
    sh.histogram(bin_scale=4)
    assert sh.H.shape == (2574 // 4, 3448 // 4) and sh.H.sum() > 0
    sc = diag.Schlieren(1064e-9, rf)
    sc.DF_solve()
    sc.histogram(bin_scale=4)
    it = diag.Interferometry(1064e-9, rf, Jf)
    it.two_lens_solve()
    it.interferogram(bin_scale=8)
    assert it.H.shape == (2574 // 8 - 1, 3448 // 8 - 1) and np.isfinite(it.H).all()
    with pytest.raises(ValueError):
        d.ScalarDomain(2 * ext, 16, probing_direction="w")


# The only end-to-end numbers the reference stores for the JAX-generation API: the surviving-ray counts its notebook printed
# (examples/notebooks/test_SynthRayTracer.ipynb, cells 12-15: "rf size expected: (300000, 300000)" then "rf after clearing
# nan's: (N, N)").  (fixture key, class, constructor keywords, solve method, rays left of 300000 in the notebook)
NOTEBOOK_SURVIVORS = [("refractometry", "Refractometry", {}, "incoherent_solve", 200047),
                      ("refractometry_L50", "Refractometry", {"L": 50}, "incoherent_solve", 245676),
                      ("shadow_single", "Shadowgraphy", {}, "single_lens_solve", 200047),
                      ("schlieren_DF", "Schlieren", {}, "DF_solve", 125338)]


def _notebook_case():
    """The notebook's set-up (cells 4-6): box 2 x [5, 5, 10] mm, 128 nodes per axis, n_e = 1e24 * 10^(x / 2 mm) * (1 + cos(2 pi y /
    1 mm)) -- up to 0.64 of the critical density: rays are bent by up to 0.7 rad -- a circular beam of radius 5 mm, 5e-5 rad."""
    g = golden("g11_notebook")
    return g, float(g["extent_x"]), float(g["extent_z"]), int(g["n"]), int(g["N"]), int(g["M"])


def test_notebook_setup_against_the_reference_run(eng):
    """tests/golden/g11_notebook.npz: the notebook's volume and beam (seeded, 2e4 rays) run through the reference's OWN solver
    and diagnostics classes (oracle/make_golden.py g11_notebook: full_solver.solve at its default tolerance, its RHS integrated
    at rtol 1e-9 on the first 4000 rays, rtm_solver's four chains): which rays survive.  The mirror classes on the GPU, from the
    same s0: the SAME rays survive as in the reference's tight run, ray for ray, in all four diagnostics; against the
    reference's default run (RK45 rtol 1e-3, one step size for all rays, 0.7 rad off its own tight run on this volume) the sets
    differ in < 1 % of the rays.  Half of the rays agree with the tight run to 2e-8 rad; the strongly bent ones are chaotic in
    the cos(y) ripples and differ by up to 0.02 rad -- without changing side at any mask."""
    from synthpy_amd.solvers_legacy import full_solver as fs, rtm_solver as rtm

    g, ex, ez, n, N, M = _notebook_case()
    x, z = np.linspace(-ex, ex, n), np.linspace(-ez, ez, n)
    dom = fs.ScalarDomain(x, x, z, ez)
    dom.test_exponential_cos(n_e0=1e24, Ly=1e-3, s=2e-3)
    dom.calc_dndr(float(g["lwl"]))
    np.random.seed(int(g["seed"]))
    s0 = fs.init_beam(N, float(g["beam_size"]), float(g["divergence"]), ez, "circular", "z")  # the reference's draw, bit for bit
    rf = dom.solve(s0)
    d_ang = np.abs(rf[1::2, :M] - g["rf_tight"][1::2]).max(axis=0)
    assert np.median(d_ang) <= 1e-7 and np.percentile(d_ang, 99) <= 5e-3 and d_ang.max() <= 0.1
    for key, cls, kw, solve, _ in NOTEBOOK_SURVIVORS:
        o = getattr(rtm, cls)(rf, **kw)
        assert o.on_device
        getattr(o, solve)()
        kept = ~np.isnan(o.rf[0]) & ~np.isnan(o.rf[2])
        tight = np.unpackbits(g["kept_tight_" + key])[:M].astype(bool)
        default = np.unpackbits(g["kept_default_" + key])[:N].astype(bool)
        assert np.array_equal(kept[:M], tight), f"{key}: {int((kept[:M] != tight).sum())} of {M} rays on the other side of a mask than in the reference's tight run"
        assert (kept != default).sum() <= 0.01 * N, (key, int((kept != default).sum()))
        # the fused deposit counts exactly those rays on a detector wide enough for all of them
        wide = getattr(rtm, cls)(rf, Lx=2e6, Ly=2e6, **kw)
        getattr(wide, solve)()
        wide.histogram(bin_scale=8)
        assert wide.on_device and int(wide.H.sum()) == int(kept.sum()), key


def test_simulator_flow_and_the_notebooks_surviving_ray_counts(eng):
    """examples/notebooks/test_SynthRayTracer.ipynb cells 4-15 as written there, through the JAX-generation mirror:
    ScalarDomain(2*[5e-3, 5e-3, 10e-3], 128, ne_type="test_exponential_cos"), Beam(300000, 5e-3, 5e-5, 10e-3, circular, NOT
    seeded), solve, four diagnostics whose histogram() printed how many rays were left.

    Fractions of rays left:        notebook    reference's own solver on this volume (g11_notebook: default / tight run)
      Refractometry.incoherent      0.6668      0.788 / 0.790
      Refractometry(L=50)           0.8189      0.992 / 0.990
      Shadowgraphy.single_lens      0.6668      0.788 / 0.790
      Schlieren.DF                  0.4178      0.493 / 0.495
    This flow must reproduce the RIGHT column (another draw of the same beam: within 4 sigma of the binomial spread), and does.
    The notebook's column is 12-17 points lower in every row: it is not what the reference's RHS gives on this volume when it is
    integrated.  The notebook's solve is diffrax Tsit5 with PIDController(rtol=1, atol=1e-5) from dt0 = 4.7e-11 of the normalised
    time (propagator.py:550-572): with rtol = 1 against velocities of 3e8 every step is accepted and the step grows tenfold each
    time, so the 20 mm of plasma -- twelve periods of the cos(y) ripple, gradients that bend rays by up to 0.7 rad -- are crossed
    in two or three steps.  (As shipped today the JAX profile also lacks the factor ne_0, domain.py:426-447: the volume would be
    vacuum and every ray would survive; the notebook's output predates that.)  DESIGN.md section 2 records this."""
    from synthpy_amd.simulator import beam, diagnostics as diag, domain as d, propagator as p

    g, ex, ez, n, N_fix, _ = _notebook_case()
    N = 300000
    dom = d.ScalarDomain(np.array([ex, ex, ez]) * 2, n, ne_type="test_exponential_cos")
    np.random.seed(2)
    b = beam.Beam(N, 5e-3, 5e-5, ez, probing_direction="z", wavelength=1064e-9, beam_type="circular")
    rf, Jf, _ = p.solve(b.s0, dom, ez)
    assert rf.shape == (4, N) and Jf is None
    for key, cls, kw, solve, in_notebook in NOTEBOOK_SURVIVORS:
        o = getattr(diag, cls)(1064e-9, rf, **kw)
        assert o.on_device
        getattr(o, solve)()
        o.histogram(bin_scale=1, clear_mem=False)
        left = int(np.sum(~np.isnan(o.rf[0]) & ~np.isnan(o.rf[2])))  # what the reference's histogram() prints (diagnostics.py:335-345)
        ref = float(np.unpackbits(g["kept_default_" + key])[:N_fix].sum()) / N_fix
        sigma = np.sqrt(ref * (1 - ref) * (1 / N + 1 / N_fix))
        assert abs(left / N - ref) <= 4 * sigma + 0.003, f"{cls}.{solve}{kw}: {left / N:.4f} of the rays left, the reference's solver leaves {ref:.4f}"
        assert left / N - in_notebook / 300000 > 0.05  # the documented gap to the notebook's crude integration


def test_c3_shaped_dense_bundle_takes_the_tile_path_by_itself_vs_oracle(eng, orc):
    """BASELINE configs[2] in miniature, the library choosing its kernel: 2e5 rays in a NARROW beam (radius 0.6 mm: ~50 rays
    per lateral cell of the beam) through bench.make_volume(512) with the phase integral.  The bundle is dense where it is, so
    sr_rays_trace takes the tile path by itself (the records kernel, four segments of node planes, as on the headline) -- against the oracle FROM
    s0: exit rays, step count, shadowgram counts (exact), interferogram (<= 1e-5 of its maximum)."""
    import bench

    ne, x = bench.make_volume(512, device=True)
    ext, lwl, N = 5e-3, 1064e-9, 200000
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    np.random.seed(7)
    s0 = init_beam(N, 0.6e-3, 5e-5, ext, "circular", "z")
    vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)
    assert os.environ.get("SYNTHRAY_F64_TILE") is None
    rays = eng.RayBundle(N).upload(s0)
    st = rays.trace(vol, eng.default_t_end(ext), ext)  # precision "auto": the phase integral is on -> float64
    assert rays.tile_segments == 4 and rays.tile_records, f"library's own choice: tile_segments = {rays.tile_segments}, records {rays.tile_records}"
    sf, rf, Jf = rays.download()
    dom = orc.Domain.from_ne(ne, x, x, x, lwl, phaseshift=True)
    so, steps = orc.trace_rk4(dom, s0, (x[1] - x[0]) / orc.c, orc.default_t_end(ext), "z", "planes", 1)
    ro, Jo = orc.ray_to_jones(so, ext, "z", "legacy")
    assert st.ray_steps == steps
    assert np.max(np.abs(rf[0::2] - ro[0::2])) <= 1e-13 and np.max(np.abs(rf[1::2] - ro[1::2])) <= 1e-11
    assert np.max(np.abs(sf[7] - so[7])) <= 1e-10 * max(1.0, np.max(np.abs(so[7])))
    img = eng.DetectorImage.counts(bin_scale=1)
    rays.deposit(img, eng.chain_shadow_two())
    r_o, _ = orc.optics(orc.m_to_mm(ro), orc.chain_shadow_two())
    assert np.array_equal(img.download(), orc.histogram(r_o, bin_scale=1).astype(np.uint32))
    cimg = eng.DetectorImage.complex_field(bin_scale=1)
    rays.deposit(cimg, eng.chain_shadow_two(), kwave=2 * np.pi / lwl, ref_beam=(10, 10))
    r_o, E_o = orc.optics(orc.m_to_mm(ro), orc.chain_shadow_two(), E=orc.interfere_ref_beam(ro, Jo, 10, 10), kwave=2 * np.pi / lwl)
    H_o = orc.interferogram(r_o, E_o, bin_scale=1)
    assert np.max(np.abs(cimg.amplitude() - H_o)) <= 1e-5 * H_o.max()
    # the same rays spread over the whole lateral grid (radius 4 mm: 1.5 rays per cell) are a sparse bundle: the per-ray kernel
    np.random.seed(7)
    wide = eng.RayBundle(N).upload(init_beam(N, 4e-3, 5e-5, ext, "circular", "z"))
    wide.trace(vol, eng.default_t_end(ext), ext)
    assert wide.tile_segments == 0


# ---------------------------------------------------------------- RCCL binding (one rank; the 8-GPU run is the driver's)
def test_rccl_image_reduce_single_rank(eng):
    """librccl is bound at first use; a one-rank communicator must leave the image as it is (sum over one rank),
    for both image kinds and for reduce-to-root and all-reduce."""
    import ctypes as C

    from synthpy_amd._ffi import check, lib

    ident = C.create_string_buffer(128)
    check(lib.sr_comm_unique_id(ident))
    comm = C.c_void_p()
    check(lib.sr_comm_create(C.byref(comm), ident, 0, 1))
    g = golden("g2_trace_blob32_z_s0")
    x, ext, N = g["x"], float(g["extent"]), g["s0"].shape[1]
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    rays = eng.RayBundle(N).upload(g["s0"])
    rays.trace(vol, eng.default_t_end(ext), ext)
    for img, kw in ((eng.DetectorImage.counts(bin_scale=10), {}),
                    (eng.DetectorImage.complex_field(bin_scale=10), dict(kwave=2 * np.pi / 532e-9, ref_beam=(10, 20)))):
        rays.deposit(img, eng.chain_shadow_two(), **kw)
        before = img.download()
        for root in (0, -1):
            check(lib.sr_image_reduce(img._h, comm, root))
            eng.synchronize()
            assert np.array_equal(img.download(), before)
    lib.sr_comm_destroy(comm)


def test_ray_shard_group_single_process(eng):
    from synthpy_amd.distributed import RayShardGroup

    grp = RayShardGroup(rank=0, world=1)
    assert grp.shard(10) == (0, 10) and grp.max_over_ranks(3.5) == 3.5 and grp.sum_over_ranks(2.0) == 2.0
    img = eng.DetectorImage.counts(bin_scale=20)
    grp.reduce_image(img)  # no-op at world 1
    grp.barrier()
    grp.close()


def test_stripes_of_a_dense_bundle_take_the_tile_path_and_sum_to_the_bundles_image(eng):
    """bench.py --scaling strong cuts ONE bundle into equal-count stripes of the beam (distributed.shard_stripe): a rank's share
    keeps the bundle's density, so it is traced by the tile path like the whole bundle, where an index range of the same size (the
    whole beam at 1/4 of the density, below the tile path's threshold here) runs the per-ray kernel.  Either way every ray's arrays
    are the whole bundle's, bit for bit, and the stripes' counts images add up to the bundle's."""
    import bench
    from synthpy_amd.distributed import shard_range, shard_stripe
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    ne, x = bench.make_volume(256)
    ext, lwl = 5e-3, 1064e-9
    t_end = eng.default_t_end(ext)
    np.random.seed(8)
    s0 = init_beam(330_000, 2.5e-3, 5e-5, ext, "circular", "z")  # 20 rays per cell of the beam's box on 256^3 (a quarter by index: 5)
    vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)

    def trace(part):
        r = eng.RayBundle(part.shape[1]).upload(np.ascontiguousarray(part))
        r.trace(vol, t_end, ext, precision="f64")
        img = eng.DetectorImage.counts(bin_scale=8)
        r.deposit(img, eng.chain_shadow_two())
        out = (r.download(), img.download().copy(), r.tile_segments)
        img.close()
        r.close()
        return out

    (sf, rf, Jf), H, segs = trace(s0)
    assert segs > 0, "the whole bundle is dense: the tile path"
    world = 4
    H_sum, tiled = np.zeros_like(H), []
    for rank in range(world):
        idx = shard_stripe(s0[0], rank, world)
        (sf_p, rf_p, Jf_p), H_p, segs_p = trace(s0[:, idx])
        tiled.append(segs_p > 0)
        assert np.array_equal(sf_p, sf[:, idx], equal_nan=True) and np.array_equal(rf_p, rf[:, idx], equal_nan=True)
        assert np.array_equal(Jf_p, Jf[:, idx], equal_nan=True)
        H_sum += H_p
    assert np.array_equal(H_sum, H) and all(tiled), tiled
    lo, hi = shard_range(s0.shape[1], 1, world)
    (sf_i, _, _), _, segs_i = trace(s0[:, lo:hi])
    assert segs_i == 0 and np.array_equal(sf_i, sf[:, lo:hi], equal_nan=True)  # the reference's cut: sparse, the per-ray kernel
    vol.close()


def test_two_streams_share_a_volume_whose_records_are_built_by_the_first_trace(eng):
    """The job driver alternates its bundles between the library's two streams (run_trace.chunked_trace), and the tile path's
    ready-made records are built lazily by the FIRST tiled trace through a volume: the second stream's trace, queued right behind
    it, must not read records that are still being written.  Two dense bundles through a fresh 256^3 volume, one per stream,
    back to back, against the per-ray kernel's arrays.  (A guard of the ordering tile_records() gives -- the stream is waited for
    before the volume shows the pointer --, not a reproducer: the hardware ran the second stream's kernels behind the 2 ms build
    without it as well.)"""
    import bench
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    ne, x = bench.make_volume(256)
    ext, lwl = 5e-3, 1064e-9
    t_end = eng.default_t_end(ext)
    np.random.seed(21)
    beams = [init_beam(120_000, 0.8e-3, 5e-5, ext, "circular", "z") for _ in range(2)]
    beams[1][0] += 1.5e-3  # another part of the volume
    os.environ["SYNTHRAY_F64_TILE"] = "0"
    try:
        vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)
        ref = []
        for s0 in beams:
            r = eng.RayBundle(s0.shape[1]).upload(s0)
            r.trace(vol, t_end, ext, precision="f64")
            ref.append(r.download())
            r.close()
        vol.close()
    finally:
        del os.environ["SYNTHRAY_F64_TILE"]
    for attempt in range(3):  # a fresh volume each time: the records are built again
        vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)
        rays = []
        for sid, s0 in enumerate(beams):
            eng.select_stream(sid)
            rays.append(eng.RayBundle(s0.shape[1]).upload(s0))
        eng.synchronize()
        for sid, r in enumerate(rays):  # queued back to back, nothing waited for in between
            eng.select_stream(sid)
            r.trace(vol, t_end, ext, precision="f64", want_stats=False)
        eng.synchronize()
        for sid, r in enumerate(rays):
            eng.select_stream(sid)
            assert r.tile_segments > 0 and r.tile_records
            for u, w, what in zip(ref[sid], r.download(), ("sf", "rf", "Jf")):
                assert np.array_equal(u, w, equal_nan=True), (attempt, sid, what, int((u != w).sum()))
            r.close()
        eng.select_stream(0)
        vol.close()


def test_beam_box_of_a_bundle_and_parts_uploaded_side_by_side(eng):
    """What the library judges the ray density by (sr_rays_get_bbox / sr_rays_set_bbox): found at upload, known from the
    parameters of a device-drawn beam, lost when rays arrive by hand-off -- unless the caller has named their beam (ranks > 0 of a
    slab pipeline, distributed.SlabPipeline) --, and found over the WHOLE bundle when it is put together from parts
    (sr_rays_upload_part: the job driver's merged chunks).  A bundle uploaded in parts traces to the arrays of the bundle uploaded
    whole, bit for bit."""
    g = golden("g2_trace_turb32_z_s0")
    x, ext = g["x"], float(g["extent"])
    s0 = np.ascontiguousarray(g["s0"], np.float64)
    N = s0.shape[1]
    whole = eng.RayBundle(N).upload(s0)
    want = np.concatenate([s0[:3].min(axis=1), s0[:3].max(axis=1)])
    assert np.array_equal(whole.bbox, want)
    parts = eng.RayBundle(N)
    cuts = [0, 7, 100, N]
    for a, b in list(zip(cuts[:-1], cuts[1:]))[::-1]:  # any order; `last` on the final call
        parts.upload_part(s0[:, a:b], a, last=(a == 0))
    assert np.array_equal(parts.bbox, want)
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    t_end = eng.default_t_end(ext)
    whole.trace(vol, t_end, ext, precision="f64")
    parts.trace(vol, t_end, ext, precision="f64")
    for u, w in zip(whole.download(), parts.download()):
        assert np.array_equal(u, w, equal_nan=True)
    with pytest.raises(ValueError):
        parts.upload_part(s0[:, :10], N - 5)
    # a device-drawn beam: the box of its parameters
    drawn = eng.RayBundle(1000).generate(beam_size=2e-3, divergence=1e-4, ne_extent=ext, probing_direction="z", seed=3)
    assert np.allclose(drawn.bbox, [-2e-3, -2e-3, -ext, 2e-3, 2e-3, -ext])
    # rays that arrive by hand-off have no box ... unless the caller names their beam; an upload takes the caller's word back
    slab = eng.Volume.from_ne_slab(eng.slab_source(g["ne"], 2, 0, 16), x, x, x, float(g["lwl"]), "z", 0, 16, phaseshift=True)
    whole.trace(slab, t_end, ext, precision="f64", handoff=eng.HANDOFF_EXIT)
    rec = whole.handoff_download()
    other = eng.RayBundle(N)
    other.handoff_upload(rec)
    assert other.bbox is None
    other.bbox = want
    other.handoff_upload(rec)
    assert np.array_equal(other.bbox, want)
    other.bbox = None
    assert other.bbox is None
    with pytest.raises(RuntimeError):
        other.bbox = [1, 0, 0, 0, 1, 1]  # min > max
    other.upload(s0)
    assert np.array_equal(other.bbox, want)


# ---------------------------------------------------------------- the chunked job driver (pvti_trace_mpi.py flow)
def test_chunked_driver_equals_single_pass(eng):
    """Summing per-chunk images in HBM (pvti_trace_mpi.py:144-163) gives exactly the image of one pass over all rays."""
    from synthpy_amd import run_trace as rt

    g = golden("g2_trace_blob32_z_s0")
    x, ext, N = g["x"], float(g["extent"]), g["s0"].shape[1]
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    names = ["shadow", "schlieren_lf", "refract", "interf"]
    one = rt.standard_diagnostics(names, 532e-9, bin_scale=10)
    many = rt.standard_diagnostics(names, 532e-9, bin_scale=10)
    t1 = rt.chunked_trace(vol, ext, N, lambda n, ci: g["s0"], one, chunk=N)
    sizes = rt.chunk_sizes(N, 60)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    src = lambda n, ci: g["s0"][:, offs[ci]:offs[ci] + n]
    tm = rt.chunked_trace(vol, ext, N, src, many, chunk=60, merge_rays=0)  # every chunk on its own; two streams, alternating
    serial = rt.standard_diagnostics(names, 532e-9, bin_scale=10)
    ts = rt.chunked_trace(vol, ext, N, src, serial, chunk=60, streams=1, merge_rays=0)
    # consecutive chunks merged on the device before the trace (sr_rays_upload_part): bundles of >= 100 rays, and the default
    # (everything in one bundle here)
    merged, dflt = rt.standard_diagnostics(names, 532e-9, bin_scale=10), rt.standard_diagnostics(names, 532e-9, bin_scale=10)
    tg = rt.chunked_trace(vol, ext, N, src, merged, chunk=60, merge_rays=100)
    td = rt.chunked_trace(vol, ext, N, src, dflt, chunk=60)
    assert tm["bundles"] == tm["chunks"] == len(sizes) and 1 < tg["bundles"] < tg["chunks"] and td["bundles"] == 1
    assert t1["rays"] == tm["rays"] == ts["rays"] == tg["rays"] == td["rays"] == N
    assert t1["ray_steps"] == tm["ray_steps"] == ts["ray_steps"] == tg["ray_steps"] == td["ray_steps"]
    for a, *others in zip(one, many, serial, merged, dflt):
        for b in others:
            if a.complex_field:
                ra, rb = a.image.download(), b.image.download()
                assert np.max(np.abs(ra - rb)) <= 1e-9 * max(1.0, np.max(np.abs(ra)))  # float64 atomic sums, order differs
            else:
                assert np.array_equal(a.result(), b.result()) and a.result().sum() > 0


def test_driver_cli(eng, tmp_path):
    from synthpy_amd import run_trace as rt

    out = str(tmp_path / "o.npz")
    rt.main(["-d", "32", "-r", "3000", "--chunk", "1024", "--ne-type", "test_exponential_cos",
             "--diagnostics", "shadow,interf", "--bin-scale", "8", "-o", out])
    z = np.load(out)
    assert int(z["rays"]) == 3000 and z["shadow"].shape == (2574 // 8, 3448 // 8) and z["shadow"].sum() > 2500
    assert z["interf"].shape == (2574 // 8 - 1, 3448 // 8 - 1) and np.isfinite(z["interf"]).all()


def test_driver_cli_ray_workers(tmp_path):
    """The job script as a command: the host ray chunks drawn ahead by forked workers (--ray-workers 3, forked before the
    process touches the GPU) give the images of the chunks drawn one after the other (--ray-workers 0), exactly."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for w in (0, 3):
        out = str(tmp_path / f"w{w}.npz")
        cmd = [sys.executable, "-m", "synthpy_amd.run_trace", "-d", "32", "-r", "6300", "--chunk", "1000", "--ne-type", "test_exponential_cos",
               "--diagnostics", "shadow,interf", "--bin-scale", "8", "--ray-workers", str(w), "-o", out]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
        assert res.returncode == 0, res.stderr[-2000:]
        outs.append(np.load(out))
    a, b = outs
    assert int(a["rays"]) == int(b["rays"]) == 6300 and int(a["ray_steps"]) == int(b["ray_steps"])
    assert np.array_equal(a["shadow"], b["shadow"]) and a["shadow"].sum() > 5000
    assert np.max(np.abs(a["interf"] - b["interf"])) <= 1e-12 * np.max(np.abs(a["interf"]))  # atomic sums: order of the adds


# ---------------------------------------------------------------- A3's optional terms: inverse bremsstrahlung, Faraday rotation
def _aux_volume(eng, orc, g, pd, phase=True):
    x = g["x"]
    om = orc.omega(float(g["lwl"]))
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), pd, phaseshift=phase)
    vol.attach_aux(orc.kappa(g["ne"], g["Te"], g["Z"], om), g["ne"], g["B"], orc.verdet(float(g["lwl"])))
    return vol


def test_aux_gathers_vs_reference(eng, orc):
    """atten / get_ne / get_B gathers (full_solver.py:334-355) against the reference's interpolators, all layouts."""
    g = golden("g5_fields_aux")
    for pd in "xyz":
        vol = eng.Volume.from_ne(g["ne"], g["x"], g["y"], g["z"], float(g["lwl"]), pd)
        vol.attach_aux(g["kappa"], g["ne"], g["B"], float(g["verdet"]))
        X = vol.sample_aux(g["pts"])
        ref = np.concatenate([g["kappa_at"][None], g["ne_at"][None], g["B_at"]])
        assert np.array_equal(np.isnan(X), np.isnan(ref))
        ok = ~np.isnan(ref)
        scale = np.max(np.abs(ref[:, ok[0]]), axis=1, keepdims=True)
        assert np.max((np.abs(X - ref) / scale)[ok]) <= 1e-14, pd


@pytest.mark.parametrize("name", ["g5_trace_aux24_z", "g5_trace_aux20_x"])
@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_aux_trace_vs_oracle_and_reference(eng, orc, name, precision):
    """amp and pol through the same RK4 steps, against the oracle: float64 build <= 1e-12 relative of the accumulated
    change, mixed build (float32 stage weights, velocities and corner values, float64 rates and accumulation) <= 1e-6 (measured
    4e-8); both against the reference's tight solve to 1e-6."""
    g = golden(name)
    ext, pd, x = float(g["extent"]), str(g["pdir"]), g["x"]
    vol = _aux_volume(eng, orc, g, pd)
    sf, rf, Jf, st = eng.trace(vol, g["s0"], eng.default_t_end(ext), ext, precision=precision)
    dom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), True, g["Te"], g["Z"], g["B"])
    so, steps = orc.trace_rk4(dom, g["s0"], (x[1] - x[0]) / orc.c, orc.default_t_end(ext), pd, "planes", 1)
    assert st.ray_steps == steps and st.fallback_rays == 0
    tight = g["sf_tight"]
    d_amp, d_pol = np.max(np.abs(tight[6] - g["s0"][6])), np.max(np.abs(tight[8] - g["s0"][8]))
    tol = 1e-12 if precision == "f64" else 1e-6
    print(f"{name} {precision}: d amp {np.max(np.abs(sf[6] - so[6])) / d_amp:.2e}, d pol {np.max(np.abs(sf[8] - so[8])) / d_pol:.2e} of the accumulated change")
    assert np.max(np.abs(sf[6] - so[6])) <= tol * d_amp and np.max(np.abs(sf[8] - so[8])) <= tol * d_pol
    assert np.max(np.abs(sf[:3] - so[:3])) <= (1e-13 if precision == "f64" else 1e-9)
    assert np.max(np.abs(sf[7] - so[7])) <= (1e-9 if precision == "f64" else 1e-7) * np.max(np.abs(so[7]))
    assert np.max(np.abs(sf[6] - tight[6])) <= 1e-6 * d_amp and np.max(np.abs(sf[8] - tight[8])) <= 1e-6 * d_pol
    assert np.max(np.abs(Jf - g["Jf_tight"])) <= 1e-5 * np.max(np.abs(tight[7]))


@pytest.mark.parametrize("name", ["g5_trace_aux24_z", "g5_trace_aux20_x"])
def test_inverse_bremsstrahlung_alone_runs_the_kappa_only_kernel(eng, orc, monkeypatch, name):
    """`inv_brems=True` without `B_on` (full_solver.py:243-268, 334-339, 540): the volume carries kappa and nothing of the Faraday
    term, and k_trace_f64<., true, false, 1> (trace_f64.inc, SEL = 1: two wavefronts per SIMD) traces it -- sparse bundles and,
    unforced, dense ones.  Against the oracle with kappa alone (amp to 1e-12 of its change, pol untouched), and bit for bit against
    the five-field kernel (SYNTHRAY_AUX_ONE_PASS=1) and the tile path's optional-terms kernel (forced) on a dense bundle."""
    g = golden(name)
    ext, pd, x = float(g["extent"]), str(g["pdir"]), g["x"]
    om = orc.omega(float(g["lwl"]))
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), pd, phaseshift=True)
    vol.attach_aux(kappa=orc.kappa(g["ne"], g["Te"], g["Z"], om))
    s0 = np.ascontiguousarray(g["s0"])
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    st = rays.trace(vol, eng.default_t_end(ext), ext, precision="f64")
    sf, rf, Jf = rays.download()
    dom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), True, g["Te"], g["Z"], None)
    so, steps = orc.trace_rk4(dom, s0, (x[1] - x[0]) / orc.c, orc.default_t_end(ext), pd, "planes", 1)
    d_amp = np.max(np.abs(so[6] - s0[6]))
    assert st.ray_steps == steps and d_amp > 1e-3
    assert np.max(np.abs(sf[6] - so[6])) <= 1e-12 * d_amp and np.array_equal(sf[8], s0[8])
    assert np.max(np.abs(sf[:3] - so[:3])) <= 1e-13 and np.max(np.abs(sf[7] - so[7])) <= 1e-9 * np.max(np.abs(so[7]))
    # a dense bundle: the library's own choice is still the per-ray kernel (kappa only); the same arrays from the five-field
    # kernel and from the tile path's kernel
    dense = np.tile(s0, (1, 30))
    lat = [k for k in range(3) if k != "xyz".index(pd)]
    dense[lat[1]] += np.linspace(-1e-4, 1e-4, dense.shape[1])
    big = eng.RayBundle(dense.shape[1]).upload(dense)
    big.trace(vol, eng.default_t_end(ext), ext, precision="f64")
    assert big.tile_segments == 0
    ref = big.download()
    for var, val in (("SYNTHRAY_AUX_ONE_PASS", "1"), ("SYNTHRAY_F64_TILE", "1")):
        monkeypatch.setenv(var, val)
        big.trace(vol, eng.default_t_end(ext), ext, precision="f64")
        assert (big.tile_segments > 0) == (var == "SYNTHRAY_F64_TILE")
        for u, w, what in zip(ref, big.download(), ("sf", "rf", "Jf")):
            assert np.array_equal(u, w, equal_nan=True), (var, what, int((u != w).sum()))
        monkeypatch.delenv(var)


@pytest.mark.parametrize("name", ["g5_trace_aux24_z", "g5_trace_aux20_x"])
def test_tile_kernel_with_optional_terms(eng, orc, monkeypatch, name):
    """k_trace_tile<., AUX>: kappa / Faraday fields as five more coefficient fields of a cell's LDS record, built by a second
    wavefront of producers.  Forced onto the reference's fixtures: against the oracle (amp, pol <= 1e-12 of the accumulated
    change) and the reference's tight solve, and bit for bit the per-ray kernel k_trace_f64<., AUX, .> -- on a dense bundle, in
    several segments, rows 6 and 8 of sf included."""
    g = golden(name)
    ext, pd, x = float(g["extent"]), str(g["pdir"]), g["x"]
    vol = _aux_volume(eng, orc, g, pd)
    sf, rf, Jf, st = _forced_kernel_trace(eng, vol, np.ascontiguousarray(g["s0"]), eng.default_t_end(ext), ext, 1, aux=True, precision="f64")
    dom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), True, g["Te"], g["Z"], g["B"])
    so, steps = orc.trace_rk4(dom, g["s0"], (x[1] - x[0]) / orc.c, orc.default_t_end(ext), pd, "planes", 1)
    tight = g["sf_tight"]
    d_amp, d_pol = np.max(np.abs(tight[6] - g["s0"][6])), np.max(np.abs(tight[8] - g["s0"][8]))
    assert st.ray_steps == steps
    assert np.max(np.abs(sf[6] - so[6])) <= 1e-12 * d_amp and np.max(np.abs(sf[8] - so[8])) <= 1e-12 * d_pol
    assert np.max(np.abs(sf[:3] - so[:3])) <= 1e-13 and np.max(np.abs(sf[7] - so[7])) <= 1e-9 * np.max(np.abs(so[7]))
    assert np.max(np.abs(sf[6] - tight[6])) <= 1e-6 * d_amp and np.max(np.abs(sf[8] - tight[8])) <= 1e-6 * d_pol
    # a dense bundle (30 copies of the fixture's rays, shifted), whole volume and in segments of 5 node planes
    s0 = np.tile(g["s0"], (1, 30))
    lat = [k for k in range(3) if k != "xyz".index(pd)]
    s0[lat[1]] += np.linspace(-1e-4, 1e-4, s0.shape[1])
    ref = _forced_kernel_trace(eng, vol, s0, eng.default_t_end(ext), ext, 0, precision="f64")
    assert np.max(np.abs(ref[0][6] - s0[6])) > 1e-3 and np.max(np.abs(ref[0][8] - s0[8])) > 1e-6  # the terms are on
    for geom in (None, "6,7,2,3,5", "5,5,1,2,7"):
        if geom:
            monkeypatch.setenv("SYNTHRAY_TILE", geom)
        got = _forced_kernel_trace(eng, vol, s0, eng.default_t_end(ext), ext, 1, aux=True, precision="f64")
        for u, w, what in zip(ref[:3], got[:3], ("sf", "rf", "Jf")):
            assert np.array_equal(u, w, equal_nan=True), (geom, what, int((u != w).sum()))
        assert got[3].ray_steps == ref[3].ray_steps, geom


def test_aux_fallback_rays(eng, orc):
    """Rays the plane form cannot take (launched inside the volume, or backwards) carry amp and pol through the
    time-stepping form, as the oracle's trace_one."""
    g = golden("g5_trace_aux24_z")
    ext, x = float(g["extent"]), g["x"]
    s0 = g["s0"].copy()
    s0[2, :20] = -0.4 * ext          # start inside
    s0[5, 20:30] *= -1.0             # heading away from the volume
    s0[2, 20:30] = 0.3 * ext         # ... from inside it
    vol = _aux_volume(eng, orc, g, "z")
    dt = float(np.float32(x)[1] - np.float32(x)[0]) / orc.c
    sf, rf, Jf, st = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="f64", dt=dt)
    assert st.fallback_rays == 30
    dom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), True, g["Te"], g["Z"], g["B"])
    so, _ = orc.trace_rk4(dom, s0, dt, orc.default_t_end(ext), "z", "planes", 1)
    assert np.max(np.abs(so[6, :30] - s0[6, :30])) > 1e-4 and np.max(np.abs(so[8, :30] - s0[8, :30])) > 1e-4
    assert np.max(np.abs(sf[6] - so[6])) <= 1e-10 and np.max(np.abs(sf[8] - so[8])) <= 1e-10
    assert np.max(np.abs(sf[:3] - so[:3])) <= 1e-10


def test_legacy_api_optional_terms(eng, orc):
    """ScalarDomain(B_on=True, inv_brems=True, phaseshift=True): kappa(), set_up_interps(), dsdt rows 6 and 8 and
    solve() through the mirror against the reference's fixtures."""
    from synthpy_amd.solvers_legacy import full_solver as fs

    f = golden("g5_fields_aux")
    d = fs.ScalarDomain(f["x"], f["y"], f["z"], float(f["extent"]), B_on=True, inv_brems=True, phaseshift=True)
    d.external_ne(f["ne"])
    d.external_Te(f["Te_in"])
    d.external_Z(f["Z"])
    d.external_B(f["B"])
    d.calc_dndr(float(f["lwl"]))
    assert d.VerdetConst == float(f["verdet"]) and np.array_equal(d.Te, f["Te"])
    assert np.array_equal(d.kappa(), f["kappa"])
    d.set_up_interps()
    ds = fs.dsdt(0.0, f["s"].flatten(), d).reshape(9, -1)
    ok = ~np.isnan(f["dsdt"][3])
    for row in (6, 8):
        ref = f["dsdt"][row][ok]
        assert np.max(np.abs(ds[row][ok] - ref)) <= 1e-13 * np.max(np.abs(ref))
    g = golden("g5_trace_aux24_z")
    x = g["x"]
    d2 = fs.ScalarDomain(x, x, x, float(g["extent"]), B_on=True, inv_brems=True, phaseshift=True)
    d2.external_ne(g["ne"]); d2.external_Te(g["Te"]); d2.external_Z(g["Z"]); d2.external_B(g["B"])
    d2.calc_dndr(float(g["lwl"]))
    rf, Jf = d2.solve(g["s0"], return_E=True)  # set_up_interps() is called for the caller
    t = g["sf_tight"]
    assert np.max(np.abs(d2.sf[6] - t[6])) <= 1e-6 * np.max(np.abs(t[6] - 1)) and np.max(np.abs(d2.sf[8] - t[8])) <= 1e-6
    # against the reference as shipped (RK45 rtol 1e-3): inside its own error against its tight run
    own = np.max(np.abs(g["sf_default"][[6, 8]] - t[[6, 8]]))
    assert np.max(np.abs(d2.sf[[6, 8]] - g["sf_default"][[6, 8]])) <= own + 1e-6


def test_simulator_api_optional_terms(eng, orc):
    from synthpy_amd.simulator import domain as d, propagator as p

    g = golden("g5_trace_aux20_x")
    ext, n = float(g["extent"]), int(g["n"])
    dom = d.ScalarDomain(2 * ext, n, inv_brems=True, phaseshift=True, B_on=True, probing_direction="x")
    dom.external_ne(g["ne"]); dom.external_Te(g["Te"]); dom.external_Z(g["Z"]); dom.external_B(g["B"])
    rf, Jf, _ = p.solve(g["s0"], dom, ext, return_E=True, lwl=float(g["lwl"]))
    assert np.max(np.abs(Jf - g["Jf_tight"])) <= 1e-5 * np.max(np.abs(g["sf_tight"][7]))
    assert np.max(np.abs(np.abs(Jf[1]) / np.cos(g["sf_tight"][8]) - g["sf_tight"][6])) <= 1e-6


def test_simulator_dsdt_with_the_references_argument_list(eng):
    """propagator.dsdt(t, s, parallelise, inv_brems, phaseshift, B_on, ne, B, Te, Z, x, y, z, omega, VerdetConst, ...)
    (propagator.py:94-175) against the RHS the reference's legacy dsdt returned for the same states (fixture g5_fields_aux:
    the same gathers, full_solver.py:516-544), every row, and against the legacy mirror's dsdt."""
    from synthpy_amd.simulator import propagator as p
    from synthpy_amd.solvers_legacy import full_solver as fs

    f = golden("g5_fields_aux")
    omega = 2 * np.pi * eng.c / float(f["lwl"])
    out = p.dsdt(0.0, f["s"].flatten(), False, True, True, True, f["ne"], f["B"], f["Te"], f["Z"], f["x"], f["y"], f["z"], omega,
                 float(f["verdet"]), None, None).reshape(9, -1)
    ref = f["dsdt"]
    ok = ~np.isnan(ref[3])
    assert ok.sum() > 0.5 * ok.size
    assert np.array_equal(out[:3], f["s"][3:6])
    for row, tol in ((3, 1e-12), (4, 1e-12), (5, 1e-12), (6, 1e-13), (7, 1e-9), (8, 1e-13)):
        scale = np.max(np.abs(ref[row][ok]))
        assert scale > 0 and np.max(np.abs(out[row][ok] - ref[row][ok])) <= tol * scale, row
    d = fs.ScalarDomain(f["x"], f["y"], f["z"], float(f["extent"]), B_on=True, inv_brems=True, phaseshift=True)
    d.external_ne(f["ne"]); d.external_Te(f["Te_in"]); d.external_Z(f["Z"]); d.external_B(f["B"])
    d.calc_dndr(float(f["lwl"]))
    d.set_up_interps()
    mine = fs.dsdt(0.0, f["s"].flatten(), d).reshape(9, -1)
    assert np.array_equal(np.nan_to_num(mine), np.nan_to_num(out))
    # the switches: a term that is off stays zero
    off = p.dsdt(0.0, f["s"].flatten(), False, False, False, False, f["ne"], None, None, None, f["x"], f["y"], f["z"], omega, 0.0).reshape(9, -1)
    assert np.array_equal(off[3:6], out[3:6], equal_nan=True) and not np.nan_to_num(off[6:]).any()
    assert fs.ScalarDomain.omega_pe(4.0) == 5.64e4 * 2 and d.omega_pe(4.0) == 5.64e4 * 2


class _Axes:
    def __init__(self):
        self.lines = []

    def plot(self, x, y):
        self.lines.append((np.asarray(x), np.asarray(y)))


def test_small_members_of_the_two_apis(eng):
    """plot_midline_gradients (full_solver.py:291-315), Diagnostic.propagate_E (diagnostics.py:315-321), ray (:258-263), and the two
    members that cannot be carried over saying so (bkg, fresnel_solve)."""
    from synthpy_amd.simulator import diagnostics as dg
    from synthpy_amd.solvers_legacy import full_solver as fs

    g = golden("g2_trace_blob32_z_s0")
    x = g["x"]
    d = fs.ScalarDomain(x, x, x, float(g["extent"]))
    d.external_ne(g["ne"])
    d.calc_dndr(float(g["lwl"]))
    m = len(x) // 2
    for direction, line in (("x", (slice(None), m, m)), ("y", (m, slice(None), m)), ("z", (m, m, slice(None))), ("w", (m, slice(None), m))):
        ax = _Axes()
        d.plot_midline_gradients(ax, direction)
        assert len(ax.lines) == 3
        for (xs, ys), grad in zip(ax.lines, (d.dndx, d.dndy, d.dndz)):
            assert np.array_equal(xs, d.y) and np.array_equal(ys, grad[line])
    rng = np.random.default_rng(3)
    rf = rng.normal(size=(4, 50)) * 1e-3
    Jf = rng.normal(size=(2, 50)) + 1j * rng.normal(size=(2, 50))
    it = dg.Interferometry(1064e-9, rf.copy(), Jf.copy())
    r1 = dg.travel(it.r0, 25.0)
    it.propagate_E(r1, it.r0)
    want = Jf * np.exp(1j * (2 * np.pi / 1064e-9) * np.sqrt((r1[0] - it.r0[0]) ** 2 + (r1[2] - it.r0[2]) ** 2))
    assert np.array_equal(it.Jf, want)
    assert dg.ray(1, 2, 3, 4).shape == (4, 1)
    with pytest.raises(NotImplementedError, match="probing_direction"):
        it.bkg(1.0, 10, 10, 5e-3)
    with pytest.raises(NotImplementedError, match="fresnel_integral"):
        dg.Refractometry(1064e-9, rf.copy()).fresnel_solve()


# ---------------------------------------------------------------- coherent refractometer, knife edge, phase-only travel
def test_coherent_refractometer_vs_reference(eng, orc):
    """Refractometry.coherent_solve + seeded refractogram through the legacy mirror (rtm_solver.py:288-369)."""
    from synthpy_amd.solvers_legacy import rtm_solver as rtm

    g = golden("g6_optics_extra")
    d = rtm.Refractometry(g["rf"].copy(), E=g["E"].copy(), focal_plane=2.0)
    d.coherent_solve(wl=1064e-9)
    ok = ~np.isnan(g["coh_rf"][0])
    assert np.array_equal(np.isnan(d.rf[0]), ~ok) and np.array_equal(d.rf[:, ok], g["coh_rf"][:, ok])
    assert np.max(np.abs(d.rE[:, ok] - g["coh_rE"][:, ok])) <= 1e-6  # k*|dr| ~ 1e7 rad as written
    d.rE = g["coh_rE"]  # the reference's field in: isolates speckle + binning
    np.random.seed(9)
    d.refractogram(bin_scale=10)
    assert d.H.shape == g["coh_H10_seed9"].shape and np.max(np.abs(d.H - g["coh_H10_seed9"])) <= 1e-11
    # knife edge, in-place NaN columns as the reference's function
    r0 = rtm.m_to_mm(g["rf"].copy())
    for k, (off, row, dr) in enumerate(g["knife_args"]):
        r = rtm.knife_edge(r0.copy(), off, "x" if row == 0 else "y", dr)
        ref = g[f"knife{k}"]
        assert np.array_equal(np.isnan(r), np.isnan(ref)) and np.array_equal(r[~np.isnan(ref)], ref[~np.isnan(ref)])


def test_coherent_refractometer_jax_as_written(eng, orc):
    """diagnostics.py:505-524 through the simulator mirror against the oracle's chain with the phase-only first leg."""
    from synthpy_amd.simulator import diagnostics as diag

    g = golden("g6_optics_extra")
    d = diag.Refractometry(1064e-9, g["rf"].copy(), g["E"].copy(), focal_plane=2.0)
    d.coherent_solve()
    r0 = orc.optics(g["rf"], [(orc.SCALE, 1e3)])[0]
    r, E = orc.optics(r0, orc.chain_refractometry_coherent(focal_plane=2.0, as_written_jax=True), g["E"], 2 * np.pi / 1064e-9)
    ok = ~np.isnan(r[0])
    assert np.array_equal(np.isnan(d.rf[0]), ~ok) and np.array_equal(d.rf[:, ok], r[:, ok])
    assert np.max(np.abs(d.Jf[:, ok] - E[:, ok])) <= 1e-6
    assert not np.array_equal(r[:, ok], g["coh_rf"][:, ok])  # the two generations differ, as written


# ---------------------------------------------------------------- A12: slab-decomposed volume, ray hand-off
def _slab_chain(eng, g, pd, cuts, precision, phase=True, aux=None, via_host=True, s0=None, requeued=0, tiles=None):
    x, ext = g["x"], float(g["extent"])
    axis = "xyz".index(pd)
    s0 = g["s0"] if s0 is None else s0
    N = s0.shape[1]
    rays = eng.RayBundle(N).upload(s0)
    steps, vols = 0, []
    for q, (lo, hi) in enumerate(cuts):
        vol = eng.Volume.from_ne_slab(eng.slab_source(g["ne"], axis, lo, hi), x, x, x, float(g["lwl"]), pd, lo, hi, phaseshift=phase)
        if aux is not None:
            sl = [slice(None)] * 3
            sl[axis] = slice(lo, hi + 1)
            vol.attach_aux(np.ascontiguousarray(aux[0][tuple(sl)]), np.ascontiguousarray(g["ne"][tuple(sl)]),
                           np.ascontiguousarray(g["B"][tuple(sl)]), aux[1])
        vols.append(vol)
        flags = (eng.HANDOFF_ENTER if q > 0 else 0) | (eng.HANDOFF_EXIT if q + 1 < len(cuts) else 0)
        st = rays.trace(vol, eng.default_t_end(ext), ext, precision=precision, handoff=flags)
        steps += st.ray_steps
        if tiles is None:
            assert st.fallback_rays == requeued  # rays the first kernel passed on (mixed build: to the float64 plane kernel)
        else:
            tiles.append(rays.tile_segments)  # which kernel carried this slab
        if via_host and q + 1 < len(cuts):  # through the host, into a fresh bundle (what another GPU would hold)
            rec = rays.handoff_download()
            rays = eng.RayBundle(N).handoff_upload(rec)
    return rays.download(), steps


@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("name", ["g2_trace_turb32_z_s0", "g2_trace_blob24_x_s0", "g2_trace_blob24_y_s0"])
def test_slab_chain_equals_whole_volume(eng, name, precision):
    """A chain of slab volumes with the rays handed over on the shared node planes gives the whole-volume trace bit
    for bit (same gradients, same steps), in both builds, through the host and in place."""
    g = golden(name)
    x, ext, pd = g["x"], float(g["extent"]), str(g["pdir"])
    ph = bool(g["phaseshift"])
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), pd, phaseshift=ph)
    sf, rf, Jf, st = eng.trace(vol, g["s0"], eng.default_t_end(ext), ext, precision=precision)
    n = len(x)
    for cuts, via_host in ((eng.slab_cuts(n, 2), True), (eng.slab_cuts(n, 4), False), ([(0, 1), (1, 2), (2, n - 2), (n - 2, n - 1)], True)):
        (sf2, rf2, Jf2), steps = _slab_chain(eng, g, pd, cuts, precision, phase=ph, via_host=via_host)
        assert np.array_equal(sf2, sf) and np.array_equal(rf2, rf) and np.array_equal(Jf2, Jf), cuts
        assert steps == st.ray_steps


@pytest.mark.parametrize("name", ["g2_trace_turb32_z_s0", "g2_trace_blob24_x_s0"])
def test_slab_chain_through_the_tile_kernel(eng, monkeypatch, name):
    """A12 with the headline's kernel: slabs of node planes are traced by k_trace_tile (arrivals binned again by the cell they
    are in, records in, records out, the rays a tile loses carried through the slab by k_trace_f64's slab form) -- the chain
    still equals the whole-volume trace of the per-ray kernel bit for bit, step counts included; slabs too thin for a
    segment (fewer than three node planes) fall to the per-ray kernel inside the same chain."""
    g = golden(name)
    x, ext, pd = g["x"], float(g["extent"]), str(g["pdir"])
    s0 = np.tile(g["s0"], (1, 24))
    lat = [k for k in range(3) if k != "xyz".index(pd)]
    s0[lat[0]] += np.linspace(-2e-4, 2e-4, s0.shape[1])  # distinct rays
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), pd, phaseshift=True)
    monkeypatch.setenv("SYNTHRAY_F64_TILE", "0")
    sf, rf, Jf, st = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="f64")
    monkeypatch.setenv("SYNTHRAY_F64_TILE", "1")
    n = len(x)
    for cuts, via_host in ((eng.slab_cuts(n, 2), True), (eng.slab_cuts(n, 3), False), ([(0, 1), (1, 9), (9, n - 2), (n - 2, n - 1)], True)):
        tiles = []
        (sf2, rf2, Jf2), steps = _slab_chain(eng, g, pd, cuts, "f64", via_host=via_host, s0=s0, tiles=tiles)
        assert np.array_equal(sf2, sf, equal_nan=True) and np.array_equal(rf2, rf, equal_nan=True) and np.array_equal(Jf2, Jf, equal_nan=True), cuts
        assert steps == st.ray_steps, (cuts, steps, st.ray_steps)
        assert [t > 0 for t in tiles] == [hi - lo >= 2 for lo, hi in cuts], (cuts, tiles)
    # short segments inside the slabs as well (SYNTHRAY_TILE: 8 x 8 tiles, 5 planes per segment)
    monkeypatch.setenv("SYNTHRAY_TILE", "8,8,2,2,5")
    tiles = []
    (sf2, rf2, Jf2), steps = _slab_chain(eng, g, pd, eng.slab_cuts(n, 2), "f64", via_host=False, s0=s0, tiles=tiles)
    assert np.array_equal(sf2, sf, equal_nan=True) and np.array_equal(Jf2, Jf, equal_nan=True) and steps == st.ray_steps and min(tiles) >= 3


def test_slab_gradients_equal_whole_volume(eng):
    g = golden("g2_trace_turb32_z_s0")
    x, n = g["x"], len(g["x"])
    for pd in "xyz":
        axis = "xyz".index(pd)
        whole = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), pd, phaseshift=True).fields(phase=True)
        for lo, hi in eng.slab_cuts(n, 3):
            part = eng.Volume.from_ne_slab(eng.slab_source(g["ne"], axis, lo, hi), x, x, x, float(g["lwl"]), pd, lo, hi,
                                           phaseshift=True).fields(phase=True)
            sl = [slice(None)] * 3
            sl[axis] = slice(lo, hi + 1)
            for a, b in zip(part, whole):
                assert np.array_equal(a, b[tuple(sl)]), (pd, lo, hi)


def test_slab_chain_aux_terms_and_oracle(eng, orc):
    g = golden("g5_trace_aux24_z")
    x, ext = g["x"], float(g["extent"])
    om = orc.omega(float(g["lwl"]))
    kap = orc.kappa(g["ne"], g["Te"], g["Z"], om)
    (sf, rf, Jf), _ = _slab_chain(eng, g, "z", eng.slab_cuts(len(x), 3), "f64", aux=(kap, orc.verdet(float(g["lwl"]))))
    dom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), True, g["Te"], g["Z"], g["B"])
    rec, total = None, 0
    for q, (lo, hi) in enumerate(eng.slab_cuts(len(x), 3)):  # the oracle's own slab chain
        rec, st = orc.trace_slab(dom, orc.default_t_end(ext), "z", lo, hi, s0=g["s0"] if q == 0 else None, rec=rec, last=q == 2)
    d_amp, d_pol = np.max(np.abs(rec[6] - g["s0"][6])), np.max(np.abs(rec[8] - g["s0"][8]))
    assert np.max(np.abs(sf[6] - rec[6])) <= 1e-12 * d_amp and np.max(np.abs(sf[8] - rec[8])) <= 1e-12 * d_pol
    assert np.max(np.abs(sf[:3] - rec[:3])) <= 1e-13


def test_slab_lost_rays_and_state_errors(eng, orc):
    g = golden("g2_trace_blob32_z_s0")
    x, ext = g["x"], float(g["extent"])
    s0 = g["s0"].copy()
    s0[5, :7] *= -1.0
    s0[2, 7:9] = 0.0
    cuts = eng.slab_cuts(len(x), 2)
    (sf, rf, Jf), _ = _slab_chain(eng, g, "z", cuts, "mixed", s0=s0, requeued=9)
    assert np.isnan(sf[:, :9]).all() and np.isnan(rf[:, :9]).all() and not np.isnan(sf[:, 9:]).any()
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    ref = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision="mixed")[0]
    assert np.array_equal(sf[:, 9:], ref[:, 9:])
    # a slab cannot be traced as a whole volume, rays cannot start on a later slab or finish on an earlier one
    lo, hi = cuts[1]
    part = eng.Volume.from_ne_slab(eng.slab_source(g["ne"], 2, lo, hi), x, x, x, float(g["lwl"]), "z", lo, hi)
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    for flags in (0, eng.HANDOFF_EXIT):
        with pytest.raises(RuntimeError):
            rays.trace(part, eng.default_t_end(ext), ext, handoff=flags)
    with pytest.raises(RuntimeError, match="without hand-off records"):
        rays.trace(part, eng.default_t_end(ext), ext, handoff=eng.HANDOFF_ENTER)
    with pytest.raises(RuntimeError):
        rays.handoff_download()


def test_slab_pipeline_two_processes_one_gpu(tmp_path):
    """Config 5's pipeline with the real stage: two processes (both on this box's one GPU), each holding one slab,
    ragged chunks handed over through gloo (transport "host"; the RCCL transport needs one GPU per rank and is the
    driver's 8-GPU run); the last rank checks final states and the detector image against the whole-volume trace."""
    import textwrap

    from test_distributed_gloo import _run_workers

    worker = textwrap.dedent("""
        import os, sys
        import numpy as np
        sys.path.insert(0, {root!r})
        sys.path.insert(0, os.path.join({root!r}, "tests"))
        from conftest import golden
        from synthpy_amd import engine as eng
        from synthpy_amd.distributed import RayShardGroup, SlabPipeline

        grp = RayShardGroup(timeout_s=120)
        eng.init_rank(grp.local_rank, grp.local_world, shared=True)  # both ranks open the one GPU in the same instant (sr_device_count)
        g = golden("g2_trace_turb32_z_s0")
        x, ext, lwl = g["x"], float(g["extent"]), float(g["lwl"])
        sizes = [100, 56, 100]
        offs = [0, 100, 156]
        pipe = SlabPipeline(grp, transport="host")
        lo, hi = eng.slab_cuts(len(x), grp.world)[grp.rank]
        vol = eng.Volume.from_ne_slab(eng.slab_source(g["ne"], 2, lo, hi), x, x, x, lwl, "z", lo, hi, phaseshift=True)
        img = eng.DetectorImage.counts(bin_scale=10)
        steps, finished = pipe.trace_chunks(vol, ext, sizes, lambda n, ci: g["s0"][:, offs[ci]:offs[ci] + n],
                                            deposits=[(img, eng.chain_shadow_two(), {{}})])
        grp.barrier()
        if pipe.last:
            whole = eng.Volume.from_ne(g["ne"], x, x, x, lwl, "z", phaseshift=True)
            rays = eng.RayBundle(256).upload(g["s0"])
            rays.trace(whole, eng.default_t_end(ext), ext)
            ref = eng.DetectorImage.counts(bin_scale=10)
            rays.deposit(ref, eng.chain_shadow_two())
            assert finished == 256 and np.array_equal(img.download(), ref.download()) and img.download().sum() > 200
            print("PIPE OK", steps)
        grp.close()
    """)
    outs = _run_workers(tmp_path, worker, 2)
    assert "PIPE OK" in outs[-1]


@pytest.mark.parametrize("scaling", ["strong", "weak"])
def test_bench_n_gt_1_job_rehearsed_on_one_gpu(scaling):
    """`python bench.py --gpus 2` as the driver types it, on real kernels: the command starts its own two ranks; with
    --rehearse-shared-gpu both open this box's one GPU and the image sum goes through gloo (RCCL refuses two ranks on one
    device).  One JSON line, and the N > 1 checks: the summed image == the sum of the ranks' deposits == ONE GPU tracing
    every rank's rays (counts exact, interferogram sums to rounding)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--rehearse-shared-gpu", "--scaling", scaling, "--grid", "96",
           "--rays", "200000", "--steps", "1", "--warmup", "0", "--full", "--cpu-sample", "0", "--other-steps", "0", "--spawn-timeout", "240"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    d = json.loads(lines[0])
    m = d["check"]["multi_gpu"]
    assert d["n_gpus"] == 2 and d["scaling"] == scaling and d["value"] is None and "rehearsal" in d
    assert d["config"]["rays_all_gpus"] == (200000 if scaling == "strong" else 400000)
    assert m["ranks_seen"] == 2 and m["comm_ranks_consistent"] and m["counts_sum_equals_sum_of_deposited"]
    assert m["counts_image_equals_single_gpu_image"] and m["interferogram_sums_max_diff_over_max"] < 1e-12
    assert m["deposited_rays_all_ranks"] > 0.9 * d["config"]["rays_all_gpus"]


def test_bench_says_so_when_rccl_cannot_sum_the_images():
    """A host on which RCCL cannot start (here: two ranks on this box's one GPU, which RCCL refuses for real -- sr_comm_create
    returns its error on every rank) must not cost the whole N > 1 line and must not pass silently either: the ranks agree over
    the control plane, say so on stderr, sum the images through the host, and the line is marked (`collective`, `rccl_failed`).
    The checks of the sum itself are those of the rehearsal."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--shared-gpu-rccl", "--grid", "96", "--rays", "200000",
           "--steps", "1", "--warmup", "0", "--full", "--cpu-sample", "0", "--other-steps", "0", "--spawn-timeout", "240"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "RCCL COULD NOT SUM THE IMAGES" in res.stderr
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    d = json.loads(lines[0])
    assert d["collective"].startswith("HOST FALLBACK, NOT RCCL") and "rccl_failed" in d
    assert d["value"] is None and d["rays_per_s"] is None and d["value_with_the_host_sum"] > 0  # a host sum is not the N-GPU metric
    m = d["check"]["multi_gpu"]
    assert m["ranks_seen"] == 2 and m["counts_sum_equals_sum_of_deposited"] and m["counts_image_equals_single_gpu_image"]


def test_bench_plain_run_is_the_job_and_dumps_what_it_computed(tmp_path):
    """`python bench.py` without --full: set-up, warm-up, the timed steps and one line -- the other build, the oracle check, the CPU
    baseline and the API flow are --full's (null here, present there).  --dump-outputs writes the timed path's results; with the
    same arguments the two runs (plain and --full) dump the same exit rays bit for bit and the same interferogram to rounding."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--grid", "96", "--rays", "200000", "--steps", "3", "--warmup", "1"]
    lines = {}
    for tag, extra in (("plain", []), ("full", ["--full", "--cpu-sample", "20000", "--other-steps", "1", "--api-flow-reps", "1"])):
        res = subprocess.run(base + extra + ["--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        out = [ln for ln in res.stdout.splitlines() if ln.strip()]
        assert len(out) == 1, res.stdout
        lines[tag] = json.loads(out[0])
    p, f = lines["plain"], lines["full"]
    for d in (p, f):
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "ray-steps/s"
        assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["config"]["precision"] == "f64"
    assert p["full"] is False and all(p[k] is None for k in ("check", "cpu_baseline", "other_build", "api_flow"))
    assert f["full"] is True and all(f[k] is not None for k in ("check", "cpu_baseline", "other_build", "api_flow"))
    assert "max_dx_m" in f["check"] and f["other_build"]["steps"] == 1
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) == sorted(
        ["rays_index.npy", "rays_sf.npy", "rays_rf.npy", "rays_Jf_re.npy", "rays_Jf_im.npy", "image_interferogram.npy"])
    assert sum(os.path.getsize(tmp_path / "plain" / n) for n in names) <= 64 * 2 ** 20
    a = {n[:-4]: np.load(tmp_path / "plain" / n) for n in names}
    b = {n[:-4]: np.load(tmp_path / "full" / n) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["rays_rf"].shape == (4, 2 ** 17) and a["rays_sf"].shape == (9, 2 ** 17) and a["image_interferogram"].shape == (2573, 3447)
    for k in ("rays_index", "rays_sf", "rays_rf", "rays_Jf_re", "rays_Jf_im"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.isfinite(a["rays_rf"]).sum() > 0.9 * a["rays_rf"].size
    Ha, Hb = a["image_interferogram"].astype(np.float64), b["image_interferogram"].astype(np.float64)
    assert Ha.max() > 0 and np.max(np.abs(Ha - Hb)) <= 1e-5 * Ha.max()


# ---------------------------------------------------------------- the step before the path: volume synthesis on the GPU
def test_domain_fft_on_device_vs_reference(eng):
    """gaussian3D.domain_fft(device=True): seeded, against the field the reference generated (fixture g0_domain_fft)
    and against the host path; FFT rounding only (1e-12 of the unit-normalised field)."""
    from synthpy_amd.field_generator.gaussian3D import gaussian3D

    g = golden("g0_domain_fft")
    np.random.seed(int(g["seed"]))
    f = gaussian3D(lambda k: k ** (-11 / 3)).domain_fft(float(g["l_max"]), float(g["l_min"]), int(g["extent"]), int(g["res"]),
                                                       float(g["factor"]), device=True)
    assert f.shape == g["field"].shape and np.max(np.abs(f - g["field"])) <= 1e-12 and np.max(np.abs(f)) == 1.0
    for res, factor in ((24, 1.0), (20, 0.5)):  # a non-power-of-two and a non-cubic grid
        np.random.seed(7)
        a = gaussian3D(lambda k: k ** (-11 / 3)).domain_fft(1.0, 0.05, 5, res, factor)
        np.random.seed(7)
        b = gaussian3D(lambda k: k ** (-11 / 3)).domain_fft(1.0, 0.05, 5, res, factor, device=True)
        assert a.shape == b.shape == (2 * res, 2 * res, int(2 * res * factor)) and np.max(np.abs(a - b)) <= 1e-12


def test_radial_2Dspectrum_vs_reference(eng):
    """After the path: radial_2Dspectrum of an image (power_spectrum.py:372-421) against the reference's output:
    same wavenumber bins, the same empty (NaN) bins, bin means to 1e-12 (FFT and summation order)."""
    from synthpy_amd.utils.power_spectrum import radial_2Dspectrum

    g = golden("g7_spectrum")
    for tag in "abc":
        lx, ly = g[f"l_{tag}"]
        kn, kc, sp = radial_2Dspectrum(g[f"img_{tag}"], lx, ly)
        assert kn == pytest.approx(float(g[f"kn_{tag}"]), rel=1e-15) and np.allclose(kc, g[f"kc_{tag}"], rtol=1e-14, atol=0)
        ref = g[f"sp_{tag}"]
        assert np.array_equal(np.isnan(sp), np.isnan(ref)) and np.isnan(ref).sum() < 60
        ok = ~np.isnan(ref)
        assert np.max(np.abs(sp[ok] - ref[ok]) / ref[ok]) <= 1e-12, tag
        _, _, sps = radial_2Dspectrum(g[f"img_{tag}"], lx, ly, smooth=True)
        m = ~np.isnan(g[f"sps_{tag}"])
        assert np.array_equal(np.isnan(sps), ~m) and np.allclose(sps[m], g[f"sps_{tag}"][m], rtol=1e-11)
    # a whole (non-square) detector image: total power is conserved by the binning
    img = np.random.default_rng(0).poisson(20, (257, 344)).astype(float)
    kn, kc, sp = radial_2Dspectrum(img, 13.5, 18.0)
    assert sp.shape == (99,) and np.nanmax(sp) > 0


# ---------------------------------------------------------------- BASELINE.json configs[0] and [1], end to end
@pytest.mark.parametrize("precision", ["auto", "f64", "mixed"])
def test_config_c1_end_to_end(eng, orc, precision):
    """C1: 1e4 rays x 64^3 analytic Gaussian blob, two-lens shadowgraphy, through the legacy API mirror.  Histogram
    against the reference's tight run (first 2000 rays): EXACT; against the oracle on all 1e4 rays FROM s0: exact with the
    default precision ("auto": rf goes back to the caller, so float64) and with "f64"; the mixed build asked for by name
    may put a ray in the neighbouring bin (1e-11 m at a bin edge: at most 2 rays); against the reference as shipped (RK45
    rtol 1e-3): same total, within the reference's own integration error."""
    from test_oracle_golden import _c1_inputs
    from synthpy_amd.solvers_legacy import full_solver as fs, rtm_solver as rtm

    g = golden("g8_config1")
    x, ne, s0 = _c1_inputs(g)
    ext, M = float(g["extent"]), int(g["M"])
    d = fs.ScalarDomain(x, x, x, ext)
    d.precision = precision
    d.external_ne(ne)
    d.calc_dndr(float(g["lwl"]))
    np.random.seed(int(g["seed"]))
    assert np.array_equal(fs.init_beam(int(g["N"]), float(g["beam_size"]), float(g["divergence"]), ext, "circular", "z"), s0)
    rf = d.solve(s0)
    assert np.max(np.abs(rf[0::2, :M] - g["rf_tight"][0::2])) <= 1e-8 and np.max(np.abs(rf[1::2, :M] - g["rf_tight"][1::2])) <= 1e-6
    sh = rtm.Shadowgraphy(rf[:, :M].copy()); sh.two_lens_solve(); sh.histogram(bin_scale=10)
    assert np.array_equal(sh.H, g["H_tight"])
    sh = rtm.Shadowgraphy(rf.copy()); sh.two_lens_solve(); sh.histogram(bin_scale=10)
    dom = orc.Domain.from_ne(ne, x, x, x, float(g["lwl"]))
    sf_o, _ = orc.trace_rk4(dom, s0, (x[1] - x[0]) / orc.c, orc.default_t_end(ext), "z", "planes", 1)
    r_o, _ = orc.optics(orc.optics(orc.ray_to_jones(sf_o, ext, "z")[0], [(orc.SCALE, 1e3)])[0], orc.chain_shadow_two())
    H_o = orc.histogram(r_o, bin_scale=10)
    diff = np.abs(sh.H - H_o).sum()
    assert diff == 0 if precision != "mixed" else diff <= 4
    Hd = g["H_default"].astype(np.float64)
    assert sh.H.sum() == Hd.sum() == 10000 and np.abs(sh.H - Hd).sum() <= 0.02 * Hd.sum()


def _counts_from_s0(eng, orc, ne, x, s0, lwl=1064e-9, ext=5e-3, bin_scale=1, t_end_factor=1.0):
    """The DEFAULT device-resident flow (RayBundle.trace precision "auto" -> deposit) and the oracle's flow from the same
    s0, for the three counts diagnostics: [(name, H_gpu, H_oracle, retraced)], the bundle and the oracle's exit rays."""
    vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z")
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    assert eng.resolve_precision("auto", vol) == "mixed"
    rays.trace(vol, t_end_factor * eng.default_t_end(ext), ext)
    dom = orc.Domain.from_ne(ne, x, x, x, lwl)
    so, _ = orc.trace_rk4(dom, s0, (x[1] - x[0]) / orc.c, t_end_factor * orc.default_t_end(ext), "z", "planes", 1)
    ro, _ = orc.ray_to_jones(so, ext, "z")
    out = []
    for name, ce, co in (("shadow two-lens", eng.chain_shadow_two(), orc.chain_shadow_two()),
                         ("schlieren DF", eng.chain_schlieren(), orc.chain_schlieren()),
                         ("refractometry", eng.chain_refractometry(), orc.chain_refractometry())):
        img = eng.DetectorImage.counts(bin_scale=bin_scale)
        rays.deposit(img, ce)
        r_o, _ = orc.optics(orc.m_to_mm(ro), co)
        out.append((name, img.download(), orc.histogram(r_o, bin_scale=bin_scale), rays.retraced))
    return out, rays, vol, ro


def test_default_counts_equal_oracle_from_s0_c1(eng, orc):
    """north_star: "bit-exact for the integer histogram counts".  C1 (all 1e4 rays, 64^3 Gaussian blob) through the DEFAULT
    device-resident flow -- mixed-precision trace + the deposit's edge guard (rtm_solver.py:156-178 = np.histogram2d's
    rules) -- against the oracle FROM THE SAME s0: two-lens shadowgraphy, dark-field schlieren and refractometry, at the
    full detector resolution and at bin_scale 10, every count equal."""
    from test_oracle_golden import _c1_inputs

    g = golden("g8_config1")
    x, ne, s0 = _c1_inputs(g)
    for bs in (1, 10):
        res, rays, vol, _ = _counts_from_s0(eng, orc, ne, x, s0, float(g["lwl"]), float(g["extent"]), bs)
        for name, H, H_o, n_again in res:
            assert H.sum() == H_o.sum() and np.array_equal(H, H_o.astype(np.uint32)), (name, bs)
            assert n_again <= 0.05 * s0.shape[1], (name, n_again)
    # a caller's t_end five times the default: rf is the back-projection onto the plane `extent` along the same straight line the
    # rays flew after the volume, so the edge guard's position bound (sr_rays.guard_len: the volume's length + the distance from its
    # last node plane to that plane) does not grow with t_end, and the images stay the oracle's
    res, rays, vol, _ = _counts_from_s0(eng, orc, ne, x, s0, float(g["lwl"]), float(g["extent"]), 1, t_end_factor=5.0)
    for name, H, H_o, n_again in res:
        assert np.array_equal(H, H_o.astype(np.uint32)), (name, "t_end x 5")


@pytest.mark.parametrize("grid", [256, 512])
def test_default_counts_equal_oracle_from_s0_turbulence(eng, orc, grid):
    """The same on BASELINE's turbulent volumes: a 2e5-ray sample of C2 (256^3) and of C4's per-GPU share (512^3), default
    precision, full-resolution detector (5.2 um bins): H_gpu == H_oracle from s0 for the three counts diagnostics.  Also
    reported: the share of rays the guard traced again (refractometry maps angle to position and has the largest: its
    lever is a few hundred mm per radian), and that WITHOUT the guard the mixed build's image is not guaranteed."""
    import bench

    ne, x = bench.make_volume(grid)
    N = 200_000
    s0 = bench.make_rays(N, 5e-3, 0)
    res, rays, vol, ro = _counts_from_s0(eng, orc, ne, x, s0)
    for name, H, H_o, n_again in res:
        assert np.array_equal(H, H_o.astype(np.uint32)), (name, int(np.abs(H.astype(np.int64) - H_o.astype(np.int64)).sum()))
        assert n_again <= 0.05 * N, (name, n_again)
        print(f"{grid}^3 {name}: counts equal to the oracle's from s0; {n_again} of {N} rays traced again ({100.0 * n_again / N:.2f} %)")
    # a second pass over the same bundle finds (almost) nothing left to refine: the refined rays carry bound 0
    img = eng.DetectorImage.counts()
    rays.deposit(img, eng.chain_refractometry())
    assert rays.retraced == 0 and np.array_equal(img.download(), res[2][1])
    # sr_rays_refine: ONE re-trace for the three diagnostics, then plain deposits -- the same images
    rays.trace(vol, eng.default_t_end(5e-3), 5e-3)
    imgs = [eng.DetectorImage.counts() for _ in range(3)]
    chains = [eng.chain_shadow_two(), eng.chain_schlieren(), eng.chain_refractometry()]
    n_all = rays.refine(list(zip(imgs, chains)))
    assert 0 < n_all <= sum(r[3] for r in res)
    for im, ch, (name, H, H_o, _) in zip(imgs, chains, res):
        rays.deposit(im, ch, exact_counts=False)
        assert np.array_equal(im.download(), H_o.astype(np.uint32)), name


def test_edge_guard_bound_holds(eng, orc):
    """The per-ray bound the mixed kernel writes (trace_mx.inc: 8 * 2^-24 * sum |lateral velocity change| / v_a) against
    what it bounds: the difference between the mixed build's and the float64 build's exit rays, on 1e6 rays through the
    256^3 turbulent volume and on the C1 blob (coherent deflection).  The largest |d angle| / bound and
    |d position| / (length * bound) stay below 1/2."""
    import bench
    from test_oracle_golden import _c1_inputs

    g = golden("g8_config1")
    xb, neb, s0b = _c1_inputs(g)
    ne, x = bench.make_volume(256)
    worst = {}
    for tag, (ne_, x_, s0_) in {"turbulence 256^3": (ne, x, bench.make_rays(10 ** 6, 5e-3, 0)), "blob 64^3": (neb, xb, s0b)}.items():
        vol = eng.Volume.from_ne(ne_, x_, x_, x_, 1064e-9, "z")
        rays = eng.RayBundle(s0_.shape[1]).upload(s0_)
        t_end, ext = eng.default_t_end(5e-3), 5e-3
        rays.trace(vol, t_end, ext, precision="f64")
        _, rf64, _ = rays.download(sf=False, Jf=False)
        assert not rays.error_bound().any()
        rays.trace(vol, t_end, ext, precision="mixed")
        _, rfm, _ = rays.download(sf=False, Jf=False)
        b = rays.error_bound().astype(np.float64)
        ok = np.isfinite(rfm).all(axis=0) & np.isfinite(rf64).all(axis=0) & (b > 0)
        assert ok.sum() > 0.99 * ok.size
        d_ang = np.maximum(np.abs(rfm[1] - rf64[1]), np.abs(rfm[3] - rf64[3]))[ok]
        d_pos = np.maximum(np.abs(rfm[0] - rf64[0]), np.abs(rfm[2] - rf64[2]))[ok]
        length = float(x_[-1] - x_[0])
        worst[tag] = (float(np.max(d_ang / b[ok])), float(np.max(d_pos / (length * b[ok]))), float(np.median(b[ok])))
        print(f"{tag}: max |d angle| / bound {worst[tag][0]:.3f}, max |d pos| / (L * bound) {worst[tag][1]:.3f}, median bound {worst[tag][2]:.2e} rad")
        assert worst[tag][0] < 0.5 and worst[tag][1] < 0.5, (tag, worst[tag])



def test_tile_kernel_is_bit_identical_to_the_per_ray_kernel(eng, monkeypatch):
    """k_trace_tile (coefficients once per workgroup in LDS, trace_tile.inc) against k_trace_f64 (everything per ray) on the
    same launch: sf, rf, Jf equal bit for bit, NaN for NaN, and the same step and fallback counts -- a collimated beam
    through turbulence (rays that stay in their tiles), one segment and several (re-binning in between), small tiles and
    short segments (many rays leave their tile and are carried through that segment by k_trace_f64, from record to record),
    a strongly divergent beam that overfills the volume (rays outside it, lateral exits and entries), with and without the
    phase integral.  The library's own choice (no SYNTHRAY_F64_TILE) is the tile path for a dense bundle, the per-ray
    kernel for a sparse one."""
    import bench
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    ne, x = bench.make_volume(128)
    ext, lwl = 5e-3, 1064e-9
    t_end = eng.default_t_end(ext)
    np.random.seed(5)
    beams = {"collimated": init_beam(400_000, 4e-3, 5e-5, ext, "circular", "z"),
             "divergent, overfilling": init_beam(200_000, 6e-3, 2e-2, ext, "circular", "z")}
    beams["collimated"][:, :7] = np.nan  # NaN rays and a ray flying backwards: not plane-form rays
    beams["collimated"][5, 7:9] *= -1
    for phase in (True, False):
        vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=phase)
        for tag, s0 in beams.items():
            rays = eng.RayBundle(s0.shape[1]).upload(s0)
            monkeypatch.setenv("SYNTHRAY_F64_TILE", "0")
            st0 = rays.trace(vol, t_end, ext, precision="f64")
            assert rays.tile_segments == 0
            ref = rays.download()
            # (geometry, records): tiles of eight rows run the records kernel unless told not to (a tile column = one DMA's kilobyte)
            for geom, recs in (("8,7,2,4,32", "1"), ("8,8,2,2,171", "1"), ("8,8,2,2,43", "1"), ("8,8,2,2,43", "0"), ("8,5,1,3,16", "1"),
                               ("12,16,4,4,32", "1"), ("6,8,1,4,16", "1"), ("16,12,4,8,40", "1")):
                monkeypatch.setenv("SYNTHRAY_F64_TILE", "1")
                monkeypatch.setenv("SYNTHRAY_TILE", geom)
                monkeypatch.setenv("SYNTHRAY_TILE_RECORDS", recs)
                st1 = rays.trace(vol, t_end, ext, precision="f64")
                assert rays.tile_segments == -(-127 // int(geom.split(",")[-1]))  # 127 cell layers in segments of that many planes
                assert rays.tile_records == (geom.startswith("8,") and recs == "1"), (geom, recs)
                geom = geom + (" records" if rays.tile_records else " producers")
                got = rays.download()
                for a, b, name in zip(ref, got, ("sf", "rf", "Jf")):
                    assert np.array_equal(a, b, equal_nan=True), (tag, phase, geom, name, int((a != b).sum()))
                assert st1.ray_steps == st0.ray_steps, (tag, geom)
                # rays a tile lost were carried through their segment by k_trace_f64 from their records (k_first / k_last)
                # and are back in the bundle: with small tiles or a divergent beam that is many rays, in every segment
                if geom.startswith(("6,8", "8,5")) or tag != "collimated":
                    assert st1.fallback_rays > 1000, (tag, geom, st1.fallback_rays)
                print(f"{tag}, phase {phase}, tile {geom}: identical; {st1.fallback_rays} of {s0.shape[1]} rays through k_trace_f64 (per-ray kernel alone: {st0.fallback_rays} to the time-stepping form)")
            rays.close()
        vol.close()
    # non-uniform node coordinates on all three axes (the tile's own node tables, the step table, np.gradient's other branch)
    rng = np.random.default_rng(11)
    xs = [np.sort(x + rng.uniform(-0.3, 0.3, x.size) * (x[1] - x[0])) for _ in range(3)]
    for q in xs:
        q[0], q[-1] = x[0], x[-1]
    vol = eng.Volume.from_ne(ne, xs[0], xs[1], xs[2], lwl, "z", phaseshift=True)
    s0 = beams["collimated"]
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    for prec, var in (("f64", "SYNTHRAY_F64_TILE"),):
        monkeypatch.setenv(var, "0")
        st0 = rays.trace(vol, t_end, ext, precision=prec)
        ref = rays.download()
        monkeypatch.setenv(var, "1")
        monkeypatch.setenv("SYNTHRAY_TILE", "12,16,4,4,40")
        st1 = rays.trace(vol, t_end, ext, precision=prec)
        assert rays.tile_segments == 4 and st1.ray_steps == st0.ray_steps
        for a, b, name in zip(ref, rays.download(), ("sf", "rf", "Jf")):
            assert np.array_equal(a, b, equal_nan=True), ("non-uniform grid", prec, name, int((a != b).sum()))
        monkeypatch.delenv(var)
    rays.close()
    vol.close()
    # the other probing axes (the packed node order follows the axis; y-probing has the legacy row order of rf)
    for axis in ("x", "y"):
        vol = eng.Volume.from_ne(ne, x, x, x, lwl, axis, phaseshift=True)
        np.random.seed(8)
        s0a = init_beam(200_000, 4e-3, 5e-5, ext, "circular", axis)
        rays = eng.RayBundle(s0a.shape[1]).upload(s0a)
        monkeypatch.setenv("SYNTHRAY_F64_TILE", "0")
        st0 = rays.trace(vol, t_end, ext, precision="f64")
        ref = rays.download()
        monkeypatch.setenv("SYNTHRAY_F64_TILE", "1")
        monkeypatch.setenv("SYNTHRAY_TILE", "8,8,2,2,43")
        st1 = rays.trace(vol, t_end, ext, precision="f64")
        assert rays.tile_segments == 3 and st1.ray_steps == st0.ray_steps == 127 * s0a.shape[1]
        for a, b, name in zip(ref, rays.download(), ("sf", "rf", "Jf")):
            assert np.array_equal(a, b, equal_nan=True), (axis, name, int((a != b).sum()))
        # what the tile path does not take, forced or not: unsorted launches, sub-steps, the optional terms
        rays.trace(vol, t_end, ext, precision="f64", sort_rays=False)
        assert rays.tile_segments == 0
        rays.trace(vol, t_end, ext, precision="f64", substeps=2)
        assert rays.tile_segments == 0
        monkeypatch.delenv("SYNTHRAY_F64_TILE")
        rays.close()
        vol.close()
    # the library's choice: >= 8 rays per lateral cell of the BEAM's bounding box (found at upload) -> the float64 tile path (the
    # measured break-even, profiles/r04_tile_variants.txt); the mixed one is opt-in.  A beam over the whole grid: 8 / 7 rays per
    # cell of the grid; the same 7 per grid cell drawn into a beam of 4 mm radius (64 % of the grid's cells in its box) are 11 per
    # cell there: tiled
    monkeypatch.delenv("SYNTHRAY_TILE")
    vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)
    for per_cell, radius, tiled64 in ((8, 5e-3, True), (7, 5e-3, False), (7, 4e-3, True)):
        n_rays = 127 * 127 * per_cell
        rays = eng.RayBundle(n_rays).upload(init_beam(n_rays, radius, 5e-5, ext, "circular", "z"))
        rays.trace(vol, t_end, ext, precision="f64")
        assert (rays.tile_segments > 0) == tiled64, (n_rays, radius, rays.tile_segments)
    # a device-drawn bundle knows its box from the beam's parameters (no kernel, no wait)
    for radius, tiled64 in ((1e-3, True), (5e-3, False)):
        rays = eng.RayBundle(100000).generate(radius, 5e-5, ext, "circular", "z", seed=3)
        rays.trace(vol, t_end, ext, precision="f64")
        assert (rays.tile_segments > 0) == tiled64, (radius, rays.tile_segments)
        rays.trace(vol, t_end, ext, precision="mixed")
        assert rays.tile_segments == 0
        rays.trace(vol, t_end, ext, precision="f64", substeps=2)  # sub-steps: the per-ray kernel
        assert rays.tile_segments == 0
        rays.close()
    vol.close()


def test_config_c2_end_to_end_sample(eng, orc):
    """C2: 256^3 power-law turbulent n_e, shadowgraphy + dark-field schlieren, 1e6 rays on the GPU; the first 2e4 rays
    against the oracle (positions / angles as in the mixed-precision tolerance), counts summing to the rays that reach
    the detector, and the fused device deposit equal to the host-buffer path (counts FROM s0 against the oracle:
    test_default_counts_equal_oracle_from_s0_turbulence)."""
    import bench

    ne, x = bench.make_volume(256)
    ext, lwl, N, ns = 5e-3, 1064e-9, 10 ** 6, 20000
    s0 = bench.make_rays(N, ext, 0)
    vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z")
    rays = eng.RayBundle(N).upload(s0)
    st = rays.trace(vol, eng.default_t_end(ext), ext)
    assert st.ray_steps == 255 * N and st.fallback_rays == 0
    sf, rf, _ = rays.download(Jf=False)
    dom = orc.Domain.from_ne(ne, x, x, x, lwl)
    so, _ = orc.trace_rk4(dom, s0[:, :ns], (x[1] - x[0]) / orc.c, orc.default_t_end(ext), "z", "planes", 1)
    ro, _ = orc.ray_to_jones(so, ext, "z")
    assert np.max(np.abs(rf[0::2, :ns] - ro[0::2])) <= 5e-11 and np.max(np.abs(rf[1::2, :ns] - ro[1::2])) <= 2e-8
    for chain in (eng.chain_shadow_two(), eng.chain_schlieren()):
        img = eng.DetectorImage.counts(bin_scale=1)
        _, hit = rays.deposit(img, chain, exact_counts=False)  # the mixed build's rays as they are: rf above is what was binned
        H = img.download()
        r_host = eng.optics(eng.optics(rf, [(eng.OP_SCALE, 1e3)])[0], chain)[0]
        H_host = eng.hist2d(r_host[0], r_host[2], 3448, 2574, -9.0, 9.0, -6.75, 6.75)
        assert int(H.sum()) == hit == int(H_host.sum()) and np.array_equal(H, H_host)
        assert hit > 0.5 * N if chain is not None else True


def test_simulator_region_count_equals_whole_volume(eng):
    """ScalarDomain(region_count=R) (the reference's region loop, propagator.py:366-452): traced slab by slab with the
    rays handed over on the shared planes -- same rf, Jf as the whole volume, bit for bit."""
    from synthpy_amd.simulator import beam, domain as d, propagator as p

    ext = 5e-3
    whole = d.ScalarDomain(2 * ext, 40, ne_type="test_exponential_cos", phaseshift=True)
    parts = d.ScalarDomain(2 * ext, 40, ne_type="test_exponential_cos", phaseshift=True, region_count=3)
    b = beam.Beam(3000, 4e-3, 5e-5, ext, probing_direction="z", wavelength=1064e-9, seeded=True)
    rf1, Jf1, _ = p.solve(b.s0, whole, ext, return_E=True)
    rf3, Jf3, _ = p.solve(b.s0, parts, ext, return_E=True)
    assert parts.region_count == 3 and np.array_equal(rf1, rf3) and np.array_equal(Jf1, Jf3)
    assert p.solve.last_stats.ray_steps == 39 * 3000


def test_simulator_region_count_with_optional_terms(eng):
    """region_count = R with inv_brems / B_on (the region loop of propagator.py:366-452 with dsdt's optional terms,
    :137-165): every slab gets its own node planes of kappa, n_e and B -- same rf, Jf as the whole volume, bit for bit."""
    from synthpy_amd.simulator import beam, domain as d, propagator as p

    ext, n = 5e-3, 36
    kw = dict(ne_type="test_exponential_cos", phaseshift=True, inv_brems=True, B_on=True)
    whole = d.ScalarDomain(2 * ext, n, **kw)
    parts = d.ScalarDomain(2 * ext, n, region_count=3, **kw)
    X, Y, Z = np.meshgrid(np.asarray(whole.x), np.asarray(whole.y), np.asarray(whole.z), indexing="ij", sparse=True)
    B = np.stack(np.broadcast_arrays(3.0 * Y / ext, -2.0 * X / ext + 1.0, 8.0 * (1 + Z / ext) + 0 * X), -1)
    for dom in (whole, parts):
        dom.external_Te(np.full((n, n, n), 200.0) * (1 + 0.1 * np.cos(2e2 * X)))
        dom.external_Z(np.full((n, n, n), 3.5))
        dom.external_B(np.ascontiguousarray(B))
    b = beam.Beam(2000, 4e-3, 5e-5, ext, probing_direction="z", wavelength=1064e-9, seeded=True)
    rf1, Jf1, _ = p.solve(b.s0, whole, ext, return_E=True)
    rf3, Jf3, _ = p.solve(b.s0, parts, ext, return_E=True)
    assert np.array_equal(rf1, rf3) and np.array_equal(Jf1, Jf3)
    assert np.abs(np.abs(Jf1[1]) - 1).max() > 1e-6  # the amplitude did change: the terms were on
    # auto_batching: with room in HBM the volume is traced whole; told that (almost) nothing is free, in regions -- same result
    auto = d.ScalarDomain(2 * ext, n, **kw)
    for src in ("Te", "Z", "B"):
        setattr(auto, src, getattr(whole, src))
    assert auto.auto_batching and auto.regions_for_memory() == 1
    need = eng.volume_bytes_estimate(n ** 3, True, True, True) * auto.leeway_factor
    auto.regions_for_memory = lambda free_bytes=None: d.ScalarDomain.regions_for_memory(auto, int(need / 3.5))
    rfa, Jfa, _ = p.solve(b.s0, auto, ext, return_E=True)
    # the decision is kept beside region_count (which stays the caller's), once per domain: a second solve() does not ask again
    assert auto.region_count == 1 and auto._auto_regions[1] == 4 and np.array_equal(rf1, rfa) and np.array_equal(Jf1, Jfa)
    auto.regions_for_memory = lambda free_bytes=None: 1 / 0
    rfb, _, _ = p.solve(b.s0, auto, ext, return_E=False)
    assert np.array_equal(rf1, rfb)


@pytest.mark.parametrize("pd", ["z", "x"])
def test_non_uniform_grid_vs_oracle(eng, orc, pd):
    """A genuinely non-uniform (stretched) grid on every axis: np.gradient's non-uniform branch, scipy's cell search and
    per-cell widths, and the tracer's node-plane steps of unequal length -- gradients bit-exact against the oracle,
    traces within the usual tolerances in both builds."""
    rng = np.random.default_rng(12)
    n, ext = (30, 26, 34), 5e-3
    axes = []
    for m in n:
        w = 1.0 + 0.6 * rng.random(m - 1)  # cell widths vary by up to 60 %
        c = np.concatenate([[0.0], np.cumsum(w)])
        axes.append((2 * c / c[-1] - 1) * ext)
    x, y, z = axes
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij", sparse=True)
    ne = 1e25 * np.exp(-(X ** 2 + 1.3 * Y ** 2 + 0.8 * Z ** 2) / (2e-3) ** 2) * (1 + 0.2 * np.sin(3e3 * X + 2e3 * Y) * np.cos(2.5e3 * Z))
    lwl = 1064e-9
    vol = eng.Volume.from_ne(ne, x, y, z, lwl, pd, phaseshift=True)
    om, gx, gy, gz = orc.calc_dndr(ne, x, y, z, lwl)
    fx, fy, fz, nm1 = vol.fields(phase=True)
    assert np.array_equal(fx, gx) and np.array_equal(fy, gy) and np.array_equal(fz, gz)
    np.random.seed(2)
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    s0 = init_beam(2000, 3.5e-3, 2e-3, ext, "circular", pd)  # a divergent beam: rays cross many cells
    dom = orc.Domain.from_ne(ne, x, y, z, lwl, phaseshift=True)
    dt = float(np.float32(z)[1] - np.float32(z)[0]) / orc.c
    so, steps = orc.trace_rk4(dom, s0, dt, orc.default_t_end(ext), pd, "planes", 1)
    ro, _ = orc.ray_to_jones(so, ext, pd)
    for precision, tol_x, tol_a in (("f64", 1e-13, 1e-11), ("mixed", 5e-11, 2e-8)):
        sf, rf, Jf, st = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision=precision, dt=dt)
        assert st.ray_steps == steps
        assert np.max(np.abs(rf[0::2] - ro[0::2])) <= tol_x and np.max(np.abs(rf[1::2] - ro[1::2])) <= tol_a, precision
    for tile in (0, 1, 2):  # each float64 plane kernel by name; the tile kernels' node table and cell search on unequal cells
        sf, rf, Jf, st = _forced_kernel_trace(eng, vol, s0, eng.default_t_end(ext), ext, tile, precision="f64", dt=dt)
        assert st.ray_steps == steps
        assert np.max(np.abs(rf[0::2] - ro[0::2])) <= 1e-13 and np.max(np.abs(rf[1::2] - ro[1::2])) <= 1e-11, tile
        assert np.max(np.abs(sf[7] - so[7])) <= 1e-10 * max(1.0, np.max(np.abs(so[7]))), tile


def test_rays_crossing_lateral_faces(eng, orc):
    """A beam that overfills the volume with a large divergence: rays start outside the lateral faces, leave through
    them, come in through them.  Outside, the field is the fill value (rays keep going straight: a virtual cell beyond
    the face, slopes scaled by 0); a ray that ENTERS through a lateral face in mid-step finds its cell by the float64
    table search of the kernel's rarely-taken region -- in both builds, no second level involved.
    Every ray is finite and agrees with the oracle, on the whole volume and on a chain of slabs."""
    g = golden("g2_trace_blob32_z_s0")
    x, ext = g["x"], float(g["extent"])
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    np.random.seed(11)
    s0 = init_beam(6000, 1.5 * ext, 0.08, ext, "square", "z")  # +-7.5 mm square beam on a +-5 mm volume, 0.08 rad rms
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    dom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), phaseshift=True)
    dt = float(np.float32(x)[1] - np.float32(x)[0]) / orc.c
    so, _ = orc.trace_rk4(dom, s0, dt, orc.default_t_end(ext), "z", "planes", 1)
    ro, _ = orc.ray_to_jones(so, ext, "z")
    outside0 = (np.abs(s0[0]) > ext) | (np.abs(s0[1]) > ext)
    assert 1000 < outside0.sum() < 5000
    ang = np.hypot(s0[3], s0[4]) / s0[5]
    for precision in ("mixed", "f64"):
        sf, rf, Jf, st = eng.trace(vol, s0, eng.default_t_end(ext), ext, precision=precision, dt=dt)
        assert np.isfinite(sf).all() and np.isfinite(rf).all()
        dpos = np.max(np.abs(rf[0::2] - ro[0::2]), axis=0)
        dang = np.max(np.abs(rf[1::2] - ro[1::2]), axis=0)
        if precision == "f64":  # every ray on the exact route, lateral entries included
            assert st.fallback_rays == 0 and dpos.max() <= 1e-12 and dang.max() <= 1e-10
        else:  # float32 stage arithmetic: the error grows with the inclination (measured 3e-11 m below 0.02 rad, 5e-10 m above 0.1)
            assert st.fallback_rays == 0  # lateral entries are taken in the kernel (k_trace_mx), none passed on
            assert np.all(dpos <= 1e-10 + 1e-8 * ang) and dang.max() <= 2e-5, (dpos.max(), dang.max())
    # the same through two slabs (A12): no ray is dropped at a lateral entry
    for precision in ("mixed", "f64"):
        rays = eng.RayBundle(s0.shape[1]).upload(s0)
        cuts = eng.slab_cuts(len(x), 2)
        for q, (lo, hi) in enumerate(cuts):
            part = eng.Volume.from_ne_slab(eng.slab_source(g["ne"], 2, lo, hi), x, x, x, float(g["lwl"]), "z", lo, hi, phaseshift=True)
            flags = (eng.HANDOFF_ENTER if q > 0 else 0) | (eng.HANDOFF_EXIT if q + 1 < len(cuts) else 0)
            st = rays.trace(part, eng.default_t_end(ext), ext, precision=precision, handoff=flags, dt=dt)
            assert st.fallback_rays == 0
        sf2, rf2, _ = rays.download()
        assert np.isfinite(sf2).all()
        dpos = np.max(np.abs(rf2[0::2] - ro[0::2]), axis=0)
        if precision == "f64":
            assert dpos.max() <= 1e-12 and np.array_equal(sf2, sf)  # sf: the float64 whole-volume pass above
        else:
            assert np.all(dpos <= 1e-10 + 1e-8 * ang), dpos.max()
    # rays that never touch the volume go straight
    never = outside0 & (np.abs(so[0]) > ext) & (np.abs(so[1]) > ext) & (np.sign(s0[0]) == np.sign(so[0]))
    assert never.sum() > 100 and np.allclose(sf[3:6, never], s0[3:6, never], rtol=0, atol=0)


# ---------------------------------------------------------------- the bundle drawn on the device
def test_device_beam_distributions(eng):
    """RayBundle.generate: init_beam's distributions (full_solver.py:563-640) from a Philox stream.  Not NumPy's sample, so
    the check is statistical against init_beam's own draws (means, spreads, the disc's radial law, |v| = c), plus exact
    structure: launch plane, amplitude 1, and the stream keyed by the ray index (chunking does not change the rays)."""
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    N, ext, bs, div = 400000, 5e-3, 4e-3, 5e-4
    for pd in "xyz":
        a = "xyz".index(pd)
        l1, l2 = {"x": (1, 2), "y": (0, 2), "z": (0, 1)}[pd]
        s = eng.RayBundle(N).generate(bs, div, ext, "circular", pd, seed=3).download_s0()
        np.random.seed(1)
        h = init_beam(N, bs, div, ext, "circular", pd)
        assert np.all(s[a] == -ext) and np.all(s[6] == 1.0) and np.all(s[7] == 0.0) and np.all(s[8] == 0.0)
        assert np.max(np.abs(np.sqrt((s[3:6] ** 2).sum(0)) / eng.c - 1)) <= 1e-15
        r, rh = np.hypot(s[l1], s[l2]), np.hypot(h[l1], h[l2])
        assert r.max() <= bs and abs(r.mean() - rh.mean()) <= 4 * rh.std() / np.sqrt(N) * 2
        q = np.linspace(0.05, 0.95, 10)
        assert np.max(np.abs(np.quantile(r, q) - np.quantile(rh, q))) <= 0.01 * bs  # the folded-sum radial law
        for row in (l1, l2, 3 + l1, 3 + l2):
            assert abs(s[row].mean() - h[row].mean()) <= 6 * h[row].std() / np.sqrt(N)
            assert abs(s[row].std() / h[row].std() - 1) <= 0.01
        chi, chih = np.arccos(s[3 + a] / eng.c), np.arccos(h[3 + a] / eng.c)
        assert abs(chi.std() / chih.std() - 1) <= 0.01 and abs(np.mean(chi ** 2) ** 0.5 / div - 1) <= 0.01
    # the ray index keys the stream: a bundle generated in two chunks equals the bundle generated at once
    whole = eng.RayBundle(1000).generate(bs, div, ext, seed=9).download_s0()
    p1 = eng.RayBundle(300).generate(bs, div, ext, seed=9, first_ray=0).download_s0()
    p2 = eng.RayBundle(700).generate(bs, div, ext, seed=9, first_ray=300).download_s0()
    assert np.array_equal(np.concatenate([p1, p2], axis=1), whole)
    assert not np.array_equal(eng.RayBundle(1000).generate(bs, div, ext, seed=10).download_s0(), whole)
    sq = eng.RayBundle(20000).generate((1e-3, 2e-3), div, ext, "rectangular", "z", seed=1).download_s0()
    assert np.abs(sq[0]).max() <= 1e-3 and np.abs(sq[1]).max() <= 2e-3 and abs(sq[0].std() / (1e-3 / np.sqrt(3)) - 1) < 0.03
    # 'linear' (full_solver.py:707-721): a line in x, angles in the x-z plane, against init_beam's own draw
    ln = eng.RayBundle(N).generate(bs, div, ext, "linear", "z", seed=4).download_s0()
    np.random.seed(2)
    hl = init_beam(N, bs, div, ext, "linear", "z")
    assert np.all(ln[1] == 0) and np.all(ln[4] == 0) and np.all(ln[2] == -ext) and np.all(ln[6] == 1.0)
    assert np.max(np.abs(np.hypot(ln[3], ln[5]) / eng.c - 1)) <= 1e-15 and np.abs(ln[0]).max() <= bs
    assert abs(ln[0].std() / hl[0].std() - 1) <= 0.01 and abs(ln[3].std() / hl[3].std() - 1) <= 0.01
    assert abs(ln[0].mean()) <= 6 * hl[0].std() / np.sqrt(N) and abs(ln[3].mean()) <= 6 * hl[3].std() / np.sqrt(N)
    # the JAX generation's radial law, u = np.random.power(2) (src/simulator/beam.py:66-77): radii with density 2u,
    # i.e. positions uniform over the disc -- against NumPy's own power(2) sample and the closed-form quantiles sqrt(q)
    pw = eng.RayBundle(N).generate(bs, div, ext, "circular", "z", seed=5, radial_law="power").download_s0()
    rp = np.hypot(pw[0], pw[1]) / bs
    q = np.linspace(0.05, 0.95, 10)
    np.random.seed(3)
    assert np.max(np.abs(np.quantile(rp, q) - np.sqrt(q))) <= 0.005
    assert np.max(np.abs(np.quantile(rp, q) - np.quantile(np.random.power(2, N), q))) <= 0.005
    assert rp.max() < 1 and np.all(pw[2] == -ext) and np.max(np.abs(np.sqrt((pw[3:6] ** 2).sum(0)) / eng.c - 1)) <= 1e-15


def test_driver_device_beam_independent_of_chunking(eng, tmp_path):
    from synthpy_amd import run_trace as rt

    outs = []
    for chunk in ("4096", "1000"):
        out = str(tmp_path / f"o{chunk}.npz")
        rt.main(["-d", "32", "-r", "6000", "--chunk", chunk, "--ne-type", "test_exponential_cos", "--diagnostics", "shadow",
                 "--bin-scale", "8", "--device-beam", "--seed", "4", "-o", out])
        outs.append(np.load(out)["shadow"])
    assert outs[0].sum() > 4000 and np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("nlat", [1025, 2049])
def test_large_lateral_grid_binning(eng, orc, nlat):
    """The ray binning's LDS counters at their largest (2^10 and 2^11 coarse / fine Morton digits): thin volumes with
    1024^2 and 2048^2 lateral cells; results must not depend on the binning, and agree with the oracle on a sample."""
    ext, nz = 5e-3, 33
    xl = np.linspace(-ext, ext, nlat)
    z = np.linspace(-ext, ext, nz)
    X, Y, Z = np.meshgrid(xl, xl, z, indexing="ij", sparse=True)
    ne = (1e25 * np.exp(-(X ** 2 + Y ** 2) / (2e-3) ** 2) * (1 + 0.1 * np.sin(4e3 * X) * np.cos(3e3 * Y))).astype(np.float32) + 0 * Z.astype(np.float32)
    vol = eng.Volume.from_ne(ne, xl, xl, z, 1064e-9, "z")
    np.random.seed(4)
    from synthpy_amd.solvers_legacy.full_solver import init_beam

    # the cells are 0.3 mm long and 10 or 5 um wide: a ray that crosses more than one lateral cell in a stage is handed
    # to the time-stepping form by the mixed build (checked below: a few per cent at most)
    s0 = init_beam(300000, 4.5e-3, 2e-4, ext, "circular", "z")
    a = eng.trace(vol, s0, eng.default_t_end(ext), ext, sort_rays=True)
    b = eng.trace(vol, s0, eng.default_t_end(ext), ext, sort_rays=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3].ray_steps == b[3].ray_steps
    assert a[3].fallback_rays <= 0.05 * s0.shape[1]
    if a[3].fallback_rays == 0:
        assert a[3].ray_steps == (nz - 1) * s0.shape[1]
    ns = 2000
    dom = orc.Domain.from_ne(ne, xl, xl, z, 1064e-9)
    so, _ = orc.trace_rk4(dom, s0[:, :ns], float(np.float32(z)[1] - np.float32(z)[0]) / orc.c, orc.default_t_end(ext), "z", "planes", 1)
    ro, _ = orc.ray_to_jones(so, ext, "z")
    assert np.max(np.abs(a[1][0::2, :ns] - ro[0::2])) <= 1e-8 and np.max(np.abs(a[1][1::2, :ns] - ro[1::2])) <= 2e-5
    f = eng.trace(vol, s0[:, :ns], eng.default_t_end(ext), ext, precision="f64")  # the float64 build keeps every ray
    assert f[3].fallback_rays == 0 and np.max(np.abs(f[1][0::2] - ro[0::2])) <= 1e-12


def test_trace_counters_carried_until_read(eng):
    """sr_rays_trace with stats == NULL queues the work and leaves its counters to add up; sr_rays_trace_stats (or
    the next trace that asks for stats) returns the totals since the last read and starts again from zero."""
    g = golden("g2_trace_blob32_z_s0")
    x, ext = g["x"], float(g["extent"])
    s0 = g["s0"].copy()
    s0[5, :5] *= -1.0  # five rays for the time-stepping form
    N = s0.shape[1]
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    rays = eng.RayBundle(N).upload(s0)
    one = rays.trace(vol, eng.default_t_end(ext), ext)
    assert one.fallback_rays == 5 and one.ray_steps > 0
    assert rays.trace_stats() == eng.TraceStats()  # nothing unread
    for _ in range(3):
        rays.trace(vol, eng.default_t_end(ext), ext, want_stats=False)
    tot = rays.trace_stats()
    assert tot.ray_steps == 3 * one.ray_steps and tot.fallback_rays == 15
    rays.trace(vol, eng.default_t_end(ext), ext, want_stats=False)
    both = rays.trace(vol, eng.default_t_end(ext), ext)  # a trace that asks reads what is unread, its own included
    assert both.ray_steps == 2 * one.ray_steps and both.fallback_rays == 10
    again = rays.trace(vol, eng.default_t_end(ext), ext)
    assert again.ray_steps == one.ray_steps and again.fallback_rays == 5


# ---------------------------------------------------------------- BASELINE config 3's sizes, by properties
def test_full_size_properties(eng, orc):
    """1e7 rays x 512^3 (BASELINE config 3), too large for the oracle's trace: properties that do not depend on size.
    (a) empty volume: velocities untouched bit for bit, positions the straight line, zero phase, and the shadowgram
    counts equal to the oracle's optics + histogram of the same rf (integer: exact); (b) a structured volume: the
    result of a ray does not depend on where it sits in the bundle (shuffled bundle, bit for bit); (c) four slabs with
    hand-off == the whole volume, bit for bit, same number of ray-steps -- in the float64 build that is also the per-ray
    kernel (the slabs) against the tile path (the whole volume) on all 1e7 rays; (d) mirror symmetry x -> -x of volume and
    bundle."""
    n, N, ext, lwl = 512, 10_000_000, 5e-3, 1064e-9
    x = np.linspace(-ext, ext, n)
    t_end = eng.default_t_end(ext)
    rays = eng.RayBundle(N).generate(4e-3, 5e-5, ext, "circular", "z", seed=7)
    s0 = rays.download_s0()
    assert s0.shape == (9, N) and np.all(s0[2] == -ext)

    # (a) no plasma
    vol = eng.Volume.from_ne(np.zeros((n, n, n), np.float32), x, x, x, lwl, "z", phaseshift=True)
    st = rays.trace(vol, t_end, ext, precision="mixed")
    assert st.ray_steps == (n - 1) * N and st.fallback_rays == 0
    sf, rf, _ = rays.download(Jf=False)
    assert np.array_equal(sf[3:6], s0[3:6]) and np.all(sf[7] == 0.0) and np.array_equal(sf[6], s0[6])
    slope_x, slope_y = s0[3] / s0[5], s0[4] / s0[5]
    # the mixed build forms the lateral slope v_b / v_a in float32: 6e-8 of a displacement of <= 3e-6 m
    assert np.max(np.abs(rf[0] - (s0[0] + slope_x * 2 * ext))) <= 1e-12 and np.max(np.abs(rf[2] - (s0[1] + slope_y * 2 * ext))) <= 1e-12
    assert np.array_equal(rf[1], np.arctan(slope_x)) and np.array_equal(rf[3], np.arctan(slope_y))
    img = eng.DetectorImage.counts(bin_scale=1)
    _, hit = rays.deposit(img, eng.chain_shadow_two())
    H = img.download()
    r_o = orc.optics(orc.m_to_mm(rf), orc.chain_shadow_two())[0]
    H_o = orc.histogram(r_o, bin_scale=1)
    assert hit == int(H.sum()) == int(H_o.sum()) and np.array_equal(H, H_o) and hit > 0.9 * N
    vol.close()
    del sf, rf, H, H_o, r_o

    # a structured volume: smooth modes + an off-centre column (n_e > 0), not symmetric in x
    c = (x / ext).astype(np.float32)
    X, Y, Z = c[:, None, None], c[None, :, None], c[None, None, :]
    ne = (1e25 * (1.0 + 0.4 * np.sin(5.0 * X + 1.0) * np.cos(7.0 * Y) * np.cos(3.0 * Z + 0.5) + 0.3 * np.exp(-((X - 0.2) / 0.1) ** 2 - (Y / 0.3) ** 2))).astype(np.float32)
    vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)
    st = rays.trace(vol, t_end, ext, precision="mixed")
    assert st.ray_steps == (n - 1) * N and st.fallback_rays == 0
    sf, rf, Jf = rays.download()
    assert np.isfinite(sf).all() and np.max(np.abs(rf[1])) > 1e-4  # the rays are deflected

    # (b) position in the bundle does not matter
    perm = np.random.default_rng(3).permutation(N)
    shuffled = eng.RayBundle(N).upload(np.ascontiguousarray(s0[:, perm]))
    shuffled.trace(vol, t_end, ext, precision="mixed")
    sf_p = shuffled.download(rf=False, Jf=False)[0]
    assert np.array_equal(sf_p, sf[:, perm])
    shuffled.close()
    del sf_p

    # (c) four slabs.  float64 build: bit for bit.  Mixed build: a slab's kernel finds every ray's cell by table search
    # on its first plane, the whole-volume pass walked there from the neighbour cell; for a ray exactly on a cell face
    # the two can hold different cells -- the same trilinear value, rounded differently in float32 (measured: 1 ray of
    # 1e7, phase only, 4e-8 rad)
    for precision in ("mixed", "f64"):
        if precision == "f64":
            rays.trace(vol, t_end, ext, precision="f64")
            assert rays.tile_segments == 4 and rays.tile_records  # a dense bundle: the whole volume went through the TILE path (the records kernel, four segments) ...
            sf, rf, Jf = rays.download()
        steps = 0
        cuts = eng.slab_cuts(n, 4)
        for q, (lo, hi) in enumerate(cuts):
            part = eng.Volume.from_ne_slab(eng.slab_source(ne, 2, lo, hi), x, x, x, lwl, "z", lo, hi, phaseshift=True)
            flags = (eng.HANDOFF_ENTER if q > 0 else 0) | (eng.HANDOFF_EXIT if q + 1 < len(cuts) else 0)
            steps += rays.trace(part, t_end, ext, handoff=flags, precision=precision).ray_steps
            part.close()
        sf_s, rf_s, Jf_s = rays.download()
        assert steps == (n - 1) * N
        # ... and so does every slab of the float64 chain since round 4 (one 128-plane segment each, the arrivals binned again by
        # the cell they are in); the mixed build's slabs run its per-ray kernel
        assert rays.tile_segments == (1 if precision == "f64" else 0)
        if precision == "f64":
            assert np.array_equal(sf_s, sf) and np.array_equal(rf_s, rf) and np.array_equal(Jf_s, Jf)
        else:
            differ = np.flatnonzero(np.any(sf_s != sf, axis=0))
            assert len(differ) <= N // 100000, len(differ)
            assert np.max(np.abs(sf_s[:3] - sf[:3])) <= 1e-13 and np.max(np.abs(sf_s[3:6] - sf[3:6])) / orc.c <= 1e-10
            assert np.max(np.abs(sf_s[7] - sf[7])) <= 1e-6
        del sf_s, rf_s, Jf_s
    rays.trace(vol, t_end, ext, precision="mixed")  # the mixed build's whole-volume pass again, for (d)
    sf = rays.download(rf=False, Jf=False)[0]
    vol.close()

    # (d) mirror image: n_e(-x), rays mirrored in x; the float32 node coordinates are symmetric, so are the gradients
    assert np.array_equal(np.float32(x), -np.float32(x)[::-1])
    s0m = s0.copy()
    s0m[0] *= -1.0
    s0m[3] *= -1.0
    volm = eng.Volume.from_ne(np.ascontiguousarray(ne[::-1]), x, x, x, lwl, "z", phaseshift=True)
    rays.upload(s0m)
    rays.trace(volm, t_end, ext, precision="mixed")
    sf_m = rays.download(rf=False, Jf=False)[0]
    sgn = np.array([-1, 1, 1, -1, 1, 1, 1, 1, 1.0])[:, None]
    d = np.abs(sf_m * sgn - sf)
    # two mixed-build runs, each within ~1e-10 m of the exact route (float32 stage arithmetic is not mirror-symmetric)
    assert d[:3].max() <= 5e-10 and d[3:6].max() / orc.c <= 5e-8 and d[7].max() <= 5e-5, (d[:3].max(), d[3:6].max() / orc.c, d[7].max())
    volm.close()
    rays.close()


# ---------------------------------------------------------------- maximum sizes: more nodes than 32 bits count
def test_volume_beyond_32_bit_node_count(eng, orc):
    """1700^3 = 4.9e9 nodes (> 2^32; 79 GB of packed gradients): every index on the path is 64-bit.  (1) the gathers at
    cells all over the volume, the far corner included, against the oracle's np.gradient + trilinear form evaluated on
    the 4 x 4 x 4 nodes around each cell; (2) the whole volume against a chain of two slabs (2.5e9 nodes each, below
    2^32): bit for bit in the float64 build, to float32 rounding in the mixed build; every ray takes n - 1 steps."""
    n, N, ext, lwl = 1700, 200_000, 5e-3, 1064e-9
    x = np.linspace(-ext, ext, n)
    c = np.linspace(-1.0, 1.0, n).astype(np.float32)
    fx, fy, fz = np.sin(5.0 * c + 1.0), np.cos(7.0 * c), np.cos(3.0 * c + 0.5)
    ne = np.empty((n, n, n), np.float32)
    np.multiply((np.float32(0.4e25) * fx[:, None] * fy[None, :])[:, :, None], fz[None, None, :], out=ne)  # two passes over 20 GB
    ne += np.float32(1e25)
    vol = eng.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)
    assert vol.nbytes > 4 * 2 ** 32 * 4

    # (1) gathers
    rng = np.random.default_rng(5)
    cells = np.concatenate([rng.integers(1, n - 3, (150, 3)), np.array([[n - 4, n - 4, n - 4], [n - 4, 1, n - 4], [1, n - 4, 1], [n // 2, n // 2, n // 2]])])
    frac = rng.random((len(cells), 3))
    x32 = np.float32(x).astype(np.float64)
    pts = x32[cells] + frac * (x32[cells + 1] - x32[cells])
    F = vol.sample(pts)
    want = np.empty((3, len(cells)))
    # np.gradient takes its uniform-spacing branch when ALL the float32 coordinate differences of an axis are equal
    # (never on the 1700-node axes, often on four of their nodes): a fifth, oddly spaced node behind the block keeps the
    # block on the non-uniform branch without touching the gradients at the cell's own corners
    def block_axis(i):
        return np.append(x32[i - 1:i + 3], x32[i + 2] + 3.0 * (x32[i + 2] - x32[i + 1]))

    threads = orc.num_threads()
    orc.set_num_threads(1)  # 125-node blocks: a parallel region per call costs more than the work
    for m, (i, j, k) in enumerate(cells):
        sub = np.pad(ne[i - 1:i + 3, j - 1:j + 3, k - 1:k + 3], ((0, 1), (0, 1), (0, 1)), mode="edge")
        co = [block_axis(i), block_axis(j), block_axis(k)]
        _, gx, gy, gz = orc.calc_dndr(sub, co[0], co[1], co[2], lwl)
        for q, g in enumerate((gx, gy, gz)):
            want[q, m] = orc.interp(np.float32(co[0]), np.float32(co[1]), np.float32(co[2]), g, pts[m], 0.0)[0]
    orc.set_num_threads(threads)
    assert np.max(np.abs(F[:3] - want)) <= 1e-14 * np.max(np.abs(want))

    # (2) whole volume against two slabs, both builds
    t_end = eng.default_t_end(ext)
    bundles = {p: eng.RayBundle(N).generate(4e-3, 5e-5, ext, "circular", "z", seed=11) for p in ("mixed", "f64")}
    whole = {}
    for p, rays in bundles.items():
        st = rays.trace(vol, t_end, ext, precision=p)
        assert st.ray_steps == (n - 1) * N and st.fallback_rays == 0
        whole[p] = rays.download(rf=False, Jf=False)[0]
    vol.close()
    assert np.isfinite(whole["f64"]).all() and np.max(np.abs(whole["f64"][3])) > 1e3  # deflected
    cuts = eng.slab_cuts(n, 2)
    steps = {p: 0 for p in bundles}
    for q, (lo, hi) in enumerate(cuts):
        part = eng.Volume.from_ne_slab(eng.slab_source(ne, 2, lo, hi), x, x, x, lwl, "z", lo, hi, phaseshift=True)
        flags = (eng.HANDOFF_ENTER if q > 0 else 0) | (eng.HANDOFF_EXIT if q + 1 < len(cuts) else 0)
        for p, rays in bundles.items():
            steps[p] += rays.trace(part, t_end, ext, handoff=flags, precision=p).ray_steps
        part.close()
    for p, rays in bundles.items():
        sf = rays.download(rf=False, Jf=False)[0]
        assert steps[p] == (n - 1) * N
        if p == "f64":
            assert np.array_equal(sf, whole[p])
        else:
            assert np.max(np.abs(sf[:3] - whole[p][:3])) <= 1e-13 and np.max(np.abs(sf[3:6] - whole[p][3:6])) / orc.c <= 1e-10
            assert np.max(np.abs(sf[7] - whole[p][7])) <= 1e-6
        rays.close()
    # the two builds agree as on the fixtures
    assert np.max(np.abs(whole["mixed"][:3] - whole["f64"][:3])) <= 5e-10


# ---------------------------------------------------------------- the format either side of the path: field files
def test_driver_field_pvti_equals_npy(eng, tmp_path):
    """run_trace --field on a .pvti (the reference's pvti_readin flow, pvti_trace_mpi.py:71-92) == the same field given as
    .npy: the VTI is written from the VTK XML format rules by the test (tests/test_filetypes._spec_vti, not by the
    package's writer), the PVTI header is the reference's own wording (export_pvti, handle_filetypes.py:72-84)."""
    from synthpy_amd import run_trace as rt
    from test_filetypes import _spec_vti

    n = 32
    x = np.linspace(-5e-3, 5e-3, n)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij", sparse=True)
    ne = 1e25 * np.exp(-(X ** 2 + Y ** 2 + Z ** 2) / (1.5e-3) ** 2) + 3e24 * (1 + np.sin(1.5e3 * X) * np.cos(2e3 * Y + 1e3 * Z))
    np.save(tmp_path / "f.npy", ne)
    _spec_vti(str(tmp_path / "f.vti"), ne, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), where="appended-base64", header_type="UInt64", compress=True)
    (tmp_path / "f.pvti").write_text(f"""<?xml version="1.0"?>
        <VTKFile type="PImageData" version="0.1" byte_order="LittleEndian" header_type="UInt32" compressor="vtkZLibDataCompressor">
        <PImageData WholeExtent="0 {n} 0 {n} 0 {n}" GhostLevel="0" Origin="0 0 0" Spacing="1.0 1.0 1.0">
            <PCellData Scalars="rnec"><PDataArray type="Float64" Name="rnec"></PDataArray></PCellData>
            <Piece Extent="0 {n} 0 {n} 0 {n}" Source="f.vti"/>
        </PImageData>
        </VTKFile>""")
    outs = []
    for field in ("f.pvti", "f.npy"):
        out = str(tmp_path / (field + ".npz"))
        rt.main(["--field", str(tmp_path / field), "-r", "4000", "--chunk", "2048", "--diagnostics", "shadow,schlieren,interf",
                 "--bin-scale", "8", "-o", out])
        outs.append(np.load(out))
    a, b = outs
    assert int(a["rays"]) == int(b["rays"]) == 4000 and a["shadow"].sum() > 3000
    for key in ("shadow", "schlieren"):
        assert np.array_equal(a[key], b[key]), key  # integer counts: exact
    # the complex sums are float64 atomics: two runs of the same rays differ by the order of their additions
    assert np.max(np.abs(a["interf"] - b["interf"])) <= 1e-9 * np.max(b["interf"])
