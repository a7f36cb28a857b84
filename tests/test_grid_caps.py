"""Every launch whose grid is capped (sr::capped_grid, common.hpp: min(the blocks the work needs, n_cu * k), the rest by a
grid-stride loop) run PAST its cap, at small shapes.

On an MI355X (256 compute units) the second trip of those loops starts at sizes no other test module reaches for k_emission_z,
k_project, k_resample, k_modesum and k_modesum_tables, while every production size runs two trips or more.  What goes wrong in
such a loop -- state carried from one item to the next, a stride off by the lanes-per-item factor, a ragged last trip in which
part of a wavefront has left before a shuffle, an index permutation that assumes one trip -- is invisible while gridDim covers
the work.  Every case here runs one entry point on one input up to three ways:

  (a) as it is, at the device's caps;
  (b) under engine.grid_cus(1), the caps of a device of ONE compute unit.  The shape is chosen so that the launch wants at least
      three times the blocks it gets and not a multiple of them (the last trip is ragged): computed from the sizes and asserted
      (`_ragged`), and engine.grid_stats() must report that every capped launch of the entry got fewer blocks than it wanted;
  (c) where listed, a shape built from engine.compute_units() that crosses the device's OWN cap (about 2.5 times the cap, an
      awkward count), without an override, with the same assertion from grid_stats().

(b) must equal (a) bit for bit: none of these kernels adds with floating-point atomics, and each item is computed by one thread
or one wavefront whatever the grid.  (a) and (c) are compared with the restatement the project already has for the entry, imported
from that entry's own test module with its own derived bound.  NO tolerance is introduced here: every comparison is bit equality,
integer equality, or a bound of the module named.

Where a shape differs from the obvious small one, the cap says why:
* k_modesum's cap is 64 blocks of 4 waves per compute unit, so one compute unit still holds 256 tiles: 40 x 33 x 130 (135 tiles),
  300 x 200 (76) and 5000 points (79) would take ONE trip under (b).  The shapes below are long on the tile axis that costs the
  fewest nodes, and have few modes, so that the host mirror they are compared with stays quick, while k_modesum_tables (32 blocks
  of 256 entries per compute unit) still wants three times its blocks.
* k_resample numbers its bricks in supertiles of 64, so the blocks it wants are a multiple of the 8 it gets from one compute unit,
  whatever the view: (b) runs at one compute unit (64 full trips) AND at three (24 blocks: the last trip is ragged).
* sr_field_modesum in 3-D at the device's own cap would need 1 GB of output: it has no (c).  The 1-D (c) crosses
  k_modesum_tables' cap cheaply, with many modes on few points.

* 10 007 rays want 40 blocks of k_bbox, five full trips of one compute unit's 8: the bundle has 10 519 (42 blocks).
* The records build runs on the blob32 fixture, whose 30 752 records want 121 blocks where one compute unit gives 64: two
  trips, the second ragged, not three.
* The gridding's second pass (k_locate_team) launches one team per node it still has to place: capped only when there are more
  than four, so the gridding cases count it as a launch with extra trips only then.

Every capped launch of synthpy_amd/csrc has a case here.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import test_emission as te
import test_field_generators as tf
import test_projection as tp
import test_resample as tr
import test_table_emission as tt

LATERAL = (13, 11)  # 143 columns


@pytest.fixture(scope="module")
def eng():
    from synthpy_amd import _ffi, engine

    engine.init(0)
    yield engine
    now = C.c_int(-1)
    _ffi.check(_ffi.lib.sr_grid_cus(-1, C.byref(now)))
    assert now.value == engine.compute_units(), f"a test left the grid caps sized for {now.value} compute units"


def _ragged(wanted, per_cu, n_cu=1):
    """The shape rule of (b): the launch wants at least three times the blocks it gets, and not a multiple of them."""
    got = per_cu * n_cu
    assert wanted >= 3 * got and wanted % got != 0, (wanted, got)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f"{what}: other bits under another grid"


def _awkward(target, other):
    """n with n * other about `target`, odd."""
    return max(3, int(round(target / other))) | 1


# ================================================================ k_emission_z: one wavefront per column, 4 to a block, k = 8
def _emission_blocks(lateral):
    return (lateral[0] * lateral[1] + 3) // 4


@pytest.mark.gpu
@pytest.mark.parametrize("n", (3, 65, 129))
def test_emission_z(eng, n):
    K = te._case(2, n, LATERAL)
    _ragged(_emission_blocks(LATERAL), 8)
    for toward, nb in itertools.product((+1, -1), (4, 1)):
        what = f"emission z {n} planes toward {toward:+d} {nb} band(s)"
        args = (K["ne"], K["Te"], K["Z"], K["co"], te.WAVELENGTHS[:nb], 2, toward, K["back"][:nb])
        a = te._run(eng, *args)
        with eng.grid_cus(1):
            b = te._run(eng, *args)
            assert eng.grid_stats() == (1, 1), (what, eng.grid_stats())
        _same(a[0], b[0], what + " I")
        _same(a[1], b[1], what + " tau")
        ref = tuple(v[:nb] for v in K["refs"][toward])
        te._assert_inputs(ref, what)
        te._assert_close(a[0], a[1], ref, what)


def _wide_lateral(eng):
    """(nu, 97) with about 2.5 * 32 * n_cu columns: 2.5 times what k_emission_z's grid holds at the device's own cap."""
    return (_awkward(2.5 * 32 * eng.compute_units(), 97), 97)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (3, 65))
def test_emission_z_at_the_device_cap(eng, n):
    lateral = _wide_lateral(eng)
    assert _emission_blocks(lateral) > 2 * 8 * eng.compute_units() and _emission_blocks(lateral) % (8 * eng.compute_units())
    rng = np.random.default_rng(n)
    shape = lateral + (n,)
    ncol = lateral[0] * lateral[1]
    per_col = 10.0 ** (-3 * rng.permutation(ncol) / (ncol - 1)).reshape(lateral + (1,))
    ne = 1e26 * 10.0 ** (-rng.random(shape)) * per_col
    Te, Z = rng.uniform(1.0, 500.0, shape), rng.uniform(1.0, 30.0, shape)
    co = [te._coords(m, 7 + k) for k, m in enumerate(shape)]
    bands = te._bands(te.WAVELENGTHS[:1])
    ne = ne * np.sqrt(10.0 / te.restate(ne, Te, Z, co[2], bands, 2)[1].max())
    back = rng.uniform(0.0, 2e-7, (1,) + lateral)
    for dtype, toward in itertools.product((np.float32, np.float64), (+1, -1)):
        what = f"emission z {lateral} x {n} {np.dtype(dtype).name} toward {toward:+d}"
        f = [a.astype(dtype) for a in (ne, Te, Z)]
        ref = te.restate(*(np.float64(a) for a in f), co[2], bands, 2, toward, back)
        te._assert_inputs(ref, what)
        with eng.grid_cus(0):
            I, tau = te._run(eng, *f, co, te.WAVELENGTHS[:1], 2, toward, back)
            assert eng.grid_stats() == (1, 1), (what, eng.grid_stats())
        te._assert_close(I, tau, ref, what)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("lds", "global"))
def test_emission_table_z(eng, which):
    K = tt._case(2, 65, LATERAL)
    table = K["table"] if which == "lds" else tt._other_tables()["48x48 4 bands (global)"]
    assert (tt.packed_bytes(table) <= tt.LDS_BUDGET) == (which == "lds")
    _ragged(_emission_blocks(LATERAL), 8)
    H = tt.host_arrays(table)
    for toward in (+1, -1):
        what = f"table emission z ({which}) toward {toward:+d}"
        args = (K["ne"], K["Te"], K["Z"], K["co"], table, 2, toward, K["back"])
        a = tt._run(eng, *args)
        with eng.grid_cus(1):
            b = tt._run(eng, *args)
            assert eng.grid_stats() == (1, 1), (what, eng.grid_stats())
        _same(a[0], b[0], what + " I")
        _same(a[1], b[1], what + " tau")
        ref = K["refs"][toward] if which == "lds" else tt.restate(K["ne"], K["Te"], K["Z"], K["co"][2], H, 2, toward, K["back"])
        tt._assert_close(a[0], a[1], ref, what)


@pytest.mark.gpu
def test_emission_table_z_at_the_device_cap(eng):
    lateral = _wide_lateral(eng)
    K = tt._case(2, 3, lateral)
    assert tt.packed_bytes(K["table"]) <= tt.LDS_BUDGET
    for toward in (+1, -1):
        what = f"table emission z {lateral} x 3 toward {toward:+d}"
        with eng.grid_cus(0):
            I, tau = tt._run(eng, K["ne"], K["Te"], K["Z"], K["co"], K["table"], 2, toward, K["back"])
            assert eng.grid_stats() == (1, 1), (what, eng.grid_stats())
        tt._assert_close(I, tau, K["refs"][toward], what)


# ================================================================ k_project: eight lanes per column, 32 columns to a block, k = 8
def _proj_fields(shape, axis, seed):
    """test_projection._fields' recipe (it is keyed to that module's own shapes) on non-uniform axes."""
    rng = np.random.default_rng(seed)
    x, y, z = tp._coords(shape, False, seed + 1)
    m = -5e-3 * rng.random(shape)
    h_max = float(np.max(np.diff(np.float64((x, y, z)["xyz".index(axis)])))) / 299792458.0
    B = np.empty(shape + (3,))
    B[...] = (0.3, -0.5, 0.7)
    return dict(x=x, y=y, z=z, m=m, ne=-m * (2.0 + m) * tp._ne_scale(), kappa=-(1e-3 / h_max) * rng.random(shape),
                ne_f=1e24 * (0.5 + rng.random(shape)), B=B, verdet=2.62e-13 * tp.LWL ** 2)


def _project_case(eng, F, axis, na, flags, n_cu, what):
    """The volume's maps at the caps of n_cu compute units (0: the device's own), asserted to be one multi-trip launch, and its
    reference (test_projection: the fields read back, summed wide)."""
    phase, kap, far = flags
    vol = tp._volume(eng, F, axis, phase, kap, far)
    try:
        with eng.grid_cus(n_cu):
            maps = vol.project()
            assert eng.grid_stats() == (1, 1), (what, eng.grid_stats())
        plain = vol.project() if n_cu else None
        ref = tp._reference(vol, F[axis], axis, F["kappa"] if kap else None, F["ne_f"] if far else None, F["B"])
    finally:
        vol.close()
    return maps, plain, ref


@pytest.mark.gpu
@pytest.mark.parametrize("na", (2, 9, 17))
def test_project(eng, na):
    """All eight instantiations of k_project (phase, kappa, Faraday), 37 x 29 columns."""
    shape = (37, 29, na)
    _ragged((37 * 29 * 8 + 255) // 256, 8)
    F = _proj_fields(shape, "z", 100 + na)
    for flags in itertools.product((False, True), repeat=3):
        what = f"project {shape} z phase, kappa, faraday = {flags}"
        b, a, ref = _project_case(eng, F, "z", na, flags, 1, what)
        assert [a[k] is None for k in sorted(a)] == [b[k] is None for k in sorted(b)]
        for k in sorted(a):
            if a[k] is not None:
                _same(a[k], b[k], f"{what} {k}")
        tp._assert_maps(tp._flat(a), ref, na, what)


@pytest.mark.gpu
@pytest.mark.parametrize("axis", "zy")
@pytest.mark.parametrize("na", (2, 9))
def test_project_at_the_device_cap(eng, na, axis):
    """About 2.5 * 256 * n_cu columns; probing along y takes the kernel's swap branch."""
    n_cu = eng.compute_units()
    lateral = (397, _awkward(2.5 * 256 * n_cu, 397))
    wanted = (lateral[0] * lateral[1] * 8 + 255) // 256
    assert wanted > 2 * 8 * n_cu and wanted % (8 * n_cu)
    shape = lateral + (na,) if axis == "z" else (lateral[0], na, lateral[1])
    F = _proj_fields(shape, axis, 200 + na)
    what = f"project {shape} {axis}"
    maps, _, ref = _project_case(eng, F, axis, na, (True, True, True), 0, what)
    tp._assert_maps(tp._flat(maps), ref, na, what)


# ================================================================ k_resample: one brick of 4 x 4 x 16 nodes per block, k = 8
def _numbered_bricks(view):
    """resample.hip's nvb for the default brick: supertiles of 4 x 4 x 4 bricks, the padded bricks included."""
    bricks = [-(-m // b) for m, b in zip(view, (4, 4, 16))]
    return 64 * int(np.prod([-(-nb // 4) for nb in bricks]))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("vector", (False, True), ids=("scalar", "vector"))
def test_resample(eng, vector, dtype):
    """View 21 x 19 x 70 (6 x 5 x 5 bricks in 2 x 2 x 2 supertiles: 512 numbered, 150 real) under a generic rotation and a shift
    that leaves part of the view outside."""
    view = (21, 19, 70)
    nvb = _numbered_bricks(view)
    assert nvb == 512 and nvb >= 3 * 8 and nvb % 8 == 0  # a multiple of one compute unit's 8 blocks whatever the view ...
    _ragged(nvb, 8, 3)                                   # ... so the ragged last trip comes from three compute units
    rng = np.random.default_rng(51)
    axes = tr._axes((24, 20, 22), 52)
    out_axes = tr._axes(view, 53, half=(2.5e-3, 2.2e-3, 2.4e-3))
    src = (0.5 + rng.random((24, 20, 22) + ((3,) if vector else ()))).astype(dtype)
    M, t = tr._generic(), np.array([1.5e-3, -0.5e-3, 1.0e-3])
    V = M.T if vector else None
    fill = (-7.25, -8.5, -9.75) if vector else -7.25
    what = f"resample 24x20x22 -> {view} {np.dtype(dtype).name} {'vector' if vector else 'scalar'}"
    f = eng.Field(src, *axes)
    try:
        a = f.resample(M, t, out_axes, V=V, fill=fill)
        for n_cu in (1, 3):
            with eng.grid_cus(n_cu):
                b = f.resample(M, t, out_axes, V=V, fill=fill)
                assert eng.grid_stats() == (1, 1), (what, n_cu, eng.grid_stats())
            _same(a, b, f"{what} at {n_cu} compute unit(s)")
    finally:
        f.close()
    ref, outside, S = tr.restate(src, *axes, M, t, *out_axes, V=V, fill=fill)
    assert 0.1 * outside.size < outside.sum() < 0.9 * outside.size
    if vector:
        for c in range(3):
            tr._assert_close(a[..., c], ref[..., c], outside, S[..., c], tr.K_V, f"{what} component {c}", fill[c])
    else:
        tr._assert_close(a, ref, outside, S, tr.K_BLEND, what, fill)


@pytest.mark.gpu
@pytest.mark.parametrize("vector,dtype", [(False, np.float32), (True, np.float64)], ids=["f32-scalar", "f64-vector"])
def test_resample_at_the_device_cap(eng, vector, dtype):
    """65 x 65 x (130 on 256 compute units): 17 x 17 x 9 bricks padded to 5 x 5 x 3 supertiles, about 2.5 * 8 * n_cu numbered."""
    n_cu = eng.compute_units()
    sz = max(1, int(round(2.5 * 8 * n_cu / 64 / 25)))
    view = (65, 65, 64 * sz - 62)
    nvb = _numbered_bricks(view)
    assert nvb == 64 * 25 * sz and nvb > 2 * 8 * n_cu and nvb % (8 * n_cu)
    rng = np.random.default_rng(61)
    axes = [np.float32(np.linspace(-h, h, 64)) for h in (4e-3, 3e-3, 3.5e-3)]
    out_axes = [np.float32(np.linspace(-h, h, m)) for m, h in zip(view, (3.6e-3, 3.1e-3, 3.3e-3))]
    src = rng.standard_normal((64, 64, 64) + ((3,) if vector else ())).astype(dtype)
    M, t = tr._generic(), (1e-4, -2e-4, 1.5e-4)
    V = M.T if vector else None
    fill = (-7.25, -8.5, -9.75) if vector else -7.25
    what = f"resample 64^3 -> {view} {np.dtype(dtype).name} {'vector' if vector else 'scalar'}"
    f = eng.Field(src, *axes)
    try:
        with eng.grid_cus(0):
            got = f.resample(M, t, out_axes, V=V, fill=fill)
            assert eng.grid_stats() == (1, 1), (what, eng.grid_stats())
    finally:
        f.close()
    ref, outside, S = tr.restate(src, *axes, M, t, *out_axes, V=V, fill=fill)
    assert 0 < outside.sum() < outside.size
    if vector:
        for c in range(3):
            tr._assert_close(got[..., c], ref[..., c], outside, S[..., c], tr.K_V, f"{what} component {c}", fill[c])
    else:
        tr._assert_close(got, ref, outside, S, tr.K_BLEND, what, fill)


# ================================================================ k_modesum_tables (k = 32) and k_modesum (4 tiles to a block, k = 64)
def _modesum_blocks(shape, nmodes):
    """(blocks k_modesum_tables wants, blocks k_modesum wants) as field.hip's run_modesum sizes them."""
    n = ((1, 1, shape[0]), (shape[0], 1, shape[-1]), tuple(shape))[len(shape) - 1]
    T, JT = (8, 4) if n[1] > 1 else (16, 1)
    p0, p1 = -(-n[0] // T) * T, -(-n[1] // JT) * JT
    tiles = -(-n[2] // 64) * (p1 // JT) * (p0 // T)
    return -(-(p0 + p1 + n[2]) * nmodes // 256), -(-tiles // 4)


def _cos(nd, args, seed, device):
    np.random.seed(seed)
    return tf.CLASSES[nd](tf.k41).cos(*args, device=device)


# (lengths..., sizes..., modes, first wavenumber): 201 x 2 x 2 tiles of 8 x 4 x 64 with a ragged row of each kind; 257 x 3 tiles of
# 16 x 64; 782 tiles of 64
MODESUM = {"3d": (3, (1.0, 1.1, 0.9, 1601, 5, 70, 15, 3.0)), "2d": (2, (1.0, 0.8, 4111, 130, 7, 2 * np.pi)),
           "1d": (1, (3.0, 50001, 3, 1.0)), "1d-mirror": (1, (3.0, 5000, 300, 1.0))}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(MODESUM))
def test_modesum(eng, tag):
    """sr_field_modesum: k_modesum<8, 4> in 3-D, k_modesum<16, 1> in 2-D and 1-D, and the tables' kernel before either.  No (c)
    in 3-D: a field that crosses the device's own cap of 64 * 4 * n_cu tiles is 1 GB of output.
    A 1-D signal long enough for three trips of k_modesum (49 153 points at least) has phases k x up to pi * n = 1.6e5 rad, whose
    own rounding (2^-36 rad) is beyond what the 1e-12 rule allows EITHER side of the comparison: measured on an MI355X,
    5.4e-13 against 1e-12 * max|ref| = 2.0e-13.  That signal ("1d") is therefore held to bit equality of (b) and (a) only, and
    the host mirror is compared on test_field_generators' own 5000 points x 300 modes ("1d-mirror"), where the tables' kernel
    takes its extra trips and k_modesum does not."""
    nd, args = MODESUM[tag]
    shape, nmodes = args[nd:2 * nd], args[2 * nd]
    tables, tiles = _modesum_blocks(shape, nmodes)
    _ragged(tables, 32)
    if tag != "1d-mirror":
        _ragged(tiles, 64)
    a = _cos(nd, args, 70 + nd, True)
    with eng.grid_cus(1):
        b = _cos(nd, args, 70 + nd, True)
        assert eng.grid_stats() == (2, 1 if tag == "1d-mirror" else 2), (tag, eng.grid_stats())
    _same(a, b, f"mode sum {tag} {shape} x {nmodes} modes")
    if tag != "1d":
        tf.assert_close(a, _cos(nd, args, 70 + nd, False), 1e-12, f"mode sum {tag}")


@pytest.mark.gpu
def test_modesum_tables_at_the_device_cap(eng):
    """1-D, about 6000 points and enough modes for 2.5 * 32 * 256 * n_cu table entries."""
    n_cu = eng.compute_units()
    n = 6007
    nmodes = _awkward(2.5 * 32 * 256 * n_cu, 16 + 1 + n)
    tables, tiles = _modesum_blocks((n,), nmodes)
    assert tables > 2 * 32 * n_cu and tables % (32 * n_cu) and tiles <= 64 * n_cu
    args = (3.0, n, nmodes, 1.0)
    with eng.grid_cus(0):
        got = _cos(1, args, 75, True)
        assert eng.grid_stats() == (2, 1), eng.grid_stats()
    tf.assert_close(got, _cos(1, args, 75, False), 1e-12, f"mode sum 1-D {n} points x {nmodes} modes")


# ================================================================ k_bbox (trace.hip): k = 8
@pytest.mark.gpu
def test_upload_bbox(eng):
    n = 10519  # 42 blocks of 256 (10 007 rays want 40, five full trips of one compute unit's 8)
    _ragged((n + 255) // 256, 8)
    rng = np.random.default_rng(81)
    s0 = rng.standard_normal((9, n))
    s0[:, rng.integers(0, n, 500)] = np.nan
    s0[1, rng.integers(0, n, 300)] = np.nan
    s0[0, int(np.nanargmax(s0[0]))] = np.nan  # the extreme of a row must come from a ray that has one
    want = np.concatenate([np.nanmin(s0[:3], axis=1), np.nanmax(s0[:3], axis=1)])
    rays = eng.RayBundle(n)
    a = rays.upload(s0).bbox
    with eng.grid_cus(1):
        b = rays.upload(s0).bbox
        assert eng.grid_stats() == (1, 1), eng.grid_stats()
        rays.upload(np.full((9, n), np.nan))
        assert eng.grid_stats() == (2, 2) and rays.bbox is None, "an all-NaN bundle has no bounding box"
    assert a is not None and np.array_equal(a, want) and np.array_equal(a, b), (a, b, want)


# ================================================================ sr_power_spectrum: k_to_complex (k = 32), k_spectrum_bins (k = 8)
@pytest.mark.gpu
def test_power_spectrum(eng):
    """101 x 101 x 97 as test_power_spectrum.test_odd_prime_sizes, the three binnings (both rules).  The bins are summed with
    floating-point atomics, so (b) against (a) is that module's check_bins: counts equal, sums by its rule."""
    import test_power_spectrum as tps
    from synthpy_amd.utils import power_spectrum as ps
    from synthpy_amd.utils import spectrum_prep as prep

    r = np.random.default_rng(5).standard_normal((101, 101, 97))
    lengths, dx = (3.0, 5.0, 4.0), 0.1
    blocks = (r.size + 255) // 256
    _ragged(blocks, 32)
    _ragged(blocks, 8)
    tps.check_all_3(ps, r, lengths, dx, "101x101x97")
    binnings = {"radial": prep.radial(r.shape, lengths, 50)[0], "scalar_fft": prep.scalar_fft(r.shape, dx)[0],
                "knyquist": prep.knyquist(r.shape, lengths)[0]}
    for name, b in binnings.items():
        s_a, c_a, over_a = ps.binned_power(r, b)
        with eng.grid_cus(1):
            s_b, c_b, over_b = ps.binned_power(r, b)
            assert eng.grid_stats() == (2, 2), (name, eng.grid_stats())
        assert over_a == over_b
        tps.check_bins(s_b, c_b, s_a, c_a, f"{name} 101x101x97, one compute unit against the device's own")


# ================================================================ sr_field_ifft_real: k_shape_noise, k_real_scaled, k_divide (k = 32)
@pytest.mark.gpu
@pytest.mark.parametrize("normalise", (1, 0), ids=("normalised", "plain"))
def test_ifft_real(eng, normalise):
    """48 x 40 x 36 against np.fft.ifftn by test_gpu_parity.test_domain_fft_on_device_vs_reference's rule: 1e-12 of the
    unit-normalised field (the plain field: the same 1e-12 of ITS largest value, which is what the normalisation divides by)."""
    from synthpy_amd._ffi import check, lib, ptr

    shape = (48, 40, 36)
    _ragged((int(np.prod(shape)) + 255) // 256, 32)
    rng = np.random.default_rng(91)
    noise = np.ascontiguousarray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    amp = np.ascontiguousarray(rng.random(shape), dtype=np.float32)
    out = {}
    for n_cu in (0, 1):
        out[n_cu] = np.empty(shape)
        with eng.grid_cus(n_cu):
            check(lib.sr_field_ifft_real(ptr(noise), ptr(amp), *shape, normalise, ptr(out[n_cu])))
            assert eng.grid_stats() == (3 if normalise else 2,) * 2 if n_cu else eng.grid_stats()[1] == 0, (n_cu, eng.grid_stats())
    _same(out[0], out[1], f"ifft {shape}")
    ref = np.fft.ifftn(noise * amp).real
    scale = np.abs(ref).max()
    assert np.max(np.abs(out[0] - (ref / scale if normalise else ref))) <= 1e-12 * (1.0 if normalise else scale)
    assert not normalise or np.max(np.abs(out[0])) == 1.0


# ================================================================ volume.hip: the pack, unpack and aux kernels (k = 32)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_volume_pack_and_unpack(eng, orc, dtype):
    """g14's 41 x 29 x 23 grid, probed along each axis: from_ne (two launches), fields() (four), attach_aux (one), from_fields
    (one) and that volume's fields() (four) -- twelve capped launches, all with extra trips under (b).  (a) is the existing
    bit-exact comparison (the reference's calc_dndr for float64 n_e, the oracle's for float32); sample() and sample_aux() read
    what the pack kernels wrote."""
    from conftest import golden

    g = golden("g14_shapes")
    shape = g["ne"].shape
    _ragged((int(np.prod(shape)) + 255) // 256, 32)
    ne = np.ascontiguousarray(g["ne"], dtype=dtype)
    axes, lwl = (g["x"], g["y"], g["z"]), float(g["lwl"])
    want = (g["dndx"], g["dndy"], g["dndz"]) if dtype is np.float64 else orc.calc_dndr(ne, *axes, lwl)[1:]
    rng = np.random.default_rng(14)
    kappa, B = -rng.random(shape), rng.standard_normal(shape + (3,))
    half = np.array([float(a[-1]) for a in axes])
    pts = rng.uniform(-1.05, 1.05, (3000, 3)) * half
    pts[::97] = np.nan

    def run(pd):
        vol = eng.Volume.from_ne(ne, *axes, lwl, pd, phaseshift=True)
        f = vol.fields(phase=True)
        vol.attach_aux(kappa, np.float64(ne), B, 1e-20)
        s, sa = vol.sample(pts), vol.sample_aux(pts)
        again = eng.Volume.from_fields(f[0], f[1], f[2], *axes, vol.omega, pd, nref=1.0 + f[3])
        f2 = again.fields(phase=True)
        vol.close()
        again.close()
        return list(f) + [s, sa] + list(f2)

    for pd in "xyz":
        a = run(pd)
        with eng.grid_cus(1):
            b = run(pd)
            assert eng.grid_stats() == (12, 12), (pd, eng.grid_stats())
        for k, (u, v) in enumerate(zip(a, b)):
            _same(u, v, f"41x29x23 probed along {pd}, output {k}")
        for k in range(3):
            assert np.array_equal(a[k], want[k]) and np.array_equal(a[6 + k], want[k]), (pd, k)
        assert np.isfinite(a[4][:, 1]).all() and np.isnan(a[4][:, 0]).all() and np.any(a[5][0] != 0)


# ================================================================ trace.hip: k_build_records (k = 64), k_trace_time (k = 4)
@pytest.mark.gpu
def test_records_build(eng):
    """The blob32 fixture through the tile path's records kernel, the volume made AND first traced at one compute unit, so that
    its coefficient records are built there: 32 x 31 x 31 records want 121 blocks of 256, one compute unit gives 64 (two trips, the
    second ragged; the fixture is too small for three).  The rule is test_tile_kernel_is_bit_identical_to_the_per_ray_kernel's:
    sf, rf, Jf equal the per-ray kernel's bit for bit, and so do the steps."""
    from conftest import golden
    from test_gpu_parity import _forced_kernel_trace

    g = golden("g2_trace_blob32_z_s0")
    x, ext = g["x"], float(g["extent"])
    n = len(x)
    wanted = (n * (n - 1) * (n - 1) + 255) // 256
    assert wanted > 64 and wanted % 64
    s0 = np.ascontiguousarray(g["s0"], np.float64)
    make = lambda: eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    vol = make()
    ref = _forced_kernel_trace(eng, vol, s0, eng.default_t_end(ext), ext, 0, precision="f64")
    a = _forced_kernel_trace(eng, vol, s0, eng.default_t_end(ext), ext, 1, precision="f64")
    with eng.grid_cus(1):
        vol_b = make()
        assert eng.grid_stats() == (2, 2), eng.grid_stats()
    with eng.grid_cus(1):
        b = _forced_kernel_trace(eng, vol_b, s0, eng.default_t_end(ext), ext, 1, precision="f64")
        # the upload's k_bbox and the trace's k_trace_time queue want one block for 256 rays; the records build is the third
        assert eng.grid_stats() == (3, 1), eng.grid_stats()
    for got in (a, b):
        for u, v, name in zip(ref[:3], got[:3], ("sf", "rf", "Jf")):
            assert np.array_equal(u, v, equal_nan=True), name
        assert got[3].ray_steps == ref[3].ray_steps
    vol.close()
    vol_b.close()


@pytest.mark.gpu
def test_time_stepping_fallback(eng, orc):
    """test_gpu_parity.test_fallback_rays_time_stepping's construction on 32 copies of the blob32 rays, shifted a little: 4224 of
    8192 rays go to k_trace_time, whose queue one compute unit walks in five trips of 4 x 256, the last one ragged."""
    from conftest import golden

    g = golden("g2_trace_blob32_z_s0")
    x, ext = g["x"], float(g["extent"])
    rng = np.random.default_rng(32)
    s0 = np.tile(g["s0"], (1, 32))
    n = s0.shape[1]
    s0[:2] += rng.uniform(-1e-4, 1e-4, (2, n))
    k = np.arange(n) % 64
    s0[2, k < 17] = 0.0                                 # start inside the volume
    s0[5, (k >= 17) & (k < 25)] *= -1.0                 # flying away from the volume
    s0[3:6, (k >= 25) & (k < 33)] *= 0.5                # half speed: still inside at t_end
    vol = eng.Volume.from_ne(g["ne"], x, x, x, float(g["lwl"]), "z", phaseshift=True)
    dt = float(x[1] - x[0]) / orc.c
    rays = eng.RayBundle(n).upload(s0)
    st_a = rays.trace(vol, eng.default_t_end(ext), ext, dt=dt, precision="f64")
    a = rays.download()
    with eng.grid_cus(1):
        st_b = rays.trace(vol, eng.default_t_end(ext), ext, dt=dt, precision="f64")
        assert eng.grid_stats() == (1, 1), eng.grid_stats()
        b = rays.download()
    assert st_b.fallback_rays == st_a.fallback_rays == 33 * n // 64, (st_a.fallback_rays, st_b.fallback_rays)
    assert st_b.fallback_rays > 3 * 4 * 256 and st_b.fallback_rays % (4 * 256) != 0
    assert st_a.ray_steps == st_b.ray_steps
    for u, v, name in zip(a, b, ("sf", "rf", "Jf")):
        assert np.array_equal(u, v, equal_nan=True), name
    dom = orc.Domain.from_ne(g["ne"], x, x, x, float(g["lwl"]), phaseshift=True)
    sf_o, steps_o = orc.trace_rk4(dom, s0, dt, orc.default_t_end(ext), "z", "planes", 1)
    sf = a[0]
    assert st_a.ray_steps == steps_o
    assert np.max(np.abs(sf[:3] - sf_o[:3])) <= 1e-10
    assert np.max(np.abs(sf[3:6] - sf_o[3:6])) <= 1e-1
    assert np.max(np.abs(sf[7] - sf_o[7])) <= 1e-8
    vol.close()


# ================================================================ deposit.hip: k_deposit_list, the edge guard's re-deposit (k = 8)
@pytest.mark.gpu
def test_guard_redeposit(eng):
    """The default counts path (mixed trace + edge guard) on test_edge_guard's slab16 case with the refractometry chain at
    bin_scale 1, where the guard sends every ray back through the float64 trace: its queue (k_trace_time's capped launch) and
    k_deposit_list walk more than three trips of 8 x 256 at one compute unit.  The image is the float64 trace's, integer for
    integer, at either grid."""
    import test_edge_guard as tg

    ne, axes, pd, s0 = tg._case("slab16 step")
    n = s0.shape[1]
    vol = tg._volume(eng, ne, axes, pd)
    rays = eng.RayBundle(n).upload(s0)
    ops = eng.chain_refractometry()
    img = eng.DetectorImage.counts(bin_scale=1)
    t_end = eng.default_t_end(tg.EXT)
    rays.trace(vol, t_end, tg.EXT, precision="f64")
    rays.deposit(img, ops)
    ref = img.download()
    rays.trace(vol, t_end, tg.EXT)
    img.zero()
    rays.deposit(img, ops)
    a, again_a = img.download(), rays.retraced
    rays.trace(vol, t_end, tg.EXT)  # the rays the guard traced again hold float64 results now: the mixed trace once more
    img.zero()
    with eng.grid_cus(1):
        rays.deposit(img, ops)
        assert eng.grid_stats() == (2, 2), eng.grid_stats()
    b, again_b = img.download(), rays.retraced
    assert again_a == again_b and again_b > 3 * 8 * 256 and again_b % (8 * 256) != 0, (again_a, again_b, n)
    assert int(ref.sum()) > 0 and np.array_equal(a, ref) and np.array_equal(b, ref)
    img.close()
    vol.close()


# ================================================================ fresnel.hip: the capped launches of the gridding and the propagation
def _fresnel_layout(name):
    import test_fresnel_layouts as tfl

    if name == "random20011" and name not in tfl.LAYOUTS:  # check() and hull_masks() look a layout up by its name
        rng = np.random.RandomState(20011)
        flat = rng.choice(4096 * 4096, 20011, replace=False)
        q = np.arange(-64, 4096 + 65, 96)
        tfl.LAYOUTS[name] = tfl.Layout(name, np.c_[flat % 4096, flat // 4096], q, q, 20011)
    return tfl, tfl.LAYOUTS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("lattice64", "far_corners", "random20011"))
def test_fresnel_gridding(eng, name):
    """grid_rays on test_fresnel_layouts' lattice64 and far_corners (4096 and 4100 rays) and on 20 011 random rays, at the
    device's caps and at one compute unit: that module's exact checks on both (the triangle of a node may differ where several
    are Delaunay: the bin order is the atomics'), every capped launch of the gridding counted."""
    from synthpy_amd.simulator import fresnel_integral as fi

    tfl, L = _fresnel_layout(name)
    assert (L.n + 255) // 256 > 8
    amp, ph = tfl.ray_values(L)
    _, inside, _ = tfl.hull_masks(name)
    for n_cu in (0, 1):
        with eng.grid_cus(n_cu):
            a, p, tri, stats = fi.grid_rays(L.gx, L.gy, L.jones(), amp / 2.0 ** tfl.VAL_BITS, ph / 2.0 ** tfl.VAL_BITS, return_triangles=True)
            launches, short = eng.grid_stats()
        print(f"{name} at {n_cu or 'all'} compute unit(s): {launches} capped launches, {short} with extra trips; {stats}")
        if n_cu:
            # the four passes over the rays always; the second pass's teams only when there are more of them than 4 blocks
            assert launches >= 4 and short >= launches - (1 if stats.second_pass <= 4 else 0) and short >= 4, (launches, short, stats)
        assert np.array_equal(tri[..., 0] >= 0, inside) and stats.outside == int((~inside).sum())
        code = tfl.check(L, tri)
        assert (code == tfl.OK).all(), [tfl.REASON[c] for c in np.unique(code)]
        tfl.assert_close(a, tfl.interpolate(L, tri, amp), 1e-12, f"{name} amplitude")
        tfl.assert_close(p, tfl.interpolate(L, tri, ph), 1e-12, f"{name} phase")


@pytest.mark.gpu
def test_fresnel_propagate_of_rays(eng):
    """propagate (sr_fresnel_rays: the gridding, k_pad_window, k_transfer, k_crop) on lattice64 at one compute unit, by
    test_propagate_of_a_lattice_beam_keeps_its_border's rule: 1e-10 of fresnel_propagate of the field prepared from the exact
    interpolation in the gridding's own triangles."""
    from synthpy_amd.simulator import fresnel_integral as fi

    tfl, L = _fresnel_layout("lattice64")
    amp, ph = tfl.ray_values(L)
    va, vp = amp / 2.0 ** tfl.VAL_BITS, ph / 2.0 ** tfl.VAL_BITS
    ext = float(L.gx[-1] - L.gx[0])
    for n_cu in (0, 1):
        with eng.grid_cus(n_cu):
            tri = fi.grid_rays(L.gx, L.gy, L.jones(), va, vp, return_triangles=True)[2]
        with eng.grid_cus(n_cu):
            out = fi.propagate(tfl.LWL, L.gx, L.gy, ext, ext, L.jones(), va, vp, tfl.Z)
            launches, short = eng.grid_stats()
        assert not n_cu or (launches >= 7 and short >= launches - 1), (launches, short)  # all but, at most, a few second-pass teams
        U0 = tfl.interpolate(L, tri, amp) * np.exp(-1j * tfl.interpolate(L, tri, ph))
        ref = fi.fresnel_propagate(fi.prepare_field_for_propagation(U0), (ext, ext), tfl.LWL, tfl.Z, U0.shape)
        tfl.assert_close(out, ref, 1e-10, f"propagate on lattice64 at {n_cu or 'all'} compute unit(s)")
