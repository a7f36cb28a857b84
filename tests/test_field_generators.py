"""The field generators of synthpy_amd/field_generator (src/field_generator/gaussian{1,2,3}D.py of the reference): the host
mirrors of cos, fft and domain_fft against the reference's own seeded outputs (tests/golden/g13_fields.npz, made by
tests/golden/make_g13_fields.py) bit for bit, with the global np.random stream left where the reference leaves it; the
exports; and cos(..., device=True), the mode sum on the GPU (sr_field_modesum), against the fixtures, the host mirror and,
at 256^3 x 1000 modes, the reference's expression evaluated directly at sampled cells.
"""
import ctypes as C
import pickle

import numpy as np
import pytest

from conftest import golden

import synthpy_amd.field_generator.gaussian1D as g1
import synthpy_amd.field_generator.gaussian2D as g2
import synthpy_amd.field_generator.gaussian3D as g3


def k41(k):
    return k ** (-5.0 / 3.0)


def k_neg(k):
    return k ** (-5.0 / 3.0) * (9.0 - k)


def k_fft(k):
    return 1.0 / (1.0 + (20.0 * k) ** 2)


SPECTRA = {"k41": k41, "k_neg": k_neg, "k_fft": k_fft}
CLASSES = {1: g1.gaussian1D, 2: g2.gaussian2D, 3: g3.gaussian3D}
# the cases of make_g13_fields.py: tag -> (dimension, spectrum, method, arguments, seed)
CASES = {
    "cos1a": (1, "k41", "cos", (1.0, 64, 100, 2 * np.pi), 3),
    "cos1b": (1, "k41", "cos", (2.5, 37, 1, 0.7), 4),
    "cos1n": (1, "k_neg", "cos", (1.0, 50, 80, 1.0), 5),
    "cos2a": (2, "k41", "cos", (1.0, 1.3, 24, 20, 60, 2 * np.pi / 1.3), 6),
    "cos2n": (2, "k_neg", "cos", (1.0, 1.0, 16, 16, 40, 1.0), 7),
    "cos3a": (3, "k41", "cos", (1.0, 1.3, 0.7, 12, 10, 8, 40, 4.0), 3),
    "cos3n": (3, "k_neg", "cos", (1.0, 1.0, 1.0, 8, 8, 8, 30, 1.0), 8),
    "fft1a": (1, "k_fft", "fft", (50, 1), 9),
    "fft1b": (1, "k_fft", "fft", (40, 0.5), 10),
    "fft2a": (2, "k_fft", "fft", (20,), 11),
    "dom1a": (1, "k41", "domain_fft", (1.0, 0.05, 1.0, 64), 12),
    "dom2a": (2, "k41", "domain_fft", (1.0, 0.05, 1.0, 24), 13),
}
COS = [t for t in CASES if t.startswith("cos")]


@pytest.fixture(scope="module")
def g13():
    return golden("g13_fields")


def run(tag, **kw):
    """the mirror's call of a case, seeded; returns (generator, outputs as a tuple, the next np.random.random())"""
    nd, spec, method, args, seed = CASES[tag]
    np.random.seed(seed)
    g = CLASSES[nd](SPECTRA[spec])
    with np.errstate(all="ignore"):
        r = getattr(g, method)(*args, **kw)
    return g, (r if isinstance(r, tuple) else (r,)), np.random.random()


# ---------------------------------------------------------------- host mirrors: no library, no GPU
@pytest.mark.parametrize("tag", list(CASES))
def test_host_mirror_equals_reference(g13, tag):
    """every output, the generator's xc / yc / zc and the stream position equal the reference's bit for bit"""
    g, outs, nxt = run(tag)
    n_out = len([f for f in g13.files if f.endswith("_" + tag) and f.startswith("out")])
    assert len(outs) == n_out, (tag, len(outs), n_out)
    for q, v in enumerate(outs):
        ref = g13[f"out{q}_{tag}"]
        assert v.shape == ref.shape and v.dtype == ref.dtype, (tag, q, v.shape, ref.shape)
        assert np.array_equal(v, ref, equal_nan=True), (tag, q, np.nanmax(np.abs(v - ref)))
    assert np.array_equal(g.ne, outs[-1])
    for ax in ("xc", "yc", "zc"):
        if f"{ax}_{tag}" in g13.files:
            assert np.array_equal(getattr(g, ax), g13[f"{ax}_{tag}"]), (tag, ax)
    assert nxt == float(g13[f"next_{tag}"]), f"{tag}: the stream is not where the reference leaves it"


def test_negative_spectrum_modes_are_clipped(g13):
    """k_neg is negative past k = 9: those modes carry no amplitude (fields of only the low modes differ from k41's)"""
    for tag in ("cos1n", "cos2n", "cos3n"):
        assert np.all(np.isfinite(g13[f"out0_{tag}"])) and np.abs(g13[f"out0_{tag}"]).max() > 0, tag


def test_module_paths_as_the_reference_scripts_write_them():
    import importlib

    for nd in (1, 2, 3):
        mod = importlib.import_module(f"synthpy_amd.field_generator.gaussian{nd}D")
        cls = getattr(mod, f"gaussian{nd}D")
        g = cls(k41)
        assert g.xc is None and g.k_func is k41
        for name in ("cos", "fft", "domain_fft", "export_scalar_field"):
            assert callable(getattr(g, name)), (nd, name)
    from synthpy_amd.field_generator.gaussian1D import gaussian1D  # noqa: F401
    from synthpy_amd.field_generator.gaussian2D import gaussian2D  # noqa: F401


def test_export_1d_txt(tmp_path):
    """{fname}.txt, columns (xc, ne); after fft(N): x = arange(-(n//2), n//2 + 1)"""
    g, (ne,), _ = run("cos1a")
    g.export_scalar_field(fname=str(tmp_path / "a"))
    back = np.loadtxt(tmp_path / "a.txt")
    assert back.shape == (64, 2)
    assert np.array_equal(back[:, 0], g.xc) and np.array_equal(back[:, 1], ne)
    g, (ne,), _ = run("fft1a")
    g.export_scalar_field("ne", str(tmp_path / "b"))
    back = np.loadtxt(tmp_path / "b.txt")
    assert np.array_equal(back[:, 0], np.arange(-50, 51)) and np.array_equal(back[:, 1], ne)
    with pytest.raises(ValueError):
        g.export_scalar_field("B", str(tmp_path / "c"))
    assert not (tmp_path / "c.txt").exists()
    with pytest.raises(Exception, match="No electron density"):
        g1.gaussian1D(k41).export_scalar_field(fname=str(tmp_path / "d"))


def test_export_2d_pkl(tmp_path):
    """{fname}.pkl: concatenate((column_stack((xc, yc)), ne), axis=1); after fft(N): arange(-(n//2), n//2 + 1) twice"""
    g, (ne,), _ = run("cos2n")
    g.export_scalar_field(fname=str(tmp_path / "a"))
    with open(tmp_path / "a.pkl", "rb") as fh:
        v = pickle.load(fh)
    assert v.shape == (16, 18)
    assert np.array_equal(v[:, 0], g.xc) and np.array_equal(v[:, 1], g.yc) and np.array_equal(v[:, 2:], ne)
    g, (ne,), _ = run("fft2a")
    g.export_scalar_field("ne", str(tmp_path / "b"))
    with open(tmp_path / "b.pkl", "rb") as fh:
        v = pickle.load(fh)
    assert np.array_equal(v[:, 0], np.arange(-20, 21)) and np.array_equal(v[:, 1], np.arange(-20, 21))
    assert np.array_equal(v[:, 2:], ne)
    with pytest.raises(ValueError):
        g.export_scalar_field("B", str(tmp_path / "c"))
    assert not (tmp_path / "c.pkl").exists()


def test_modesum_rejects_bad_arguments():
    """argument errors come back as SR_ERR_INVALID with text, before the device is touched"""
    from synthpy_amd import _ffi

    lib, ptr = _ffi.lib, _ffi.ptr
    shape, c = np.array([4, 5, 6], dtype=np.int64), np.zeros(15)
    k, a, p, out = np.zeros((3, 3)), np.zeros(3), np.zeros((4, 3)), np.zeros(120)

    def call(ndim=3, shape_=shape, c_=c, nmodes=3, k_=k, a_=a, p_=p, out_=out):
        rc = lib.sr_field_modesum(ndim, ptr(shape_), ptr(c_), nmodes, ptr(k_), ptr(a_), ptr(p_), ptr(out_))
        return rc, _ffi.last_error()

    for kw in ({"shape_": None}, {"c_": None}, {"k_": None}, {"a_": None}, {"p_": None}, {"out_": None}):
        rc, err = call(**kw)
        assert rc == -1 and "NULL" in err, (kw, rc, err)
    for nd in (0, 4, -1):
        rc, err = call(ndim=nd)
        assert rc == -1 and "ndim" in err, (nd, rc, err)
    for bad in ([0, 5, 6], [4, -2, 6], [4, 5, 0]):
        rc, err = call(shape_=np.array(bad, dtype=np.int64))
        assert rc == -1 and "bad size" in err, (bad, rc, err)
    for nm in (0, -3):
        rc, err = call(nmodes=nm)
        assert rc == -1 and "nmodes" in err, (nm, rc, err)
    assert C.c_int(lib.sr_field_modesum(2, ptr(shape), ptr(c), 3, ptr(k), ptr(a), None, ptr(out))).value == -1


# ---------------------------------------------------------------- cos(..., device=True): the mode sum on the GPU
@pytest.fixture(scope="module")
def dev():
    from synthpy_amd import engine

    engine.init(0)
    return engine


def assert_close(a, ref, rel, what):
    scale = np.abs(ref).max()
    err = np.abs(a - ref).max()
    assert a.shape == ref.shape and a.dtype == np.float64, (what, a.shape, ref.shape, a.dtype)
    assert err <= rel * scale, f"{what}: max |diff| {err:.3e} > {rel:g} * {scale:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("tag", COS)
def test_device_cos_equals_reference(dev, g13, tag):
    g, (ne,), nxt = run(tag, device=True)
    assert_close(ne, g13[f"out0_{tag}"], 1e-12, tag)
    assert g.ne is ne
    for ax in ("xc", "yc", "zc"):
        if f"{ax}_{tag}" in g13.files:
            assert np.array_equal(getattr(g, ax), g13[f"{ax}_{tag}"]), (tag, ax)
    assert nxt == float(g13[f"next_{tag}"]), f"{tag}: device=True leaves the stream elsewhere"


# (dimension, cos arguments, seed): awkward sizes, axes of length 1, one mode, a wide 2-D field, a long 1-D signal
AWKWARD = [
    (3, (1.0, 1.1, 0.9, 40, 33, 29, 257, 3.0), 21),
    (3, (1.0, 1.0, 1.0, 1, 17, 70, 64, 2.0), 22),
    (3, (1.0, 1.0, 1.0, 20, 1, 9, 64, 2.0), 23),
    (3, (1.0, 1.0, 1.0, 13, 11, 1, 64, 2.0), 24),
    (3, (1.0, 2.0, 3.0, 9, 7, 5, 1, 2.0), 25),
    (2, (1.0, 0.8, 300, 200, 1000, 2 * np.pi), 26),
    (2, (1.0, 1.0, 1, 50, 30, 2.0), 27),
    (2, (1.0, 1.0, 70, 1, 1, 2.0), 28),
    (1, (3.0, 5000, 300, 1.0), 29),
    (1, (1.0, 1, 5, 1.0), 30),
]


@pytest.mark.gpu
@pytest.mark.parametrize("nd,args,seed", AWKWARD)
def test_device_cos_equals_host_mirror(dev, nd, args, seed):
    out = {}
    for device in (False, True):
        np.random.seed(seed)
        out[device] = (CLASSES[nd](k41).cos(*args, device=device), np.random.random())
    assert_close(out[True][0], out[False][0], 1e-12, f"{nd}-D {args}")
    assert out[True][1] == out[False][1]


@pytest.mark.gpu
def test_device_cos_256_against_reference_expression(dev):
    """256^3 x 1000 modes (the host mirror would take ~35 min): the reference's four-cosine expression evaluated in numpy
    at 2048 sampled cells, from the same seeded draws"""
    n, nm, seed = 256, 1000, 31
    L = (1.0, 1.2, 0.8)
    np.random.seed(seed)
    g = g3.gaussian3D(k41)
    ne = g.cos(*L, n, n, n, nm, 2.0, device=True)
    # the reference's draws (gaussian3D.py:19-151), restated
    dx, dy, dz = (v / n for v in L)
    wnn = max(np.pi / dx, np.pi / dy, np.pi / dz)
    dk = (wnn - 2.0) / nm
    wn = 2.0 + 0.5 * dk + np.arange(0, nm) * dk
    A_m = np.sqrt(2.0 * k41(wn).clip(0.0) * (np.ones(nm) * dk) ** 3)
    np.random.seed(seed)
    psi = [2.0 * np.pi * np.random.uniform(0.0, 1.0, nm) for _ in range(4)]
    theta = 2.0 * np.pi * np.random.uniform(0.0, 1.0, nm)
    phi = 2.0 * np.pi * np.random.uniform(0.0, 1.0, nm)
    kx, ky, kz = np.sin(theta) * np.cos(phi) * wn, np.sin(theta) * np.sin(phi) * wn, np.cos(theta) * wn
    rng = np.random.default_rng(256)
    idx = rng.integers(0, n, size=(2048, 3))
    idx[:8] = [[0, 0, 0], [n - 1, n - 1, n - 1], [0, n - 1, 0], [n - 1, 0, n - 1], [5, 255, 128], [255, 3, 0], [0, 0, 255],
               [128, 128, 128]]
    x, y, z = g.xc[idx[:, 0], None], g.yc[idx[:, 1], None], g.zc[idx[:, 2], None]
    s = (np.cos(kx * x + ky * y + kz * z + psi[0]) + np.cos(kx * x + ky * y - kz * z + psi[1]) +
         np.cos(kx * x - ky * y + kz * z + psi[2]) + np.cos(kx * x - ky * y - kz * z + psi[3]))
    ref = np.sum(A_m * np.sqrt(2.0) * s, axis=-1)
    got = ne[idx[:, 0], idx[:, 1], idx[:, 2]]
    scale = np.abs(ne).max()
    assert np.abs(got - ref).max() <= 1e-11 * scale, (np.abs(got - ref).max(), scale)



@pytest.mark.gpu
def test_device_cos_is_repeatable(dev):
    """two calls on the same draws, bit-identical fields (fixed summation order, no atomics)"""
    for nd, args in ((3, (1.0, 1.1, 0.9, 96, 70, 130, 500, 3.0)), (2, (1.0, 1.0, 333, 257, 700, 2.0))):
        out = []
        for _ in range(2):
            np.random.seed(41)
            out.append(CLASSES[nd](k41).cos(*args, device=True))
        assert np.array_equal(out[0], out[1]), nd
