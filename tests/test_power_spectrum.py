"""The power spectra of utils/power_spectrum.py (src/utils/power_spectrum.py of the reference): radial_1D/3Dspectrum,
scalar1D/2D/3D_fft and scalar1D/2D/3D_knyquist, transformed and binned on the GPU (sr_power_spectrum).

Against the reference's own outputs (tests/golden/g12_spectra.npz, made by tests/golden/make_g12_spectra.py): returned
wavenumbers equal, empty bins at the same places, values to 1e-12.  Beyond the fixtures' sizes, against a vectorised
numpy restatement of the reference (np.fft.fftn + np.bincount over the bins the reference's grids give): counts exactly
equal, sums to FFT round-off.  The host preparation (spectrum_prep.py) is checked without the library or a GPU.
"""
import numpy as np
import pytest

from conftest import golden

from synthpy_amd.utils import spectrum_prep as prep

TAGS = ("d1a", "d1b", "d2a", "d3a", "d3b", "d3c")
RADIAL_NUM = {1: 100, 3: 50}


def case(g, tag):
    r = g[f"r_{tag}"]
    return r, tuple(float(v) for v in g[f"l_{tag}"]), float(g[f"dx_{tag}"])


# ---------------------------------------------------------------- numpy restatements (the reference, vectorised)
def grid(axes, indexing):
    """the magnitude sqrt((a0**2 + a1**2) + a2**2) over the meshgrid of the axes, numpy's rounding"""
    G = np.meshgrid(*axes, indexing=indexing) if len(axes) > 1 else [axes[0]]
    K = G[0] ** 2
    for A in G[1:]:
        K = K + A ** 2
    return np.sqrt(K)


def bincount(idx, w, n):
    return np.bincount(idx, weights=w, minlength=n)[:n], np.bincount(idx, minlength=n)[:n].astype(np.uint64)


def edge_bins(K, P, edges):
    ok = (K >= edges[0]) & (K < edges[-1])
    return bincount(np.searchsorted(edges, K[ok], side="right") - 1, P[ok], len(edges) - 1)


def power(r):
    F = np.fft.fftn(r)
    return F.real ** 2 + F.imag ** 2


def np_radial(r, lengths):
    """radial_1D/3Dspectrum: the reference's k grid (1-D: signed; 3-D: meshgrid in 'xy' order, nx == ny), unshifted
    (the reference shifts the spectrum and the grid alike).  Returns (edges, sum, count)."""
    ks = [2.0 * np.pi * np.fft.fftfreq(n, d=l / n) for n, l in zip(r.shape, lengths)]
    K = ks[0] if r.ndim == 1 else grid(ks, "xy")
    edges = np.logspace(np.log10(K[K > 0].min()), np.log10(K.max()), num=RADIAL_NUM[r.ndim])
    return (edges,) + edge_bins(K.ravel(), power(r).ravel() / (r.size ** 2), edges)


def np_scalar_fft(r, dx, k_bin_num=100):
    """scalar*D_fft: bins [(i-1) w, i w) of |k| over the 'ij' grid of fftfreq (by axis, also for a non-square 2-D
    field).  Returns (sum, count) of the k_bin_num - 1 bins."""
    K = grid([np.fft.fftfreq(m, dx) for m in r.shape], "ij")
    w = K.max() / k_bin_num
    return edge_bins(K.ravel(), power(r).ravel(), w * np.arange(0, k_bin_num))


def np_knyquist(r):
    """scalar*D_knyquist: the loops range(-n//2, n//2 - 1) per axis, shells round(sqrt(sum k^2)), tkeh[kx, ky, kz].
    Returns (sum, count) over the nx shells (asserts none reaches nx)."""
    loops = [np.arange(-n // 2, n // 2 - 1) for n in r.shape]
    rh = np.fft.fftn(r) / r.size
    tkeh = (rh * np.conj(rh)).real
    shell = np.round(grid([v.astype(np.float64) for v in loops], "ij")).astype(np.int64).ravel()
    w = tkeh[np.ix_(*loops)].ravel()
    assert shell.max() < r.shape[0]
    return bincount(shell, w, r.shape[0])


# ---------------------------------------------------------------- host preparation: no library, no GPU
def test_host_preparation_equals_reference_arrays():
    """coordinates, edges, centres, knyquist and wave_numbers from spectrum_prep equal the reference's returned arrays
    bit for bit; the numpy restatement of the GPU pass on prep's coordinates gives the reference's spectra."""
    g = golden("g12_spectra")
    for tag in TAGS:
        r, lengths, dx = case(g, tag)
        nd = r.ndim
        if f"radial_kc_{tag}" in g:
            b, kn, kc = prep.radial(r.shape, lengths, RADIAL_NUM[nd])
            assert kn == g[f"radial_kn_{tag}"] and np.array_equal(kc, g[f"radial_kc_{tag}"]), tag
            s, c = np_binning(r, b)
            with np.errstate(invalid="ignore"):
                assert_spectrum(s / c, g[f"radial_sp_{tag}"], f"radial {tag}")
        if f"fft_kw_{tag}" in g:
            for key, kbn in (("fft", 100), ("fft7", 7)):
                b, kw = prep.scalar_fft(r.shape, dx, kbn)
                assert np.array_equal(kw, g[f"{key}_kw_{tag}"]), (tag, key)
                s, c = np_binning(r, b)
                sp = np.zeros(kbn)
                with np.errstate(invalid="ignore"):
                    sp[:-1] = s / c
                assert_spectrum(sp, g[f"{key}_sp_{tag}"], f"{key} {tag}")
        if f"kny_wn_{tag}" in g:
            b, knorm, kn, wn = prep.knyquist(r.shape, lengths)
            assert kn == g[f"kny_kn_{tag}"] and np.array_equal(wn, g[f"kny_wn_{tag}"]), tag
            s, _ = np_binning(r, b)
            assert_spectrum(s / knorm, g[f"kny_sp_{tag}"], f"knyquist {tag}")
    g7 = golden("g7_spectrum")  # radial_2Dspectrum's fixture: the same preparation
    for tag in "abc":
        img = g7[f"img_{tag}"]
        b, kn, kc = prep.radial(img.shape, tuple(g7[f"l_{tag}"]), 100)
        assert kn == g7[f"kn_{tag}"] and np.array_equal(kc, g7[f"kc_{tag}"]), tag
        s, c = np_binning(img, b)
        with np.errstate(invalid="ignore"):
            assert_spectrum(s / c, g7[f"sp_{tag}"], f"radial 2-D {tag}")


def test_knyquist_loop_values():
    """range(-n//2, n//2 - 1) read as tkeh[v]: one storage index left out, odd n's upper half by loop value"""
    assert np.array_equal(prep.loop_values(8), [0, 1, 2, np.nan, -4, -3, -2, -1], equal_nan=True)
    assert np.array_equal(prep.loop_values(9), [0, 1, 2, np.nan, -5, -4, -3, -2, -1], equal_nan=True)
    assert np.isnan(prep.loop_values(1)).all()


def np_binning(r, b):
    """what sr_power_spectrum computes, in numpy, from a Binning: m over the coordinates' 'ij' grid, NaN dropped"""
    m = grid(list(b.coords), "ij").ravel()
    P = power(r).ravel() / b.norm
    if b.rule == prep.EDGES:
        return edge_bins(m, P, b.edges)
    ok = ~np.isnan(m)
    sh = np.rint(m[ok]).astype(np.int64)
    assert sh.max() < b.n_bins
    return bincount(sh, P[ok], b.n_bins)


def assert_spectrum(sp, ref, what, rtol=1e-12):
    assert sp.shape == ref.shape, what
    assert np.array_equal(np.isnan(sp), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    assert np.all(np.abs(sp[ok] - ref[ok]) <= rtol * np.abs(ref[ok])), (what, np.max(np.abs(sp[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-300)))


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ps():
    from synthpy_amd import engine
    from synthpy_amd.utils import power_spectrum

    engine.init(0)
    return power_spectrum


@pytest.mark.gpu
def test_spectra_vs_reference(ps):
    """every helper on every fixture input against the reference's outputs, smooth=True included"""
    g = golden("g12_spectra")
    for tag in TAGS:
        r, lengths, dx = case(g, tag)
        nd = r.ndim
        if f"radial_kc_{tag}" in g:
            fn = getattr(ps, f"radial_{nd}Dspectrum")
            kn, kc, sp = fn(r, *lengths)
            assert kn == pytest.approx(float(g[f"radial_kn_{tag}"]), rel=1e-15)
            assert np.allclose(kc, g[f"radial_kc_{tag}"], rtol=1e-15, atol=0)
            assert_spectrum(sp, g[f"radial_sp_{tag}"], f"radial {tag}")
            assert_spectrum(fn(r, *lengths, smooth=True)[2], g[f"radial_sps_{tag}"], f"radial smooth {tag}", 1e-11)
        if f"fft_kw_{tag}" in g:
            fn = getattr(ps, f"scalar{nd}D_fft")
            for key, kbn in (("fft", 100), ("fft7", 7)):
                kw, sp = fn(r, dx, k_bin_num=kbn)
                assert np.allclose(kw, g[f"{key}_kw_{tag}"], rtol=1e-15, atol=0), (tag, key)
                assert sp[-1] == 0.0
                assert_spectrum(sp, g[f"{key}_sp_{tag}"], f"{key} {tag}")
        if f"kny_wn_{tag}" in g:
            fn = getattr(ps, f"scalar{nd}D_knyquist")
            kn, wn, sp = fn(r, *lengths)
            assert kn == pytest.approx(float(g[f"kny_kn_{tag}"]), rel=1e-15)
            assert np.allclose(wn, g[f"kny_wn_{tag}"], rtol=1e-15, atol=0)
            assert_spectrum(sp, g[f"kny_sp_{tag}"], f"knyquist {tag}")
            assert_spectrum(fn(r, *lengths, smooth=True)[2], g[f"kny_sps_{tag}"], f"knyquist smooth {tag}", 1e-11)


def check_bins(s, c, s_ref, c_ref, what):
    """counts exactly; sums to 1e-10 |ref| + 1e-18 max(ref) (FFT round-off is absolute in the field's norm)"""
    assert np.array_equal(c, c_ref), (what, np.flatnonzero(c != c_ref)[:10])
    tol = 1e-10 * np.abs(s_ref) + 1e-18 * np.max(s_ref)
    worst = float(np.max(np.abs(s - s_ref) / tol))
    print(f"{what}: {int(c.sum())} modes in {len(c)} bins, worst |sum - ref| / tolerance {worst:.3g}")
    assert worst <= 1.0, what


def check_all_3(ps, r, lengths, dx, what):
    b, _, _ = prep.radial(r.shape, lengths, 50 if r.ndim == 3 else 100)
    s, c, _ = ps.binned_power(r, b)
    edges, s_ref, c_ref = np_radial(r, lengths)
    assert np.array_equal(b.edges, edges), what
    check_bins(s, c, s_ref, c_ref, f"radial {what}")
    b, _ = prep.scalar_fft(r.shape, dx)
    s, c, _ = ps.binned_power(r, b)
    check_bins(s, c, *np_scalar_fft(r, dx), f"scalar_fft {what}")
    b, _, _, _ = prep.knyquist(r.shape, lengths)
    s, c, over = ps.binned_power(r, b)
    assert over == 0
    check_bins(s, c, *np_knyquist(r), f"knyquist {what}")


@pytest.mark.gpu
def test_gaussian3D_volume_256(ps):
    """a 256^3 turbulent volume made on the GPU (gaussian3D.domain_fft), its three 3-D spectra"""
    from synthpy_amd.field_generator.gaussian3D import gaussian3D

    np.random.seed(3)
    ne = gaussian3D(lambda k: k ** (-11 / 3)).domain_fft(1.0, 0.05, 5, 128, 1.0, device=True)
    assert ne.shape == (256, 256, 256)
    check_all_3(ps, ne, (10.0, 10.0, 10.0), 0.04, "256^3")
    kn, kc, sp = ps.radial_3Dspectrum(ne, 10, 10, 10)  # the reference notebooks' call
    assert sp.shape == kc.shape == (49,) and kn > 0


@pytest.mark.gpu
def test_odd_prime_sizes(ps):
    """101 x 101 x 97: hipFFT's non-power-of-two paths, odd loop ranges"""
    r = np.random.default_rng(5).standard_normal((101, 101, 97))
    check_all_3(ps, r, (3.0, 5.0, 4.0), 0.1, "101x101x97")


@pytest.mark.gpu
def test_long_1d(ps):
    """10^7 points: the shell spectrum's 10^7 bins go through the global atomics"""
    n = 10 ** 7
    x = np.linspace(0.0, 1.0, n)
    r = np.random.default_rng(6).standard_normal(n) + 3.0 * np.sin(2 * np.pi * 40 * x)
    check_all_3(ps, r, (2.0,), 1e-3, "1e7")


@pytest.mark.gpu
def test_index_errors(ps):
    """knyquist where the reference indexes past its nx bins"""
    rng = np.random.default_rng(7)
    with pytest.raises(IndexError):
        ps.scalar3D_knyquist(rng.standard_normal((9, 10, 11)), 1.0, 1.0, 1.0)
    with pytest.raises(IndexError):
        ps.scalar2D_knyquist(rng.standard_normal((8, 64)), 1.0, 1.0)
    ps.scalar2D_knyquist(rng.standard_normal((64, 8)), 1.0, 1.0)  # the other way round fits


@pytest.mark.gpu
def test_decided_pairings(ps):
    """radial_3Dspectrum with nx != ny (the reference raises) and scalar2D_fft on a non-square field (the reference
    scrambles): modes pair with their own axes' wavenumbers"""
    rng = np.random.default_rng(8)
    r = rng.standard_normal((24, 18, 20))
    lengths = (2.0, 3.0, 4.0)
    kn, kc, sp = ps.radial_3Dspectrum(r, *lengths)
    ks = [2.0 * np.pi * np.fft.fftfreq(n, d=l / n) for n, l in zip(r.shape, lengths)]
    K = grid(ks, "ij").ravel()
    edges = np.logspace(np.log10(K[K > 0].min()), np.log10(K.max()), num=50)
    s_ref, c_ref = edge_bins(K, power(r).ravel() / r.size ** 2, edges)
    assert kn == K.max() / 2 and np.array_equal(kc, np.sqrt(edges[:-1] * edges[1:]))
    with np.errstate(invalid="ignore"):
        assert_spectrum(sp, s_ref / c_ref, "radial_3D 24x18x20")
    d = rng.standard_normal((40, 26))
    kw, sp = ps.scalar2D_fft(d, 0.5)
    s_ref, c_ref = np_scalar_fft(d, 0.5)
    with np.errstate(invalid="ignore"):
        assert_spectrum(sp[:-1], s_ref / c_ref, "scalar2D_fft 40x26")
    assert sp[-1] == 0.0
