"""Power spectra of fields and images: mirror of src/utils/power_spectrum.py, every public function of it.

    radial_1Dspectrum, radial_2Dspectrum, radial_3Dspectrum   (r, lx[, ly, lz], smooth=False) -> (knyquist, k_centers, spectrum)
    scalar1D_fft, scalar2D_fft, scalar3D_fft                  (data, dx, k_bin_num=100)       -> (k_bins_weighted, spectrum)
    scalar1D_knyquist, scalar2D_knyquist, scalar3D_knyquist   (r, lx[, ly, lz], smooth=False) -> (knyquist, wave_numbers, spectrum)
    movingaverage                                             (interval, window_size)

The transform and the binning of every mode run on the GPU (hipFFT Z2Z forward and one binning pass,
sr_power_spectrum / sr_radial_spectrum2d); the per-axis coordinates, the bin edges, the returned wavenumbers and the
means are numpy's, computed as the reference computes them (spectrum_prep.py).  Bin membership equals the reference's
mode for mode; the spectrum values differ by FFT and summation order only.

Where the reference cannot run, or runs on a pairing of modes and wavenumbers it did not mean, this mirror decides:
  * radial_2Dspectrum / radial_3Dspectrum on a field with nx != ny: the reference's meshgrid is (ny, nx[, nz]) and its
    mask does not fit the spectrum (IndexError); here index (i, j[, l]) pairs (kx[i], ky[j][, kz[l]]).  With nx == ny
    the reference's pairing (ky[i], kx[j][, kz[l]]) is kept, which matters when lx != ly.
  * scalar2D_fft on a non-square field: the reference runs, but pairs its (My, Mx) grid of |k| with the (Mx, My)
    spectrum by flat index, which scrambles them.  That quirk is not copied: modes pair with their own axis
    frequencies (kx[i], ky[j]).
  * scalar*D_knyquist keep the reference's loop ranges range(-n//2, n//2 - 1) exactly (one index per axis is left
    out; for odd n some indices are binned by their loop value, not their frequency), and raise IndexError where the
    reference indexes past its nx bins (odd cubes such as 9 x 10 x 11, 2-D fields with ny >> nx).
"""
from __future__ import annotations

import numpy as np

from .._ffi import check, lib, ptr
from . import spectrum_prep as prep


def movingaverage(interval, window_size):
    """power_spectrum.py:190-192."""
    window = np.ones(int(window_size)) / float(window_size)
    return np.convolve(interval, window, "same")


def radial_2Dspectrum(r, lx, ly, smooth=False):
    """Radially averaged power spectrum of a 2-D field r (nx, ny) over a domain lx x ly:
    returns (knyquist, k_centers (99,), spectrum (99,)): |fft2(r)|^2/(nx*ny)^2 averaged in 99 log-spaced bins from the
    smallest non-zero wavenumber to the largest; an empty bin is NaN (np.mean of nothing).

    The reference builds its wavenumber grid with np.meshgrid(kx, ky) (shape (ny, nx)) against a spectrum of shape
    (nx, ny) (power_spectrum.py:398-404): it only runs for square fields and then pairs index (i, j) with
    (ky[i], kx[j]).  That pairing is kept for square fields; a non-square field (a whole 2574 x 3448 detector image)
    pairs (kx[i], ky[j])."""
    r = _field(r, 2, "radial_2Dspectrum")
    b, kn, k_centers = prep.radial(r.shape, (lx, ly), 100)
    s = np.zeros(b.n_bins)
    c = np.zeros(b.n_bins, np.uint64)
    check(lib.sr_radial_spectrum2d(ptr(r), r.shape[0], r.shape[1], ptr(b.coords[0]), ptr(b.coords[1]), ptr(b.edges),
                                   len(b.edges), ptr(s), ptr(c)))
    spectrum = _means(s, c)
    if smooth:
        spectrum = movingaverage(spectrum, 5)
    return kn, k_centers, spectrum


def binned_power(r, b: prep.Binning):
    """The GPU pass: |fftn(r)|^2 / b.norm summed and counted per bin of b (sr_power_spectrum).
    Returns (sum, count, overflow): overflow counts the modes of a SHELL binning whose shell is >= b.n_bins."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    shape = np.array(r.shape, dtype=np.int64)
    if r.ndim != len(b.coords) or any(len(c) != n for c, n in zip(b.coords, r.shape)):
        raise ValueError(f"binning for {tuple(len(c) for c in b.coords)} applied to a field of shape {r.shape}")
    coords = np.ascontiguousarray(np.concatenate(b.coords), dtype=np.float64)
    edges = None if b.edges is None else np.ascontiguousarray(b.edges, dtype=np.float64)
    s = np.zeros(b.n_bins)
    c = np.zeros(b.n_bins, np.uint64)
    over = np.zeros(1, np.uint64)
    check(lib.sr_power_spectrum(ptr(r), r.ndim, ptr(shape), ptr(coords), b.rule, ptr(edges), b.n_bins, b.norm, ptr(s),
                                ptr(c), ptr(over)))
    return s, c, int(over[0])


def _means(s, c):
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / c  # an empty bin is NaN, as np.mean of nothing


def _field(r, ndim, name):
    r = np.ascontiguousarray(r, dtype=np.float64)
    if r.ndim != ndim:
        raise ValueError(f"{name} takes a {ndim}-D field, not shape {r.shape}")
    return r


def _radial(r, lengths, num, smooth):
    b, kn, k_centers = prep.radial(r.shape, lengths, num)
    s, c, _ = binned_power(r, b)
    spectrum = _means(s, c)
    if smooth:
        spectrum = movingaverage(spectrum, 5)
    return kn, k_centers, spectrum


def radial_1Dspectrum(r, lx, smooth=False):
    """power_spectrum.py:327-370: |fft(r)|^2/nx^2 averaged in 99 log-spaced bins of the positive wavenumbers
    2 pi fftfreq(nx, lx/nx).  Returns (knyquist, k_centers (99,), spectrum (99,)); an empty bin is NaN."""
    return _radial(_field(r, 1, "radial_1Dspectrum"), (lx,), 100, smooth)


def radial_3Dspectrum(r, lx, ly, lz, smooth=False):
    """power_spectrum.py:423-469: |fftn(r)|^2/(nx*ny*nz)^2 averaged in 49 log-spaced bins of |k|, from the smallest
    non-zero wavenumber to the largest.  Returns (knyquist, k_centers (49,), spectrum (49,)); an empty bin is NaN.
    Index (i, j, l) pairs (ky[i], kx[j], kz[l]) as the reference's meshgrid does when nx == ny; for nx != ny (where the
    reference raises IndexError) it pairs (kx[i], ky[j], kz[l])."""
    return _radial(_field(r, 3, "radial_3Dspectrum"), (lx, ly, lz), 50, smooth)


def _scalar_fft(data, ndim, dx, k_bin_num, name):
    data = _field(data, ndim, name)
    b, k_bins_weighted = prep.scalar_fft(data.shape, dx, k_bin_num)
    spectrum = np.zeros_like(k_bins_weighted)
    if b.n_bins > 0:
        s, c, _ = binned_power(data, b)
        spectrum[: b.n_bins] = _means(s, c)
    return k_bins_weighted, spectrum


def scalar1D_fft(data, dx, k_bin_num=100):
    """power_spectrum.py:9-64: unnormalised |fft(data)|^2 averaged over [(i-1) w, i w), i = 1 .. k_bin_num-1,
    w = max|k| / k_bin_num, k = fftfreq(M, dx).  Returns (k_bins_weighted (midpoints), spectrum (k_bin_num,)); the
    last value stays 0.0, an empty bin is NaN."""
    return _scalar_fft(data, 1, dx, k_bin_num, "scalar1D_fft")


def scalar2D_fft(data, dx, k_bin_num=100):
    """power_spectrum.py:66-121, as scalar1D_fft over |k| = sqrt(kx^2 + ky^2); bin centres are RMS of the edges.
    A non-square field pairs each mode with its own (kx[i], ky[j]) (see the module's notes)."""
    return _scalar_fft(data, 2, dx, k_bin_num, "scalar2D_fft")


def scalar3D_fft(data, dx, k_bin_num=100):
    """power_spectrum.py:123-179, as scalar1D_fft over |k| = sqrt(kx^2 + ky^2 + kz^2); bin centres are the cube
    mean of the edges."""
    return _scalar_fft(data, 3, dx, k_bin_num, "scalar3D_fft")


def _knyquist(r, lengths, smooth):
    b, knorm, kn, wave_numbers = prep.knyquist(r.shape, lengths)
    s, _, over = binned_power(r, b)
    if over:
        raise IndexError(f"index out of bounds for axis 0 with size {b.n_bins}: {over} modes fall in a shell >= nx "
                         "(the reference raises here)")
    tke_spectrum = s / knorm
    if smooth:
        smoothed = movingaverage(tke_spectrum, 5)
        smoothed[0:4] = tke_spectrum[0:4]  # the first 4 values from the original data
        tke_spectrum = smoothed
    return kn, wave_numbers, tke_spectrum


def scalar1D_knyquist(r, lx, smooth=False):
    """power_spectrum.py:194-232: |fft(r)/nx|^2 summed into the integer shells |kx| of the loop kx in
    range(-nx//2, nx//2 - 1), divided by knorm = 2 pi / lx.  Returns (knyquist, wave_numbers (nx,), spectrum (nx,))."""
    return _knyquist(_field(r, 1, "scalar1D_knyquist"), (lx,), smooth)


def scalar2D_knyquist(r, lx, ly, smooth=False):
    """power_spectrum.py:234-276: as scalar1D_knyquist over round(sqrt(kx^2 + ky^2)), knorm the mean of 2 pi/lx and
    2 pi/ly, nx shells; IndexError where a shell reaches nx (the reference's tke_spectrum[k])."""
    return _knyquist(_field(r, 2, "scalar2D_knyquist"), (lx, ly), smooth)


def scalar3D_knyquist(r, lx, ly, lz, smooth=False):
    """power_spectrum.py:278-323: as scalar2D_knyquist over round(sqrt(kx^2 + ky^2 + kz^2)), knorm the mean of the
    three 2 pi/l."""
    return _knyquist(_field(r, 3, "scalar3D_knyquist"), (lx, ly, lz), smooth)
