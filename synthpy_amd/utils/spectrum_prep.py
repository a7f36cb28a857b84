"""Host preparation of the power spectra of power_spectrum.py, in numpy alone (no library): the per-axis coordinates the
GPU pass (sr_power_spectrum) bins the modes by, the bin edges, and the arrays the reference returns beside the spectrum.

Everything here is computed as src/utils/power_spectrum.py computes it, from the axes only: the reference's wavenumber
grids are never materialised.  A grid's extremes lie on an axis (the smallest non-zero magnitude) or at the corner (the
largest), and float64 rounding is monotone, so min/max over the axes give the grid's values exactly.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np

EDGES, SHELL = 0, 1  # SR_SPECTRUM_EDGES, SR_SPECTRUM_SHELL (include/synthray.h)


class Binning(NamedTuple):
    """What sr_power_spectrum needs besides the field: coords[d] holds the coordinate of every index d of the
    UNSHIFTED transform (NaN drops the mode), norm divides |F|^2; edges (n_bins + 1) under EDGES, None under SHELL."""
    coords: Tuple[np.ndarray, ...]
    rule: int
    edges: Optional[np.ndarray]
    n_bins: int
    norm: float


def _max_magnitude(axes):
    """max over the grid of sqrt((a0**2 + a1**2) + a2**2): the corner of the per-axis maxima."""
    acc = None
    for a in axes:
        m = np.max(a * a)
        acc = m if acc is None else acc + m
    return np.sqrt(acc)


def _min_positive_magnitude(axes):
    """min over the grid of the magnitude where it is > 0: on an axis, where it is |a| exactly (sqrt(a*a) == |a|)."""
    vals = [np.min(np.abs(a)[np.abs(a) > 0]) for a in axes if np.any(np.abs(a) > 0)]
    if not vals:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")  # numpy's, as k[k>0].min()
    return min(vals)


def radial(shape, lengths, num):
    """radial_1Dspectrum / radial_2Dspectrum (num = 100) and radial_3Dspectrum (num = 50), power_spectrum.py:327-469.
    Returns (Binning, knyquist, k_centers)."""
    ndim = len(shape)
    ks = [2.0 * np.pi * np.fft.fftfreq(n, d=l / n) for n, l in zip(shape, lengths)]
    if ndim == 1:
        # the bins act on the SIGNED shifted k: the negative frequencies never fall in one
        k = ks[0]
        kmin, kmax = np.min(k[k > 0]), np.max(k)
        coords = (np.where(k >= 0, k, np.nan),)
    else:
        # meshgrid(kx, ky[, kz]) is (ny, nx[, nz]): with nx == ny index (i, j[, l]) meets (ky[i], kx[j][, kz[l]]); with
        # nx != ny the reference's mask does not fit the spectrum (IndexError) and the natural pairing is taken
        coords = (ks[1], ks[0]) + tuple(ks[2:]) if shape[0] == shape[1] else tuple(ks)
        kmin, kmax = _min_positive_magnitude(coords), _max_magnitude(coords)
    k_bins = np.logspace(np.log10(kmin), np.log10(kmax), num=num)
    norm = float(int(np.prod(shape, dtype=np.int64)) ** 2)
    b = Binning(tuple(np.ascontiguousarray(c) for c in coords), EDGES, k_bins, num - 1, norm)
    return b, kmax / 2, np.sqrt(k_bins[:-1] * k_bins[1:])


def scalar_fft(shape, dx, k_bin_num=100):
    """scalar1D_fft / scalar2D_fft / scalar3D_fft (power_spectrum.py:9-179): unnormalised |F|^2 averaged over
    [(i-1) w, i w) for i = 1 .. k_bin_num-1, w = max|k| / k_bin_num.  Returns (Binning, k_bins_weighted); the GPU bins
    fill the spectrum's first k_bin_num - 1 values, the last stays 0.0."""
    ndim = len(shape)
    coords = tuple(np.fft.fftfreq(m, dx) for m in shape)  # pairs by axis (the 2-D reference pairs a non-square field by flat index)
    w = _max_magnitude(coords) / k_bin_num
    k_bins = w * np.arange(0, k_bin_num + 1)
    if ndim == 1:
        k_bins_weighted = 0.5 * (k_bins[:-1] + k_bins[1:])
    elif ndim == 2:
        k_bins_weighted = (0.5 * (k_bins[:-1] ** 2 + k_bins[1:] ** 2)) ** (1 / 2)
    else:
        k_bins_weighted = (0.5 * (k_bins[:-1] ** 3 + k_bins[1:] ** 3)) ** (1 / 3)
    return Binning(coords, EDGES, k_bins[:k_bin_num], k_bin_num - 1, 1.0), k_bins_weighted


def loop_values(n):
    """The reference's loop range(-n//2, n//2 - 1) as a coordinate per storage index (tkeh[v] is index v mod n): one
    index per axis is never visited (NaN), and for odd n index n//2 + 1.. carry their loop value, not their frequency."""
    s = np.full(n, np.nan)
    v = np.arange(-n // 2, n // 2 - 1)
    s[v % n] = v
    return s


def knyquist(shape, lengths):
    """scalar1D_knyquist / scalar2D_knyquist / scalar3D_knyquist (power_spectrum.py:194-323): |fftn(r)/nt|^2 summed into
    the integer shells round(sqrt(kx^2 + ky^2 + kz^2)) < nx, then divided by knorm.
    Returns (Binning, knorm, knyquist, wave_numbers)."""
    ndim = len(shape)
    nx = shape[0]
    nt = int(np.prod(shape, dtype=np.int64))
    k0 = [2.0 * np.pi / l for l in lengths]
    if ndim == 1:
        knorm = k0[0]
        kn = knorm * nx / 2
    elif ndim == 2:
        knorm = (k0[0] + k0[1]) / 2.0
        kn = knorm * min(shape) / 2
    else:
        knorm = (k0[0] + k0[1] + k0[2]) / 3.0
        kn = knorm * min(shape) / 2
    wave_numbers = knorm * np.arange(0, nx)
    b = Binning(tuple(loop_values(n) for n in shape), SHELL, None, nx, float(nt * nt))
    return b, knorm, kn, wave_numbers
