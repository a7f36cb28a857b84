"""The cosine mode sum of gaussian1D/2D/3D.cos on the GPU (sr_field_modesum).

The host keeps everything that touches the seeded np.random stream (wavenumbers, amplitudes, the uniform draws, in the
reference's order); this module hands the per-axis cell centres, the wavenumber components, A_m*sqrt(2) and the phases to
the library, which evaluates

    out[i, j, l] = sum_m amp[m] * sum_s cos(k0[m]*x0[i] + sg1(s)*k1[m]*x1[j] + sg2(s)*k2[m]*x2[l] + phase[s][m])

over the reference's 2^(ndim-1) terms (3-D: ++, +-, -+, --; 2-D: +, -; 1-D: +) in float64.
"""
from __future__ import annotations

import numpy as np


def modesum(coords, ks, amp, phases):
    """coords: ndim arrays of cell centres; ks: ndim arrays (nmodes) of wavenumber components; amp: (nmodes);
    phases: 2^(ndim-1) arrays (nmodes).  Returns the float64 field of shape (len(c) for c in coords)."""
    from .._ffi import check, lib, ptr

    ndim = len(coords)
    shape = np.array([len(c) for c in coords], dtype=np.int64)
    c = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in coords]))
    k = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.float64) for v in ks]))
    a = np.ascontiguousarray(amp, dtype=np.float64)
    p = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.float64) for v in phases]))
    assert len(ks) == ndim and len(phases) == 1 << (ndim - 1) and k.shape[1] == a.shape[0] == p.shape[1]
    out = np.empty(tuple(int(n) for n in shape))
    check(lib.sr_field_modesum(ndim, ptr(shape), ptr(c), int(a.shape[0]), ptr(k), ptr(a), ptr(p), ptr(out)))
    return out
