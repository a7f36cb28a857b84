"""Host mirror of src/field_generator/gaussian1D.py: 1-D Gaussian random fields with a prescribed spectrum.

Every generator draws from the global np.random stream in the reference's order, so a seeded call reproduces the
reference's signal bit for bit and leaves the stream where the reference leaves it (tests/test_field_generators.py,
fixture g13).  `cos(..., device=True)` sums the modes on the GPU (sr_field_modesum); the draws stay on the host.

Quirks decided rather than copied:
  - the reference's progress prints ("This function will generate data up to wavenumber", "Generating 1-D
    turbulence...", the export's success line) are not printed;
  - export_scalar_field(property != 'ne'): the reference opens {fname}.txt and then fails in np.savetxt(None), leaving an
    empty file; here it raises ValueError before any file is touched.
"""
from __future__ import annotations

import numpy as np


class gaussian1D:
    def __init__(self, k_func):
        """k_func(k): spectral power at wavenumber k."""
        self.xc = None
        self.k_func = k_func

    def cos(self, lx, nx, nmodes, wn1, device=False):
        """Mode-sum generator (Shinozuka & Deodatis 1996; gaussian1D.py:26-107): nmodes cosine modes kx = wn with random
        phases phi, amplitudes sqrt(2*E(k)*dk) (no power on dk).  psi is drawn after phi and never used, as the reference
        does, so the stream stays in step.  Returns the (nx,) signal.  device=True: the sum runs on the GPU."""
        dx = lx / nx
        wnn = np.pi / dx
        dk = (wnn - wn1) / nmodes
        wn = wn1 + 0.5 * dk + np.arange(0, nmodes) * dk
        espec = self.k_func(wn).clip(0.0)
        A_m = np.sqrt(2.0 * espec * (np.ones(nmodes) * dk))
        phi = 2.0 * np.pi * np.random.uniform(0.0, 1.0, nmodes)
        np.random.uniform(0.0, 1.0, nmodes)  # psi: drawn, unused
        kx = wn
        self.xc = dx / 2.0 + np.arange(0, nx) * dx
        amp = A_m * np.sqrt(2.0)
        if device:
            from .modesum import modesum

            out = modesum([self.xc], [kx], amp, [phi])
        else:
            arg = kx[None, :] * self.xc[:, None] + phi[None, :]  # (nx, modes)
            out = np.sum(amp * np.cos(arg), axis=-1)
        self.ne = out
        return out

    def fft(self, N, d=1):
        """Timmer & Koenig (1995) generator on a grid of 2N+1 points, frequency spacing from d (gaussian1D.py:109-163)."""
        M = 2 * N + 1
        k = np.fft.fftfreq(M, d)
        K = np.fft.fftshift(np.sqrt(k ** 2))
        Wr = np.random.randn(M)
        Wi = np.random.randn(M)
        Wr = Wr + np.flip(Wr)  # f(-k) = f*(k)
        Wi = Wi - np.flip(Wi)
        F = (Wr + 1j * Wi) * np.sqrt(self.k_func(K))
        F_shift = np.fft.ifftshift(F)
        F_shift[0] = 0  # zero mean
        self.ne = np.fft.ifftn(F_shift).real
        return self.ne

    def domain_fft(self, l_max, l_min, extent, res):
        """Band-limited FFT generator (gaussian1D.py:165-209): spectrum k_func on 2*pi/l_max <= |k| <= 2*pi/l_min (the
        reference's mask keeps the positive frequencies only), complex Gaussian noise, inverse FFT, real part normalised to
        max |field| = 1.  Returns (x, field), 2*res points over [-extent, extent)."""
        dx = extent / res
        x = np.linspace(-extent, extent, 2 * res, endpoint=False)
        self.xc = x
        k = 2 * np.pi * np.fft.fftfreq(2 * res, d=dx)
        k_min, k_max = 2 * np.pi / l_max, 2 * np.pi / l_min
        S = np.zeros_like(k)
        mask = (k >= k_min) & (k <= k_max)
        S[mask] = self.k_func(k[mask])
        noise = np.random.normal(0, 1, k.shape) + 1j * np.random.normal(0, 1, k.shape)
        field = np.fft.ifft(noise * np.sqrt(S)).real
        field = field / np.abs(field).max()
        self.ne = field
        return x, field

    def export_scalar_field(self, property: str = "ne", fname: str = None):
        """Write <fname>.txt, columns (x, field) (gaussian1D.py:211-265).  x is the generator's own xc (cos / domain_fft);
        after fft(N), which keeps none, arange(-(n//2), n//2 + 1).  Default name ./plasma_PVTI_D_M_YYYY_H_MIN."""
        if fname is None:
            import datetime as dt

            now = dt.datetime.now()
            fname = f"./plasma_PVTI_{now.day}_{now.month}_{now.year}_{now.hour}_{now.minute}"
        if property != "ne":
            raise ValueError(f"export_scalar_field: property {property!r} (only 'ne' is exported)")
        if getattr(self, "ne", None) is None:
            raise Exception("No electron density currently loaded!")
        if self.xc is None:
            half = np.shape(self.ne)[0] // 2
            xc = np.arange(-half, half + 1, 1)
        else:
            xc = self.xc
        np.savetxt(f"{fname}.txt", np.column_stack((xc, self.ne)))
