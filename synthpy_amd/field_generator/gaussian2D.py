"""Host mirror of src/field_generator/gaussian2D.py: 2-D Gaussian random fields with a prescribed spectrum.

Every generator draws from the global np.random stream in the reference's order, so a seeded call reproduces the
reference's field bit for bit and leaves the stream where the reference leaves it (tests/test_field_generators.py,
fixture g13).  `cos(..., device=True)` sums the modes on the GPU (sr_field_modesum); the draws stay on the host.

Quirks decided rather than copied:
  - the reference's progress prints (cos; the extent print of export_scalar_field) are not printed;
  - export_scalar_field does not import pyvista (the reference imports it and never uses it);
  - export_scalar_field(property != 'ne'): the reference fails with UnboundLocalError after nothing is written; here it
    raises ValueError.  As in the reference, the columns only stack for a square field (nx == ny).
"""
from __future__ import annotations

import numpy as np


class gaussian2D:
    def __init__(self, k_func):
        """k_func(k): spectral power at wavenumber k."""
        self.xc = None
        self.k_func = k_func

    def cos(self, lx, ly, nx, ny, nmodes, wn1, device=False):
        """Mode-sum generator (Shinozuka & Deodatis 1996; gaussian2D.py:18-116): nmodes cosine modes of direction theta,
        amplitudes sqrt(2*E(k)*dk^2); draws phi, psi, theta in that order; each mode adds cos(kx x + ky y + phi) +
        cos(kx x - ky y + psi).  Returns the (nx, ny) field.  device=True: the sum runs on the GPU."""
        dx, dy = lx / nx, ly / ny
        wnn = max(np.pi / dx, np.pi / dy)
        dk = (wnn - wn1) / nmodes
        wn = wn1 + 0.5 * dk + np.arange(0, nmodes) * dk
        espec = self.k_func(wn).clip(0.0)
        A_m = np.sqrt(2.0 * espec * (np.ones(nmodes) * dk) ** 2)
        phi = 2.0 * np.pi * np.random.uniform(0.0, 1.0, nmodes)
        psi = 2.0 * np.pi * np.random.uniform(0.0, 1.0, nmodes)
        theta = 2.0 * np.pi * np.random.uniform(0.0, 1.0, nmodes)
        kx = np.cos(theta) * wn
        ky = np.sin(theta) * wn
        self.xc = dx / 2.0 + np.arange(0, nx) * dx
        self.yc = dy / 2.0 + np.arange(0, ny) * dy
        amp = A_m * np.sqrt(2.0)
        if device:
            from .modesum import modesum

            out = modesum([self.xc, self.yc], [kx, ky], amp, [phi, psi])
        else:
            out = np.zeros((nx, ny))
            ax = kx[None, :] * self.xc[:, None]  # (nx, modes)
            ay = ky[None, :] * self.yc[:, None]  # (ny, modes)
            for i in range(nx):  # row by row: (ny, modes) temporaries stay small
                base = ax[i][None, :]
                s = np.cos(base + ay + phi) + np.cos(base - ay + psi)
                out[i] = np.sum(amp * s, axis=-1)
        self.ne = out
        return out

    def fft(self, N):
        """Timmer & Koenig (1995) generator on a (2N+1)^2 grid (gaussian2D.py:118-167)."""
        M = 2 * N + 1
        k = np.fft.fftfreq(M)
        KX, KY = np.meshgrid(k, k)
        K = np.fft.fftshift(np.sqrt(KX ** 2 + KY ** 2))
        Wr = np.random.randn(M, M)
        Wi = np.random.randn(M, M)
        Wr = Wr + np.flip(Wr)  # f(-k) = f*(k)
        Wi = Wi - np.flip(Wi)
        F = (Wr + 1j * Wi) * np.sqrt(self.k_func(K))
        F_shift = np.fft.ifftshift(F)
        F_shift[0, 0] = 0  # zero mean
        self.ne = np.fft.ifftn(F_shift).real
        return self.ne

    def domain_fft(self, l_max, l_min, extent, res):
        """Band-limited FFT generator (gaussian2D.py:169-217): spectrum k_func on 2*pi/l_max <= k <= 2*pi/l_min, zero
        outside, complex Gaussian noise, inverse FFT, real part normalised to max |field| = 1.  Returns (xx, yy, field):
        meshgrid in its default 'xy' indexing over 2*res points per axis on [-extent, extent)."""
        dx = extent / res
        x = y = np.linspace(-extent, extent, 2 * res, endpoint=False)
        xx, yy = np.meshgrid(x, y)
        self.xc, self.yc = x, y
        kx = ky = 2 * np.pi * np.fft.fftfreq(2 * res, d=dx)
        kxx, kyy = np.meshgrid(kx, ky)
        k = np.sqrt(kxx ** 2 + kyy ** 2)
        k_min, k_max = 2 * np.pi / l_max, 2 * np.pi / l_min
        S = np.zeros_like(k)
        mask = (k >= k_min) & (k <= k_max)
        S[mask] = self.k_func(k[mask])
        noise = np.random.normal(0, 1, k.shape) + 1j * np.random.normal(0, 1, k.shape)
        field = np.fft.ifft2(noise * np.sqrt(S)).real
        field = field / np.abs(field).max()
        self.ne = field
        return xx, yy, field

    def export_scalar_field(self, property: str = "ne", fname: str = None):
        """Write <fname>.pkl, a pickle of concatenate((column_stack((xc, yc)), ne), axis=1): columns x, y, then the field's
        rows (gaussian2D.py:219-284).  xc, yc are the generator's own (cos / domain_fft); after fft(N), which keeps none,
        arange(-(n//2), n//2 + 1) on both.  Default name ./plasma_PVTI_D_M_YYYY_H_MIN."""
        import pickle

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
            xc = yc = np.arange(-half, half + 1, 1)
        else:
            xc, yc = self.xc, self.yc
        values = np.concatenate((np.column_stack((xc, yc)), self.ne), axis=1)
        with open(f"{fname}.pkl", "wb") as fh:
            pickle.dump(values, fh)
