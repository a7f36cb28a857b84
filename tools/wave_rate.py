"""Rate of the wave-optics march (sr_field_wave: hipFFT + k_spectral + k_screen, and k_slab for a z march) on an N^3 float64 domain.

    python tools/wave_rate.py [--grid 512] [--frame 1024] [--reps 5] [--out profiles/wave_rate.txt]

A frame^2 complex128 field (16 MiB at 1024^2) is marched through the N node planes of the domain along x (node planes contiguous:
gathered in place) and along z (node planes strided: brought in as slabs of 32 planes through an LDS transpose).  Per axis: the
whole march (HIP events around it, `kernel_ms[0]`: median and minimum of `reps` calls after one warm-up call), the time per step
(one cell: two transforms, k_spectral, k_screen), and from ONE further call with an event between all the launches (time_parts)
the share of hipFFT against the library's own kernels.  The yardstick is what one step must move at least: four passes over the
field (k_spectral and k_screen each read and write it; the transforms' own passes come on top) plus two node planes of ne."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--frame", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import engine, wave

    engine.init(0)
    n, m = a.grid, a.frame
    lam = 532e-9
    n_crit = (2 * np.pi * 299792458.0 / lam) ** 2 / (5.64e4 ** 2 * 1e-6)
    rng = np.random.default_rng(n)
    x = np.float32(np.linspace(-5e-3, 5e-3, n))
    ne = 0.02 * n_crit * rng.random((n, n, n))
    fld = engine.Field(ne, x, x, x)
    del ne
    src = wave.Source.gaussian((m, m), 8e-3 / m, lam, 1.5e-3)
    absorber = wave.edge_absorber(m, m, 0.1)
    field_bytes, plane_bytes = 16 * m * m, 8 * n * n
    must = 4 * field_bytes + 2 * plane_bytes
    lines = [f"sr_field_wave: a {m}^2 complex128 field ({field_bytes / 2 ** 20:.0f} MiB) through the {n} node planes ({n - 1} cells) of a "
             f"{n}^3 float64 domain, edge absorber on; 1 warm-up + {a.reps} timed calls, HIP events",
             f"one step must move at least 4 x {field_bytes / 2 ** 20:.0f} MiB + 2 x {plane_bytes / 2 ** 20:.0f} MiB = {must / 2 ** 20:.0f} MiB",
             f"{'axis':4} {'march ms median':>16} {'min':>9} {'ms/step':>9} {'must-move TB/s':>15} {'hipFFT ms':>10} {'own ms':>8} "
             f"{'hipFFT share':>13} {'timed-by-parts march ms':>24}"]
    med = {}
    try:
        for axis in (0, 2):
            ms = []
            for k in range(1 + a.reps):
                out, power = engine.wave(fld, None, None, src.U, src.frame, lam, axis, +1, absorber)
                if k >= 1:
                    ms.append(fld.last_kernel_ms)
            assert np.all(np.isfinite(out.view(float))) and np.all(power > 0)
            _, _, (fft_ms, own_ms) = engine.wave(fld, None, None, src.U, src.frame, lam, axis, +1, absorber, time_parts=True)
            whole = fld.last_kernel_ms
            ms = np.array(ms)
            med[axis] = float(np.median(ms))
            step = med[axis] / (n - 1)
            lines.append(f"{'xyz'[axis]:4} {med[axis]:16.3f} {ms.min():9.3f} {step:9.4f} {must / (step * 1e-3) / 1e12:15.3f} {fft_ms:10.3f} "
                         f"{own_ms:8.3f} {fft_ms / (fft_ms + own_ms):13.3f} {whole:24.3f}")
            print(lines[-1], flush=True)
    finally:
        fld.close()
    lines.append(f"z against x: {med[2] / med[0]:.3f} x the time (the z march also reads the whole volume once through k_slab and writes "
                 f"it plane-major: 2 x {8 * n ** 3 / 2 ** 30:.2f} GiB over the march)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
