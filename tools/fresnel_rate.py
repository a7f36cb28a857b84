"""Warm whole-call times of fresnel_integral.propagate (rays from host arrays -> propagated field on the host) and of the
gridding alone (grid_rays), at 1e6 and 1e7 seeded rays onto 256^2, 512^2 and 1024^2 grids (pad_factor 2: FFTs of 5x the
grid per axis).

    python tools/fresnel_rate.py [--only 1e7x512] [--reps 3]          GPU box: the table (profiles/r06_fresnel.txt)
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/fresnel_rate.py --only 1e7x512 --reps 1
                                                                       GPU box, a run of its own: the kernels' split
    python tools/fresnel_rate.py --reference REF --only 1e6x256       build machine: the reference's propagate (scipy) on the
                                                                       same seeded input, with the CPU count

The rays: uniform over a box 10 % wider than the grid (np.random.RandomState(0)), amplitude and phase smooth functions of
position."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, LWL, Z = 5e-3, 1064e-9, 0.05


def inputs(n, g):
    rng = np.random.RandomState(0)
    jones = np.zeros((4, n))
    jones[0] = rng.uniform(-0.55 * L, 0.55 * L, n)
    jones[2] = rng.uniform(-0.55 * L, 0.55 * L, n)
    amp = 1.0 + 0.3 * np.cos(7.0 * jones[0] / L) * np.sin(5.0 * jones[2] / L)
    phase = 50.0 * (jones[0] ** 2 + jones[2] ** 2) / L ** 2
    x = np.linspace(-L / 2, L / 2, g)
    return x, x.copy(), jones, amp, phase


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one size, e.g. 1e7x512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference", default=None, help="the reference tree: time its propagate on the host instead")
    a = ap.parse_args()
    sizes = [(int(float(n)), g) for n in ("1e6", "1e7") for g in (256, 512, 1024)]
    if a.only:
        n, g = a.only.split("x")
        sizes = [(int(float(n)), int(g))]
    if a.reference:
        sys.path.insert(0, os.path.join(a.reference, "src", "simulator"))
        import fresnel_integral as ref  # the reference (scipy on the host)

        for n, g in sizes:
            x, y, jones, amp, phase = inputs(n, g)
            t0 = time.perf_counter()
            ref.propagate(LWL, x, y, L, L, jones, amp, phase, Z)
            print(f"reference propagate  {n:.0e} rays x {g}^2: {time.perf_counter() - t0:.2f} s  ({os.cpu_count()} CPUs)", flush=True)
        return
    from synthpy_amd import engine
    from synthpy_amd.simulator import fresnel_integral as fi

    engine.init(0)
    for n, g in sizes:
        x, y, jones, amp, phase = inputs(n, g)
        fi.propagate(LWL, x, y, L, L, jones, amp, phase, Z)  # warm: the FFT plan, the device buffers' first touch
        tp, tg = [], []
        for _ in range(a.reps):
            engine.synchronize()
            t0 = time.perf_counter()
            fi.propagate(LWL, x, y, L, L, jones, amp, phase, Z)
            tp.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            *_, stats = fi.grid_rays(x, y, jones, amp, phase, return_triangles=True)
            tg.append(time.perf_counter() - t0)
        print(f"propagate {n:.0e} rays x {g}^2 (FFT {5 * g}^2): {1e3 * min(tp):8.1f} ms (median {1e3 * np.median(tp):.1f});  "
              f"grid_rays alone {1e3 * min(tg):8.1f} ms;  hull {stats.hull_vertices} vertices from {stats.filter_survivors} "
              f"filter survivors, bins {stats.bins_x} x {stats.bins_y}, {stats.outside} nodes outside, "
              f"{stats.second_pass} by the second pass", flush=True)


if __name__ == "__main__":
    main()
