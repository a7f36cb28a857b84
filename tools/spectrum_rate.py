"""Warm-call times of the 3-D power spectra from a host array (radial_3Dspectrum, scalar3D_fft, scalar3D_knyquist; the
hipFFT plan cached by the first call), and where one call's time goes: host-to-device copy, FFT, binning.

    python tools/spectrum_rate.py [--sizes 256 512] [--reps 5]     times (median and min of the warm calls)
    python tools/spectrum_rate.py --split OUTDIR [--sizes 512]     the same run under rocprofv3 --kernel-trace
                                                                   --memory-copy-trace --stats; prints the split per call

Output quoted as profiles/r06_spectrum.txt."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = ("radial_3Dspectrum", "scalar3D_fft", "scalar3D_knyquist")


def field(n):
    x = np.linspace(0.0, 1.0, n)
    r = np.random.default_rng(n).standard_normal((n, n, n))
    r += np.sin(2 * np.pi * 3 * x)[:, None, None] + np.cos(2 * np.pi * 5 * x)[None, :, None]
    return r


def times(sizes, reps):
    from synthpy_amd import engine
    from synthpy_amd.utils import power_spectrum as ps

    engine.init(0)
    for n in sizes:
        r = field(n)
        args = {"radial_3Dspectrum": (r, 10.0, 10.0, 10.0), "scalar3D_fft": (r, 0.04),
                "scalar3D_knyquist": (r, 10.0, 10.0, 10.0)}
        for name in CALLS:
            fn = getattr(ps, name)
            t = time.perf_counter()
            fn(*args[name])  # plan creation on the first call of a size
            first = time.perf_counter() - t
            dts = []
            for _ in range(reps):
                t = time.perf_counter()
                fn(*args[name])
                dts.append(time.perf_counter() - t)
            print(f"{n}^3 {name:18s} warm median {np.median(dts) * 1e3:8.1f} ms  min {min(dts) * 1e3:8.1f} ms  "
                  f"({reps} calls; first call {first * 1e3:.0f} ms; field {r.nbytes / 2 ** 30:.2f} GiB)", flush=True)
        del r


def stats(path):
    rows = list(csv.DictReader(open(path))) if path else []
    return [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in rows]


def split(outdir, sizes, reps):
    cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "-d", outdir, "-o", "s", "--output-format",
           "csv", "--", sys.executable, os.path.abspath(__file__), "--sizes", *map(str, sizes), "--reps", str(reps)]
    subprocess.run(cmd, check=True, timeout=1200)
    find = lambda what: (sorted(glob.glob(os.path.join(outdir, "**", f"*{what}_stats.csv"), recursive=True)) or [None])[0]
    kern, copy = stats(find("kernel")), stats(find("memory_copy"))
    n_calls = len(sizes) * len(CALLS) * (reps + 1)
    groups = {"host-to-device copy": 0.0, "to complex (k_to_complex)": 0.0, "FFT (rocFFT kernels)": 0.0,
              "binning (k_spectrum_bins)": 0.0, "device-to-host copy": 0.0}
    for name, _, ns in copy:
        groups["host-to-device copy" if "HOST_TO_DEVICE" in name.upper() else "device-to-host copy"] += ns
    for name, _, ns in kern:
        key = ("binning (k_spectrum_bins)" if "k_spectrum_bins" in name else
               "to complex (k_to_complex)" if "k_to_complex" in name else "FFT (rocFFT kernels)")
        groups[key] += ns
    print(f"\nrocprofv3 split, {n_calls} calls at {'/'.join(f'{n}^3' for n in sizes)} (all three spectra), mean per call:")
    for key, ns in groups.items():
        print(f"  {key:28s} {ns / n_calls / 1e6:9.2f} ms")
    print("kernels:")
    for name, calls, ns in sorted(kern, key=lambda t: -t[2])[:12]:
        print(f"  {name[:90]:90s} {calls:5d} calls  {ns / calls / 1e6:8.3f} ms avg")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--split", metavar="OUTDIR")
    a = ap.parse_args()
    if a.split:
        split(a.split, a.sizes, a.reps)
    else:
        times(a.sizes, a.reps)


if __name__ == "__main__":
    main()
