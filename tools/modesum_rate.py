"""Rates of the cosine mode sum (gaussian{2,3}D.cos(..., device=True), sr_field_modesum): whole-call times from Python, the
kernels' own times under rocprofv3, point-modes per second, and the host mirror's time at a size it finishes.

    python tools/modesum_rate.py [--reps 3]             whole-call times (median, min) of every case
    python tools/modesum_rate.py --split OUTDIR         each case under rocprofv3 --kernel-trace --stats: kernel ms, rates
    python tools/modesum_rate.py --host                 the host mirror at 48^3 x 300 modes

Output quoted as profiles/r06_modesum.txt."""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = 1000
CASES = {"2d4096": (2, 4096), "3d128": (3, 128), "3d256": (3, 256), "3d512": (3, 512)}


def k41(k):
    return k ** (-5.0 / 3.0)


def call(nd, n, nmodes=MODES, device=True):
    from synthpy_amd.field_generator import gaussian2D, gaussian3D

    np.random.seed(1)
    if nd == 2:
        return gaussian2D.gaussian2D(k41).cos(1.0, 1.0, n, n, nmodes, 2 * np.pi, device=device)
    return gaussian3D.gaussian3D(k41).cos(1.0, 1.0, 1.0, n, n, n, nmodes, 2 * np.pi, device=device)


def times(tags, reps):
    from synthpy_amd import engine

    engine.init(0)
    for tag in tags:
        nd, n = CASES[tag]
        t = time.perf_counter()
        call(nd, n)
        first = time.perf_counter() - t
        dts = []
        for _ in range(reps):
            t = time.perf_counter()
            call(nd, n)
            dts.append(time.perf_counter() - t)
        pm = float(n) ** nd * MODES
        print(f"{tag:7s} {n}^{nd} x {MODES} modes  whole call median {np.median(dts) * 1e3:9.1f} ms  min {min(dts) * 1e3:9.1f} ms  "
              f"({reps} calls; first {first * 1e3:.0f} ms)  {pm / min(dts):.3g} point-modes/s", flush=True)


def split(outdir, reps):
    for tag, (nd, n) in CASES.items():
        d = os.path.join(outdir, tag)
        cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "-d", d, "-o", "s", "--output-format", "csv",
               "--", sys.executable, os.path.abspath(__file__), "--cases", tag, "--reps", str(reps)]
        subprocess.run(cmd, check=True, timeout=900)
        f = (sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)) or [None])[0]
        rows = list(csv.DictReader(open(f))) if f else []
        pm = float(n) ** nd * MODES
        for r in rows:
            if "modesum" not in r["Name"]:
                continue
            avg = float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e6
            name = re.search(r"k_modesum(_tables|<[^>]*>)", r["Name"]).group(0)
            rate = f"  {pm / (avg * 1e-3):.3g} point-modes/s" if "tables" not in r["Name"] else ""
            print(f"{tag:7s} {name:24s} {int(r['Calls']):3d} calls  {avg:9.3f} ms avg  min "
                  f"{float(r['MinNs']) / 1e6:9.3f} ms{rate}", flush=True)


def host():
    n, nm = 48, 300
    t = time.perf_counter()
    call(3, n, nm, device=False)
    dt = time.perf_counter() - t
    print(f"host mirror {n}^3 x {nm} modes: {dt:.2f} s  {float(n) ** 3 * nm / dt:.3g} point-modes/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--split", metavar="OUTDIR")
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    if a.host:
        host()
    elif a.split:
        split(a.split, a.reps)
    else:
        times(a.cases, a.reps)


if __name__ == "__main__":
    main()
