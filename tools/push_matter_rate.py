"""Rate of the particle push through matter (k_push_matter; sr_particles_push_matter) beside the plain push (k_push) in one run.

    python tools/push_matter_rate.py [--grid 256] [--particles 10000000] [--reps 5] [--resources FILE] [--out profiles/push_matter_rate.txt]

tools/push_rate.py's workload: 14.7 MeV protons from a point source 15 mm before a box of N^3 float64 nodes, half-angle 0.4 rad,
sorted by entry cell, through B alone and through E and B.  Per field set three kernels are timed on the same particles (HIP events
around the launch, median and minimum of `reps` calls after 1 warm-up call): k_push; k_push_matter with ne = 0 everywhere -- the same
steps, so the ratio is what the two scalar gathers' eight corner rows (ne alone here: Z is uniform), the path length and the branch
cost; and k_push_matter with aluminium (Z = 3, ne = 1e29 m^-3) in the half z >= 0 of the box, where half of the steps also run the
stopping and scattering lines (a sqrt, two logs, ten divisions).  The particle-steps differ a little there, because slowed particles
take more steps to leave; the ratio is per particle-step.  Then the registers, scratch and waves per SIMD of every instantiation,
from tools/kernel_resources.py (run here, or read from --resources, a file with its output for push.hip and push_matter.hip)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "push_matter_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import engine, radiography

    engine.init(0)
    n = a.grid
    rng = np.random.default_rng(n)
    x = np.float32(np.linspace(-5e-3, 5e-3, n))
    g = [np.float64(x)] * 3
    lo, hi = np.full(3, g[0][0]), np.full(3, g[0][-1])
    t0 = time.time()
    fB = engine.Field(10.0 * rng.standard_normal((n, n, n, 3)), x, x, x)
    fE = engine.Field(1e8 * rng.standard_normal((n, n, n, 3)), x, x, x)
    half = np.zeros((n, n, n))
    half[:, :, n // 2:] = 1e29
    f0, fH = engine.Field(np.zeros((n, n, n)), x, x, x), engine.Field(half, x, x, x)
    del half
    print(f"fields up after {time.time() - t0:.1f} s", flush=True)
    al = radiography.Material.Al()
    src = radiography.ProtonSource(14.7, (0.0, 0.0, -15e-3), "z", half_angle=0.4, n=a.particles, seed=1)
    dt, max_steps = radiography.default_steps(type("D", (), dict(x=x, y=x, z=x)), src)
    s_in, meets = radiography.entry(src.states(), lo, hi)
    s_in = s_in[:, meets]
    s = np.ascontiguousarray(s_in[:, radiography.entry_cell_order(s_in, g)])
    matter = dict(mass=src.mass, z=1.0, Zn=al.Zn, I=al.I, lnLs=al.coulomb_log)
    lines = [f"k_push_matter beside k_push through {n}^3 float64 fields; {s.shape[1]} protons of 14.7 MeV (of {a.particles}: the ones that meet the "
             f"box), point source 15 mm before the box, half-angle 0.4 rad, sorted by entry cell; 1 warm-up + {a.reps} timed calls, HIP events",
             f"{'fields':6} {'kernel':34} {'kernel ms median':>17} {'min':>9} {'steps/particle':>14} {'ns/particle-step':>16} {'ratio to k_push':>15} "
             f"{'stopped':>8}"]
    try:
        for name, E in (("B", None), ("E+B", fE)):
            base = None
            for kernel, ne in (("k_push", None), ("k_push_matter, ne = 0", f0), ("k_push_matter, Al in z >= 0", fH)):
                ms = []
                for k in range(1 + a.reps):
                    if ne is None:
                        out = engine.push_particles(E, fB, s, src.qm, dt, max_steps, 2, 0.1, want=("steps",))
                    else:
                        out = engine.push_particles_matter(E, fB, ne, 3.0, s, src.qm, dt, max_steps, 2, 0.1, want=("steps",), **matter)
                    if k >= 1:
                        ms.append(out["stats"].kernel_ms)
                ms = np.array(ms)
                total = float(out["steps"].sum(dtype=np.int64))
                per = np.median(ms) * 1e6 / total
                base = per if base is None else base
                lines.append(f"{name:6} {kernel:34} {np.median(ms):17.3f} {ms.min():9.3f} {total / s.shape[1]:14.1f} {per:16.4f} {per / base:15.3f} "
                             f"{getattr(out['stats'], 'stopped', 0):8d}")
                print(lines[-1], flush=True)
    finally:
        for f in (fB, fE, f0, fH):
            f.close()
    if a.resources:
        res = open(a.resources).read()
    else:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "push.hip", "push_matter.hip"],
                             capture_output=True, text=True, check=True).stdout
    text = "\n".join(lines) + "\n\n" + "\n".join(l for l in res.splitlines() if "k_push" in l or l.startswith("#")) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
