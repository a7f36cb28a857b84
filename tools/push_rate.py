"""Rate of the particle push kernel (k_push; sr_particles_push) through N^3 float64 fields.

    python tools/push_rate.py [--grid 256] [--particles 1000000 10000000] [--reps 7] [--out profiles/push_rate.txt]

Cases: 1e6 and 1e7 protons of 14.7 MeV from a point source 10 mm before the box (a cone that overfills the far face, so that part of
the particles leave laterally) through B alone (E absent: the k_push<false, true, double> instantiation) and through E and B; the
particles sorted by entry cell before the upload or in the source's order; random and lattice sources.  The fields stay in HBM
across the cases.  Per case: the kernel's time (HIP events around the launch, what sr_push_stats.kernel_ms returns: median and
minimum of `reps` calls after 1 warm-up call), particle-steps per second, the bytes the steps gather (four corner rows of 48 B per
field and step) over that time, and the ratio to the yardstick.  The yardstick is measured in the same run: hipMemcpyAsync device to
device over a buffer the size of one field, timed by HIP events; a copy reads and writes every byte, so its HBM traffic is twice
the buffer over its time.  Gathered bytes are what the lanes ask for, not HBM traffic: neighbouring particles share lines, which is
what the sort is for.  `idle` is the fraction of lane-steps in which a lane had already left the box while its wavefront (64
consecutive particles of the upload order) still ran: 1 - sum(steps) / sum over wavefronts of 64 * max(steps); it says what a
compaction of the survivors could save at most."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def idle_fraction(steps):
    n = len(steps)
    pad = (-n) % 64
    s = np.concatenate([steps, np.zeros(pad, steps.dtype)]).reshape(-1, 64).astype(np.int64)
    lanes = np.concatenate([np.ones(n, bool), np.zeros(pad, bool)]).reshape(-1, 64)
    ran = (s.max(axis=1)[:, None] * lanes).sum()
    return 1.0 - float(s.sum()) / float(ran)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--particles", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "push_rate.txt"))
    a = ap.parse_args()
    from emission_rate import copy_rate
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
    field_bytes = 8 * 3 * n ** 3
    print(f"fields up after {time.time() - t0:.1f} s", flush=True)
    lines = [f"k_push through {n}^3 float64 vector fields ({field_bytes / 2 ** 30:.2f} GiB each); 14.7 MeV protons, point source 10 mm before "
             f"the box, half-angle 0.4 rad; 1 warm-up + {a.reps} timed calls, HIP events"]
    med, best = copy_rate(field_bytes, a.reps)
    lines.append(f"yardstick: hipMemcpyAsync device to device over {field_bytes / 2 ** 30:.2f} GiB, read + write traffic: "
                 f"median {med / 1e12:.3f} TB/s, best {best / 1e12:.3f} TB/s")
    lines.append(f"{'particles':>9} {'fields':6} {'source':7} {'sort':4} {'kernel ms median':>17} {'min':>9} {'steps/particle':>14} "
                 f"{'particle-steps/s':>16} {'gathered TB/s':>13} {'of copy':>8} {'idle':>6} {'unfinished':>10}")
    try:
        for n_part in a.particles:
            for pattern in ("random", "lattice"):
                src = radiography.ProtonSource(14.7, (0.0, 0.0, -15e-3), "z", half_angle=0.4, n=n_part, seed=1, pattern=pattern)
                dt, max_steps = radiography.default_steps(type("D", (), dict(x=x, y=x, z=x)), src)
                s_in, meets = radiography.entry(src.states(), lo, hi)
                s_in = s_in[:, meets]
                for sort in (True, False):
                    s = np.ascontiguousarray(s_in[:, radiography.entry_cell_order(s_in, g)]) if sort else s_in
                    for name, E in (("B", None), ("E+B", fE)):
                        ms = []
                        for k in range(1 + a.reps):
                            out = engine.push_particles(E, fB, s, src.qm, dt, max_steps, 2, 0.1, want=("steps",))
                            if k >= 1:
                                ms.append(out["stats"].kernel_ms)
                        ms = np.array(ms)
                        steps = out["steps"]
                        total = float(steps.sum(dtype=np.int64))
                        t = np.median(ms) * 1e-3
                        gathered = total * 4 * 48 * (1 if E is None else 2)
                        lines.append(f"{s.shape[1]:9d} {name:6} {pattern:7} {'yes' if sort else 'no':4} {np.median(ms):17.3f} {ms.min():9.3f} "
                                     f"{total / s.shape[1]:14.1f} {total / t:16.3e} {gathered / t / 1e12:13.3f} {gathered / t / med:8.3f} "
                                     f"{idle_fraction(steps):6.3f} {out['stats'].unfinished:10d}")
                        print(lines[-1], flush=True)
    finally:
        fB.close()
        fE.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
