"""Rate of the sightlines kernel (k_sightlines; sr_field_sightlines) on N^3 float64 fields, Te and Z as fields, beside the grid
marches (sr_field_emission, sr_field_emission_table) on the same fields in the same run.

    python tools/sightlines_rate.py [--grid 512] [--pixels 512] [--reps 5] [--out profiles/sightlines_rate.txt]

Cases, each with the NRL node (one band) and a 10x10 table (one band, with emission opacities: staged into LDS):
  pinhole, backlighter   pixels^2 lines of an oblique sightlines.PinholeCamera / PointBacklighter whose detector covers the box,
                         step = half a cell (the default), handed over in 8x8 tiles in Morton order (sightlines.tile_order) and,
                         for comparison, in plain row-major pixel order
  yardstick              axis-parallel Chords from the lo face through every lateral node with step = the cell size: the samples
                         are the cell midpoints, the work of self_emission / table_emission along that axis (z and x), whose
                         kernel time on the same fields stands beside it
Per case: the kernel's time (HIP events around the launch, what the entry returns in *kernel_ms: median and minimum of `reps`
calls after 2 warm-up calls), the samples marched (the sum of `steps`) and samples per second; for the yardstick the ratio to
the grid march.  Nothing is asserted on the rates."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIGHT = 299792458.0


def table(seed=2):
    from synthpy_amd.utils.eos_opacity import OpacityTable

    rng = np.random.default_rng(seed)
    la = rng.uniform(np.log(1e-1), np.log(1e3), (1, 10, 10))
    le = la + rng.uniform(-1.0, 1.0, la.shape)
    return OpacityTable(np.geomspace(1.0, 500.0, 10), np.geomspace(1e17, 1e21, 10), np.exp(la), [12.4], 12.011, emission=np.exp(le))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--pixels", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sightlines_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import engine, sightlines

    engine.init(0)
    n, m = a.grid, a.pixels
    rng = np.random.default_rng(n)
    half = 5e-3
    x = np.float32(np.linspace(-half, half, n))
    g = np.float64(x)
    cell = float(np.min(np.diff(g)))
    shape = (n, n, n)
    Z = 1.0 + 29.0 * rng.random(shape)
    ne = 10.0 ** (17.0 + 4.0 * rng.random(shape)) * Z * 1e6  # ni over the table's four decades
    Te = 1.0 + 499.0 * rng.random(shape)
    fields = [engine.Field(f, x, x, x) for f in (ne, Te, Z)]
    field_bytes = ne.nbytes
    del ne, Te, Z
    om = np.float64([2 * np.pi * LIGHT / 100e-9])
    tab = table()
    nodes = (("NRL, 1 band", dict(omegas=om)), ("table 10x10, 1 band", dict(table=tab)))
    lines = [f"sightlines kernel on {n}^3 float64 fields ({field_bytes / 2 ** 30:.2f} GiB each), Te and Z as fields; "
             f"2 warm-up + {a.reps} timed calls, HIP events"]
    head = f"{'case':34} {'node':20} {'lines':>8} {'samples':>11} {'kernel ms median':>17} {'min':>8} {'samples/s':>11}"
    lines.append(head + f" {'grid march ms':>14} {'ratio':>6}")
    print("\n".join(lines), flush=True)

    def timed(call):
        ms, out = [], None
        for k in range(2 + a.reps):
            out = call()
            if k >= 2:
                ms.append(fields[0].last_kernel_ms)
        return np.array(ms), out

    def row(case, node, ms, steps, march=None):
        samples = int(np.sum(steps, dtype=np.int64))
        text = (f"{case:34} {node:20} {len(steps):8d} {samples:11d} {np.median(ms):17.3f} {ms.min():8.3f} "
                f"{samples / (np.median(ms) * 1e-3):11.3e}")
        if march is not None:
            text += f" {np.median(march):14.3f} {np.median(ms) / np.median(march):6.2f}"
        lines.append(text)
        print(text, flush=True)

    try:
        D, det = 40e-3, 0.2  # the detector covers the box's width at the distance of its centre: m pixels * pitch * D / det = 2 half
        pitch = 2 * half * (det / D) / m
        views = (("pinhole", sightlines.PinholeCamera((-4e-3, 8e-3, D), (0.1, -0.2, -1.0), (0, 1, 0), det, (m, m), pitch)),
                 ("backlighter", sightlines.PointBacklighter((4e-3, -8e-3, -D), (-0.1, 0.2, 1.0), (0, 1, 0), det, (m, m), pitch, 2e-7)))
        for name, view in views:
            o, d = view.lines()
            perm = view.order()
            for order, (oo, dd) in (("tiles, Morton", (o[:, perm], d[:, perm])), ("row-major", (o, d))):
                for node, kw in nodes:
                    ms, out = timed(lambda: engine.sightlines(*fields, oo, dd, toward=view.toward, step=0.5 * cell, max_steps=12 * n, **kw))
                    assert np.all(np.isfinite(out["intensity"])) and np.any(out["steps"] > 0)
                    row(f"{name} {m}^2, {order}", node, ms, out["steps"])
        for axis in (2, 0):
            lat = [k for k in range(3) if k != axis]
            U, V = np.meshgrid(g, g, indexing="ij")
            o = np.empty((3, n * n))
            o[axis], o[lat[0]], o[lat[1]] = g[0], U.ravel(), V.ravel()
            d = np.zeros((3, n * n))
            d[axis] = 1.0
            for node, kw in nodes:
                if "table" in kw:
                    march, _ = timed(lambda: engine.emission_table(*fields, tab, axis))
                else:
                    march, _ = timed(lambda: engine.emission(*fields, om, axis))
                ms, out = timed(lambda: engine.sightlines(*fields, o, d, toward=+1, step=cell, max_steps=2 * n, **kw))
                assert np.all(out["steps"] >= n - 1)
                row(f"yardstick: Chords along {'xyz'[axis]}, step = cell", node, ms, out["steps"], march)
    finally:
        for f in fields:
            f.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
