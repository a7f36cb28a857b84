"""Rate of the sightline-spectra kernel (k_sightline_spectra; sr_field_sightline_spectra) on N^3 float64 fields, Te and Z as
fields, beside the only other way to the same numbers: ceil(F / 4) calls of engine.sightlines (k_sightlines, 4 bands a call) on the
same lines, in the same process.

    python tools/sightline_spectra_rate.py [--grid 256] [--reps 5] [--out profiles/sightline_spectra_rate.txt]

Cases, each with the NRL node and a table on a 64x64 lattice (with emission opacities):
  (a) spectrometer   16 chords (a fan through the box) x 2048 frequencies; table: 16 chords x 128 groups
  (b) image          a 256x256 oblique sightlines.PinholeCamera (8x8 tiles in Morton order) x 64 frequencies / groups
  (c) lane width     FL = 64 against FL = 256 (SYNTHRAY_SPECTRA_FL) at 64, 96 and 128 frequencies, on (a)'s chords and on a 128x128
                     pinhole view: which width should serve 65..128 frequencies; and at 256 and 320: whether 256 is right above
step = half a cell (the default).  Per case: the new entry's kernel time (HIP events around the launch, *kernel_ms: median and
minimum of `reps` calls after 2 warm-up calls) and its wall time; for the loop the SUM of the calls' kernel times and the wall time
of the whole loop (median of `reps` loops after 1 warm-up loop); the ratios loop / new.  One spectrum is compared with the loop's
bits.  Nothing is asserted on the rates."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIGHT = 299792458.0


def spectral_table(nf, lattice=64, seed=2):
    from synthpy_amd.utils.eos_opacity import SpectralOpacityTable

    rng = np.random.default_rng(seed)
    la = rng.uniform(np.log(1e-1), np.log(1e3), (nf, lattice, lattice))
    le = la + rng.uniform(-1.0, 1.0, la.shape)
    e = np.geomspace(30.0, 3000.0, nf)
    return SpectralOpacityTable(np.geomspace(1.0, 500.0, lattice), np.geomspace(1e17, 1e21, lattice), np.exp(la), e, 12.011, emission=np.exp(le))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sightline_spectra_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import engine, sightlines

    engine.init(0)
    n = a.grid
    rng = np.random.default_rng(n)
    half = 5e-3
    x = np.float32(np.linspace(-half, half, n))
    cell = float(np.min(np.diff(np.float64(x))))
    shape = (n, n, n)
    Z = 1.0 + 29.0 * rng.random(shape)
    ne = 10.0 ** (17.0 + 4.0 * rng.random(shape)) * Z * 1e6  # ni over the table's four decades
    Te = 1.0 + 499.0 * rng.random(shape)
    fields = [engine.Field(f, x, x, x) for f in (ne, Te, Z)]
    del ne, Te, Z
    common = dict(step=0.5 * cell, max_steps=12 * n)
    lines = [f"sightline spectra on {n}^3 float64 fields, Te and Z as fields, step = half a cell; new: 2 warm-up + {a.reps} timed calls; "
             f"loop of engine.sightlines calls (4 bands each): 1 warm-up + {a.reps} timed loops; kernel ms by HIP events, medians [minimum]"]
    lines.append(f"{'case':44} {'node':12} {'lines':>6} {'freqs':>6} {'samples/line':>12} {'new kernel ms':>20} {'new wall ms':>12} "
                 f"{'loop calls':>10} {'loop kernel ms':>20} {'loop wall ms':>12} {'kernel x':>9} {'wall x':>7}")
    print("\n".join(lines), flush=True)

    def node_kw(kind, nf, bands=None):
        if kind == "NRL":
            om = 2 * np.pi * LIGHT / np.geomspace(1064e-9, 100e-9, nf)
            return dict(omegas=om if bands is None else om[bands])
        if nf not in tables:
            tables[nf] = spectral_table(nf)
        t = tables[nf]
        return dict(table=t if bands is None else t.bands(bands))

    tables = {}

    def new(o, d, toward, kind, nf):
        ms, wall, out = [], [], None
        for k in range(2 + a.reps):
            t0 = time.perf_counter()
            out = engine.sightline_spectra(*fields, o, d, toward=toward, **node_kw(kind, nf), **common)
            if k >= 2:
                wall.append(1e3 * (time.perf_counter() - t0))
                ms.append(fields[0].last_kernel_ms)
        return np.array(ms), np.array(wall), out

    def loop(o, d, toward, kind, nf):
        groups = [np.arange(k, min(k + 4, nf)) for k in range(0, nf, 4)]
        kws = [node_kw(kind, nf, b) for b in groups]
        ms, wall, outs = [], [], None
        for k in range(1 + a.reps):
            t0 = time.perf_counter()
            total, outs = 0.0, []
            for kw in kws:
                outs.append(engine.sightlines(*fields, o, d, toward=toward, want=("intensity", "optical_depth"), **kw, **common))
                total += fields[0].last_kernel_ms
            if k >= 1:
                wall.append(1e3 * (time.perf_counter() - t0))
                ms.append(total)
        return np.array(ms), np.array(wall), outs, len(groups)

    def row(case, kind, o, d, toward, nf, against_loop=True):
        ms, wall, out = new(o, d, toward, kind, nf)
        assert np.all(np.isfinite(out["intensity"])) and np.any(out["steps"] > 0)
        per_line = float(np.mean(out["steps"]))
        text = (f"{case:44} {kind:12} {o.shape[1]:6d} {nf:6d} {per_line:12.1f} {np.median(ms):11.3f} [{ms.min():7.3f}] {np.median(wall):12.2f}")
        if against_loop:
            lms, lwall, outs, calls = loop(o, d, toward, kind, nf)
            same = all(np.array_equal(out["intensity"][:, 4 * k:4 * k + 4].T, r["intensity"])
                       and np.array_equal(out["optical_depth"][:, 4 * k:4 * k + 4].T, r["optical_depth"]) for k, r in enumerate(outs))
            text += (f" {calls:10d} {np.median(lms):11.3f} [{lms.min():7.3f}] {np.median(lwall):12.2f} {np.median(lms) / np.median(ms):9.2f} "
                     f"{np.median(lwall) / np.median(wall):7.2f}   same bits: {same}")
        lines.append(text)
        print(text, flush=True)
        return np.median(ms)

    try:
        # 16 chords: a fan from a point beside the box through its middle
        src = np.array([-3 * half, 0.3 * half, -0.2 * half])
        aim = np.stack([np.zeros(16), np.linspace(-0.8, 0.8, 16) * half, np.linspace(0.5, -0.5, 16) * half])
        co, cd = np.ascontiguousarray(np.broadcast_to(src[:, None], (3, 16))), np.ascontiguousarray(aim - src[:, None])
        D, det = 40e-3, 0.2

        def camera(m):
            cam = sightlines.PinholeCamera((-4e-3, 8e-3, D), (0.1, -0.2, -1.0), (0, 1, 0), det, (m, m), 2 * half * (det / D) / m)
            o, d = cam.lines()
            perm = cam.order()
            return np.ascontiguousarray(o[:, perm]), np.ascontiguousarray(d[:, perm])

        row("(a) spectrometer: 16 chords", "NRL", co, cd, -1, 2048)
        row("(a) spectrometer: 16 chords", "table 64x64", co, cd, -1, 128)
        po, pd = camera(256)
        row("(b) image: 256x256 pinhole", "NRL", po, pd, -1, 64)
        row("(b) image: 256x256 pinhole", "table 64x64", po, pd, -1, 64)
        qo, qd = camera(128)
        for nf in (64, 96, 128, 256, 320):
            for kind in ("NRL", "table 64x64"):
                for name, (o, d) in (("16 chords", (co, cd)), ("128x128 pinhole", (qo, qd))):
                    got = {}
                    for fl in (64, 256):
                        os.environ["SYNTHRAY_SPECTRA_FL"] = str(fl)
                        got[fl] = row(f"(c) FL = {fl}: {name}", kind, o, d, -1, nf, against_loop=False)
                    del os.environ["SYNTHRAY_SPECTRA_FL"]
                    text = f"{'':44} FL 64 / FL 256 at {nf} frequencies, {name}, {kind}: {got[64] / got[256]:.2f}"
                    lines.append(text)
                    print(text, flush=True)
    finally:
        os.environ.pop("SYNTHRAY_SPECTRA_FL", None)
        for f in fields:
            f.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
