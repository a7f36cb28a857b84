"""Rate of the line-spectra kernel (k_sightline_lines; sr_field_sightline_lines) on N^3 float64 fields -- ne, Te, Z, Ti and V all
as fields, thin lines (no LK) and with absorption, the continuum off and on -- beside engine.sightline_spectra's kernel on the same
chords and frequencies: the yardstick for the added cost, which is the continuum alone.

    python tools/sightline_lines_rate.py [--grid 256] [--reps 5] [--resources FILE] [--out profiles/sightline_lines_rate.txt]

Cases:
  (a) spectrometer   16 chords (a fan through the box) x 2048 frequencies (sorted) x 1, 8 and 32 lines
  (b) image          a 128x128 oblique sightlines.PinholeCamera (8x8 tiles in Morton order) x 128 frequencies x 8 lines
Lines sit 2e-4 w0 apart from 250 nm on; the frequencies span them +- 3e-3 w0.  Ti and V are smooth functions of position put on the
grid, so that the host can count the terms without a gather of its own: a (sample, frequency, line) term is COUNTED when
|omega - wc| <= sqrt(40) wd with wc and wd from Ti and V at the sample's position (the analytic values; the kernel's are the
trilinear ones, a difference of a few terms in a million), everything else is dropped.  Per case: the kernel time (HIP events around
the launch, *kernel_ms: median and minimum of `reps` calls after 2 warm-up calls), counted terms per second of it, the share of
dropped terms, and sightline_spectra's kernel time.  --resources: a file holding the output of
`python tools/kernel_resources.py sightline_lines.hip`, appended (without it the tool runs that command).  Nothing is asserted."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIGHT, E_CH, M_P = 299792458.0, 1.602176634e-19, 1.67262192369e-27
HALF = 5e-3


def ion_temperature(p):
    return 300.0 * (1.0 + 0.6 * np.sin(2 * np.pi * p[0] / (2 * HALF)) * np.cos(np.pi * p[1] / (2 * HALF)))


def flow(p):
    return np.stack([2e5 * np.sin(np.pi * p[1] / HALF), 1e5 * np.cos(np.pi * p[2] / HALF), -1.5e5 * np.sin(np.pi * p[0] / HALF)])


def make_lines(n_line, absorb, lattice=32, seed=3):
    from synthpy_amd.utils.eos_opacity import LineTable

    rng = np.random.default_rng(seed)
    w0 = (2 * np.pi * LIGHT / 250e-9) * (1.0 + 2e-4 * np.arange(n_line))
    T, D = np.geomspace(1.0, 500.0, lattice), np.geomspace(1e17, 1e21, lattice)
    lnK = np.log(2e13 / n_line) + rng.uniform(-1.0, 1.0, (n_line, lattice, lattice))
    t = LineTable(T, D, np.ones((n_line, lattice, lattice)), wavelengths=2 * np.pi * LIGHT / w0, mass_number=12.011)
    J = np.exp(lnK + np.log(t.planck())[:, :, None])
    return LineTable(T, D, J, wavelengths=2 * np.pi * LIGHT / w0, mass_number=12.011, absorption=np.exp(lnK) if absorb else None)


def count_terms(lines, om, o, d, toward, steps, lo, hi):
    """(counted, all) terms of the chords o + d t with `steps` samples each between the faces lo, hi of the box."""
    om = np.sort(om)
    with np.errstate(all="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
    t0 = np.maximum(0.0, np.max(np.where(d == 0, -np.inf, np.minimum(ta, tb)), axis=0))
    t1 = np.min(np.where(d == 0, np.inf, np.maximum(ta, tb)), axis=0)
    unit = d / np.linalg.norm(d, axis=0)
    counted = 0
    for k in np.nonzero(steps > 0)[0]:
        n = int(steps[k])
        t = t0[k] + (np.arange(n) + 0.5) * ((t1[k] - t0[k]) / n)
        p = o[:, k:k + 1] + d[:, k:k + 1] * t
        beta = toward * (unit[:, k] @ flow(p)) / LIGHT
        wd_rel = np.sqrt(2 * E_CH * ion_temperature(p) / (lines.mass_number[:, None] * M_P)) / LIGHT  # (n_line, n)
        wc = lines.omega0[:, None] * (1.0 + beta)
        half = np.sqrt(40.0) * lines.omega0[:, None] * wd_rel
        counted += int(np.sum(np.searchsorted(om, wc + half, side="right") - np.searchsorted(om, wc - half, side="left")))
    return counted, int(steps.sum()) * len(om) * lines.n_line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sightline_lines_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import engine, sightlines

    engine.init(0)
    n = a.grid
    rng = np.random.default_rng(n)
    x = np.float32(np.linspace(-HALF, HALF, n))
    g = np.float64(x)
    cell = float(np.min(np.diff(g)))
    shape = (n, n, n)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"))
    Z = 1.0 + 7.0 * rng.random(shape)
    arrays = dict(ne=10.0 ** (18.0 + 2.0 * rng.random(shape)) * Z * 1e6, Te=10.0 + 290.0 * rng.random(shape), Z=Z, Ti=ion_temperature(P),
                  V=np.ascontiguousarray(np.moveaxis(flow(P), 0, -1)))
    del P, Z
    f = {k: engine.Field(v, x, x, x) for k, v in arrays.items()}
    del arrays
    common = dict(step=0.5 * cell, max_steps=12 * n)
    lo, hi = np.full((3, 1), g[0]), np.full((3, 1), g[-1])
    text = [f"line spectra on {n}^3 float64 fields (ne, Te, Z, Ti, V all fields), step = half a cell; 2 warm-up + {a.reps} timed calls; "
            f"kernel ms by HIP events, median [minimum]; LINES_CHUNK = {engine.LINES_CHUNK}",
            f"{'case':34} {'lines':>5} {'LK':>3} {'cont':>4} {'chords':>6} {'freqs':>5} {'samples/chord':>13} {'kernel ms':>20} {'counted terms':>14} "
            f"{'dropped':>8} {'counted terms/s':>16} {'sightline_spectra ms':>22} {'lines / spectra':>15}"]
    print("\n".join(text), flush=True)

    terms = {}

    def timed(call):
        ms, out = [], None
        for k in range(2 + a.reps):
            out = call()
            if k >= 2:
                ms.append(f["ne"].last_kernel_ms)
        return np.array(ms), out

    def row(case, o, d, toward, om, n_line, absorb, cont, spectra_ms):
        lines = make_lines(n_line, absorb)
        ms, out = timed(lambda: engine.sightline_lines(f["ne"], f["Te"], f["Ti"], f["Z"], f["V"], o, d, lines=lines, omegas=om, continuum=cont,
                                                       toward=toward, **common))
        assert np.all(np.isfinite(out["intensity"])) and np.any(out["steps"] > 0)
        if (case, n_line) not in terms:  # the same for every LK and continuum
            terms[case, n_line] = count_terms(lines, om, o, d, toward, out["steps"], lo, hi)
        counted, total = terms[case, n_line]
        line = (f"{case:34} {n_line:5d} {'yes' if absorb else 'no':>3} {'on' if cont else 'off':>4} {o.shape[1]:6d} {len(om):5d} "
                f"{float(np.mean(out['steps'])):13.1f} {np.median(ms):11.3f} [{ms.min():7.3f}] {counted:14d} {1 - counted / total:8.3f} "
                f"{counted / (1e-3 * np.median(ms)):16.3e} {np.median(spectra_ms):13.3f} [{spectra_ms.min():7.3f}] {np.median(ms) / np.median(spectra_ms):15.2f}")
        text.append(line)
        print(line, flush=True)

    def freqs(n_line, nf):
        w0 = make_lines(n_line, False).omega0
        return np.linspace(w0.min() * (1 - 3e-3), w0.max() * (1 + 3e-3), nf)

    try:
        src = np.array([-3 * HALF, 0.3 * HALF, -0.2 * HALF])
        aim = np.stack([np.zeros(16), np.linspace(-0.8, 0.8, 16) * HALF, np.linspace(0.5, -0.5, 16) * HALF])
        co, cd = np.ascontiguousarray(np.broadcast_to(src[:, None], (3, 16))), np.ascontiguousarray(aim - src[:, None])
        D, det = 40e-3, 0.2
        cam = sightlines.PinholeCamera((-4e-3, 8e-3, D), (0.1, -0.2, -1.0), (0, 1, 0), det, (128, 128), 2 * HALF * (det / D) / 128)
        po, pd = cam.lines()
        perm = cam.order()
        po, pd = np.ascontiguousarray(po[:, perm]), np.ascontiguousarray(pd[:, perm])
        for case, o, d, nf, counts in (("(a) spectrometer: 16 chords", co, cd, 2048, (1, 8, 32)), ("(b) image: 128x128 pinhole", po, pd, 128, (8,))):
            for n_line in counts:
                om = freqs(n_line, nf)
                sms, _ = timed(lambda: engine.sightline_spectra(f["ne"], f["Te"], f["Z"], o, d, omegas=om, toward=-1, **common))
                for absorb, cont in ((False, False), (True, False), (True, True)):
                    row(case, o, d, -1, om, n_line, absorb, cont, sms)
    finally:
        for v in f.values():
            v.close()
    if a.resources:
        res = open(a.resources).read()
    else:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "sightline_lines.hip"], capture_output=True,
                             text=True, check=True).stdout
    text.append("")
    text.append("tools/kernel_resources.py sightline_lines.hip (the dynamic LDS of a launch, 2 x LINES_CHUNK x (10 + 4 n_line) x 8 bytes -- "
                "5 376 bytes for one line, 52 992 for 32 -- comes on top of the static figure):")
    text.append(res.rstrip("\n"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
