"""Rate of the Voigt line kernel (k_sightline_voigt; sr_field_sightline_voigt) on N^3 float64 fields -- ne, Te, Z, Ti and V all as
fields, lines with absorption, no continuum -- beside k_sightline_lines (engine.sightline_lines) on the same chords, frequencies and
table, measured in the same run: the Gaussian kernel is the yardstick, the ratio to it is the number to read.

    python tools/sightline_voigt_rate.py [--grid 256] [--reps 5] [--resources FILE] [--out profiles/sightline_voigt_rate.txt]

Cases, chords, frequencies, Ti and V are tools/sightline_lines_rate.py's (imported):
  (a) spectrometer   16 chords x 2048 frequencies (sorted) x 1, 8 and 32 lines, wing = +inf and wing = 30
  (b) image          a 128x128 oblique pinhole view x 128 frequencies x 8 lines, wing = +inf and wing = 30
The Lorentzian half-width of line l is the same at every lattice node, 10^(-1.5 + 2.2 l/(n_line - 1)) of the thermal width at 300 eV
(0.3 for a single line), so that the damping parameter a = gam/wd of a (sample, line) follows from Ti at the sample's position alone
and the host can count, without a gather of its own, the terms that are COUNTED (|x| <= wing) and the region of V each falls in
(x*x + a*a >= 100: the 10-level continued fraction; otherwise by a: 40 levels for a >= 2, the sampled sums for a <= 0.5 and between).
Per case: the kernel time (HIP events, *kernel_ms: median and minimum of `reps` calls after 2 warm-up calls), counted terms per
second of it, the share of dropped terms, the shares of the counted terms per region, k_sightline_lines' time and the ratio.
--resources: a file holding the output of `python tools/kernel_resources.py sightline_voigt.hip`, appended (without it the tool runs
that command).  Nothing is asserted."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sightline_lines_rate as base  # noqa: E402

LIGHT, E_CH, M_P, HALF = base.LIGHT, base.E_CH, base.M_P, base.HALF


def make_voigt(n_line):
    from synthpy_amd.utils.eos_opacity import VoigtLineTable

    lines = base.make_lines(n_line, True)
    rel = 10.0 ** (-1.5 + 2.2 * np.arange(n_line) / max(n_line - 1, 1)) if n_line > 1 else np.array([0.3])
    gam = rel * lines.thermal_width(300.0)
    return lines, VoigtLineTable.from_lines(lines, np.broadcast_to(gam[:, None, None], lines.emissivity.shape))


def count_terms(lines, om, o, d, toward, steps, lo, hi, wing):
    """(counted, all, per region [CF(10), CF(40), h = 1/4, h = 3/16]) terms; tools/sightline_lines_rate.py's count with a and z2."""
    om = np.sort(om)
    with np.errstate(all="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
    t0 = np.maximum(0.0, np.max(np.where(d == 0, -np.inf, np.minimum(ta, tb)), axis=0))
    t1 = np.min(np.where(d == 0, np.inf, np.maximum(ta, tb)), axis=0)
    unit = d / np.linalg.norm(d, axis=0)
    gam = lines.lorentz_width[:, 0, 0][:, None]
    counted, region = 0, np.zeros(4, np.int64)

    def within(wc, half):
        return np.searchsorted(om, wc + half, side="right") - np.searchsorted(om, wc - half, side="left")

    for k in np.nonzero(steps > 0)[0]:
        n = int(steps[k])
        t = t0[k] + (np.arange(n) + 0.5) * ((t1[k] - t0[k]) / n)
        p = o[:, k:k + 1] + d[:, k:k + 1] * t
        beta = toward * (unit[:, k] @ base.flow(p)) / LIGHT
        wd = lines.omega0[:, None] * np.sqrt(2 * E_CH * base.ion_temperature(p) / (lines.mass_number[:, None] * M_P)) / LIGHT  # (n_line, n)
        wc = lines.omega0[:, None] * (1.0 + beta)
        a = gam / wd
        all_in = within(wc, np.minimum(wing, 1e300) * wd) if np.isfinite(wing) else np.full(wc.shape, len(om))
        near = np.where(a < 10.0, within(wc, np.minimum(np.sqrt(np.maximum(100.0 - a * a, 0.0)), wing) * wd), 0)
        counted += int(all_in.sum())
        region[0] += int((all_in - near).sum())
        region[1] += int(near[a >= 2.0].sum())
        region[2] += int(near[a <= 0.5].sum())
        region[3] += int(near[(a > 0.5) & (a < 2.0)].sum())
    return counted, int(steps.sum()) * len(om) * lines.n_line, region


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sightline_voigt_rate.txt"))
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
    arrays = dict(ne=10.0 ** (18.0 + 2.0 * rng.random(shape)) * Z * 1e6, Te=10.0 + 290.0 * rng.random(shape), Z=Z, Ti=base.ion_temperature(P),
                  V=np.ascontiguousarray(np.moveaxis(base.flow(P), 0, -1)))
    del P, Z
    f = {k: engine.Field(v, x, x, x) for k, v in arrays.items()}
    del arrays
    common = dict(step=0.5 * cell, max_steps=12 * n)
    lo, hi = np.full((3, 1), g[0]), np.full((3, 1), g[-1])
    text = [f"Voigt lines on {n}^3 float64 fields (ne, Te, Z, Ti, V all fields), lines with absorption, no continuum, step = half a cell; 2 warm-up + "
            f"{a.reps} timed calls; kernel ms by HIP events, median [minimum]; VOIGT_CHUNK = {engine.VOIGT_CHUNK}, LINES_CHUNK = {engine.LINES_CHUNK}",
            f"{'case':30} {'lines':>5} {'wing':>5} {'chords':>6} {'freqs':>5} {'samples/chord':>13} {'voigt kernel ms':>20} {'counted terms':>14} {'dropped':>8} "
            f"{'counted terms/s':>16} {'CF(10)':>7} {'CF(40)':>7} {'h=1/4':>7} {'h=3/16':>7} {'sightline_lines ms':>20} {'voigt / lines':>13}"]
    print("\n".join(text), flush=True)

    def timed(call):
        ms, out = [], None
        for k in range(2 + a.reps):
            out = call()
            if k >= 2:
                ms.append(f["ne"].last_kernel_ms)
        return np.array(ms), out

    def freqs(lines, nf):
        return np.linspace(lines.omega0.min() * (1 - 3e-3), lines.omega0.max() * (1 + 3e-3), nf)

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
                gauss, voigt = make_voigt(n_line)
                om = freqs(gauss, nf)
                kw = dict(omegas=om, continuum=False, toward=-1, **common)
                lms, _ = timed(lambda: engine.sightline_lines(f["ne"], f["Te"], f["Ti"], f["Z"], f["V"], o, d, lines=gauss, **kw))
                for wing in (np.inf, 30.0):
                    ms, out = timed(lambda: engine.sightline_voigt(f["ne"], f["Te"], f["Ti"], f["Z"], f["V"], o, d, lines=voigt, wing=wing, **kw))
                    assert np.all(np.isfinite(out["intensity"])) and np.any(out["steps"] > 0)
                    counted, total, region = count_terms(voigt, om, o, d, -1, out["steps"], lo, hi, wing)
                    share = region / max(counted, 1)
                    line = (f"{case:30} {n_line:5d} {wing:5g} {o.shape[1]:6d} {len(om):5d} {float(np.mean(out['steps'])):13.1f} {np.median(ms):11.3f} "
                            f"[{ms.min():7.3f}] {counted:14d} {1 - counted / total:8.3f} {counted / (1e-3 * np.median(ms)):16.3e} "
                            + " ".join(f"{s:7.3f}" for s in share) + f" {np.median(lms):11.3f} [{lms.min():7.3f}] {np.median(ms) / np.median(lms):13.2f}")
                    text.append(line)
                    print(line, flush=True)
    finally:
        for v in f.values():
            v.close()
    if a.resources:
        res = open(a.resources).read()
    else:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "sightline_voigt.hip"], capture_output=True,
                             text=True, check=True).stdout
    text.append("")
    text.append("tools/kernel_resources.py sightline_voigt.hip (the dynamic LDS of a launch, 2 x VOIGT_CHUNK x (10 + 6 n_line) x 8 bytes -- "
                "4 096 bytes for one line, 51 712 for 32 -- comes on top of the static figure):")
    text.append(res.rstrip("\n"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
