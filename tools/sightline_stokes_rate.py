"""Rate of the polarised-transfer kernel (k_sightline_stokes; sr_field_sightline_stokes) on N^3 float64 fields beside
k_sightline_zeeman (engine.sightline_zeeman) on the same chords, frequencies and table, measured in the same run with the calls
alternating.  k_sightline_zeeman compiles from what it compiled from at the parent commit (its helpers moved into zeeman_node.inc
unchanged), so its time here is the parent's kernel's; profiles/sightline_zeeman_rate.txt holds the parent's own record of it.

    python tools/sightline_stokes_rate.py [--grid 256] [--reps 5] [--resources FILE] [--out profiles/sightline_stokes_rate.txt]

Workloads, fields, chords, frequencies, widths and patterns are tools/sightline_zeeman_rate.py's:
  (a) spectrometer   16 chords x 2048 frequencies (sorted) x 1, 8 and 32 lines
  (b) image          a 128x128 oblique pinhole view x 128 frequencies x 8 lines
with the normal triplet on every line, and for 8 lines of (a) the 18-component pattern of J = 7/2 -> 5/2 as well.  Three entries
are called in turn, 2 warm-up calls and `reps` timed ones each (kernel ms by HIP events, *kernel_ms; median and minimum):
  zeeman     engine.sightline_zeeman, the table with absorption: one Voigt profile per term, the scalar update
  profiles   engine.sightline_stokes on the same table WITHOUT absorption, faraday off: both profiles per term (voigt_w) and, every
             sample being on the scalar shortcut, sr_field_sightline_zeeman's update (and its bits)
  stokes     engine.sightline_stokes, the table with absorption, faraday on, a polarised backlight: both profiles and the 4 x 4
             update (13 Horner steps and s squarings) on every sample the lines or the continuum's rotation reach
So stokes - profiles is what the matrix update costs beyond the scalar one ("update share": that difference over stokes), and
profiles - zeeman what the second profile costs (the table's absorption changes neither entry's work per term).  The spread of s is
not a kernel output; what the file records is s of a sample with its chord's MEAN eI*h = tau/steps, a lower bound of the typical s
(K's row-sum norm is at least eI): the share of (chord, frequency) pairs per s.  --resources: a file holding the output of `python tools/kernel_resources.py
sightline_stokes.hip`, summarised per instantiation family and appended (without it the tool runs that command).  Nothing is
asserted beyond finite results and the bits of the shortcut."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sightline_lines_rate as base  # noqa: E402
import sightline_voigt_rate as vbase  # noqa: E402
import sightline_zeeman_rate as zbase  # noqa: E402

HALF = base.HALF
OUT = os.path.join(ROOT, "profiles", "sightline_stokes_rate.txt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from synthpy_amd import engine, sightlines
    from synthpy_amd.utils.eos_opacity import ZeemanLineTable, lande_pattern, normal_triplet

    try:
        engine.init(0)
    except Exception as e:  # a session without a GPU leaves the record saying so
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(f"k_sightline_stokes beside k_sightline_zeeman: not measured yet (no GPU in the session that wrote this file: {type(e).__name__}).\n"
                     "Run `python tools/sightline_stokes_rate.py` on an MI355X to fill it in.\n")
        print("no GPU: wrote 'not measured yet' to", a.out)
        return
    n = a.grid
    rng = np.random.default_rng(n)
    x = np.float32(np.linspace(-HALF, HALF, n))
    g = np.float64(x)
    cell = float(np.min(np.diff(g)))
    shape = (n, n, n)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"))
    Z = 1.0 + 7.0 * rng.random(shape)
    arrays = dict(ne=10.0 ** (18.0 + 2.0 * rng.random(shape)) * Z * 1e6, Te=10.0 + 290.0 * rng.random(shape), Z=Z, Ti=base.ion_temperature(P),
                  V=np.ascontiguousarray(np.moveaxis(base.flow(P), 0, -1)), B=rng.uniform(-40.0, 40.0, shape + (3,)))
    del P, Z
    f = {k: engine.Field(v, x, x, x) for k, v in arrays.items()}
    del arrays
    common = dict(step=0.5 * cell, max_steps=12 * n)
    triplet, wide = ("triplet", normal_triplet()), ("J 7/2->5/2", lande_pattern(3.5, 1.2, 2.5, 0.9))
    text = [f"Polarised transfer on {n}^3 float64 fields (ne, Te, Z, Ti, V, B all fields), Voigt lines, no continuum, wing = +inf, step = half a cell; "
            f"2 warm-up + {a.reps} timed calls of each entry, in turn; kernel ms by HIP events, median [minimum]; STOKES_CHUNK = {engine.STOKES_CHUNK}, "
            f"ZEEMAN_CHUNK = {engine.ZEEMAN_CHUNK}",
            f"{'case':30} {'lines':>5} {'pattern':>11} {'comps':>5} {'chords':>6} {'freqs':>5} {'samples/chord':>13} {'zeeman ms':>22} {'profiles ms':>22} "
            f"{'stokes ms':>22} {'profiles/zeeman':>15} {'stokes/zeeman':>13} {'update share':>12} {'tau max':>9}  share of pairs by s at the mean eI*h (s: %)"]
    print("\n".join(text), flush=True)

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
        up = np.array([0.0, 1.0, 0.0])
        work = [("(a) spectrometer: 16 chords", co, cd, 2048, 1, triplet), ("(a) spectrometer: 16 chords", co, cd, 2048, 8, triplet),
                ("(a) spectrometer: 16 chords", co, cd, 2048, 8, wide), ("(a) spectrometer: 16 chords", co, cd, 2048, 32, triplet),
                ("(b) image: 128x128 pinhole", po, pd, 128, 8, triplet)]
        for case, o, d, nf, n_line, (pname, pat) in work:
            gauss, voigt = vbase.make_voigt(n_line)
            om = freqs(gauss, nf)
            kw = dict(omegas=om, continuum=False, toward=-1, **common)
            full = ZeemanLineTable.from_lines(voigt, pat)
            bare = ZeemanLineTable.from_lines(voigt, pat)
            bare.absorption = None
            back = np.full((o.shape[1], nf), 1e-3)
            args = (f["ne"], f["Te"], f["Ti"], f["Z"], f["V"], f["B"], o, d, up)
            calls = [lambda: engine.sightline_zeeman(*args, lines=full, **kw),
                     lambda: engine.sightline_stokes(*args, lines=bare, **kw),
                     lambda: engine.sightline_stokes(*args, lines=full, backlight=back, polarisation=(0.6, 0.0, 0.3), faraday=True, **kw)]
            ms, outs = [[] for _ in calls], [None] * len(calls)
            for k in range(2 + a.reps):
                for c, call in enumerate(calls):
                    outs[c] = call()
                    if k >= 2:
                        ms[c].append(f["ne"].last_kernel_ms)
            ms = [np.array(m) for m in ms]
            for out in outs:
                assert all(np.all(np.isfinite(out[k])) for k in ("intensity", "Q", "U", "V")) and np.array_equal(out["steps"], outs[0]["steps"])
            shortcut = engine.sightline_zeeman(*args, lines=bare, **kw)
            assert all(np.array_equal(shortcut[k], outs[1][k]) for k in ("intensity", "Q", "U", "V", "optical_depth"))
            med = [float(np.median(m)) for m in ms]
            tau, steps = outs[2]["optical_depth"], np.maximum(outs[2]["steps"], 1)[:, None]
            with np.errstate(divide="ignore"):
                s = np.maximum(0, np.ceil(np.log2(np.maximum(tau / steps, 1e-300) / 0.25))).astype(int)
            hist = np.bincount(s.ravel())
            spread = ", ".join(f"{k}: {100.0 * v / s.size:.1f}" for k, v in enumerate(hist) if v)
            line = (f"{case:30} {n_line:5d} {pname:>11} {len(pat):5d} {o.shape[1]:6d} {len(om):5d} {float(np.mean(outs[0]['steps'])):13.1f} "
                    + " ".join(f"{np.median(m):12.3f} [{m.min():8.3f}]" for m in ms)
                    + f" {med[1] / med[0]:15.2f} {med[2] / med[0]:13.2f} {(med[2] - med[1]) / med[2]:12.2f} {float(tau.max()):9.2e}  {spread}")
            text.append(line)
            print(line, flush=True)
    finally:
        for v in f.values():
            v.close()
    if a.resources:
        res = open(a.resources).read()
    else:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "sightline_stokes.hip"], capture_output=True,
                             text=True, check=True).stdout
    text.append("")
    text.append("tools/kernel_resources.py sightline_stokes.hip, per instantiation family (the dynamic LDS of a launch, 2 x STOKES_CHUNK x (18 + 6 n_line) "
                "x 8 bytes -- 6 144 bytes for one line, 53 760 for 32 -- comes on top of the static figure; scratch is 0):")
    text += zbase.summarise_resources(res.replace("k_sightline_stokes<", "k_sightline_zeeman<"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
