"""Rate of the Zeeman line kernel (k_sightline_zeeman; sr_field_sightline_zeeman) on N^3 float64 fields -- ne, Te, Z, Ti, V and B all
as fields, lines with absorption and a Lorentzian width, no continuum, wing = +inf -- beside k_sightline_voigt
(engine.sightline_voigt) on the same chords, frequencies and table, measured in the same run with the calls alternating.
k_sightline_voigt compiles from what it compiled from at the parent commit (the .inc files it includes only gained functions), so its
time here is the parent's kernel's; profiles/sightline_voigt_rate.txt holds the parent's own record of it.

    python tools/sightline_zeeman_rate.py [--grid 256] [--reps 5] [--resources FILE] [--out profiles/sightline_zeeman_rate.txt]

Workloads, fields, chords, frequencies and widths are tools/sightline_voigt_rate.py's (imported):
  (a) spectrometer   16 chords x 2048 frequencies (sorted) x 1, 8 and 32 lines
  (b) image          a 128x128 oblique pinhole view x 128 frequencies x 8 lines
each with two patterns on every line: the normal triplet (3 components) and the 18-component pattern of J = 7/2 -> 5/2
(g = 1.2, 0.9).  B: every component uniform in +-40 T, node by node.  With wing = +inf no term is dropped, so the Voigt terms of a
call are samples x frequencies x components, counted from the steps the call returns.  Per case: the kernel times (HIP events,
*kernel_ms: median and minimum of `reps` calls after 2 warm-up calls of each entry, the three entries called in turn), Voigt terms
per second, and the ratio to k_sightline_voigt.  --resources: a file holding the output of `python tools/kernel_resources.py
sightline_zeeman.hip`, summarised per instantiation family and appended (without it the tool runs that command).  Nothing is
asserted beyond finite results."""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sightline_lines_rate as base  # noqa: E402
import sightline_voigt_rate as vbase  # noqa: E402

HALF = base.HALF


def summarise_resources(res):
    """kernel_resources.py's lines per (dtype, lane width): the range of VGPRs, AGPRs, spilled VGPRs, static LDS and scratch."""
    fam = {}
    for line in res.splitlines():
        m = re.match(r"\S+: k_sightline_zeeman<(\w+), .*, (\d+)>\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+) / (\d+)\s+(\d+)\s+(\d+)\s+(\d+)", line)
        if m:
            fam.setdefault((m.group(1), int(m.group(2))), []).append([int(v) for v in m.groups()[2:]])
    out = [f"{'dtype':7} {'lanes':>5} {'instantiations':>14} {'VGPR (unified)':>15} {'AGPR':>9} {'VGPRs parked in AGPRs':>22} {'LDS static B':>12} "
           f"{'scratch B/lane':>14} {'waves/SIMD':>10}"]
    for (dt, fl), rows in sorted(fam.items()):
        r = np.array(rows)
        span = lambda c: f"{r[:, c].min()}..{r[:, c].max()}" if r[:, c].min() != r[:, c].max() else f"{r[0, c]}"
        out.append(f"{dt:7} {fl:5d} {len(rows):14d} {span(0):>15} {span(1):>9} {span(3):>22} {span(5):>12} {span(6):>14} {span(7):>10}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sightline_zeeman_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import engine, sightlines
    from synthpy_amd.utils.eos_opacity import ZeemanLineTable, lande_pattern, normal_triplet

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
                  V=np.ascontiguousarray(np.moveaxis(base.flow(P), 0, -1)), B=rng.uniform(-40.0, 40.0, shape + (3,)))
    del P, Z
    f = {k: engine.Field(v, x, x, x) for k, v in arrays.items()}
    del arrays
    common = dict(step=0.5 * cell, max_steps=12 * n)
    patterns = (("triplet", normal_triplet()), ("J 7/2->5/2", lande_pattern(3.5, 1.2, 2.5, 0.9)))
    assert len(patterns[1][1]) == 18
    text = [f"Zeeman-split Voigt lines on {n}^3 float64 fields (ne, Te, Z, Ti, V, B all fields), lines with absorption, no continuum, wing = +inf, "
            f"step = half a cell; 2 warm-up + {a.reps} timed calls of each entry, in turn; kernel ms by HIP events, median [minimum]; "
            f"ZEEMAN_CHUNK = {engine.ZEEMAN_CHUNK}, VOIGT_CHUNK = {engine.VOIGT_CHUNK}",
            f"{'case':30} {'lines':>5} {'pattern':>11} {'comps':>5} {'chords':>6} {'freqs':>5} {'samples/chord':>13} {'zeeman kernel ms':>22} {'Voigt terms':>14} "
            f"{'Voigt terms/s':>14} {'sightline_voigt ms':>22} {'its terms/s':>12} {'zeeman / voigt':>14} {'per component':>13}"]
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
        for case, o, d, nf, counts in (("(a) spectrometer: 16 chords", co, cd, 2048, (1, 8, 32)), ("(b) image: 128x128 pinhole", po, pd, 128, (8,))):
            for n_line in counts:
                gauss, voigt = vbase.make_voigt(n_line)
                om = freqs(gauss, nf)
                kw = dict(omegas=om, continuum=False, toward=-1, **common)
                tables = [ZeemanLineTable.from_lines(voigt, p) for _, p in patterns]
                calls = [lambda: engine.sightline_voigt(f["ne"], f["Te"], f["Ti"], f["Z"], f["V"], o, d, lines=voigt, **kw)]
                calls += [lambda t=t: engine.sightline_zeeman(f["ne"], f["Te"], f["Ti"], f["Z"], f["V"], f["B"], o, d, up, lines=t, **kw) for t in tables]
                ms, outs = [[] for _ in calls], [None] * len(calls)
                for k in range(2 + a.reps):
                    for c, call in enumerate(calls):
                        outs[c] = call()
                        if k >= 2:
                            ms[c].append(f["ne"].last_kernel_ms)
                ms = [np.array(m) for m in ms]
                vterms = int(outs[0]["steps"].sum()) * len(om) * n_line
                for c, (name, p) in enumerate(patterns, 1):
                    out = outs[c]
                    assert all(np.all(np.isfinite(out[k])) for k in ("intensity", "Q", "U", "V")) and np.array_equal(out["steps"], outs[0]["steps"])
                    terms = vterms * len(p)
                    ratio = np.median(ms[c]) / np.median(ms[0])
                    line = (f"{case:30} {n_line:5d} {name:>11} {len(p):5d} {o.shape[1]:6d} {len(om):5d} {float(np.mean(out['steps'])):13.1f} "
                            f"{np.median(ms[c]):12.3f} [{ms[c].min():8.3f}] {terms:14d} {terms / (1e-3 * np.median(ms[c])):14.3e} "
                            f"{np.median(ms[0]):12.3f} [{ms[0].min():8.3f}] {vterms / (1e-3 * np.median(ms[0])):12.3e} {ratio:14.2f} {ratio / len(p):13.2f}")
                    text.append(line)
                    print(line, flush=True)
    finally:
        for v in f.values():
            v.close()
    if a.resources:
        res = open(a.resources).read()
    else:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "sightline_zeeman.hip"], capture_output=True,
                             text=True, check=True).stdout
    text.append("")
    text.append("tools/kernel_resources.py sightline_zeeman.hip, per instantiation family (the dynamic LDS of a launch, 2 x ZEEMAN_CHUNK x (16 + 6 n_line) "
                "x 8 bytes -- 5 632 bytes for one line, 53 248 for 32 -- comes on top of the static figure; 'parked in AGPRs' are VGPRs the compiler "
                "keeps in accumulation registers, not in memory: scratch is 0):")
    text += summarise_resources(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
