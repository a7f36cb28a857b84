"""Rate of the line-integral kernel (k_project, sr_volume_project) on a grid^3 volume, with the phase field alone and with the
phase, kappa and Faraday fields; the same sums in NumPy on the host; and, on the C3 turbulent volume, how far the traced phase
of real (refracted, slightly divergent) rays is from the line integral at their launch positions.

    python tools/project_rate.py [--grid 512] [--reps 10] [--rays 2e5] [--out profiles/project_rate.txt]
    python tools/project_rate.py --case phase|all [--grid N] [--reps K]     one case alone: what the first form profiles

Kernel times come from `rocprofv3 --kernel-trace --stats`, each case in a run of its own (2 warm-up calls + `reps`); the rate is
the bytes of records the kernel reads (sr_volume_bytes: 16 B per packed node, + 4 with the phase, + 8 kappa, + 32 {n_e, B})
over the kernel's average time, set against the 6.3 TB/s a float4 copy reaches on an MI355X.  Whole-call times (host clock
around Volume.project(), which ends in a device synchronise and includes the download of the six maps) are taken with the
profiler off.  The last figure is a physics number, not a pass mark."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # B/s
LWL, EXT = 1064e-9, 5e-3


def volume(engine, grid, case):
    """A grid^3 volume with smooth fields (the kernel's time does not depend on the values): (volume, host arrays)."""
    x = np.linspace(-EXT, EXT, grid)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij", sparse=True)
    ne = 1e25 * (1.0 + 0.5 * np.sin(2e3 * X) * np.cos(3e3 * Y) * np.sin(1e3 * Z))
    vol = engine.Volume.from_ne(ne, x, x, x, LWL, "z", phaseshift=True)
    host = {"x": x}
    if case == "all":
        host["kappa"] = -1e6 * (ne / 1e25)
        host["ne"] = ne
        host["B"] = np.empty(ne.shape + (3,))
        host["B"][...] = (0.3, -0.5, 0.7)
        vol.attach_aux(host["kappa"], host["ne"], host["B"], 2.62e-13 * LWL ** 2)
    return vol, host


def numpy_sums(vol, host, case):
    """The same sums on the host, from arrays already in memory: seconds (best of 2)."""
    from synthpy_amd import engine

    dndx, dndy, _, nm1 = vol.fields(phase=True)
    w = engine.trapezoid_weights(np.float64(np.float32(host["x"])))
    K = vol.omega ** 2 * 1e6 / 5.64e4 ** 2
    best = np.inf
    for _ in range(2):
        t = time.perf_counter()
        maps = [np.float64(dndx) @ w, np.float64(dndy) @ w, nm1 @ w, (-nm1 * (2.0 + nm1) * K) @ w]
        if case == "all":
            maps += [host["kappa"] @ w, (host["ne"] * host["B"][..., 2]) @ w]
        best = min(best, time.perf_counter() - t)
    return best, maps


def one_case(case, grid, reps, host_too):
    from synthpy_amd import engine

    engine.init(0)
    vol, host = volume(engine, grid, case)
    for _ in range(2):
        maps = vol.project()
    dts = []
    for _ in range(reps):
        t = time.perf_counter()
        vol.project()
        dts.append(time.perf_counter() - t)
    print(f"CASE {case} grid {grid} bytes {vol.nbytes} whole_call_ms median {np.median(dts) * 1e3:.3f} min {min(dts) * 1e3:.3f} reps {reps}", flush=True)
    if host_too:
        dt, ref = numpy_sums(vol, host, case)
        got = [maps["grad"][0], maps["grad"][1], maps["nm1"], maps["ne"]] + ([maps["kappa"], maps["neB"]] if case == "all" else [])
        worst = max(float(np.max(np.abs(g - r)) / np.max(np.abs(r))) for g, r in zip(got, ref) if np.max(np.abs(r)) > 0)
        print(f"HOST {case} numpy_s {dt:.3f} worst relative difference of a map to NumPy's (float64 sums) {worst:.2e}", flush=True)
    vol.close()


def run(cmd):
    r = subprocess.run(cmd, timeout=900, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"project_rate: {' '.join(cmd)} ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return r.stdout


def child(args, profiled):
    cmd = [sys.executable, os.path.abspath(__file__), "--grid", str(args.grid), "--reps", str(args.reps)]
    return cmd + ["--case", profiled] if profiled else cmd


def run_cases(args, lines):
    for case in ("phase", "all"):
        what = "phase field" if case == "phase" else "phase, kappa and Faraday fields"
        # profiler off: whole-call time and the host's sums
        out = run(child(args, case) + ["--host"])
        info = {ln.split()[0]: ln for ln in out.splitlines() if ln.startswith(("CASE", "HOST"))}
        nbytes = int(info["CASE"].split(" bytes ")[1].split()[0])
        # profiler on, a run of its own: the kernel's time
        with tempfile.TemporaryDirectory() as d:
            run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "s", "--output-format", "csv", "--"] + child(args, case))
            f = (sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)) or [None])[0]
            rows = [r for r in csv.DictReader(open(f))] if f else []
        rows = [r for r in rows if "k_project" in r["Name"]]
        if not rows:
            raise SystemExit("project_rate: rocprofv3 listed no k_project kernel")
        r = rows[0]
        avg, mn = float(r["TotalDurationNs"]) / int(r["Calls"]) * 1e-9, float(r["MinNs"]) * 1e-9
        lines.append(f"{args.grid}^3, {what}: {nbytes / 1e9:.3f} GB of records read once")
        lines.append(f"  kernel {avg * 1e3:.3f} ms average of {r['Calls']} calls (min {mn * 1e3:.3f} ms): {nbytes / avg / 1e12:.2f} TB/s = "
                     f"{nbytes / avg / HBM_ACHIEVABLE:.0%} of the achievable {HBM_ACHIEVABLE / 1e12:.1f} TB/s (at the minimum: {nbytes / mn / HBM_ACHIEVABLE:.0%})")
        lines.append("  " + info["CASE"].split(" bytes ")[1].split(" ", 1)[1] + " (Volume.project(): kernel + download of 6 maps + synchronise; profiler off)")
        lines.append("  " + info["HOST"].split(" ", 2)[2] + " (arrays already in memory)")
        for ln in lines[-4:]:
            print(ln, flush=True)


def traced_against_projection(args, lines):
    import bench
    from synthpy_amd import engine, projection

    engine.init(0)
    ne, x = bench.make_volume(args.grid)
    n_rays = int(args.rays)
    s0 = bench.make_rays(n_rays, EXT, 0)
    vol = engine.Volume.from_ne(ne, x, x, x, LWL, "z", phaseshift=True)
    g = np.float64(np.float32(x))
    P = projection.Projection(vol.project(), vol.omega, vol.verdet, ("x", "y"), (g, g))
    rays = engine.RayBundle(n_rays).upload(s0)
    rays.trace(vol, engine.default_t_end(EXT), EXT, precision="f64")
    sf = rays.download(rf=False, Jf=False)[0]
    want = P.sample(s0[0], s0[1], "phase")
    ok = ~(np.isnan(want) | np.isnan(sf[7]))
    d = sf[7][ok] - want[ok]
    lines.append(f"C3 turbulent volume {args.grid}^3 (bench.make_volume), {n_rays} rays of bench.make_rays traced in float64: traced phase - "
                 f"Projection.sample(x0, y0, 'phase') over {int(ok.sum())} rays inside the grid: max |d| {np.max(np.abs(d)):.4e} rad, "
                 f"RMS {np.sqrt(np.mean(d * d)):.4e} rad; the phase itself: mean {np.mean(want[ok]):.4e} rad, RMS about the mean "
                 f"{np.std(want[ok]):.4e} rad (a physics number: refraction and the beam's divergence move a ray off its launch column)")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rays", type=float, default=2e5)
    ap.add_argument("--case", choices=("phase", "all"))
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "project_rate.txt"))
    a = ap.parse_args()
    if a.case:
        one_case(a.case, a.grid, a.reps, a.host)
        return
    from synthpy_amd import _ffi  # no device opened here: the cases run in processes of their own

    lines = [f"project_rate: sr_volume_project / k_project, z-probing, {_ffi.lib.sr_version().decode()}"]
    run_cases(a, lines)
    traced_against_projection(a, lines)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
