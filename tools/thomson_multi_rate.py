"""Rate of the multi-species Thomson kernel (k_thomson_multi; sr_field_thomson_multi) beside k_thomson's, on tools/thomson_rate.py's
workload: an N^3 float64 domain, `volumes` scattering volumes of `points` quadrature points at `wavelengths` wavelengths.

    python tools/thomson_multi_rate.py [--grid 256] [--volumes 1024] [--points 32] [--wavelengths 1024] [--reps 9]
                                       [--resources FILE] [--out profiles/thomson_multi_rate.txt]

Cases, all with ne / Te / Ti fields and the flow V: k_thomson (Z a field); k_thomson_multi with 1 species (the same Z field,
f = 1: the same bits), with 2 and with 4 species (the first charge the Z field, the other charges and all fractions uniform), and
with 2 species and the drift Vd.  Per case: the kernel's time (HIP events around the launch) as the median of `reps` calls after 2
warm-up calls, with the smallest and largest, samples per second from the median, and the ratio to k_thomson's median beside the
ratio the count of plasma-dispersion evaluations predicts, (1 + NS)/2.  The kernels' registers, LDS and scratch are the
compiler's (tools/kernel_resources.py, run here, or the text of --resources when it was run elsewhere).  Nothing here is a target;
the table says what was measured."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--volumes", type=int, default=1024)
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--wavelengths", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thomson_multi_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import engine

    engine.init(0)
    n, M, nq, nl = a.grid, a.volumes, a.points, a.wavelengths
    rng = np.random.default_rng(n)  # thomson_rate.py's fields, volumes and wavelengths
    x = np.float32(np.linspace(-5e-3, 5e-3, n))
    shape = (n, n, n)
    host = dict(ne=1e24 * (0.5 + rng.random(shape)), Te=50 + 100 * rng.random(shape), Ti=20 + 60 * rng.random(shape),
                Z=2 + 3 * rng.random(shape))
    F = {k: engine.Field(v, x, x, x) for k, v in host.items()}
    del host
    F["V"] = engine.Field(1e5 * rng.standard_normal(shape + (3,)), x, x, x)
    lam_i, A = 532e-9, 12.0
    centres = -4e-3 + 8e-3 * rng.random((M, 3))
    t, w = np.polynomial.legendre.leggauss(nq)
    ki = np.array([0.0, 0.0, 1.0])
    pts = np.ascontiguousarray(centres[:, None, :] + (1e-4 * t)[None, :, None] * ki[None, None, :])
    wts = np.ascontiguousarray(np.broadcast_to(1e-4 * w, (M, nq)))
    d = rng.standard_normal((M, 3))
    d[:, 2] *= 0.3
    ks = d / np.sqrt(np.sum(d * d, axis=1, keepdims=True))
    lam = np.linspace(lam_i - 3e-9, lam_i + 3e-9, nl)
    F["Vd"] = engine.Field(3e5 * rng.standard_normal(shape + (3,)), x, x, x)
    print("fields up", flush=True)
    samples = M * nq * nl
    species = {1: [(A, F["Z"], 1.0)], 2: [(A, F["Z"], 0.5), (1.0, 1.0, 0.5)],
               4: [(A, F["Z"], 0.4), (1.0, 1.0, 0.3), (27.0, 11.0, 0.2), (16.0, 6.0, 0.1)]}
    multi = lambda ns, Vd=None: (lambda: engine.thomson_multi(F["ne"], F["Te"], F["Ti"], F["V"], Vd, species[ns], lam_i, pts, wts, ki, ks, lam))
    cases = [("k_thomson", 1, lambda: engine.thomson(F["ne"], F["Te"], F["Ti"], F["Z"], F["V"], lam_i, A, pts, wts, ki, ks, lam)),
             ("k_thomson_multi, 1 species", 1, multi(1)), ("k_thomson_multi, 2 species", 2, multi(2)),
             ("k_thomson_multi, 4 species", 4, multi(4)), ("k_thomson_multi, 2 species + Vd", 2, multi(2, F["Vd"]))]
    lines = [f"k_thomson and k_thomson_multi on a {n}^3 float64 domain (ne, Te, Ti, Z fields, V and Vd vector fields): {M} volumes x {nq} "
             f"points x {nl} wavelengths = {samples:.3e} samples; 2 warm-up + {a.reps} timed calls, HIP events",
             f"{'case':32} {'kernel ms median':>17} {'min':>9} {'max':>9} {'samples/s':>11} {'x k_thomson':>12} {'(1 + NS)/2':>11}"]
    base, first = None, None
    try:
        for name, ns, call in cases:
            ms = []
            for k in range(2 + a.reps):
                P, weight = call()
                if k >= 2:
                    ms.append(F["ne"].last_kernel_ms)
            ms = np.array(ms)
            assert np.all(np.isfinite(P)) and np.all(P > 0) and np.all(weight > 0)
            if base is None:
                base, first = float(np.median(ms)), P
            elif name.endswith("1 species"):
                assert P.tobytes() == first.tobytes(), "one species through k_thomson_multi differs from k_thomson"
            lines.append(f"{name:32} {np.median(ms):17.3f} {ms.min():9.3f} {ms.max():9.3f} {samples / (np.median(ms) * 1e-3):11.3e} "
                         f"{np.median(ms) / base:12.2f} {(1 + ns) / 2:11.1f}")
            print(lines[-1], flush=True)
    finally:
        for f in F.values():
            f.close()
    lines.append("one species through k_thomson_multi returned k_thomson's bits")
    if a.resources:
        res = open(a.resources).read()
    else:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "thomson.hip", "thomson_multi.hip"],
                             check=True, capture_output=True, text=True).stdout
    text = "\n".join(lines) + "\n" + res
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
