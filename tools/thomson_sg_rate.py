"""Rate of the super-Gaussian Thomson kernel (k_thomson_sg; sr_field_thomson_sg) beside k_thomson_multi's in the same run, on
tools/thomson_multi_rate.py's workload: an N^3 float64 domain, `volumes` scattering volumes of `points` quadrature points at
`wavelengths` wavelengths.

    python tools/thomson_sg_rate.py [--grid 256] [--volumes 1024] [--points 32] [--wavelengths 1024] [--reps 9]
                                    [--resources FILE] [--out profiles/thomson_sg_rate.txt]

Cases, all with ne / Te / Ti fields and the flow V: k_thomson_multi with 2 species, without and with the drift Vd (the yardstick);
k_thomson_sg with the uniform order 2 on the same two (the same arithmetic, and the same bits: asserted), with the uniform order 3.5
and 1, 2 and 4 species, with 2 species and the drift, with an order field spanning 2..5, and with the order 3.5 over +-60 nm, the
electron feature, where |xs| passes T and the incomplete gamma function runs its continued fraction (the other cases span +-3 nm,
the ion feature).  Per case: the kernel's time (HIP events around the launch) as the median of `reps` calls after 2 warm-up calls,
with the smallest and largest, samples per second and quadrature-node terms per second (48 per super-Gaussian sample) from the
median, and the ratio to k_thomson_multi's median of the same species and drift.  The kernels' registers, LDS and scratch are the
compiler's (tools/kernel_resources.py, run here, or the text of --resources when it was run elsewhere).  Nothing here is a target;
the table says what was measured."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NODES = 48  # kNN of thomson_sg.hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--volumes", type=int, default=1024)
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--wavelengths", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thomson_sg_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import engine

    engine.init(0)
    n, M, nq, nl = a.grid, a.volumes, a.points, a.wavelengths
    rng = np.random.default_rng(n)  # thomson_multi_rate.py's fields, volumes and wavelengths
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
    lam_wide = np.linspace(lam_i - 60e-9, lam_i + 60e-9, nl)
    F["Vd"] = engine.Field(3e5 * rng.standard_normal(shape + (3,)), x, x, x)
    F["order"] = engine.Field(2.0 + 3.0 * rng.random(shape), x, x, x)
    print("fields up", flush=True)
    samples = M * nq * nl
    species = {1: [(A, F["Z"], 1.0)], 2: [(A, F["Z"], 0.5), (1.0, 1.0, 0.5)],
               4: [(A, F["Z"], 0.4), (1.0, 1.0, 0.3), (27.0, 11.0, 0.2), (16.0, 6.0, 0.1)]}
    multi = lambda ns, Vd=None: (lambda: engine.thomson_multi(F["ne"], F["Te"], F["Ti"], F["V"], Vd, species[ns], lam_i, pts, wts, ki, ks, lam))
    sg = lambda ns, order, Vd=None, lam=lam: (lambda: engine.thomson_sg(F["ne"], F["Te"], F["Ti"], F["V"], Vd, species[ns], order, lam_i,
                                                                        pts, wts, ki, ks, lam))
    # name, the yardstick's name (None: this is one), super-Gaussian samples?, the call
    cases = [("k_thomson_multi, 2 species", None, False, multi(2)),
             ("k_thomson_multi, 2 species + Vd", None, False, multi(2, F["Vd"])),
             ("k_thomson_sg m = 2, 2 species", "k_thomson_multi, 2 species", False, sg(2, 2.0)),
             ("k_thomson_sg m = 2, 2 species + Vd", "k_thomson_multi, 2 species + Vd", False, sg(2, 2.0, F["Vd"])),
             ("k_thomson_sg m = 3.5, 1 species", "k_thomson_multi, 2 species", True, sg(1, 3.5)),
             ("k_thomson_sg m = 3.5, 2 species", "k_thomson_multi, 2 species", True, sg(2, 3.5)),
             ("k_thomson_sg m = 3.5, 4 species", "k_thomson_multi, 2 species", True, sg(4, 3.5)),
             ("k_thomson_sg m = 3.5, 2 species + Vd", "k_thomson_multi, 2 species + Vd", True, sg(2, 3.5, F["Vd"])),
             ("k_thomson_sg m field 2..5, 2 species", "k_thomson_multi, 2 species", True, sg(2, F["order"])),
             ("k_thomson_sg m = 3.5, 2 sp., +-60 nm", "k_thomson_multi, 2 species", True, sg(2, 3.5, None, lam_wide))]
    lines = [f"k_thomson_multi and k_thomson_sg on a {n}^3 float64 domain (ne, Te, Ti, Z, order fields, V and Vd vector fields): {M} volumes x "
             f"{nq} points x {nl} wavelengths = {samples:.3e} samples; 2 warm-up + {a.reps} timed calls, HIP events",
             f"{'case':38} {'kernel ms median':>17} {'min':>9} {'max':>9} {'samples/s':>11} {'node terms/s':>13} {'x k_thomson_multi':>18}"]
    med, kept = {}, {}
    try:
        for name, yard, is_sg, call in cases:
            ms = []
            for k in range(2 + a.reps):
                P, weight = call()
                if k >= 2:
                    ms.append(F["ne"].last_kernel_ms)
            ms = np.array(ms)
            assert np.all(np.isfinite(P)) and np.all(P >= 0) and np.all(weight > 0)
            med[name], kept[name] = float(np.median(ms)), P
            if yard and not is_sg:
                assert P.tobytes() == kept[yard].tobytes(), "the order 2 through k_thomson_sg differs from k_thomson_multi"
            rate = samples / (med[name] * 1e-3)
            lines.append(f"{name:38} {med[name]:17.3f} {ms.min():9.3f} {ms.max():9.3f} {rate:11.3e} "
                         f"{(f'{NODES * rate:13.3e}' if is_sg else '-'):>13} {(f'{med[name] / med[yard]:18.2f}' if yard else '-'):>18}")
            print(lines[-1], flush=True)
    finally:
        for f in F.values():
            f.close()
    lines.append("the uniform order 2 through k_thomson_sg returned k_thomson_multi's bits, without and with the drift")
    if a.resources:
        res = open(a.resources).read()
    else:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "thomson_multi.hip", "thomson_sg.hip"],
                             check=True, capture_output=True, text=True).stdout
    text = "\n".join(lines) + "\n" + res
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
