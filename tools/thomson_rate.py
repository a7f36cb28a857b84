"""Rate of the Thomson-scattering kernel (k_thomson; sr_field_thomson) on an N^3 float64 domain.

    python tools/thomson_rate.py [--grid 256] [--volumes 1024] [--points 32] [--wavelengths 1024] [--reps 9] [--host-samples 1048576]
                                 [--out profiles/thomson_rate.txt]

Cases: `volumes` scattering volumes of `points` quadrature points at `wavelengths` wavelengths (a sample is one point at one
wavelength), with the flow V (k_thomson<true, double>) and without it (k_thomson<false, double>), ne / Te / Ti / Z as fields; the
fields stay in HBM across the cases.  Per case: the kernel's time (HIP events around the launch, what *kernel_ms returns) as the
median of `reps` calls after 2 warm-up calls with the smallest and largest, samples per second from the median, and the whole call
from host arrays to host arrays by the host clock (it ends in a stream synchronise).  A sample's arithmetic is counted from the
rule, not measured: 6 exp, 31 divisions (26 in the two Dawson sums), 2 rint, about 300 further float64 products and sums.
The CPU comparison is the same physics through scipy.special.wofz in NumPy on this machine's host, one thread, on `host-samples`
of the same samples (whole rows of wavelengths of the first volumes' points), gathered values given: samples per second.
Nothing here is a target; the table says what was measured."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QE, ME, MP, EPS0, LIGHT = 1.602176634e-19, 9.1093837015e-31, 1.67262192369e-27, 8.8541878128e-12, 299792458.0


def host_wofz(ne, Te, Ti, Z, vs, vi, cth, lam, lam_i, A):
    """S (n_points, n_lambda) through the Faddeeva function, NumPy float64."""
    from scipy.special import wofz

    w_s, w_i = 2 * np.pi * LIGHT / lam[None, :], 2 * np.pi * LIGHT / lam_i
    k_s, k_i = w_s / LIGHT, w_i / LIGHT
    k = np.sqrt(k_s ** 2 + k_i ** 2 - 2 * k_s * k_i * cth)
    w = (w_s - w_i) - (k_s * vs[:, None] - k_i * vi[:, None])
    vte, vti = np.sqrt(2 * QE * Te / ME)[:, None], np.sqrt(2 * QE * Ti / (A * MP))[:, None]
    xe, xi = w / (k * vte), w / (k * vti)
    al2 = (ne * QE / (EPS0 * Te))[:, None] / k ** 2
    W = lambda x: 1 + x * 1j * np.sqrt(np.pi) * wofz(x)
    che, chi = al2 * W(xe), al2 * (Z * Te / Ti)[:, None] * W(xi)
    eps = 1 + che + chi
    return 2 * np.sqrt(np.pi) / k * (np.abs(1 + chi) ** 2 / np.abs(eps) ** 2 * np.exp(-xe ** 2) / vte
                                     + Z[:, None] * np.abs(che) ** 2 / np.abs(eps) ** 2 * np.exp(-xi ** 2) / vti)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--volumes", type=int, default=1024)
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--wavelengths", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-samples", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thomson_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import engine

    engine.init(0)
    n, M, nq, nl = a.grid, a.volumes, a.points, a.wavelengths
    rng = np.random.default_rng(n)
    x = np.float32(np.linspace(-5e-3, 5e-3, n))
    shape = (n, n, n)
    t0 = time.time()
    host = dict(ne=1e24 * (0.5 + rng.random(shape)), Te=50 + 100 * rng.random(shape), Ti=20 + 60 * rng.random(shape),
                Z=2 + 3 * rng.random(shape))
    F = {k: engine.Field(v, x, x, x) for k, v in host.items()}
    F["V"] = engine.Field(1e5 * rng.standard_normal(shape + (3,)), x, x, x)
    print(f"fields up after {time.time() - t0:.1f} s", flush=True)
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
    samples = M * nq * nl
    lines = [f"k_thomson on a {n}^3 float64 domain (ne, Te, Ti, Z fields, V a vector field): {M} volumes x {nq} points x {nl} wavelengths "
             f"= {samples:.3e} samples; 2 warm-up + {a.reps} timed calls, HIP events",
             f"{'case':10} {'kernel ms median':>17} {'min':>9} {'max':>9} {'samples/s':>11} {'whole call ms median':>21}"]
    try:
        for name, V in (("with V", F["V"]), ("without V", None)):
            ms, call = [], []
            for k in range(2 + a.reps):
                t1 = time.perf_counter()
                P, weight = engine.thomson(F["ne"], F["Te"], F["Ti"], F["Z"], V, lam_i, A, pts, wts, ki, ks, lam)
                t2 = time.perf_counter()
                if k >= 2:
                    ms.append(F["ne"].last_kernel_ms)
                    call.append((t2 - t1) * 1e3)
            ms = np.array(ms)
            assert np.all(np.isfinite(P)) and np.all(P > 0) and np.all(weight > 0)
            lines.append(f"{name:10} {np.median(ms):17.3f} {ms.min():9.3f} {ms.max():9.3f} {samples / (np.median(ms) * 1e-3):11.3e} "
                         f"{np.median(call):21.3f}")
            print(lines[-1], flush=True)
    finally:
        for f in F.values():
            f.close()
    # the host comparison: whole volumes, their gathered values from the nearest node (the gather is not what is compared)
    n_vol = max(1, min(M, a.host_samples // (nq * nl)))
    p = pts[:n_vol].reshape(-1, 3)
    idx = tuple(np.clip(np.searchsorted(np.float64(x), p[:, k]), 0, n - 1) for k in range(3))
    g = {k: v[idx] for k, v in host.items()}
    vs, vi = 3e4 * np.ones(len(p)), -3e4 * np.ones(len(p))
    cth = np.repeat(ks[:n_vol] @ ki, nq)[:, None]
    times = []
    for _ in range(3):
        t1 = time.perf_counter()
        S = host_wofz(g["ne"], g["Te"], g["Ti"], g["Z"], vs, vi, cth, lam, lam_i, A)
        times.append(time.perf_counter() - t1)
    assert np.all(np.isfinite(S))
    lines.append(f"host, scipy.special.wofz in NumPy, one thread, {S.size:.3e} of the same samples: best of 3 {min(times) * 1e3:.1f} ms, "
                 f"{S.size / min(times):.3e} samples/s")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
