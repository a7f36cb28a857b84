"""Rate of the tabulated self-emission kernels (k_emission_z / k_emission_xy with the table node; sr_field_emission_table) on
N^3 float64 fields, beside sr_field_emission on the same fields in the same run.

    python tools/table_emission_rate.py [--grid 512] [--reps 7] [--out profiles/table_emission_rate.txt]

Cases: axis z and axis x; 1 band and 4 bands; a 10x10 table (1.8 KB for one band: staged into LDS by every workgroup) and a
64x64 table with emission opacities (66 KB for one band, 263 KB for four: beyond the 64 KiB LDS budget, read from global memory
through L2); Te and Z as fields.  Per case: the kernel's time (HIP events around the launch, what the entry returns in
*kernel_ms: median and minimum of `reps` calls after 2 warm-up calls), the bytes of the three fields over that time, the ratio to
the yardsticks -- sr_field_emission (the NRL node) with the same number of bands on the same fields, and tools/emission_rate.py's
device-to-device hipMemcpyAsync over one field's size (read + write traffic) -- and node-bands per second.  Nothing is asserted
on the rates."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIGHT = 299792458.0
WAVELENGTHS = (1064e-9, 532e-9, 266e-9, 100e-9)
PHOTON_EV = (12.4, 30.0, 90.0, 250.0)


def table(n_t, n_d, n_band, lte, seed):
    from synthpy_amd.utils.eos_opacity import OpacityTable

    rng = np.random.default_rng(seed)
    la = rng.uniform(np.log(1e-1), np.log(1e3), (n_band, n_t, n_d))
    le = la + rng.uniform(-1.0, 1.0, la.shape)
    return OpacityTable(np.geomspace(1.0, 500.0, n_t), np.geomspace(1e17, 1e21, n_d), np.exp(la), PHOTON_EV[:n_band], 12.011,
                        emission=None if lte else np.exp(le))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_emission_rate.txt"))
    a = ap.parse_args()
    from emission_rate import copy_rate
    from synthpy_amd import engine

    engine.init(0)
    n = a.grid
    rng = np.random.default_rng(n)
    x = np.float32(np.linspace(-5e-3, 5e-3, n))
    shape = (n, n, n)
    Z = 1.0 + 29.0 * rng.random(shape)
    ne = 10.0 ** (17.0 + 4.0 * rng.random(shape)) * Z * 1e6  # ni over the table's four decades
    Te = 1.0 + 499.0 * rng.random(shape)
    fields = [engine.Field(f, x, x, x) for f in (ne, Te, Z)]
    field_bytes = ne.nbytes
    del ne, Te, Z
    lines = [f"tabulated self-emission kernels on {n}^3 float64 fields ({field_bytes / 2 ** 30:.2f} GiB each), Te and Z as fields; "
             f"2 warm-up + {a.reps} timed calls, HIP events"]
    med, best = copy_rate(field_bytes, a.reps)
    lines.append(f"yardstick: hipMemcpyAsync device to device over {field_bytes / 2 ** 30:.2f} GiB, read + write traffic: "
                 f"median {med / 1e12:.3f} TB/s, best {best / 1e12:.3f} TB/s")
    lines.append(f"{'axis':4} {'bands':5} {'node':26} {'table KB':>9} {'kernel ms median':>17} {'min':>8} {'read TB/s':>10} {'of copy':>8} "
                 f"{'of NRL':>7} {'node-bands/s':>13}")

    def timed(call):
        ms = []
        for k in range(2 + a.reps):
            I, tau = call()
            if k >= 2:
                ms.append(fields[0].last_kernel_ms)
        assert np.all(np.isfinite(I)) and np.all(tau > 0)
        return np.array(ms)

    try:
        for axis in (2, 0):
            for nb in (1, 4):
                om = 2 * np.pi * LIGHT / np.float64(WAVELENGTHS[:nb])
                nrl = timed(lambda: engine.emission(*fields, om, axis))
                cases = [("NRL (sr_field_emission)", 0.0, nrl)]
                for name, t in (("table 10x10 LTE, LDS", table(10, 10, nb, True, 1)), ("table 10x10, LDS", table(10, 10, nb, False, 2)),
                                ("table 64x64, global", table(64, 64, nb, False, 3))):
                    kb = 8 * (t.absorption.size * (1 if t.emission is None else 2) + len(t.temperatures) + len(t.densities)) / 1e3
                    cases.append((name, kb, timed(lambda: engine.emission_table(*fields, t, axis))))
                for name, kb, ms in cases:
                    rate = 3 * field_bytes / (np.median(ms) * 1e-3)
                    lines.append(f"{'xyz'[axis]:4} {nb:5d} {name:26} {kb:9.1f} {np.median(ms):17.3f} {ms.min():8.3f} {rate / 1e12:10.3f} "
                                 f"{rate / med:8.3f} {np.median(nrl) / np.median(ms):7.3f} {n ** 3 * nb / (np.median(ms) * 1e-3):13.3e}")
                    print(lines[-1], flush=True)
    finally:
        for f in fields:
            f.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
