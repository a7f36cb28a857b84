"""Rate of the self-emission kernels (k_emission_z, k_emission_xy; sr_field_emission) on N^3 float64 fields.

    python tools/emission_rate.py [--grid 512] [--reps 7] [--out profiles/emission_rate.txt]

Cases: axis z (one wavefront per column, cells composed by a shuffle tree) and axis x (one lane per column), 1 band (1064 nm) and
4 bands (1064, 532, 266, 100 nm), Te and Z as fields and as uniform values.  Per case: the kernel's time (HIP events around the
launch, what sr_field_emission returns in *kernel_ms: median and minimum of `reps` calls after 2 warm-up calls), the bytes of
the fields the kernel reads -- each once -- over that time, and the ratio to the yardstick.  The yardstick is measured in the same
run: hipMemcpyAsync device to device over a buffer the size of one field, timed by HIP events (2 warm-up copies, `reps` timed);
a copy reads and writes every byte, so its HBM traffic is twice the buffer over its time, and that traffic rate is what the
kernel's read rate is set against.  Node-bands per second (nodes x bands over the kernel's time) says what the arithmetic
sustains: several float64 exp / expm1 / log calls per node and band."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIGHT = 299792458.0
WAVELENGTHS = (1064e-9, 532e-9, 266e-9, 100e-9)


def copy_rate(nbytes, reps):
    """(median, best) HBM traffic rate [B/s] of a device-to-device hipMemcpyAsync over nbytes: 2 * nbytes / time."""
    hip = C.CDLL("libamdhip64.so")

    def ok(rc, what):
        if rc:
            raise RuntimeError(f"{what} failed: hipError {rc}")

    src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)), "hipMalloc")
    ok(hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)), "hipMalloc")
    try:
        ok(hip.hipMemset(src, 1, C.c_size_t(nbytes)), "hipMemset")
        ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
        ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
        times = []
        for k in range(2 + reps):
            ok(hip.hipEventRecord(e0, None), "hipEventRecord")
            ok(hip.hipMemcpyAsync(dst, src, C.c_size_t(nbytes), 3, None), "hipMemcpyAsync")  # 3: hipMemcpyDeviceToDevice
            ok(hip.hipEventRecord(e1, None), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = C.c_float(0)
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
            if k >= 2:
                times.append(ms.value * 1e-3)
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
    finally:
        hip.hipFree(src)
        hip.hipFree(dst)
    t = np.array(times)
    return 2 * nbytes / float(np.median(t)), 2 * nbytes / float(t.min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emission_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import engine

    engine.init(0)
    n = a.grid
    rng = np.random.default_rng(n)
    x = np.float32(np.linspace(-5e-3, 5e-3, n))
    shape = (n, n, n)
    ne = 1e25 * 10.0 ** (-2 * rng.random(shape))
    Te = 1.0 + 499.0 * rng.random(shape)
    Z = 1.0 + 29.0 * rng.random(shape)
    fields = [engine.Field(f, x, x, x) for f in (ne, Te, Z)]
    del Te, Z
    field_bytes = ne.nbytes
    lines = [f"self-emission kernels on {n}^3 float64 fields ({field_bytes / 2 ** 30:.2f} GiB each); 2 warm-up + {a.reps} timed calls, HIP events"]
    med, best = copy_rate(field_bytes, a.reps)
    lines.append(f"yardstick: hipMemcpyAsync device to device over {field_bytes / 2 ** 30:.2f} GiB, read + write traffic: "
                 f"median {med / 1e12:.3f} TB/s, best {best / 1e12:.3f} TB/s")
    lines.append(f"{'axis':4} {'bands':5} {'Te, Z':8} {'kernel ms median':>17} {'min':>8} {'fields read GB':>15} {'read TB/s':>10} "
                 f"{'of copy':>8} {'node-bands/s':>13}")
    try:
        for axis in (2, 0):
            for nb in (1, 4):
                om = 2 * np.pi * LIGHT / np.float64(WAVELENGTHS[:nb])
                for uniform in (False, True):
                    Te_arg, Z_arg = (100.0, 5.0) if uniform else fields[1:]
                    ms = []
                    for k in range(2 + a.reps):
                        I, tau = engine.emission(fields[0], Te_arg, Z_arg, om, axis)
                        if k >= 2:
                            ms.append(fields[0].last_kernel_ms)
                    assert np.all(np.isfinite(I)) and np.all(tau > 0)
                    ms = np.array(ms)
                    read = field_bytes * (1 if uniform else 3)
                    rate = read / (np.median(ms) * 1e-3)
                    lines.append(f"{'xyz'[axis]:4} {nb:5d} {'uniform' if uniform else 'fields':8} {np.median(ms):17.3f} {ms.min():8.3f} "
                                 f"{read / 1e9:15.3f} {rate / 1e12:10.3f} {rate / med:8.3f} {n ** 3 * nb / (np.median(ms) * 1e-3):13.3e}")
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
