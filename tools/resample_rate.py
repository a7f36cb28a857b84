"""Rate of the resampling kernel (k_resample, sr_field_resample): an N^3 field turned onto a grid of its own size.

    python tools/resample_rate.py [--grids 256 512] [--reps 5] [--out profiles/resample_rate.txt] [--no-host]

Cases: float32 and float64 scalar fields at every grid, and the 3-component field at the smallest; the identity, 45 degrees
about y and a generic three-angle rotation.  Per case: the kernel's time (HIP events around the launch, what sr_field_resample
returns in *kernel_ms: median and minimum of `reps` calls after 2 warm-up calls), the whole call from host array to host array
(host clock around Field.resample, which ends in a device synchronise and includes the download), and the compulsory bytes --
the source read once and the view written once -- over the kernel's time, beside the 6.3 TB/s a float4 copy reaches on an
MI355X (what profiles/project_rate.txt is set against).  The upload of the source (engine.Field(...)) is timed once per field.
Then the brick sweep: every instantiated brick on the largest grid, the bricks alternating inside each repeat.  Then what the
geometry says about the difference between the orientations: the distinct 128-byte source lines one wavefront's corner load
touches, counted on the host for a sample of wavefronts.  Last, the NumPy restatement of the rule (tests/test_resample.py's,
here in slabs of view planes so that it fits in memory) and, where SciPy is installed, RegularGridInterpolator, on this
machine's CPU."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # B/s
EXT = 5e-3
BRICKS = ("4x4x16", "8x8x4", "8x4x8", "2x8x16", "16x1x16", "1x1x256")


def rotations():
    from synthpy_amd import orientation as o

    return {"identity": np.eye(3), "45 deg about y": o.rotation_matrix(45.0, "y"),
            "generic": o.compose(o.rotation_matrix(31.0, "z"), o.rotation_matrix(17.0, "y"), o.rotation_matrix(-23.0, "x"))}


def source(n, dtype, n_comp):
    rng = np.random.default_rng(n + n_comp)
    return rng.random((n, n, n) + ((3,) if n_comp == 3 else ()), dtype=np.float32).astype(dtype, copy=False)


def timed(field, R, axes, reps, V=None):
    for _ in range(2):
        field.resample(R, (0, 0, 0), axes, V=V)
    ker, whole = [], []
    for _ in range(reps):
        t = time.perf_counter()
        field.resample(R, (0, 0, 0), axes, V=V)
        whole.append(time.perf_counter() - t)
        ker.append(field.last_kernel_ms)
    return np.array(ker), np.array(whole) * 1e3


def restate_slabs(src, g, R, slab=8):
    """The header's rule in NumPy float64 (scalar field, view grid = source grid, t = 0, fill 0), slab by slab."""
    n = len(g)
    out = np.empty((n, n, n), src.dtype)
    for lo in range(0, n, slab):
        q0, q1, q2 = np.meshgrid(g[lo:lo + slab], g, g, indexing="ij")
        p = [(R[a, 0] * q0 + R[a, 1] * q1) + R[a, 2] * q2 for a in range(3)]
        inside = np.ones(q0.shape, bool)
        cell, w = [], []
        for a in range(3):
            ok = (p[a] >= g[0]) & (p[a] <= g[-1])
            ps = np.where(ok, p[a], g[0])
            i = np.clip(np.searchsorted(g, ps, side="right") - 1, 0, n - 2)
            cell.append(i)
            w.append((ps - g[i]) / (g[i + 1] - g[i]))
            inside &= ok
        (i, j, k), (wx, wy, wz) = cell, w
        ux, uy, uz = 1.0 - wx, 1.0 - wy, 1.0 - wz
        w00, w01, w10, w11 = uy * uz, uy * wz, wy * uz, wy * wz
        s0 = ((src[i, j, k] * w00 + src[i, j, k + 1] * w01) + src[i, j + 1, k] * w10) + src[i, j + 1, k + 1] * w11
        s1 = ((src[i + 1, j, k] * w00 + src[i + 1, j, k + 1] * w01) + src[i + 1, j + 1, k] * w10) + src[i + 1, j + 1, k + 1] * w11
        out[lo:lo + slab] = np.where(inside, ux * s0 + wx * s1, 0.0)
    return out


def lines_per_wavefront(n, itemsize, R, brick, samples=200):
    """Distinct 128-byte source lines the 64 lanes of one wavefront touch with ONE of their eight corner loads (the low corner),
    mean over sampled wavefronts wholly inside the source: what one load instruction costs the CU's vector-memory pipe."""
    bx, by, bz = (int(v) for v in brick.split("x"))
    g = np.float64(np.float32(np.linspace(-EXT, EXT, n)))
    rng = np.random.default_rng(1)
    t = np.arange(256)
    lz, ly, lx = t % bz, (t // bz) % by, t // (bz * by)
    counts = []
    while len(counts) < samples:
        b = rng.integers(0, [n // bx, n // by, n // bz])
        wave = rng.integers(0, 4)
        sel = slice(64 * wave, 64 * wave + 64)
        q = np.stack([g[b[0] * bx + lx[sel]], g[b[1] * by + ly[sel]], g[b[2] * bz + lz[sel]]])
        p = R @ q
        if np.any(p < g[0]) or np.any(p > g[-1]):
            continue
        c = np.clip(np.searchsorted(g, p.ravel(), side="right").reshape(p.shape) - 1, 0, n - 2)
        byte = ((c[0].astype(np.int64) * n + c[1]) * n + c[2]) * itemsize
        counts.append(len(np.unique(byte // 128)))
    return float(np.mean(counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy / SciPy timings")
    ap.add_argument("--out", default=os.path.join("profiles", "resample_rate.txt"))
    a = ap.parse_args()
    from synthpy_amd import _ffi, engine

    engine.init(0)
    rots = rotations()
    default_brick = os.environ.get("SYNTHRAY_RESAMPLE_BRICK", BRICKS[0])
    lines = [f"resample_rate: sr_field_resample / k_resample, view grid = source grid, {_ffi.lib.sr_version().decode()}",
             f"kernel: HIP events, median (min) of {a.reps} calls after 2 warm-up calls; whole call: host array to host array, same calls; "
             f"bytes = source once + view once; achievable HBM rate {HBM_ACHIEVABLE / 1e12:.1f} TB/s (as profiles/project_rate.txt); brick {default_brick}"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    kernel_ms = {}
    cases = [(n, dt, 1) for n in a.grids for dt in (np.float32, np.float64)] + [(min(a.grids), dt, 3) for dt in (np.float32, np.float64)]
    for n, dt, nc in cases:
        x = np.linspace(-EXT, EXT, n)
        src = source(n, dt, nc)
        t = time.perf_counter()
        f = engine.Field(src, x, x, x)
        up = time.perf_counter() - t
        nbytes = 2 * src.nbytes
        emit(f"{n}^3 {np.dtype(dt).name}{' x 3 components' if nc == 3 else ''}: source {src.nbytes / 1e9:.3f} GB, upload (Field(...)) {up * 1e3:.1f} ms = {src.nbytes / up / 1e9:.1f} GB/s")
        for name, R in rots.items():
            ker, whole = timed(f, R, (x, x, x), a.reps, V=R.T if nc == 3 else None)
            kernel_ms[(n, np.dtype(dt).name, nc, name)] = float(np.median(ker))
            emit(f"  {name:15s} kernel {np.median(ker):8.3f} ms (min {ker.min():.3f}): {nbytes / np.median(ker) / 1e9:7.2f} TB/s = "
                 f"{nbytes / (np.median(ker) * 1e-3) / HBM_ACHIEVABLE:5.1%} of achievable; whole call {np.median(whole):8.1f} ms (min {whole.min():.1f}) = "
                 f"{src.nbytes / np.median(whole) / 1e6:.1f} GB/s of view downloaded: the PCIe copy is {1 - np.median(ker) / np.median(whole):.1%} of it")
        f.close()
        del src

    # the brick sweep on the largest grid: bricks alternate inside every repeat
    n = max(a.grids)
    x = np.linspace(-EXT, EXT, n)
    for dt in (np.float32, np.float64):
        f = engine.Field(source(n, dt, 1), x, x, x)
        emit(f"brick sweep, {n}^3 {np.dtype(dt).name}: kernel ms, median of {a.reps} (bricks alternating inside each repeat)")
        for name, R in rots.items():
            t = {b: [] for b in BRICKS}
            for rep in range(a.reps + 1):
                for b in BRICKS:
                    os.environ["SYNTHRAY_RESAMPLE_BRICK"] = b
                    f.resample(R, (0, 0, 0), (x, x, x))
                    if rep:
                        t[b].append(f.last_kernel_ms)
            emit(f"  {name:15s} " + "  ".join(f"{b} {np.median(t[b]):.3f}" for b in BRICKS))
        os.environ["SYNTHRAY_RESAMPLE_BRICK"] = default_brick
        f.close()

    # where the orientations differ
    emit(f"distinct 128-byte source lines per wavefront and corner load (host count over 200 wavefronts, {n}^3; a load instruction "
         "occupies the CU's vector-memory pipe once per line):")
    for dt in (np.float32, np.float64):
        for b in BRICKS:
            emit(f"  {np.dtype(dt).name} brick {b:8s} " + "  ".join(f"{name} {lines_per_wavefront(n, np.dtype(dt).itemsize, R, b):.1f}" for name, R in rots.items()))
    for (m, dname, nc, name), ms in sorted(kernel_ms.items()):
        if name == "generic" and nc == 1:
            ident = kernel_ms[(m, dname, nc, "identity")]
            emit(f"  {m}^3 {dname}: generic / identity kernel time = {ms / ident:.2f}" + (
                " -- more than twice: the bytes from HBM are the same (every source line is still needed once), the difference sits in the "
                "vector-memory pipe and the L1/L2 line traffic, which grow with the lines per load above" if ms > 2 * ident else ""))

    if not a.no_host:
        R = rots["generic"]
        for n in a.grids:
            g = np.float64(np.float32(np.linspace(-EXT, EXT, n)))
            src = np.float64(source(n, np.float32, 1))
            t = time.perf_counter()
            ref = restate_slabs(src, g, R)
            dt_np = time.perf_counter() - t
            f = engine.Field(src, g, g, g)
            got = f.resample(R, (0, 0, 0), (g, g, g))
            f.close()
            emit(f"host, {n}^3 float64 generic: NumPy restatement {dt_np:.2f} s on one core (kernel {kernel_ms[(n, 'float64', 1, 'generic')]:.3f} ms); "
                 f"GPU result bit-equal to it: {np.array_equal(got, ref)}, max |d| {float(np.max(np.abs(got - ref))):.3e}")
            try:
                from scipy.interpolate import RegularGridInterpolator
            except ImportError:
                emit("  SciPy is not installed: RegularGridInterpolator not timed")
                continue
            if n > 256:
                emit(f"  RegularGridInterpolator not timed at {n}^3 (its (N, 3) point array alone is {n ** 3 * 24 / 1e9:.1f} GB)")
                continue
            t = time.perf_counter()
            q = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) @ R.T
            sp = RegularGridInterpolator((g, g, g), src, bounds_error=False, fill_value=0.0)(q).reshape(n, n, n)
            dt_sp = time.perf_counter() - t
            emit(f"  scipy RegularGridInterpolator {dt_sp:.2f} s; max |d| to the GPU result {float(np.max(np.abs(sp - got))):.3e}")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
