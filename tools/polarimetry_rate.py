"""The 3-channel intensity deposit (k_deposit_intensity) beside the complex deposit (k_deposit<SR_IMG_COMPLEX, .>) on the same
resident rays: the C3-shaped bundle (1e7 rays x 512^3, phase integral), two-lens chain, full detector (bin_scale=1).

    python tools/polarimetry_rate.py [grid] [rays] [repeats] [--out FILE]      (defaults 512 1e7 12 profiles/r07_polarimetry.txt)

Times are sr_deposit_stats.kernel_ms (HIP events around the deposit's launches); two untimed warm-up deposits per case, then
`repeats` timed ones into a zeroed image, the cases alternating inside every repeat; median, minimum and maximum are reported.  The complex deposit skips zero contributions,
and E_x of an unrotated ray is exactly -0, so it issues 2 float64 atomics per ray on the bundle as C3 launches it (pol = 0) and
4 on the same rays launched with pol = 0.1; the intensity deposit issues 3 either way.  Both are measured."""
import os, sys, statistics
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from synthpy_amd import engine

argv = list(sys.argv[1:])
out_path = os.path.join("profiles", "r07_polarimetry.txt")
if "--out" in argv:
    k = argv.index("--out")
    out_path = argv[k + 1]
    del argv[k:k + 2]
grid = int(argv[0]) if len(argv) > 0 else 512
N = int(float(argv[1])) if len(argv) > 1 else 10 ** 7
reps = int(argv[2]) if len(argv) > 2 else 12

engine.init(0)
lwl, ext = 1064e-9, 5e-3
ne, x = bench.make_volume(grid)
vol = engine.Volume.from_ne(ne, x, x, x, lwl, "z", phaseshift=True)
s0 = bench.make_rays(N, ext, 0)
rays = engine.RayBundle(N)
ops, an, kwave = engine.chain_shadow_two(), (np.pi / 4, -np.pi / 4, None), 2 * np.pi / lwl
lines = [f"polarimetry_rate: {N} rays x {grid}^3 (phase integral, float64), two-lens chain, detector 3448 x 2574 (bin_scale=1); "
         f"{engine._ffi.lib.sr_version().decode()}; kernel_ms of {reps} deposits after 2 warm-ups: median [min .. max]"]


def timed(cases):
    """cases: [(label, image, deposit)].  The cases ALTERNATE inside every repeat, so that a drift of the shared host or of the
    clocks falls on all of them alike."""
    ms, hits = {c[0]: [] for c in cases}, {}
    for it in range(reps + 2):
        for label, image, deposit in cases:
            image.zero()
            t, hits[label] = deposit()
            if it >= 2:
                ms[label].append(t)
    med = {}
    for label, _, _ in cases:
        m = med[label] = statistics.median(ms[label])
        lines.append(f"  {label:<46s} {m:8.3f} ms [{min(ms[label]):.3f} .. {max(ms[label]):.3f}]   {hits[label] / m / 1e6:7.2f} G rays/s   "
                     f"{hits[label]} rays on the detector")
        print(lines[-1], flush=True)
    return med


for pol in (0.0, 0.1):
    s0[8] = pol
    rays.upload(s0)
    st = rays.trace(vol, engine.default_t_end(ext), ext, precision="f64")
    lines.append(f"launch pol = {pol}: trace kernel {st.trace_kernel_ms:.2f} ms, tile segments {rays.tile_segments}")
    print(lines[-1], flush=True)
    img_c, img_i, img_1 = engine.DetectorImage.complex_field(), engine.DetectorImage.intensity(3), engine.DetectorImage.intensity(1)
    cplx = dict(kwave=kwave, ref_beam=(10, 20))
    med = timed([("complex deposit, LDS tiles", img_c, lambda: rays.deposit(img_c, ops, **cplx)),
                 ("intensity deposit, 3 channels, LDS tiles", img_i, lambda: rays.deposit_intensity(img_i, ops, an)),
                 ("complex deposit, global atomics only", img_c, lambda: rays.deposit(img_c, ops, lds_tiles=False, **cplx)),
                 ("intensity deposit, 3 channels, global atomics", img_i, lambda: rays.deposit_intensity(img_i, ops, an, lds_tiles=False)),
                 ("intensity deposit, 1 channel, LDS tiles", img_1, lambda: rays.deposit_intensity(img_1, ops, (None,)))])
    t_c, t_i = med["complex deposit, LDS tiles"], med["intensity deposit, 3 channels, LDS tiles"]
    lines.append(f"  intensity / complex (tiles): {t_i / t_c:.3f}; the tile's worth: complex {med['complex deposit, global atomics only'] / t_c:.2f}x, "
                 f"intensity {med['intensity deposit, 3 channels, global atomics'] / t_i:.2f}x")
    print(lines[-1], flush=True)
    for img in (img_c, img_i, img_1):
        img.close()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
