"""Repeated create / trace / deposit / destroy cycles, and one call of every host-array entry point that owns its device buffers
for the length of the call (volume from fields and back, power spectrum, FFT field, mode sum, Fresnel gridding and
propagation, host-array histogram and intensity image, sightlines and sightline spectra): device memory in use must not grow."""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthpy_amd import engine as eng
from synthpy_amd.field_generator.gaussian2D import gaussian2D
from synthpy_amd.field_generator.gaussian3D import gaussian3D
from synthpy_amd.simulator import fresnel_integral as fi
from synthpy_amd.solvers_legacy.full_solver import init_beam
from synthpy_amd.utils import power_spectrum as ps

eng.init(0)
hip = C.CDLL("libamdhip64.so")
def used():
    free, total = C.c_size_t(), C.c_size_t()
    hip.hipMemGetInfo(C.byref(free), C.byref(total))
    return (total.value - free.value) / 2 ** 20
x = np.linspace(-5e-3, 5e-3, 64)
X, Y, Z = np.meshgrid(x, x, x, indexing="ij", sparse=True)
ne = 1e25 * np.exp(-(X ** 2 + Y ** 2 + Z ** 2) / (1.5e-3) ** 2)
np.random.seed(0)
s0 = init_beam(100000, 4e-3, 5e-5, 5e-3, "circular", "z")
k41 = lambda k: k ** (-5.0 / 3.0)
rng = np.random.default_rng(0)
gx = np.linspace(-2e-3, 2e-3, 96)
jones = np.zeros((4, 20000))
jones[0], jones[2] = rng.uniform(-2.2e-3, 2.2e-3, (2, jones.shape[1]))
amp, phase = 1.0 + rng.random(jones.shape[1]), rng.standard_normal(jones.shape[1])
E = rng.standard_normal((2, jones.shape[1])) + 1j * rng.standard_normal((2, jones.shape[1]))
lines_o = np.stack([rng.uniform(-4e-3, 4e-3, 300), np.full(300, -9e-3), rng.uniform(-4e-3, 4e-3, 300)])
lines_d = np.stack([rng.uniform(-0.2, 0.2, 300), np.ones(300), rng.uniform(-0.2, 0.2, 300)])
marks = []
for it in range(60):
    vol = eng.Volume.from_ne(ne, x, x, x, 1064e-9, "z", phaseshift=True)
    if it % 3 == 0:
        vol.attach_aux(np.ones_like(ne), ne, np.zeros(ne.shape + (3,)), 1e-25)
    rays = eng.RayBundle(s0.shape[1]).upload(s0)
    rays.trace(vol, eng.default_t_end(5e-3), 5e-3, precision="mixed" if it % 2 else "f64")
    for img in (eng.DetectorImage.counts(bin_scale=4), eng.DetectorImage.complex_field(bin_scale=4)):
        rays.deposit(img, eng.chain_shadow_two(), kwave=5.9e6 if img.kind else 0.0)
        img.download(); img.close()
    rays.download(); rays.close()
    back = eng.Volume.from_fields(*vol.fields(phase=True)[:3], x, x, x, vol.omega, "z", nref=ne * 0 + 1 if it % 2 else None)
    back.fields(phase=bool(it % 2)); back.close(); vol.close()
    ps.radial_3Dspectrum(ne, 1e-2, 1e-2, 1e-2) if it % 2 else ps.scalar2D_knyquist(ne[32], 1e-2, 1e-2)
    gaussian3D(k41).domain_fft(1.0, 0.05, 5, 24, 1.0, device=True)
    gaussian3D(k41).cos(1.0, 1.0, 1.0, 24, 20, 70, 64, 2.0, device=True) if it % 2 else gaussian2D(k41).cos(1.0, 1.0, 90, 70, 64, 2.0, device=True)
    fi.grid_rays(gx, gx, jones, amp, phase, return_triangles=bool(it % 2))
    fi.propagate(1064e-9, gx, gx, 4e-3, 4e-3, jones, amp, phase, 0.1)
    eng.hist2d(jones[0], jones[2], 64, 48, -2e-3, 2e-3, -2e-3, 2e-3)
    eng.intensity2d(jones[0], jones[2], E, [np.pi / 4, -np.pi / 4, None], 64, 48, -2e-3, 2e-3, -2e-3, 2e-3)
    eng.trace(eng.Volume.from_ne(ne, x, x, x, 1064e-9, "z"), s0[:, :1000], eng.default_t_end(5e-3), 5e-3)
    f_ne = eng.Field(ne, x, x, x)
    eng.sightlines(f_ne, 60.0, 3.0, lines_o, lines_d, omegas=[3.5e15, 1.9e16], toward=-1, step=1e-4, max_steps=300,
                   backlight=np.full((2, 300), 1e-8) if it % 2 else None)
    eng.sightline_spectra(f_ne, 60.0, 3.0, lines_o[:, :16], lines_d[:, :16], omegas=np.geomspace(2e15, 2e16, 70 + 200 * (it % 2)),
                          toward=+1, step=1e-4, max_steps=300, want=("intensity", "optical_depth", "column"))
    f_ne.close()
    if it in (9, 59):
        eng.synchronize(); marks.append(used())
print("device MiB in use after 10 and 60 cycles:", [round(m, 1) for m in marks])
assert marks[1] - marks[0] < 64, "device memory grows with the number of cycles"
print("LEAK CHECK OK")
