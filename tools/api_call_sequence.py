"""Every call into libsynthray.so that the two API generations make for one fixed flow, in order, with a hash of what each
step handed back.  Run on two versions of the Python layer (TREE = a checkout with its library built; default: this one), the
two logs must be equal line for line: the check that a change to the mirror classes reaches the device with the same calls
and hands back the same bits (profiles/api_mirrors_rate.txt).  --emission: the flow through the emission family instead
(self_emission, table_emission, sightline_emission, sightline_spectra on a domain of each generation: emission_family below;
profiles/emission_family_rate.txt).
    python tools/api_call_sequence.py OUTFILE [TREE] [--emission]"""
import hashlib, os, pickle, sys
import numpy as np

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
sys.path.insert(0, os.path.abspath(ARGS[1]) if len(ARGS) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthpy_amd import _ffi

log = []


class Recorder:
    def __init__(self, real):
        self.__dict__["_real"] = real

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.startswith("sr_"):
            return f

        def call(*a):
            log.append(name)
            return f(*a)

        return call


_ffi.lib = Recorder(_ffi.lib)
from synthpy_amd import engine, resident  # noqa: E402
from synthpy_amd.simulator import diagnostics as diag, domain as d, propagator as p  # noqa: E402
from synthpy_amd.solvers_legacy import full_solver as fs, rtm_solver as rtm  # noqa: E402

assert isinstance(engine.lib, Recorder)


def mark(label, *arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(b"None" if a is None else np.ascontiguousarray(np.asarray(a)).tobytes())
    log.append(f"# {label} {h.hexdigest()[:16]}")


def finish():
    with open(ARGS[0], "w") as f:
        f.write("\n".join(log) + "\n")
    print(len(log), "lines ->", ARGS[0])


def emission_family():
    """Every entry of the emission family on a 24 x 20 x 16 domain of each generation, both nodes, a pixel grid (handed over in
    tile order) and chords with a backlight."""
    from synthpy_amd import sightlines
    from synthpy_amd.utils.eos_opacity import OpacityTable, SpectralOpacityTable

    dims, cell = (24, 20, 16), 2.5e-4
    lengths = tuple(cell * (m - 1) for m in dims)
    rng = np.random.default_rng(22)
    ne = (1e25 * rng.uniform(0.5, 1.5, dims)).astype(np.float32)
    Te = (80.0 * rng.uniform(0.5, 1.5, dims)).astype(np.float32)
    T, D = np.geomspace(1.0, 500.0, 10), np.geomspace(1e17, 1e21, 12)
    opac = lambda nb: 10.0 ** rng.uniform(1.0, 3.0, (nb, len(T), len(D)))
    table = OpacityTable(T, D, opac(3), [90.0, 200.0, 450.0], 12.011, emission=opac(3), edges=[[60, 130], [130, 300], [300, 700]])
    e30 = np.geomspace(30.0, 900.0, 30)
    spectral = SpectralOpacityTable(T, D, opac(30), e30, 12.011, emission=opac(30), edges=np.stack([e30 / 1.06, e30 * 1.06], axis=1))
    cam = sightlines.PinholeCamera((0, 0, 20e-3), (0.1, 0, -1), (0, 1, 0), 60e-3, (12, 10), cell * 3)
    nch = 7
    origins = np.stack([np.linspace(-2e-3, 2e-3, nch), np.full(nch, -8e-3), np.linspace(-1e-3, 1e-3, nch)])
    dirs = np.stack([np.linspace(0.1, -0.1, nch), np.ones(nch), np.linspace(-0.05, 0.3, nch)])
    chords = lambda toward, backlight: sightlines.Chords(origins, dirs, toward, backlight=backlight)
    lam, e70 = [532e-9, 100e-9], np.geomspace(1.0, 60.0, 70)
    sight = ("intensity", "optical_depth", "column", "chord", "steps")
    for gen, dom in (("simulator", d.ScalarDomain(lengths, dims)),
                     ("legacy", fs.ScalarDomain(*[np.linspace(-L / 2, L / 2, m) for L, m in zip(lengths, dims)], lengths[2] / 2))):
        dom.external_ne(ne)
        dom.external_Te(Te)
        dom.external_Z(3.0)
        back = rng.uniform(0.0, 2e-7, (2, dims[0], dims[1]))
        for toward in ("+", "-"):
            em = dom.self_emission(lam, toward=toward, backlight=back)
            mark(f"{gen} self_emission {toward}", em.intensity, em.optical_depth, em.transmission)
        em = dom.table_emission(table)
        mark(f"{gen} table_emission", em.intensity, em.optical_depth, em.transmission, em.band_radiance)
        for name, view, kw in (("pinhole", cam, {"wavelengths": lam}), ("pinhole", cam, {"table": table}),
                               ("chords", chords(-1, rng.uniform(0.0, 2e-7, (2, nch))), {"wavelengths": lam}),
                               ("chords", chords(-1, rng.uniform(0.0, 2e-7, (3, nch))), {"table": table})):
            em = dom.sightline_emission(view, **kw)
            mark(f"{gen} sightline_emission {name} {list(kw)[0]}", *(getattr(em, k) for k in sight), em.transmission)
        mark(f"{gen} sightline_emission band_radiance", em.band_radiance)
        for name, view, kw in (("chords", chords(-1, 1e-8), {"photon_energies": e70}),
                               ("chords", chords(+1, rng.uniform(0.0, 2e-7, (30, nch))), {"table": spectral}),
                               ("pinhole", cam, {"table": spectral})):
            sp = dom.sightline_spectra(view, **kw)
            mark(f"{gen} sightline_spectra {name} {list(kw)[0]}", *(getattr(sp, k) for k in sight), sp.transmission, sp.signal())
        mark(f"{gen} sightline_spectra band_radiance", sp.band_radiance)


engine.init(0)
if "--emission" in sys.argv:
    emission_family()
    finish()
    sys.exit(0)
n, ext, lwl, N = 48, 5e-3, 1064e-9, 20000
x = np.linspace(-ext, ext, n)
X, Y, Z = np.meshgrid(x, x, x, indexing="ij", sparse=True)
ne = 1e25 * np.exp(-(X ** 2 + Y ** 2 + Z ** 2) / (1.5e-3) ** 2) + 2e24 * (1 + np.sin(2e3 * X) * np.cos(3e3 * Y))
Te, Zi = 50.0 + 0 * ne + 1e3 * np.abs(X), 3.0 + 0 * ne
B = np.zeros(ne.shape + (3,))
B[..., 2] = 5.0 * (1 + X / ext)
np.random.seed(0)
s0 = fs.init_beam(N, 4e-3, 5e-5, ext, "circular", "z")

# ---- legacy generation ----
dom = fs.ScalarDomain(x, x, x, ext, phaseshift=True, inv_brems=True, B_on=True)
dom.external_ne(np.float32(ne))  # float32: kappa() scales it in float32
dom.external_Te(Te)
dom.external_Z(Zi)
dom.external_B(B)
dom.calc_dndr(lwl)
mark("legacy kappa()", dom.kappa())
rf, Jf = dom.solve(s0, return_E=True)
mark("legacy solve", rf, Jf, dom.sf)
sh = rtm.Shadowgraphy(rf)
sh.two_lens_solve()
sh.histogram()
mark("legacy shadow", sh.H)
sc = rtm.Schlieren(rf)
sc.DF_solve()
sc.histogram(bin_scale=4)
mark("legacy schlieren", sc.H, sc.rf, sc.r0)
it = rtm.Interferometry(rf, E=Jf)
it.two_lens_solve(wl=lwl)
it.interferogram(bin_scale=10)
mark("legacy interferogram", it.rf, it.rE)
rr = rtm.Refractometry(rf, E=Jf)
rr.coherent_solve()
rr.incoherent_solve()
mark("legacy refractometry", rr.rf, rr.rE)
rr.rf = np.array(rr.rf)
rr.coherent_solve()
rr.histogram(clear_mem=True)
mark("legacy refractometry after rf assigned", rr.H, rr.rE)
po = rtm.Polarimetry(rf, Jf)
po.two_lens_solve()
po.polarogram(bin_scale=4)
mark("legacy polarogram shape", np.array(po.I.shape))
clone = pickle.loads(pickle.dumps(po))
mark("legacy pickle", clone.rf, clone.r0, np.array(sorted(clone.__dict__)))
it.E = np.array(Jf) * 0.5
it.two_lens_solve(wl=lwl)
mark("legacy E assigned", it.rf, it.rE)
rf2 = dom.solve(np.ascontiguousarray(s0[:, : N // 2]))
mark("legacy second solve, another size", rf2)
dom.clear_memory()

# ---- simulator generation ----
for regions in (1, 3):
    sd = d.ScalarDomain(2 * ext, n, phaseshift=True, inv_brems=True, B_on=True, region_count=regions, auto_batching=False)
    sd.external_ne(ne)
    sd.external_Te(np.float32(Te))
    sd.external_Z(3.0)
    sd.external_B(B)
    mark(f"simulator aux fields ({regions})", *p._aux_fields(sd, lwl)[:3])
    rf, Jf, _ = p.solve(s0, sd, ext, return_E=True, lwl=lwl)
    mark(f"simulator solve ({regions})", rf, Jf, np.array(p.solve.last_stats.ray_steps))
    a = diag.Shadowgraphy(lwl, rf, Jf)
    a.two_lens_solve()
    a.histogram(bin_scale=4)
    mark("simulator shadow", a.H, a.rf, a.Jf, a.r0)
    b = diag.Interferometry(lwl, rf, Jf)
    b.interfere_ref_beam(10, 10)
    mark("simulator ref beam", b.Jf)
    b.two_lens_solve()
    b.interferogram(bin_scale=10)
    mark("simulator interferogram", b.rf, b.Jf)
    b.Jf = np.array(b.Jf) * 0.5
    b.two_lens_solve()
    b.interferogram(bin_scale=10)
    mark("simulator Jf assigned", b.rf, b.Jf, np.array(b.on_device))
    c = diag.Refractometry(lwl, rf, Jf)
    c.coherent_solve()
    c.incoherent_solve()
    c.rf = np.array(c.rf)
    c.histogram(clear_mem=True)
    mark("simulator refractometry", c.H)
    q = diag.Polarimetry(lwl, rf, Jf)
    q.single_lens_solve()
    q.polarogram(bin_scale=4)
    clone = pickle.loads(pickle.dumps(q))
    mark("simulator pickle", clone.rf, clone.Jf, clone.r0, np.array(sorted(clone.__dict__)))
    e = diag.Schlieren(lwl, rf)
    e.r0 = np.array(e.r0)
    e.LF_solve()
    e.histogram(bin_scale=4)
    mark("simulator r0 assigned", e.H)
    resident.release(sd._rays)
    mark("simulator after release", a.rf, a.Jf)
s = s0[:, :64].flatten()
ds = p.dsdt(0.0, s, True, True, True, True, ne, B, np.float32(Te), 3.0, sd.x, sd.y, sd.z, 2 * np.pi * engine.c / lwl, 2.62e-13 * lwl ** 2)
mark("simulator dsdt", ds)
finish()
