"""Every call into libsynthray.so that the two API generations make for one fixed flow, in order, with a hash of what each
step handed back.  Run on two versions of the Python layer (TREE = a checkout with its library built; default: this one), the
two logs must be equal line for line: the check that a change to the mirror classes reaches the device with the same calls
and hands back the same bits (profiles/api_mirrors_rate.txt).
    python tools/api_call_sequence.py OUTFILE [TREE]"""
import hashlib, os, pickle, sys
import numpy as np

sys.path.insert(0, os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


engine.init(0)
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
with open(sys.argv[1], "w") as f:
    f.write("\n".join(log) + "\n")
print(len(log), "lines ->", sys.argv[1])
