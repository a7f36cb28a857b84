"""Makes g14_shapes.npz: the reference's legacy ScalarDomain.solve on a grid whose three node counts and half-lengths all
differ (41 x 29 x 23 nodes over +-5, +-4, +-3 mm), probed along x, y and z -- its float32 gradients, its default solve
and a solve_ivp run of its own dsdt at rtol 1e-10 / atol 1e-12 (as g2_trace) -- what the oracle and every trace kernel are
held to on a non-cubic grid (tests/test_oracle_golden.py, tests/test_grid_shapes.py).

    python tests/golden/make_g14_shapes.py <reference tree (the directory holding src/)>

Only this script reads the reference; the tests need only the committed npz."""
import contextlib
import io
import os
import sys

import numpy as np
from scipy.integrate import solve_ivp

HERE = os.path.dirname(os.path.abspath(__file__))
LWL = 1064e-9
NODES = (41, 29, 23)
HALF = (5e-3, 4e-3, 3e-3)
N_RAYS = 96


def axes():
    return [np.linspace(-h, h, n) for n, h in zip(NODES, HALF)]


def blob(x, y, z):
    """a smooth, off-centre Gaussian blob, narrower along the shorter axes, with a weak ripple (no symmetry plane)"""
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    r2 = ((X - 3e-4) / 2.0e-3) ** 2 + ((Y + 2e-4) / 1.6e-3) ** 2 + (Z / 1.2e-3) ** 2
    return 1e25 * np.exp(-r2) * (1.0 + 0.1 * np.sin(1.3e3 * X + 0.9e3 * Y) * np.cos(1.1e3 * Z))


def main():
    sys.path.insert(0, os.path.join(sys.argv[1], "src", "solvers-legacy"))
    import full_solver as fs  # noqa: E402  (the reference)

    fs.omega_pe = lambda ne: 5.64e4 * np.sqrt(ne)  # the method lacks `self` and is looked up as a module global (make_golden.py)
    x, y, z = axes()
    ne = np.float64(np.float32(blob(x, y, z)))  # float64 values that hold 24 significant bits: the file stays small
    out = {"versions": np.array(f"numpy {np.__version__}"), "x": x, "y": y, "z": z, "ne": ne, "lwl": LWL}
    for a, pdir in enumerate("xyz"):
        ext = HALF[a] + 1e-4  # the rays start 0.1 mm before the first node plane of the probing axis
        dom = fs.ScalarDomain(x, y, z, ext, phaseshift=True, probing_direction=pdir)
        dom.external_ne(ne)
        dom.calc_dndr(LWL)
        if a == 0:
            out.update(omega=np.float64(dom.omega), dndx=dom.dndx, dndy=dom.dndy, dndz=dom.dndz)
        np.random.seed(40 + a)
        s0 = fs.init_beam(N_RAYS, 2.5e-3, 5e-5, ext, "circular", probing_direction=pdir)
        with contextlib.redirect_stdout(io.StringIO()):
            rf_d, Jf_d = dom.solve(s0.copy(), return_E=True)
        t_end = np.sqrt(8.0) * ext / fs.c
        sol = solve_ivp(lambda t, yv: fs.dsdt(t, yv, dom), [0, t_end], s0.flatten(), t_eval=[0, t_end], rtol=1e-10, atol=1e-12)
        sf_t = sol.y[:, -1].reshape(9, N_RAYS)
        rf_t, Jf_t = fs.ray_to_Jonesvector(sf_t, ext, probing_direction=pdir)
        out.update({f"extent_{pdir}": np.float64(ext), f"s0_{pdir}": s0, f"sf_default_{pdir}": dom.sf.copy(),
                    f"rf_default_{pdir}": rf_d, f"Jf_default_{pdir}": Jf_d, f"sf_tight_{pdir}": sf_t, f"rf_tight_{pdir}": rf_t,
                    f"Jf_tight_{pdir}": Jf_t})
    path = os.path.join(HERE, "g14_shapes.npz")
    np.savez_compressed(path, **out)
    print(f"g14_shapes.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
