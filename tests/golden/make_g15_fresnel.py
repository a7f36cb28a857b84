"""Makes g15_fresnel.npz: the reference's own outputs of src/simulator/fresnel_integral.py -- prepare_field_for_propagation,
fresnel_propagate (LANEX PSF off and on) and propagate -- and the amplitude and phase grids of scipy's
LinearNDInterpolator called as propagate calls it: what synthpy_amd/simulator/fresnel_integral.py has to reproduce
(tests/test_fresnel.py).

    python tests/golden/make_g15_fresnel.py <reference tree (the directory holding src/)>

Only this script reads the reference; the tests need only the committed npz.  The npz holds seeds and outputs: the inputs
are drawn again from np.random.RandomState(seed) by rays() and field() below, which the tests import."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# propagate cases: tag -> (seed, rays, beam, len(x), len(y), x_length, y_length, pad_factor)
RAY_CASES = {
    "square": (1, 3000, "box", 32, 32, 4e-3, 4e-3, 2),
    "rect": (2, 2500, "box", 40, 24, 6e-3, 3e-3, 1),  # len(x) != len(y), x_length != y_length: the dx quirk
    "circle": (3, 2000, "circle", 36, 36, 5e-3, 5e-3, 2),  # a beam narrower than the grid: corner nodes outside the hull
    "sparse": (4, 300, "box", 48, 40, 4e-3, 3e-3, 1),  # fewer rays than nodes: large triangles
    "dense": (5, 20000, "box", 20, 16, 2e-3, 2e-3, 2),  # many more rays than nodes
}
LWL, Z = 1064e-9, 0.05

# fresnel_propagate / prepare_field_for_propagation cases: tag -> (seed, shape, L, pad_factor, lanex_fwhm_m)
FIELD_CASES = {
    "f12x10_p2": (11, (12, 10), (3e-3, 2e-3), 2, None),
    "f12x10_p2_psf": (11, (12, 10), (3e-3, 2e-3), 2, 60e-6),
    "f9x13_p1": (12, (9, 13), (2e-3, 3e-3), 1, None),
    "f9x13_p1_psf": (12, (9, 13), (2e-3, 3e-3), 1, 25e-6),
    "f1x7_p2": (13, (1, 7), (1e-3, 1e-3), 2, None),  # an axis of length 1: numpy's reflect repeats its value
}


def rays(tag):
    """(x, y, jones_vector (4, n), amplitudes, phases) of a propagate case"""
    seed, n, beam, nx, ny, xl, yl, _ = RAY_CASES[tag]
    rng = np.random.RandomState(seed)
    if beam == "box":  # uniform over a box 10 % wider than the grid
        xr = rng.uniform(-0.55 * xl, 0.55 * xl, n)
        yr = rng.uniform(-0.55 * yl, 0.55 * yl, n)
    else:  # uniform over a disc of radius 0.4 x_length
        rad = 0.4 * xl * np.sqrt(rng.uniform(0.0, 1.0, n))
        th = rng.uniform(0.0, 2 * np.pi, n)
        xr, yr = rad * np.cos(th), rad * np.sin(th)
    jones = np.zeros((4, n))
    jones[0], jones[2] = xr, yr
    jones[1], jones[3] = rng.normal(0.0, 1e-3, n), rng.normal(0.0, 1e-3, n)
    amp = 1.0 + 0.5 * np.cos(2 * np.pi * xr / xl) * np.sin(3 * np.pi * yr / yl) + 0.05 * rng.uniform(0.0, 1.0, n)
    phase = 40.0 * ((xr / xl) ** 2 + (yr / yl) ** 2) + 0.2 * rng.normal(0.0, 1.0, n)
    x = np.linspace(-xl / 2, xl / 2, nx)
    y = np.linspace(-yl / 2, yl / 2, ny)
    return x, y, jones, amp, phase


def field(tag):
    """the complex field of a fresnel_propagate / prepare case"""
    seed, shape = FIELD_CASES[tag][:2]
    rng = np.random.RandomState(seed)
    return rng.uniform(0.5, 1.5, shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))


def main():
    sys.path.insert(0, os.path.join(sys.argv[1], "src", "simulator"))
    import fresnel_integral as fi  # noqa: E402  (the reference)
    from scipy.interpolate import LinearNDInterpolator as LND

    out = {"versions": np.array(f"numpy {np.__version__}")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for tag, (seed, shape, L, pf, lanex) in FIELD_CASES.items():
            U0 = field(tag)
            prep = fi.prepare_field_for_propagation(U0.copy(), pad_factor=pf)
            out[f"prep_{tag}"] = prep
            out[f"fp_{tag}"] = fi.fresnel_propagate(prep.copy(), L, LWL, Z, shape, pad_factor=pf, lanex_fwhm_m=lanex)
        for tag, (seed, n, beam, nx, ny, xl, yl, pf) in RAY_CASES.items():
            x, y, jones, amp, phase = rays(tag)
            out[f"prop_{tag}"] = fi.propagate(LWL, x, y, xl, yl, jones.copy(), amp.copy(), phase.copy(), Z, pad_factor=pf)
            XX, YY = np.meshgrid(x, y)
            out[f"amp_{tag}"] = LND((jones[0], jones[2]), amp, fill_value=0.0)((XX, YY))
            out[f"phase_{tag}"] = LND((jones[0], jones[2]), phase, fill_value=0.0)((XX, YY))
    path = os.path.join(HERE, "g15_fresnel.npz")
    np.savez_compressed(path, **out)
    print(f"g15_fresnel.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
