"""Makes g12_spectra.npz: seeded fields and the reference's own outputs of every power-spectrum helper of
src/utils/power_spectrum.py (radial_1D/3Dspectrum, scalar1D/2D/3D_fft, scalar1D/2D/3D_knyquist, and the smooth=True
variants) -- what synthpy_amd/utils/power_spectrum.py has to reproduce (tests/test_power_spectrum.py).

    python tests/golden/make_g12_spectra.py <reference tree (the directory holding src/)>

Only this script reads the reference; the tests need only the committed npz."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def field(rng, shape):
    """white noise plus a low-order sinusoid, as g7_spectrum's images"""
    f = rng.standard_normal(shape)
    for d, n in enumerate(shape):
        x = np.linspace(0.0, 1.0, n).reshape([n if e == d else 1 for e in range(len(shape))])
        f = f + (1.5 + d) * np.sin(2 * np.pi * (2 + d) * x)
    return f


# tag -> (shape, domain lengths, dx of scalar*D_fft, functions the reference runs on it)
CASES = {
    "d1a": ((4096,), (7.0,), 0.01, ("radial", "fft", "knyquist")),
    "d1b": ((1001,), (3.5,), 0.25, ("radial", "fft", "knyquist")),
    "d2a": ((64, 64), (5.0, 8.0), 0.1, ("fft", "knyquist")),  # radial_2Dspectrum has g7_spectrum
    "d3a": ((32, 32, 32), (10.0, 10.0, 10.0), 0.5, ("radial", "fft", "knyquist")),
    "d3b": ((20, 20, 16), (4.0, 6.0, 5.0), 0.2, ("radial", "fft", "knyquist")),  # lx != ly: the (ky, kx, kz) pairing
    "d3c": ((16, 20, 24), (1.0, 1.0, 1.0), 0.3, ("fft",)),  # the reference's radial / knyquist raise on it
}


def main():
    sys.path.insert(0, os.path.join(sys.argv[1], "src", "utils"))
    import power_spectrum as ps  # noqa: E402  (the reference)

    rng = np.random.default_rng(12)
    out = {"versions": np.array(f"numpy {np.__version__}")}
    for tag, (shape, lengths, dx, kinds) in CASES.items():
        nd = len(shape)
        r = field(rng, shape)
        out[f"r_{tag}"], out[f"l_{tag}"], out[f"dx_{tag}"] = r, np.array(lengths), np.float64(dx)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            if "radial" in kinds:
                fn = getattr(ps, f"radial_{nd}Dspectrum")
                kn, kc, sp = fn(r.copy(), *lengths)
                _, _, sps = fn(r.copy(), *lengths, smooth=True)
                out.update({f"radial_kn_{tag}": kn, f"radial_kc_{tag}": kc, f"radial_sp_{tag}": sp, f"radial_sps_{tag}": sps})
            if "fft" in kinds:
                kw, sp = getattr(ps, f"scalar{nd}D_fft")(r.copy(), dx)
                kw7, sp7 = getattr(ps, f"scalar{nd}D_fft")(r.copy(), dx, k_bin_num=7)
                out.update({f"fft_kw_{tag}": kw, f"fft_sp_{tag}": sp, f"fft7_kw_{tag}": kw7, f"fft7_sp_{tag}": sp7})
            if "knyquist" in kinds:
                fn = getattr(ps, f"scalar{nd}D_knyquist")
                kn, wn, sp = fn(r.copy(), *lengths)
                _, _, sps = fn(r.copy(), *lengths, smooth=True)
                out.update({f"kny_kn_{tag}": np.float64(kn), f"kny_wn_{tag}": wn, f"kny_sp_{tag}": sp, f"kny_sps_{tag}": sps})
    path = os.path.join(HERE, "g12_spectra.npz")
    np.savez_compressed(path, **out)
    print(f"g12_spectra.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
