"""Makes g13_fields.npz: the reference's own outputs of the field generators of src/field_generator (gaussian1D/2D/3D:
cos, fft, domain_fft), each seeded, and the next np.random.random() after each call (where the generator leaves the
global stream) -- what synthpy_amd/field_generator has to reproduce (tests/test_field_generators.py).

    python tests/golden/make_g13_fields.py <reference tree (the directory holding src/)>

Only this script reads the reference; the tests need only the committed npz."""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def k41(k):
    return k ** (-5.0 / 3.0)


def k_neg(k):
    """goes negative for k > 9: the generators' clip(0) zeroes those modes"""
    return k ** (-5.0 / 3.0) * (9.0 - k)


def k_fft(k):
    """finite at k = 0 (the Timmer-Koenig grids hold it)"""
    return 1.0 / (1.0 + (20.0 * k) ** 2)


# tag -> (dimension, spectrum name, method, arguments, seed)
CASES = {
    "cos1a": (1, "k41", "cos", (1.0, 64, 100, 2 * np.pi), 3),
    "cos1b": (1, "k41", "cos", (2.5, 37, 1, 0.7), 4),
    "cos1n": (1, "k_neg", "cos", (1.0, 50, 80, 1.0), 5),
    "cos2a": (2, "k41", "cos", (1.0, 1.3, 24, 20, 60, 2 * np.pi / 1.3), 6),
    "cos2n": (2, "k_neg", "cos", (1.0, 1.0, 16, 16, 40, 1.0), 7),
    "cos3a": (3, "k41", "cos", (1.0, 1.3, 0.7, 12, 10, 8, 40, 4.0), 3),
    "cos3n": (3, "k_neg", "cos", (1.0, 1.0, 1.0, 8, 8, 8, 30, 1.0), 8),
    "fft1a": (1, "k_fft", "fft", (50, 1), 9),
    "fft1b": (1, "k_fft", "fft", (40, 0.5), 10),
    "fft2a": (2, "k_fft", "fft", (20,), 11),
    "dom1a": (1, "k41", "domain_fft", (1.0, 0.05, 1.0, 64), 12),
    "dom2a": (2, "k41", "domain_fft", (1.0, 0.05, 1.0, 24), 13),
}
SPECTRA = {"k41": k41, "k_neg": k_neg, "k_fft": k_fft}


def main():
    sys.path.insert(0, os.path.join(sys.argv[1], "src", "field_generator"))
    import gaussian1D  # noqa: E402  (the reference)
    import gaussian2D  # noqa: E402
    import gaussian3D  # noqa: E402

    classes = {1: gaussian1D.gaussian1D, 2: gaussian2D.gaussian2D, 3: gaussian3D.gaussian3D}
    out = {"versions": np.array(f"numpy {np.__version__}")}
    for tag, (nd, spec, method, args, seed) in CASES.items():
        np.random.seed(seed)
        g = classes[nd](SPECTRA[spec])
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            r = getattr(g, method)(*args)
        out[f"next_{tag}"] = np.float64(np.random.random())
        for q, v in enumerate(r if isinstance(r, tuple) else (r,)):
            out[f"out{q}_{tag}"] = v
        for ax in ("xc", "yc", "zc"):
            if getattr(g, ax, None) is not None:
                out[f"{ax}_{tag}"] = getattr(g, ax)
    path = os.path.join(HERE, "g13_fields.npz")
    np.savez_compressed(path, **out)
    print(f"g13_fields.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
