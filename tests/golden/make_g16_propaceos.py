"""Makes g16_propaceos.npz and the synthetic PROPACEOS files g16_*.prp beside it: small text tables in the layout the reference's
src/utils/eos_opacity.py::read_propaceos parses, and what that function returned for them -- what
synthpy_amd/utils/eos_opacity.py::read_propaceos has to reproduce bit for bit (tests/test_eos_opacity.py).

    python tests/golden/make_g16_propaceos.py <reference tree (the directory holding src/)>

Only this script reads the reference; the tests need the committed .prp files (data: numbers and title lines) and the npz.
Layout of a file: 38 header lines; a count line and rows of ten values for the temperatures [eV], the same for the ion number
densities [cm^-3]; the two grids again and 5 more lines (the reader skips them); the group count, one line, the group edges [eV]
in rows of ten; then each table after one title line, a temperature's densities in rows of ten."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = ("zf_table", "ross_opacity", "emiss_opacity", "abs_opacity", "en_table", "eion_table", "eele_table", "pion_table", "pele_table")
FLAG = {"zf_table": "need_zf_table", "ross_opacity": "need_ross_opacity", "emiss_opacity": "need_emiss_opacity",
        "abs_opacity": "need_abs_opacity", "en_table": "need_en_table", "eion_table": "need_eion", "eele_table": "need_eele",
        "pion_table": "need_pion", "pele_table": "need_pele"}
# tag -> (seed, nT, nD, groups, the tables the file holds = the flags the reader is called with)
CASES = {
    "all": (1, 20, 10, 10, ALL),
    "opac": (2, 20, 10, 10, ("ross_opacity", "emiss_opacity", "abs_opacity")),
    "t10d20": (3, 10, 20, 10, ALL),
    "onegroup": (4, 20, 10, 1, ("emiss_opacity", "abs_opacity")),
}


def path(tag):
    return os.path.join(HERE, f"g16_{tag}.prp")


def flags(tag):
    return {FLAG[k]: True for k in CASES[tag][4]}


def _rows(values):
    v = list(values)
    return [" ".join(f"{x:.8E}" for x in v[k:k + 10]) for k in range(0, len(v), 10)]


def content(tag):
    """The written numbers of a case: temperatures, densities, rad_groups and the tables, as float64 BEFORE formatting."""
    seed, n_t, n_d, n_g, tables = CASES[tag]
    rng = np.random.RandomState(seed)
    out = {"temperatures": np.sort(10.0 ** rng.uniform(0.0, 2.7, n_t)), "densities": np.sort(10.0 ** rng.uniform(17.0, 21.0, n_d)),
           "rad_groups": np.geomspace(8.0, 18.0, n_g + 1)}
    for k in tables:
        out[k] = 10.0 ** rng.uniform(-1.0, 3.0, (n_t, n_d))
    return out


def write(tag):
    c = content(tag)
    n_t, n_d, n_g = len(c["temperatures"]), len(c["densities"]), len(c["rad_groups"]) - 1
    lines = [f"header line {k + 1} of 38 (synthetic PROPACEOS layout, case {tag})" for k in range(38)]
    for _ in range(2):  # the grids, then the opacity grids (the same; skipped by the reader)
        lines += [str(n_t)] + _rows(c["temperatures"]) + [str(n_d)] + _rows(c["densities"])
    lines += [f"spacer line {k + 1} of 5" for k in range(5)]
    lines += [str(n_g), "photon energy group boundaries (eV)"] + _rows(c["rad_groups"])
    for k in CASES[tag][4]:
        lines.append(f"table {k}")
        for t in range(n_t):
            lines += _rows(c[k][t])
    with open(path(tag), "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main(reference):
    sys.path.insert(0, reference)
    from src.utils.eos_opacity import read_propaceos

    out = {}
    for tag in CASES:
        write(tag)
        got = read_propaceos(path(tag), **flags(tag))
        want = content(tag)
        out[f"{tag}/keys"] = np.array(list(got))
        out[f"{tag}/none"] = np.array([k for k, v in got.items() if v is None], dtype="U16")
        for k, v in got.items():
            if v is not None:
                out[f"{tag}/{k}"] = v
                assert v.shape == want[k].shape and np.allclose(v, want[k], rtol=1e-8, atol=0), (tag, k)  # 9 digits were written
        print(tag, {k: (None if v is None else v.shape) for k, v in got.items()})
    np.savez_compressed(os.path.join(HERE, "g16_propaceos.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
