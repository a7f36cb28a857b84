"""What the field diagnostics share on the host: a domain's fields as engine.Field uploads, and the fields' grid.

    with fields.staged(domain, caller_fields) as src:         # the caller's SourceFields, or a fresh one closed on exit
        f = src.get_all({"ne": ne, "Te": Te, "Z": None})      # one dtype for all the uploads
        engine.thomson(f["ne"], f["Te"], ...)

orientation.rotated / views, emission.self_emission / table_emission, radiography.radiograph, thomson.spectra / spectra_multi /
spectra_sg and wave.propagate stage through here, so a SourceFields of one domain serves them all: each field is uploaded once, at its first
use, and kept until close().  grid_f64 and locate are the host's restatement of what the kernels see: node coordinates rounded
to float32 (sr_field_create takes float32) and sr_field_resample's cell rule (sr::locate_in, include/synthray.h).
"""
from __future__ import annotations

from contextlib import contextmanager

import numpy as np

from . import engine


def grid_f64(domain):
    """The node coordinates of the domain's fields as the device holds them: float32 values, widened to float64."""
    return [np.float64(np.float32(a)) for a in (domain.x, domain.y, domain.z)]


def locate(g, p):
    """(cell, weight, inside) of the positions p on one axis with the nodes g: the largest cell with g[cell] <= p, clipped to
    len(g) - 2, and (p - g[cell]) / (g[cell + 1] - g[cell]); inside is False for a p outside g[0]..g[-1] or NaN, whose weight
    is that of the nearer end (NaN for a NaN)."""
    p = np.asarray(p, np.float64)
    with np.errstate(invalid="ignore"):
        inside = (p >= g[0]) & (p <= g[-1])
    cell = np.clip(np.searchsorted(g, p, side="right") - 1, 0, len(g) - 2)
    return cell, (np.clip(p, g[0], g[-1]) - g[cell]) / (g[cell + 1] - g[cell]), inside


def uniform(a):
    """The one value of a scalar, or of an array broadcast from one; None for a real array."""
    if np.ndim(a) == 0:
        return float(a)
    a = np.asarray(a)
    if a.size == 1 or all(s == 0 for s in a.strides):
        return float(a.reshape(-1)[0])
    return None


class SourceFields:
    """The fields of one domain as engine.Field handles, each uploaded at its first use and kept until close()."""

    def __init__(self, domain):
        self.domain = domain
        self.fields = {}

    def get(self, name, array):
        if name not in self.fields:
            d = self.domain
            self.fields[name] = engine.Field(array, d.x, d.y, d.z)
        return self.fields[name]

    def get_all(self, named):
        """{name: Field | None} for {name: array | None}, all in ONE dtype, as a kernel that reads several fields wants them:
        float32 only when every array is float32; otherwise float64, the float32 arrays widened (exact, so results do not
        change) and kept under name + ":float64"."""
        single = all(a.dtype == np.float32 for a in named.values() if a is not None)
        out = {}
        for name, a in named.items():
            if a is None:
                out[name] = None
            elif single or a.dtype == np.float64:
                out[name] = self.get(name, a)
            else:
                out[name] = self.get(name + ":float64", np.asarray(a, np.float64))
        return out

    @property
    def nbytes(self):
        return sum(f.nbytes for f in self.fields.values())

    def close(self):
        for f in self.fields.values():
            f.close()
        self.fields = {}


@contextmanager
def staged(domain, fields, word="fields"):
    """The SourceFields a call uploads through: the caller's `fields` (of the same domain, else ValueError; `word` names the
    caller's keyword in the text), or a fresh one that is closed when the block ends, also by an exception."""
    if fields is not None:
        if fields.domain is not domain:
            raise ValueError(f"{word} holds the fields of another domain")
        yield fields
        return
    src = SourceFields(domain)
    try:
        yield src
    finally:
        src.close()
