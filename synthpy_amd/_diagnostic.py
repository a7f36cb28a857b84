"""What the two generations of diagnostics classes (solvers_legacy/rtm_solver.py, simulator/diagnostics.py) share: the state
machine of an object whose rays may still be in the bundle a solve() left in HBM (resident.py), and the subclass bodies that
are the same in both.

ResidentRays owns the attachment, the write guard, r0, leaving the device (on a setter, on pickling, on resident.release),
the step "record the chain on the device, else run it on the host", the counts histogram, intensity(), plot() and
clear_rays().  A generation says what differs:

    _TRACKED            the attributes whose arrays are write-tracked while the rays are resident
    _CLEARED            the attributes clear_rays() forgets
    _fetch()            the chain's output (and whatever else the generation hands out) from the device to the host
    _field()            the field array the host path reads: E, fixed at construction | Jf, which the chains rewrite
    _need_field(who)    ValueError when the object carries no field
    _records()          may a *_solve() still record on the device?
    _output(r, E, f)    keep a chain's output: (None, None) after a recording, the host path's arrays otherwise
"""
from __future__ import annotations

import numpy as np

from . import engine, resident


class ResidentRays:
    _TRACKED = _CLEARED = ()

    def _attach(self, rf, field):
        """True when rf (and field) are the arrays a solve() has just returned: the object then works on that bundle."""
        bundle = resident.attach(self, rf, field)
        self._dev = None if bundle is None else resident.DeviceRays(bundle, field is not None)
        return self._dev is not None

    @property
    def on_device(self) -> bool:
        """True while histogram() / interferogram() deposit from the bundle solve() left in HBM."""
        return self._dev is not None and self._dev.live

    def _guard(self):
        """The reference reads its arrays when *_solve() / histogram() / interferogram() run, so a write to any of them since
        this object took the device path counts: the arrays it holds or hands out while its rays are resident are write-tracked
        (resident.TrackedArray), and once one has been written to the object works on its host arrays, as they are now, from
        here on."""
        if self._dev is not None and any(resident.dirty(getattr(self, a)) for a in self._TRACKED):
            self._leave_device(keep=True)

    @property
    def r0(self):
        if self._r0 is None and self.on_device:
            self._r0 = resident.track(self._dev.host(ops=[], with_E=False)[0])
        return self._r0

    @r0.setter
    def r0(self, value):
        self._leave_device(keep=False)  # other rays than the resident ones from here on
        self._r0 = value

    def _to_host(self):
        """Bring r0 (and the last *_solve()'s output) to the host and let go of the bundle (resident.release, pickling)."""
        self._leave_device(keep=True)

    def _leave_device(self, keep):
        if self._dev is None:
            return
        if keep and self._dev.live:
            _ = self.r0
            self._fetch()
        self._dev.drop(self)
        self._dev = None

    def __getstate__(self):
        self._to_host()
        return self.__dict__.copy()

    def _records(self):
        return self.on_device

    def _run(self, ops, kwave=None):
        """A *_solve(): the chain is recorded for the deposit while the rays are resident, else applied to r0 on the host.
        With kwave the chain carries the field: E *= exp(1j*kwave*|dr|) over its legs."""
        carries = kwave is not None
        self._guard()
        if self._records():
            self._dev.record(ops, kwave=kwave or 0.0)
            self._output(None, None, carries)
        else:
            self._output(*engine.optics(self.r0, ops, E=self._field() if carries else None, kwave=kwave or 0.0), carries)

    def _deposits_from_device(self):
        return self.on_device and self._dev.ops is not None and not self._assigned

    def _detector(self, bin_scale, pix_x, pix_y):
        """histogram()'s detector: (nx, ny, range); sets xedges / yedges as numpy returns them."""
        nx, ny = pix_x // bin_scale, pix_y // bin_scale
        self.xedges = np.linspace(-self.Lx / 2, self.Lx / 2, nx + 1)
        self.yedges = np.linspace(-self.Ly / 2, self.Ly / 2, ny + 1)
        return nx, ny, (-self.Lx / 2, self.Lx / 2, -self.Ly / 2, self.Ly / 2)

    def histogram(self, bin_scale=1, pix_x=3448, pix_y=2574, clear_mem=False):
        """np.histogram2d of the detector-plane positions; H [y_bin, x_bin] float64 holding exact counts, xedges / yedges as
        numpy returns them (rtm_solver.py:156-178, where bin_scale defaults to 10; diagnostics.py:323-353)."""
        nx, ny, rng = self._detector(bin_scale, pix_x, pix_y)
        self._guard()
        if self._deposits_from_device():
            self.H = self._dev.counts(nx, ny, *rng)
        else:
            self.H = engine.hist2d(self.rf[0], self.rf[2], nx, ny, *rng).astype(np.float64)
        if clear_mem:
            self.clear_rays()

    def intensity(self, analyser=None, bin_scale=1, pix_x=3448, pix_y=2574, clear_mem=False):
        """Analyser-weighted intensity images of the detector-plane rays: I (n_ch, pix_y // bin_scale, pix_x // bin_scale),
        I[c] = np.histogram2d(..., weights=w_c) on histogram()'s detector, xedges / yedges as histogram() sets them; .H is
        left alone.  No reference counterpart (the reference shows amplitude and polarisation in no image).

        analyser: None, one angle [rad], or a sequence of up to 4 angles, None among them = no analyser.  An analyser at
        angle beta, measured from the y axis in the sense `pol` is, passes the component of the field (E | Jf) along
        (-sin beta, cos beta): w = |(-sin beta) E_x + (cos beta) E_y|^2 = amp^2 cos^2(pol - beta); without analyser
        w = |E_x|^2 + |E_y|^2 (the attenuation image).  The sum over a pixel's rays is incoherent, so the field factors of a
        chain's legs (modulus 1) play no part: no reference beam, no field propagation, the weights come from the field as
        given."""
        self._need_field("intensity")
        nx, ny, rng = self._detector(bin_scale, pix_x, pix_y)
        self._guard()
        # a reference beam added to the resident field is part of what .Jf holds: then the host arrays are what is binned
        if self._deposits_from_device() and self._dev.has_E and not self._dev.refs:
            self.I = self._dev.intensity(analyser, nx, ny, *rng)
        else:
            self.I = engine.intensity2d(self.rf[0], self.rf[2], self._field(), analyser, nx, ny, *rng)
        if clear_mem:
            self.clear_rays()

    def plot(self, ax, clim=None, cmap=None):
        ax.imshow(self.H, interpolation="nearest", origin="lower", clim=clim, cmap=cmap,
                  extent=[self.xedges[0], self.xedges[-1], self.yedges[0], self.yedges[-1]])

    def clear_rays(self):
        self._leave_device(keep=False)
        for a in self._CLEARED:
            setattr(self, a, None)
        self._assigned = False


# ---- the subclass bodies both generations have: each derives its class from one of these and its own base ----------------
class ShadowgraphyChains:
    def single_lens_solve(self):
        self._run(engine.chain_shadow_single(self.L, self.R, self.focal_plane))

    def two_lens_solve(self):
        self._run(engine.chain_shadow_two(self.L, self.R, self.focal_plane))


class SchlierenChains:
    def DF_solve(self, R=1):
        self._run(engine.chain_schlieren(self.L, self.R, self.focal_plane, R, dark_field=True))

    def LF_solve(self, R=1):
        self._run(engine.chain_schlieren(self.L, self.R, self.focal_plane, R, dark_field=False))


class RefractometryChains:
    def incoherent_solve(self):
        self._run(engine.chain_refractometry(self.L, self.R, self.focal_plane))


class PolarimetryImages(ShadowgraphyChains):
    """Faraday-rotation imaging through a pair of analysers at +beta and -beta: Shadowgraphy's imaging chains, and intensity
    images weighted by what each analyser passes of the rays' Jones vector.  No reference counterpart: the reference
    carries the rotation (state row 8) into Jf and has no diagnostic that shows it."""

    def polarogram(self, beta=np.pi / 4, bin_scale=1, pix_x=3448, pix_y=2574, clear_mem=False):
        """One pass over the rays, three images: H_plus and H_minus through analysers at +beta and -beta (0 < beta < pi/2),
        H_total without analyser; .beta keeps the angle for rotation()."""
        if not 0 < beta < np.pi / 2:
            raise ValueError("beta must lie in (0, pi/2)")
        self.intensity((beta, -beta, None), bin_scale=bin_scale, pix_x=pix_x, pix_y=pix_y, clear_mem=clear_mem)
        self.H_plus, self.H_minus, self.H_total = self.I
        self.beta = beta

    def rotation(self):
        """The polarisation rotation alpha [rad] per pixel from H_plus and H_minus (engine.rotation_map): NaN where no ray
        landed; unambiguous for |alpha| < min(beta, pi/2 - beta)."""
        return engine.rotation_map(self.H_plus, self.H_minus, self.beta)
