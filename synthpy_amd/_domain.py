"""What the two ScalarDomain mirrors (solvers_legacy/full_solver.py, simulator/domain.py) share: the NRL coefficients of the
optional RHS terms, the argument tuple of engine.Volume.attach_aux, and the entry points that go beyond the reference
(a new diagnostic of a domain is added here, once)."""
from __future__ import annotations

import numpy as np


def omega_pe(ne):
    """Electron plasma frequency [rad/s] of n_e [cm^-3] (NRL formulary p.28; full_solver.py:236-239, propagator.py:23-26)."""
    return 5.64e4 * np.sqrt(ne)


def kappa(ne, Te, Z, omega):
    """Inverse-bremsstrahlung rate coefficient [1/s] of n_e [m^-3], T_e [eV], Z (NRL formulary; full_solver.py:243-268,
    propagator.py:30-60): 3.1e-5 * Z * c * (n_e[cm^-3]/omega)^2 * ln(Lambda) * Te^-1.5, ln(Lambda) = max(2, ln(v_the /
    (omega_max * L_max))).  Nothing is cast here: a float32 n_e is scaled in float32, as each caller always had it."""
    from .engine import c  # (not at import: the simulator's domain module is host NumPy and loads without the library)

    ne_cc = np.asarray(ne) * 1e-6
    omega_max = np.maximum(omega_pe(ne_cc), omega)
    L_max = np.maximum(Z * 1.602176634e-19 / Te,             # classical distance of closest approach
                       2.760428269727312e-10 / np.sqrt(Te))  # de Broglie length
    coulomb_log = np.maximum(2.0, np.log(4.19e5 * np.sqrt(Te) / (omega_max * L_max)))
    return 3.1e-5 * Z * c * np.power(ne_cc / omega, 2) * coulomb_log * np.power(Te, -1.5)


def full(a, shape):
    """`a` broadcast to the grid, contiguous float64."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), shape))


def aux_fields(inv_brems, B_on, ne, Te, Z, B, omega, verdet):
    """What set_up_interps gives dsdt besides the gradients (full_solver.py:276-289; propagator.py:30-60, 137-165): the
    arguments of engine.Volume.attach_aux, (kappa | None, ne | None, B | None, VerdetConst).  ne, Te, Z go into kappa() as
    they are given."""
    return (kappa(ne, Te, Z, omega) if inv_brems else None,
            full(ne, np.shape(ne)) if B_on else None,
            np.ascontiguousarray(B, np.float64) if B_on else None,
            float(verdet) if B_on else 0.0)


class DomainExtras:
    """The entry points of a ScalarDomain that have no reference counterpart, for a class with x, y, z and the field
    attributes ne, B, Te, Z."""

    def external_E(self, E):
        """(nx, ny, nz, 3) grid of the electric field in V/m: what proton_radiograph pushes its particles through beside B.
        The tracer does not read it."""
        E = np.asarray(E)
        shape = (len(self.x), len(self.y), len(self.z), 3)
        if E.shape != shape:
            raise ValueError(f"E has shape {E.shape}, the domain needs {shape}")
        self.E = E

    def external_Ti(self, Ti, Ti_min=1.0):
        """(nx, ny, nz) grid of T_i in eV, floored at Ti_min: what thomson_scattering reads beside Te.  Without it Ti = Te.
        The tracer does not read it."""
        self.Ti = np.maximum(Ti_min, Ti)

    def external_V(self, V):
        """(nx, ny, nz, 3) grid of the flow velocity in m/s: the Doppler shift of thomson_scattering.  The tracer does not
        read it."""
        self.V = V

    def external_Vd(self, Vd):
        """(nx, ny, nz, 3) grid of the electrons' drift relative to the ions in m/s, -J/(e ne) (thomson.drift_velocity): the
        asymmetry of the ion-acoustic peaks in thomson_scattering_multi.  The tracer does not read it."""
        self.Vd = Vd

    def external_order(self, m):
        """(nx, ny, nz) grid (or one number) of the order m of the super-Gaussian electron distribution exp(-(v/v_m)^m), 2
        (Maxwellian) to 5 (thomson.langdon_order): what thomson_scattering_sg reads.  The tracer does not read it."""
        self.order = m

    def proton_radiograph(self, source, det_pos, **kw):
        """The fluence image a radiography.ProtonSource forms on the plane coordinate[source axis] == det_pos [m] after its
        particles have crossed this domain's B (external_B / test_B) and E (external_E): a radiography.Radiograph.
        Keywords: radiography.radiograph's -- material= (a radiography.Material), stop_energy_MeV= and scatter_seed= add the
        stopping and multiple scattering in this domain's ne and Z (external_Z)."""
        from .radiography import radiograph

        return radiograph(self, source, det_pos, **kw)

    def thomson_scattering(self, probe, collection, wavelengths, ion_mass, **kw):
        """The optical Thomson-scattering spectra of this domain's ne, Te (external_Te), Z (external_Z), Ti (external_Ti) and V
        (external_V) for a thomson.Probe and a thomson.Collection at `wavelengths` [m], the ion's mass number ion_mass: a
        thomson.ThomsonSpectra.  Keywords: thomson.spectra's."""
        from .thomson import spectra

        return spectra(self, probe, collection, wavelengths, ion_mass, **kw)

    def thomson_scattering_multi(self, probe, collection, wavelengths, species, **kw):
        """thomson_scattering for a plasma of several ion species -- `species`, 1 to 4 thomson.Species (mass number, charge,
        relative number fraction; this domain's Z is not read) sharing Ti and V -- whose electrons may drift against the ions
        (external_Vd): a thomson.ThomsonSpectra.  Keywords: thomson.spectra_multi's."""
        from .thomson import spectra_multi

        return spectra_multi(self, probe, collection, wavelengths, species, **kw)

    def thomson_scattering_sg(self, probe, collection, wavelengths, species, order=None, **kw):
        """thomson_scattering_multi with super-Gaussian (Langdon) electrons of the local order m -- `order`: None reads
        external_order's grid, or an array or a number in [2, 5] -- as inverse-bremsstrahlung heating leaves them: a
        thomson.ThomsonSpectra.  Keywords: thomson.spectra_sg's."""
        from .thomson import spectra_sg

        return spectra_sg(self, probe, collection, wavelengths, species, order=order, **kw)

    def wave_propagate(self, source, **kw):
        """The wave-optics march of a wave.Source through this domain's ne along its probing_direction: a wave.WaveField on
        the exit plane.  Keywords: wave.propagate's."""
        from .wave import propagate

        return propagate(self, source, **kw)

    def rotated(self, angle_deg=None, about="y", **kw):
        """This domain seen from a frame turned by angle_deg about the lab axis `about` (or matrix=R): a new ScalarDomain of the
        same generation (a legacy one wants its calc_dndr) whose probing axis is an oblique line of sight of this one
        (orientation.rotated)."""
        from .orientation import rotated

        return rotated(self, angle_deg, about, **kw)

    def self_emission(self, wavelengths, toward="+", backlight=None):
        """The plasma's own light along the probing axis, emission with self-absorption: an emission.Emission with the
        intensity and optical-depth maps per wavelength.  Needs external_Te() and external_Z()."""
        from .emission import self_emission

        return self_emission(self, wavelengths, toward=toward, backlight=backlight)

    def table_emission(self, table, toward="+", backlight=None):
        """self_emission with the opacities of an utils.eos_opacity.OpacityTable (PROPACEOS tables) in place of the NRL
        coefficient: an emission.TableEmission, one band per band of the table.  Needs external_Te() and external_Z().  Not
        modelled: Z from the table's zf_table, group-integrated Planck functions, refraction, detector optics."""
        from .emission import table_emission

        return table_emission(self, table, toward=toward, backlight=backlight)

    def sightline_emission(self, view, wavelengths=None, table=None, step=None, max_steps=None):
        """What a sightlines.PinholeCamera, PointBacklighter or Chords sees of this domain: emission with self-absorption
        along lines that converge on a pinhole, diverge from a point backlighter, or are single chords at any angle -- a
        sightlines.SightlineEmission.  Exactly one of wavelengths (self_emission's node) and table (table_emission's).  Needs
        external_Te() and external_Z().  Not modelled: a finite pinhole or source, the cos^4 and solid-angle factors of a film's
        exposure, refraction, the detector's response, a table's own ionisation; one GPU."""
        from .sightlines import sightline_emission

        return sightline_emission(self, view, wavelengths=wavelengths, table=table, step=step, max_steps=max_steps)

    def sightline_spectra(self, view, wavelengths=None, photon_energies=None, table=None, step=None, max_steps=None):
        """The spectrum every line of a sightlines.Chords, PinholeCamera or PointBacklighter sees of this domain: sightline_emission
        at many frequencies (up to 16384) in one call, a GPU lane per frequency -- a sightlines.SightlineSpectra.  Exactly one of
        wavelengths [m], photon_energies [eV] (the NRL node, which holds only for hbar*omega <~ Te) and table (an
        utils.eos_opacity.SpectralOpacityTable: one frequency per group).  Needs external_Te() and external_Z().  Not modelled: a
        finite pinhole or source, the cos^4 and solid-angle factors of a film's exposure, refraction, the detector's response
        beyond SightlineSpectra.signal, a table's own ionisation; one GPU.  Spectral lines are sightline_lines."""
        from .sightlines import sightline_spectra

        return sightline_spectra(self, view, wavelengths=wavelengths, photon_energies=photon_energies, table=table, step=step,
                                 max_steps=max_steps)

    def sightline_lines(self, view, lines, wavelengths=None, photon_energies=None, continuum=False, step=None, max_steps=None):
        """The line spectrum every chord of a sightlines.Chords, PinholeCamera or PointBacklighter sees of this domain: the lines
        of an utils.eos_opacity.LineTable, Doppler-shifted by the flow (external_V; without it no shift) and broadened by the ion
        temperature (external_Ti; without it Ti = Te) sample by sample, optionally on sightline_spectra's NRL continuum -- a
        sightlines.LineSpectra, whose moments() give the flow velocity and Ti a spectrometer would infer.  Exactly one of
        wavelengths [m] and photon_energies [eV].  Needs external_Te() and external_Z().  Not modelled: Lorentzian, Stark and
        Voigt wings, Zeeman splitting, line blending through the cutoff at exp(-40), partial redistribution, refraction, the
        instrument function; one GPU."""
        from .sightlines import sightline_lines

        return sightline_lines(self, view, lines, wavelengths=wavelengths, photon_energies=photon_energies, continuum=continuum,
                               step=step, max_steps=max_steps)

    def sightline_voigt(self, view, lines, wavelengths=None, photon_energies=None, continuum=False, wing=None, step=None, max_steps=None):
        """sightline_lines with Voigt profiles: the lines of an utils.eos_opacity.VoigtLineTable, each with the Lorentzian (Stark,
        natural) half-width its table gives at the sample's temperature and ion density beside the thermal width of Ti -- a
        sightlines.LineSpectra, whose fwhm() gives the width an electron density is read from.  wing: terms further than that
        many thermal 1/e widths from a line's centre are dropped (None: never).  Everything else is sightline_lines'.  Not
        modelled: Zeeman splitting, asymmetric and shifted Stark profiles, ion dynamics, blending through wing, partial
        redistribution, refraction, the instrument function; one GPU."""
        from .sightlines import sightline_voigt

        return sightline_voigt(self, view, lines, wavelengths=wavelengths, photon_energies=photon_energies, continuum=continuum,
                               wing=wing, step=step, max_steps=max_steps)

    def sightline_zeeman(self, view, lines, wavelengths=None, photon_energies=None, continuum=False, wing=None, step=None, max_steps=None,
                         reference=None):
        """sightline_voigt in this domain's magnetic field (external_B): the lines of an utils.eos_opacity.ZeemanLineTable, each
        split by B at every sample into the pi and sigma components of its Zeeman pattern, and the Stokes parameters I, Q, U, V
        along every chord -- a sightlines.StokesSpectra, whose analysed() gives what a linear or circular analyser passes and
        b_parallel() the field along the chord a polarisation-resolved spectrometer would infer.  reference: the direction Q is
        measured from, (3,) or one per chord; None: a pixel view's up, for Chords the lab axis least aligned with each chord.
        Everything else is sightline_voigt's.  Not modelled: dichroism and magneto-optical (anomalous-dispersion) rotation in the
        absorption matrix (absorption acts equally on all four parameters), Faraday rotation of the continuum, the Paschen-Back
        regime, hyperfine structure, and what sightline_voigt does not model; one GPU."""
        from .sightlines import sightline_zeeman

        return sightline_zeeman(self, view, lines, wavelengths=wavelengths, photon_energies=photon_energies, continuum=continuum,
                                wing=wing, step=step, max_steps=max_steps, reference=reference)

    def sightline_stokes(self, view, lines, wavelengths=None, photon_energies=None, continuum=False, wing=None, step=None, max_steps=None,
                         reference=None, polarisation=None, faraday=False):
        """sightline_zeeman with the full polarised transfer equation: the lines' absorption is dichroic (it takes the pi and
        sigma components out of a backlight's Q, U, V and lets a thick line depolarise towards its source function), the plane of
        polarisation turns inside the lines (magneto-optical rotation) and, with faraday=True, in the continuum (Faraday
        rotation, kF ne B.n^ / omega^2 per metre) -- a sightlines.StokesSpectra.  polarisation: (q, u, v) of the view's backlight
        as fractions of its intensity, q^2 + u^2 + v^2 <= 1; None: unpolarised.  Everything else is sightline_zeeman's; a table
        without absorption, faraday=False and polarisation=None give its bits.  Not modelled: the Paschen-Back regime, hyperfine
        structure, cyclotron dichroism of the continuum, scattering polarisation, the Hanle effect, and what sightline_voigt does
        not model; one GPU."""
        from .sightlines import sightline_stokes

        return sightline_stokes(self, view, lines, wavelengths=wavelengths, photon_energies=photon_energies, continuum=continuum,
                                wing=wing, step=step, max_steps=max_steps, reference=reference, polarisation=polarisation,
                                faraday=faraday)

    def export_scalar_field(self, property: str = "ne", fname: str = None):
        """Save n_e as <fname>.vti + <fname>.pvti (full_solver.py:442-512, domain.py:505-579), written without pyvista."""
        from .utils.handle_filetypes import export_scalar_field

        export_scalar_field(self, property, fname)
