"""Equation-of-state and opacity tables (src/utils/eos_opacity.py of the reference): read_propaceos, the reference's reader of
PROPACEOS text tables, and OpacityTable, what the tabulated self-emission consumes (emission.table_emission,
engine.emission_table -> sr_field_emission_table; no reference counterpart).

    d = read_propaceos("carbon.prp", need_emiss_opacity=True, need_abs_opacity=True)
    table = OpacityTable.from_propaceos(d, A=12.011)
    em = domain.table_emission(table)

LineTable holds spectral lines on the same kind of lattice, from arrays: what sightlines.sightline_lines consumes
(engine.sightline_lines -> sr_field_sightline_lines; no reference counterpart); VoigtLineTable adds each line's Lorentzian width for
sightlines.sightline_voigt (engine.sightline_voigt -> sr_field_sightline_voigt), ZeemanLineTable each line's Zeeman pattern for
sightlines.sightline_zeeman (engine.sightline_zeeman -> sr_field_sightline_zeeman).
"""
from __future__ import annotations

import numpy as np

_HEADER_LINES = 38
# (flag, key) in FILE order: each table follows one title line, so a table is found only by reading every table before it
_TABLES = (("need_zf_table", "zf_table"), ("need_ross_opacity", "ross_opacity"), ("need_emiss_opacity", "emiss_opacity"),
           ("need_abs_opacity", "abs_opacity"), ("need_en_table", "en_table"), ("need_eion", "eion_table"),
           ("need_eele", "eele_table"), ("need_pion", "pion_table"), ("need_pele", "pele_table"))
_KEYS = ("temperatures", "densities", "rad_groups") + tuple(key for _, key in _TABLES)


class _Lines:
    """The file's lines one after another: skip() as next() on a file does (StopIteration at the end), line() as readline()
    (an empty string at the end)."""

    def __init__(self, fh):
        self._it = iter(fh)

    def skip(self, n=1):
        for _ in range(n):
            next(self._it)

    def line(self):
        return next(self._it, "")

    def values(self, n_lines):
        out = []
        for _ in range(n_lines):
            out.extend(float(v) for v in self.line().strip().split())
        return out


def read_propaceos(file_name, need_zf_table=False, need_en_table=False, need_eion=False, need_eele=False, need_pion=False,
                   need_pele=False, need_ross_opacity=False, need_emiss_opacity=False, need_abs_opacity=False):
    """The reference's read_propaceos: a dict with "temperatures" [eV], "densities" [ion number density, cm^-3], "rad_groups"
    (the photon-energy group edges [eV]) and, for every need_* flag set, the (n_temperature, n_density) table -- "zf_table"
    (mean ionisation), "ross_opacity", "emiss_opacity", "abs_opacity" [cm^2/g], "en_table", "eion_table", "eele_table" [J/g],
    "pion_table", "pele_table" [dyne/cm^2]; a table that was not asked for is None.

    The file is read as the reference reads it, quirks included:
    * 38 header lines are skipped; then a count line and the temperature grid, a count line and the density grid.  A grid of n
      values is read as n // 10 lines (of ten values): a count that is no multiple of ten loses its last, short line -- the grid
      comes back short and every later block is read from the wrong line (usually a ValueError from a title line or from a row
      of the wrong length), exactly as in the reference.
    * the same two grids again and 5 more lines are skipped (n_T // 10 + n_D // 10 + 2 + 5 lines), then the group count, one
      skipped line and ngroups // 10 + 1 lines of group edges.
    * the tables follow in FILE order -- zf, Rosseland, emission, absorption, en, eion, eele, pion, pele -- each after ONE skipped
      title line, n_D // 10 lines per temperature.  A table is only skipped over when it is asked for: asking for a later table
      without every earlier one reads an earlier table's block under the later name (or fails on its rows).
    A count <= 0 raises ValueError; a file that ends early raises StopIteration or ValueError, whichever the reference's
    next() / readline() at that place gives."""
    wanted = dict(need_zf_table=need_zf_table, need_en_table=need_en_table, need_eion=need_eion, need_eele=need_eele,
                  need_pion=need_pion, need_pele=need_pele, need_ross_opacity=need_ross_opacity,
                  need_emiss_opacity=need_emiss_opacity, need_abs_opacity=need_abs_opacity)
    data = dict.fromkeys(_KEYS)
    with open(file_name, "r") as fh:
        src = _Lines(fh)
        src.skip(_HEADER_LINES)
        n_t = int(src.line().strip())
        if n_t <= 0:
            raise ValueError("No temperature grid found in the PROPACEOS file.")
        temperatures = src.values(n_t // 10)
        n_d = int(src.line().strip())
        if n_d <= 0:
            raise ValueError("No density grid found in the PROPACEOS file.")
        densities = src.values(n_d // 10)
        data["temperatures"] = np.array(temperatures)
        data["densities"] = np.array(densities)
        src.skip(n_t // 10 + n_d // 10 + 2 + 5)
        n_groups = int(src.line().strip())
        src.skip()
        data["rad_groups"] = np.array(src.values(n_groups // 10 + 1))
        for flag, key in _TABLES:
            if not wanted[flag]:
                continue
            if key == "en_table":
                src.line()  # the reference skips this one title with readline(): no StopIteration at the end of the file
            else:
                src.skip()
            table = np.zeros((n_t, n_d))
            for t in range(n_t):
                table[t, :] = src.values(n_d // 10)
            data[key] = table
    return data


MAX_LATTICE = 512  # sr_field_emission_table: 2..512 nodes per lattice axis
ATOMIC_MASS_G = 1.66053906660e-24  # u [g]


class OpacityTable:
    """Absorption (and emission) opacities on a temperature x ion-density lattice, for up to 4 bands: what
    sr_field_emission_table interpolates (bilinearly in log T, log n_i, on the logarithm of the opacity; outside the lattice the
    edge value holds).

    temperatures [eV] and densities [ion number density, cm^-3]: strictly increasing, finite, positive, 2 to 512 entries each.
    absorption, emission [cm^2/g]: (n_band, nT, nD) (a 2-D array is one band), finite and positive; emission=None is LTE
    (emission opacity = absorption opacity).  photon_energy [eV] per band: where the Planck function is taken.  edges: optional
    (n_band, 2) band edges [eV].  A: the atomic mass [u] that turns n_i into a mass density.  ValueError names the offending member."""

    def __init__(self, temperatures, densities, absorption, photon_energy, A, emission=None, edges=None):
        from .._ffi import MAX_BANDS

        self.temperatures = np.array(temperatures, np.float64, ndmin=1)
        self.densities = np.array(densities, np.float64, ndmin=1)
        for name in ("temperatures", "densities"):
            a = getattr(self, name)
            if a.ndim != 1 or not 2 <= len(a) <= MAX_LATTICE:
                raise ValueError(f"{name} must hold 2 to {MAX_LATTICE} values in one dimension, got shape {a.shape}")
            if not np.all(np.isfinite(a) & (a > 0)):
                raise ValueError(f"{name} must be finite and positive")
            if not np.all(a[1:] > a[:-1]):
                raise ValueError(f"{name} must be strictly increasing")
        lattice = (len(self.temperatures), len(self.densities))
        self.absorption = self._opacity("absorption", absorption, lattice)
        n_band = len(self.absorption)
        if not 1 <= n_band <= MAX_BANDS:
            raise ValueError(f"absorption must hold 1 to {MAX_BANDS} bands, got {n_band}")
        self.emission = None if emission is None else self._opacity("emission", emission, lattice)
        if self.emission is not None and self.emission.shape != self.absorption.shape:
            raise ValueError(f"emission has shape {self.emission.shape}, absorption {self.absorption.shape}")
        self.photon_energy = np.array(photon_energy, np.float64, ndmin=1)
        if self.photon_energy.shape != (n_band,) or not np.all(np.isfinite(self.photon_energy) & (self.photon_energy > 0)):
            raise ValueError(f"photon_energy must be {n_band} finite positive value(s), got {self.photon_energy.tolist()}")
        self.edges = None
        if edges is not None:
            self.edges = np.array(edges, np.float64, ndmin=2)
            if self.edges.shape != (n_band, 2) or not np.all(np.isfinite(self.edges) & (self.edges >= 0)) or not np.all(
                    self.edges[:, 1] > self.edges[:, 0]):
                raise ValueError(f"edges must be ({n_band}, 2), finite, non-negative and increasing per band, got {self.edges.tolist()}")
        self.A = float(A)
        if not (np.isfinite(self.A) and self.A > 0):
            raise ValueError(f"A must be a finite positive atomic mass [u], got {A!r}")

    @staticmethod
    def _opacity(name, values, lattice):
        a = np.array(values, np.float64)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1:] != lattice:
            raise ValueError(f"{name} has shape {a.shape}, the lattice gives (n_band, {lattice[0]}, {lattice[1]})")
        if not np.all(np.isfinite(a) & (a > 0)):
            raise ValueError(f"{name} must be finite and positive")
        return np.ascontiguousarray(a)

    @property
    def n_band(self):
        return len(self.absorption)

    @property
    def m_ion(self):
        """The ion mass [g]."""
        return self.A * ATOMIC_MASS_G

    def logs(self):
        """(LT, LD, LA, LE): the float64 logarithms sr_field_emission_table takes; LE is None for LTE."""
        return (np.log(self.temperatures), np.log(self.densities), np.ascontiguousarray(np.log(self.absorption)),
                None if self.emission is None else np.ascontiguousarray(np.log(self.emission)))

    @classmethod
    def from_propaceos(cls, data, A, photon_energy=None):
        """A one-band table from read_propaceos' dict (the reader yields group MEANS only; multi-band tables come from arrays):
        absorption from "abs_opacity", emission from "emiss_opacity" when it was read, edges = the first and the last entry of
        "rad_groups", photon_energy = their geometric mean unless given."""
        if data.get("abs_opacity") is None:
            raise ValueError("abs_opacity is missing: call read_propaceos(..., need_abs_opacity=True)")
        groups = np.asarray(data["rad_groups"], np.float64)
        if groups.ndim != 1 or len(groups) < 2:
            raise ValueError(f"rad_groups must hold at least 2 edges, got shape {groups.shape}")
        edges = np.array([[groups[0], groups[-1]]])
        if photon_energy is None:
            photon_energy = np.sqrt(groups[0] * groups[-1])
        return cls(data["temperatures"], data["densities"], data["abs_opacity"], photon_energy, A,
                   emission=data.get("emiss_opacity"), edges=edges)


class SpectralOpacityTable(OpacityTable):
    """An OpacityTable of many photon-energy groups (1 to _ffi.MAX_FREQS = 16384 bands): what sr_field_sightline_spectra
    interpolates, one group per frequency of a spectrum (sightlines.sightline_spectra, engine.sightline_spectra).  The members,
    their units and their conditions are OpacityTable's, checked by OpacityTable itself four bands at a time, so a ValueError names
    the offending member in its words; edges, when given, must be (n_band, 2).  The entries that take at most 4 bands
    (table_emission, sightline_emission) do not take this table: bands(indices) gives them an ordinary OpacityTable of up to 4
    chosen groups.  read_propaceos yields group MEANS only, as the reference's reader does: multigroup tables come from arrays."""

    def __init__(self, temperatures, densities, absorption, photon_energy, A, emission=None, edges=None):
        from .._ffi import MAX_BANDS, MAX_FREQS

        absorption = np.array(absorption, np.float64)
        if absorption.ndim == 2:
            absorption = absorption[None]
        if absorption.ndim != 3:
            raise ValueError(f"absorption has shape {absorption.shape}, a table is (n_band, nT, nD)")
        n_band = len(absorption)
        if not 1 <= n_band <= MAX_FREQS:
            raise ValueError(f"absorption must hold 1 to {MAX_FREQS} bands, got {n_band}")
        photon_energy = np.array(photon_energy, np.float64, ndmin=1)
        if photon_energy.shape != (n_band,):
            raise ValueError(f"photon_energy must be {n_band} finite positive value(s), got shape {photon_energy.shape}")
        if emission is not None:
            emission = np.array(emission, np.float64)
            emission = emission[None] if emission.ndim == 2 else emission
            if emission.shape != absorption.shape:
                raise ValueError(f"emission has shape {emission.shape}, absorption {absorption.shape}")
        if edges is not None:
            edges = np.array(edges, np.float64)
            if edges.shape != (n_band, 2):
                raise ValueError(f"edges must be ({n_band}, 2), got shape {edges.shape}")
        parts = [OpacityTable(temperatures, densities, absorption[k:k + MAX_BANDS], photon_energy[k:k + MAX_BANDS], A,
                              emission=None if emission is None else emission[k:k + MAX_BANDS],
                              edges=None if edges is None else edges[k:k + MAX_BANDS]) for k in range(0, n_band, MAX_BANDS)]
        self.temperatures, self.densities, self.A = parts[0].temperatures, parts[0].densities, parts[0].A
        self.absorption = np.ascontiguousarray(absorption)
        self.emission = None if emission is None else np.ascontiguousarray(emission)
        self.photon_energy, self.edges = photon_energy, edges

    def bands(self, indices):
        """An ordinary OpacityTable of the chosen groups (up to 4 indices, or a slice), for the entries that take at most 4 bands."""
        idx = np.arange(self.n_band)[indices].ravel()
        return OpacityTable(self.temperatures, self.densities, self.absorption[idx], self.photon_energy[idx], self.A,
                            emission=None if self.emission is None else self.emission[idx],
                            edges=None if self.edges is None else self.edges[idx])

    def packed(self):
        """(LT, LD, LA, LE) with the groups innermost -- LA and LE (nT, nD, n_band), C order, the transposes of logs()' -- as
        sr_field_sightline_spectra lays the table out for its kernel; LE is None for LTE."""
        LT, LD, LA, LE = self.logs()
        return LT, LD, np.ascontiguousarray(LA.transpose(1, 2, 0)), None if LE is None else np.ascontiguousarray(LE.transpose(1, 2, 0))


MAX_LINES = 32  # sr_field_sightline_lines: 1..32 spectral lines
_HBAR, _E_CHARGE, _C = 6.62607015e-34 / (2 * np.pi), 1.602176634e-19, 299792458.0


class LineTable:
    """Spectral lines on a temperature x ion-density lattice: what sr_field_sightline_lines interpolates
    (sightlines.sightline_lines, engine.sightline_lines), from arrays.

    temperatures [eV] and ion_densities [cm^-3]: strictly increasing, finite, positive, 2 to 512 entries each (OpacityTable's
    lattice).  emissivity: (n_line, nT, nD) (a 2-D array is one line), the frequency-integrated emission coefficient of each line
    [W m^-3 sr^-1], finite and positive, 1 to 32 lines.  Exactly one of wavelengths [m] and photon_energy [eV], one per line: the
    line's rest position (omega0 [rad/s] keeps it).  mass_number: the emitting ion's mass number, a number or one per line (the
    thermal width is sqrt(2 e Ti / (A m_p)) omega0 / c).  absorption: (n_line, nT, nD), the frequency-integrated absorption
    coefficient [m^-1 rad s^-1], or None: optically thin lines.  ValueError names the offending member."""

    def __init__(self, temperatures, ion_densities, emissivity, wavelengths=None, photon_energy=None, mass_number=None,
                 absorption=None):
        lattice = OpacityTable(temperatures, ion_densities, np.ones((1, np.size(temperatures), np.size(ion_densities))), 1.0, 1.0)
        self.temperatures, self.ion_densities = lattice.temperatures, lattice.densities
        shape = (len(self.temperatures), len(self.ion_densities))
        self.emissivity = OpacityTable._opacity("emissivity", emissivity, shape)
        n_line = len(self.emissivity)
        if not 1 <= n_line <= MAX_LINES:
            raise ValueError(f"emissivity must hold 1 to {MAX_LINES} lines, got {n_line}")
        self.absorption = None if absorption is None else OpacityTable._opacity("absorption", absorption, shape)
        if self.absorption is not None and self.absorption.shape != self.emissivity.shape:
            raise ValueError(f"absorption has shape {self.absorption.shape}, emissivity {self.emissivity.shape}")
        if (wavelengths is None) == (photon_energy is None):
            raise ValueError("exactly one of wavelengths [m] and photon_energy [eV] must be given")
        name = "wavelengths" if photon_energy is None else "photon_energy"
        pos = np.array(wavelengths if photon_energy is None else photon_energy, np.float64, ndmin=1)
        if pos.shape != (n_line,) or not np.all(np.isfinite(pos) & (pos > 0)):
            raise ValueError(f"{name} must be {n_line} finite positive value(s), got {pos.tolist()}")
        self.omega0 = 2 * np.pi * _C / pos if photon_energy is None else pos * _E_CHARGE / _HBAR
        if mass_number is None:
            raise ValueError("mass_number must be given: the emitting ion's mass number, a number or one per line")
        A = np.array(mass_number, np.float64, ndmin=1)
        if A.shape not in ((1,), (n_line,)) or not np.all(np.isfinite(A) & (A > 0)):
            raise ValueError(f"mass_number must be a finite positive number or {n_line} of them, got {A.tolist()}")
        self.mass_number = np.array(np.broadcast_to(A, (n_line,)))

    @property
    def n_line(self):
        return len(self.emissivity)

    @property
    def wavelengths(self):
        """The lines' rest wavelengths [m]."""
        return 2 * np.pi * _C / self.omega0

    @property
    def photon_energy(self):
        """The lines' rest photon energies [eV]."""
        return _HBAR * self.omega0 / _E_CHARGE

    def thermal_width(self, Ti):
        """The 1/e half-width in angular frequency of every line at the ion temperature Ti [eV]: omega0 sqrt(2 e Ti / (A m_p)) / c."""
        return self.omega0 * np.sqrt(2 * _E_CHARGE * float(Ti) / (self.mass_number * 1.67262192369e-27)) / _C

    def planck(self):
        """B_omega(omega0, T) on the lattice's temperatures, (n_line, nT) [W m^-2 sr^-1 (rad/s)^-1]."""
        w = self.omega0[:, None]
        return _HBAR * w ** 3 / (4 * np.pi ** 3 * _C ** 2) / np.expm1(_HBAR * w / _E_CHARGE / self.temperatures[None, :])

    def with_lte_absorption(self):
        """This table with absorption = emissivity / B_omega(omega0, T) (Kirchhoff: ln K = ln J - ln B on the lattice), so that
        every line's source function is Planck's and a thick line saturates at it."""
        out = LineTable.__new__(LineTable)
        out.__dict__.update(self.__dict__)
        out.absorption = np.ascontiguousarray(self.emissivity / self.planck()[:, :, None])
        if not np.all(np.isfinite(out.absorption) & (out.absorption > 0)):
            raise ValueError("the Planck function under- or overflows on this lattice: no LTE absorption")
        return out


class VoigtLineTable(LineTable):
    """A LineTable whose lines also have a Lorentzian width on the lattice: what sr_field_sightline_voigt interpolates
    (sightlines.sightline_voigt, engine.sightline_voigt).

    LineTable's arguments, and lorentz_width: (n_line, nT, nD) (a 2-D array is one line), each line's Lorentzian half width at half
    maximum in angular frequency [rad/s] -- Stark and natural broadening together -- finite and positive.  ValueError names the
    offending member.  from_lines() adds widths to a LineTable, power_law() makes them from the usual scaling of a Stark width with
    the electron density."""

    def __init__(self, temperatures, ion_densities, emissivity, wavelengths=None, photon_energy=None, mass_number=None,
                 absorption=None, lorentz_width=None):
        super().__init__(temperatures, ion_densities, emissivity, wavelengths=wavelengths, photon_energy=photon_energy,
                         mass_number=mass_number, absorption=absorption)
        if lorentz_width is None:
            raise ValueError("lorentz_width must be given: the Lorentzian HWHM [rad/s] of every line on the lattice")
        self.lorentz_width = OpacityTable._opacity("lorentz_width", lorentz_width, (len(self.temperatures), len(self.ion_densities)))
        if self.lorentz_width.shape != self.emissivity.shape:
            raise ValueError(f"lorentz_width has shape {self.lorentz_width.shape}, emissivity {self.emissivity.shape}")

    @classmethod
    def from_lines(cls, table, lorentz_width):
        """`table` (a LineTable) with these Lorentzian widths."""
        out = cls(table.temperatures, table.ion_densities, table.emissivity, wavelengths=table.wavelengths, mass_number=table.mass_number,
                  absorption=table.absorption, lorentz_width=lorentz_width)
        out.omega0 = np.array(table.omega0, np.float64)  # the bits of the table it came from, not those of 2 pi c / (2 pi c / omega0)
        return out

    @classmethod
    def power_law(cls, table, width_ref, ne_ref, Te_ref=None, ne_exponent=1.0, Te_exponent=0.0, zbar=1.0, natural=0.0):
        """`table` with gamma = natural + width_ref * (zbar * ni / ne_ref)^ne_exponent * (Te / Te_ref)^Te_exponent on its lattice:
        width_ref [rad/s] is the Stark HWHM at the electron density ne_ref [m^-3] and the temperature Te_ref [eV] (None: no
        temperature dependence), zbar the ion charge that turns the lattice's ion density (converted from cm^-3) into an electron
        density, natural [rad/s] a density-independent half-width.  Each argument is a number or one value per line.  With
        natural = 0 ln gamma is linear in ln Te and ln ni, so the kernel's bilinear interpolation in logs reproduces the law at
        every (Te, ni), up to rounding."""
        n_line = table.n_line

        def per_line(name, v, positive=True):
            a = np.array(v, np.float64, ndmin=1)
            if a.shape not in ((1,), (n_line,)) or not np.all(np.isfinite(a)) or (positive and not np.all(a > 0)):
                raise ValueError(f"{name} must be a finite{' positive' if positive else ''} number or {n_line} of them, got {a.tolist()}")
            return np.broadcast_to(a, (n_line,))[:, None, None]

        w, n0 = per_line("width_ref", width_ref), per_line("ne_ref", ne_ref)
        p, q = per_line("ne_exponent", ne_exponent, False), per_line("Te_exponent", Te_exponent, False)
        zb, nat = per_line("zbar", zbar), per_line("natural", natural, False)
        if np.any(nat < 0):
            raise ValueError(f"natural must not be negative, got {np.ravel(nat).tolist()}")
        T0 = per_line("Te_ref", 1.0 if Te_ref is None else Te_ref)
        if Te_ref is None and np.any(q != 0):
            raise ValueError("Te_ref must be given where Te_exponent is not 0")
        ne = zb * (table.ion_densities[None, None, :] * 1e6)
        ln = np.log(w) + p * np.log(ne / n0) + q * np.log(table.temperatures[None, :, None] / T0)
        return cls.from_lines(table, nat + np.exp(ln))

    def with_lte_absorption(self):
        """LineTable.with_lte_absorption(), with the widths kept."""
        lte = LineTable.with_lte_absorption(self)
        out = VoigtLineTable.__new__(VoigtLineTable)
        out.__dict__.update(lte.__dict__)
        return out

    def voigt_fwhm(self, Ti, Te, ni):
        """An ESTIMATE of every line's full width at half maximum [rad/s] at the ion temperature Ti [eV], the temperature Te [eV]
        and the ion density ni [cm^-3]: Olivero and Longbothum's fit, 0.5346 fL + sqrt(0.2166 fL^2 + fG^2), with the Lorentzian
        FWHM fL = 2 gamma (gamma interpolated as the kernel does, bilinearly in logs, the edge value outside the lattice) and the
        Gaussian FWHM fG = 2 sqrt(ln 2) thermal_width(Ti).  The fit is good to about 0.02 % of the true Voigt width."""
        lt, ld = np.log(self.temperatures), np.log(self.ion_densities)

        def locate(L, v):
            i = int(np.clip(np.searchsorted(L, v, side="right") - 1, 0, len(L) - 2))
            return i, float(np.clip((v - L[i]) / (L[i + 1] - L[i]), 0.0, 1.0))

        (i, ft), (j, fd) = locate(lt, np.log(float(Te))), locate(ld, np.log(float(ni)))
        G = np.log(self.lorentz_width)
        lo, hi = G[:, i, j] + fd * (G[:, i, j + 1] - G[:, i, j]), G[:, i + 1, j] + fd * (G[:, i + 1, j + 1] - G[:, i + 1, j])
        fL = 2.0 * np.exp(lo + ft * (hi - lo))
        fG = 2.0 * np.sqrt(np.log(2.0)) * self.thermal_width(Ti)
        return 0.5346 * fL + np.sqrt(0.2166 * fL ** 2 + fG ** 2)


MAX_ZEEMAN = 24  # SR_MAX_ZEEMAN: components of one line (J = 7/2 <-> 7/2 has 22)
_M_E = 9.1093837015e-31
LARMOR = _E_CHARGE / (2.0 * _M_E)  # kL [rad/s/T]: the Larmor angular frequency per tesla, as sr_field_sightline_zeeman forms it


def normal_triplet():
    """The normal Zeeman triplet: (q, g, s) = (-1, -1, 1), (0, 0, 1), (+1, +1, 1)."""
    return np.array([[-1.0, -1.0, 1.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]])


def lande_pattern(J_upper, g_upper, J_lower, g_lower):
    """The anomalous Zeeman pattern of J_upper -> J_lower in LS coupling and a weak field, (n, 3) rows (q, g, s): for every allowed
    m_u -> m_l, q = m_u - m_l, the shift g = g_u m_u - g_l m_l in Larmor units, the strength the squared 3j symbol
    (J_u 1 J_l; -m_u q m_l)^2 by its closed forms for J_u - J_l = 0, +1, -1, normalised to 1 over each q group.  Components of one
    group whose shifts are the same float64 are merged (g_u = g_l: g = g_u q for all of them, the normal triplet scaled by g_u);
    rows are ordered by q, then by g."""
    Ju, Jl = float(J_upper), float(J_lower)
    for name, J in (("J_upper", Ju), ("J_lower", Jl)):
        if not (np.isfinite(J) and J >= 0 and 2 * J == np.rint(2 * J)):
            raise ValueError(f"{name} must be a non-negative integer or half-integer, got {J!r}")
    dJ = Ju - Jl
    if dJ not in (-1.0, 0.0, 1.0) or (Ju == 0 and Jl == 0) or (2 * Ju) % 2 != (2 * Jl) % 2:
        raise ValueError(f"J_upper -> J_lower = {Ju} -> {Jl} is not an electric-dipole transition (J changes by 0 or 1, not 0 -> 0)")
    gu, gl = float(g_upper), float(g_lower)
    if not (np.isfinite(gu) and np.isfinite(gl)):
        raise ValueError(f"g_upper and g_lower must be finite, got {g_upper!r} and {g_lower!r}")
    J = Jl
    rows = {}
    for q in (-1, 0, 1):
        for m in np.arange(-Jl, Jl + 0.5):  # m: the lower level's
            mu = m + q
            if abs(mu) > Ju:
                continue
            if dJ == 0:
                s = m * m if q == 0 else 0.5 * (J - q * m) * (J + q * m + 1)
            elif dJ == 1:
                s = (J + 1) ** 2 - m * m if q == 0 else 0.5 * (J + q * m + 1) * (J + q * m + 2)
            else:
                s = J * J - m * m if q == 0 else 0.5 * (J - q * m) * (J - q * m - 1)
            if s > 0:
                key = (float(q), gu * q if gu == gl else gu * mu - gl * m)  # equal factors: g (m_u - m_l), without rounding
                rows[key] = rows.get(key, 0.0) + s
    out = np.array([[q, g, s] for (q, g), s in sorted(rows.items())])
    for q in (-1.0, 0.0, 1.0):
        sel = out[:, 0] == q
        if sel.any():
            out[sel, 2] /= out[sel, 2].sum()
    return out


class ZeemanLineTable(VoigtLineTable):
    """A line table whose lines also have a Zeeman pattern: what sr_field_sightline_zeeman takes (sightlines.sightline_zeeman,
    engine.sightline_zeeman).

    VoigtLineTable's arguments -- but lorentz_width may be None: Gaussian components -- and patterns: one (n, 3) array of rows
    (q, g, s) per line (a single 2-D array serves every line), 1 to 24 rows: q in {-1, 0, +1} is m_upper - m_lower, g the
    component's shift in units of the Larmor frequency e B / (2 m_e), s > 0 its strength; the strengths of every q group that is
    present sum to 1 within 1e-9.  ValueError names the offending member.  from_lines() adds patterns to a LineTable or a
    VoigtLineTable, from_lande() makes them from the levels' J and Lande factors."""

    def __init__(self, temperatures, ion_densities, emissivity, wavelengths=None, photon_energy=None, mass_number=None,
                 absorption=None, lorentz_width=None, patterns=None):
        LineTable.__init__(self, temperatures, ion_densities, emissivity, wavelengths=wavelengths, photon_energy=photon_energy,
                           mass_number=mass_number, absorption=absorption)
        self.lorentz_width = None
        if lorentz_width is not None:
            self.lorentz_width = OpacityTable._opacity("lorentz_width", lorentz_width, (len(self.temperatures), len(self.ion_densities)))
            if self.lorentz_width.shape != self.emissivity.shape:
                raise ValueError(f"lorentz_width has shape {self.lorentz_width.shape}, emissivity {self.emissivity.shape}")
        self.patterns = self._patterns(patterns, self.n_line)

    @staticmethod
    def _patterns(patterns, n_line):
        if patterns is None:
            raise ValueError("patterns must be given: the Zeeman components (q, g, s) of every line")
        if isinstance(patterns, np.ndarray) and patterns.ndim == 2:
            patterns = [patterns] * n_line
        patterns = [np.array(p, np.float64, ndmin=2) for p in patterns]
        if len(patterns) != n_line:
            raise ValueError(f"patterns must hold one array per line ({n_line}), got {len(patterns)}")
        for l, p in enumerate(patterns):
            if p.ndim != 2 or p.shape[1] != 3 or not 1 <= len(p) <= MAX_ZEEMAN:
                raise ValueError(f"patterns[{l}] must be (n, 3) with n in 1..{MAX_ZEEMAN}, got shape {p.shape}")
            if not np.all(np.isin(p[:, 0], (-1.0, 0.0, 1.0))):
                raise ValueError(f"patterns[{l}]: q must be -1, 0 or +1, got {p[:, 0].tolist()}")
            if not np.all(np.isfinite(p[:, 1])):
                raise ValueError(f"patterns[{l}]: g must be finite, got {p[:, 1].tolist()}")
            if not np.all(np.isfinite(p[:, 2]) & (p[:, 2] > 0)):
                raise ValueError(f"patterns[{l}]: s must be finite and positive, got {p[:, 2].tolist()}")
            for q in (-1.0, 0.0, 1.0):
                s = p[p[:, 0] == q, 2]
                if len(s) and abs(float(np.sum(s)) - 1.0) > 1e-9:
                    raise ValueError(f"patterns[{l}]: the strengths of the q = {q:+.0f} group sum to {float(np.sum(s))!r}, not 1")
        return patterns

    @classmethod
    def from_lines(cls, table, patterns):
        """`table` (a LineTable or a VoigtLineTable, whose widths are kept) with these patterns."""
        out = cls(table.temperatures, table.ion_densities, table.emissivity, wavelengths=table.wavelengths, mass_number=table.mass_number,
                  absorption=table.absorption, lorentz_width=getattr(table, "lorentz_width", None), patterns=patterns)
        out.omega0 = np.array(table.omega0, np.float64)  # the bits of the table it came from
        return out

    @classmethod
    def from_lande(cls, table, J_upper, g_upper, J_lower, g_lower):
        """`table` with the anomalous pattern lande_pattern() gives each line; every argument is a number or one value per line."""
        n = table.n_line
        args = [np.broadcast_to(np.array(a, np.float64, ndmin=1), (n,)) if np.size(a) in (1, n) else None
                for a in (J_upper, g_upper, J_lower, g_lower)]
        if any(a is None for a in args):
            raise ValueError(f"J_upper, g_upper, J_lower and g_lower must each be a number or {n} of them")
        return cls.from_lines(table, [lande_pattern(*(a[l] for a in args)) for l in range(n)])

    normal_triplet = staticmethod(normal_triplet)

    @property
    def g_eff(self):
        """Per line, the strength-weighted mean shift of the q = +1 group in Larmor units: the effective Lande factor, which for an
        LS pattern is (g_u + g_l)/2 + (g_u - g_l)(J_u(J_u + 1) - J_l(J_l + 1))/4.  NaN for a line without a q = +1 component."""
        out = np.full(self.n_line, np.nan)
        for l, p in enumerate(self.patterns):
            sel = p[:, 0] == 1.0
            if sel.any():
                out[l] = float(np.sum(p[sel, 1] * p[sel, 2]) / np.sum(p[sel, 2]))
        return out

    def packed_patterns(self):
        """(n_comp (n_line) int32, comp (sum n_comp, 3) float64) as sr_zeeman_table takes them."""
        return (np.array([len(p) for p in self.patterns], np.int32), np.ascontiguousarray(np.concatenate(self.patterns, axis=0)))

    def with_lte_absorption(self):
        """LineTable.with_lte_absorption(), with the widths and the patterns kept."""
        lte = LineTable.with_lte_absorption(self)
        out = ZeemanLineTable.__new__(ZeemanLineTable)
        out.__dict__.update(lte.__dict__)
        return out
