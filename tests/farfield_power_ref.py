"""Yardsticks of the far-field back end (csrc/farfield_project.hip project_point, csrc/farfield_sums.hip
accumulate_kernel, accumulate_finish_kernel) for tests/farfield_power_cases.py: the projection of the four radiation vectors onto the
two amplitudes and the power P, ELEMENTWISE - so that it serves a pair list as well as a tensor grid - and the sums
of P over a source sweep.  NumPy and math only, float64, in the reference's order of operations
(oracle/farfield_oracle.py project, nearfield_farfield.py:153-189): test_farfield_power_cases.py holds
project_points equal to the oracle bit for bit on a tensor grid.  No test is collected from here."""
import math
from math import pi

import numpy as np


def _uz(ux, uy):
    """the reference's float64 `1 - ux**2 - uy**2`, NaN where it is negative, then its root.  That expression - two
    squares rounded on their own, subtracted one after the other - is the contract, not the exact value: at
    (0.28, 0.96) it is exactly 0, at (0.6, 0.8) it is -1.1e-16 and the direction is NaN."""
    uz = 1 - ux ** 2 - uy ** 2
    uz = np.where(uz < 0, np.nan, uz)
    return uz ** 0.5


def _mag(*terms):
    """sum of the magnitudes of complex terms, per component: .real bounds the real parts' sum, .imag the imaginary"""
    return sum(np.abs(t.real) for t in terms) + 1j * sum(np.abs(t.imag) for t in terms)


def project_points(Nx, Ny, Lx, Ly, ux, uy, wavelength, n_glass, Z0):
    """-> P, a_theta, a_phi, mag_theta, mag_phi for directions (ux, uy) of the vectors' shape (a pair list as it is,
    a tensor grid through meshgrid(indexing='ij')).  farfield_oracle.project restated elementwise: the +1e-9 and
    +1e-5 regularisers, the (0, 0) rule (both cosines zero, of either sign: the vectors themselves) and the NaN rule.
    mag_*: complex, the sums of |Re| and of |Im| of the four terms each amplitude is added up from - what a rounding
    error of the amplitude is measured against."""
    Nx, Ny, Lx, Ly = (np.asarray(v, dtype=complex) for v in (Nx, Ny, Lx, Ly))
    ux = np.asarray(ux, dtype=float)
    uy = np.asarray(uy, dtype=float)
    assert ux.shape == uy.shape == Nx.shape == Ny.shape == Lx.shape == Ly.shape
    with np.errstate(invalid='ignore'):
        uz = _uz(ux, uy)
        sintheta = (ux ** 2 + uy ** 2) ** 0.5
        nth = (Nx * ux * uz / (sintheta + 1e-9), Ny * uy * uz / (sintheta + 1e-9))
        nph = (-Nx * uy / (sintheta + 1e-9), Ny * ux / (sintheta + 1e-9))
        lth = (Lx * ux * uz / (sintheta + 1e-9), Ly * uy * uz / (sintheta + 1e-9))
        lph = (-Lx * uy / (sintheta + 1e-9), Ly * ux / (sintheta + 1e-9))
        Nth, Nph, Lth, Lph = nth[0] + nth[1], nph[0] + nph[1], lth[0] + lth[1], lph[0] + lph[1]
        zero = (ux == 0) & (uy == 0)
        Nth, Nph = np.where(zero, Nx, Nth), np.where(zero, Ny, Nph)
        Lth, Lph = np.where(zero, Lx, Lth), np.where(zero, Ly, Lph)
        Z = Z0 / n_glass
        a_theta = Lph + Z * Nth
        a_phi = Lth - Z * Nph
        mag_theta = np.where(zero, _mag(Ly, Z * Nx), _mag(lph[0], lph[1], Z * nth[0], Z * nth[1]))
        mag_phi = np.where(zero, _mag(Lx, Z * Ny), _mag(lth[0], lth[1], Z * nph[0], Z * nph[1]))
        P = power_from_amplitudes(a_theta, a_phi, ux, uy, wavelength, n_glass, Z0)
    return P, a_theta, a_phi, mag_theta, mag_phi


def power_from_amplitudes(a_theta, a_phi, ux, uy, wavelength, n_glass, Z0):
    """the last two lines of the projection alone (nearfield_farfield.py:186-189): P from the two amplitudes"""
    ux = np.asarray(ux, dtype=float)
    uy = np.asarray(uy, dtype=float)
    with np.errstate(invalid='ignore'):
        uz = _uz(ux, uy)
        Z = Z0 / n_glass
        P = ((2 * pi * n_glass / wavelength) ** 2 / (32 * pi ** 2 * Z)
             * (abs(a_theta) ** 2 + abs(a_phi) ** 2)) / (uz + 1e-5)
        P = P * 2
    return P


def cell_of(ux, uy, pair_list):
    """dux * duy as the library takes it (ml_farfield_accumulate): the axes' first steps, a factor 1 for an axis of one
    direction, and 1 for a pair list"""
    if pair_list:
        return 1.0
    cell = 1.0
    if len(ux) > 1:
        cell *= ux[1] - ux[0]
    if len(uy) > 1:
        cell *= uy[1] - uy[0]
    return float(cell)


def cone_masks(ux, uy, pair_list, cone, centre):
    """-> (inside, on_edge) boolean, of P's shape: (ux - c0) * (ux - c0) + (uy - c1) * (uy - c1) <= cone * cone with
    every operation rounded on its own, and where the two sides are equal"""
    ux = np.asarray(ux, dtype=float) - centre[0]
    uy = np.asarray(uy, dtype=float) - centre[1]
    if pair_list:
        rho2 = ux * ux + uy * uy
    else:
        rho2 = (ux * ux).reshape(-1, 1) + (uy * uy).reshape(1, -1)
    lim = float(cone) * float(cone)
    return rho2 <= lim, rho2 == lim


def sweep_sums(P, ux, uy, pair_list, cone, centre):
    """-> dict(total, cone, inside, on_edge, cell): the exactly rounded sums (math.fsum) of the float64 products
    P * cell over the finite P, and of those inside the cone; the counts of directions inside the cone and exactly on
    its edge (finite P or not)"""
    P = np.asarray(P, dtype=float)
    cell = cell_of(ux, uy, pair_list)
    inside, edge = cone_masks(ux, uy, pair_list, cone, centre)
    assert inside.shape == P.shape
    terms = P * cell
    ok = np.isfinite(P)
    return dict(total=math.fsum(terms[ok]), cone=math.fsum(terms[ok & inside]), inside=int(inside.sum()),
                on_edge=int(edge.sum()), cell=cell)


def p_sum(maps, weights, resets):
    """P_sum after ml_farfield_accumulate(map, weight, reset) in call order: w * P on reset, else sum + w * P - the
    kernel's own two operations, so the result is expected bit for bit; NaN stays NaN (0.0 * NaN too)"""
    acc = None
    with np.errstate(invalid='ignore'):
        for P, w, reset in zip(maps, weights, resets):
            P = np.asarray(P, dtype=float)
            assert reset or acc is not None
            acc = w * P if reset else acc + w * P
    return acc


def sum_bound_units(n_directions):
    """the roundings between the exact sum of the products and the device's two-level sum, in units of 2**-53 of the
    total (all terms >= 0): the block tree of 256 (8 levels), the strided loop of accumulate_finish_kernel
    (ceil(blocks / 256) - 1 additions per lane) and its finishing tree (8 levels)"""
    blocks = -(-n_directions // 256)
    return 8 + (-(-blocks // 256) - 1) + 8
