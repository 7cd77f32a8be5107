"""The Stokes records of a propagated image (metalens_amd/csrc/propagate_stokes.hip, ml_propagate_stokes) restated from
downloaded arrays: the yardstick of tests/test_gpu_propagate_stokes.py, and the layout of csrc/propagate_stokes.h for
tests/test_propagate_stokes_host.py.

Per target the five components are ``metalens_amd.postprocess.stokes_maps`` - the kernel's operations, to the bit; every sum
over targets is ``math.fsum`` of the terms - correctly rounded, so what a comparison shows is the GPU's summation.  The
membership rule and the cut into chunks are those of tests/propagate_focus_ref.py.

Bound of a sum of n terms in any order: ``|err| <= (n + 16) u sum |term|``, ``u = 2^-53``; the 16 allows for forming a component
per target, and ``|term|`` is what the component is made of before it cancels: ``|Ex|^2 + |Ey|^2`` for S0 and S1, ``2 (|Ex.r Ey.r|
+ |Ex.i Ey.i|)`` for S2, ``2 (|Ex.r Ey.i| + |Ex.i Ey.r|)`` for S3, ``|Ez|^2`` for Iz.  From the sums the terms are the stored
doubles: ``n u sum |term|``."""
import math

import numpy as np

from metalens_amd.postprocess import stokes_maps
from propagate_focus_ref import inside

U = 2.0 ** -53
RADII_MAX, COMPONENTS = 32, 5                                  # csrc/propagate_stokes.h
PEAK_I, PEAK_INDEX, SUMS, CENTRE, ENC, PARTIAL = 0, 1, 2, 7, 9, 7 + 5 * 32


def record_doubles(K):
    return ENC + COMPONENTS * K


def terms(d):
    """a result dict -> (maps (5, ...), magnitudes (5, ...)): the components and what each is made of before it cancels"""
    Ex, Ey, Ez = d['Ex'], d['Ey'], d['Ez']
    M = stokes_maps(Ex, Ey, Ez)
    s0 = M[0]
    return M, np.stack([s0, s0, 2 * (np.abs(Ex.real * Ey.real) + np.abs(Ex.imag * Ey.imag)),
                        2 * (np.abs(Ex.real * Ey.imag) + np.abs(Ex.imag * Ey.real)), M[4]])


def _sum(v):
    return math.fsum(np.ravel(v).tolist())


def record(M, mag, dx, dy, radii, centre=None):
    """one plane (``M``, ``mag``: (5, mx, my); ``mag`` None: the stored doubles' moduli) -> the record as a dict, with the sum of
    |term| beside every sum (``*_abs``) and the number of targets inside every radius.  ``centre``: (ci, cj) in index units,
    None: the peak.  ``radii`` ascending."""
    M = np.asarray(M, dtype=float)
    mag = np.abs(M) if mag is None else mag
    I = M[0] + M[4]
    flat = int(np.argmax(I))                       # the lowest index of equals
    out = {'peak_I': float(I.ravel()[flat]), 'peak_index': flat, 'n': I.size}
    ci, cj = (float(flat // I.shape[1]), float(flat % I.shape[1])) if centre is None else (float(centre[0]), float(centre[1]))
    out['centre'] = (ci, cj)
    masks = [inside(I.shape, dx, dy, ci, cj, R)[0] for R in radii]
    out['n_inside'] = [int(m.sum()) for m in masks]
    out['sums'] = [_sum(M[q]) for q in range(COMPONENTS)]
    out['sums_abs'] = [_sum(mag[q]) for q in range(COMPONENTS)]
    out['enc'] = [[_sum(M[q][m]) for q in range(COMPONENTS)] for m in masks]
    out['enc_abs'] = [[_sum(mag[q][m]) for q in range(COMPONENTS)] for m in masks]
    return out


def check_record(rec, want, K, from_sums=False):
    """one plane's record of the entry against ``record`` -> the worst ratio of an error to its bound"""
    extra, worst = (0 if from_sums else 16), 0.0
    pairs = [(rec[SUMS + q], want['sums'][q], want['sums_abs'][q], want['n']) for q in range(COMPONENTS)]
    pairs += [(rec[ENC + COMPONENTS * r + q], want['enc'][r][q], want['enc_abs'][r][q], want['n_inside'][r])
              for r in range(K) for q in range(COMPONENTS)]
    for got, exact, mag, n in pairs:
        bound = (n + extra) * U * mag
        assert abs(got - exact) <= bound, (got, exact, bound)
        if bound:
            worst = max(worst, abs(got - exact) / bound)
    return worst
