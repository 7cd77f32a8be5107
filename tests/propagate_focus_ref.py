"""The focus metrics of a propagated image (metalens_amd/csrc/propagate_focus.hip, ml_propagate_focus) restated in NumPy
from downloaded arrays: the yardstick of tests/test_gpu_propagate_focus.py, and the plan arithmetic of
csrc/propagate_focus.h for tests/test_propagate_focus_host.py.

Per target the weights are formed in the kernel's order of operations (that of ``propagate_accumulate_kernel``); every
sum over targets is ``math.fsum`` of the terms - correctly rounded, so what a comparison shows is the GPU's summation.
A target (i, j) is inside radius R about (ci, cj) iff ``fx fx + fy fy <= R R`` with ``fx = dx (i - ci)``, ``fy = dy (j - cj)``:
three separately rounded NumPy operations per line, as the kernel's.

Bound of a sum of n terms in any order: ``|err| <= (n + 16) u sum |term|``, ``u = 2^-53``; the 16 allows for forming I or Sz
per target, for which ``|term|`` is taken as ``(|Ex||Hy| + |Ey||Hx|) / 2`` times the geometric factor (Sz cancels inside a
target).  From the sums the terms are the stored doubles: ``n u sum |term|``."""
import math

import numpy as np

U = 2.0 ** -53
RADII_MAX, CHUNK_MIN, CHUNKS_MAX, STEP, FINISH_TILE = 32, 1024, 1024, 512, 32        # csrc/propagate_focus.h
PEAK_I, PEAK_INDEX, MOM_I, MOM_SZ, CENTRE, ENC, PARTIAL = 0, 1, 2, 8, 14, 16, 14 + 2 * 32


def record_doubles(K):
    return ENC + 2 * K


def chunk_targets(P):
    """targets per chunk of a plane of P targets: 1024, doubled until the plane has at most 1024 chunks"""
    c = CHUNK_MIN
    while -(-P // c) > CHUNKS_MAX:
        c *= 2
    return c


def plan(mx, my, K):
    P = mx * my
    c = chunk_targets(P)
    chunks = -(-P // c)
    return dict(mx=mx, my=my, P=P, chunk=c, chunks=chunks, steps=c // STEP, last=P - (chunks - 1) * c,
                record_doubles=record_doubles(K), partial_doubles=PARTIAL)


def finish(mx, my):
    """the tiles of the second launch, which takes the chunks' partial records 32 at a time (focus_finish_tiles): what
    ``propagate_focus_plan finish`` prints"""
    chunks = plan(mx, my, 0)['chunks']
    tiles = -(-chunks // FINISH_TILE)
    return dict(mx=mx, my=my, chunks=chunks, finish_tile=FINISH_TILE, finish_tiles=tiles, last_tile=chunks - (tiles - 1) * FINISH_TILE)


def weights(d, want_h):
    """-> I, Sz, Sz's scale (both None without H) of a result dict of ``PlanePropagator``: the kernel's operations"""
    sq = [d[k].real * d[k].real + d[k].imag * d[k].imag for k in ('Ex', 'Ey', 'Ez')]
    I = (sq[0] + sq[1]) + sq[2]
    if not want_h:
        return I, None, None
    Sz = 0.5 * ((d['Ex'].real * d['Hy'].real + d['Ex'].imag * d['Hy'].imag)
                - (d['Ey'].real * d['Hx'].real + d['Ey'].imag * d['Hx'].imag))
    return I, Sz, 0.5 * (np.abs(d['Ex']) * np.abs(d['Hy']) + np.abs(d['Ey']) * np.abs(d['Hx']))


def geometry(shape):
    """the six factors 1, i, j, i^2, j^2, i j of the moments, exact doubles of shape ``shape``"""
    fi, fj = np.meshgrid(np.arange(shape[0], dtype=float), np.arange(shape[1], dtype=float), indexing='ij')
    return [np.ones(shape), fi, fj, fi * fi, fj * fj, fi * fj]


def inside(shape, dx, dy, ci, cj, R):
    fi, fj = np.meshgrid(np.arange(shape[0], dtype=float), np.arange(shape[1], dtype=float), indexing='ij')
    fx = dx * (fi - ci)
    fy = dy * (fj - cj)
    r2 = fx * fx + fy * fy
    return r2 <= R * R, r2


def _sum(terms):
    return math.fsum(np.ravel(terms).tolist())


def record(I, Sz, dx, dy, radii, centre=None, scale=None):
    """one plane (2-D arrays; Sz may be None) -> the record as a dict, with the sum of |term| beside every sum (``*_abs``; for
    Sz with ``scale`` in place of |Sz| where given) and the number of targets inside every radius.  ``centre``: (ci, cj) in
    index units, None: the peak.  ``radii`` ascending."""
    I = np.asarray(I, dtype=float)
    flat = int(np.argmax(I))                       # the lowest index of equals
    out = {'peak_I': float(I.ravel()[flat]), 'peak_index': flat, 'n': I.size}
    ci, cj = (float(flat // I.shape[1]), float(flat % I.shape[1])) if centre is None else (float(centre[0]), float(centre[1]))
    out['centre'] = (ci, cj)
    masks = [inside(I.shape, dx, dy, ci, cj, R)[0] for R in radii]
    out['masks'] = masks
    out['n_inside'] = [int(m.sum()) for m in masks]
    geo = geometry(I.shape)
    for name, w, mag in (('I', I, np.abs(I)), ('Sz', Sz, None if Sz is None else (np.abs(Sz) if scale is None else scale))):
        if w is None:
            continue
        out['mom_' + name] = [_sum(w * g) for g in geo]
        out['mom_%s_abs' % name] = [_sum(mag * g) for g in geo]
        out['enc_' + name] = [_sum(w[m]) for m in masks]
        out['enc_%s_abs' % name] = [_sum(mag[m]) for m in masks]
    return out
