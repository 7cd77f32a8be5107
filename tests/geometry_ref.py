"""The exact statements of the three discrete decisions of the synthesis (csrc/nearfield_geometry.hip sample_geometry), in
NumPy, mpmath and scipy, for tests/geometry_cases.py.  Everything here is a statement of integers: nothing has a tolerance.

ring    np.searchsorted(B, np.sqrt(x*x + y*y), 'left'), the reference's expression (nearfield.py:125-128).  The library is
        built without contraction, so the kernel's r is this fp64 value.
sector  clip(rint(phi / dphi), -half, half) with phi the CORRECTLY ROUNDED arctangent of the fp64 coordinates as given:
        float(mpmath.atan2(y, x)) at 240 bits.  mpmath has no signed zero, so a coordinate that is zero takes IEEE 754's
        rule through math.atan2, which is exact there (0, +-pi and +-pi/2 rounded once).  Beside it the oracle's
        round(np.arctan2(y, x) / dphi), for the census of where the two differ.
cell    the cell with the smallest d2 = ex*ex + ey*ey in fp64 - the kernel's own expression - over ALL cells, the lowest
        original index among equals; tie = the minimum is shared.  `nearest_cell_brute` is that statement word for word, in
        chunks.  `nearest_cell` gives the same answer faster: it evaluates the same d2 over the K cells scipy's cKDTree
        finds nearest, and that is every cell that can hold the minimum whenever the K-th lies beyond the best by more
        than 1e-9 relative (the tree's own distances are good to ~1e-16); a point where this cannot be shown goes through
        the brute force.  tests/test_geometry_cases.py holds the two against each other on a strided subset of every set.
"""
import math

import mpmath
import numpy as np
from scipy.spatial import cKDTree

MP_BITS = 240


def ring_of(B, x, y):
    with np.errstate(over='ignore', under='ignore'):
        r = np.sqrt(x * x + y * y)
    return np.searchsorted(B, r, 'left').astype(np.int64), r


def atan2_exact(x, y):
    """the correctly rounded arctan2(y, x) of fp64 coordinates, one at a time"""
    out = np.empty(len(x))
    with mpmath.workprec(MP_BITS):
        for i, (xi, yi) in enumerate(zip(x.tolist(), y.tolist())):
            if xi == 0.0 or yi == 0.0:
                out[i] = math.atan2(yi, xi)
            else:
                out[i] = float(mpmath.atan2(mpmath.mpf(yi), mpmath.mpf(xi)))
    return out


def tie_distance(x, y, dphi):
    """how far arctan2(y, x) / dphi lies from the nearest k + 1/2, in sectors, signed, worked out at MP_BITS"""
    out = np.empty(len(x))
    with mpmath.workprec(MP_BITS):
        for i, (xi, yi, di) in enumerate(zip(x.tolist(), y.tolist(), np.broadcast_to(dphi, (len(x),)).tolist())):
            q = mpmath.atan2(mpmath.mpf(yi), mpmath.mpf(xi)) / mpmath.mpf(di)
            out[i] = float(q - mpmath.floor(q) - mpmath.mpf(0.5))
    return out


def sector_of(x, y, dphi, half):
    """-> (correctly rounded decision, the oracle's decision with NumPy's arctangent)"""
    phi = atan2_exact(x, y)
    exact = np.clip(np.rint(phi / dphi), -half, half).astype(np.int64)
    numpy_ = np.clip(np.round(np.arctan2(y, x) / dphi), -half, half).astype(np.int64)
    return exact, numpy_


def nearest_cell_brute(x, y, cells, chunk=256):
    cx, cy = np.ascontiguousarray(cells[:, 0]), np.ascontiguousarray(cells[:, 1])
    idx, tie = np.empty(x.size, np.int64), np.empty(x.size, bool)
    for a in range(0, x.size, chunk):
        ex = x[a:a + chunk, None] - cx[None, :]
        ey = y[a:a + chunk, None] - cy[None, :]
        d2 = ex * ex + ey * ey
        idx[a:a + chunk] = d2.argmin(1)                       # the first minimum: the lowest original index
        tie[a:a + chunk] = (d2 == d2.min(1)[:, None]).sum(1) > 1
    return idx, tie


def nearest_cell(x, y, cells, k=16):
    n = len(cells)
    if n <= k:
        return nearest_cell_brute(x, y, cells)
    cx, cy = cells[:, 0], cells[:, 1]
    dist, near = cKDTree(cells[:, :2]).query(np.column_stack((x, y)), k=k)
    order = np.sort(near, axis=1)                             # candidates by original index: argmin takes the lowest
    ex, ey = x[:, None] - cx[order], y[:, None] - cy[order]
    d2 = ex * ex + ey * ey
    best = d2.min(1)
    idx = order[np.arange(x.size), d2.argmin(1)]
    tie = (d2 == best[:, None]).sum(1) > 1
    unsure = ~(dist[:, -1] > np.sqrt(best) * (1 + 1e-9))      # a cell beyond the K could still share the minimum
    if unsure.any():
        idx[unsure], tie[unsure] = nearest_cell_brute(x[unsure], y[unsure], cells)
    return idx, tie
