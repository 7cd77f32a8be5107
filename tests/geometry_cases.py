"""The case table of the synthesis decisions: layouts, points on every edge of every decision, and what
tests/geometry_ref.py says about them.  tests/test_geometry_cases.py checks the table itself on the CPU;
tests/test_gpu_geometry_cases.py holds ml_geometry_probe against it at EVERY point.

A case = one layout (what packing.upload_layout takes) + points + the expected (ring, pick, tie).  `case(name)` builds it
once per process (functools.lru_cache); nobody may write into what it returns.

Layouts
  small     _synthetic_lens(40e-6, 0.4, 580e-9, switch_deg=9.0): 13 rings, 7267 hexagonal cells
  na094     extra_random_sweep.lens_of(1e-3, 0.94, 580e-9): 1195 rings, the narrowest 0.6 um
  narrow    small with ring 5 cut into 24 rings of 0.2 nm and one of no width: 2 r_max / narrowest = 4e5 > 65536, so the
            bucket records are 0.62 nm wide and hold three boundaries each
  odd       small with num_around_circle = 45, 7001 (odd: +-pi is a sector boundary) and 36, 44 (4 mod 8: the diagonals
            are) on rings 1, 3, 5, 7
  cell sets on small: hex (its own), holes, jitter, shuffled (as test_nearest_cell_on_irregular_cell_sets makes them),
            cluster (jitter + 12 cells within 0.2 pitch + two identical cells), sparse (7 lattice cells 4 um apart), one, none
The ring and sector cases carry no cells (their centre points expect pick -1); the cell cases carry small's rings.
"""
import copy
import functools
import math

import mpmath
import numpy as np
from scipy.spatial import Delaunay, cKDTree

import geometry_ref as ref

WL = 580e-9
PITCH = 320e-9                     # of small's hexagonal cells
OFFS = (0.0, 1e-16, 3e-16, 1e-15, 1e-14, 1e-12, 0.99e-9, 1.01e-9, 1e-6)   # |off| in sectors; every one but 0 with both signs
TIE_WINDOW = 1e-9                  # nearfield_geometry.hip sector_of_fast
ODD_NUMS = {1: 45, 3: 7001, 5: 36, 7: 44}
MP_POINT_CAP, CASE_POINT_CAP = 40000, 1 << 18

# ML_GEO_* of include/metalens_hip.h
RING_RECORD, RING_SEARCH, SECTOR_EXACT, SECTOR_CLAMPED = 1, 2, 4, 8
CELL_NODE, CELL_FOUR, CELL_BINS, CELL_MORE, CELL_GROW, TIE = 16, 32, 64, 128, 256, 512

RING_CASES = ['small-rings', 'na094-rings', 'narrow-rings']
SECTOR_CASES = ['small-sectors', 'na094-sectors', 'odd-sectors']
CELL_SETS = ['hex', 'holes', 'jitter', 'shuffled', 'cluster', 'sparse', 'one', 'none']
CELL_CASES = ['cells-' + s for s in CELL_SETS]
CASES = RING_CASES + SECTOR_CASES + CELL_CASES


# ---- lens_pack.h restated (tests/test_geometry_cases.py pins both to the packers' own output) -----------------------
def record_buckets(B):
    """pack_ring_search: -> (nb, hb) of the bucket records"""
    w = np.diff(B)
    narrowest = min(B[-1], w[w > 0].min())
    nb = int(min(65536.0, max(1024.0, math.ceil(2.0 * B[-1] / narrowest))))
    return nb, B[-1] / nb


def ring_by_record(B, r):
    """boundaries_below_fast: True where the bucket record (or r > r_outer) settles the ring, False where the search runs"""
    nb, hb = record_buckets(B)
    first = np.searchsorted(B, np.arange(nb) * hb, 'left')
    ext = np.concatenate(([-np.inf], B, [np.inf, np.inf]))
    with np.errstate(over='ignore', invalid='ignore'):
        b = np.clip(np.minimum(r * (1.0 / hb), 2.0 ** 31 - 1).astype(np.int64), 0, nb - 1)
    return (r > B[-1]) | ((ext[first[b]] < r) & ~(ext[first[b] + 2] < r))


def cell_bins(cells):
    """bin_cells: -> (bins_x, bins_y, x0, y0, h)"""
    x0, x1, y0, y1 = cells[:, 0].min(), cells[:, 0].max(), cells[:, 1].min(), cells[:, 1].max()
    wx, wy = x1 - x0, y1 - y0
    h = math.sqrt(max(wx * wy, 1e-300) / len(cells))
    if not (h > 0) or not math.isfinite(h) or (wx <= 0 and wy <= 0):
        h = 1.0
    bx = max(int(min(math.floor(wx / h) + 1, 8192)), 1)
    by = max(int(min(math.floor(wy / h) + 1, 8192)), 1)
    h = max(h, max(wx / bx, wy / by) * (1 + 1e-12))
    return bx, by, x0, y0, h


# ---- layouts --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lens(name):
    if name == 'small':
        from test_gpu_parity import _synthetic_lens
        return _synthetic_lens(40e-6, 0.4, WL, switch_deg=9.0)
    import extra_random_sweep
    return extra_random_sweep.lens_of(1e-3, 0.94, WL)


RING_KEYS = ('r_center_list', 'r_min_list', 'r_max_list', 'grating_period_list', 'gratingcollection_index_here_list',
             'num_around_circle_list')
NARROW_RING, NARROW_CUTS, NARROW_STEP, NARROW_TWICE = 5, 24, 2e-10, 12


def _narrow(S):
    """ring 5 of small cut: boundaries r_min + j 0.2 nm, j = 1 ... 24, the twelfth of them twice (a ring of no width)"""
    out = copy.copy(S)
    r_min, r_max = np.asarray(S['r_min_list'], float), np.asarray(S['r_max_list'], float)
    k = NARROW_RING
    cuts = [r_min[k] + j * NARROW_STEP for j in range(1, NARROW_CUTS + 1)]
    cuts.insert(NARROW_TWICE, cuts[NARROW_TWICE - 1])
    new_min = np.concatenate((r_min[:k + 1], cuts, r_min[k + 1:]))
    new_max = np.concatenate((new_min[1:], r_max[-1:]))
    rep = np.concatenate((np.arange(k + 1), np.full(len(cuts), k), np.arange(k + 1, r_min.size)))
    for key in RING_KEYS:
        out[key] = np.asarray(S[key])[rep]
    out['r_min_list'], out['r_max_list'], out['r_center_list'] = new_min, new_max, 0.5 * (new_min + new_max)
    return out


def _odd(S):
    out = copy.copy(S)
    num = np.array(S['num_around_circle_list'])
    for ring, n in ODD_NUMS.items():
        num[ring] = n
    out['num_around_circle_list'] = num
    return out


def _cells(kind):
    cells = np.array(lens('small')['lens_center_summary'], dtype=float)
    removed = None
    if kind in ('holes', 'jitter', 'shuffled', 'cluster'):
        rng = np.random.default_rng({'holes': 1, 'jitter': 2, 'shuffled': 3, 'cluster': 2}[kind])
        if kind == 'holes':
            keep = rng.random(len(cells)) > 0.1
            removed, cells = cells[~keep], cells[keep]
        elif kind in ('jitter', 'cluster'):
            cells[:, :2] += rng.uniform(-0.05, 0.05, (len(cells), 2)) * PITCH
        else:
            cells = cells[rng.permutation(len(cells))]
        if kind == 'cluster':
            knot = np.column_stack((3.33e-6 + rng.uniform(-0.1, 0.1, 12) * PITCH, -2.1e-6 + rng.uniform(-0.1, 0.1, 12) * PITCH,
                                    np.arange(12.0)))
            twin = np.array([[-5.013e-6, 4.021e-6, 3.0], [-5.013e-6, 4.021e-6, 4.0]])
            cells = np.vstack((cells, knot, twin))
    elif kind == 'sparse':
        # 4 um apart on two neighbouring rows: the bins come out ~1 um wide, so most of the disc is farther than a bin
        # width from every cell and the 3 x 3 bin runs cannot settle it
        want = [((j - 3) * 4e-6, (j % 2) * 0.28e-6) for j in range(7)]
        cells = cells[cKDTree(cells[:, :2]).query(want)[1]]
    elif kind == 'one':
        cells = cells[len(cells) // 2:len(cells) // 2 + 1]
    elif kind == 'none':
        cells = None
    return cells, removed


@functools.lru_cache(maxsize=None)
def layout(name):
    """-> (periphery summary, cells or None): the arguments of packing.upload_layout"""
    kind = name.split('-')[0]
    if kind == 'cells':
        return lens('small')['lens_periphery_summary'], _cells(name.split('-')[1])[0]
    S = lens('na094' if kind == 'na094' else 'small')['lens_periphery_summary']
    return {'narrow': _narrow, 'odd': _odd}.get(kind, lambda s: s)(S), None


def packed(name):
    from metalens_amd import packing
    S, cells = layout(name)
    return packing.pack_layout(S, cells)


# ---- points ---------------------------------------------------------------------------------------------------------
class Points:
    def __init__(self):
        self.x, self.y, self.family, self.off, self.edge = [], [], [], [], []

    def add(self, family, x, y, off=np.nan, edge=-1):
        x, y = np.atleast_1d(np.asarray(x, float)), np.atleast_1d(np.asarray(y, float))
        x, y = np.broadcast_arrays(x, y)
        self.x.append(x.ravel())
        self.y.append(y.ravel())
        self.family += [family] * x.size
        self.off.append(np.broadcast_to(np.asarray(off, float), x.shape).ravel())
        self.edge.append(np.broadcast_to(np.asarray(edge, np.int64), x.shape).ravel())

    def done(self):
        return dict(x=np.concatenate(self.x), y=np.concatenate(self.y), family=np.array(self.family),
                    off=np.concatenate(self.off), edge=np.concatenate(self.edge))


def ulps(v, n):
    """v moved by n units in the last place (n of either sign)"""
    v = np.asarray(v, float)
    for _ in range(abs(n)):
        v = np.nextafter(v, np.inf if n > 0 else -np.inf)
    return v


OBLIQUE = (0.3, 1.1, 2.5)          # radians; the third in the second quadrant


def _oblique(target, angle):
    """an fp64 point near `angle` whose computed r = sqrt(x*x + y*y) IS `target`, by search over the neighbours of
    (target cos, target sin); None if there is none within 12 ulp"""
    x0, y0 = target * math.cos(angle), target * math.sin(angle)
    xs = np.array([ulps(x0, n) for n in range(-12, 13)])
    ys = np.array([ulps(y0, n) for n in range(-12, 13)])
    r = np.sqrt(xs[:, None] * xs[:, None] + ys[None, :] * ys[None, :])
    hit = np.argwhere(r == target)
    if not len(hit):
        return None
    i, j = hit[np.abs(hit - 12).sum(1).argmin()]
    return xs[i], ys[j]


def ring_points(B, max_edges=512, seed=11):
    P = Points()
    n = B.size
    if n > max_edges:
        w = np.diff(B)
        k = int(np.where(w > 0, w, np.inf).argmin())
        must = {0, n - 1, k, k + 1}
        rest = [e for e in np.random.default_rng(seed).permutation(n).tolist() if e not in must]
        edges = sorted(must | set(rest[:max_edges - len(must)]))
    else:
        edges = list(range(n))
    for k in edges:
        for u in (-2, -1, 0, 1, 2):
            P.add('axis', ulps(B[k], u), 0.0, edge=k)
        for angle in OBLIQUE:
            for u in (-1, 0, 1):
                p = _oblique(float(ulps(B[k], u)), angle)
                if p is not None:
                    P.add('oblique', p[0], p[1], edge=k)
    nb, hb = record_buckets(B)
    for b in np.random.default_rng(seed + 1).choice(np.arange(1, nb), 256, replace=False):
        for u in (-1, 0, 1):
            P.add('bucket', ulps(b * hb, u), 0.0, edge=int(b))
    P.add('extreme', [0.0, 1e-300, B[-1], ulps(B[-1], 1), 1e300], 0.0)
    return P


def sector_points(L, seed=23):
    """near-tie points per distinct dphi, the axes with both signed zeros, the diagonals"""
    P = Points()
    rng = np.random.default_rng(seed)
    B, dphi_all, rc = L['boundaries'], L['dphi'], L['r_center']
    distinct = np.unique(dphi_all)
    if distinct.size > 8:
        distinct = distinct[np.linspace(0, distinct.size - 1, 8).astype(int)]
    offs = [0.0] + [s * o for o in OFFS[1:] for s in (1, -1)]
    with mpmath.workprec(ref.MP_BITS):
        for d in distinct:
            ring = int(np.flatnonzero(dphi_all == d)[0])
            N = int(round(2 * math.pi / d))
            ks = [-(N // 2) - 1, -(N // 2), -1, 0, N // 2 - 1, N // 2] + rng.integers(-(N // 2), N // 2, 16).tolist()
            r = mpmath.mpf(float(rc[ring]))
            for k in ks:
                for off in offs:
                    th = (mpmath.mpf(k) + mpmath.mpf(0.5) + mpmath.mpf(off)) * mpmath.mpf(float(d))
                    P.add('tie', float(r * mpmath.cos(th)), float(r * mpmath.sin(th)), off=off, edge=ring)
            v = float(rc[ring])
            P.add('axes', [v, v, -v, -v, 0.0, -0.0, 0.0, -0.0], [0.0, -0.0, 0.0, -0.0, v, v, -v, -v], edge=ring)
    for r in rng.uniform(B[0] * 1.001, B[-1] * 0.999, 500):
        v = r / math.sqrt(2.0)
        for w in (v, float(ulps(v, -1)), float(ulps(v, 1))):
            P.add('diagonal', [v, v, -v, -v], [w, -w, w, -w])
    return P


def cell_points(cells, removed, B0, seed=37):
    P = Points()
    rng = np.random.default_rng(seed)
    P.add('rim', B0, 0.0)                                        # r == B[0] on the axis: still the centre disc
    phi, rad = rng.uniform(0, 2 * math.pi, 10000), B0 * np.sqrt(rng.uniform(0, 1, 10000))
    P.add('random', rad * np.cos(phi), rad * np.sin(phi))
    if cells is None:
        return P
    xy = cells[:, :2]
    P.add('centre', xy[:, 0], xy[:, 1])
    if len(cells) >= 2:
        near = cKDTree(xy).query(xy, k=min(7, len(cells)))[1]
        pairs = np.unique(np.sort(np.column_stack((np.repeat(near[:, 0], near.shape[1] - 1), near[:, 1:].ravel())), 1), axis=0)
        pairs = pairs[pairs[:, 0] != pairs[:, 1]]
        mx, my = 0.5 * (xy[pairs[:, 0], 0] + xy[pairs[:, 1], 0]), 0.5 * (xy[pairs[:, 0], 1] + xy[pairs[:, 1], 1])
        P.add('midpoint', mx, my)
        for u in (-1, 1):
            P.add('midpoint', ulps(mx, u), my)
            P.add('midpoint', mx, ulps(my, u))
    if len(cells) >= 3:
        tri = Delaunay(xy).simplices
        side = np.max([np.hypot(*(xy[tri[:, a]] - xy[tri[:, b]]).T) for a, b in ((0, 1), (1, 2), (0, 2))], axis=0)
        if len(cells) > 7:                                       # neighbour triangles only: no slivers along the hull
            tri = tri[side < 1.6 * PITCH]
        c = xy[tri].sum(1) / 3.0
        P.add('centroid', c[:, 0], c[:, 1])
    if removed is not None:
        P.add('hole', removed[:, 0], removed[:, 1])
    bx, by, x0, y0, h = cell_bins(cells)
    for k in range(256):
        along = rng.uniform(-0.7, 0.7) * B0
        if k % 2 == 0:
            e = x0 + rng.integers(0, bx + 1) * h
            for u in (-1, 0, 1):
                P.add('bin', ulps(e, u), along)
        else:
            e = y0 + rng.integers(0, by + 1) * h
            for u in (-1, 0, 1):
                P.add('bin', along, ulps(e, u))
    return P


# ---- cases ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: S, cells (layout); x, y, family, off, edge (points); ring, pick, tie (expected), r, numpy_sector (the
    oracle's sector, ring samples), mp_points (how many needed mpmath), L (packing.pack_layout's output)"""
    S, cells = layout(name)
    L = packed(name)
    B = L['boundaries']
    kind = name.split('-')[1] if not name.startswith('cells') else 'cells'
    if kind == 'rings':
        P = ring_points(B)
    elif kind == 'sectors':
        P = sector_points(L)
    else:
        P = cell_points(cells, _cells(name.split('-')[1])[1], B[0])
    c = P.done()
    if kind == 'cells':                      # the cell families belong to the centre disc
        keep = ref.ring_of(B, c['x'], c['y'])[0] == 0
        c = {k: v[keep] for k, v in c.items()}
    x, y = c['x'], c['y']
    ring, r = ref.ring_of(B, x, y)
    n_rings = B.size - 1
    pick = np.full(x.size, -1, np.int64)
    numpy_sector = np.full(x.size, -1, np.int64)
    tie = np.zeros(x.size, bool)
    on_ring = (ring >= 1) & (ring <= n_rings)
    if on_ring.any():
        at = ring[on_ring] - 1
        pick[on_ring], numpy_sector[on_ring] = ref.sector_of(x[on_ring], y[on_ring], L['dphi'][at], L['rot_half'][at])
    centre = ring == 0
    if centre.any() and cells is not None:
        pick[centre], tie[centre] = ref.nearest_cell(x[centre], y[centre], cells)
    c.update(S=S, cells=cells, L=L, ring=ring, r=r, pick=pick, tie=tie, numpy_sector=numpy_sector, on_ring=on_ring,
             mp_points=int(on_ring.sum()), name=name)
    return c


def grow_certain(c):
    """centre points that MUST reach the ring-growing search: farther than one bin width from every cell, which the bin
    runs do not accept, and farther than a pitch, which bounds what the lattice stages accept"""
    cells = c['cells']
    h = cell_bins(cells)[4]
    d = cKDTree(cells[:, :2]).query(np.column_stack((c['x'], c['y'])))[0]
    return (c['ring'] == 0) & (d > h * (1 + 1e-6)) & (d > PITCH)
