"""The cases of the direct pair sum of the finite-distance propagator (csrc/propagate.hip ``propagate_kernel<WANT_H, NS>`` with
csrc/propagate_direct.h, ``method='direct'``) that the suite compares with the long-double sum target by target, in one
table, and the instantiations, launch shapes, LDS tile edges, target edges and field states the table has to reach.  Plain
data and pure functions, no test collects from here: test_propagate_direct_cases.py holds every row's ``expect`` against
what tools/propagate_direct_plan prints and the table against ``INVENTORY``; test_gpu_propagate_direct_cases.py runs the rows
on the GPU.

A row: ``(nx, ny, targets, want_h, state, sets, claims, expect)``.  The aperture has nx x ny samples at the pitch lambda / 2.2
by lambda / 2.3 (``test_gpu_fft_mixed._axes``) unless ``state`` is 'resident'.  ``targets``: ('points', T) - a list of T
points with z of their own from 2 um to 1 mm, a third of them up to two and a half aperture widths outside -, ('plane', mx,
my) - a tensor grid 20 um behind the aperture -, ('near',) - ``NEAR`` -, ('one',) - one point.  ``want_h``: the variants run,
'EH' and 'E'.  ``state``: 'uploaded' (through the Python class: no row extents), 'cabi' (uploaded and propagated through the
C ABI: the class needs two samples per axis) or 'resident' (synthesised on the GPU on the window ``RESIDENT`` names: row
extents; ``sets`` field sets in one pass).  ``claims``: what the synthesised field has to show for the row to reach a field
state - the GPU test asserts each from the downloaded field, not from the geometry.

``expect``: tiles (workgroups along the targets), splits (workgroups per target tile; workgroup s sums the aperture rows s, s
+ splits, ...), rows_min and rows_max (rows of the least and the most loaded of them) - what ``propagate_direct_plan`` prints
- and ny_tiles, ny_tail: the whole LDS tiles of PROP_TILE = 128 samples in a row read whole, and the samples behind them.
"""
import collections
import fractions

import numpy as np

import propagate_ref as ref

Row = collections.namedtuple('Row', 'nx ny targets want_h state sets claims expect')
Expect = collections.namedtuple('Expect', 'tiles splits rows_min rows_max ny_tiles ny_tail')

WL, N_GLASS = ref.WL, ref.N_GLASS
K = 2 * np.pi * N_GLASS / WL
THREADS, TILE, BLOCKS = 256, 128, 2048          # csrc/propagate_direct.h PROP_THREADS, PROP_TILE, PROP_BLOCKS
KERNEL = 'propagate_kernel<%s, %d>'             # WANT_H, NS
MAX_COMPARED = 64

EXTENT_SPAN = 'resident: a row extent with first > 0 spans more than one tile'
SKIP_THEN_LIVE = 'resident: a workgroup skips its first row and sums a later one'
LIVE_THEN_SKIP = 'resident: a workgroup sums a row and skips a later one'

# ---- what has to be reached ------------------------------------------------------------------------------------------
INVENTORY = frozenset(
    [KERNEL % (h, ns) for h in ('true', 'false') for ns in (1, 2, 3)]
    + ['splits == nx', 'splits < nx, rows_min < rows_max', 'rows_max >= 3', 'splits == 2', 'splits == 1 by the tile count, nx > 1',
       'ny <= 64', '64 < ny < 128', 'ny == 128', 'ny == 129', 'ny of exactly two tiles', 'ny of two tiles and a tail',
       'T == 1', 'T == 64', 'T == 65', 'T == 256', 'T == 257',
       'an axis of one sample',
       EXTENT_SPAN, SKIP_THEN_LIVE, LIVE_THEN_SKIP, 'uploaded: no extents',
       'target in the near zone, k R < 1', 'target exactly above a sample, dx = dy = 0'])

BOTH = ('EH', 'E')


def _ny(n):
    return n // TILE, n % TILE


def _row(nx, ny, targets, state, expect4, sets=1, claims=()):
    return Row(nx, ny, targets, BOTH, state, sets, tuple(claims), Expect(*(expect4 + _ny(ny))))


ROWS = {
    # one pair, against the closed form
    'd-one': _row(1, 1, ('one',), 'cabi', (1, 1, 1, 1)),
    # one live wave exactly, one lane of a second wave; one workgroup exactly, a second one with one live lane
    'd-wave-64': _row(7, 5, ('points', 64), 'uploaded', (1, 7, 1, 1)),
    'd-wave-65': _row(7, 5, ('points', 65), 'uploaded', (1, 7, 1, 1)),
    'd-tile-256': _row(7, 5, ('points', 256), 'uploaded', (1, 7, 1, 1)),
    'd-tile-257': _row(7, 5, ('points', 257), 'uploaded', (2, 7, 1, 1)),
    # the LDS tile's edges: no second staging column, one sample in it, one tile, a tail of one, two tiles, two and one
    'd-ny-1': _row(3, 1, ('points', 70), 'cabi', (1, 3, 1, 1)),
    'd-ny-64': _row(3, 64, ('points', 70), 'uploaded', (1, 3, 1, 1)),
    'd-ny-65': _row(3, 65, ('points', 70), 'uploaded', (1, 3, 1, 1)),
    'd-ny-128': _row(3, 128, ('points', 70), 'uploaded', (1, 3, 1, 1)),
    'd-ny-129': _row(3, 129, ('points', 70), 'uploaded', (1, 3, 1, 1)),
    'd-ny-256': _row(3, 256, ('points', 70), 'uploaded', (1, 3, 1, 1)),
    'd-ny-257': _row(3, 257, ('points', 70), 'uploaded', (1, 3, 1, 1)),
    # 25 target tiles, 82 workgroups each: 48 of two rows and 34 of one; 36 of three rows and 46 of two
    'd-two-rows': _row(130, 5, ('plane', 80, 80), 'uploaded', (25, 82, 1, 2)),
    'd-three-rows': _row(200, 3, ('plane', 80, 80), 'uploaded', (25, 82, 2, 3)),
    # image planes: two workgroups per target tile (three rows and two), and the whole aperture in one
    'd-splits-2': _row(5, 3, ('plane', 512, 512), 'uploaded', (1024, 2, 2, 3)),
    'd-splits-1': _row(5, 3, ('plane', 1024, 512), 'uploaded', (2048, 1, 5, 5)),
    # 30 nm behind the aperture: on samples, between samples, just outside the footprint
    'd-near': _row(7, 5, ('near',), 'uploaded', (1, 7, 1, 1)),
    # window A of test_gpu_propagate_sets.py, NS = 3 and 2: its last rows lie outside the lens
    'd-sets-A-xyz': _row(96, 130, ('plane', 80, 80), 'resident', (25, 82, 1, 2), sets=3, claims=(LIVE_THEN_SKIP,)),
    'd-sets-A-xy': _row(96, 130, ('plane', 80, 80), 'resident', (25, 82, 1, 2), sets=2, claims=(LIVE_THEN_SKIP,)),
    # window A mirrored at the lens' axis: its FIRST rows lie outside the lens, the workgroups that skip them sum row s + 82
    'd-skip-first': _row(96, 130, ('plane', 80, 80), 'resident', (25, 82, 1, 2), claims=(SKIP_THEN_LIVE,)),
    # 40 x 300 across the lens' edge: chords of 57 to 262 samples, each inside its row
    'd-extent-span': _row(40, 300, ('points', 70), 'resident', (1, 40, 1, 1), claims=(EXTENT_SPAN,)),
}

# the windows of the resident rows on the lens of test_gpu_propagate_sets._lens (centre disc to 21.9 um, rings to 60.6 um):
# (centre x, centre y, batch of test_gpu_propagate_sets)
RESIDENT = {
    'd-sets-A-xyz': (50.5e-6, 1.0e-6, 'DIPOLES'), 'd-sets-A-xy': (50.5e-6, 1.0e-6, 'TWO_DIPOLES'),
    'd-skip-first': (-50.5e-6, 1.0e-6, 'ONE_DIPOLE'), 'd-extent-span': (55.0e-6, 0.0, 'ONE_DIPOLE'),
}
ONE_DIPOLE = ('one dipole', (0.3e-6, -0.2e-6, None), 'x')      # NS = 1, the source of test_gpu_propagate_sets.DIPOLES
PITCH = WL / 2.2                                               # of the resident windows, both axes
# rows whose second call must give the bits of the first, and rows whose sums are checked (one reset and one adding call)
REPEATED = ('d-splits-1', 'd-splits-2', 'd-two-rows', 'd-three-rows')
SUMMED = ('d-one', 'd-tile-256', 'd-tile-257')

# the near-zone targets in units of the pitch from sample (0, 0) of the 7 x 5 aperture, 30 nm behind it: eight on samples
# (the first four exactly: the kernel's dx = fma(-i, dx', x - x0) is 0 for i = 0 and 1), sixteen between samples, sixteen
# half a pitch outside the footprint
NEAR_Z = 30e-9
NEAR = ([(0, 0), (1, 1), (0, 1), (1, 0), (3, 2), (6, 4), (6, 0), (0, 4)]
        + [(i + 0.5, j + 0.5) for i in (0, 2, 3, 5) for j in (0, 3)] + [(i + 0.5, j) for i in (0, 1, 4, 5) for j in (1, 4)]
        + [(-0.5, j) for j in (0, 1.5, 2, 4)] + [(6.5, j) for j in (0, 2, 3.5, 4)]
        + [(i, -0.5) for i in (0, 2.5, 3, 6)] + [(i, 4.5) for i in (0, 3, 4.5, 6)])


# ---- the launch arithmetic, restated --------------------------------------------------------------------------------
def n_targets(row):
    kind = row.targets[0]
    return {'one': 1, 'near': len(NEAR)}.get(kind) or (row.targets[1] if kind == 'points' else row.targets[1] * row.targets[2])


def plan(T, nx):
    """tiles, splits, rows_min, rows_max as csrc/propagate_direct.h has them"""
    tiles = -(-T // THREADS)
    splits = max(1, min(nx, -(-BLOCKS // tiles)))
    rows = [len(range(s, nx, splits)) for s in range(splits)]
    return tiles, splits, min(rows), max(rows)


# ---- axes, fields and targets ---------------------------------------------------------------------------------------
def axes(name):
    """-> x, y, (dx', dy') of the aperture of a row"""
    row = ROWS[name]
    if row.state == 'resident':
        cx, cy, _ = RESIDENT[name]
        x, y = cx + (np.arange(row.nx) - (row.nx - 1) / 2) * PITCH, cy + (np.arange(row.ny) - (row.ny - 1) / 2) * PITCH
        return x, y, (float(x[1] - x[0]), float(y[1] - y[0]))
    from test_gpu_fft_mixed import _axes
    x, y = _axes(max(row.nx, 2), max(row.ny, 2))
    pitch = (float(x[1] - x[0]), float(y[1] - y[0]))
    return x[:row.nx], y[:row.ny], pitch


def uploaded_fields(name):
    from test_gpu_fft import fields
    row = ROWS[name]
    return fields(row.nx, row.ny, row.nx + row.ny)


def targets(name):
    """-> tx, ty, tz, point_list"""
    row = ROWS[name]
    x, y, (dxp, dyp) = axes(name)
    kind = row.targets[0]
    cx, cy = x.mean(), y.mean()
    if kind == 'one':
        return np.array([x[0] + 0.7e-6]), np.array([y[0] - 0.4e-6]), np.array([1.3e-6]), True
    if kind == 'near':
        at = np.array(NEAR, dtype=float)
        tx, ty = np.empty(len(at)), np.empty(len(at))
        for d, (i, j) in enumerate(at):
            # on a sample: the axis' own number; elsewhere the origin plus the pitches
            tx[d] = x[int(i)] if i == int(i) and 0 <= i < row.nx else x[0] + i * dxp
            ty[d] = y[int(j)] if j == int(j) and 0 <= j < row.ny else y[0] + j * dyp
        return tx, ty, np.full(len(at), NEAR_Z), True
    if kind == 'plane':
        # (for window A: the plane of test_gpu_propagate_sets._targets) an axis of a few samples gets 20 um all the same
        wx, wy = max(np.ptp(x), 20e-6), max(np.ptp(y), 20e-6)
        _, mx, my = row.targets
        return cx + np.linspace(-0.6, 0.55, mx) * wx, cy + np.linspace(-0.5, 0.6, my) * wy, np.array([20e-6]), False
    T = row.targets[1]
    rng = np.random.default_rng(1000 + T)
    wx, wy = max(np.ptp(x), 4 * dxp), max(np.ptp(y), 4 * dyp)
    spread = np.where(np.arange(T) % 3 == 0, 2.5, 0.5)
    return (cx + rng.uniform(-1, 1, T) * spread * wx, cy + rng.uniform(-1, 1, T) * spread * wy,
            2e-6 * 500 ** rng.uniform(0, 1, T), True)


def points(name):
    """-> [T][3], flat in the order of the result"""
    tx, ty, tz, point_list = targets(name)
    if point_list:
        return np.stack([tx, ty, tz], axis=1)
    TX, TY = np.meshgrid(tx, ty, indexing='ij')
    return np.stack([TX.ravel(), TY.ravel(), np.full(TX.size, tz[0])], axis=1)


def compared(name):
    """the flat targets of a row that are compared with the long-double sum, at most ``MAX_COMPARED``: 0, 63, 64, 255, 256 and
    T - 1 where they exist, the four corners of a plane, and targets spread evenly over the rest"""
    row = ROWS[name]
    T = n_targets(row)
    must = {t for t in (0, 63, 64, 255, 256, T - 1) if t < T}
    if row.targets[0] == 'plane':
        _, mx, my = row.targets
        must |= {0, my - 1, (mx - 1) * my, mx * my - 1}
    spread = [int(t) for t in np.unique(np.rint(np.linspace(0, T - 1, MAX_COMPARED)).astype(np.int64))]
    for t in spread[::2] + spread[1::2]:
        if len(must) >= min(T, MAX_COMPARED):
            break
        must.add(t)
    return np.array(sorted(must), dtype=np.int64)


Yardstick = collections.namedtuple('Yardstick', 'at pts El Hl E64 H64 bound_E bound_H eE_ref eH_ref ratio_E64 ratio_H64 q_max')


def yardstick(name, F, Z0=ref.Z0_SI, n_glass=N_GLASS):
    """the long-double sum of the fields ``F`` = (Ex, Ey, Hx, Hy) at the compared targets of a row, the plain-fp64 NumPy sum
    there with its ``max_error`` (e_ref), the bound per target of ``propagate_ref.target_bound`` for E and for H, and the
    fp64 NumPy sum's largest error in units of that bound"""
    row = ROWS[name]
    x, y, pitch = axes(name)
    at = compared(name)
    pts = points(name)[at]
    El, Hl = ref.direct_sum(*F, x, y, WL, n_glass, pts, Z0, real=np.longdouble, pitch=pitch)
    E64, H64 = ref.direct_sum(*F, x, y, WL, n_glass, pts, Z0, pitch=pitch)
    A_E, A_H, Phi, q_max = ref.term_sums(*F, x, y, WL, n_glass, pts, Z0, pitch=pitch)
    bE, bH = ref.target_bound(row.nx * row.ny, Phi, A_E), ref.target_bound(row.nx * row.ny, Phi, A_H)
    return Yardstick(at, pts, El, Hl, E64, H64, bE, bH, ref.max_error(E64, El), ref.max_error(H64, Hl),
                     ref.bound_ratio(E64, El, bE), ref.bound_ratio(H64, Hl, bH), float(q_max.max()))


LENS_R = 60.6e-6          # the outer boundary of the lens of the resident rows, to 0.1 um


def stand_in_fields(name):
    """for a resident row where no GPU synthesises its field: random fields of its shape, exact zeros outside the lens"""
    from test_gpu_fft import fields
    row = ROWS[name]
    x, y, _ = axes(name)
    inside = np.hypot(x[:, None], y[None, :]) <= LENS_R
    return [f * inside for f in fields(row.nx, row.ny, row.nx + row.ny)]


def row_firsts(F):
    """per aperture row the extent the kernel may skip to, from the fields themselves: min(j, ny - 1 - j) over the samples
    that are not exact zeros in all four fields (nearfield.hip row_extent_kernel), None for a row of zeros"""
    live = np.zeros(F[0].shape, dtype=bool)
    for f in F:
        live |= np.asarray(f) != 0
    ny = live.shape[1]
    out = []
    for r in live:
        j = np.flatnonzero(r)
        out.append(None if j.size == 0 else int(min(j[0], ny - 1 - j[-1])))
    return out


def claims_shown(F, splits):
    """which of the field-state claims the fields ``F`` show for workgroups that sum the rows s, s + splits, ..."""
    first = row_firsts(F)
    nx, ny = F[0].shape
    out = set()
    if any(f is not None and f > 0 and ny - 2 * f > TILE for f in first):
        out.add(EXTENT_SPAN)
    for s in range(min(splits, nx)):
        mine = [first[i] is not None for i in range(s, nx, splits)]
        if len(mine) > 1 and not mine[0] and any(mine[1:]):
            out.add(SKIP_THEN_LIVE)
        if any(a and not b for a, b in zip(mine, mine[1:])):
            out.add(LIVE_THEN_SKIP)
    return out


# ---- what a row reaches ------------------------------------------------------------------------------------------------
def nearest_kR(name):
    """the smallest k R over the samples and the compared targets of a row"""
    x, y, _ = axes(name)
    p = points(name)[compared(name)]
    R = np.sqrt((p[:, 0, None, None] - x[None, :, None]) ** 2 + (p[:, 1, None, None] - y[None, None, :]) ** 2 + p[:, 2, None, None] ** 2)
    return float(K * R.min())


def exactly_above(name):
    """the compared targets (flat) for which the kernel's own dx = fma(-i, dx', x - x0) and dy are 0 for one sample (i, j): in
    rationals from the doubles the plan takes"""
    row = ROWS[name]
    x, y, (dxp, dyp) = axes(name)
    F = fractions.Fraction
    out = []
    p = points(name)
    for t in compared(name):
        tx, ty = float(p[t, 0] - x[0]), float(p[t, 1] - y[0])          # what ml_propagate_plan stores
        if any(F(tx) == i * F(dxp) for i in range(row.nx)) and any(F(ty) == j * F(dyp) for j in range(row.ny)):
            out.append(int(t))
    return out


def reach(name):
    row = ROWS[name]
    e, T = row.expect, n_targets(row)
    out = {KERNEL % ('true' if h == 'EH' else 'false', row.sets) for h in row.want_h}
    if e.splits == row.nx:
        out.add('splits == nx')
    elif e.rows_min < e.rows_max:
        out.add('splits < nx, rows_min < rows_max')
    if e.rows_max >= 3:
        out.add('rows_max >= 3')
    if e.splits == 2:
        out.add('splits == 2')
    if e.splits == 1 and e.tiles >= BLOCKS and row.nx > 1:
        out.add('splits == 1 by the tile count, nx > 1')
    ny = row.ny
    for label, hit in (('ny <= 64', ny <= 64), ('64 < ny < 128', 64 < ny < 128), ('ny == 128', ny == 128), ('ny == 129', ny == 129),
                       ('ny of exactly two tiles', ny == 2 * TILE), ('ny of two tiles and a tail', 2 * TILE < ny < 3 * TILE)):
        if hit:
            out.add(label)
    if T in (1, 64, 65, 256, 257):
        out.add('T == %d' % T)
    if row.nx == 1 or row.ny == 1:
        out.add('an axis of one sample')
    if row.state == 'resident':
        out |= set(row.claims)
    else:
        out.add('uploaded: no extents')
    if row.targets[0] == 'near':
        if nearest_kR(name) < 1:
            out.add('target in the near zone, k R < 1')
        if exactly_above(name):
            out.add('target exactly above a sample, dx = dy = 0')
    return out


def reached_by_the_table():
    out = set()
    for name in ROWS:
        out |= reach(name)
    return out
