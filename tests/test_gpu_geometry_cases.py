"""The three discrete decisions of the synthesis on the GPU - ring, sector, nearest centre cell (csrc/nearfield_geometry.hip
sample_geometry) - one point per lane through ml_geometry_probe, against the exact statements of tests/geometry_ref.py at
EVERY point of the case table (tests/geometry_cases.py).  Needs an MI355X.

Every comparison is of integers.  The expected sector is the correctly rounded one, also at the near-tie points where
the oracle's NumPy arctangent says otherwise (profiles/geometry_probe.txt counts them).  Per case the census of `path`
shows that the stage the case was made for really decided: floors that follow from the inputs (a point farther than one
bin width from every cell cannot be settled by the bin runs, a cell's own position is settled by its node, ...), not
from what the kernel returned.  Run with -s for the census lines (``CENSUS ...``)."""
import numpy as np
import pytest

import geometry_cases as gc

pytestmark = pytest.mark.gpu

BITS = (('record', gc.RING_RECORD), ('search', gc.RING_SEARCH), ('exact', gc.SECTOR_EXACT), ('clamped', gc.SECTOR_CLAMPED),
        ('node', gc.CELL_NODE), ('four', gc.CELL_FOUR), ('bins', gc.CELL_BINS), ('more', gc.CELL_MORE), ('grow', gc.CELL_GROW),
        ('tie', gc.TIE))


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


@pytest.fixture
def ctx(ma):
    from metalens_amd import _lib
    return _lib.default_context()


def probe(ctx, x, y, n=None):
    from metalens_amd import _lib
    x, y = _lib.f64(x), _lib.f64(y)
    n = x.size if n is None else n
    ring, pick, path = (np.full(max(n, 1), -7, np.int32) for _ in range(3))
    _lib.check(ctx.lib.ml_geometry_probe(ctx.handle, _lib.dptr(x), _lib.dptr(y), n, _lib.iptr(ring), _lib.iptr(pick),
                                         _lib.iptr(path)))
    return ring, pick, path


def run_case(ctx, name):
    from metalens_amd import packing
    c = gc.case(name)
    packing.upload_layout(ctx, c['S'], c['cells'])
    ring, pick, path = probe(ctx, c['x'], c['y'])
    print('CENSUS %-15s %7d points:' % (name, c['x'].size), ' '.join('%s %d' % (k, ((path & b) != 0).sum()) for k, b in BITS))

    def where(bad):
        return [(c['family'][i], float(c['off'][i]), '%.17g' % c['x'][i], '%.17g' % c['y'][i], int(ring[i]), int(pick[i]),
                 int(c['ring'][i]), int(c['pick'][i]), int(path[i])) for i in np.flatnonzero(bad)[:8]]

    # no point is left out
    bad = ring != c['ring']
    assert not bad.any(), ('ring', name, int(bad.sum()), where(bad))
    bad = pick != c['pick']
    assert not bad.any(), ('pick', name, int(bad.sum()), where(bad))
    bad = ((path & gc.TIE) != 0) != c['tie']
    assert not bad.any(), ('tie', name, int(bad.sum()), where(bad))
    one_ring_bit = ((path & gc.RING_RECORD) != 0) ^ ((path & gc.RING_SEARCH) != 0)
    assert one_ring_bit.all(), (name, where(~one_ring_bit))
    return c, path


def has(path, bit):
    return (path & bit) != 0


@pytest.mark.parametrize('name', gc.RING_CASES)
def test_rings(ctx, name):
    c, path = run_case(ctx, name)
    # the bucket record settles exactly the points its three boundaries bracket (geometry_cases.ring_by_record)
    assert np.array_equal(has(path, gc.RING_RECORD), gc.ring_by_record(c['L']['boundaries'], c['r']))
    if name == 'narrow-rings':
        assert has(path, gc.RING_SEARCH).sum() >= 100
    else:
        assert not has(path, gc.RING_SEARCH).any()
    assert not has(path, gc.SECTOR_CLAMPED | gc.TIE).any()
    assert not has(path[~c['on_ring']], gc.SECTOR_EXACT).any()


@pytest.mark.parametrize('name', gc.SECTOR_CASES)
def test_sectors(ctx, name):
    c, path = run_case(ctx, name)
    near = c['family'] == 'tie'
    inside, outside = near & (np.abs(c['off']) <= 0.99e-9), near & (np.abs(c['off']) >= 1.01e-9)
    assert inside.sum() == 13 * outside.sum() // 4 > 0
    assert has(path[inside], gc.SECTOR_EXACT).all() and not has(path[outside], gc.SECTOR_EXACT).any()
    # half = ceil(pi / dphi) + 1 lies beyond every sector a point can have: the clamps never act
    assert not has(path, gc.SECTOR_CLAMPED).any()
    # on the diagonals phi / dphi = N / 8: an exact tie where N = 4 mod 8
    N = np.rint(2 * np.pi / c['L']['dphi'][c['ring'] - 1]).astype(int)
    diag = c['family'] == 'diagonal'
    assert has(path[diag & (N % 8 == 4)], gc.SECTOR_EXACT).all() and not has(path[diag & (N % 8 != 4)], gc.SECTOR_EXACT).any()
    if name == 'odd-sectors':
        assert (diag & (N % 8 == 4)).sum() > 100
        # +-pi is a sector boundary where N is odd: (-x, +0.0) and (-x, -0.0) lie on either side of it
        axes = (c['family'] == 'axes') & (N % 2 == 1) & (c['x'] < 0) & (c['y'] == 0)
        assert axes.sum() == 4 and has(path[axes], gc.SECTOR_EXACT).all()
        for n in (45, 7001):
            up, down = c['pick'][axes & (N == n) & ~np.signbit(c['y'])], c['pick'][axes & (N == n) & np.signbit(c['y'])]
            assert up.size == down.size == 1 and up[0] == -down[0] and up[0] in (n // 2, n // 2 + 1)


@pytest.mark.parametrize('name', gc.CELL_CASES)
def test_cells(ctx, name):
    c, path = run_case(ctx, name)
    kind = name.split('-')[1]
    cell_bits = gc.CELL_NODE | gc.CELL_FOUR | gc.CELL_BINS | gc.CELL_MORE | gc.CELL_GROW
    assert not has(path, gc.SECTOR_EXACT | gc.SECTOR_CLAMPED | gc.RING_SEARCH).any()
    if kind == 'none':
        assert not has(path, cell_bits | gc.TIE).any()
        return
    settled = has(path, gc.CELL_NODE).astype(int) + has(path, gc.CELL_FOUR) + has(path, gc.CELL_BINS) + has(path, gc.CELL_GROW)
    assert (settled == 1).all()                                         # one stage settles a point
    own = c['family'] == 'centre'
    if kind in ('hex', 'shuffled', 'holes'):
        # a cell's own position is settled by its node; an exact tie never is (the pick demands a margin) and goes to
        # the four nodes around it (at the lattice's rim, where corners are missing, beyond them)
        assert has(path[own], gc.CELL_NODE).all()
        assert c['tie'].sum() >= 50 and not has(path[c['tie']], gc.CELL_NODE).any()
        assert has(path[c['tie']], gc.CELL_FOUR).sum() >= 50
        if kind == 'holes':                                             # an empty node settles nothing
            assert not has(path[c['family'] == 'hole'], gc.CELL_NODE).any()
    if kind in ('jitter', 'cluster', 'sparse', 'one'):                  # no lattice: the bins or the growing search
        assert not has(path, gc.CELL_NODE | gc.CELL_FOUR).any()
        assert has(path[own], gc.CELL_BINS).all()                       # distance 0 is within one bin width
    if kind == 'jitter':
        assert has(path, gc.CELL_BINS).sum() >= 1000
    if kind == 'cluster':
        # the knot's bin holds twelve cells: at their own positions the runs are longer than a batch of four
        knot = own & np.isin(c['pick'], np.arange(len(c['cells']) - 14, len(c['cells']) - 2))
        assert knot.sum() == 12 and has(path[knot], gc.CELL_MORE).all()
    if kind == 'sparse':
        must = gc.grow_certain(c)
        assert must.sum() >= 100 and has(path[must], gc.CELL_GROW).all()
    if kind == 'one':
        assert has(path, gc.CELL_BINS).all() and (c['pick'] == 0).all()


def test_probe_leaves_the_context_alone(ma, ctx):
    """a synthesis in its steady state, the probe, the same synthesis again: fields and power bit-equal, pending ties and the kernels the
    synthesis reports unchanged"""
    from metalens_amd import _lib, ties
    lens = gc.lens('small')
    c = gc.case('cells-hex')
    pitch = gc.WL / 2.2
    x = (np.arange(96) - 47.5) * pitch + 0.16e-6                         # x = 0 is no sample, but the hexagons' mirror lines are met
    y = (np.arange(80) - 40) * pitch
    args = (0.2e-6, -0.1e-6, -lens['source_distance'], 'x', gc.WL, lens['lens_periphery_summary'], lens['lens_center_summary'],
            lens['hexgridset'])
    ma.build_nearfield(*args, x_pts=x, y_pts=y, ctx=ctx)
    # (the second synthesis on a geometry is the steady state: launched from the patch lists, with the forms it keeps)
    first = ma.build_nearfield(*args, x_pts=x, y_pts=y, ctx=ctx)
    before = (ties.pending(ctx).tolist(), ctx.nearfield_kernels(), ctx.synth_forms())
    pick = np.random.default_rng(3).choice(c['x'].size, 1000, replace=False)
    pick[:50] = np.flatnonzero(c['tie'])[:50]                              # ties among them: the probe's own scratch takes them
    ring, got, path = probe(ctx, c['x'][pick], c['y'][pick])
    assert np.array_equal(ring, c['ring'][pick]) and np.array_equal(got, c['pick'][pick])
    assert np.array_equal(has(path, gc.TIE), c['tie'][pick])
    assert (ties.pending(ctx).tolist(), ctx.nearfield_kernels(), ctx.synth_forms()) == before
    F = [np.empty((x.size, y.size), dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    for a, b in zip(F, first[:4]):
        assert np.array_equal(a, b)                                         # the resident fields were not touched
    again = ma.build_nearfield(*args, x_pts=x, y_pts=y, ctx=ctx)
    for a, b in zip(first[:4], again[:4]):
        assert np.array_equal(a, b)
    assert first[6] == again[6]
    assert (ties.pending(ctx).tolist(), ctx.nearfield_kernels(), ctx.synth_forms()) == before


def test_refusals(ctx):
    from metalens_amd import _lib, packing
    c = gc.case('cells-one')
    packing.upload_layout(ctx, c['S'], c['cells'])
    x = np.array([0.0, 1e-6, 2e-6, 3e-6])
    out = np.zeros(4, np.int32)
    lib, h = ctx.lib, ctx.handle
    args = (_lib.dptr(x), _lib.dptr(x), 4, _lib.iptr(out), _lib.iptr(out), _lib.iptr(out))
    for k in (0, 1, 3, 4, 5):
        with pytest.raises(_lib.MetalensHipError, match='NULL argument'):
            _lib.check(lib.ml_geometry_probe(h, *[None if i == k else a for i, a in enumerate(args)]))
    with pytest.raises(_lib.MetalensHipError, match='NULL argument'):
        _lib.check(lib.ml_geometry_probe(None, *args))
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(_lib.MetalensHipError, match='1 ... 2\\^20'):
            _lib.check(lib.ml_geometry_probe(h, args[0], args[1], n, *args[3:]))
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[2] = bad
        with pytest.raises(_lib.MetalensHipError, match='point 2 is not finite'):
            _lib.check(lib.ml_geometry_probe(h, _lib.dptr(xb), args[1], 4, *args[3:]))
        with pytest.raises(_lib.MetalensHipError, match='point 2 is not finite'):
            _lib.check(lib.ml_geometry_probe(h, args[0], _lib.dptr(xb), 4, *args[3:]))
    assert not out.any()                                                    # nothing was launched
    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.MetalensHipError, match='ml_upload_layout has not been called'):
            _lib.check(fresh.lib.ml_geometry_probe(fresh.handle, *args))
    finally:
        fresh.close()
    ring, pick, path = probe(ctx, x, x)                                     # and the context still answers
    assert (ring == 0).all() and (pick == 0).all()
