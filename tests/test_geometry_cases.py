"""The case table of the synthesis decisions (tests/geometry_cases.py) checked on its own, without a GPU: its sizes, that
every edge has points on each side, that the hexagonal set meets exact ties, that the restated bucket and bin rules are
the packers' own, that the fast nearest-cell reference is the brute force, and the census of where the oracle's NumPy
arctangent departs from the correctly rounded one - which it may only do closer than 1e-12 sectors to a tie and never on
the axes and diagonals.  The census goes to profiles/geometry_probe.txt."""
import os

import numpy as np
import pytest

import geometry_cases as gc
import geometry_ref as ref
from test_lens_pack import pack_lens, tool   # noqa: F401  (the host tool of lens_pack.h, a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sizes():
    mp = 0
    for name in gc.CASES:
        c = gc.case(name)
        assert 0 < c['x'].size <= gc.CASE_POINT_CAP, name
        assert np.isfinite(c['x']).all() and np.isfinite(c['y']).all(), name
        mp += c['mp_points']
    assert mp <= gc.MP_POINT_CAP
    B = gc.case('na094-rings')['L']['boundaries']
    edges = set(gc.case('na094-rings')['edge'][np.isin(gc.case('na094-rings')['family'], ('axis', 'oblique'))].tolist())
    k = int(np.diff(B).argmin())
    assert len(edges) == 512 and {0, B.size - 1, k, k + 1} <= edges
    for name in gc.RING_CASES:
        c = gc.case(name)
        n_edges = len(set(c['edge'][c['family'] == 'axis'].tolist()))
        assert n_edges == min(c['L']['boundaries'].size, 512), name
        assert len(set(c['edge'][c['family'] == 'bucket'].tolist())) == 256 and (c['family'] == 'extreme').sum() == 5, name
    for name in gc.SECTOR_CASES:
        c = gc.case(name)
        n_dphi = min(np.unique(c['L']['dphi']).size, 8)
        assert (c['family'] == 'tie').sum() == n_dphi * 22 * 17 and (c['family'] == 'axes').sum() == 8 * n_dphi, name
        assert (c['family'] == 'diagonal').sum() == 500 * 12 and c['on_ring'].all(), name
    assert np.unique(gc.case('odd-sectors')['L']['dphi']).size == 6
    for name in gc.CELL_CASES:
        c = gc.case(name)
        assert (c['ring'] == 0).all() and 9000 < (c['family'] == 'random').sum() <= 10000 and (c['family'] == 'rim').sum() == 1, name
        if c['cells'] is not None and len(c['cells']) > 1:
            assert (c['family'] == 'bin').sum() > 256, name
    assert len(gc.case('cells-sparse')['cells']) == 7 and len(gc.case('cells-one')['cells']) == 1
    assert (gc.case('cells-holes')['family'] == 'hole').sum() > 500
    knot = gc.case('cells-cluster')['cells'][-14:-2, :2]
    assert np.ptp(knot, axis=0).max() <= 0.2 * gc.PITCH and np.array_equal(*gc.case('cells-cluster')['cells'][-2:, :2])


@pytest.mark.parametrize('name', gc.RING_CASES)
def test_ring_edges_have_points_on_each_side(name):
    c = gc.case(name)
    B = c['L']['boundaries']
    n_edges, found = 0, 0
    for fam in ('axis', 'oblique'):
        sel = c['family'] == fam
        for k in set(c['edge'][sel].tolist()):
            r = c['r'][sel & (c['edge'] == k)]
            n_edges += 1
            ok = (r < B[k]).any() and (r == B[k]).any() and (r > B[k]).any()
            found += ok
            assert ok or fam == 'oblique', (name, fam, k)
    # (an oblique triple exists where the search over the neighbouring fp64 points finds it: nearly everywhere)
    assert found >= 0.95 * n_edges
    nb, hb = gc.record_buckets(B)
    sel = c['family'] == 'bucket'
    for b in set(c['edge'][sel].tolist()):
        r = c['r'][sel & (c['edge'] == b)]
        assert (r < b * hb).any() and (r == b * hb).any() and (r > b * hb).any()
    # both answers of searchsorted at an edge, and the three regions
    assert {0, B.size} <= set(c['ring'].tolist()) and c['on_ring'].sum() > 100
    if name == 'narrow-rings':
        assert nb == 65536 and 2 * B[-1] / np.diff(B)[np.diff(B) > 0].min() > 65536 and (np.diff(B) == 0).sum() == 1
        assert (~gc.ring_by_record(B, c['r'])).sum() >= 100        # what the GPU test's floor rests on
    else:
        assert gc.ring_by_record(B, c['r']).all()


@pytest.mark.parametrize('name', gc.SECTOR_CASES)
def test_sector_points_lie_where_they_say(name):
    """the signed distance to the nearest tie, worked out exactly from the fp64 coordinates, is the nominal offset to
    within the rounding of the coordinates: the points of |off| <= 0.99e-9 lie inside the kernel's tie window, those of
    |off| >= 1.01e-9 outside, each by more than the fast arctangent's error (a few 1e-12 sectors at the finest dphi)"""
    c = gc.case(name)
    sel = c['family'] == 'tie'
    at = c['ring'][sel] - 1
    assert np.array_equal(at, c['edge'][sel])                       # every point on the ring it was made for
    eff = ref.tie_distance(c['x'][sel], c['y'][sel], c['L']['dphi'][at])
    off = c['off'][sel]
    assert np.abs(eff - off).max() < 5e-12
    assert (np.abs(eff[np.abs(off) <= 0.99e-9]) < 0.995e-9).all() and (np.abs(eff[np.abs(off) >= 1.01e-9]) > 1.005e-9).all()
    # both sides of every tie: the offsets of either sign round to neighbouring sectors
    pick = c['pick'][sel].reshape(-1, 17)
    lo, hi = pick[:, 2::2], pick[:, 1::2]                           # off < 0, off > 0 (geometry_cases.sector_points)
    N = np.rint(2 * np.pi / c['L']['dphi'][at]).astype(int).reshape(-1, 17)[:, :1]
    wide = slice(-3, None)                                          # |off| = 0.99e-9, 1.01e-9, 1e-6: far beyond the coordinates' rounding
    assert ((hi[:, wide] - lo[:, wide] == 1) | (hi[:, wide] - lo[:, wide] == 1 - N)).all()      # (1 - N: across +-pi, N odd)


@pytest.mark.parametrize('name', gc.CELL_CASES)
def test_cell_points(name):
    c = gc.case(name)
    cells = c['cells']
    if cells is None:
        assert (c['pick'] == -1).all()
        return
    # the reference that finds its candidates through the tree IS the brute force over all cells
    sub = slice(0, None, 16)
    idx, tie = ref.nearest_cell_brute(c['x'][sub], c['y'][sub], cells)
    assert np.array_equal(idx, c['pick'][sub]) and np.array_equal(tie, c['tie'][sub])
    centre = c['family'] == 'centre'                                   # a cell's own position picks that cell (or its twin)
    assert np.array_equal(cells[c['pick'][centre], :2], np.column_stack((c['x'][centre], c['y'][centre])))
    if name == 'cells-hex':
        assert c['tie'].sum() >= 50
    if len(cells) > 7:
        # the midpoints' neighbours of +-1 ulp decide differently from one another: both sides of the edge between two cells
        mid = c['pick'][c['family'] == 'midpoint']
        assert len(np.unique(mid)) > 0.9 * (c['family'] == 'centre').sum()
        # bin edges: the neighbours of -1 and +1 ulp lie in different bins
        bx, by, x0, y0, h = gc.cell_bins(cells)
        sel = c['family'] == 'bin'
        bins = np.floor((c['x'][sel] - x0) / h) * (by + 2) + np.floor((c['y'][sel] - y0) / h)
        assert len(np.unique(bins)) > 256
    if name == 'cells-cluster':
        assert c['tie'][(c['x'] == -5.013e-6) & (c['y'] == 4.021e-6)].all()          # the two identical cells
    if name == 'cells-sparse':
        assert gc.grow_certain(c).sum() >= 100


def test_restated_bucket_and_bin_rules_are_the_packers(tool):   # noqa: F811
    small = gc.lens('small')
    for name in ('small-rings', 'narrow-rings'):
        S, _ = gc.layout(name)
        tables, centre, layout = pack_lens(S, small['lens_center_summary'], small['hexgridset'], 580)
        got = tool(tables, centre, layout)
        nb, hb = gc.record_buckets(layout['boundaries'])
        assert (got['lutrec_buckets'][0], got['lutrec_inv_h'][0]) == (nb, 1.0 / hb), name
    for kind in ('hex', 'jitter', 'cluster', 'sparse', 'one'):
        S, cells = gc.layout('cells-' + kind)
        tables, centre, layout = pack_lens(S, cells, small['hexgridset'], 580)
        got = tool(tables, centre, layout)
        bx, by, x0, y0, h = gc.cell_bins(cells)
        assert (got['bins_x'][0], got['bins_y'][0], got['bin_x0'][0], got['bin_y0'][0], got['bin_h'][0]) == (bx, by, x0, y0, h), kind


def test_census_of_numpy_against_correctly_rounded():
    lines = ['census of round(np.arctan2(y, x) / dphi) against the correctly rounded decision (tests/geometry_ref.py)',
             'numpy %s; points that differ / points, per case and nominal |off| in sectors' % np.__version__]
    for name in gc.SECTOR_CASES:
        c = gc.case(name)
        differ = c['pick'] != c['numpy_sector']
        where = ['%s (%.17g, %.17g)' % (c['family'][i], c['x'][i], c['y'][i]) for i in np.flatnonzero(differ)[:20]]
        for fam in ('axes', 'diagonal'):
            sel = c['family'] == fam
            lines.append('%-14s %-10s %4d / %d' % (name, fam, differ[sel].sum(), sel.sum()))
            assert not differ[sel].any(), (name, fam, where)
        for off in gc.OFFS:
            sel = (c['family'] == 'tie') & (np.abs(c['off']) == off)
            lines.append('%-14s off %-7.3g %3d / %d' % (name, off, differ[sel].sum(), sel.sum()))
            assert off < 1e-12 or not differ[sel].any(), (name, off, where)
        sector = c['family'] == 'tie'     # (the share among the near-tie points alone: the others never differ)
        share = differ[sector].sum() / sector.sum()
        lines.append('%-14s near-tie   %4d / %d = %.2f %%' % (name, differ[sector].sum(), sector.sum(), 100 * share))
        assert share <= 0.05, (name, share, where)
    for name in gc.RING_CASES:       # the ring cases' points are no near-ties: the two agree
        c = gc.case(name)
        assert np.array_equal(c['pick'], c['numpy_sector']), name
    try:
        with open(os.path.join(ROOT, 'profiles', 'geometry_probe.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')
    except OSError:                  # a read-only checkout: the census above still held
        pass
