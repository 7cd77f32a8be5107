"""The table of far-field power cases (tests/farfield_power_cases.py) and its yardsticks
(tests/farfield_power_ref.py) without a GPU: the elementwise projection equals the oracle's bit for bit on a tensor
grid, every claim the table makes about its rows holds in NumPy, the inventory names a row for both arms of every
branch, FOLDED takes the route it is chosen for (tools/transform_route), and the sweep sums agree with
metalens_amd/postprocess.py to what the different grouping of the cell allows."""
import math

import numpy as np
import pytest

import farfield_power_cases as cases
import farfield_power_ref as ref
from test_transform_route import route  # noqa: F401  (the fixture that builds and runs the tool)

U = 2.0 ** -53


def _vectors(shape, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(shape) + 1j * rng.standard_normal(shape) for _ in range(4)]


def test_project_points_is_the_oracle_elementwise():
    """on the tensor grid of RIM's axes - every class of direction among its points - P and both amplitudes have the
    oracle's bits, NaN included"""
    from oracle import farfield_oracle
    ux, uy = cases.rim_axes()
    V = _vectors((ux.size, uy.size), 1)
    want = farfield_oracle.project(*V, ux, uy, cases.WL, cases.N_GLASS, cases.Z0, return_amplitudes=True)
    UX, UY = np.meshgrid(ux, uy, indexing='ij')
    got = ref.project_points(*V, UX, UY, cases.WL, cases.N_GLASS, cases.Z0)
    for g, w in zip(got[:3], want):
        assert np.array_equal(g, w, equal_nan=True)
    assert set(cases.classify(UX, UY).ravel()) == {'uz0', 'tiny', 'nan', 'zero', 'interior'}
    # the power alone, from those amplitudes: the same bits again
    P = ref.power_from_amplitudes(got[1], got[2], UX, UY, cases.WL, cases.N_GLASS, cases.Z0)
    assert np.array_equal(P, want[0], equal_nan=True)
    # the term magnitudes bound the amplitudes they belong to
    ok = ~np.isnan(want[0])
    for a, mag in ((got[1], got[3]), (got[2], got[4])):
        assert np.all(np.abs(a.real[ok]) <= mag.real[ok] * (1 + 4 * U)) and np.all(np.abs(a.imag[ok]) <= mag.imag[ok] * (1 + 4 * U))


def test_rim_directions_are_what_the_table_says():
    ux, uy, classes = cases.rim()
    assert ux.size == 64 and len(set(zip(ux.tolist(), uy.tolist()))) >= 63   # ((0, 0) and (-0.0, 0.0) compare equal)
    assert list(cases.classify(ux, uy)) == classes
    counts = {c: classes.count(c) for c in set(classes)}
    assert counts == {'uz0': 14, 'tiny': 12, 'nan': 10, 'zero': 2, 'interior': 4 + cases.RIM_SEEDED}
    uz2 = 1 - ux ** 2 - uy ** 2
    at = {(x, y): v for x, y, v in zip(ux.tolist(), uy.tolist(), uz2.tolist())}
    assert at[(0.28, 0.96)] == 0 and at[(0.1, 0.99 ** 0.5)] == 0 and at[(8 / 17, 15 / 17)] == 0
    assert at[(0.96, 0.28)] == 2.0 ** -56 and abs(at[(0.96, 0.28)] - 1.4e-17) < 1e-18
    assert at[(0.6, 0.8)] == -2.0 ** -53
    assert at[(1.0, 0.0)] == 0 and at[(0.0, 1.0)] == 0 and at[(1.0, 1e-8)] < 0
    # what one fused multiply-add would make of the first two (the exact product in place of the rounded one):
    # positive, and negative
    from fractions import Fraction
    for (x, y), sign in (((0.28, 0.96), 1), ((0.1, 0.99 ** 0.5), -1)):
        fused = Fraction(1 - x * x) - Fraction(y) * Fraction(y)
        assert fused * sign > 0 and abs(fused) < 1e-16
    shift = 1 - 1e-5 / (math.sqrt(4.3e-17) + 1e-5)      # of P at (0.28, 0.96), relative
    assert 6e-4 < shift < 7e-4
    # the yardstick at these directions: NaN where the table says, finite elsewhere; next to the axis the amplitudes
    # are NOT the vectors
    V = _vectors(ux.shape, 2)
    P, a_theta, a_phi = ref.project_points(*V, ux, uy, cases.WL, cases.N_GLASS, cases.Z0)[:3]
    nan = np.array([c == 'nan' for c in classes])
    for a in (P, a_theta.real, a_theta.imag, a_phi.real, a_phi.imag):
        assert np.array_equal(np.isnan(a), nan)
    Z = cases.Z0 / cases.N_GLASS
    for k, c in enumerate(classes):
        assert (a_theta[k] == V[3][k] + Z * V[0][k]) == (c == 'zero'), k


def test_rim_axes_fill_two_column_blocks():
    ux, uy = cases.rim_axes()
    assert (ux.size, uy.size) == (19, 261) and -(-uy.size // 256) == 2 and uy.size - 256 == 5
    UX, UY = np.meshgrid(ux, uy, indexing='ij')
    cls = cases.classify(UX, UY)
    assert {'uz0', 'tiny', 'nan'} <= set(cls[:, 256:].ravel())      # the short block holds rim directions
    rux, ruy, _ = cases.rim()
    assert set(np.abs(rux[:-cases.RIM_SEEDED]).tolist()) == set(np.abs(ux).tolist())
    assert set(ruy[:-cases.RIM_SEEDED].tolist()) <= set(uy.tolist())


def test_folded_takes_the_fused_kernel_with_slabs(route):  # noqa: F811
    nx, ny, mx, my = cases.FOLDED.shape
    ux, uy = cases.folded_axes()
    for u, m in ((ux, mx), (uy, my)):
        assert m % 2 == 1 and m % 8 != 0 and np.array_equal(u, -u[::-1]) and u[m // 2] == 0 and u[-1] == 0.9
    UX, UY = np.meshgrid(ux, uy, indexing='ij')
    cls = cases.classify(UX, UY)
    assert cls[0, 0] == cls[-1, -1] == cls[0, -1] == 'nan' and cls[mx // 2, my // 2] == 'zero'
    assert (mx + 7) // 8 * 8 - mx == 5 and (my + 7) // 8 * 8 - my == 3        # idle lanes in the last tiles

    def kinds(r):
        return (r['stage1'], r['stage2'], int(r['stage2_splits']))
    assert kinds(route(**cases.folded_plan_facts())) == cases.FOLDED.expect_whole
    assert cases.FOLDED.expect_whole[2] >= 2
    for piece, expect in zip(cases.FOLDED.pieces, cases.FOLDED.expect_pieces):
        assert kinds(route(**cases.folded_plan_facts(piece))) == expect
    # the pieces are uneven and cover every row once
    rows = np.concatenate([cases.mirrored_rows(nx, *p) for p in cases.FOLDED.pieces])
    assert sorted(rows.tolist()) == list(range(nx)) and cases.FOLDED.pieces[0][1] != cases.FOLDED.pieces[1][1]
    # a plain block of rows would leave nothing pending: the generic stage 2
    for row0, nxl in cases.FOLDED.blocks:
        r = route(**dict(cases.folded_plan_facts(), nxl=nxl, row0=row0))
        assert (r['stage1'], r['stage2']) == ('folded', 'generic')
    assert sum(b[1] for b in cases.FOLDED.blocks) == nx and cases.FOLDED.blocks[1][0] == cases.FOLDED.blocks[0][1]


def _row_P(row, seed=3):
    """a stand-in power map of the row's shape: positive, NaN outside the unit circle"""
    rng = np.random.default_rng(seed)
    if row.kind == 'pairs':
        UX, UY = row.ux, row.uy
    else:
        UX, UY = np.meshgrid(row.ux, row.uy, indexing='ij')
    P = rng.uniform(0.1, 2.0, UX.shape) / (1.0001 - np.minimum(UX ** 2 + UY ** 2, 1.0))
    P[1 - UX ** 2 - UY ** 2 < 0] = np.nan
    return P


@pytest.mark.parametrize('name', sorted(cases.SUM_ROWS))
def test_sum_rows_are_what_the_table_says(name):
    row = cases.SUM_ROWS[name]
    pair = row.kind == 'pairs'
    n = row.ux.size if pair else row.ux.size * row.uy.size
    P = _row_P(row)
    s = ref.sweep_sums(P, row.ux, row.uy, pair, row.cone[0], row.cone[1:])
    claims = row.claims
    if 'blocks' in claims:
        assert (-(-n // 256), n - (n - 1) // 256 * 256) == (claims['blocks'], claims['last'])
    assert np.isnan(P).any() == claims['nan']
    assert 0 < s['inside'] <= n and 0 < s['cone'] <= s['total']
    if 'inside' in claims:
        assert (s['inside'], s['on_edge']) == (claims['inside'], claims['on_edge'])
        # with `<` in place of `<=` the edge directions drop out
        strict = ref.cone_masks(row.ux, row.uy, pair, row.cone[0], row.cone[1:])
        assert int((strict[0] & ~strict[1]).sum()) == 69
    if name == 'two-rounds':
        assert ref.sum_bound_units(n) == 8 + 1 + 8 and s['inside'] < n
    else:
        assert ref.sum_bound_units(n) == 16
    # the cell: an axis of one direction counts 1, a pair list has none
    want_cell = 1.0 if pair else (row.ux[1] - row.ux[0] if row.ux.size > 1 else 1.0) * (row.uy[1] - row.uy[0] if row.uy.size > 1 else 1.0)
    assert s['cell'] == want_cell
    if name == 'pairs':
        assert np.isnan(P).any() and not np.isnan(P).all()


def test_weights_row_reaches_what_it_names():
    calls = [c for seq in cases.WEIGHTS_CALLS for c in seq]
    assert {c[1] for c in calls} >= {1.0, -0.5, 0.0} and {c[2] for c in calls} == {0, 1, cases.MAX_SLOTS - 1}
    for seq in cases.WEIGHTS_CALLS:
        assert seq[0][3] == 1                                       # every sequence starts a new sum
    assert any(c[3] for c in cases.WEIGHTS_CALLS[1][1:-1])          # a reset in the middle of the second
    ux, uy = cases.WEIGHTS_GRID
    UX, UY = np.meshgrid(ux, uy, indexing='ij')
    assert 'nan' in set(cases.classify(UX, UY).ravel())
    # p_sum: NaN stays NaN under a weight of 0, and a reset forgets what was there
    maps = [_row_P(cases.SumRow('grid', ux, uy, cases.WEIGHTS_CONE, {}), seed=k) for k in range(3)]
    seq = cases.WEIGHTS_CALLS[1]
    got = ref.p_sum([maps[c[0]] for c in seq], [c[1] for c in seq], [c[3] for c in seq])
    nan = np.isnan(maps[0])
    assert np.array_equal(np.isnan(got), nan) and nan.any()
    assert np.array_equal(got[~nan], (0.25 * maps[1] + 0.0 * maps[2])[~nan])


def test_the_inventory_names_rows_that_exist():
    _, _, classes = cases.rim()
    for what, (part, key) in cases.INVENTORY.items():
        if part == 'RIM':
            assert key in ('pairs', 'axes') or key in classes, what
        elif part == 'FOLDED':
            assert key in ('whole', 'pieces', 'blocks'), what
        else:
            assert part == 'SUM' and (key == 'weights' or key in cases.SUM_ROWS), what
    named = {v for v in cases.INVENTORY.values()}
    # both arms of every branch and every edge listed for this back end
    assert {('RIM', c) for c in ('uz0', 'tiny', 'nan', 'zero', 'interior', 'pairs', 'axes')} <= named
    assert {('FOLDED', 'whole'), ('FOLDED', 'pieces')} <= named
    assert {('SUM', k) for k in list(cases.SUM_ROWS) + ['weights']} <= named
    keys = ' '.join(cases.INVENTORY)
    for arm in ('isfinite false', 'isfinite true', '<= against <', 'pair list', 'mx = 1', 'my = 1', 'more than 256 blocks',
                'fewer than 256 blocks', 'accumulate', 'bit-equal', 'stage 1 + stage 2', 'never written', 'P_sum untouched'):
        assert arm in keys, arm


@pytest.mark.parametrize('name', sorted(k for k, r in cases.SUM_ROWS.items() if r.kind == 'grid'))   # (tensor grids)
def test_sweep_sums_against_postprocess(name):
    """postprocess groups (P * dux) * duy, the library and sweep_sums P * (dux * duy): per term the two differ by at
    most 3 roundings (two products against one product of a rounded cell), 3 * 2**-53 relative, and so do the sums of
    non-negative terms; that is the bound.  (postprocess adds with NumPy's pairwise sum, sweep_sums with math.fsum;
    on these rows the two sums differ by at most 2.0 units in all, printed below.)  The inclusion counts are equal."""
    from metalens_amd import postprocess
    row = cases.SUM_ROWS[name]
    P = _row_P(row)
    s = ref.sweep_sums(P, row.ux, row.uy, False, row.cone[0], row.cone[1:])
    dux = row.ux[1] - row.ux[0] if row.ux.size > 1 else 1.0
    duy = row.uy[1] - row.uy[0] if row.uy.size > 1 else 1.0
    total = postprocess.total_power(P, dux, duy)
    cone = postprocess.encircled_power(P, row.ux, row.uy, dux, duy, sin_max=row.cone[0], center=row.cone[1:])
    units = 3
    print('%s: total off by %.2f units, cone by %.2f (bound %d)' % (
        name, abs(total - s['total']) / (U * s['total']), abs(cone - s['cone']) / (U * s['cone']), units))
    assert abs(total - s['total']) <= units * U * s['total']
    assert abs(cone - s['cone']) <= units * U * s['cone']
    inside = postprocess._sin2(row.ux - row.cone[1], row.uy - row.cone[2]) <= row.cone[0] * row.cone[0]
    assert int(inside.sum()) == s['inside']
