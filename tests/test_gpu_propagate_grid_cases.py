"""The rows of tests/propagate_grid_cases.py on the GPU: the launches of csrc/propagate_grid*.hip that no case of
tests/test_gpu_propagate_grid.py, _long, _tiled or _fine reached - columns of 256 and of 4096 (two streaming stages
above blocks of 1024), rows of 512, 1024 and 4096, both axes of 'fft' mid-size at once, its shortest axes, and the
streamed fine plan across more than one batch of tiles - every row as EH and as E.  Needs an MI355X.

Errors and bounds are those of tests/test_gpu_propagate_grid.py: max |difference| over components and targets / max
|field| of the long-double sum (``propagate_ref.max_error``); ``e_ref`` is that error of the plain fp64 direct NumPy sum,
``e_np`` of the NumPy restatement of the row's method.  Parity: ``e_gpu <= 8 e_np`` on the targets of the long-double sum
and ``<= 16 e_np`` against the NumPy form on every target; against ``method='direct'``: ``8 e_np + 8 e_ref``.  The
yardsticks are the NumPy restatement and the long-double sum, never the code under test.  The measured triples are printed
as ``PARITY ...`` lines (run with -s; they belong in profiles/propagate_parity.txt).

The rows are thin or small: a plane is 2 MiB at the most, the largest workspace 30 planes of 4096 x 32."""
import numpy as np
import pytest

import propagate_grid_cases as cases
import propagate_ref as ref
from test_gpu_fft_mixed import _upload

pytestmark = pytest.mark.gpu

WL, N_GLASS = cases.WL, cases.N_GLASS
E_KEYS, H_KEYS = ('Ex', 'Ey', 'Ez'), ('Hx', 'Hy', 'Hz')
SHARED = sorted(n for n, row in cases.ROWS.items() if row.method != 'fft-fine')       # on the default context
STREAMED = sorted(n for n, row in cases.ROWS.items() if row.cache_kernels is False)   # each on a context of its own
assert sorted(SHARED + STREAMED) == sorted(cases.ROWS)


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


@pytest.fixture
def ctx():
    from metalens_amd import _lib
    c = _lib.default_context()
    c.set_method('auto')
    c.set_precision('f64')
    return c


def _stack(out, keys):
    return np.stack([out[k].ravel() for k in keys])


def _contiguous(F):
    return [np.ascontiguousarray(f, dtype=np.complex128) for f in F]


def _propagator(ma, c, name, **kw):
    """the row's own method, tile, pitch ratios and mode unless ``kw`` says otherwise"""
    row, r = cases.ROWS[name], cases.reference(name)
    kw.setdefault('method', row.method)
    if kw['method'] == row.method:
        for key in ('tile', 'subsample', 'cache_kernels'):
            if getattr(row, key) is not None:
                kw.setdefault(key, getattr(row, key))
    return ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], ctx=c, **kw)


def _parity(name, out, want_h):
    """the assertions of tests/test_gpu_propagate_grid.py::test_against_the_long_double_sum"""
    row, r = cases.ROWS[name], cases.reference(name)
    assert out['Ex'].shape == (r['tx'].size, r['ty'].size)
    sub, tag = r['sub'], 'EH' if want_h else 'E'
    for comp, keys, i in (('E', E_KEYS, 0), ('H', H_KEYS, 1))[:2 if want_h else 1]:
        got = _stack(out, keys)
        e = ref.max_error(got[:, sub], r[comp + 'l'])
        print('PARITY %-9s %-15s %-2s %s: e_ref %.3e e_np %.3e gpu %.3e' % (row.method, name, tag, comp, r['e_ref'][i], r['e_np'][i], e))
        e_all = ref.max_error(got, r[comp + 'np'])
        print('PARITY %-9s %-15s %-2s %s against the NumPy form on every target: %.3e (bound %.3e)'
              % (row.method, name, tag, comp, e_all, 16 * r['e_np'][i]))
        assert e <= 8 * r['e_np'][i]
        assert e_all <= 16 * r['e_np'][i]
    assert set(out) == set(E_KEYS + (H_KEYS + ('Sz',) if want_h else ('I',)))


def _planned(name, info, want_h):
    """plan_info against the row's ``expect``: lengths, tiles, batch, lattices, mode.  -> the planes of the workspace"""
    row = cases.ROWS[name]
    nx, ny, mx, my = row.sizes
    expect, outputs = row.expect, 6 if want_h else 3
    want = {'method': row.method, 'Lx': expect.L[0], 'Ly': expect.L[1], 'workspace_bytes': info['workspace_bytes']}
    if row.method == 'fft':
        assert info == want
        return 12 + outputs
    sx, sy = row.subsample or (1, 1)
    m_cx, m_cy = -(-mx // sx), -(-my // sy)
    want.update(tiles=expect.tiles, batch=expect.batch, tile_samples=(expect.L[0] - m_cx + 1, expect.L[1] - m_cy + 1))
    tiles = expect.tiles[0] * expect.tiles[1]
    if row.method == 'fft-tiled':
        assert info == want
        return 8 * tiles + 4 * expect.batch + outputs
    want.update(subsample=row.subsample, lattice_targets=(m_cx, m_cy), cache_kernels=row.cache_kernels)
    assert info == want
    assert (min(sx, mx), min(sy, my)) == expect.lattices
    return 16 * expect.batch + 4 * tiles + 2 * outputs


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('name', SHARED)
def test_against_the_long_double_sum(ma, ctx, name, want_h):
    from metalens_amd.propagate import plan_info
    r, expect = cases.reference(name), cases.ROWS[name].expect
    _upload(ctx, _contiguous(r['F']))
    p = _propagator(ma, ctx, name, want_h=want_h)
    _parity(name, p.propagate(), want_h)
    info = plan_info(ctx)
    planes = _planned(name, info, want_h)
    assert info['workspace_bytes'] >= planes * expect.L[0] * expect.L[1] * 16
    assert info == p.plan_info()


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('name', STREAMED)
def test_streamed_across_batches_against_the_long_double_sum_and_the_cached_plan(ma, name, want_h):
    """cache_kernels=False with more tiles than a batch holds, on a context of its own so that the workspace it reports is
    what this mode reserved - the streamed formula exactly; then the cached plan on the same context: the same bits (as
    tests/test_gpu_propagate_grid_fine.py::test_streamed_kernels_give_the_bits_of_cached_ones for one batch)"""
    from metalens_amd import _lib
    r, expect = cases.reference(name), cases.ROWS[name].expect
    assert expect.tiles[0] * expect.tiles[1] > expect.batch
    c = _lib.Context(0)
    try:
        _upload(c, _contiguous(r['F']))
        p = _propagator(ma, c, name, want_h=want_h)
        streamed, again = p.propagate(), p.propagate()
        _parity(name, streamed, want_h)
        info = p.plan_info()
        planes = _planned(name, info, want_h)
        assert info['workspace_bytes'] == planes * expect.L[0] * expect.L[1] * 16
        q = _propagator(ma, c, name, want_h=want_h, cache_kernels=True)
        cached = q.propagate()
        info = q.plan_info()
        lattices = expect.lattices[0] * expect.lattices[1]
        assert info['cache_kernels'] is True and (info['tiles'], info['batch']) == (expect.tiles, expect.batch)
        cached_planes = (8 * lattices + 4) * expect.tiles[0] * expect.tiles[1] + 2 * (6 if want_h else 3)
        assert info['workspace_bytes'] >= cached_planes * expect.L[0] * expect.L[1] * 16
        assert set(streamed) == set(cached)
        for key in cached:
            assert np.abs(cached[key]).min() > 0, key
            assert np.array_equal(streamed[key], cached[key]) and np.array_equal(streamed[key], again[key]), key
    finally:
        c.close()


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('name', ['k-4096x', 'k-4096y'])
def test_the_long_plan_gives_the_bits_of_fft(ma, ctx, name, want_h):
    """the assertion of tests/test_gpu_propagate_grid_long.py::test_is_the_fft_method_where_both_exist"""
    r, expect = cases.reference(name), cases.ROWS[name].expect
    _upload(ctx, _contiguous(r['F']))
    got = {}
    for method in ('fft', 'fft-long'):
        p = _propagator(ma, ctx, name, want_h=want_h, method=method)
        got[method] = p.propagate(), p.plan_info()
    (a, ia), (b, ib) = got['fft'], got['fft-long']
    assert set(a) == set(b) == set(E_KEYS + (H_KEYS + ('Sz',) if want_h else ('I',)))
    for key in a:
        assert np.abs(a[key]).max() > 0 and np.array_equal(a[key], b[key]), key
    assert ia['method'] == 'fft' and ib['method'] == 'fft-long'
    assert (ia['Lx'], ia['Ly']) == (ib['Lx'], ib['Ly']) == expect.L
    assert ia['workspace_bytes'] == ib['workspace_bytes'] >= (12 + (6 if want_h else 3)) * expect.L[0] * expect.L[1] * 16


@pytest.mark.parametrize('name', ['tk-4096x', 'tk-4096y'])
def test_against_the_direct_method(ma, ctx, name):
    """every target, as tests/test_gpu_propagate_grid_tiled.py::test_against_the_direct_method"""
    r = cases.reference(name)
    _upload(ctx, _contiguous(r['F']))
    tiled = _propagator(ma, ctx, name).propagate()
    direct = _propagator(ma, ctx, name, method='direct').propagate()
    for keys, e_np, e_ref in zip((E_KEYS, H_KEYS), r['e_np'], r['e_ref']):
        d = ref.max_error(_stack(tiled, keys), _stack(direct, keys))
        print('PARITY fft-tiled against direct, %s %s: %.3e (bound %.3e)' % (name, keys[0][0], d, 8 * e_np + 8 * e_ref))
        assert 0 < d <= 8 * e_np + 8 * e_ref
