"""``PlanePropagator(method='fft-tiled')`` on the GPU (csrc/propagate_grid_tiled.hip, ml_propagate_plan_grid_tiled):
the FFT form of the finite-distance propagator by overlap-add over tiles of the aperture.  Needs an MI355X.

Errors and bounds are those of tests/test_gpu_propagate_grid.py: max |difference| over components and targets / max
|field| of the long-double sum; ``e_ref`` is that error of the plain fp64 direct NumPy sum, ``e_np`` of the NumPy tiled
form (tests/propagate_grid_tiled_ref.py).  Parity: ``e_gpu <= 8 e_np`` on the targets of the long-double sum and
``<= 16 e_np`` against the NumPy form on every target; against ``method='direct'``: ``8 e_np + 8 e_ref``.  The yardsticks
are the NumPy restatement and the long-double sum, never the code under test.  The measured triples are printed as
``PARITY ...`` lines (run with -s; they belong in profiles/propagate_parity.txt).

The cases are small or thin: a plane is 1 MB at the most, and the largest plan ('td-many', 330 tiles of 32 x 32) holds
43 MB."""
import numpy as np
import pytest

import propagate_grid_ref as gref
import propagate_grid_tiled_ref as tref
import propagate_ref as ref
from test_gpu_fft_mixed import _upload
from test_gpu_propagate_sets import _check_sums, _lens

pytestmark = pytest.mark.gpu

WL, N_GLASS = gref.WL, gref.N_GLASS
E_KEYS, H_KEYS = ('Ex', 'Ey', 'Ez'), ('Hx', 'Hy', 'Hz')


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


def _propagator(ma, ctx, r, **kw):
    kw.setdefault('method', 'fft-tiled')
    if kw['method'] == 'fft-tiled':
        kw.setdefault('tile', r['tile'])
    return ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], ctx=ctx, **kw)


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', sorted(tref.CASES))
def test_against_the_long_double_sum(ma, ctx, case, want_h):
    r = tref.reference(case)
    _upload(ctx, _contiguous(r['F']))
    p = _propagator(ma, ctx, r, want_h=want_h)
    out = p.propagate()
    assert out['Ex'].shape == (r['tx'].size, r['ty'].size)
    sub = r['sub']
    eE = ref.max_error(_stack(out, E_KEYS)[:, sub], r['El'])
    print('PARITY fft-tiled %-13s %-2s E: e_ref %.3e e_np %.3e gpu %.3e' % (case, 'EH' if want_h else 'E', r['e_ref'][0], r['e_np'][0], eE))
    eE_all = ref.max_error(_stack(out, E_KEYS), r['Enp'])
    print('PARITY fft-tiled %-13s %-2s E against the NumPy form on every target: %.3e (bound %.3e)'
          % (case, 'EH' if want_h else 'E', eE_all, 16 * r['e_np'][0]))
    assert eE <= 8 * r['e_np'][0]
    assert eE_all <= 16 * r['e_np'][0]
    if want_h:
        eH = ref.max_error(_stack(out, H_KEYS)[:, sub], r['Hl'])
        print('PARITY fft-tiled %-13s EH H: e_ref %.3e e_np %.3e gpu %.3e' % (case, r['e_ref'][1], r['e_np'][1], eH))
        eH_all = ref.max_error(_stack(out, H_KEYS), r['Hnp'])
        print('PARITY fft-tiled %-13s EH H against the NumPy form on every target: %.3e (bound %.3e)' % (case, eH_all, 16 * r['e_np'][1]))
        assert eH <= 8 * r['e_np'][1]
        assert eH_all <= 16 * r['e_np'][1]
        assert set(out) == set(E_KEYS + H_KEYS + ('Sz',))
    else:
        assert set(out) == set(E_KEYS + ('I',))
    from metalens_amd.propagate import plan_info
    info, plan = plan_info(ctx), r['plan']
    assert plan['L'] == tref.PLANS[case]['L'] and plan['tiles'] == tref.PLANS[case]['tiles']
    assert info == {'method': 'fft-tiled', 'Lx': plan['L'][0], 'Ly': plan['L'][1], 'workspace_bytes': info['workspace_bytes'],
                    'tiles': plan['tiles'], 'tile_samples': plan['tile_samples'], 'batch': plan['batch']}
    (cx, cy), outputs = plan['tiles'], 6 if want_h else 3
    assert info['workspace_bytes'] >= (8 * cx * cy + 4 * plan['batch'] + outputs) * plan['L'][0] * plan['L'][1] * 16
    assert info == p.plan_info()


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', ['tc-far', 'a-near'])
def test_one_tile_is_the_fft_method(ma, ctx, case, want_h):
    """the default tile of a problem that fits one: the lengths, the planes and the launches of 'fft', and its bits"""
    x, y, tx, ty, z = tref.geometry(case) if case in tref.CASES else gref.geometry(case)
    _upload(ctx, _contiguous(gref.random_fields(x.size, y.size, x.size + y.size)))
    got = {}
    for method in ('fft', 'fft-tiled'):
        p = ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, want_h=want_h, ctx=ctx, method=method)
        got[method] = p.propagate(), p.plan_info()
    (a, ia), (b, ib) = got['fft'], got['fft-tiled']
    assert set(a) == set(b) == set(E_KEYS + (H_KEYS + ('Sz',) if want_h else ('I',)))
    for key in a:
        assert np.abs(a[key]).max() > 0 and np.array_equal(a[key], b[key]), key
    assert ib['method'] == 'fft-tiled' and ib['tiles'] == (1, 1) and ib['batch'] == 1
    assert (ib['Lx'], ib['Ly']) == (ia['Lx'], ia['Ly']) == (gref.padded_length(x.size, tx.size), gref.padded_length(y.size, ty.size))
    assert set(ia) == {'method', 'Lx', 'Ly', 'workspace_bytes'}      # the dicts of the other methods stay as they are


@pytest.mark.parametrize('case', ['tf-beyond', 'td-many'])
def test_against_the_direct_method(ma, ctx, case):
    """every target; 'tf-beyond' is an aperture no other FFT form takes"""
    r = tref.reference(case)
    _upload(ctx, _contiguous(r['F']))
    tiled = _propagator(ma, ctx, r).propagate()
    direct = _propagator(ma, ctx, r, method='direct').propagate()
    if case == 'tf-beyond':
        with pytest.raises(ValueError, match='n = 16500 samples and m = 40 targets to L = 32768 > 16384'):
            _propagator(ma, ctx, r, method='fft-long')
    for keys, e_np, e_ref in zip((E_KEYS, H_KEYS), r['e_np'], r['e_ref']):
        d = ref.max_error(_stack(tiled, keys), _stack(direct, keys))
        print('PARITY fft-tiled against direct, %s %s: %.3e (bound %.3e)' % (case, keys[0][0], d, 8 * e_np + 8 * e_ref))
        assert 0 < d <= 8 * e_np + 8 * e_ref


def test_repeatable_and_linear(ma, ctx):
    r = tref.reference('ta-near')
    F = _contiguous(r['F'])
    p = _propagator(ma, ctx, r)
    _upload(ctx, F)
    a, b = p.propagate(), p.propagate()
    _upload(ctx, [2 * f for f in F])
    c = p.propagate()
    for key in E_KEYS + H_KEYS:
        assert np.abs(a[key]).min() > 0
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(c[key], 2 * a[key]), key


def test_resident_equals_uploaded(ma, ctx):
    """the 512^2 lens of test_gpu_propagate_grid.test_resident_equals_uploaded with tiles of 256 - 40 + 1 = 217 samples,
    2 tiles an axis short of a third: every tile boundary cuts the lens, and the tiles of the corners hold rows whose
    extents leave them empty (samples outside the extents are written as zeros by the padding)"""
    lens = _lens()
    n = 512
    x = (np.arange(n) - (n - 1) / 2) * (WL / 2.2)
    assert x[-1] > lens['lens_periphery_summary']['r_max_list'][-1]
    args = dict(source_x=0.2e-6, source_y=-0.1e-6, source_z=-lens['source_distance'], source_pol='x', wavelength=WL,
                lens_periphery_summary=lens['lens_periphery_summary'], lens_center_summary=lens['lens_center_summary'],
                hexgridset=lens['hexgridset'], x_pts=x, y_pts=x, ctx=ctx)
    _, _, _, _, xs, ys, _, n_glass = ma.build_nearfield(**args, download=False)
    tx, ty = gref.target_axis(xs, 200.3, 32), gref.target_axis(ys, 230.75, 40)
    kw = dict(ctx=ctx, method='fft-tiled', tile=(256, 256))
    resident = ma.field_at_plane(None, None, None, None, xs, ys, WL, n_glass, tx, ty, 20e-6, **kw)
    from metalens_amd.propagate import plan_info
    assert plan_info(ctx)['tiles'] == (3, 3) and plan_info(ctx)['tile_samples'] == (225, 217)
    F = ma.build_nearfield(**args)[:4]
    assert max(np.abs(f[0]).max() for f in F) == 0 and np.abs(F[0]).max() > 0
    uploaded = ma.field_at_plane(*F, xs, ys, WL, n_glass, tx, ty, 20e-6, **kw)
    for key in E_KEYS + H_KEYS + ('Sz',):
        assert resident[key].shape == (32, 40) and np.abs(resident[key]).max() > 0
        assert np.array_equal(resident[key], uploaded[key]), key
    with pytest.raises(ValueError, match='resident near field is 512 x 512'):
        ma.field_at_plane(None, None, None, None, xs[:500], ys, WL, n_glass, tx, ty, 20e-6, **kw)


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_sets_and_sums(ma, ctx, want_h):
    """'td-many' (six batches of tiles per set): the sums of a pass as tests/test_gpu_propagate_sets.py asserts them for
    the direct method, and a pass added twice doubles them exactly"""
    from metalens_amd import _lib
    r = tref.reference('td-many')
    _upload(ctx, _contiguous(r['F']))
    p = _propagator(ma, ctx, r, want_h=want_h)
    with pytest.raises(_lib.MetalensHipError, match='has not run on the active propagation plan'):
        p.sums()
    assert p.queue_sets(0, 1) == 1
    fields = p._download(0)
    single = p.propagate()
    for key in fields:
        assert np.array_equal(fields[key], single[key]), key
    w = 1.5
    with pytest.raises(_lib.MetalensHipError, match='reset = 1'):
        p.accumulate([w], reset=False)
    p.accumulate([w], reset=True)
    I1, Sz1 = p.sums()
    assert I1.shape == (30, 25)
    _check_sums(I1, Sz1, [[(w, fields)]], want_h)
    p.accumulate([w], reset=False)
    I2, Sz2 = p.sums()
    assert np.array_equal(I2, 2 * I1) and (not want_h or np.array_equal(Sz2, 2 * Sz1))


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_three_sets_in_one_call_equal_the_single_passes(ma, ctx, want_h):
    """the batch of a synthesis (window A of tests/test_gpu_propagate_sets.py: three dipoles, rows with extents and rows
    outside the lens) through tiles of 32 x 64: three sets in one propagate_sets call against the three single passes,
    bit for bit, and their sums"""
    from test_gpu_propagate_sets import DIPOLES, _batch, _same, _select
    x, y, n_glass, n = _batch(ma, ctx, 'A', DIPOLES)
    tx, ty, z = gref.target_axis(x, -7.3, 26), gref.target_axis(y, 40.6, 19), 20e-6
    p = ma.PlanePropagator(x, y, WL, n_glass, tx, ty, z, want_h=want_h, ctx=ctx, method='fft-tiled', tile=(32, 64))
    sets = p.propagate_sets()
    assert len(sets) == n == 3
    assert p.plan_info()['tiles'] == (14, 3) and p.plan_info()['tile_samples'] == (7, 46)
    singles = []
    for m in range(n):
        _select(ctx, m)
        singles.append(p.propagate())
        _same(sets[m], singles[m], want_h)
    assert not np.array_equal(singles[0]['Ex'], singles[1]['Ex'])
    tail = p.propagate_sets(first=1)
    assert len(tail) == 2
    _same(tail[0], singles[1], want_h)
    _same(tail[1], singles[2], want_h)
    weights = np.array([1.0, 0.5, 2.0])
    p.propagate_sets()
    p.accumulate(weights, reset=True)
    I, Sz = p.sums()
    assert I.shape == (26, 19)
    _check_sums(I, Sz, [list(zip(weights, sets))], want_h)
    _select(ctx, 0)


def test_refusals_leave_the_previous_plan_usable(ma, ctx, monkeypatch):
    from metalens_amd import _lib
    r = tref.reference('ta-near')
    x, y, tx, ty, z = r['x'], r['y'], r['tx'], r['ty'], r['z']
    _upload(ctx, _contiguous(r['F']))
    p = _propagator(ma, ctx, r)
    first = p.propagate()
    info = p.plan_info()
    assert info['method'] == 'fft-tiled' and info['tiles'] == (4, 2)
    make = lambda **kw: ma.PlanePropagator(x, y, WL, N_GLASS, kw.pop('tx', tx), ty, z, ctx=ctx, **kw)   # noqa: E731
    with pytest.raises(ValueError, match='x axis of n = 48 samples and m = 20 targets is L = 16'):     # a tile below m
        make(method='fft-tiled', tile=(16, 64))
    with pytest.raises(ValueError, match='y axis of n = 40 samples and m = 30 targets is L = 48'):     # no power of two
        make(method='fft-tiled', tile=(32, 48))
    with pytest.raises(ValueError, match='x axis of n = 48 samples has m = 8193 targets'):
        make(tx=gref.target_axis(x, 0.0, 8193), method='fft-tiled')
    with pytest.raises(ValueError, match="tile lengths belong to method='fft-tiled', not to method='fft'"):
        make(method='fft', tile=(32, 64))
    with pytest.raises(ValueError, match='method must be one of'):
        make(method='auto')
    # the C entry on its own, with a field set resident: n is that set's
    geometry = (ctx.handle, x[0], y[0], x[1] - x[0], y[1] - y[0], WL, N_GLASS, tx[0], ty[0])
    entry = ctx.lib.ml_propagate_plan_grid_tiled
    for args, said in (((20, 30, z, 1, 16, 64), b'x axis of n = 48 samples and m = 20 targets is L = 16'),
                       ((20, 30, z, 1, 32, 48), b'y axis of n = 40 samples and m = 30 targets is L = 48'),
                       ((20, 30, z, 1, 16384, 64), b'x axis of n = 48 samples and m = 20 targets is L = 16384'),
                       ((8193, 30, z, 1, 0, 0), b'x axis of n = 48 samples has m = 8193 targets'),
                       ((20, 8193, z, 0, 32, 8192), b'y axis of n = 40 samples has m = 8193 targets'),
                       ((20, 30, -z, 1, 32, 64), b'needs z > 0')):
        rc = entry(*geometry, *args)
        assert rc != 0 and b'ml_propagate_plan_grid_tiled: ' in ctx.lib.ml_last_error() + b'ml_propagate_plan_grid_tiled: ' \
            and said in ctx.lib.ml_last_error(), ctx.lib.ml_last_error()
    assert ctx.propagate_owner == p.owner
    monkeypatch.setattr(p, '_plan', lambda: pytest.fail('planned again'))
    again = p.propagate()
    assert p.plan_info() == info
    assert all(np.array_equal(first[k], again[k]) for k in first)
    # ml_propagate_plan_tiles serves a tiled plan only
    t = [_lib.c_int(0) for _ in range(5)]
    assert ctx.lib.ml_propagate_plan_tiles(ctx.handle, *[_lib.byref(v) for v in t]) == 0
    assert [v.value for v in t] == [4, 2, 13, 35, 8]
    monkeypatch.undo()
    q = ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=ctx, method='fft')
    assert ctx.lib.ml_propagate_plan_tiles(ctx.handle, *[_lib.byref(v) for v in t]) != 0
    assert b'no tiled propagation plan is active' in ctx.lib.ml_last_error()
    assert set(q.plan_info()) == {'method', 'Lx', 'Ly', 'workspace_bytes'}
    # a multi-rank context
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        with pytest.raises(_lib.MetalensHipError, match='ml_propagate_plan_grid_tiled: this context belongs to a communicator of 2 ranks'):
            ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=c, method='fft-tiled')
    finally:
        c.close()
