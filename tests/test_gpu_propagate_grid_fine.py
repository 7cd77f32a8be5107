"""``PlanePropagator(method='fft-fine')`` on the GPU (csrc/propagate_grid_fine.hip, ml_propagate_plan_grid_fine):
the FFT form of the finite-distance propagator for a patch of targets on the aperture's pitch divided by integers - the
interleave of lattices on the pitch, each a tiled convolution of the same current spectra.  Needs an MI355X.

Errors and bounds are those of tests/test_gpu_propagate_grid_tiled.py: max |difference| over components and targets / max
|field| of the long-double sum; ``e_ref`` is that error of the plain fp64 direct NumPy sum, ``e_np`` of the NumPy fine
form (tests/propagate_grid_fine_ref.py).  Parity: ``e_gpu <= 8 e_np`` on the targets of the long-double sum and
``<= 16 e_np`` against the NumPy form on every target; against ``method='direct'``: ``8 e_np + 8 e_ref``.  The yardsticks
are the NumPy restatement and the long-double sum, never the code under test.  A lattice that holds the planned count of
targets on both axes is the ``'fft-tiled'`` propagator planned on its own targets, bit for bit: that pins the pair
contraction, the single remainder and the scatter to code that has tests of its own.  The measured triples are printed
as ``PARITY ...`` lines (run with -s; they belong in profiles/propagate_parity.txt).

The cases are small: the largest plan ('fc-batches', 4 lattices of 490 tiles of 16 x 16) holds 65 MB."""
import numpy as np
import pytest

import propagate_grid_fine_ref as fref
import propagate_grid_ref as gref
import propagate_grid_tiled_ref as tref
import propagate_ref as ref
from test_gpu_fft_mixed import _upload
from test_gpu_propagate_sets import _check_sums, _lens

pytestmark = pytest.mark.gpu

WL, N_GLASS = gref.WL, gref.N_GLASS
E_KEYS, H_KEYS = ('Ex', 'Ey', 'Ez'), ('Hx', 'Hy', 'Hz')
TILED_KEYS = {'method', 'Lx', 'Ly', 'workspace_bytes', 'tiles', 'tile_samples', 'batch'}


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
    kw.setdefault('method', 'fft-fine')
    if kw['method'] == 'fft-fine':
        kw.setdefault('tile', r['tile'])
        kw.setdefault('subsample', r['subsample'])
    return ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], ctx=ctx, **kw)


def _planes(plan, want_h, cached):
    """the workspace of a mode in planes (tests/propagate_grid_fine_ref.py)"""
    tiles, A = plan['tiles'][0] * plan['tiles'][1], plan['active'][0] * plan['active'][1]
    return (8 * A * tiles if cached else 16 * plan['batch']) + 4 * tiles + 2 * (6 if want_h else 3)


def _info_of(plan, info, cached=True):
    return {'method': 'fft-fine', 'Lx': plan['L'][0], 'Ly': plan['L'][1], 'workspace_bytes': info['workspace_bytes'],
            'tiles': plan['tiles'], 'tile_samples': plan['tile_samples'], 'batch': plan['batch'],
            'subsample': plan['subsample'], 'lattice_targets': plan['lattice_targets'], 'cache_kernels': cached}


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', sorted(fref.CASES))
def test_against_the_long_double_sum(ma, ctx, case, want_h):
    r = fref.reference(case)
    _upload(ctx, _contiguous(r['F']))
    p = _propagator(ma, ctx, r, want_h=want_h)
    out = p.propagate()
    assert out['Ex'].shape == (r['tx'].size, r['ty'].size)
    sub, tag = r['sub'], 'EH' if want_h else 'E'
    eE = ref.max_error(_stack(out, E_KEYS)[:, sub], r['El'])
    print('PARITY fft-fine %-15s %-2s E: e_ref %.3e e_np %.3e gpu %.3e' % (case, tag, r['e_ref'][0], r['e_np'][0], eE))
    eE_all = ref.max_error(_stack(out, E_KEYS), r['Enp'])
    print('PARITY fft-fine %-15s %-2s E against the NumPy form on every target: %.3e (bound %.3e)'
          % (case, tag, eE_all, 16 * r['e_np'][0]))
    assert eE <= 8 * r['e_np'][0]
    assert eE_all <= 16 * r['e_np'][0]
    if want_h:
        eH = ref.max_error(_stack(out, H_KEYS)[:, sub], r['Hl'])
        print('PARITY fft-fine %-15s EH H: e_ref %.3e e_np %.3e gpu %.3e' % (case, r['e_ref'][1], r['e_np'][1], eH))
        eH_all = ref.max_error(_stack(out, H_KEYS), r['Hnp'])
        print('PARITY fft-fine %-15s EH H against the NumPy form on every target: %.3e (bound %.3e)' % (case, eH_all, 16 * r['e_np'][1]))
        assert eH <= 8 * r['e_np'][1]
        assert eH_all <= 16 * r['e_np'][1]
        assert set(out) == set(E_KEYS + H_KEYS + ('Sz',))
    else:
        assert set(out) == set(E_KEYS + ('I',))
    from metalens_amd.propagate import plan_info
    info, plan = plan_info(ctx), r['plan']
    stated = fref.PLANS[case]
    assert all(plan[k] == stated[k] for k in stated)
    assert info == _info_of(plan, info) and set(info) == TILED_KEYS | {'subsample', 'lattice_targets', 'cache_kernels'}
    assert info['workspace_bytes'] >= _planes(plan, want_h, True) * plan['L'][0] * plan['L'][1] * 16
    assert info == p.plan_info()


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', ['fa-ragged', 'fb-fewer-than-s'])
def test_streamed_kernels_give_the_bits_of_cached_ones(ma, case, want_h):
    """cache_kernels=False on a context of its own, so that the workspace it reports is what this mode reserved: the
    streamed formula exactly; then the cached plan on the same context: the same bits"""
    from metalens_amd import _lib
    r = fref.reference(case)
    plan, c = r['plan'], _lib.Context(0)
    try:
        _upload(c, _contiguous(r['F']))
        p = _propagator(ma, c, r, want_h=want_h, cache_kernels=False)
        streamed, again = p.propagate(), p.propagate()
        info = p.plan_info()
        assert info == _info_of(plan, info, cached=False)
        assert info['workspace_bytes'] == _planes(plan, want_h, False) * plan['L'][0] * plan['L'][1] * 16
        q = _propagator(ma, c, r, want_h=want_h)
        cached = q.propagate()
        info = q.plan_info()
        assert info['cache_kernels'] is True
        assert info['workspace_bytes'] >= _planes(plan, want_h, True) * plan['L'][0] * plan['L'][1] * 16
        assert set(streamed) == set(cached) == set(E_KEYS + (H_KEYS + ('Sz',) if want_h else ('I',)))
        for key in cached:
            assert np.abs(cached[key]).min() > 0, key
            assert np.array_equal(streamed[key], cached[key]) and np.array_equal(streamed[key], again[key]), key
    finally:
        c.close()


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', ['fa-ragged', 'fb-fewer-than-s', 'fd-eight'])
def test_full_lattices_are_the_tiled_method(ma, ctx, case, want_h):
    """every lattice with m_a = m_cx and m_b = m_cy against 'fft-tiled' planned on that lattice's own targets with the same
    tile: bit for bit, every key.  'fa-ragged': lattice (0, 0) of six; 'fb-fewer-than-s': all three - the first and the
    second of a pair and the single remainder; 'fd-eight': the eight lattices (a, 0) of 64 (17 targets along y at s = 8:
    lattice 0 alone holds three)"""
    r = fref.reference(case)
    (sx, sy), (m_cx, m_cy) = r['subsample'], r['plan']['lattice_targets']
    tile = r['tile'] or r['plan']['L']     # (the default of the fine plan is the default of the tiled plan on m_c)
    _upload(ctx, _contiguous(r['F']))
    fine = _propagator(ma, ctx, r, want_h=want_h).propagate()
    full = [(a, b) for a, m_a in fref.lattices(r['tx'].size, sx) for b, m_b in fref.lattices(r['ty'].size, sy)
            if (m_a, m_b) == (m_cx, m_cy)]
    assert len(full) == {'fa-ragged': 1, 'fb-fewer-than-s': 3, 'fd-eight': 8}[case]
    for a, b in full:
        p = ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'][a::sx], r['ty'][b::sy], r['z'], want_h=want_h, ctx=ctx,
                               method='fft-tiled', tile=tile)
        tiled = p.propagate()
        assert p.plan_info()['tiles'] == r['plan']['tiles'] and (p.plan_info()['Lx'], p.plan_info()['Ly']) == r['plan']['L']
        assert set(tiled) == set(fine) == set(E_KEYS + (H_KEYS + ('Sz',) if want_h else ('I',)))
        for key in tiled:
            assert tiled[key].shape == (m_cx, m_cy) and np.abs(tiled[key]).max() > 0
            assert np.array_equal(fine[key][a::sx, b::sy], tiled[key]), (a, b, key)


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_subsample_1_is_the_tiled_method(ma, ctx, want_h):
    r = tref.reference('ta-near')
    _upload(ctx, _contiguous(r['F']))
    got = {}
    for method, kw in (('fft-tiled', {}), ('fft-fine', dict(subsample=(1, 1)))):
        p = ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], want_h=want_h, ctx=ctx, method=method,
                               tile=r['tile'], **kw)
        got[method] = p.propagate(), p.plan_info()
    (a, ia), (b, ib) = got['fft-tiled'], got['fft-fine']
    assert set(a) == set(b) == set(E_KEYS + (H_KEYS + ('Sz',) if want_h else ('I',)))
    for key in a:
        assert np.abs(a[key]).max() > 0 and np.array_equal(a[key], b[key]), key
    assert set(ia) == TILED_KEYS                                        # the dicts of the other methods stay as they are
    assert all(ib[k] == ia[k] for k in TILED_KEYS - {'method', 'workspace_bytes'})
    assert ib['subsample'] == (1, 1) and ib['lattice_targets'] == (20, 30) and ib['method'] == 'fft-fine'


@pytest.mark.parametrize('case', ['fc-batches', 'fd-eight'])
def test_against_the_direct_method(ma, ctx, case):
    """every fine target"""
    r = fref.reference(case)
    _upload(ctx, _contiguous(r['F']))
    fine = _propagator(ma, ctx, r).propagate()
    direct = _propagator(ma, ctx, r, method='direct').propagate()
    for keys, e_np, e_ref in zip((E_KEYS, H_KEYS), r['e_np'], r['e_ref']):
        d = ref.max_error(_stack(fine, keys), _stack(direct, keys))
        print('PARITY fft-fine against direct, %s %s: %.3e (bound %.3e)' % (case, keys[0][0], d, 8 * e_np + 8 * e_ref))
        assert 0 < d <= 8 * e_np + 8 * e_ref


def test_repeatable_and_linear(ma, ctx):
    r = fref.reference('fa-ragged')
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


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_sets_and_sums(ma, ctx, want_h):
    """'fc-batches' (eight batches of tiles per set, two pairs of lattices): the sums of a pass as
    tests/test_gpu_propagate_sets.py asserts them for the direct method, and a pass added twice doubles them exactly"""
    from metalens_amd import _lib
    r = fref.reference('fc-batches')
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
    outside the lens) at half the pitch through tiles of 32 x 64: three sets in one propagate_sets call against the three
    single passes, bit for bit, and their sums"""
    from test_gpu_propagate_sets import DIPOLES, _batch, _same, _select
    x, y, n_glass, n = _batch(ma, ctx, 'A', DIPOLES)
    tx, ty, z = fref.fine_axis(x, -7.3, 27, 2), fref.fine_axis(y, 40.6, 19, 2), 20e-6
    p = ma.PlanePropagator(x, y, WL, n_glass, tx, ty, z, want_h=want_h, ctx=ctx, method='fft-fine', subsample=(2, 2),
                           tile=(32, 64))
    sets = p.propagate_sets()
    assert len(sets) == n == 3
    info = p.plan_info()
    assert info['lattice_targets'] == (14, 10) and info['tiles'] == (6, 3) and info['tile_samples'] == (19, 55)
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
    assert I.shape == (27, 19)
    _check_sums(I, Sz, [list(zip(weights, sets))], want_h)
    _select(ctx, 0)


def test_resident_equals_uploaded(ma, ctx):
    """the 512^2 lens of test_gpu_propagate_grid_tiled.test_resident_equals_uploaded at half the pitch: 32 x 40 fine targets,
    four lattices of 16 x 20, tiles of 256 - 16 + 1 = 241 and 237 samples - every tile boundary cuts the lens, and the tiles
    of the corners hold rows whose extents leave them empty"""
    lens = _lens()
    n = 512
    x = (np.arange(n) - (n - 1) / 2) * (WL / 2.2)
    assert x[-1] > lens['lens_periphery_summary']['r_max_list'][-1]
    args = dict(source_x=0.2e-6, source_y=-0.1e-6, source_z=-lens['source_distance'], source_pol='x', wavelength=WL,
                lens_periphery_summary=lens['lens_periphery_summary'], lens_center_summary=lens['lens_center_summary'],
                hexgridset=lens['hexgridset'], x_pts=x, y_pts=x, ctx=ctx)
    _, _, _, _, xs, ys, _, n_glass = ma.build_nearfield(**args, download=False)
    tx, ty = fref.fine_axis(xs, 240.3, 32, 2), fref.fine_axis(ys, 250.75, 40, 2)
    kw = dict(ctx=ctx, method='fft-fine', tile=(256, 256), subsample=(2, 2))
    resident = ma.field_at_plane(None, None, None, None, xs, ys, WL, n_glass, tx, ty, 20e-6, **kw)
    from metalens_amd.propagate import plan_info
    info = plan_info(ctx)
    assert info['tiles'] == (3, 3) and info['tile_samples'] == (241, 237) and info['lattice_targets'] == (16, 20)
    F = ma.build_nearfield(**args)[:4]
    assert max(np.abs(f[0]).max() for f in F) == 0 and np.abs(F[0]).max() > 0
    uploaded = ma.field_at_plane(*F, xs, ys, WL, n_glass, tx, ty, 20e-6, **kw)
    for key in E_KEYS + H_KEYS + ('Sz',):
        assert resident[key].shape == (32, 40) and np.abs(resident[key]).max() > 0
        assert np.array_equal(resident[key], uploaded[key]), key
    with pytest.raises(ValueError, match='resident near field is 512 x 512'):
        ma.field_at_plane(None, None, None, None, xs[:500], ys, WL, n_glass, tx, ty, 20e-6, **kw)


def test_refusals_leave_the_previous_plan_usable(ma, ctx, monkeypatch):
    from metalens_amd import _lib
    r = fref.reference('fa-ragged')
    x, y, tx, ty, z = r['x'], r['y'], r['tx'], r['ty'], r['z']
    _upload(ctx, _contiguous(r['F']))
    p = _propagator(ma, ctx, r)
    first = p.propagate()
    info = p.plan_info()
    assert info['method'] == 'fft-fine' and info['tiles'] == (3, 2)
    # the C entry on its own, with a field set resident: n is that set's
    geometry = (ctx.handle, x[0], y[0], x[1] - x[0], y[1] - y[0], WL, N_GLASS)
    entry = ctx.lib.ml_propagate_plan_grid_fine
    fx, fy = _lib.f64(tx[:2]), _lib.f64(ty[:3])
    down, wide = _lib.f64([tx[1], tx[0]]), _lib.f64([ty[0], ty[1], ty[0] + 1.5 * (y[1] - y[0])])
    same = _lib.f64([tx[0], tx[0]])
    for args, said in (((fx, 0, fy, 3, 21, 31, z, 1, 32, 32, 1), b'x axis of n = 48 samples and m = 21 fine targets has s = 0'),
                       ((fx, 2, fy, 9, 21, 31, z, 1, 32, 32, 1), b'y axis of n = 40 samples and m = 31 fine targets has s = 9'),
                       ((down, 2, fy, 3, 21, 31, z, 1, 32, 32, 1), b'the tx origins of the lattices must ascend strictly: tx_first[1]'),
                       ((same, 2, fy, 3, 21, 31, z, 1, 32, 32, 0), b'the tx origins of the lattices must ascend strictly: tx_first[1]'),
                       ((fx, 2, wide, 3, 21, 31, z, 1, 32, 32, 1), b"the ty origins of the lattices must span less than the aperture's pitch"),
                       ((fx, 2, fy, 3, 21, 31, -z, 1, 32, 32, 1), b'needs z > 0'),
                       ((fx, 2, fy, 3, 21, 31, z, 1, 8, 32, 1), b'x axis of n = 48 samples and m_c = 11 targets per lattice (m = 21 fine '
                                                                b'targets at s = 2) is L = 8'),
                       ((fx, 2, fy, 3, 21, 31, z, 0, 32, 48, 0), b'y axis of n = 40 samples and m_c = 11 targets per lattice (m = 31 fine '
                                                                 b'targets at s = 3) is L = 48')):
        rc = entry(*geometry, _lib.dptr(args[0]), args[1], _lib.dptr(args[2]), *args[3:])
        assert rc != 0 and ctx.lib.ml_last_error().startswith(b'ml_propagate_plan_grid_fine: ') \
            and said in ctx.lib.ml_last_error(), ctx.lib.ml_last_error()
    assert ctx.propagate_owner == p.owner
    monkeypatch.setattr(p, '_plan', lambda: pytest.fail('planned again'))
    again = p.propagate()
    assert p.plan_info() == info
    assert all(np.array_equal(first[k], again[k]) for k in first)
    # ml_propagate_plan_lattices serves a fine plan only, ml_propagate_plan_tiles a fine plan too
    t = [_lib.c_int(0) for _ in range(5)]
    assert ctx.lib.ml_propagate_plan_lattices(ctx.handle, *[_lib.byref(v) for v in t]) == 0
    assert [v.value for v in t] == [2, 3, 11, 11, 1]
    assert ctx.lib.ml_propagate_plan_tiles(ctx.handle, *[_lib.byref(v) for v in t]) == 0
    assert [v.value for v in t] == [3, 2, 22, 22, 6]
    monkeypatch.undo()
    q = ma.PlanePropagator(x, y, WL, N_GLASS, tx[::2], ty[::3], z, ctx=ctx, method='fft-tiled', tile=(32, 32))
    assert ctx.lib.ml_propagate_plan_lattices(ctx.handle, *[_lib.byref(v) for v in t]) != 0
    assert b'no fine propagation plan is active' in ctx.lib.ml_last_error()
    assert set(q.plan_info()) == TILED_KEYS
    # a multi-rank context
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        with pytest.raises(_lib.MetalensHipError, match='ml_propagate_plan_grid_fine: this context belongs to a communicator of 2 ranks'):
            ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=c, method='fft-fine', subsample=(2, 3))
    finally:
        c.close()
