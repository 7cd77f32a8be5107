"""``PlanePropagator(method='fft-stack')`` on the GPU (csrc/propagate_stack.hip, ml_propagate_plan_grid_stack): the fine FFT
form of the finite-distance propagator for a stack of planes - one plan, the currents transformed once, every (plane,
lattice) one more layer of kernel spectra.  Needs an MI355X.

Errors and bounds are those of tests/test_gpu_propagate_grid_fine.py: max |difference| over components and targets / max
|field| of the long-double sum; ``e_ref`` is that error of the plain fp64 direct NumPy sum, ``e_np`` of the NumPy stack
form (tests/propagate_grid_stack_ref.py).  Parity: ``e_gpu <= 8 e_np`` on the targets of the long-double sum and
``<= 16 e_np`` against the NumPy form on every target; against ``method='direct'`` as a point list over the volume:
``8 e_np + 8 e_ref``.  The yardsticks are the NumPy restatement and the long-double sum, never the code under test.  Plane
``p`` is the ``'fft-fine'`` propagator planned at ``z[p]``, bit for bit: that pins the layer table, the fill, the pairs that
straddle planes, the single remainder and the scatter to code that has tests of its own.  The measured triples are printed
as ``PARITY ...`` lines (run with -s; they belong in profiles/propagate_parity.txt).

The cases are small: the largest plan ('sd-batches', 8 layers of 490 tiles of 16 x 16) holds 136 MB."""
import numpy as np
import pytest

import propagate_grid_ref as gref
import propagate_grid_stack_ref as sref
import propagate_ref as ref
from test_gpu_fft_mixed import _upload
from test_gpu_propagate_sets import _check_sums, _lens

pytestmark = pytest.mark.gpu

WL, N_GLASS = gref.WL, gref.N_GLASS
E_KEYS, H_KEYS = ('Ex', 'Ey', 'Ez'), ('Hx', 'Hy', 'Hz')
STACK_KEYS = {'method', 'Lx', 'Ly', 'workspace_bytes', 'tiles', 'tile_samples', 'batch', 'subsample', 'lattice_targets',
              'cache_kernels', 'planes'}


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


def _keys(want_h):
    return set(E_KEYS + (H_KEYS + ('Sz',) if want_h else ('I',)))


def _propagator(ma, ctx, r, **kw):
    kw.setdefault('method', 'fft-stack')
    kw.setdefault('tile', r['tile'])
    kw.setdefault('subsample', r['subsample'])
    z = kw.pop('z', r['z'])
    return ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], z, ctx=ctx, **kw)


def _planes(plan, want_h, cached):
    """the workspace of a mode in planes of Lx Ly complex128 (tests/propagate_grid_stack_ref.py)"""
    tiles = plan['tiles'][0] * plan['tiles'][1]
    return (8 * plan['layers'] * tiles if cached else 16 * plan['batch']) + 4 * tiles + 2 * (6 if want_h else 3)


def _info_of(plan, info, cached=True):
    return {'method': 'fft-stack', 'Lx': plan['L'][0], 'Ly': plan['L'][1], 'workspace_bytes': info['workspace_bytes'],
            'tiles': plan['tiles'], 'tile_samples': plan['tile_samples'], 'batch': plan['batch'],
            'subsample': plan['subsample'], 'lattice_targets': plan['lattice_targets'], 'cache_kernels': cached,
            'planes': plan['planes']}


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', sorted(sref.CASES))
def test_against_the_long_double_sum(ma, ctx, case, want_h):
    r = sref.reference(case)
    _upload(ctx, _contiguous(r['F']))
    p = _propagator(ma, ctx, r, want_h=want_h)
    out = p.propagate()
    shape = (r['z'].size, r['tx'].size, r['ty'].size)
    assert p.shape == shape and set(out) == _keys(want_h) and all(out[k].shape == shape for k in out)
    sub, tag = r['sub'], 'EH' if want_h else 'E'
    eE = ref.max_error(_stack(out, E_KEYS)[:, sub], r['El'])
    print('PARITY fft-stack %-12s %-2s E: e_ref %.3e e_np %.3e gpu %.3e' % (case, tag, r['e_ref'][0], r['e_np'][0], eE))
    eE_all = ref.max_error(_stack(out, E_KEYS), r['Enp'])
    print('PARITY fft-stack %-12s %-2s E against the NumPy form on every target: %.3e (bound %.3e)'
          % (case, tag, eE_all, 16 * r['e_np'][0]))
    assert eE <= 8 * r['e_np'][0]
    assert eE_all <= 16 * r['e_np'][0]
    if want_h:
        eH = ref.max_error(_stack(out, H_KEYS)[:, sub], r['Hl'])
        print('PARITY fft-stack %-12s EH H: e_ref %.3e e_np %.3e gpu %.3e' % (case, r['e_ref'][1], r['e_np'][1], eH))
        eH_all = ref.max_error(_stack(out, H_KEYS), r['Hnp'])
        print('PARITY fft-stack %-12s EH H against the NumPy form on every target: %.3e (bound %.3e)' % (case, eH_all, 16 * r['e_np'][1]))
        assert eH <= 8 * r['e_np'][1]
        assert eH_all <= 16 * r['e_np'][1]
    from metalens_amd.propagate import plan_info
    info, plan = plan_info(ctx), r['plan']
    stated = sref.PLANS[case]
    assert all(plan[k] == stated[k] for k in stated)
    assert info == _info_of(plan, info) and set(info) == STACK_KEYS and info['planes'] == r['z'].size
    assert info['workspace_bytes'] >= _planes(plan, want_h, True) * plan['L'][0] * plan['L'][1] * 16
    assert info == p.plan_info()


@pytest.mark.parametrize('case', ['sa-ragged', 'sd-batches'])
def test_against_the_direct_method(ma, ctx, case):
    """every target of the volume as a point list"""
    r = sref.reference(case)
    _upload(ctx, _contiguous(r['F']))
    stack = _propagator(ma, ctx, r).propagate()
    zz, xx, yy = np.meshgrid(r['z'], r['tx'], r['ty'], indexing='ij')
    direct = ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, xx.ravel(), yy.ravel(), zz.ravel(), point_list=True, ctx=ctx).propagate()
    for keys, e_np, e_ref in zip((E_KEYS, H_KEYS), r['e_np'], r['e_ref']):
        d = ref.max_error(_stack(stack, keys), _stack(direct, keys))
        print('PARITY fft-stack against direct, %s %s: %.3e (bound %.3e)' % (case, keys[0][0], d, 8 * e_np + 8 * e_ref))
        assert 0 < d <= 8 * e_np + 8 * e_ref


@pytest.mark.parametrize('cached', [True, False], ids=['cached', 'streamed'])
@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', ['sa-ragged', 'sb-straddle', 'se-far'])
def test_every_plane_is_the_fine_method(ma, ctx, case, want_h, cached):
    """plane p against 'fft-fine' planned at z[p] with the same subsample and tile: bit for bit, every key.  'sa-ragged':
    ragged lattices, unsorted planes; 'sb-straddle': the pair (2, 3) holds the last lattice of plane 0 and the first of
    plane 1, layer 8 is contracted alone; 'se-far': 64 lattices a plane, 50 um and 1 mm"""
    r = sref.reference(case)
    _upload(ctx, _contiguous(r['F']))
    stack = _propagator(ma, ctx, r, want_h=want_h, cache_kernels=cached).propagate()
    assert set(stack) == _keys(want_h)
    for p, z in enumerate(r['z']):
        q = _propagator(ma, ctx, r, method='fft-fine', z=z, want_h=want_h, cache_kernels=cached)
        fine = q.propagate()
        info = q.plan_info()
        assert info['tiles'] == r['plan']['tiles'] and (info['Lx'], info['Ly']) == r['plan']['L'] and info['cache_kernels'] is cached
        assert set(fine) == set(stack)
        for key in fine:
            assert fine[key].shape == stack[key].shape[1:] and np.abs(fine[key]).min() > 0
            assert np.array_equal(stack[key][p], fine[key]), (p, key)


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_planes_alone_are_the_tiled_method(ma, ctx, want_h):
    """'sc-planes', subsample (1, 1): a layer is a plane, every pair straddles two planes; each plane equals 'fft-tiled' at
    that z, and the two planes at 20 um are equal"""
    r = sref.reference('sc-planes')
    _upload(ctx, _contiguous(r['F']))
    stack = _propagator(ma, ctx, r, want_h=want_h).propagate()
    assert r['z'][0] == r['z'][2] and np.unique(r['z']).size == 4
    for key in stack:
        assert np.array_equal(stack[key][0], stack[key][2]), key
        assert not np.array_equal(stack[key][0], stack[key][1]), key
    for p, z in enumerate(r['z']):
        tiled = ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], z, want_h=want_h, ctx=ctx, method='fft-tiled').propagate()
        assert set(tiled) == set(stack) == _keys(want_h)
        for key in tiled:
            assert np.abs(tiled[key]).max() > 0 and np.array_equal(stack[key][p], tiled[key]), (p, key)


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', ['sa-ragged', 'sb-straddle', 'sd-batches'])
def test_streamed_kernels_give_the_bits_of_cached_ones(ma, case, want_h):
    """cache_kernels=False on a context of its own, so that the workspace it reports is what this mode reserved: the
    streamed formula exactly - no nz in it; then the cached plan on the same context: the same bits.  'sd-batches': eight
    batches of tiles, the contraction continues from the stored sums (FIRST = false) on seven of them"""
    from metalens_amd import _lib
    r = sref.reference(case)
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
        assert set(streamed) == set(cached) == _keys(want_h)
        for key in cached:
            assert np.abs(cached[key]).min() > 0, key
            assert np.array_equal(streamed[key], cached[key]) and np.array_equal(streamed[key], again[key]), key
    finally:
        c.close()


@pytest.mark.parametrize('cached', [True, False], ids=['cached', 'streamed'])
def test_reversed_planes_repeatable_and_linear(ma, ctx, cached):
    """'sa-ragged': z reversed gives the planes reversed; two passes give the same bits; a field times two gives the output
    times two, exactly"""
    r = sref.reference('sa-ragged')
    F = _contiguous(r['F'])
    _upload(ctx, F)
    p = _propagator(ma, ctx, r, cache_kernels=cached)
    a, b = p.propagate(), p.propagate()
    back = _propagator(ma, ctx, r, z=r['z'][::-1], cache_kernels=cached).propagate()
    _upload(ctx, [2 * f for f in F])
    c = p.propagate()
    for key in E_KEYS + H_KEYS:
        assert np.abs(a[key]).min() > 0
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(back[key], a[key][::-1]), key
        assert np.array_equal(c[key], 2 * a[key]), key


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_sets_and_sums(ma, ctx, want_h):
    """'sd-batches': the sums of a pass as tests/test_gpu_propagate_sets.py asserts them for the direct method, on the shape
    (nz, mx, my), and a pass added twice doubles them exactly"""
    from metalens_amd import _lib
    r = sref.reference('sd-batches')
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
    assert I1.shape == (2, 30, 25)
    _check_sums(I1, Sz1, [[(w, fields)]], want_h)
    p.accumulate([w], reset=False)
    I2, Sz2 = p.sums()
    assert np.array_equal(I2, 2 * I1) and (not want_h or np.array_equal(Sz2, 2 * Sz1))


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_three_sets_in_one_call_equal_the_single_passes(ma, ctx, want_h):
    """the batch of a synthesis (window A of tests/test_gpu_propagate_sets.py: three dipoles, rows with extents and rows
    outside the lens) at half the pitch through tiles of 32 x 64, three planes: three sets in one propagate_sets call
    against the three single passes, bit for bit, and their sums"""
    from propagate_grid_fine_ref import fine_axis
    from test_gpu_propagate_sets import DIPOLES, _batch, _same, _select
    x, y, n_glass, n = _batch(ma, ctx, 'A', DIPOLES)
    tx, ty, z = fine_axis(x, -7.3, 27, 2), fine_axis(y, 40.6, 19, 2), (20e-6, 30e-6, 10e-6)
    p = ma.PlanePropagator(x, y, WL, n_glass, tx, ty, z, want_h=want_h, ctx=ctx, method='fft-stack', subsample=(2, 2),
                           tile=(32, 64))
    sets = p.propagate_sets()
    assert len(sets) == n == 3
    info = p.plan_info()
    assert info['lattice_targets'] == (14, 10) and info['tiles'] == (6, 3) and info['tile_samples'] == (19, 55) and info['planes'] == 3
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
    assert I.shape == (3, 27, 19)
    _check_sums(I, Sz, [list(zip(weights, sets))], want_h)
    _select(ctx, 0)


def test_through_the_sweep(ma, ctx):
    """a short ``SourceSweep.run(image=stack)``: ``I_sum`` and ``Sz_sum`` have the shape (nz, mx, my) and are the weighted
    host sums of ``image_each``"""
    from propagate_grid_fine_ref import fine_axis
    from test_gpu_propagate_sets import SWEEP_WEIGHTS, _common, _sweep_sources, _window
    lens = _lens()
    x, y = _window('A')
    u = np.linspace(-0.2, 0.2, 24)
    sw = ma.SourceSweep(*_common(lens), x, y, u, u, ctx=ctx)
    tx, ty, z = fine_axis(x, 40.3, 12, 2), fine_axis(y, 60.6, 9, 3), (20e-6, 30e-6, 10e-6)
    p = ma.PlanePropagator(x, y, WL, sw.n_glass, tx, ty, z, ctx=ctx, method='fft-stack', subsample=(2, 3))
    sources, weights = _sweep_sources(lens), SWEEP_WEIGHTS
    got = sw.run(sources, weights=weights, image=p, keep_each=True)
    each = got['image_each']
    assert len(each) == 5 and got['I_sum'].shape == got['Sz_sum'].shape == p.shape == (3, 12, 9)
    assert all(each[k]['Ex'].shape == (3, 12, 9) and np.abs(each[k]['Ex']).max() > 0 for k in range(5))
    passes = [[(weights[k], each[k]) for k in (0, 1, 2)], [(weights[k], each[k]) for k in (3, 4)]]
    _check_sums(got['I_sum'], got['Sz_sum'], passes, True)


def test_resident_equals_uploaded(ma, ctx):
    """the 512^2 lens of test_gpu_propagate_grid_fine.test_resident_equals_uploaded at half the pitch in two planes: tiles of
    241 and 237 samples - every tile boundary cuts the lens, and the tiles of the corners hold rows whose extents leave them
    empty"""
    from propagate_grid_fine_ref import fine_axis
    lens = _lens()
    n = 512
    x = (np.arange(n) - (n - 1) / 2) * (WL / 2.2)
    assert x[-1] > lens['lens_periphery_summary']['r_max_list'][-1]
    args = dict(source_x=0.2e-6, source_y=-0.1e-6, source_z=-lens['source_distance'], source_pol='x', wavelength=WL,
                lens_periphery_summary=lens['lens_periphery_summary'], lens_center_summary=lens['lens_center_summary'],
                hexgridset=lens['hexgridset'], x_pts=x, y_pts=x, ctx=ctx)
    _, _, _, _, xs, ys, _, n_glass = ma.build_nearfield(**args, download=False)
    tx, ty, z = fine_axis(xs, 240.3, 32, 2), fine_axis(ys, 250.75, 40, 2), (20e-6, 25e-6)
    kw = dict(ctx=ctx, method='fft-stack', tile=(256, 256), subsample=(2, 2))
    resident = ma.field_at_plane(None, None, None, None, xs, ys, WL, n_glass, tx, ty, z, **kw)
    from metalens_amd.propagate import plan_info
    info = plan_info(ctx)
    assert info['tiles'] == (3, 3) and info['tile_samples'] == (241, 237) and info['lattice_targets'] == (16, 20) and info['planes'] == 2
    F = ma.build_nearfield(**args)[:4]
    assert max(np.abs(f[0]).max() for f in F) == 0 and np.abs(F[0]).max() > 0
    uploaded = ma.field_at_plane(*F, xs, ys, WL, n_glass, tx, ty, z, **kw)
    for key in E_KEYS + H_KEYS + ('Sz',):
        assert resident[key].shape == (2, 32, 40) and np.abs(resident[key]).max() > 0
        assert np.array_equal(resident[key], uploaded[key]), key
    with pytest.raises(ValueError, match='resident near field is 512 x 512'):
        ma.field_at_plane(None, None, None, None, xs[:500], ys, WL, n_glass, tx, ty, z, **kw)


def test_refusals_leave_the_previous_plan_usable(ma, ctx, monkeypatch):
    """argument errors of the C entry with a field set resident: each names the entry and leaves the plan that was active
    reproducible"""
    from metalens_amd import _lib
    r = sref.reference('sa-ragged')
    x, y, tx, ty, z = r['x'], r['y'], r['tx'], r['ty'], r['z']
    _upload(ctx, _contiguous(r['F']))
    p = _propagator(ma, ctx, r)
    first = p.propagate()
    info = p.plan_info()
    assert info['method'] == 'fft-stack' and info['tiles'] == (3, 2) and info['planes'] == 3
    geometry = (ctx.handle, x[0], y[0], x[1] - x[0], y[1] - y[0], WL, N_GLASS)
    entry = ctx.lib.ml_propagate_plan_grid_stack
    fx, fy, zs = _lib.f64(tx[:2]), _lib.f64(ty[:3]), _lib.f64(z)
    down, wide = _lib.f64([tx[1], tx[0]]), _lib.f64([ty[0], ty[1], ty[0] + 1.5 * (y[1] - y[0])])
    many = _lib.f64(np.full(4097, 2e-6))
    for args, said in (((fx, 2, fy, 3, 21, 31, zs, 0, 1, 32, 32, 1), b'a stack has 1 to 4096 planes, got nz = 0'),
                       ((fx, 2, fy, 3, 21, 31, many, 4097, 1, 32, 32, 1), b'a stack has 1 to 4096 planes, got nz = 4097'),
                       ((fx, 2, fy, 3, 21, 31, _lib.f64([20e-6, 0.0, 5e-6]), 3, 1, 32, 32, 1), b'plane 1 of the stack lies at z[1] = 0:'),
                       ((fx, 2, fy, 3, 21, 31, _lib.f64([20e-6, 2e-6, -5e-6]), 3, 1, 32, 32, 0), b'plane 2 of the stack lies at z[2] = -5e-06:'),
                       ((fx, 2, fy, 3, 21, 31, _lib.f64([np.nan]), 1, 1, 32, 32, 1), b'plane 0 of the stack lies at z[0] = nan:'),
                       ((fx, 2, fy, 3, 21, 31, _lib.f64([2e-6, np.inf]), 2, 1, 32, 32, 1), b'plane 1 of the stack lies at z[1] = inf:'),
                       ((fx, 1, fy, 1, 4096, 4096, _lib.f64(np.full(5, 2e-6)), 5, 1, 0, 0, 0),
                        b'83886080 targets (5 planes of 4096 x 4096 fine targets): at most 2^26 per plan'),
                       ((fx, 2, fy, 3, 21, 31, _lib.f64([2e-6, 1e3]), 2, 1, 32, 32, 1), b'the phase arithmetic covers k R up to 1e+09'),
                       # the fine entry's own, with the same wording
                       ((fx, 0, fy, 3, 21, 31, zs, 3, 1, 32, 32, 1), b'x axis of n = 48 samples and m = 21 fine targets has s = 0'),
                       ((fx, 2, fy, 9, 21, 31, zs, 3, 1, 32, 32, 1), b'y axis of n = 40 samples and m = 31 fine targets has s = 9'),
                       ((down, 2, fy, 3, 21, 31, zs, 3, 1, 32, 32, 1), b'the tx origins of the lattices must ascend strictly: tx_first[1]'),
                       ((fx, 2, wide, 3, 21, 31, zs, 3, 1, 32, 32, 1), b"the ty origins of the lattices must span less than the aperture's pitch"),
                       ((fx, 2, fy, 3, 21, 31, zs, 3, 1, 8, 32, 1), b'x axis of n = 48 samples and m_c = 11 targets per lattice (m = 21 fine '
                                                                    b'targets at s = 2) is L = 8'),
                       ((fx, 2, fy, 3, 21, 31, zs, 3, 0, 32, 48, 0), b'y axis of n = 40 samples and m_c = 11 targets per lattice (m = 31 fine '
                                                                     b'targets at s = 3) is L = 48')):
        rc = entry(*geometry, _lib.dptr(args[0]), args[1], _lib.dptr(args[2]), args[3], args[4], args[5], _lib.dptr(args[6]), *args[7:])
        assert rc != 0 and ctx.lib.ml_last_error().startswith(b'ml_propagate_plan_grid_stack: ') \
            and said in ctx.lib.ml_last_error(), ctx.lib.ml_last_error()
    assert ctx.propagate_owner == p.owner
    monkeypatch.setattr(p, '_plan', lambda: pytest.fail('planned again'))
    again = p.propagate()
    assert p.plan_info() == info
    assert all(np.array_equal(first[k], again[k]) for k in first)
    # the plan entries that answer for a stack plan as for a fine plan; ml_propagate_plan_planes for a stack plan alone
    t, nz = [_lib.c_int(0) for _ in range(5)], _lib.c_int(0)
    assert ctx.lib.ml_propagate_plan_lattices(ctx.handle, *[_lib.byref(v) for v in t]) == 0
    assert [v.value for v in t] == [2, 3, 11, 11, 1]
    assert ctx.lib.ml_propagate_plan_tiles(ctx.handle, *[_lib.byref(v) for v in t]) == 0
    assert [v.value for v in t] == [3, 2, 22, 22, 6]
    assert ctx.lib.ml_propagate_plan_planes(ctx.handle, _lib.byref(nz)) == 0 and nz.value == 3
    method = _lib.c_int(0)
    assert ctx.lib.ml_propagate_plan_info(ctx.handle, _lib.byref(method), None, None, None) == 0 and method.value == 5
    monkeypatch.undo()
    q = _propagator(ma, ctx, r, method='fft-fine', z=z[0])
    assert ctx.lib.ml_propagate_plan_planes(ctx.handle, _lib.byref(nz)) != 0
    assert b'no stack propagation plan is active' in ctx.lib.ml_last_error()
    assert 'planes' not in q.plan_info()
    # the Python surface: several z stay an error of every other method, and the stack takes the sums' shape from its planes
    with pytest.raises(ValueError, match='a tensor grid of targets lies in one plane: z must be one number, got 3'):
        _propagator(ma, ctx, r, method='fft-fine')
    one = _propagator(ma, ctx, r, z=z[:1])
    assert one.shape == (1, 21, 31) and one.propagate()['Ex'].shape == (1, 21, 31)
    # a multi-rank context
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        with pytest.raises(_lib.MetalensHipError, match='ml_propagate_plan_grid_stack: this context belongs to a communicator of 2 ranks'):
            ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=c, method='fft-stack', subsample=(2, 3))
    finally:
        c.close()
