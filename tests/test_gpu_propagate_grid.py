"""``PlanePropagator(method='fft')`` on the GPU (csrc/propagate_grid.hip, ml_propagate_plan_grid): the finite-distance
pair sum for targets on the aperture's pitch as an FFT convolution.  Needs an MI355X.

Errors are normalised as in tests/test_gpu_propagate.py: max |difference| over components and targets / max |field| of
the long-double sum.  ``e_ref`` is that error of the plain fp64 direct NumPy sum, ``e_np`` of the NumPy FFT form
(tests/propagate_grid_ref.py).  Parity: ``e_gpu <= 8 e_np`` - two correct fp64 evaluations of one algorithm in
different order (the 8 x convention of test_gpu_propagate.py).  Against ``method='direct'``: ``8 e_np + 8 e_ref``, each
method's own bound, by the triangle inequality.  The measured triples are printed as ``PARITY ...`` lines (run with
-s; they belong in profiles/propagate_parity.txt)."""
import numpy as np
import pytest

import propagate_grid_ref as gref
import propagate_ref as ref
from test_gpu_fft_mixed import _upload
from test_gpu_propagate_sets import (DIPOLES, SWEEP_WEIGHTS, TWO_DIPOLES, _batch, _check_sums, _common, _lens, _same, _select,
                                     _sweep_sources, _window)

pytestmark = pytest.mark.gpu

WL, N_GLASS = gref.WL, gref.N_GLASS
E_KEYS, H_KEYS = ('Ex', 'Ey', 'Ez'), ('Hx', 'Hy', 'Hz')
PARITY_CASES = ('a-near', 'b-more-targets', 'c-far', 'd-exact-power', 'e-one-target', 'e-one-row', 'f-long', 'f-long-y')


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


def _on_pitch(axis, origin_pitches, m):
    return gref.target_axis(axis, origin_pitches, m)


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', PARITY_CASES)
def test_against_the_long_double_sum(ma, ctx, case, want_h):
    r = gref.reference(case)
    out = ma.field_at_plane(*r['F'], r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], want_h=want_h, ctx=ctx,
                            method='fft')
    assert out['Ex'].shape == (r['tx'].size, r['ty'].size)
    sub = r['sub']
    eE = ref.max_error(_stack(out, E_KEYS)[:, sub], r['El'])
    print('PARITY fft %-14s %-2s E: e_ref %.3e e_np %.3e gpu %.3e' % (case, 'EH' if want_h else 'E', r['e_ref'][0], r['e_np'][0], eE))
    assert eE <= 8 * r['e_np'][0]
    # every target against the NumPy FFT form: 8 e_np + e_np by the triangle inequality where the long-double sum was
    # taken on every target; 16 where e_np was measured on a subset only
    assert ref.max_error(_stack(out, E_KEYS), r['Enp']) <= 16 * r['e_np'][0]
    if want_h:
        eH = ref.max_error(_stack(out, H_KEYS)[:, sub], r['Hl'])
        print('PARITY fft %-14s EH H: e_ref %.3e e_np %.3e gpu %.3e' % (case, r['e_ref'][1], r['e_np'][1], eH))
        assert eH <= 8 * r['e_np'][1]
        assert ref.max_error(_stack(out, H_KEYS), r['Hnp']) <= 16 * r['e_np'][1]
        assert set(out) == set(E_KEYS + H_KEYS + ('Sz',))
    else:
        assert set(out) == set(E_KEYS + ('I',))
    from metalens_amd.propagate import plan_info
    info = plan_info(ctx)
    nx, ny, mx, my = r['x'].size, r['y'].size, r['tx'].size, r['ty'].size
    Lx, Ly = gref.padded_length(nx, mx), gref.padded_length(ny, my)
    assert info == {'method': 'fft', 'Lx': Lx, 'Ly': Ly, 'workspace_bytes': info['workspace_bytes']}
    assert info['workspace_bytes'] >= (12 + (6 if want_h else 3)) * Lx * Ly * 16


def test_against_the_direct_method(ma, ctx):
    r = gref.reference('a-near')
    args = (*r['F'], r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'])
    fft, direct = ma.field_at_plane(*args, ctx=ctx, method='fft'), ma.field_at_plane(*args, ctx=ctx, method='direct')
    default = ma.field_at_plane(*args, ctx=ctx)
    for keys, e_np, e_ref in zip((E_KEYS, H_KEYS), r['e_np'], r['e_ref']):
        assert all(np.array_equal(default[k], direct[k]) for k in keys)      # 'direct' is the default
        d = ref.max_error(_stack(fft, keys), _stack(direct, keys))
        print('PARITY fft against direct, a-near %s: %.3e (bound %.3e)' % (keys[0][0], d, 8 * e_np + 8 * e_ref))
        assert 0 < d <= 8 * e_np + 8 * e_ref


def test_resident_equals_uploaded(ma, ctx):
    """the 512^2 lens of test_gpu_propagate.test_resident_equals_uploaded: a synthesised field (row extents: samples
    outside them are written as zeros by the padding) against the same arrays uploaded, by equality"""
    lens = _lens()
    n = 512
    x = (np.arange(n) - (n - 1) / 2) * (WL / 2.2)
    assert x[-1] > lens['lens_periphery_summary']['r_max_list'][-1]
    args = dict(source_x=0.2e-6, source_y=-0.1e-6, source_z=-lens['source_distance'], source_pol='x', wavelength=WL,
                lens_periphery_summary=lens['lens_periphery_summary'], lens_center_summary=lens['lens_center_summary'],
                hexgridset=lens['hexgridset'], x_pts=x, y_pts=x, ctx=ctx)
    _, _, _, _, xs, ys, _, n_glass = ma.build_nearfield(**args, download=False)
    tx, ty = _on_pitch(xs, 200.3, 32), _on_pitch(ys, 230.75, 40)
    resident = ma.field_at_plane(None, None, None, None, xs, ys, WL, n_glass, tx, ty, 20e-6, ctx=ctx, method='fft')
    F = ma.build_nearfield(**args)[:4]
    assert max(np.abs(f[0]).max() for f in F) == 0 and np.abs(F[0]).max() > 0
    uploaded = ma.field_at_plane(*F, xs, ys, WL, n_glass, tx, ty, 20e-6, ctx=ctx, method='fft')
    for key in E_KEYS + H_KEYS + ('Sz',):
        assert resident[key].shape == (32, 40) and np.abs(resident[key]).max() > 0
        assert np.array_equal(resident[key], uploaded[key]), key
    with pytest.raises(ValueError, match='resident near field is 512 x 512'):
        ma.field_at_plane(None, None, None, None, xs[:500], ys, WL, n_glass, tx, ty, 20e-6, ctx=ctx, method='fft')


def _image_targets(x, y):
    """26 x 19 targets on the pitch of window A or B, off its lattice, reaching outside the window on one side"""
    return _on_pitch(x, -7.3, 26), _on_pitch(y, 40.6, 19), 20e-6


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('window,batch', [('A', DIPOLES), ('A', TWO_DIPOLES), ('B', DIPOLES)], ids=['A-xyz', 'A-xy', 'B-xyz'])
def test_sets_equal_singles_bit_for_bit(ma, ctx, window, batch, want_h):
    x, y, n_glass, n = _batch(ma, ctx, window, batch)
    p = ma.PlanePropagator(x, y, WL, n_glass, *_image_targets(x, y), want_h=want_h, ctx=ctx, method='fft')
    sets = p.propagate_sets()
    assert len(sets) == n
    singles = []
    for m in range(n):
        _select(ctx, m)
        singles.append(p.propagate())
        _same(sets[m], singles[m], want_h)
    assert not np.array_equal(singles[0]['Ex'], singles[1]['Ex'])
    _same(p.propagate_sets(first=n - 1, n=1)[0], singles[n - 1], want_h)
    if n == 3:
        tail = p.propagate_sets(first=1)
        assert len(tail) == 2
        _same(tail[0], singles[1], want_h)
        _same(tail[1], singles[2], want_h)
    from metalens_amd import _lib
    for first, count in ((0, n + 1), (n, 1), (-1, 1), (0, 0), (0, 4)):
        with pytest.raises(_lib.MetalensHipError):
            p.propagate_sets(first=first, n=count)
    _select(ctx, 0)


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_sums(ma, ctx, want_h):
    """as tests/test_gpu_propagate_sets.py asserts for the direct method"""
    from metalens_amd import _lib
    x, y, n_glass, n = _batch(ma, ctx, 'A', DIPOLES)
    p = ma.PlanePropagator(x, y, WL, n_glass, *_image_targets(x, y), want_h=want_h, ctx=ctx, method='fft')
    weights = np.array([1.0, 0.5, 2.0])
    with pytest.raises(_lib.MetalensHipError, match='has not run on the active propagation plan'):
        p.sums()
    sets = p.propagate_sets()
    with pytest.raises(_lib.MetalensHipError, match='reset = 1'):
        p.accumulate(weights, reset=False)
    p.accumulate(weights, reset=True)
    I1, Sz1 = p.sums()
    assert I1.shape == (26, 19)
    _check_sums(I1, Sz1, [list(zip(weights, sets))], want_h)
    # the same pass added a second time: every addend doubles, exactly
    p.accumulate(weights, reset=False)
    I2, Sz2 = p.sums()
    assert np.array_equal(I2, 2 * I1)
    if want_h:
        assert np.array_equal(Sz2, 2 * Sz1)
    # reset: the first pass does not depend on what the buffer held
    p.accumulate(7 * weights, reset=False)
    p.accumulate(weights, reset=True)
    I3, Sz3 = p.sums()
    assert np.array_equal(I3, I1) and (not want_h or np.array_equal(Sz3, Sz1))
    # fewer members than the pass holds; a second pass on top of the first
    p.accumulate(weights[:2], reset=True)
    tail = p.propagate_sets(first=2, n=1)
    p.accumulate(weights[2:], reset=False)
    I4, Sz4 = p.sums()
    _check_sums(I4, Sz4, [list(zip(weights[:2], sets[:2])), [(weights[2], tail[0])]], want_h)
    with pytest.raises(_lib.MetalensHipError):   # the last pass holds one set
        p.accumulate(weights, reset=False)


def test_through_the_sweep(ma, ctx):
    """``SourceSweep.run(image=...)`` with an 'fft' and with a 'direct' propagator on the same targets.  Per source the
    fields differ by at most d = 8 e_np + 8 e_ref of max |E| (the bound of test_against_the_direct_method, with e_np and
    e_ref of that source's own near field on every 7th target); for the intensities that means, per target,
    |I_fft - I_direct| <= sum_k w_k 3 (2 d_k + d_k^2) A_k^2 with A_k = max |E_k|: | |a|^2 - |b|^2 | <= |a - b| (|a| + |b|)
    per component."""
    lens = _lens()
    x, y = _window('A')
    u = np.linspace(-0.2, 0.2, 24)
    sw = ma.SourceSweep(*_common(lens), x, y, u, u, ctx=ctx)
    tx, ty, z = _image_targets(x, y)
    sources, weights = _sweep_sources(lens), SWEEP_WEIGHTS
    p_fft = ma.PlanePropagator(x, y, WL, sw.n_glass, tx, ty, z, ctx=ctx, method='fft')
    got = sw.run(sources, weights=weights, image=p_fft, keep_each=True)
    p_dir = ma.PlanePropagator(x, y, WL, sw.n_glass, tx, ty, z, ctx=ctx)
    want = sw.run(sources, weights=weights, image=p_dir, keep_each=True)
    for key in ('P_sum', 'total_P', 'power_in'):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert got['I_sum'].shape == got['Sz_sum'].shape == (26, 19)
    TX, TY = np.meshgrid(tx, ty, indexing='ij')
    pts = np.stack([TX.ravel(), TY.ravel(), np.full(TX.size, z)], axis=1)[::7]
    bound = np.zeros(())
    for k, (sx, sy, sz, pol) in enumerate(sources):
        F = ma.build_nearfield(sx, sy, sz, pol, *_common(lens), x_pts=x, y_pts=y, ctx=ctx)[:4]
        El = ref.direct_sum(*F, x, y, WL, sw.n_glass, pts, Z0=p_fft.Z0, real=np.longdouble, want_h=False)
        e_ref = ref.max_error(ref.direct_sum(*F, x, y, WL, sw.n_glass, pts, Z0=p_fft.Z0, want_h=False), El)
        Enp = gref.grid_sum(*F, x, y, WL, sw.n_glass, tx[0], ty[0], tx.size, ty.size, z, Z0=p_fft.Z0, want_h=False)
        e_np = ref.max_error(Enp[:, ::7], El)
        d = 8 * e_np + 8 * e_ref
        a, b = _stack(got['image_each'][k], E_KEYS), _stack(want['image_each'][k], E_KEYS)
        print('PARITY sweep source %d: fft against direct %.3e (bound %.3e)' % (k, ref.max_error(a, b), d))
        assert ref.max_error(a, b) <= d
        bound = bound + weights[k] * 3 * (2 * d + d * d) * np.abs(b).max() ** 2
    err = np.abs(got['I_sum'] - want['I_sum']).max()
    print('PARITY sweep I_sum: fft against direct %.3e of the peak (bound %.3e)' % (err / want['I_sum'].max(), bound / want['I_sum'].max()))
    assert err <= bound
    _check_sums(got['I_sum'], got['Sz_sum'], [[(weights[k], got['image_each'][k]) for k in (0, 1, 2)],
                                              [(weights[k], got['image_each'][k]) for k in (3, 4)]], True)


def _farfield_sums(ctx, shape):
    from metalens_amd import _lib
    P, total, cone = np.empty(shape), np.zeros(1), np.zeros(1)
    _lib.check(ctx.lib.ml_farfield_sums(ctx.handle, _lib.dptr(P), _lib.dptr(total), _lib.dptr(cone), 1))
    return P, total, cone


def test_guest_on_a_shared_context(ma, ctx, monkeypatch):
    """an 'fft' and a 'direct' propagator alternating on one context: each reproduces its own bits, the far-field
    side is left as found, ml_propagate_plan_info tells which plan is active"""
    from metalens_amd import _lib
    r = gref.reference('b-more-targets')
    nx, ny = r['x'].size, r['y'].size
    ux, uy = np.linspace(-0.3, 0.3, 20), np.linspace(-0.2, 0.22, 24)
    ctx.set_method('gemm')
    t = ma.FarfieldTransform(nx, ny, r['x'][1] - r['x'][0], r['y'][1] - r['y'][0], WL, N_GLASS, ux, uy, ctx=ctx)
    F = [_lib.c128(f) for f in r['F']]
    _upload(ctx, F)
    t.transform()
    vectors, proj = t.radiation_vectors(), t.project()
    _lib.check(ctx.lib.ml_farfield_accumulate(ctx.handle, 1.0, 0.1, 0.0, 0.0, 0, 1))
    sums = _farfield_sums(ctx, proj[0].shape)
    planned = []
    monkeypatch.setattr(t, '_plan', lambda: planned.append('planned again'))
    p1 = ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], ctx=ctx, method='fft')
    p2 = ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'][:40] + 1e-7, r['ty'][:9], 30e-6, want_h=False, ctx=ctx)
    assert p2.method == 'direct' and p2.plan_info()['method'] == 'direct'
    a1 = p1.propagate()
    i1 = p1.plan_info()
    a2 = p2.propagate()
    i2 = p2.plan_info()
    b1, b2 = p1.propagate(), p2.propagate()
    assert i1['method'] == 'fft' and (i1['Lx'], i1['Ly']) == (128, 128) and i1['workspace_bytes'] >= 18 * 128 * 128 * 16
    assert i2 == {'method': 'direct', 'Lx': 0, 'Ly': 0, 'workspace_bytes': i2['workspace_bytes']} and i2['workspace_bytes'] > 0
    assert a1['Ex'].shape == (70, 33) and a2['Ex'].shape == (40, 9) and 'Hx' not in a2
    for a, b in ((a1, b1), (a2, b2)):
        for key in a:
            assert np.abs(a[key]).max() > 0 and np.array_equal(a[key], b[key]), key
    alone = ma.field_at_plane(*F, r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], ctx=ctx, method='fft')
    assert all(np.array_equal(alone[key], a1[key]) for key in alone)
    # sums do not outlive their plan; the other propagator is told so
    p1.queue_sets()
    p1.accumulate([1.5], reset=True)
    assert p1.sums()[0].shape == (70, 33)
    p2.propagate()
    with pytest.raises(RuntimeError, match='another propagator has planned'):
        p1.accumulate([1.0], reset=True)
    with pytest.raises(_lib.MetalensHipError, match='has not run on the active propagation plan'):
        p1.sums()
    # the far-field side of the context is as it was
    assert ctx.method == 'gemm' and ctx.precision == 'f64' and ctx.plan_owner == t.owner
    for got, want in zip(_farfield_sums(ctx, proj[0].shape), sums):
        assert np.array_equal(got, want)
    after = t.radiation_vectors()
    assert all(np.array_equal(after[k], vectors[k]) for k in vectors)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(t.project(), proj))
    assert planned == []
    ctx.set_method('auto')


def test_repeatable_and_linear(ma, ctx):
    r = gref.reference('d-exact-power')
    F = [np.ascontiguousarray(f) for f in r['F']]
    p = ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], ctx=ctx, method='fft')
    _upload(ctx, F)
    a, b = p.propagate(), p.propagate()
    _upload(ctx, [2 * f for f in F])
    c = p.propagate()
    for key in E_KEYS + H_KEYS:
        assert np.abs(a[key]).min() > 0
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(c[key], 2 * a[key]), key


def test_refusals_leave_the_previous_plan_usable(ma, ctx, monkeypatch):
    from metalens_amd import _lib
    r = gref.reference('a-near')
    x, y, tx, ty, z = r['x'], r['y'], r['tx'], r['ty'], r['z']
    F = [np.ascontiguousarray(f) for f in r['F']]
    _upload(ctx, F)
    p = ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=ctx, method='fft')
    first = p.propagate()
    d = x[1] - x[0]
    off = tx.copy()
    off[11] += 1e-6 * d
    with pytest.raises(ValueError, match=r"aperture's pitch: x\[11\]"):
        ma.PlanePropagator(x, y, WL, N_GLASS, off, ty, z, ctx=ctx, method='fft')
    coarse = ty[0] + np.arange(30) * (y[1] - y[0]) * 1.25
    with pytest.raises(ValueError, match=r"aperture's pitch: y\[1\]") as info:
        ma.PlanePropagator(x, y, WL, N_GLASS, tx, coarse, z, ctx=ctx, method='fft')
    assert '%.17g' % (y[1] - y[0]) in str(info.value) and '%.17g' % (coarse[1] - coarse[0]) in str(info.value)
    with pytest.raises(ValueError, match='not a point list'):
        ma.PlanePropagator(x, y, WL, N_GLASS, tx, tx, np.full(tx.size, z), point_list=True, ctx=ctx, method='fft')
    with pytest.raises(ValueError, match='method must be one of'):
        ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=ctx, method='auto')
    long_x = gref.target_axis(x, 0.0, 8192 - 48 + 2)
    with pytest.raises(ValueError, match='n = 48 samples and m = 8146 targets to L = 16384 > 8192'):
        ma.PlanePropagator(x, y, WL, N_GLASS, long_x, ty, z, ctx=ctx, method='fft')
    # ... and the C entry on its own, with a field set resident
    rc = ctx.lib.ml_propagate_plan_grid(ctx.handle, x[0], y[0], d, y[1] - y[0], WL, N_GLASS, tx[0], ty[0], 8146, 30, z, 1)
    assert rc != 0 and b'n = 48 samples and m = 8146 targets to L = 16384' in ctx.lib.ml_last_error()
    assert ctx.propagate_owner == p.owner
    monkeypatch.setattr(p, '_plan', lambda: pytest.fail('planned again'))
    again = p.propagate()
    assert all(np.array_equal(first[k], again[k]) for k in first)
    # a multi-rank context
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        q = ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=c, method='fft')   # planned while single-rank
        _upload(c, F)
        assert np.array_equal(q.propagate()['Ex'], first['Ex'])
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        with pytest.raises(_lib.MetalensHipError, match='ml_propagate_sets: this context belongs to a communicator of 2 ranks'):
            q.propagate_sets()
        with pytest.raises(_lib.MetalensHipError, match='ml_propagate_plan_grid: this context belongs to a communicator of 2 ranks'):
            ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=c, method='fft')
    finally:
        c.close()
