"""``PlanePropagator(method='fft-long')`` on the GPU (csrc/propagate_grid.hip, propagate_grid_fft.hip; ml_propagate_plan_grid_long): the FFT form of
the finite-distance propagator with padded axes of 16384.  Needs an MI355X.

Errors and bounds are those of tests/test_gpu_propagate_grid.py: max |difference| over components and targets / max
|field| of the long-double sum; ``e_ref`` is that error of the plain fp64 direct NumPy sum, ``e_np`` of the NumPy FFT form
(tests/propagate_grid_long_ref.py).  Parity: ``e_gpu <= 8 e_np`` on the 16 targets of the long-double sum and
``<= 16 e_np`` against the NumPy form on every target; against ``method='direct'``: ``8 e_np + 8 e_ref``.  The yardsticks
are the NumPy restatement and the long-double sum, never the code under test.  The measured triples are printed as
``PARITY ...`` lines (run with -s; they belong in profiles/propagate_parity.txt).

The cases are thin - one axis padded to 16384, the other to 32 or 256 - so that a plane is 67 MB at most.  A case with
BOTH axes at 16384 needs a workspace of 77 GB and is a measurement (tools/propagate_bench.py --method fft-long,
profiles/propagate_bench.txt), not a test."""
import numpy as np
import pytest

import propagate_grid_long_ref as lref
import propagate_grid_ref as gref
import propagate_ref as ref
from test_gpu_fft_mixed import _upload
from test_gpu_propagate_sets import _check_sums

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


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', sorted(lref.CASES))
def test_against_the_long_double_sum(ma, ctx, case, want_h):
    from metalens_amd.propagate import plan_info
    r = lref.reference(case)
    _upload(ctx, _contiguous(r['F']))
    p = ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], want_h=want_h, ctx=ctx, method='fft-long')
    out = p.propagate()
    assert out['Ex'].shape == (r['tx'].size, r['ty'].size)
    sub = r['sub']
    eE = ref.max_error(_stack(out, E_KEYS)[:, sub], r['El'])
    print('PARITY fft-long %-9s %-2s E: e_ref %.3e e_np %.3e gpu %.3e' % (case, 'EH' if want_h else 'E', r['e_ref'][0], r['e_np'][0], eE))
    eE_all = ref.max_error(_stack(out, E_KEYS), r['Enp'])
    print('PARITY fft-long %-9s %-2s E against the NumPy form on every target: %.3e (bound %.3e)'
          % (case, 'EH' if want_h else 'E', eE_all, 16 * r['e_np'][0]))
    assert eE <= 8 * r['e_np'][0]
    assert eE_all <= 16 * r['e_np'][0]
    if want_h:
        eH = ref.max_error(_stack(out, H_KEYS)[:, sub], r['Hl'])
        print('PARITY fft-long %-9s EH H: e_ref %.3e e_np %.3e gpu %.3e' % (case, r['e_ref'][1], r['e_np'][1], eH))
        eH_all = ref.max_error(_stack(out, H_KEYS), r['Hnp'])
        print('PARITY fft-long %-9s EH H against the NumPy form on every target: %.3e (bound %.3e)' % (case, eH_all, 16 * r['e_np'][1]))
        assert eH <= 8 * r['e_np'][1]
        assert eH_all <= 16 * r['e_np'][1]
        assert set(out) == set(E_KEYS + H_KEYS + ('Sz',))
    else:
        assert set(out) == set(E_KEYS + ('I',))
    Lx, Ly = lref.PADDED[case]
    info = plan_info(ctx)
    assert info == {'method': 'fft-long', 'Lx': Lx, 'Ly': Ly, 'workspace_bytes': info['workspace_bytes']}
    assert info['workspace_bytes'] >= (12 + (6 if want_h else 3)) * Lx * Ly * 16


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('case', ['a-near', 'd-exact-power', 'f-long'])
def test_is_the_fft_method_where_both_exist(ma, ctx, case, want_h):
    """the guard that nothing existing moved: an axis of L <= 8192 of a long plan goes through the launches of 'fft'"""
    x, y, tx, ty, z = gref.geometry(case)
    _upload(ctx, _contiguous(gref.random_fields(x.size, y.size, x.size + y.size)))
    got = {}
    for method in ('fft', 'fft-long'):
        p = ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, want_h=want_h, ctx=ctx, method=method)
        got[method] = p.propagate(), p.plan_info()
    (a, ia), (b, ib) = got['fft'], got['fft-long']
    assert set(a) == set(b) == set(E_KEYS + (H_KEYS + ('Sz',) if want_h else ('I',)))
    for key in a:
        assert np.abs(a[key]).max() > 0 and np.array_equal(a[key], b[key]), key
    assert ia['method'] == 'fft' and ib['method'] == 'fft-long'
    Lx, Ly = gref.padded_length(x.size, tx.size), gref.padded_length(y.size, ty.size)
    assert (ia['Lx'], ia['Ly']) == (ib['Lx'], ib['Ly']) == (Lx, Ly) and max(Lx, Ly) <= 8192
    assert ia['workspace_bytes'] == ib['workspace_bytes'] >= (12 + (6 if want_h else 3)) * Lx * Ly * 16


def test_against_the_direct_method(ma, ctx):
    """every target of 'i-5000': 4000 x 9 targets, 5000 x 24 samples"""
    r = lref.reference('i-5000')
    _upload(ctx, _contiguous(r['F']))
    args = (r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'])
    long_ = ma.PlanePropagator(*args, ctx=ctx, method='fft-long').propagate()
    direct = ma.PlanePropagator(*args, ctx=ctx, method='direct').propagate()
    for keys, e_np, e_ref in zip((E_KEYS, H_KEYS), r['e_np'], r['e_ref']):
        d = ref.max_error(_stack(long_, keys), _stack(direct, keys))
        print('PARITY fft-long against direct, i-5000 %s: %.3e (bound %.3e)' % (keys[0][0], d, 8 * e_np + 8 * e_ref))
        assert 0 < d <= 8 * e_np + 8 * e_ref


def test_repeatable_and_linear(ma, ctx):
    r = lref.reference('h-long-y')
    F = _contiguous(r['F'])
    p = ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], ctx=ctx, method='fft-long')
    _upload(ctx, F)
    a, b = p.propagate(), p.propagate()
    _upload(ctx, [2 * f for f in F])
    c = p.propagate()
    for key in E_KEYS + H_KEYS:
        assert np.abs(a[key]).min() > 0
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(c[key], 2 * a[key]), key


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_plan_info_and_sums(ma, ctx, want_h):
    from metalens_amd import _lib
    r = lref.reference('i-5000')
    _upload(ctx, _contiguous(r['F']))
    p = ma.PlanePropagator(r['x'], r['y'], WL, N_GLASS, r['tx'], r['ty'], r['z'], want_h=want_h, ctx=ctx, method='fft-long')
    with pytest.raises(_lib.MetalensHipError, match='has not run on the active propagation plan'):
        p.sums()
    assert p.queue_sets(0, 1) == 1
    info = p.plan_info()
    assert info == {'method': 'fft-long', 'Lx': 16384, 'Ly': 32, 'workspace_bytes': info['workspace_bytes']}
    assert info['workspace_bytes'] >= (12 + (6 if want_h else 3)) * 16384 * 32 * 16
    fields = p._download(0)
    w = 1.5
    with pytest.raises(_lib.MetalensHipError, match='reset = 1'):
        p.accumulate([w], reset=False)
    p.accumulate([w], reset=True)
    I1, Sz1 = p.sums()
    assert I1.shape == (4000, 9)
    _check_sums(I1, Sz1, [[(w, fields)]], want_h)
    # the same pass added a second time: every addend doubles, exactly
    p.accumulate([w], reset=False)
    I2, Sz2 = p.sums()
    assert np.array_equal(I2, 2 * I1) and (not want_h or np.array_equal(Sz2, 2 * Sz1))


def test_refusals_leave_the_previous_plan_usable(ma, ctx, monkeypatch):
    from metalens_amd import _lib
    r = gref.reference('a-near')
    x, y, tx, ty, z = r['x'], r['y'], r['tx'], r['ty'], r['z']
    _upload(ctx, _contiguous(r['F']))
    p = ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=ctx, method='fft-long')
    first = p.propagate()
    assert p.plan_info()['method'] == 'fft-long'
    d = x[1] - x[0]
    m_long = 16384 - 48 + 2
    with pytest.raises(ValueError, match='n = 48 samples and m = 16338 targets to L = 32768 > 16384'):
        ma.PlanePropagator(x, y, WL, N_GLASS, gref.target_axis(x, 0.0, m_long), ty, z, ctx=ctx, method='fft-long')
    with pytest.raises(ValueError, match='method must be one of'):
        ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=ctx, method='auto')
    # the C entry on its own, with a field set resident
    geometry = (ctx.handle, x[0], y[0], d, y[1] - y[0], WL, N_GLASS, tx[0], ty[0])
    rc = ctx.lib.ml_propagate_plan_grid_long(*geometry, m_long, 30, z, 1)
    assert rc != 0
    assert b'ml_propagate_plan_grid_long: the FFT form pads the x axis of n = 48 samples and m = 16338 targets to L = 32768 > 16384' \
        in ctx.lib.ml_last_error()
    rc = ctx.lib.ml_propagate_plan_grid_long(*geometry, 8193, 8192, z, 1)
    assert rc != 0 and b'67117056 targets: at most 2^26 per plan' in ctx.lib.ml_last_error()
    # the old entry on the same arguments: its own text
    rc = ctx.lib.ml_propagate_plan_grid(*geometry, m_long, 30, z, 1)
    assert rc != 0 and b'ml_propagate_plan_grid: the FFT form pads the x axis of n = 48 samples and m = 16338 targets to ' \
        b'L = 32768 > 8192 (one row of L complex128 must fit the LDS)' in ctx.lib.ml_last_error()
    assert ctx.propagate_owner == p.owner
    monkeypatch.setattr(p, '_plan', lambda: pytest.fail('planned again'))
    again = p.propagate()
    assert p.plan_info()['method'] == 'fft-long'
    assert all(np.array_equal(first[k], again[k]) for k in first)
