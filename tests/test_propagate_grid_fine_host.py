"""``method='fft-fine'`` of the finite-distance propagator without a GPU: the fine plan of csrc/propagate_grid.h
(GridFinePlan) through tools/propagate_grid_fine.cpp against the plan of tests/propagate_grid_fine_ref.py, the refusals of
``grid_fine_plan`` and of ``PlanePropagator`` that need no context, and the NumPy restatement of the fine sum - the
interleave of ``tiled_sum`` over the lattices - against the long-double direct sum of tests/propagate_ref.py.

Bound of the restatement: ``e_np <= 32 e_ref``, the condition of tests/test_propagate_grid_host.py - a cap that keeps the
yardstick of the GPU tests honest, not a measurement.  Measured ratios e_np / e_ref (E, H): 1.26, 1.32 for 'fa-ragged' (2 um behind
the aperture), 1.00 ... 1.04 for the others.

The long-double sum of 'fe-default' - 665 targets behind 60 000 samples, a minute - is a record under tests/golden/
(propagate_grid_fine_ref.long_double_sum), compared here with the sum taken afresh on 18 of its targets."""
import os
import subprocess

import numpy as np
import pytest

import propagate_grid_fine_ref as fref
import propagate_grid_ref as gref
import propagate_grid_tiled_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('grid_fine')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'propagate_grid_fine_san'])

    def run(*args):
        res = subprocess.run([out + 'propagate_grid_fine_san'] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout
    return run


def _facts(line):
    return {k: int(v) for k, v in (kv.split('=') for kv in line.split())}


def _want(nx, ny, mx, my, subsample, want_h, cached, tile=None):
    p = fref.plan(nx, ny, mx, my, subsample, want_h, tile, cached)
    return dict(sx=subsample[0], sy=subsample[1], ax=p['active'][0], ay=p['active'][1], mcx=p['lattice_targets'][0],
                mcy=p['lattice_targets'][1], cached=int(cached), Lx=p['L'][0], Ly=p['L'][1], cx=p['tiles'][0], cy=p['tiles'][1],
                bx=p['tile_samples'][0], by=p['tile_samples'][1], tiles=p['tiles'][0] * p['tiles'][1], batch=p['batch'],
                outputs=6 if want_h else 3, plane_bytes=p['plane_bytes'], workspace_bytes=p['workspace_bytes'])


@pytest.mark.parametrize('cached', [1, 0], ids=['cached', 'streamed'])
@pytest.mark.parametrize('want_h', [1, 0], ids=['EH', 'E'])
@pytest.mark.parametrize('case', sorted(fref.CASES))
def test_plan_of_the_cases(tool, case, want_h, cached):
    nx, ny, mx, my = fref.CASES[case][:4]
    tile, subsample = fref.CASES[case][7:]
    want = _want(nx, ny, mx, my, subsample, want_h, cached, tile)
    stated = fref.PLANS[case]
    assert (want['Lx'], want['Ly']) == stated['L'] and (want['cx'], want['cy']) == stated['tiles']
    assert (want['bx'], want['by']) == stated['tile_samples'] and want['batch'] == stated['batch']
    assert (want['ax'], want['ay']) == stated['active'] and (want['mcx'], want['mcy']) == stated['lattice_targets']
    assert _facts(tool(nx, ny, mx, my, *subsample, want_h, cached, *(tile or ()))) == want
    # the workspace formulas, stated outright
    planes = (8 * want['ax'] * want['ay'] * want['tiles'] if cached else 16 * want['batch']) + 4 * want['tiles'] + 2 * want['outputs']
    assert want['workspace_bytes'] == planes * want['Lx'] * want['Ly'] * 16
    # every fine target lies in exactly one lattice, and lattice 0 has the planned count
    for m, s, m_c in ((mx, subsample[0], want['mcx']), (my, subsample[1], want['mcy'])):
        lat = fref.lattices(m, s)
        assert sum(m_a for _, m_a in lat) == m and lat[0][1] == m_c and all(1 <= m_a <= m_c for _, m_a in lat)
        assert tool('lattice', m, s) == ''.join('a=%d m_a=%d\n' % am for am in lat)
        assert sorted(np.concatenate([np.arange(m)[a::s] for a, _ in lat]).tolist()) == list(range(m))


def test_plan_of_the_large_sizes(tool):
    """the workspaces the documentation quotes: 128 B x padded area per lattice, kept"""
    for sizes, subsample in (((4096, 4096, 64, 64), (2, 2)), ((4096, 4096, 64, 64), (4, 4)), ((8192, 8192, 64, 64), (2, 2))):
        for cached in (1, 0):
            assert _facts(tool(*sizes, *subsample, 1, cached)) == _want(*sizes, subsample, 1, cached)
    f = _facts(tool(8192, 8192, 64, 64, 2, 2, 1, 1))
    assert (f['mcx'], f['Lx'], f['cx'], f['tiles'], f['batch']) == (32, 512, 18, 324, 8)
    assert f['workspace_bytes'] == (8 * 4 * 324 + 4 * 324 + 12) * 512 * 512 * 16 > 2 ** 32
    assert _facts(tool(8192, 8192, 64, 64, 2, 2, 1, 0))['workspace_bytes'] == (16 * 8 + 4 * 324 + 12) * 512 * 512 * 16
    # s = 1: one lattice on the tiled plan of the same sizes
    f, t = _facts(tool(4096, 4096, 64, 64, 1, 1, 1, 1)), tref.plan(4096, 4096, 64, 64, True)
    assert (f['ax'], f['ay'], f['mcx'], f['mcy']) == (1, 1, 64, 64) and (f['Lx'], f['cx'], f['batch']) == (t['L'][0], t['tiles'][0], t['batch'])


def test_refusals(tool):
    for args, said in (((48, 40, 21, 31, 0, 3, 1, 1), 'x axis of n = 48 samples and m = 21 fine targets has s = 0'),
                       ((48, 40, 21, 31, 2, 9, 1, 1), 'y axis of n = 40 samples and m = 31 fine targets has s = 9'),
                       ((48, 40, 21, 31, -1, 3, 1, 0), 'x axis of n = 48 samples and m = 21 fine targets has s = -1'),
                       ((48, 40, 16386, 31, 2, 3, 1, 1), 'x axis of n = 48 samples has m = 16386 fine targets at s = 2, m_c = 8193'),
                       ((48, 40, 21, 65537, 2, 8, 0, 0), 'y axis of n = 40 samples has m = 65537 fine targets at s = 8, m_c = 8193'),
                       ((48, 40, 21, 31, 2, 3, 1, 1, 8, 32), 'x axis of n = 48 samples and m_c = 11 targets per lattice (m = 21 fine '
                                                             'targets at s = 2) is L = 8'),
                       ((48, 40, 21, 31, 2, 3, 1, 1, 32, 48), 'y axis of n = 40 samples and m_c = 11 targets per lattice (m = 31 fine '
                                                              'targets at s = 3) is L = 48'),
                       ((48, 40, 33, 31, 1, 3, 1, 1, 32, 32), 'x axis of n = 48 samples and m_c = 33 targets per lattice (m = 33 fine '
                                                              'targets at s = 1) is L = 32'),
                       ((48, 40, 16384, 8192, 2, 1, 1, 1), '134217728 fine targets (16384 x 8192): at most 2^26 per plan')):
        out = tool(*args)
        assert out.startswith('refused=1\n') and said in out, out
    # the limits themselves are taken: s = 8, m_c = 8192, a tile of exactly m_c, 2^26 fine targets
    f = _facts(tool(48, 40, 65536, 1, 8, 1, 1, 0))
    assert (f['mcx'], f['Lx'], f['ax']) == (8192, 8192, 8)
    assert _facts(tool(48, 40, 32, 31, 2, 3, 1, 1, 16, 16))['bx'] == 1
    assert _facts(tool(48, 40, 8192, 8192, 1, 1, 1, 0))['mcx'] == 8192


def test_python_refusals_need_no_context(monkeypatch):
    from metalens_amd import _lib
    from metalens_amd import propagate
    monkeypatch.setattr(_lib, 'default_context', lambda: pytest.fail('a context was asked for'))
    assert propagate.METHODS.index('fft-fine') == 4 and propagate.METHODS[:4] == ('direct', 'fft', 'fft-long', 'fft-tiled')
    x, y = gref.axis(48), gref.axis(40)
    tx, ty = fref.fine_axis(x, 0.3, 21, 2), fref.fine_axis(y, -0.4, 31, 3)
    args = (x, y, gref.WL, gref.N_GLASS)

    def make(tx=tx, ty=ty, z=2e-6, **kw):
        return propagate.PlanePropagator(*args, tx, ty, z, **kw)
    for bad, s in (((0, 3), '0'), ((2, 9), '9'), ((2.5, 3), '2.5'), ((2, -1), '-1')):
        with pytest.raises(ValueError, match=r'integer in \[1, 8\]: subsample = .* has s = %s along' % s):
            make(method='fft-fine', subsample=bad)
    with pytest.raises(ValueError, match='subsample must be None or the two pitch ratios'):
        make(method='fft-fine', subsample=2)
    for method in ('direct', 'fft', 'fft-long', 'fft-tiled'):
        with pytest.raises(ValueError, match="pitch ratios belong to method='fft-fine', not to method='%s'" % method):
            make(method=method, subsample=(2, 3))
        with pytest.raises(ValueError, match="cache_kernels=False: the choice belongs to method='fft-fine', not to method='%s'" % method):
            make(tx=gref.target_axis(x, 0.3, 20), ty=gref.target_axis(y, -0.4, 30), method=method, cache_kernels=False)
    # the message for `tile` with the other methods, word for word
    with pytest.raises(ValueError, match="tile lengths belong to method='fft-tiled', not to method='fft'"):
        make(method='fft', tile=(32, 32))
    # an axis on the coarse pitch given with s = 2; a fine axis given to 'fft-tiled'
    with pytest.raises(ValueError, match=r"aperture's pitch / 2: x\[1\]"):
        make(tx=gref.target_axis(x, 0.3, 21), method='fft-fine', subsample=(2, 3))
    with pytest.raises(ValueError, match=r"aperture's pitch: x\[1\]"):
        make(method='fft-tiled')
    off = ty.copy()
    off[17] += 1e-6 * (y[1] - y[0])
    with pytest.raises(ValueError, match=r"aperture's pitch / 3: y\[17\]"):
        make(ty=off, method='fft-fine', subsample=(2, 3))
    with pytest.raises(ValueError, match='not a point list'):
        make(ty=tx, z=np.full(tx.size, 2e-6), point_list=True, method='fft-fine', subsample=(2, 2))
    # a tile below m_c = (11, 11), no power of two; m_c > 8192
    with pytest.raises(ValueError, match=r'x axis of n = 48 samples and m_c = 11 targets per lattice \(m = 21 fine targets at s = 2\) is L = 8'):
        make(method='fft-fine', subsample=(2, 3), tile=(8, 32))
    with pytest.raises(ValueError, match='y axis of n = 40 samples and m_c = 11 targets per lattice .* is L = 48'):
        make(method='fft-fine', subsample=(2, 3), tile=(32, 48))
    with pytest.raises(ValueError, match='tile must be None or the two tile lengths'):
        make(method='fft-fine', subsample=(2, 3), tile=(32,))
    with pytest.raises(ValueError, match='x axis of n = 48 samples has m = 16386 fine targets at s = 2, m_c = 8193 per lattice'):
        make(tx=fref.fine_axis(x, 0.0, 16386, 2), method='fft-fine', subsample=(2, 3))
    # with the checks passed the constructor goes on to the context
    for kw in (dict(), dict(tile=(32, 32)), dict(tile=(16, 0)), dict(cache_kernels=False)):
        with pytest.raises(pytest.fail.Exception, match='a context was asked for'):
            make(method='fft-fine', subsample=(2, 3), **kw)
    with pytest.raises(pytest.fail.Exception, match='a context was asked for'):      # no subsample: (1, 1)
        make(tx=gref.target_axis(x, 0.3, 20), ty=gref.target_axis(y, -0.4, 30), method='fft-fine')


def test_restatement_at_s_1_is_the_tiled_one():
    r = tref.reference('ta-near')
    E, H = fref.fine_sum(*r['F'], r['x'], r['y'], gref.WL, gref.N_GLASS, r['tx'], r['ty'], r['z'], (1, 1), tile=r['tile'])
    assert np.array_equal(E, r['Enp']) and np.array_equal(H, r['Hnp'])


@pytest.mark.parametrize('case', sorted(fref.CASES))
def test_numpy_restatement_against_the_long_double_sum(case):
    r = fref.reference(case)
    mx, my = r['tx'].size, r['ty'].size
    assert {0, my - 1, (mx - 1) * my, mx * my - 1} <= set(r['sub'].tolist())     # the four corners
    assert r['sub'].size == mx * my or (mx * my > 700 and r['sub'].size >= mx * my // 7)
    for name, e_ref, e_np in zip('EH', r['e_ref'], r['e_np']):
        print('GRID %-16s %s: e_ref %.3e e_np %.3e ratio %.2f' % (case, name, e_ref, e_np, e_np / e_ref))
        assert e_np <= 32 * e_ref


@pytest.mark.parametrize('case', fref.RECORDED)
def test_the_recorded_long_double_sum_is_the_sum(case):
    """the record under tests/golden/ is used - it was made for these inputs - and on the corners and every 41st target
    it is the long-double sum taken afresh, exactly"""
    import propagate_ref as ref
    F, x, y, sub, pts = fref.points(case)
    with np.load(fref.GOLDEN % case) as g:
        assert str(g['key']) == fref._inputs_key(F, x, y, pts)
    El, Hl = fref.long_double_sum(case, F, x, y, pts)
    assert El.dtype == np.clongdouble and El.shape == (3, sub.size)
    pick = np.union1d(np.arange(0, sub.size, 41), [sub.size - 1])
    E, H = ref.direct_sum(*F, x, y, gref.WL, gref.N_GLASS, pts[pick], real=np.longdouble)
    assert np.array_equal(E, El[:, pick]) and np.array_equal(H, Hl[:, pick])
