"""``method='fft-stack'`` of the finite-distance propagator without a GPU: the stack plan of csrc/propagate_grid.h
(GridStackPlan) through tools/propagate_grid_stack.cpp against the plan of tests/propagate_grid_stack_ref.py, the order of
the layers and their pairs, the refusals of ``grid_stack_plan`` and of ``PlanePropagator`` that need no context, and the
NumPy restatement of the stack sum - ``fine_sum`` per plane - against the long-double direct sum of tests/propagate_ref.py.

Bound of the restatement: ``e_np <= 32 e_ref``, the condition of tests/test_propagate_grid_host.py - a cap that keeps the
yardstick of the GPU tests honest, not a measurement.  The ratios e_np / e_ref are printed (run with -s); measured (E, H):
1.20, 1.06 for 'sa-ragged', 1.43, 1.14 for 'sb-straddle' (both hold a plane 2 um behind the aperture), 0.96 ... 1.13 for
the others."""
import os
import subprocess

import numpy as np
import pytest

import propagate_grid_fine_ref as fref
import propagate_grid_ref as gref
import propagate_grid_stack_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('grid_stack')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'propagate_grid_stack_san'])

    def run(*args):
        res = subprocess.run([out + 'propagate_grid_stack_san'] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout
    return run


def _facts(line):
    return {k: int(v) for k, v in (kv.split('=') for kv in line.split())}


def _want(nx, ny, mx, my, nz, subsample, want_h, cached, tile=None):
    p = sref.plan(nx, ny, mx, my, nz, subsample, want_h, tile, cached)
    return dict(nz=nz, layers=p['layers'], sx=subsample[0], sy=subsample[1], ax=p['active'][0], ay=p['active'][1],
                mcx=p['lattice_targets'][0], mcy=p['lattice_targets'][1], cached=int(cached), Lx=p['L'][0], Ly=p['L'][1],
                cx=p['tiles'][0], cy=p['tiles'][1], bx=p['tile_samples'][0], by=p['tile_samples'][1],
                tiles=p['tiles'][0] * p['tiles'][1], batch=p['batch'], outputs=6 if want_h else 3, plane_bytes=p['plane_bytes'],
                workspace_bytes=p['workspace_bytes'], fill_layers=p['fill_layers'])


def _args(nx, ny, mx, my, subsample, want_h, cached, tile, z):
    return (nx, ny, mx, my, *subsample, want_h, cached, *(tile or (0, 0)), *z)


@pytest.mark.parametrize('cached', [1, 0], ids=['cached', 'streamed'])
@pytest.mark.parametrize('want_h', [1, 0], ids=['EH', 'E'])
@pytest.mark.parametrize('case', sorted(sref.CASES))
def test_plan_of_the_cases(tool, case, want_h, cached):
    nx, ny, mx, my, z = sref.CASES[case][:5]
    tile, subsample = sref.CASES[case][7:]
    want = _want(nx, ny, mx, my, len(z), subsample, want_h, cached, tile)
    stated = sref.PLANS[case]
    assert (want['Lx'], want['Ly']) == stated['L'] and (want['cx'], want['cy']) == stated['tiles']
    assert (want['bx'], want['by']) == stated['tile_samples'] and want['batch'] == stated['batch']
    assert (want['ax'], want['ay']) == stated['active'] and (want['mcx'], want['mcy']) == stated['lattice_targets']
    assert (want['nz'], want['layers']) == (stated['planes'], stated['layers'])
    assert _facts(tool(*_args(nx, ny, mx, my, subsample, want_h, cached, tile, z))) == want
    # both workspace formulas, written out: the cached one grows with the planes, the streamed one is the fine plan's
    A = want['ax'] * want['ay']
    planes = (8 * len(z) * A * want['tiles'] if cached else 16 * want['batch']) + 4 * want['tiles'] + 2 * want['outputs']
    assert want['workspace_bytes'] == planes * want['Lx'] * want['Ly'] * 16
    one = fref.plan(nx, ny, mx, my, subsample, want_h, tile, cached)
    if not cached or len(z) == 1:
        assert want['workspace_bytes'] == one['workspace_bytes']
    else:
        assert want['workspace_bytes'] - one['workspace_bytes'] == 8 * (len(z) - 1) * A * want['tiles'] * want['plane_bytes']
    # the fine plan inside does not depend on z: the same plan for the planes reversed, and for one of them
    assert _facts(tool(*_args(nx, ny, mx, my, subsample, want_h, cached, tile, z[::-1]))) == want
    alone = _facts(tool(*_args(nx, ny, mx, my, subsample, want_h, cached, tile, z[:1])))
    varies = ('nz', 'layers', 'workspace_bytes', 'fill_layers')
    assert {k: alone[k] for k in alone if k not in varies} == {k: want[k] for k in want if k not in varies}
    assert want['fill_layers'] == min(2, want['layers'])        # the cases are small: a pair goes into one fill launch


@pytest.mark.parametrize('case', sorted(sref.CASES))
def test_layer_order_and_pairs(tool, case):
    """l = p A + a Ay + b; pairs in that order, a single layer last if nz A is odd; what each case is there for"""
    nz, stated = len(sref.CASES[case][4]), sref.PLANS[case]
    order = sref.layers(nz, stated['active'])
    pairs = sref.pairs(len(order))
    assert len(order) == stated['layers'] and sorted(l for pr in pairs for l in pr) == list(range(len(order)))
    ax, ay = stated['active']
    for l, (p, a, b) in enumerate(order):
        assert l == p * ax * ay + a * ay + b
    out = tool('layers', nz, ax, ay).splitlines()
    assert out[:len(order)] == ['l=%d p=%d a=%d b=%d' % ((l,) + pab) for l, pab in enumerate(order)]
    assert out[len(order):] == ['pair=' + ','.join(str(l) for l in pr) for pr in pairs]
    assert all(len(pr) == sref.PAIR for pr in pairs[:-1]) and len(pairs[-1]) == (1 if len(order) % 2 else 2)
    straddling = [pr for pr in pairs if len({order[l][0] for l in pr}) == 2]
    if case == 'sb-straddle':
        assert pairs[-1] == (8,) and straddling == [(2, 3)] and [order[l] for l in (2, 3)] == [(0, 2, 0), (1, 0, 0)]
    if case == 'sc-planes':
        assert straddling == [(0, 1), (2, 3)] and pairs[-1] == (4,)
    if case in ('sa-ragged', 'sd-batches', 'se-far', 'sf-one'):
        assert not straddling and len(pairs[-1]) == 2


def test_plan_of_the_large_sizes(tool):
    """the workspaces the documentation quotes: 64^2 fine targets at half the pitch behind 4096^2"""
    sizes, subsample = (4096, 4096, 64, 64), (2, 2)
    for nz in (1, 8, 32):
        for cached in (1, 0):
            assert _facts(tool(*sizes, *subsample, 1, cached, 0, 0, '%d*20e-6' % nz)) == _want(*sizes, nz, subsample, 1, cached)
    streamed = [_facts(tool(*sizes, *subsample, 1, 0, 0, 0, '%d*20e-6' % nz))['workspace_bytes'] for nz in (1, 8, 32)]
    assert len(set(streamed)) == 1
    f = _facts(tool(*sizes, *subsample, 1, 1, 0, 0, '32*20e-6'))
    assert f['layers'] == 128 and f['workspace_bytes'] == (8 * 128 * f['tiles'] + 4 * f['tiles'] + 12) * f['plane_bytes']
    # a batch of 8 tiles of 512^2 is 256 MiB of kernel planes per layer: a fill launch per layer, the pair would be 512 MiB
    assert (f['batch'], f['plane_bytes'], f['fill_layers']) == (8, 512 * 512 * 16, 1)
    assert sref.fill_layers(1, 8, 512 * 512 * 16) == 1 and sref.fill_layers(2, 4, 512 * 512 * 16) == 2
    f = _facts(tool(1024, 1024, 64, 64, 2, 2, 1, 0, 128, 128, '2*20e-6'))      # tiles of 128^2: 64 a batch, 256 MiB the pair
    assert (f['batch'], f['plane_bytes'], f['fill_layers']) == (64, 128 * 128 * 16, 2)


def test_refusals(tool):
    base = (48, 40, 21, 31, 2, 3, 1, 1, 32, 32)
    for args, said in ((base, 'a stack has 1 to 4096 planes, got nz = 0'),
                       (base + ('4097*1e-6',), 'a stack has 1 to 4096 planes, got nz = 4097'),
                       (base + (20e-6, 0.0), 'plane 1 of the stack lies at z[1] = 0: the propagator needs a finite z > 0'),
                       (base + (-2e-6,), 'plane 0 of the stack lies at z[0] = -2e-06'),
                       (base + (20e-6, 2e-6, 'nan'), 'plane 2 of the stack lies at z[2] = nan'),
                       (base + ('inf', 2e-6), 'plane 0 of the stack lies at z[0] = inf'),
                       ((48, 40, 4096, 4096, 1, 1, 1, 0, 0, 0, '5*1e-6'),
                        '83886080 targets (5 planes of 4096 x 4096 fine targets): at most 2^26 per plan'),
                       # every refusal of the fine plan, unchanged
                       ((48, 40, 21, 31, 0, 3, 1, 1, 32, 32, 1e-6), 'x axis of n = 48 samples and m = 21 fine targets has s = 0'),
                       ((48, 40, 21, 31, 2, 9, 1, 1, 32, 32, 1e-6), 'y axis of n = 40 samples and m = 31 fine targets has s = 9'),
                       ((48, 40, 16386, 31, 2, 3, 1, 1, 0, 0, 1e-6), 'x axis of n = 48 samples has m = 16386 fine targets at s = 2, m_c = 8193'),
                       ((48, 40, 21, 31, 2, 3, 1, 1, 8, 32, 1e-6), 'x axis of n = 48 samples and m_c = 11 targets per lattice (m = 21 fine '
                                                                   'targets at s = 2) is L = 8'),
                       ((48, 40, 21, 31, 2, 3, 1, 1, 32, 48, 1e-6), 'y axis of n = 40 samples and m_c = 11 targets per lattice (m = 31 fine '
                                                                    'targets at s = 3) is L = 48'),
                       ((48, 40, 16384, 8192, 2, 1, 1, 1, 0, 0, 1e-6), '134217728 fine targets (16384 x 8192): at most 2^26 per plan')):
        out = tool(*args)
        assert out.startswith('refused=1\n') and said in out, out
    # the limits themselves are taken: 4096 planes, 2^26 targets
    f = _facts(tool(*base, '4096*1e-6'))
    assert (f['nz'], f['layers']) == (4096, 4096 * 6)
    assert _facts(tool(48, 40, 4096, 4096, 1, 1, 1, 0, 0, 0, '4*1e-6'))['nz'] == 4


def test_python_refusals_need_no_context(monkeypatch):
    from metalens_amd import _lib
    from metalens_amd import propagate
    monkeypatch.setattr(_lib, 'default_context', lambda: pytest.fail('a context was asked for'))
    assert propagate.METHODS.index('fft-stack') == 5
    assert propagate.METHODS[:5] == ('direct', 'fft', 'fft-long', 'fft-tiled', 'fft-fine')
    x, y = gref.axis(48), gref.axis(40)
    tx, ty = fref.fine_axis(x, 0.3, 21, 2), fref.fine_axis(y, -0.4, 31, 3)
    args = (x, y, gref.WL, gref.N_GLASS)
    planes = (20e-6, 2e-6, 5e-6)

    def make(tx=tx, ty=ty, z=planes, method='fft-stack', **kw):
        if method == 'fft-stack':
            kw.setdefault('subsample', (2, 3))
        return propagate.PlanePropagator(*args, tx, ty, z, method=method, **kw)
    # the new refusals
    with pytest.raises(ValueError, match='no targets'):
        make(z=())
    with pytest.raises(ValueError, match="method='fft-stack' takes 1 to 4096 planes, got 4097"):
        make(z=np.full(4097, 2e-6))
    for bad, said in (((20e-6, 0.0), r'plane 1 lies at z\[1\] = 0:'), ((-2e-6,), r'plane 0 lies at z\[0\] = -2e-06:'),
                      ((20e-6, 2e-6, np.nan), r'plane 2 lies at z\[2\] = nan:'), ((np.inf, 2e-6), r'plane 0 lies at z\[0\] = inf:')):
        with pytest.raises(ValueError, match=said):
            make(z=bad)
    with pytest.raises(ValueError, match=r'83886080 targets \(5 planes of 4096 x 4096 fine targets\): at most 2\^26'):
        make(tx=fref.fine_axis(x, 0.0, 4096, 1), ty=fref.fine_axis(y, 0.0, 4096, 1), z=np.full(5, 1e-6), subsample=(1, 1))
    with pytest.raises(ValueError, match='not a point list'):
        make(ty=tx, z=np.full(tx.size, 2e-6), point_list=True)
    # an axis off the fine pitch
    with pytest.raises(ValueError, match=r"method='fft-stack' needs the targets on the aperture's pitch / 2: x\[1\]"):
        make(tx=gref.target_axis(x, 0.3, 21))
    off = ty.copy()
    off[17] += 1e-6 * (y[1] - y[0])
    with pytest.raises(ValueError, match=r"aperture's pitch / 3: y\[17\]"):
        make(ty=off)
    # the refusals of the fine method, with this method's name
    with pytest.raises(ValueError, match=r"method='fft-stack' divides the aperture's pitch by an integer in \[1, 8\]: .* has s = 9 along y"):
        make(subsample=(2, 9))
    with pytest.raises(ValueError, match=r"method='fft-stack': the tile length of the x axis of n = 48 samples and m_c = 11 targets per "
                                         r"lattice \(m = 21 fine targets at s = 2\) is L = 8"):
        make(tile=(8, 32))
    with pytest.raises(ValueError, match='tile must be None or the two tile lengths'):
        make(tile=(32,))
    with pytest.raises(ValueError, match="method='fft-stack' takes at most 8192 targets per lattice and axis: the x axis of n = 48 samples "
                                         "has m = 16386 fine targets at s = 2, m_c = 8193 per lattice"):
        make(tx=fref.fine_axis(x, 0.0, 16386, 2), z=(2e-6,))
    # several z stay an error everywhere else, word for word
    coarse = dict(tx=gref.target_axis(x, 0.3, 20), ty=gref.target_axis(y, -0.4, 30))
    for method in ('direct', 'fft', 'fft-long', 'fft-tiled', 'fft-fine'):
        with pytest.raises(ValueError, match=r'a tensor grid of targets lies in one plane: z must be one number, got 3 '
                                             r'\(point_list=True takes a z per point\)'):
            make(method=method, **coarse)
    for method in ('direct', 'fft', 'fft-long', 'fft-tiled'):
        with pytest.raises(ValueError, match="pitch ratios belong to method='fft-fine', not to method='%s'" % method):
            make(method=method, z=2e-6, subsample=(2, 3))
        with pytest.raises(ValueError, match="cache_kernels=False: the choice belongs to method='fft-fine', not to method='%s'" % method):
            make(method=method, z=2e-6, cache_kernels=False, **coarse)
    with pytest.raises(ValueError, match="tile lengths belong to method='fft-tiled', not to method='fft'"):
        make(method='fft', z=2e-6, tile=(32, 32))
    # with the checks passed the constructor goes on to the context: any number of planes, any order, repeats
    for kw in (dict(), dict(tile=(32, 32)), dict(tile=(16, 0)), dict(cache_kernels=False), dict(z=(5e-6,)), dict(z=5e-6),
               dict(z=(5e-6, 5e-6, 1e-6)), dict(z=np.full(4096, 2e-6))):
        with pytest.raises(pytest.fail.Exception, match='a context was asked for'):
            make(**kw)
    with pytest.raises(pytest.fail.Exception, match='a context was asked for'):      # no subsample: (1, 1)
        propagate.PlanePropagator(*args, coarse['tx'], coarse['ty'], planes, method='fft-stack')


def test_restatement_of_one_plane_is_the_fine_one():
    r = fref.reference('fa-ragged')
    E, H = sref.stack_sum(*r['F'], r['x'], r['y'], gref.WL, gref.N_GLASS, r['tx'], r['ty'], [r['z']], r['subsample'], tile=r['tile'])
    assert np.array_equal(E, r['Enp']) and np.array_equal(H, r['Hnp'])


@pytest.mark.parametrize('case', sorted(sref.CASES))
def test_numpy_restatement_against_the_long_double_sum(case):
    r = sref.reference(case)
    nz, mx, my = r['z'].size, r['tx'].size, r['ty'].size
    T = nz * mx * my
    assert set(sref.corners(nz, mx, my)) <= set(r['sub'].tolist())     # the four corners of every plane
    assert r['sub'].size == T or (T > 700 and r['sub'].size >= T // 7)
    assert np.array_equal(r['pts'][:, 2], r['z'][r['sub'] // (mx * my)])
    for name, e_ref, e_np in zip('EH', r['e_ref'], r['e_np']):
        print('GRID %-16s %s: e_ref %.3e e_np %.3e ratio %.2f' % (case, name, e_ref, e_np, e_np / e_ref))
        assert e_np <= 32 * e_ref
