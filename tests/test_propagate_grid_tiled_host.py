"""``method='fft-tiled'`` of the finite-distance propagator without a GPU: the tiled plan of csrc/propagate_grid.h
(GridTilePlan) through tools/propagate_grid_tiled.cpp against the chooser of tests/propagate_grid_tiled_ref.py, the
refusals of ``PlanePropagator`` that need no context, and the NumPy restatement of the tiled sum against the long-double
direct sum of tests/propagate_ref.py.

Bound of the restatement: ``e_np <= 32 e_ref``, the condition of tests/test_propagate_grid_host.py - a cap that keeps the
yardstick of the GPU tests honest, not a measurement.  Measured ratios e_np / e_ref: 0.88 ... 1.12 for 'ta-near' ...
'tg-default' and the 'te' cases, 1.95 for 'tf-beyond' (on the 16 targets of its subset)."""
import os
import subprocess

import numpy as np
import pytest

import propagate_grid_ref as gref
import propagate_grid_tiled_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tools(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('grid_tiled')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'propagate_grid_tiled_san',
                           out + 'propagate_grid_san'])

    def run(name, *args):
        res = subprocess.run([out + name] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout
    return run


@pytest.fixture
def tool(tools):
    return lambda *args: tools('propagate_grid_tiled_san', *args)


def _facts(line):
    return {k: int(v) for k, v in (kv.split('=') for kv in line.split())}


def _want(nx, ny, mx, my, want_h, tile=None, batch_bytes=tref.BATCH_BYTES):
    p = tref.plan(nx, ny, mx, my, want_h, tile, batch_bytes)
    return dict(Lx=p['L'][0], Ly=p['L'][1], cx=p['tiles'][0], cy=p['tiles'][1], bx=p['tile_samples'][0], by=p['tile_samples'][1],
                tiles=p['tiles'][0] * p['tiles'][1], batch=p['batch'], outputs=6 if want_h else 3, plane_bytes=p['plane_bytes'],
                workspace_bytes=p['workspace_bytes'])


@pytest.mark.parametrize('nm', sorted(tref.DEFAULTS))
def test_default_tile_length(tool, nm):
    n, m = nm
    L, c = tref.DEFAULTS[nm]
    assert tref.tile_default(n, m) == L and tref.tiles_of(n, m, L)[1] == c
    assert _facts(tool('default', n, m)) == dict(L=L, B=L - m + 1, c=c)
    from metalens_amd.propagate import tile_default
    assert tile_default(n, m) == L
    # no admissible length has a smaller weighted padded length, and no larger one as small a one
    costs = {1 << e: (tref.tiles_of(n, m, 1 << e)[1] << e) * tref.WEIGHT.get(1 << e, 32) for e in range(4, 14) if (1 << e) >= m}
    assert costs[L] == min(costs.values()) and all(cost > costs[L] for length, cost in costs.items() if length > L)


def test_the_weights_of_the_default():
    """the cost of a padded sample per tile length, 32nds: flat up to 512, then the square roots of the measured time per
    padded area of a pass, 1.08 : 1.37 : 1.88 : 2.14 at 512 : 1024 : 2048 : 4096, to 1 %"""
    assert tref.WEIGHT == {1024: 36, 2048: 42, 4096: 45, 8192: 45}
    for L, per_area in ((1024, 1.37), (2048, 1.88), (4096, 2.14)):
        assert abs(tref.WEIGHT[L] / 32 - (per_area / 1.08) ** 0.5) < 0.01


def test_a_problem_of_one_tile_takes_the_length_of_the_untiled_plan(tool):
    for n, m in ((48, 20), (40, 30), (61, 24), (35, 17), (40, 25), (4097, 4096), (1, 1)):
        L = gref.padded_length(n, m)
        assert tref.tile_default(n, m) == L and tref.tiles_of(n, m, L)[1] == 1
        assert _facts(tool('default', n, m)) == dict(L=L, B=L - m + 1, c=1)


@pytest.mark.parametrize('case', sorted(tref.CASES))
@pytest.mark.parametrize('want_h', [1, 0], ids=['EH', 'E'])
def test_plan_of_the_cases(tool, case, want_h):
    nx, ny, mx, my = tref.CASES[case][:4]
    tile = tref.CASES[case][7]
    want = _want(nx, ny, mx, my, want_h, tile)
    stated = tref.PLANS[case]
    assert (want['Lx'], want['Ly']) == stated['L'] and (want['cx'], want['cy']) == stated['tiles']
    assert (want['bx'], want['by']) == stated['tile_samples'] and want['batch'] == stated['batch']
    assert _facts(tool(nx, ny, mx, my, want_h, *(tile or ()))) == want
    if tile:   # one length given, the other left to the chooser
        assert _facts(tool(nx, ny, mx, my, want_h, tile[0], 0)) == _want(nx, ny, mx, my, want_h, (tile[0], 0))
    # every sample lies in exactly one tile, the last tile of an axis holds at least one
    for n, B, c in ((nx, want['bx'], want['cx']), (ny, want['by'], want['cy'])):
        assert (c - 1) * B < n <= c * B


@pytest.mark.parametrize('sizes,tile', [((8192, 8192, 64, 64), None), ((4096, 4096, 64, 64), None), ((4096, 4096, 256, 256), None),
                                        ((16384, 16384, 64, 64), None), ((2048, 2048, 64, 64), None),
                                        ((8192, 8192, 64, 64), (512, 2048)), ((16384, 16384, 64, 64), (8192, 8192))])
def test_plan_of_the_large_sizes(tool, sizes, tile):
    for want_h in (1, 0):
        assert _facts(tool(*sizes, want_h, *(tile or ()))) == _want(*sizes, want_h, tile)
    p = tref.plan(*sizes, True, tile)
    assert p['batch'] == min(p['tiles'][0] * p['tiles'][1], 64, max(1, (128 << 20) // (4 * p['plane_bytes'])))


def test_workspace_and_batch(tool):
    # 8192^2 -> 64^2 at 1024: 81 tiles; a plane is 16 MiB, so a batch is two tiles; 8 x 81 + 8 + 6 planes: beyond 2^32 bytes
    f = _facts(tool(8192, 8192, 64, 64, 1, 1024, 1024))
    assert (f['Lx'], f['cx'], f['bx'], f['tiles'], f['batch']) == (1024, 9, 961, 81, 2)
    assert f['workspace_bytes'] == (8 * 81 + 4 * 2 + 6) * 1024 * 1024 * 16 > 2 ** 32
    assert _facts(tool(8192, 8192, 64, 64, 0, 1024, 1024))['workspace_bytes'] == (8 * 81 + 4 * 2 + 3) * 1024 * 1024 * 16
    # ... and by default, at 512: 361 tiles in batches of 8
    f = _facts(tool(8192, 8192, 64, 64, 1))
    assert (f['Lx'], f['cx'], f['bx'], f['tiles'], f['batch']) == (512, 19, 449, 361, 8)
    assert f['workspace_bytes'] == (8 * 361 + 4 * 8 + 6) * 512 * 512 * 16 > 2 ** 32
    # 16384^2 -> 64^2 at 2048: a plane is 64 MiB and the batch's bytes hold no tile whole: one tile at a time
    f = _facts(tool(16384, 16384, 64, 64, 1, 2048, 2048))
    assert (f['Lx'], f['cx'], f['batch']) == (2048, 9, 1) and f['workspace_bytes'] == (8 * 81 + 4 + 6) * 2048 * 2048 * 16
    # the batch bytes of the diagnostic build: 32, 128, 512 MiB
    for mib, batch in ((32, 2), (128, 8), (512, 32)):
        f = _facts(tool(4096, 4096, 64, 64, 1, 512, 512, mib))
        assert f == _want(4096, 4096, 64, 64, 1, (512, 512), mib << 20) and f['batch'] == batch
    # structural: 64 tiles at the most, whatever the bytes allow
    assert _facts(tool(97, 80, 30, 25, 1, 32, 32))['batch'] == 64 and _facts(tool(97, 80, 30, 25, 1, 32, 32))['tiles'] == 330


def test_refusals(tool):
    for args, said in (((48, 40, 20, 30, 1, 16, 64), 'x axis of n = 48 samples and m = 20 targets is L = 16'),
                       ((48, 40, 20, 30, 1, 32, 16), 'y axis of n = 40 samples and m = 30 targets is L = 16'),
                       ((48, 40, 20, 30, 1, 48, 64), 'x axis of n = 48 samples and m = 20 targets is L = 48'),
                       ((48, 40, 20, 30, 1, 32, 16384), 'y axis of n = 40 samples and m = 30 targets is L = 16384'),
                       ((48, 40, 2, 3, 1, 8, 16), 'x axis of n = 48 samples and m = 2 targets is L = 8'),
                       ((48, 40, 20, 30, 1, -32, 64), 'x axis of n = 48 samples and m = 20 targets is L = -32'),
                       ((48, 40, 8193, 30, 1), 'x axis of n = 48 samples has m = 8193 targets'),
                       ((48, 40, 20, 8193, 0, 32, 8192), 'y axis of n = 40 samples has m = 8193 targets')):
        out = tool(*args)
        assert out.startswith('refused=1\n') and said in out, out
    assert not tool(48, 40, 8192, 30, 1).startswith('refused')     # m = 8192: one tile length is left
    assert _facts(tool(48, 40, 8192, 30, 1))['Lx'] == 8192 and _facts(tool(48, 40, 8192, 30, 1))['cx'] == 48


def test_lag_rule(tool):
    """index p of tile a's kernel plane holds (p < m ? p : p - L) - a B: over the tiles of an axis every lag of the
    problem, target minus sample, is held where the circular convolution of the tile's local indices looks for it"""
    for n, m, L in ((48, 20, 32), (40, 30, 64), (48, 1, 16), (97, 30, 32)):
        B, c = tref.tiles_of(n, m, L)
        for a in range(c):
            lag = np.array(tool('lag', L, m, a, B).split(), dtype=int)
            assert np.array_equal(lag, tref.tile_lags(L, m, a, B))
            for s in range(a * B, min(n, a * B + B)):          # sample s at the local index s - a B
                i = np.arange(m)
                assert np.array_equal(lag[np.mod(i - (s - a * B), L)], i - s)
    assert np.array_equal(tref.tile_lags(64, 25, 0, 40), gref.lags(64, 25))     # tile 0: the lags of the untiled plan


def test_the_existing_tool_is_unchanged(tools):
    """the lines of the parent commit's tools/propagate_grid.cpp, byte for byte"""
    tool = lambda *args: tools('propagate_grid_san', *args)   # noqa: E731
    assert tool(40, 20, 25, 12, 1) == 'Lx=64 Ly=32 outputs=6 plane_bytes=32768 workspace_bytes=589824\n'
    assert tool(20, 4097, 12, 4096, 0) == 'Lx=32 Ly=8192 outputs=3 plane_bytes=4194304 workspace_bytes=62914560\n'
    assert tool(4097, 20, 4097, 12, 1) == (
        'refused=1\nthe FFT form pads the x axis of n = 4097 samples and m = 4097 targets to L = 16384 > 8192 (one row of L '
        'complex128 must fit the LDS); use the direct method or fewer targets per plan\n')
    assert tool(8193, 20, 8192, 12, 1, 16384).splitlines()[1:] == [
        'route axis=rows L=32 top_stages=0 lds_len=32 forward=lds back=lds',
        'route axis=columns L=16384 top_stages=4 lds_len=1024 forward=top,lds back=lds,top']


def test_python_refusals_need_no_context(monkeypatch):
    from metalens_amd import _lib
    from metalens_amd import propagate
    monkeypatch.setattr(_lib, 'default_context', lambda: pytest.fail('a context was asked for'))
    assert propagate.METHODS.index('fft-tiled') == 3 and propagate.METHODS[:3] == ('direct', 'fft', 'fft-long')
    x, y = gref.axis(48), gref.axis(40)
    tx, ty = gref.target_axis(x, 0.3, 20), gref.target_axis(y, -0.4, 30)
    args = (x, y, gref.WL, gref.N_GLASS)

    def make(tx=tx, ty=ty, z=2e-6, **kw):
        return propagate.PlanePropagator(*args, tx, ty, z, **kw)
    with pytest.raises(ValueError, match='x axis of n = 48 samples and m = 20 targets is L = 16'):     # below m
        make(method='fft-tiled', tile=(16, 64))
    with pytest.raises(ValueError, match='y axis of n = 40 samples and m = 30 targets is L = 48'):     # no power of two
        make(method='fft-tiled', tile=(32, 48))
    with pytest.raises(ValueError, match='y axis of n = 40 samples and m = 30 targets is L = 16384'):
        make(method='fft-tiled', tile=(32, 16384))
    with pytest.raises(ValueError, match='x axis of n = 48 samples and m = 20 targets is L = 32.5'):
        make(method='fft-tiled', tile=(32.5, 64))
    with pytest.raises(ValueError, match='tile must be None or the two tile lengths'):
        make(method='fft-tiled', tile=(32,))
    with pytest.raises(ValueError, match='x axis of n = 48 samples has m = 8193 targets'):
        make(tx=gref.target_axis(x, 0.0, 8193), method='fft-tiled')
    for method in ('direct', 'fft', 'fft-long'):
        with pytest.raises(ValueError, match="tile lengths belong to method='fft-tiled', not to method='%s'" % method):
            make(method=method, tile=(32, 64))
    # the checks of 'fft': on the pitch, a tensor grid
    off = tx.copy()
    off[11] += 1e-6 * (x[1] - x[0])
    with pytest.raises(ValueError, match=r"aperture's pitch: x\[11\]"):
        make(tx=off, method='fft-tiled')
    with pytest.raises(ValueError, match='not a point list'):
        make(ty=tx, z=np.full(tx.size, 2e-6), point_list=True, method='fft-tiled')
    # with the checks passed the constructor goes on to the context: the default, given lengths, one left to the chooser
    for tile in (None, (32, 64), (0, 64), (8192, 8192)):
        with pytest.raises(pytest.fail.Exception, match='a context was asked for'):
            make(method='fft-tiled', tile=tile)
    with pytest.raises(ValueError, match='method must be one of'):
        make(method='auto')


def test_restatement_of_one_tile_is_the_untiled_one():
    """a plan of one tile is the sum of propagate_grid_ref.grid_sum: the same planes, the same transforms"""
    r = gref.reference('c-far')
    E, H = tref.tiled_sum(*r['F'], r['x'], r['y'], gref.WL, gref.N_GLASS, r['tx'][0], r['ty'][0], r['tx'].size, r['ty'].size,
                          r['z'])
    assert np.array_equal(E, r['Enp']) and np.array_equal(H, r['Hnp'])
    t = tref.reference('tc-far')
    assert all(np.array_equal(a, b) for a, b in zip(t['F'], r['F'])) and np.array_equal(t['tx'], r['tx'])
    assert np.array_equal(t['Enp'], r['Enp'])


@pytest.mark.parametrize('case', sorted(tref.CASES))
def test_numpy_restatement_against_the_long_double_sum(case):
    r = tref.reference(case)
    mx, my = r['tx'].size, r['ty'].size
    assert {0, my - 1, (mx - 1) * my, mx * my - 1} <= set(r['sub'].tolist())     # the four corners
    assert r['sub'].size >= min(16, mx * my)
    for name, e_ref, e_np in zip('EH', r['e_ref'], r['e_np']):
        print('GRID %-14s %s: e_ref %.3e e_np %.3e ratio %.2f' % (case, name, e_ref, e_np, e_np / e_ref))
        assert e_np <= 32 * e_ref
