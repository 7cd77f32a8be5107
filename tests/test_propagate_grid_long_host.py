"""``method='fft-long'`` of the finite-distance propagator without a GPU: the plan arithmetic of csrc/propagate_grid.h with the
long cap and the route of an axis through tools/propagate_grid.cpp, the refusals of ``PlanePropagator`` that need no
context, the two-pass transform restated in NumPy, and the NumPy FFT form of the cases of
tests/propagate_grid_long_ref.py against the long-double direct sum.

Bound of the restatement: ``e_np <= 32 e_ref``, the condition of tests/test_propagate_grid_host.py - a cap that keeps
the yardstick of the GPU tests honest, not a measurement.  Measured ratios e_np / e_ref (E / H): 1.00 for 'i-5000' and
'i-5000-y', 1.15 / 1.18 for 'j-both', 2.9 / 2.6 for 'h-long' and 2.4 / 4.4 for 'h-long-y' (at z = 30 um the exact-fit
cases reach 11 ... 15, hence their z = 200 um).

Bound of the two-pass transform against ``numpy.fft``: both are radix-2-like sums of log2 L stages, each rounding a
butterfly to a few 2^-53 of its magnitude; 16 log2(L) 2^-53 of the largest output covers either one's error with room."""
import os
import subprocess

import numpy as np
import pytest

import propagate_grid_long_ref as lref
import propagate_grid_ref as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('grid_long')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'propagate_grid_san'])

    def run(*args):
        res = subprocess.run([out + 'propagate_grid_san'] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout
    return run


def _facts(line):
    return dict(kv.split('=') for kv in line.split())


def test_long_cap_accepts_16384(tool):
    lines = tool(8193, 20, 8192, 12, 1, 16384).splitlines()
    facts = _facts(lines[0])
    assert facts['Lx'] == '16384' and facts['Ly'] == '32' and facts['outputs'] == '6'
    assert facts['plane_bytes'] == str(16384 * 32 * 16) and facts['workspace_bytes'] == str(18 * 16384 * 32 * 16)
    facts = _facts(tool(20, 8193, 12, 8192, 0, 16384).splitlines()[0])
    assert facts['Lx'] == '32' and facts['Ly'] == '16384' and facts['workspace_bytes'] == str(15 * 16384 * 32 * 16)
    # both axes long: 77 GB (64 GB without H), past 2^31 elements and 2^32 bytes
    facts = _facts(tool(8193, 8193, 8192, 8192, 1, 16384).splitlines()[0])
    assert facts['workspace_bytes'] == str(18 * 16384 * 16384 * 16) and int(facts['workspace_bytes']) > 77e9
    assert _facts(tool(8193, 8193, 8192, 8192, 0, 16384).splitlines()[0])['workspace_bytes'] == str(15 * 16384 * 16384 * 16)
    assert gref.padded_length(8193, 8192) == 16384 == lref.L_LONG_MAX


def test_long_cap_refuses_32768(tool):
    out = tool(8193, 20, 8193, 12, 1, 16384)
    assert out.startswith('refused=1')
    assert 'x axis of n = 8193 samples and m = 8193 targets to L = 32768 > 16384' in out
    out = tool(20, 8193, 12, 8193, 0, 16384)
    assert out.startswith('refused=1') and 'y axis of n = 8193 samples and m = 8193 targets to L = 32768 > 16384' in out
    assert gref.padded_length(8193, 8193) == 32768


@pytest.mark.parametrize('sizes', [(8193, 20, 8192, 12), (20, 8193, 12, 8192), (8193, 8193, 8192, 8192), (4097, 20, 4096, 12),
                                   (20, 4097, 12, 4096), (1025, 600, 1000, 425), (48, 40, 20, 30), (8200, 70, 100, 60)])
def test_printed_route(tool, sizes):
    """the route of either axis as the tool prints it against the helper's, for axes in the LDS alone (rows up to 8192,
    columns up to 1024), columns with one streaming pass of 1 ... 3 stages as 'fft' runs them, and the long axes"""
    nx, ny, mx, my = sizes
    lines = tool(nx, ny, mx, my, 1, 16384).splitlines()
    assert len(lines) == 3
    Lx, Ly = gref.padded_length(nx, mx), gref.padded_length(ny, my)
    for line, name, L, columns in ((lines[1], 'rows', Ly, False), (lines[2], 'columns', Lx, True)):
        words = line.split()
        assert words[0] == 'route'
        got = _facts(' '.join(words[1:]))
        want = lref.axis_route(L, columns)
        assert got == {'axis': name, 'L': str(L), 'top_stages': str(want['top_stages']), 'lds_len': str(want['lds_len']),
                       'forward': want['forward'], 'back': want['back']}
        assert want['lds_len'] << want['top_stages'] == L
    # what 'fft' runs today, stated outright: rows whole up to 8192, columns in blocks of 1024 under 1 ... 3 stages
    for L in (16, 1024, 8192):
        assert lref.axis_route(L, False) == dict(top_stages=0, lds_len=L, forward='lds', back='lds')
    for L, top in ((16, 0), (1024, 0), (2048, 1), (4096, 2), (8192, 3), (16384, 4)):
        assert lref.axis_route(L, True)['top_stages'] == top and lref.axis_route(L, True)['lds_len'] == min(L, 1024)
    assert lref.axis_route(16384, False) == dict(top_stages=2, lds_len=4096, forward='top,lds', back='lds,top')


def test_output_without_the_cap_is_unchanged(tool):
    """the lines of the parent commit's tool, byte for byte"""
    assert tool(40, 20, 25, 12, 1) == 'Lx=64 Ly=32 outputs=6 plane_bytes=32768 workspace_bytes=589824\n'
    assert tool(20, 4097, 12, 4096, 0) == 'Lx=32 Ly=8192 outputs=3 plane_bytes=4194304 workspace_bytes=62914560\n'
    assert tool(4097, 20, 4097, 12, 1) == (
        'refused=1\nthe FFT form pads the x axis of n = 4097 samples and m = 4097 targets to L = 16384 > 8192 (one row of L '
        'complex128 must fit the LDS); use the direct method or fewer targets per plan\n')
    assert tool(8193, 20, 8192, 12, 1).startswith('refused=1\n') and '> 8192 (one row' in tool(8193, 20, 8192, 12, 1)


def test_python_refusals_need_no_context(monkeypatch):
    from metalens_amd import _lib
    from metalens_amd import propagate
    monkeypatch.setattr(_lib, 'default_context', lambda: pytest.fail('a context was asked for'))
    assert 'fft-long' in propagate.METHODS and propagate.METHODS.index('fft-long') == 2
    assert propagate._padded_length(8193, 8192) == 16384 and propagate._padded_length(8193, 8193) == 32768
    x, y = gref.axis(48), gref.axis(40)
    tx, ty = gref.target_axis(x, 0.3, 20), gref.target_axis(y, -0.4, 30)
    long_x = gref.target_axis(x, 0.0, 16384 - 48 + 2)
    with pytest.raises(ValueError, match=r"method='fft-long' pads the x axis of n = 48 samples and m = 16338 targets to L = 32768 > 16384"):
        propagate.PlanePropagator(x, y, gref.WL, gref.N_GLASS, long_x, ty, 2e-6, method='fft-long')
    long_y = gref.target_axis(y, 0.0, 16384 - 40 + 2)
    with pytest.raises(ValueError, match='the y axis of n = 40 samples and m = 16346 targets to L = 32768 > 16384'):
        propagate.PlanePropagator(x, y, gref.WL, gref.N_GLASS, tx, long_y, 2e-6, method='fft-long')
    # the checks of 'fft': on the pitch, a tensor grid
    off = tx.copy()
    off[11] += 1e-6 * (x[1] - x[0])
    with pytest.raises(ValueError, match=r"aperture's pitch: x\[11\]"):
        propagate.PlanePropagator(x, y, gref.WL, gref.N_GLASS, off, ty, 2e-6, method='fft-long')
    with pytest.raises(ValueError, match='not a point list'):
        propagate.PlanePropagator(x, y, gref.WL, gref.N_GLASS, tx, tx, np.full(tx.size, 2e-6), point_list=True, method='fft-long')
    # 'fft-long' is a method: with the checks passed the constructor goes on to the context
    with pytest.raises(pytest.fail.Exception, match='a context was asked for'):
        propagate.PlanePropagator(x, y, gref.WL, gref.N_GLASS, tx, ty, 2e-6, method='fft-long')
    with pytest.raises(ValueError, match='method must be one of'):
        propagate.PlanePropagator(x, y, gref.WL, gref.N_GLASS, tx, ty, 2e-6, method='auto')


@pytest.mark.parametrize('L,R', [(64, 0), (64, 2), (64, 3), (16384, 1), (16384, 2), (16384, 4)])
def test_two_pass_transform_is_the_fft(L, R):
    """top R stages on the whole sequence, then independent transforms of blocks of L >> R: numpy.fft.fft in bit-reversed
    order, and the decimation-in-time passes undo it (times L)"""
    rng = np.random.default_rng(L + R)
    v = rng.normal(size=L) + 1j * rng.normal(size=L)
    got = lref.two_level(v, R)
    want = np.fft.fft(v)
    tol = 16 * np.log2(L) * EPS * np.abs(want).max()
    assert np.abs(got - want[lref.bit_reversed(L)]).max() <= tol
    assert np.array_equal(lref.bit_reversed(L)[lref.bit_reversed(L)], np.arange(L))
    # the same stages whatever the split (the butterflies of a stage do not depend on which pass runs them)
    assert np.array_equal(got, lref.two_level(v, 0))
    back = lref.two_level(got, R, inverse=True)
    assert np.abs(back / L - v).max() <= 16 * np.log2(L) * EPS * np.abs(v).max()
    assert np.array_equal(back, lref.two_level(got, 0, inverse=True))


@pytest.mark.parametrize('case', sorted(lref.CASES))
def test_numpy_restatement_against_the_long_double_sum(case):
    r = lref.reference(case)
    nx, ny, mx, my = lref.CASES[case][:4]
    assert (gref.padded_length(nx, mx), gref.padded_length(ny, my)) == lref.PADDED[case]
    assert r['sub'].size == 16 and {0, my - 1, (mx - 1) * my, mx * my - 1} <= set(r['sub'].tolist())
    for name, e_ref, e_np in zip('EH', r['e_ref'], r['e_np']):
        print('GRID %-10s %s: e_ref %.3e e_np %.3e ratio %.2f' % (case, name, e_ref, e_np, e_np / e_ref))
        assert e_np <= 32 * e_ref
