"""The FFT form of the finite-distance propagator without a GPU: the plan arithmetic of csrc/propagate_grid.h through
tools/propagate_grid.cpp, and the NumPy restatement (tests/propagate_grid_ref.py) against the long-double direct sum
of tests/propagate_ref.py.

Bound of the restatement.  ``e_np <= 32 e_ref`` with both errors as in tests/test_gpu_propagate.py (max |difference|
over components and targets / max |field| of the long-double sum), ``e_ref`` the plain fp64 direct sum's: the FFT
form is the same sum in another order, whose rounding grows with log L and with the dynamic range of the kernel
planes - measured 1.0 ... 15.5 x e_ref over these cases (the worst at z = 2 um), and twice that because another seed
moves it."""
import os
import subprocess

import numpy as np
import pytest

import propagate_grid_ref as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('grid')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'propagate_grid_san'])

    def run(*args):
        res = subprocess.run([out + 'propagate_grid_san'] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout
    return run


@pytest.mark.parametrize('n,m,L', [(40, 25, 64), (40, 26, 128), (1, 1, 16), (4097, 4096, 8192)])
def test_padded_length(tool, n, m, L):
    facts = dict(kv.split('=') for kv in tool(n, 20, m, 12, 1).split())
    assert facts['Lx'] == str(L) and facts['Ly'] == '32'
    assert facts['workspace_bytes'] == str(18 * L * 32 * 16) and facts['outputs'] == '6'
    facts = dict(kv.split('=') for kv in tool(20, n, 12, m, 0).split())      # the same rule along y; E only
    assert facts['Ly'] == str(L) and facts['Lx'] == '32' and facts['workspace_bytes'] == str(15 * L * 32 * 16)
    assert gref.padded_length(n, m) == L


def test_too_long_an_axis_is_refused(tool):
    out = tool(4097, 20, 4097, 12, 1)
    assert out.startswith('refused=1')
    assert 'x axis of n = 4097 samples and m = 4097 targets to L = 16384' in out
    out = tool(20, 4097, 12, 4097, 1)
    assert out.startswith('refused=1') and 'y axis of n = 4097 samples and m = 4097 targets to L = 16384' in out
    assert gref.padded_length(4097, 4097) == 16384 > gref.L_MAX


def test_lag_indexing(tool):
    for n, m in ((40, 25), (40, 26), (1, 1), (5, 12)):
        L = gref.padded_length(n, m)
        lag = np.array(tool('lag', L, m).split(), dtype=int)
        assert np.array_equal(lag, gref.lags(L, m))
        # every lag of the problem has an index of its own
        want = np.arange(-(n - 1), m)
        assert np.array_equal(np.sort(lag[np.mod(want, L)]), want)


def test_twiddle_table_is_rounded_once(tool):
    for L in (16, 1024, 8192):
        out = dict(kv.split('=') for kv in tool('twiddles', L).split())
        assert out['entries'] == str(L // 2) and float(out['worst_ulp53']) <= 1.0    # half an ulp of a number in [0.5, 1]


@pytest.mark.parametrize('case', gref.HOST_CASES)
def test_numpy_restatement_against_the_long_double_sum(case):
    r = gref.reference(case)
    assert r['sub'].size >= 50
    for name, e_ref, e_np in zip('EH', r['e_ref'], r['e_np']):
        print('GRID %-16s %s: e_ref %.3e e_np %.3e ratio %.2f' % (case, name, e_ref, e_np, e_np / e_ref))
        assert e_np <= 32 * e_ref


def test_python_pitch_rule():
    """the acceptance rule of PlanePropagator(method='fft') on the host (no context is made before it fails)"""
    from metalens_amd.propagate import _on_pitch, _padded_length
    x = gref.axis(48)
    d = x[1] - x[0]
    _on_pitch('x', gref.target_axis(x, -30.25, 70), d)
    _on_pitch('x', np.array([1.234e-6]), d)
    t = gref.target_axis(x, 0.3, 20)
    t[7] += 1e-6 * d
    with pytest.raises(ValueError, match=r'x\[7\]'):
        _on_pitch('x', t, d)
    with pytest.raises(ValueError, match=r'x\[1\]'):
        _on_pitch('x', gref.target_axis(x, 0.3, 20) * 1.5, d)
    assert [_padded_length(*nm) for nm in ((40, 25), (40, 26), (1, 1), (4097, 4096), (4097, 4097))] == [64, 128, 16, 8192, 16384]
