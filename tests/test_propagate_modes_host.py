"""The overlap of a propagated image with separable modes without a GPU: the yardstick (tests/propagate_modes_ref.py) on a
plane worked by hand, the argument checks, the caps and the launch shapes of csrc/propagate_modes.h through
tools/propagate_modes_plan.cpp - once more under the address and undefined-behaviour sanitizers -, every ``ValueError`` of
``PlanePropagator.overlap`` and of ``SourceSweep.run(image_modes=...)`` before any device call, the entries' presence in header
and binding, the axis factors of ``metalens_amd.modes`` and the NumPy twin ``postprocess.mode_overlaps``."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import propagate_modes_ref as mref
from metalens_amd.propagate import MODES_MAX          # (without the entries every test of this file fails here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('modes_plan')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'propagate_modes_plan',
                           out + 'propagate_modes_plan_san'])

    def run(*args, exe='propagate_modes_plan'):
        res = subprocess.run([out + exe] + [a if isinstance(a, str) else repr(a) for a in args], capture_output=True, text=True,
                             timeout=120)
        assert res.returncode == 0 and res.stderr == '', res.stdout + res.stderr
        return res.stdout
    return run


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to reach a device fails the test"""
    from metalens_amd import _lib

    def refuse(*a, **k):
        raise AssertionError('a device call was made before the arguments were checked')
    monkeypatch.setattr(_lib, 'default_context', refuse)
    monkeypatch.setattr(_lib, 'Context', refuse)


# ---- the yardstick --------------------------------------------------------------------------
def test_yardstick_on_a_plane_worked_by_hand():
    # 3 x 4 Gaussian integers; modes of small Gaussian integers: every triple product and every sum is exact
    F = np.array([[1 + 2j, 0, 0, 2], [0, 3 - 1j, 0, 0], [-1j, 0, 0, 2j]])
    A = np.array([[1, 1j, 0], [0, 0, 2], [1, 1, 1], [0, 0, 0]])
    B = np.array([[1, 1, 1, 1], [0, -1j, 0, 1], [0, 0, 0, 1j]])
    O, mag = mref.overlaps(F, A, B)
    # by hand.  conj(A[0]) = (1, -i, 0): rows 0 and 1.  With conj(B[0]) = 1: row sums 3 + 2i and 3 - i -> 3 + 2i - i (3 - i) = 2 - i
    assert O[0, 0] == 2 - 1j
    # conj(B[1]) = (0, i, 0, 1): row 0 -> 2, row 1 -> i (3 - i) = 1 + 3i; 2 - i (1 + 3i) = 5 - i
    assert O[0, 1] == 5 - 1j
    # A[1] = 2 delta_2, B[2] = i delta_3: 2 conj(i) F[2][3] = 2 (-i) (2i) = 4
    assert O[1, 2] == 4
    # the constant 1 on both axes: the sum of F
    assert O[2, 0] == F.sum() == 6 + 2j
    assert not O[3].any() and not mag[3].any()          # the zero mode
    assert np.array_equal(O, np.einsum('ai,bj,ij->ab', A.conj(), B.conj(), F))
    # mag: (|a.r| + |a.i|) (|b.r| + |b.i|) (|f.r| + |f.i|) summed - for A[0], B[0]: rows 0 and 1 count once each, 5 + 4
    assert mag[0, 0] == 9 and mag[1, 2] == 2 * 2 and mag[2, 0] == 3 + 2 + 4 + 1 + 2
    # worst_ratio: an entry an ulp off is inside the bound, one off by the bound's double is not
    got = O.copy()
    got[0, 0] += 4 * mref.U
    assert mref.worst_ratio(got, F, A, B) == (pytest.approx(4 / ((3 + 4 + 16) * 9)), True)
    got[0, 0] = O[0, 0] + 2j * (3 + 4 + 16) * mref.U * 9
    assert mref.worst_ratio(got, F, A, B)[1] is False
    assert mref.bound_factor(70, 61) == 70 + 61 + 16 and mref.U == 2.0 ** -53 and mref.MODES_MAX == MODES_MAX
    # rounded products: the yardstick's entry is within its own 3 u mag of the exact one (fractions)
    from fractions import Fraction
    rng = np.random.default_rng(3)
    F, A, B = (rng.normal(size=s) + 1j * rng.normal(size=s) for s in ((3, 4), (1, 3), (1, 4)))
    O, mag = mref.overlaps(F, A, B)
    frac = lambda z: (Fraction(float(z.real)), Fraction(float(z.imag)))
    re = im = Fraction(0)
    for i in range(3):
        for j in range(4):
            (ar, ai), (br, bi), (fr, fi) = frac(A[0, i].conjugate()), frac(B[0, j].conjugate()), frac(F[i, j])
            pr, pi = ar * br - ai * bi, ar * bi + ai * br
            re += pr * fr - pi * fi
            im += pr * fi + pi * fr
    assert abs(Fraction(float(O[0, 0].real)) - re) <= 3 * Fraction(mref.U) * Fraction(float(mag[0, 0]))
    assert abs(Fraction(float(O[0, 0].imag)) - im) <= 3 * Fraction(mref.U) * Fraction(float(mag[0, 0]))


# ---- the checks and the caps ----------------------------------------------------------------
def _plan_args(T=357, mx=21, my=17, planes=1, null=0, nu=3, nv=64, n_slots=4, entry=None):
    return ('check_plan', T, mx, my, planes, null, nu, nv, n_slots) + (() if entry is None else tuple(entry))


PLAN_REFUSALS = [
    (dict(planes=2), '2 planes of 21 x 17 targets are 714 targets, the active propagation plan has 357'),
    (dict(mx=17, my=20), '1 planes of 17 x 20 targets are 340 targets'),
    (dict(mx=0), '1 planes of 0 x 17 targets'),
    (dict(T=0), 'are 357 targets, the active propagation plan has 0'),
    (dict(T=65536, mx=1, my=1, planes=65536, nu=1, nv=1), '65536 planes, at most 65535 are taken per plan'),
    (dict(nu=0), '0 x 64 modes: 1 to 64 are taken per axis'),
    (dict(nu=65), '65 x 64 modes: 1 to 64'),
    (dict(nv=65), '3 x 65 modes'),
    (dict(nv=-1), '3 x -1 modes'),
    (dict(null=1), 'NULL argument (mode_x NULL, mode_y given)'),
    (dict(null=2), 'NULL argument (mode_x given, mode_y NULL)'),
    (dict(null=3), 'NULL argument (mode_x NULL, mode_y NULL)'),
    (dict(n_slots=0), '0 output slots: 1 to 4096 are reserved per plan'),
    (dict(n_slots=4097), '4097 output slots: 1 to 4096'),
    (dict(entry=(0, 2, 20, 0, 'nan')), 'mode_x[2][20] = (nan, -0.5): a table entry is finite'),
    (dict(entry=(0, 0, 0, 1, 'inf')), 'mode_x[0][0] = (1, inf)'),
    (dict(entry=(1, 63, 16, 1, '-inf')), 'mode_y[63][16] = (1, -inf)'),
    (dict(entry=(1, 5, 3, 0, 'nan')), 'mode_y[5][3] = (nan, -0.5)'),
    # the caps: 2^24 table entries, 2^25 row sums per component, 2^24 output entries
    (dict(T=300000, mx=1, my=300000, nu=1, nv=56, n_slots=1), '1 x 1 + 300000 x 56 = 16800001 table entries, at most 2^24 = 16777216'),
    (dict(T=2 ** 21, mx=2 ** 20, my=1, planes=2, nu=1, nv=17, n_slots=1),
     '2 planes x 1048576 rows x 17 modes = 35651584 row sums per component, at most 2^25 = 33554432'),
    (dict(nu=64, n_slots=1025), '1025 slots x 1 planes x 4 x 64 x 64 modes = 16793600 output entries, at most 2^24 = 16777216'),
    (dict(T=429, mx=13, my=11, planes=3, nu=64, n_slots=342), '342 slots x 3 planes x 4 x 64 x 64 modes = 16809984 output entries'),
]
PLAN_ACCEPTED = [dict(), dict(nu=1, nv=1, n_slots=1), dict(nu=64, n_slots=1024), dict(T=429, mx=13, my=11, planes=3, nu=64, n_slots=341),
                 dict(T=65535, mx=1, my=1, planes=65535, nu=1, nv=1, n_slots=64), dict(n_slots=4096, nu=1, nv=1),
                 dict(T=262143, mx=1, my=262143, nu=1, nv=64, n_slots=1),                                   # 2^24 - 63 table entries
                 dict(T=2 ** 21, mx=2 ** 20, my=1, planes=2, nu=1, nv=16, n_slots=1),                       # 2^25 row sums
                 dict(entry=(0, 2, 20, 0, '1e308'))]
QUEUE_CASES = [   # have_result planned sets n_slots source slot -> code, wording
    ((0, 1, 0, 4, 0, 0), -2, 'ml_propagate has not run on the active propagation plan'),
    ((0, 0, 0, 0, 0, 0), -2, 'ml_propagate has not run on the active propagation plan'),
    ((1, 0, 1, 0, 0, 0), -2, 'ml_propagate_modes_plan has not run on the active propagation plan'),
    ((1, 1, 1, 4, -1, 0), -1, 'source -1: a member of the last pass (>= 0); the sums of ml_propagate_accumulate carry no phase'),
    ((1, 1, 2, 4, 2, 0), -1, 'ml_propagate_modes_queue: member 2 asked for, the last pass propagated 2 field sets'),
    ((1, 1, 3, 4, 2, 4), -1, 'slot 4, the plan reserved the slots 0 ... 3'),
    ((1, 1, 3, 4, 2, -1), -1, 'slot -1'),
    ((1, 1, 3, 4, 2, 3), 0, ''), ((1, 1, 1, 1, 0, 0), 0, ''),
]
FETCH_CASES = [   # planned n_slots first_slot n null
    ((0, 0, 0, 1, 0), -2, 'ml_propagate_modes_plan has not run on the active propagation plan'),
    ((1, 4, 3, 2, 0), -1, 'slots 3 ... 4 asked for, the plan reserved the slots 0 ... 3'),
    ((1, 4, -1, 2, 0), -1, 'slots -1 ... 0 asked for'),
    ((1, 4, 0, 0, 0), -1, 'slots 0 ... -1 asked for'),
    ((1, 4, 2147483647, 2147483647, 0), -1, 'slots 2147483647 ... 4294967293 asked for'),
    ((1, 4, 0, 4, 1), -1, 'NULL argument (out NULL)'),
    ((1, 4, 0, 4, 0), 0, ''), ((1, 4, 3, 1, 0), 0, ''),
]


def _expect(out, code, said):
    if code == 0:
        assert out == 'ok=1\n', out
    else:
        assert out.startswith('refused=%d\n' % code) and said in out, out


def test_refusals_name_the_numbers(tool):
    for more, said in PLAN_REFUSALS:
        _expect(tool(*_plan_args(**more)), -1, said)
    for more in PLAN_ACCEPTED:
        assert tool(*_plan_args(**more)) == 'ok=1\n', more
    for args, code, said in QUEUE_CASES:
        _expect(tool('check_queue', *args), code, said)
    for args, code, said in FETCH_CASES:
        _expect(tool('check_fetch', *args), code, said)
    assert tool('plan', 4096, 4096, 1, 64, 64, 1) == 'table=524288 rows=262144 out=16384 segments_x=128 segments_y=128 segment=32 modes_max=64\n'
    assert tool('plan', 13, 11, 3, 1, 7, 5) == 'table=90 rows=273 out=420 segments_x=1 segments_y=1 segment=32 modes_max=64\n'
    assert (mref.MODES_MAX, mref.SEGMENT) == (64, 32)


# mx, my, nv: the shapes of tests/test_gpu_propagate_modes.py; my = 17, 61, 512, 513, 1056 and nv on either side of the two row
# kernels (8, 9); a tile of 128 and one more; rows and columns either side of a column tile of 1024; live rows 1 and 2
LAUNCH_SHAPES = [(21, 17, 1), (21, 17, 8), (21, 17, 9), (21, 17, 64), (70, 61, 8), (70, 61, 9), (70, 61, 64), (13, 11, 64), (13, 11, 7),
                 (3, 512, 8), (3, 512, 9), (3, 513, 8), (3, 513, 9), (3, 1056, 1), (3, 1056, 8), (3, 1056, 9), (3, 1056, 64),
                 (5, 128, 9), (6, 129, 64), (1024, 1, 1), (1025, 1, 9), (1100, 3, 64), (2048, 32, 16), (4096, 4096, 1), (4096, 4096, 64),
                 (1, 1, 1), (1, 1, 64)]


def _shape(tool, mx, my, nv, exe='propagate_modes_plan'):
    return {k: int(v) for k, v in (kv.split('=') for kv in tool('shape', mx, my, nv, exe=exe).split())}


def test_launch_shapes(tool):
    """modes_rows_shape and modes_columns_shape - what the kernels and launchers of propagate_modes.hip call - against the
    Python restatement, and the cover they promise: whole tiles and a last one, whole segments and a last one"""
    for mx, my, nv in LAUNCH_SHAPES:
        got = _shape(tool, mx, my, nv)
        assert got == mref.plan(mx, my, nv), (mx, my, nv)
        assert (got['rows'], got['tile']) == ((1, 512) if nv <= 8 else (2, 128)) and got['col_tile'] == 1024
        assert got['tile'] % mref.SEGMENT == 0          # a tile cuts no segment
        for n, tile, tiles, segs, seg in ((my, got['tile'], got['tiles'], got['last_segments'], got['last_segment']),
                                          (mx, 1024, got['col_tiles'], got['col_last_segments'], got['col_last_segment'])):
            assert 1 <= seg <= mref.SEGMENT and 1 <= segs <= tile // mref.SEGMENT
            assert (tiles - 1) * tile + (segs - 1) * mref.SEGMENT + seg == n
        assert 1 <= got['last_rows'] <= got['rows'] and (got['groups'] - 1) * got['rows'] + got['last_rows'] == mx
    s = mref.plan(3, 1056, 8)
    assert (s['tiles'], s['last_segments'], s['last_segment'], s['groups'], s['last_rows']) == (3, 1, 32, 3, 1)
    s = mref.plan(3, 1056, 9)
    assert (s['tiles'], s['last_segments'], s['last_segment'], s['groups'], s['last_rows']) == (9, 1, 32, 2, 1)
    s = mref.plan(3, 513, 8)
    assert (s['tiles'], s['last_segments'], s['last_segment']) == (2, 1, 1)
    s = mref.plan(70, 61, 64)
    assert (s['tiles'], s['last_segments'], s['last_segment'], s['groups'], s['last_rows']) == (1, 2, 29, 35, 2)
    s = mref.plan(1100, 3, 64)
    assert (s['col_tiles'], s['col_last_segments'], s['col_last_segment'], s['groups'], s['last_rows']) == (2, 3, 12, 550, 2)


def test_under_sanitizers(tool):
    """the same program under the address and undefined-behaviour sanitizers: same output, nothing reported"""
    san = 'propagate_modes_plan_san'
    for mx, my, nv in LAUNCH_SHAPES:
        assert tool('shape', mx, my, nv, exe=san) == tool('shape', mx, my, nv)
    for more, said in PLAN_REFUSALS:
        assert tool(*_plan_args(**more), exe=san) == tool(*_plan_args(**more))
    for more in PLAN_ACCEPTED:
        assert tool(*_plan_args(**more), exe=san) == 'ok=1\n'
    for args, code, said in QUEUE_CASES:
        assert tool('check_queue', *args, exe=san) == tool('check_queue', *args)
    for args, code, said in FETCH_CASES:
        assert tool('check_fetch', *args, exe=san) == tool('check_fetch', *args)
    assert tool('plan', 70, 61, 1, 3, 64, 4, exe=san) == tool('plan', 70, 61, 1, 3, 64, 4)


# ---- the Python argument checks -------------------------------------------------------------
PITCH = 1.3e-7


def _propagator(**more):
    """what ``_check_overlap`` reads of a PlanePropagator, without a context"""
    x = 3e-6 + np.arange(21) * PITCH
    y = -2e-6 + np.arange(17) * PITCH
    p = dict(x=x, y=y, z=np.array([2e-5]), point_list=False, method='direct', want_h=True)
    p.update(more)
    return types.SimpleNamespace(**p)


def test_overlap_argument_errors_come_before_any_device_call(no_device):
    from metalens_amd import propagate
    from metalens_amd.propagate import PlanePropagator
    overlap = lambda p, *a, **k: PlanePropagator.overlap(p, *a, **k)
    A, B = np.ones((3, 21)), np.ones((2, 17)) * 1j
    with pytest.raises(ValueError, match='not a point list'):
        overlap(_propagator(point_list=True, y=_propagator().x), A, A)
    with pytest.raises(ValueError, match='at least 2 targets along y to know their pitch, the axis has 1'):
        overlap(_propagator(y=np.array([0.0])), A, np.ones((2, 1)))
    with pytest.raises(ValueError, match=r'uniform target axes: y\[1\]'):
        overlap(_propagator(y=np.array([0.0, 1e-7, 3e-7])), A, np.ones((2, 3)))
    with pytest.raises(ValueError, match='ascending target axis: x runs from'):
        overlap(_propagator(x=_propagator().x[::-1].copy()), A, B)
    with pytest.raises(ValueError, match=r'mode_x must have shape \(modes, 21\) or \(21,\) .*, got \(3, 17\)'):
        overlap(_propagator(), np.ones((3, 17)), B)
    with pytest.raises(ValueError, match=r'mode_y must have shape \(modes, 17\) or \(17,\) .*, got \(21,\)'):
        overlap(_propagator(), A, np.ones(21))
    with pytest.raises(ValueError, match=r'mode_y must have shape .*, got \(1, 2, 17\)'):
        overlap(_propagator(), A, np.ones((1, 2, 17)))
    with pytest.raises(ValueError, match=r'mode_x must have shape .*, got \(0, 21\)'):
        overlap(_propagator(), np.ones((0, 21)), B)
    with pytest.raises(ValueError, match='mode_x must be an array of numbers'):
        overlap(_propagator(), [['a'] * 21], B)
    with pytest.raises(ValueError, match='at most 64 modes per axis: mode_y has 65'):
        overlap(_propagator(), A, np.ones((65, 17)))
    bad = B.copy()
    bad[1, 16] = complex(0.0, np.inf)
    with pytest.raises(ValueError, match=r'a mode must be finite: mode_y\[1\]\[16\] = '):
        overlap(_propagator(), A, bad)
    nan = A.astype(complex)
    nan[2, 0] = np.nan
    with pytest.raises(ValueError, match=r'a mode must be finite: mode_x\[2\]\[0\] = '):
        overlap(_propagator(), nan, B)
    for power in ('all', [1.0, 2.0], np.ones((1, 1))):
        with pytest.raises(ValueError, match=r'power must be None, a number or an array \(1,\)'):
            overlap(_propagator(), A, B, power=power)
    # what the checks hand on: contiguous complex tables, 1-D modes as one mode, the planes, the pitch
    p = _propagator(method='fft-stack', z=np.array([1e-5, 2e-5, 3e-5]))
    tx, ty, planes, dx, dy = propagate._check_overlap(p, A[0], B)
    assert tx.shape == (1, 21) and ty.shape == (2, 17) and tx.dtype == ty.dtype == np.complex128 and tx.flags.c_contiguous
    assert planes == 3 and dx == (p.x[-1] - p.x[0]) / 20 and dy == (p.y[-1] - p.y[0]) / 16
    assert propagate._check_overlap_power(None, 3) is None and propagate._check_overlap_power(2, 3).tolist() == [2.0] * 3
    assert propagate._check_overlap_power([1, 2, 3], 3).tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match=r'2000 sources x 3 planes x 4 x 64 x 64 modes are 98304000 overlaps, at most 2\^24'):
        propagate._check_overlap(p, np.ones((64, 21)), np.ones((64, 17)), n_slots=2000)
    assert propagate.MODES_MAX == mref.MODES_MAX


class _NoCalls:
    """stands in for a Context: touching its library or its handle fails the test"""
    def __getattr__(self, name):
        raise AssertionError('a device call was made before the arguments were checked')


def test_sweep_argument_errors_come_before_any_device_call(no_device):
    from metalens_amd.sweep import SourceSweep
    ctx = _NoCalls()
    sw = SourceSweep.__new__(SourceSweep)
    sw.__dict__.update(ctx=ctx, x=np.zeros(20), y=np.zeros(24))
    src = [(0.0, 0.0, -1e-4, 'x')]
    image = _propagator(ctx=ctx, aperture_shape=(20, 24), shape=(21, 17))
    A, B = np.ones((3, 21)), np.ones(17)
    with pytest.raises(ValueError, match='image_modes= needs image='):
        sw.run(src, image_modes=(A, B))
    with pytest.raises(ValueError, match=r'image_modes must be a pair \(mode_x, mode_y\)'):
        sw.run(src, image=image, image_modes=(A, B, B))
    with pytest.raises(ValueError, match=r'image_modes must be a pair \(mode_x, mode_y\)'):
        sw.run(src, image=image, image_modes=3.0)
    with pytest.raises(ValueError, match=r'mode_y must have shape \(modes, 17\)'):
        sw.run(src, image=image, image_modes=(A, A))
    with pytest.raises(ValueError, match='at most 64 modes per axis: mode_x has 70'):
        sw.run(src, image=image, image_modes=(np.ones((70, 21)), B))
    with pytest.raises(ValueError, match='a mode must be finite'):
        sw.run(src, image=image, image_modes=(A, B * np.nan))
    with pytest.raises(ValueError, match='not a point list'):
        sw.run(src, image=_propagator(ctx=ctx, aperture_shape=(20, 24), shape=(21,), point_list=True), image_modes=(A, B))
    with pytest.raises(ValueError, match=r'2000 sources x 1 planes x 4 x 64 x 64 modes are 32768000 overlaps'):
        sw.run(src * 2000, image=image, image_modes=(np.ones((64, 21)), np.ones((64, 17))))
    with pytest.raises(ValueError, match='context of this sweep'):      # the image's own checks come first, as before
        sw.run(src, image=_propagator(ctx=_NoCalls(), aperture_shape=(20, 24)), image_modes=(A, B))
    state = sw._check_image_modes(image, iter([A, B]), 5)          # (taken once: the pair may be a one-shot iterable)
    assert state['tx'].shape == (3, 21) and state['ty'].shape == (1, 17) and state['n_slots'] == 5 and not state['planned']
    assert sw._check_image_modes(image, None, 5) is None


def test_entries_in_header_and_binding():
    from metalens_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = _lib.load()
    for name, n_args in (('ml_propagate_modes_plan', 9), ('ml_propagate_modes_queue', 3), ('ml_propagate_modes_fetch', 4)):
        decl = re.search(r'int\s+%s\s*\(([^)]*)\)' % name, code)
        assert decl and len(decl.group(1).split(',')) == n_args and name in _lib.SYMBOLS, name
        assert len(getattr(lib, name).argtypes) == n_args
    assert re.search(r'#define\s+ML_MODES_MAX\s+64\b', code)
    m, out = np.zeros(2, dtype=np.complex128), np.zeros(8)
    assert lib.ml_propagate_modes_plan(None, 2, 2, 1, _lib.dptr(m), 1, _lib.dptr(m), 1, 1) != 0          # no context: refused
    assert lib.ml_propagate_modes_queue(None, 0, 0) != 0 and lib.ml_propagate_modes_fetch(None, 0, 1, _lib.dptr(out)) != 0


# ---- the axis factors -----------------------------------------------------------------------
def test_hermite_gauss_orders_are_orthonormal():
    import metalens_amd as ma
    w, wl = 2e-6, 580e-9
    t = np.arange(-6 * 16, 6 * 16 + 1) * (w / 16)          # +-6 w at pitch w / 16
    for z in (0.0, 15e-6):
        wz = w * np.sqrt(1 + (z / (np.pi * 1.46 * w * w / wl)) ** 2)
        M = np.array([ma.hermite_gauss_axis(n, t * wz / w, w, z=z, wavelength=wl, n=1.46) for n in range(7)])
        M /= np.sqrt((np.abs(M) ** 2).sum(axis=1))[:, None]
        assert np.abs(M.conj() @ M.T - np.eye(7)).max() <= 1e-9
    # order 0 is the Gaussian factor; order 1 is odd, with H_1(s) = 2 s
    g = ma.gaussian_axis(t, w, z=15e-6, centre=0.3e-6, wavelength=wl, n=1.46)
    assert np.allclose(ma.hermite_gauss_axis(0, t, w, z=15e-6, centre=0.3e-6, wavelength=wl, n=1.46), g, rtol=1e-14, atol=0)
    one = ma.hermite_gauss_axis(1, t, w, wavelength=wl)
    assert np.allclose(one, 2 * np.sqrt(2) * t / w * np.exp(-t * t / (w * w)), rtol=1e-13, atol=1e-300)
    for bad in (-1, 17, 2.5, 'two', None, [1]):
        with pytest.raises(ValueError, match=r'integer in \[0, 16\]'):
            ma.hermite_gauss_axis(bad, t, w, wavelength=wl)
    with pytest.raises(ValueError, match='waist w0 must be finite and > 0'):
        ma.gaussian_axis(t, 0.0, wavelength=wl)
    with pytest.raises(ValueError, match='wavelength and n must be finite and > 0'):
        ma.gaussian_axis(t, w, wavelength=-1.0)


def test_gaussian_axis_closed_forms():
    import metalens_amd as ma
    w, wl, n = 1.7e-6, 580e-9, 1.46
    t = np.linspace(-8e-6, 8e-6, 201)
    # at the waist: exp(-(t - c)^2 / w0^2)
    assert np.allclose(ma.gaussian_axis(t, w, wavelength=wl, n=n), np.exp(-t * t / (w * w)), rtol=1e-14, atol=1e-300)
    # a shifted centre equals a shifted axis
    c = 1.25e-6
    assert np.array_equal(ma.gaussian_axis(t, w, z=12e-6, centre=c, wavelength=wl, n=n), ma.gaussian_axis(t - c, w, z=12e-6, wavelength=wl, n=n))
    assert np.array_equal(ma.hermite_gauss_axis(3, t, w, z=12e-6, centre=c, wavelength=wl, n=n),
                          ma.hermite_gauss_axis(3, t - c, w, z=12e-6, wavelength=wl, n=n))
    # away from the waist: the modulus has the radius w(z), the phase the curvature R(z) = z (1 + (zR / z)^2)
    k = 2 * np.pi * n / wl
    zR, z = k * w * w / 2, 12e-6
    g = ma.gaussian_axis(t, w, z=z, wavelength=wl, n=n)
    wz, R = w * np.sqrt(1 + (z / zR) ** 2), z * (1 + (zR / z) ** 2)
    assert np.allclose(np.abs(g), np.exp(-t * t / (wz * wz)), rtol=1e-12, atol=1e-300)
    assert np.allclose(g, np.exp(-t * t / (wz * wz)) * np.exp(1j * k * t * t / (2 * R)), rtol=0, atol=1e-12)
    # a tilt is a linear phase in t
    tilt = 0.02
    assert np.allclose(ma.gaussian_axis(t, w, tilt=tilt, wavelength=wl, n=n), np.exp(-t * t / (w * w)) * np.exp(1j * k * np.sin(tilt) * t),
                       rtol=1e-14, atol=1e-300)


# ---- the NumPy twin -------------------------------------------------------------------------
def test_mode_overlaps_against_einsum():
    import metalens_amd as ma
    from metalens_amd.postprocess import mode_coupling, mode_norm
    rng = np.random.default_rng(5)
    x, y = 1e-6 + np.arange(9) * 2e-7, np.arange(7) * 3e-7
    dx, dy, Z = 2e-7, 3e-7, 250.0
    cn = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)
    A, B = cn(3, 9), cn(2, 7)
    f = {k: cn(2, 9, 7) for k in ('Ex', 'Ey', 'Ez', 'Hx', 'Hy', 'Hz')}
    out = ma.mode_overlaps(f, x, y, A, B, Z)
    assert set(out) == {'overlap_Ex', 'overlap_Ey', 'overlap_Hx', 'overlap_Hy', 'norm', 'power', 'coupling_x', 'coupling_y'}
    dA = ((x[-1] - x[0]) / 8) * ((y[-1] - y[0]) / 6)
    O = {k: np.einsum('ai,bj,pij->pab', A.conj(), B.conj(), f[k]) * dA for k in ('Ex', 'Ey', 'Hx', 'Hy')}
    for k, v in O.items():
        assert out['overlap_' + k].shape == (2, 3, 2) and np.allclose(out['overlap_' + k], v, rtol=1e-13, atol=0)
    norm = np.einsum('ai,ai->a', A.conj(), A).real[:, None] * np.einsum('bj,bj->b', B.conj(), B).real[None, :] * dA
    assert np.allclose(out['norm'], norm, rtol=1e-13, atol=0) and np.allclose(mode_norm(A, B, dx, dy), norm, rtol=1e-12, atol=0)
    P = (0.5 * np.real(f['Ex'] * f['Hy'].conj() - f['Ey'] * f['Hx'].conj())).sum(axis=(1, 2)) * dA
    assert np.allclose(out['power'], P, rtol=1e-13, atol=0)
    want_x = np.abs(O['Ex'] / Z + O['Hy']) ** 2 * Z / (8 * norm * P[:, None, None])
    want_y = np.abs(O['Ey'] / Z - O['Hx']) ** 2 * Z / (8 * norm * P[:, None, None])
    assert np.allclose(out['coupling_x'], want_x, rtol=1e-12, atol=0) and np.allclose(out['coupling_y'], want_y, rtol=1e-12, atol=0)
    # a given power, a number or per plane; 1-D modes and a single plane
    given = ma.mode_overlaps(f, x, y, A, B, Z, power=[2.0, 4.0])
    assert np.allclose(given['coupling_x'], want_x * (P / [2.0, 4.0])[:, None, None], rtol=1e-12, atol=0)
    one = ma.mode_overlaps({k: v[1] for k, v in f.items()}, x, y, A[2], B[0], Z, power=4.0)
    assert one['overlap_Hy'].shape == (1, 1, 1) and np.allclose(one['coupling_y'][0, 0, 0], given['coupling_y'][1, 2, 0], rtol=1e-12, atol=0)
    # without H: the Cauchy-Schwarz share of sum |E|^2 dA, at most 1; with a power |O|^2 / (2 Z norm power)
    e = {k: f[k] for k in ('Ex', 'Ey', 'Ez')}
    oe = ma.mode_overlaps(e, x, y, A, B, Z)
    I_dA = sum(np.abs(e[k]) ** 2 for k in e).sum(axis=(1, 2)) * dA
    assert set(oe) == {'overlap_Ex', 'overlap_Ey', 'norm', 'power', 'coupling_x', 'coupling_y'} and np.allclose(oe['power'], I_dA, rtol=1e-13, atol=0)
    assert np.allclose(oe['coupling_x'], np.abs(O['Ex']) ** 2 / (norm * I_dA[:, None, None]), rtol=1e-12, atol=0) and (oe['coupling_x'] <= 1).all()
    op = ma.mode_overlaps(e, x, y, A, B, Z, power=3.0)
    assert np.allclose(op['coupling_y'], np.abs(O['Ey']) ** 2 / (2 * Z * norm * 3.0), rtol=1e-12, atol=0)
    # the field that IS the mode couples fully: psi x^ with h = psi y^ / Z
    psi = A[1][:, None] * B[0][None, :]
    full = ma.mode_overlaps(dict(Ex=psi, Ey=0 * psi, Hx=0 * psi, Hy=psi / Z), x, y, A, B, Z)
    assert abs(full['coupling_x'][0, 1, 0] - 1) <= 1e-13 and not full['coupling_y'].any()
    # NaN where the norm or the reference is 0
    zero = mode_coupling({'Ex': O['Ex'], 'Ey': O['Ey']}, norm * np.array([[1.0, 0.0]]), Z, power=np.array([1.0, 0.0]))
    assert np.isfinite(zero[0][0, :, 0]).all() and np.isnan(zero[0][0, :, 1]).all() and np.isnan(zero[0][1]).all()
    with pytest.raises(ValueError, match='needs a power'):
        mode_coupling(O, norm, Z)
