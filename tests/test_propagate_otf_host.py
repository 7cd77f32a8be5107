"""The transfer function of a propagated image without a GPU: the yardstick (tests/propagate_otf_ref.py) on a plane worked
by hand, the phase arithmetic, the argument checks and the caps of csrc/propagate_otf.h through tools/propagate_otf_plan.cpp
- once more under the address and undefined-behaviour sanitizers -, every ``ValueError`` of ``PlanePropagator.otf`` and of
``SourceSweep.run(image_freqs=...)`` before any device call, and the entry's presence in header and binding."""
import os
import re
import subprocess
import types
from fractions import Fraction

import numpy as np
import pytest

import propagate_otf_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# frequencies in cycles per sample: Nyquist, values with a full mantissa, a tiny one and a denormal
FRACTION_U = [0.5, -0.5, 1 / 3, -1 / 3, 0.1, 2.0 ** -30, 12345 * 5e-324, 0.3141592653589793, -0.4999999999999999,
              0.12345678901234568, -0.2718281828459045]
FRACTION_I = [0, 1, 2, 4095, 8191, 2 ** 25 - 1]


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('otf_plan')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'propagate_otf_plan',
                           out + 'propagate_otf_plan_san'])

    def run(*args, exe='propagate_otf_plan'):
        res = subprocess.run([out + exe] + [a if isinstance(a, str) else repr(a) for a in args], capture_output=True, text=True,
                             timeout=60)
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
    I = np.arange(1.0, 13.0).reshape(3, 4)           # rows 1 2 3 4 / 5 6 7 8 / 9 10 11 12: row sums 10 26 42, columns 15 18 21 24
    Sz = -0.5 * I
    f = [0.0, 0.25, 0.5]
    got = oref.otf(I, Sz, f, f)
    O, abs_re, abs_im = got['I']
    # every phasor is a power of -i: the sums are Gaussian integers
    want = np.array([[sum(I[i, j] * (-1j) ** (ka * i + kb * j) for i in range(3) for j in range(4)) for kb in (0, 1, 2)]
                     for ka in (0, 1, 2)])
    assert want[0, 0] == 78 and want[2, 0] == 10 - 26 + 42 and want[0, 2] == -6 and want[1, 0] == -32 - 26j and want[0, 1] == -6 + 6j
    # the quarter turns come off the exact fraction: the yardstick has these integers, not cos(fl(pi / 2)) = 6e-17 for 0
    assert np.array_equal(O, want)
    assert abs_re[0, 0] == 78 and abs_im[0, 0] == 0 and abs_re[1, 0] == 10 + 42 and abs_im[1, 0] == 26 and abs_im[2, 2] == 0
    assert np.array_equal(got['Sz'][0], -0.5 * O) and np.array_equal(got['Sz'][1], 0.5 * abs_re)
    c, s = oref.cos_sin([1 / 8, -1 / 8], [0.0], 8, 1)
    r = np.sqrt(0.5)
    assert np.allclose(c[0, 0, :, 0], [1, r, 0, -r, -1, -r, 0, r], rtol=0, atol=2e-16) and (c[0, 0, ::2, 0] == [1, 0, -1, 0]).all()
    assert np.allclose(s[1], -s[0], rtol=0, atol=2e-16) and np.allclose(c[1], c[0], rtol=0, atol=2e-16)
    assert (s[0, 0, ::2, 0] == [0, 1, 0, -1]).all() and (s[1, 0, ::2, 0] == [0, -1, 0, 1]).all()
    assert 'Sz' not in oref.otf(I, None, f, f)
    # a scale in place of |Sz|
    assert np.array_equal(oref.otf(I, Sz, f, f, scale=2 * I)['Sz'][1], 2 * abs_re)
    # the fraction of u i + v j is exact where the doubles' product is not: both integer paths
    u, v = [1 / 3, -0.4999999999999999], [0.1, 2.0 ** -30]
    fr = oref.fractions(u, v, 70, 61)
    for a, b, i, j in ((0, 0, 69, 60), (1, 1, 37, 59), (1, 0, 68, 1), (0, 1, 1, 60)):
        x = Fraction(u[a]) * i + Fraction(v[b]) * j
        d = Fraction(float(fr[a, b, i, j])) - x
        assert abs(d - round(d)) <= Fraction(1, 2 ** 54)
    wide = oref.fractions([1 / 3, 12345 * 5e-324], [0.1], 5, 4)          # a denormal: Python's integers
    assert np.array_equal(wide[0], oref.fractions([1 / 3], [0.1], 5, 4)[0])
    assert abs(wide[1, 0, 4, 3] - (0.1 * 3 + 12345 * 5e-324 * 4)) <= 2.0 ** -53


# ---- the phase arithmetic -------------------------------------------------------------------
def _fractions_of(tool, pairs, exe='propagate_otf_plan'):
    args = [a for u, i in pairs for a in (float(u).hex(), int(i))]
    lines = tool('fraction', *args, exe=exe).splitlines()
    assert len(lines) == len(pairs)
    out = []
    for line in lines:
        m = re.fullmatch(r'fraction=(\S+) naive=(\S+) quarters=(-?\d) rest=(\S+)', line)
        frac, q, rest = float.fromhex(m.group(1)), int(m.group(3)), float.fromhex(m.group(4))
        # the quarter turns come off exactly
        assert -2 <= q <= 2 and abs(rest) <= 0.125 and Fraction(rest) + Fraction(q, 4) == Fraction(frac), line
        out.append((frac, float.fromhex(m.group(2))))
    return out


def _off(got, u, i):
    """how far ``got`` lies from the exact fraction of u i, modulo 1"""
    d = Fraction(got) - Fraction(float(u)) * int(i)
    return abs(d - round(d))


def test_phase_fraction_is_exact_to_2_54(tool):
    pairs = [(u, i) for u in FRACTION_U for i in FRACTION_I]
    rng = np.random.default_rng(11)
    pairs += list(zip(rng.uniform(-0.5, 0.5, 400), rng.integers(0, 2 ** 25, 400)))
    got = _fractions_of(tool, pairs)
    worst = {i: Fraction(0) for i in FRACTION_I}
    for (u, i), (frac, naive) in zip(pairs, got):
        assert abs(frac) <= 0.5 and _off(frac, u, i) <= Fraction(1, 2 ** 54), (u, i, frac)
        # the plain product carries its own rounding, half an ulp of u i, into the fraction
        assert _off(naive, u, i) <= Fraction(1, 2 ** 53) * abs(Fraction(float(u)) * int(i)) + Fraction(1, 2 ** 54), (u, i, naive)
        if i in worst:
            worst[i] = max(worst[i], _off(naive, u, i))
    # what the FMA buys: at i = 8191 the plain product is off by up to 2^-42 (half an ulp of 4095), 2^12 times the 2^-54 above
    assert worst[8191] > Fraction(1, 2 ** 46) and worst[2 ** 25 - 1] > Fraction(1, 2 ** 34)
    assert worst[0] == 0 and worst[1] == 0
    assert _fractions_of(tool, pairs[:80], exe='propagate_otf_plan_san') == got[:80]


# ---- the checks and the caps ----------------------------------------------------------------
def _check_args(have_result=1, have_sums=1, T=357, sets=1, source=0, mx=21, my=17, planes=1, null=0, nu=None, nv=None,
                u=(0.0, 0.25), v=(0.0, -0.5, 1 / 3)):
    return ('check', have_result, have_sums, T, sets, source, mx, my, planes, null, len(u) if nu is None else nu,
            len(v) if nv is None else nv, len(u), len(v)) + tuple(float(f).hex() for f in u) + tuple(float(f).hex() for f in v)


REFUSALS = [
    (dict(have_result=0, sets=0), -2, 'ml_propagate has not run on the active propagation plan'),
    (dict(have_sums=0, source=-1), -2, 'ml_propagate_accumulate has not run on the active propagation plan'),
    (dict(sets=2, source=2), -1, 'ml_propagate_otf: member 2 asked for, the last pass propagated 2 field sets'),
    (dict(source=-2), -1, 'source -2'),
    (dict(planes=2), -1, '2 planes of 21 x 17 targets are 714 targets, the active propagation plan has 357'),
    (dict(mx=17, my=20), -1, '1 planes of 17 x 20 targets are 340 targets'),
    (dict(mx=0, my=17), -1, '1 planes of 0 x 17 targets'),
    (dict(T=65536, mx=1, my=1, planes=65536), -1, '65536 planes, at most 65535 are taken per call'),
    (dict(nu=0), -1, '0 x 3 frequencies: 1 to 64 are taken per axis'),
    (dict(u=(0.0,) * 65), -1, '65 x 3 frequencies: 1 to 64'),
    (dict(v=(0.25,) * 65), -1, '2 x 65 frequencies'),
    (dict(null=1), -1, 'NULL argument (u NULL, v given, otf given)'),
    (dict(null=2), -1, 'NULL argument (u given, v NULL, otf given)'),
    (dict(null=4), -1, 'NULL argument (u given, v given, otf NULL)'),
    (dict(u=(0.0, 0.5000000000000001)), -1, 'u[1] = 0.50000000000000011: a frequency is finite and within +-0.5'),
    (dict(v=(0.0, 0.1, -0.75)), -1, 'v[2] = -0.75'),
    (dict(u=(float('nan'),)), -1, 'u[0] = nan'),
    (dict(v=(float('inf'),)), -1, 'v[0] = inf'),
    # the caps: 2^24 phasors, 2^26 row sums per weight
    (dict(T=300000, mx=1, my=300000, u=(0.0,), v=(0.1,) * 56), -1, '1 x 1 + 300000 x 56 = 16800001 phasors, at most 2^24 = 16777216'),
    (dict(T=2 ** 21, mx=2 ** 20, my=1, planes=2, u=(0.0,), v=(0.1,) * 33), -1,
     '2 planes x 1048576 rows x 33 frequencies = 69206016 row sums per weight, at most 2^26 = 67108864'),
]
ACCEPTED = [dict(), dict(T=65535, mx=1, my=1, planes=65535), dict(u=(0.5, -0.5, 0.5), v=(0.0,)), dict(u=(0.1,) * 64, v=(-0.1,) * 64), dict(source=-1, T=429, mx=13, my=11, planes=3),
            dict(have_sums=0), dict(T=64 * 262080, mx=64, my=262080, u=(0.2,) * 64, v=(0.1,) * 64),              # 2^24 phasors
            dict(T=2 ** 21, mx=2 ** 20, my=1, planes=2, u=(0.0,), v=(0.1,) * 32)]                                   # 2^26 row sums


def test_refusals_name_the_numbers(tool):
    for more, code, said in REFUSALS:
        out = tool(*_check_args(**more))
        assert out.startswith('refused=%d\n' % code) and said in out, out
    for more in ACCEPTED:
        assert tool(*_check_args(**more)) == 'ok=1\n', more
    assert tool('plan', 4096, 4096, 1, 64, 64) == 'table=524288 rows=262144 segments_x=128 segments_y=128 segment=32 freq_max=64\n'
    assert tool('plan', 13, 11, 3, 1, 7) == 'table=90 rows=273 segments_x=1 segments_y=1 segment=32 freq_max=64\n'
    assert (oref.FREQ_MAX, oref.SEGMENT) == (64, 32)


# mx, my, nv: the shapes of tests/test_gpu_propagate_otf.py, rows and columns either side of a tile of 1024 (256 for four
# rows), the frequencies either side of the two row kernels, live rows 1 to 4 of the last workgroup
LAUNCH_SHAPES = [(21, 17, 1), (21, 17, 64), (70, 61, 8), (70, 61, 9), (13, 11, 64), (3, 1100, 7), (3, 1100, 8), (3, 1100, 33),
                 (3, 1100, 64), (1100, 3, 1), (1100, 3, 64), (5, 300, 64), (6, 256, 9), (7, 257, 9), (8, 1024, 8), (8, 1025, 8),
                 (1024, 1, 1), (1025, 1, 1), (2048, 32, 16), (4096, 4096, 64), (1, 1, 1)]


def _shape(tool, mx, my, nv, exe='propagate_otf_plan'):
    return {k: int(v) for k, v in (kv.split('=') for kv in tool('shape', mx, my, nv, exe=exe).split())}


def test_launch_shapes(tool):
    """otf_rows_shape and otf_columns_shape - what the kernels and launchers of propagate_otf.hip call - against the Python
    restatement, and the cover they promise: whole tiles and a last one, whole segments and a last one"""
    for mx, my, nv in LAUNCH_SHAPES:
        got = _shape(tool, mx, my, nv)
        assert got == oref.plan(mx, my, nv), (mx, my, nv)
        assert got['rows'] == (1 if nv <= 8 else 4) and got['rows'] * got['tile'] == got['col_tile'] == 1024
        assert got['batch'] == 16 * (1 if got['rows'] == 1 else 2) and oref.FREQ_MAX % got['batch'] == 0
        assert got['tile'] % oref.SEGMENT == 0          # a tile cuts no segment
        for n, tile, tiles, segs, seg in ((my, got['tile'], got['tiles'], got['last_segments'], got['last_segment']),
                                          (mx, 1024, got['col_tiles'], got['col_last_segments'], got['col_last_segment'])):
            assert 1 <= seg <= oref.SEGMENT and 1 <= segs <= tile // oref.SEGMENT
            assert (tiles - 1) * tile + (segs - 1) * oref.SEGMENT + seg == n
        assert 1 <= got['last_rows'] <= got['rows'] and (got['groups'] - 1) * got['rows'] + got['last_rows'] == mx
    s = oref.plan(3, 1100, 7)
    assert (s['tiles'], s['last_segments'], s['last_segment'], s['groups'], s['last_rows']) == (2, 3, 12, 3, 1)
    s = oref.plan(3, 1100, 64)
    assert (s['tile'], s['tiles'], s['last_segments'], s['last_segment'], s['groups'], s['last_rows']) == (256, 5, 3, 12, 1, 3)
    s = oref.plan(1100, 3, 64)
    assert (s['col_tiles'], s['col_last_segments'], s['col_last_segment'], s['groups'], s['last_rows']) == (2, 3, 12, 275, 4)
    assert {oref.plan(mx, 17, 9)['last_rows'] for mx in (13, 21, 70, 3)} == {1, 2, 3}          # 13 and 21 leave one row, 70 two


def test_under_sanitizers(tool):
    """the same program under the address and undefined-behaviour sanitizers: same output, nothing reported"""
    for mx, my, nv in LAUNCH_SHAPES:
        assert tool('shape', mx, my, nv, exe='propagate_otf_plan_san') == tool('shape', mx, my, nv)
    for more, code, said in REFUSALS:
        assert tool(*_check_args(**more), exe='propagate_otf_plan_san') == tool(*_check_args(**more))
    for more in ACCEPTED:
        assert tool(*_check_args(**more), exe='propagate_otf_plan_san') == 'ok=1\n'
    assert tool('plan', 70, 61, 1, 3, 64, exe='propagate_otf_plan_san') == tool('plan', 70, 61, 1, 3, 64)


# ---- the Python argument checks -------------------------------------------------------------
PITCH = 1.3e-7


def _propagator(**more):
    """what ``_check_otf`` reads of a PlanePropagator, without a context"""
    x = 3e-6 + np.arange(21) * PITCH
    y = -2e-6 + np.arange(17) * PITCH
    p = dict(x=x, y=y, z=np.array([2e-5]), point_list=False, method='direct', want_h=True)
    p.update(more)
    return types.SimpleNamespace(**p)


def test_otf_argument_errors_come_before_any_device_call(no_device):
    from metalens_amd import propagate
    from metalens_amd.propagate import PlanePropagator
    otf = lambda p, *a, **k: PlanePropagator.otf(p, *a, **k)
    nyq = 0.5 / PITCH
    ok = [0.0, 1e6]
    with pytest.raises(ValueError, match='not a point list'):
        otf(_propagator(point_list=True, y=_propagator().x), ok, ok)
    with pytest.raises(ValueError, match='at least 2 targets along y to know their pitch, the axis has 1'):
        otf(_propagator(y=np.array([0.0])), ok, ok)
    with pytest.raises(ValueError, match=r'uniform target axes: y\[1\]'):
        otf(_propagator(y=np.array([0.0, 1e-7, 3e-7])), ok, ok)
    with pytest.raises(ValueError, match='ascending target axis: x runs from'):
        otf(_propagator(x=_propagator().x[::-1].copy()), ok, ok)
    for bad in ('field', 'sum', None, 0):
        with pytest.raises(ValueError, match="of must be 'fields' or 'sums'"):
            otf(_propagator(), ok, ok, of=bad)
    with pytest.raises(ValueError, match=r'fx must be a sequence of at least one frequency, got an array of shape \(1, 2\)'):
        otf(_propagator(), [ok], ok)
    with pytest.raises(ValueError, match=r'fy must be a sequence of at least one frequency, got an array of shape \(0,\)'):
        otf(_propagator(), ok, [])
    with pytest.raises(ValueError, match=r'a frequency must be finite: fy\[1\] = nan'):
        otf(_propagator(), ok, [0.0, np.nan])
    with pytest.raises(ValueError, match=r'fx\[1\] = .* lies beyond the Nyquist frequency 1 / \(2 dx\) = 384615[0-9.]* of targets'):
        otf(_propagator(), [0.0, 1.001 * nyq], ok)
    with pytest.raises(ValueError, match=r'fy\[0\] = -.* lies beyond the Nyquist frequency 1 / \(2 dy\)'):
        otf(_propagator(), ok, [-1.001 * nyq])
    with pytest.raises(ValueError, match='at most 64 frequencies per axis, 63 when 0 is not among them .*: fx has 64'):
        otf(_propagator(), np.linspace(1e5, 3e6, 64), ok)
    with pytest.raises(ValueError, match='at most 64 frequencies per axis, 63 when 0 is not among them .*: fy has 65'):
        otf(_propagator(), ok, np.linspace(0, 3e6, 65))
    for bad in ((1e-6,), (1e-6, 2e-6, 3e-6), np.zeros((2, 2)), 'centroid'):
        with pytest.raises(ValueError, match="centre must be 'peak', one"):
            otf(_propagator(), ok, ok, centre=bad)
    with pytest.raises(ValueError, match='a centre must be finite'):
        otf(_propagator(), ok, ok, centre=(np.nan, 0.0))
    # what the checks hand on: cycles per sample with 0 put in front where it is missing, the caller's entries, the planes
    p = _propagator(method='fft-stack', z=np.array([1e-5, 2e-5, 3e-5]))
    fx = np.array([nyq, -1e6, nyq])
    (u, iu, u0), (v, iv, v0), c, planes, dx, dy = propagate._check_otf(p, fx, [2e6, 0.0, -nyq], (p.x[4], p.y[2]), 'sums')
    assert u[0] == 0 and u0 == 0 and iu.tolist() == [1, 2, 3] and u[1] == 0.5 == u[3] and abs(u[2] + 1e6 * PITCH) < 1e-15
    assert v.tolist()[1:] == [0.0, -0.5] and v0 == 1 and iv.tolist() == [0, 1, 2]
    assert planes == 3 and c.tolist() == [[4.0, 2.0]] * 3 and dx == (p.x[-1] - p.x[0]) / 20 and dy == (p.y[-1] - p.y[0]) / 16
    assert propagate._check_otf(_propagator(), ok, ok, None, 'fields')[2] is None
    assert propagate._check_otf(_propagator(), ok, ok, 'peak', 'fields')[2] == 'peak'
    assert propagate._check_otf(_propagator(), np.linspace(0, 3e6, 64), np.linspace(1e5, 3e6, 63), None, 'fields')[1][0].size == 64
    assert propagate.OTF_FREQ_MAX == oref.FREQ_MAX


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
    ok = [0.0, 1e6]
    with pytest.raises(ValueError, match='image_freqs= needs image='):
        sw.run(src, image_freqs=(ok, ok))
    with pytest.raises(ValueError, match=r'image_freqs must be a pair \(fx, fy\)'):
        sw.run(src, image=image, image_freqs=(ok, ok, ok))
    with pytest.raises(ValueError, match=r'image_freqs must be a pair \(fx, fy\)'):
        sw.run(src, image=image, image_freqs=3.0)
    # a one-shot iterable is taken once: the checks hand back what run() uses at its end
    fx, fy = sw._check_image_otf(image, iter([ok, tuple(ok)]), 'peak')
    assert fx.tolist() == ok == fy.tolist() and sw._check_image_otf(image, None, 'peak') is None
    with pytest.raises(ValueError, match=r'fy\[1\] = .* lies beyond the Nyquist frequency'):
        sw.run(src, image=image, image_freqs=(ok, [0.0, 4e6]))
    with pytest.raises(ValueError, match='at most 64 frequencies per axis'):
        sw.run(src, image=image, image_freqs=(np.linspace(0, 1e6, 65), ok))
    with pytest.raises(ValueError, match="centre must be 'peak', one"):
        sw.run(src, image=image, image_freqs=(ok, ok), image_centre=(0.0,))
    with pytest.raises(ValueError, match='not a point list'):
        sw.run(src, image=_propagator(ctx=ctx, aperture_shape=(20, 24), shape=(21,), point_list=True), image_freqs=(ok, ok))
    with pytest.raises(ValueError, match='context of this sweep'):      # the image's own checks come first, as before
        sw.run(src, image=_propagator(ctx=_NoCalls(), aperture_shape=(20, 24)), image_freqs=(ok, ok))


def test_entry_in_header_and_binding():
    from metalens_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    decl = re.search(r'int\s+ml_propagate_otf\s*\(([^)]*)\)', code)
    assert decl and len(decl.group(1).split(',')) == 10 and 'ml_propagate_otf' in _lib.SYMBOLS
    assert re.search(r'#define\s+ML_OTF_FREQ_MAX\s+64\b', code) and re.search(r'#define\s+ML_PROBE_OTF_PHASOR\s+9\b', code)
    lib = _lib.load()
    assert len(lib.ml_propagate_otf.argtypes) == 10
    f, out = np.zeros(1), np.zeros(4)
    assert lib.ml_propagate_otf(None, 0, 2, 2, 1, _lib.dptr(f), 1, _lib.dptr(f), 1, _lib.dptr(out)) != 0    # no context: refused
