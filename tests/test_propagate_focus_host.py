"""The focus metrics of a propagated image without a GPU: the NumPy restatement (tests/propagate_focus_ref.py) against a
plane worked by hand, the plan arithmetic and the argument checks of csrc/propagate_focus.h through
tools/propagate_focus_plan.cpp - once more under the address and undefined-behaviour sanitizers -, every ``ValueError`` of
``PlanePropagator.focus`` and of ``SourceSweep.run(image_radii=...)`` before any device call, and the entry's presence in
header and binding."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import propagate_focus_ref as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the shapes of tests/test_gpu_propagate_focus.py, the README's stack, and planes around the points where the chunk doubles
SHAPES = [(21, 17, 5), (70, 61, 32), (13, 11, 0), (64, 64, 8), (1024, 1024, 8), (1025, 1024, 1), (4096, 4096, 32),
          (8192, 8192, 0), (1, 2, 3), (2, 1, 3), (1448, 1449, 2)]


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('focus_plan')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'propagate_focus_plan',
                           out + 'propagate_focus_plan_san'])

    def run(*args, exe='propagate_focus_plan'):
        res = subprocess.run([out + exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
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


def _facts(line):
    return {k: int(v) for k, v in (kv.split('=') for kv in line.split())}


# ---- the restatement ------------------------------------------------------------------------
def test_restatement_on_a_plane_worked_by_hand():
    I = np.arange(1.0, 13.0).reshape(3, 4)           # rows 1 2 3 4 / 5 6 7 8 / 9 10 11 12
    Sz = -0.5 * I
    r = fref.record(I, Sz, 1.0, 1.0, [0.0, 1.0, 1.5, 2.1], centre=(1.0, 1.0))
    assert (r['peak_I'], r['peak_index'], r['n']) == (12.0, 11, 12)
    # sum w = 78; sum w i = 26 + 2 x 42; sum w j = 18 + 2 x 21 + 3 x 24; sum w i^2 = 26 + 4 x 42;
    # sum w j^2 = 18 + 4 x 21 + 9 x 24; sum w i j = (6 + 14 + 24) + 2 (10 + 22 + 36)
    assert r['mom_I'] == [78.0, 110.0, 132.0, 194.0, 318.0, 180.0] == r['mom_I_abs']
    assert r['mom_Sz'] == [-39.0, -55.0, -66.0, -97.0, -159.0, -90.0] and r['mom_Sz_abs'] == [39.0, 55.0, 66.0, 97.0, 159.0, 90.0]
    # about target (1, 1) = 6: itself; its four neighbours 2, 5, 7, 10; the diagonals 1, 3, 9, 11; then (1, 3) = 8 at distance 2
    assert r['n_inside'] == [1, 5, 9, 10] and r['enc_I'] == [6.0, 30.0, 54.0, 62.0] and r['enc_Sz'] == [-3.0, -15.0, -27.0, -31.0]
    assert r['centre'] == (1.0, 1.0)
    # centre None: the peak, (2, 3); a pitch of 2 along y halves the reach along j; a fractional centre
    r = fref.record(I, None, 1.0, 2.0, [1.0, 2.0])
    assert r['centre'] == (2.0, 3.0) and r['enc_I'] == [12.0 + 8.0, 12.0 + 8.0 + 4.0 + 11.0] and 'mom_Sz' not in r
    r = fref.record(I, None, 1.0, 1.0, [0.5, 0.75], centre=(0.5, 0.5))
    assert r['n_inside'] == [0, 4] and r['enc_I'] == [0.0, 14.0]
    # of equals the lowest index
    flat = np.ones((3, 4))
    assert fref.record(flat, None, 1.0, 1.0, [])['peak_index'] == 0
    flat[1, 2] = flat[2, 0] = 2.0
    assert fref.record(flat, None, 1.0, 1.0, [])['peak_index'] == 6
    # the membership rule rounds its three operations separately: a target on the boundary in exact arithmetic
    m, r2 = fref.inside((4, 5), 0.1, 0.1, 0.0, 0.0, 0.5)
    assert r2[3, 4] == (0.1 * 3.0) * (0.1 * 3.0) + (0.1 * 4.0) * (0.1 * 4.0) and m[3, 4] == (r2[3, 4] <= 0.5 * 0.5)


def test_weights_follow_the_accumulation_kernel():
    rng = np.random.default_rng(3)
    d = {k: rng.standard_normal((4, 5)) + 1j * rng.standard_normal((4, 5)) for k in ('Ex', 'Ey', 'Ez', 'Hx', 'Hy', 'Hz')}
    I, Sz, scale = fref.weights(d, True)
    assert np.allclose(I, sum(np.abs(d[k]) ** 2 for k in ('Ex', 'Ey', 'Ez')), rtol=4e-15, atol=0)
    assert np.allclose(Sz, 0.5 * np.real(d['Ex'] * np.conj(d['Hy']) - d['Ey'] * np.conj(d['Hx'])), rtol=0, atol=4e-16 * scale.max())
    assert (np.abs(Sz) <= scale * (1 + 1e-15)).all()
    assert fref.weights(d, False)[1:] == (None, None)


# ---- the plan program -----------------------------------------------------------------------
def test_plan_of_the_shapes(tool):
    lines = tool(*[v for s in SHAPES for v in s]).splitlines()
    assert len(lines) == len(SHAPES)
    for (mx, my, K), line in zip(SHAPES, lines):
        want = fref.plan(mx, my, K)
        assert _facts(line) == want, (mx, my, K)
        # the cut covers the plane: full chunks and a last one of 1 ... chunk targets; whole steps of 512 per chunk
        assert want['chunks'] <= fref.CHUNKS_MAX and 1 <= want['last'] <= want['chunk'] and want['chunk'] % fref.STEP == 0
        assert (want['chunks'] - 1) * want['chunk'] + want['last'] == mx * my
    # of P alone: a plane and its transpose; the chunk doubles where 1024 chunks no longer hold the plane
    assert fref.chunk_targets(21 * 17) == fref.chunk_targets(1024 * 1024) == 1024 and fref.chunk_targets(1024 * 1024 + 1) == 2048
    assert fref.chunk_targets(1 << 26) == 65536 and fref.plan(70, 61, 0)['chunks'] == 5 and fref.plan(13, 11, 0)['chunks'] == 1
    assert fref.plan(30, 50, 4)['chunk'] == fref.plan(50, 30, 4)['chunk']


# mx, my: planes around the tiles of 32 partial records of the second launch - 1, 5, 32, 33, 64, 65, 513, 1024 chunks
FINISH_SHAPES = [(21, 17), (70, 61), (128, 256), (182, 181), (256, 256), (65, 1024), (1025, 1024), (4096, 4096), (8192, 8192), (1, 1)]


def test_finish_tiles_of_the_shapes(tool):
    """focus_finish_tiles and focus_finish_tile_chunks - what focus_finish_kernel calls - against the Python restatement"""
    lines = tool('finish', *[v for s in FINISH_SHAPES for v in s]).splitlines()
    assert len(lines) == len(FINISH_SHAPES)
    tiles = {}
    for (mx, my), line in zip(FINISH_SHAPES, lines):
        want = fref.finish(mx, my)
        assert _facts(line) == want, (mx, my)
        assert want['chunks'] == fref.plan(mx, my, 0)['chunks'] and want['finish_tile'] == fref.FINISH_TILE == 32
        # the tiles cover the chunks: full tiles of 32 records and a last one of 1 ... 32
        assert 1 <= want['last_tile'] <= fref.FINISH_TILE and (want['finish_tiles'] - 1) * fref.FINISH_TILE + want['last_tile'] == want['chunks']
        tiles[(mx, my)] = (want['chunks'], want['finish_tiles'], want['last_tile'])
    assert tiles[(128, 256)] == (32, 1, 32) and tiles[(182, 181)] == (33, 2, 1) and tiles[(256, 256)] == (64, 2, 32)
    assert tiles[(65, 1024)] == (65, 3, 1) and tiles[(21, 17)] == (1, 1, 1) and tiles[(4096, 4096)] == (1024, 32, 32)
    assert tiles[(1025, 1024)] == (513, 17, 1) and tiles[(70, 61)] == (5, 1, 5) and tiles[(8192, 8192)] == (1024, 32, 32)


def test_record_layout(tool):
    for K in (0, 5, 32):
        f = _facts(tool('layout', K))
        assert f == dict(peak_i=fref.PEAK_I, peak_index=fref.PEAK_INDEX, mom_i=fref.MOM_I, mom_sz=fref.MOM_SZ, centre=fref.CENTRE,
                         enc_i=fref.ENC, enc_sz=fref.ENC + K, record_doubles=fref.record_doubles(K), radii_max=fref.RADII_MAX)
    from metalens_amd import propagate
    assert (propagate._FOCUS_MOM_I, propagate._FOCUS_MOM_SZ, propagate._FOCUS_CENTRE, propagate._FOCUS_ENC,
            propagate.FOCUS_RADII_MAX) == (fref.MOM_I, fref.MOM_SZ, fref.CENTRE, fref.ENC, fref.RADII_MAX)


REFUSALS = [   # have_result have_sums T sets source mx my planes dx dy record_doubles centre radii... -> code, message
    ((0, 0, 357, 0, 0, 21, 17, 1, 1e-7, 1e-7, 16, 'peak'), -2, 'ml_propagate has not run on the active propagation plan'),
    ((1, 0, 357, 1, -1, 21, 17, 1, 1e-7, 1e-7, 16, 'peak'), -2, 'ml_propagate_accumulate has not run on the active propagation plan'),
    ((1, 1, 357, 2, 2, 21, 17, 1, 1e-7, 1e-7, 16, 'peak'), -1, 'member 2 asked for, the last pass propagated 2 field sets'),
    ((1, 1, 357, 2, -2, 21, 17, 1, 1e-7, 1e-7, 16, 'peak'), -1, 'source -2'),
    ((1, 1, 357, 1, 0, 21, 17, 2, 1e-7, 1e-7, 16, 'peak'), -1, '2 planes of 21 x 17 targets are 714 targets, the active propagation plan has 357'),
    ((1, 1, 357, 1, 0, 17, 20, 1, 1e-7, 1e-7, 16, 'peak'), -1, '1 planes of 17 x 20 targets are 340 targets'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 0.0, 1e-7, 16, 'peak'), -1, 'pitch must be finite and > 0, got dx = 0, dy = 1e-07'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 'nan', 16, 'peak'), -1, 'pitch must be finite and > 0'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 16 + 66, 'peak') + tuple(range(33)), -1, '33 radii: 0 to 32 are taken'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 22, 'peak', 1e-7, 3e-7, 2e-7), -1, 'radii[2] = 2e-07 < radii[1] = 3e-07'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 20, 'peak', 1e-7, 'inf'), -1, 'radii[1] = inf: a radius must be finite and >= 0'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 20, 'peak', -1e-7, 1e-7), -1, 'radii[0] = -1e-07'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 18, 'peak', 'nan'), -1, 'radii[0] = nan'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 18, 'nan,3.5', 1e-7), -1, 'the centre of plane 0 is (nan, 3.5)'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 19, 'peak', 1e-7, 2e-7), -1, 'a record of 2 radii has 20 doubles, record_doubles = 19'),
]


def test_refusals_name_the_numbers(tool):
    for args, code, said in REFUSALS:
        out = tool('check', *args)
        assert out.startswith('refused=%d\n' % code) and said in out, out
    # what is accepted: repeated radii, a radius of 0, 32 radii, none, a fractional centre, the sums, a longer record
    for args in ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 22, 'peak', 0.0, 1e-7, 1e-7),
                 (1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 16 + 64, 'peak') + tuple(range(32)),
                 (1, 0, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 16, '3.25,-1.5'),
                 (1, 1, 429, 3, -1, 13, 11, 3, 1e-7, 2e-7, 40, '3.25,1.5', 1e-7)):
        assert tool('check', *args) == 'ok=1\n'


def test_under_sanitizers(tool):
    """the same program under the address and undefined-behaviour sanitizers: same output, nothing reported"""
    shapes = [v for s in SHAPES for v in s]
    assert tool(*shapes, exe='propagate_focus_plan_san') == tool(*shapes)
    assert tool('layout', 32, exe='propagate_focus_plan_san') == tool('layout', 32)
    finish = [v for s in FINISH_SHAPES for v in s]
    assert tool('finish', *finish, exe='propagate_focus_plan_san') == tool('finish', *finish)
    for args, code, said in REFUSALS:
        assert tool('check', *args, exe='propagate_focus_plan_san') == tool('check', *args)


# ---- the Python argument checks -------------------------------------------------------------
def _propagator(**more):
    """what ``_check_focus`` reads of a PlanePropagator, without a context"""
    x = 3e-6 + np.arange(21) * 1.3e-7
    y = -2e-6 + np.arange(17) * 1.3e-7
    p = dict(x=x, y=y, z=np.array([2e-5]), point_list=False, method='direct', want_h=True)
    p.update(more)
    return types.SimpleNamespace(**p)


def test_focus_argument_errors_come_before_any_device_call(no_device):
    from metalens_amd import propagate
    from metalens_amd.propagate import PlanePropagator
    focus = lambda p, *a, **k: PlanePropagator.focus(p, *a, **k)
    with pytest.raises(ValueError, match='not a point list'):
        focus(_propagator(point_list=True, y=_propagator().x), [1e-7])
    with pytest.raises(ValueError, match='at least 2 targets along y to know their pitch, the axis has 1'):
        focus(_propagator(y=np.array([0.0])))
    with pytest.raises(ValueError, match='at least 2 targets along x'):
        focus(_propagator(x=np.array([1e-6])))
    bent = _propagator().x.copy()
    bent[7] += 1e-6 * 1.3e-7
    with pytest.raises(ValueError, match=r'uniform target axes: x\[7\]'):
        focus(_propagator(x=bent))
    with pytest.raises(ValueError, match=r'uniform target axes: y\[1\]'):
        focus(_propagator(y=np.array([0.0, 1e-7, 3e-7])))
    with pytest.raises(ValueError, match='ascending target axis: x runs from'):
        focus(_propagator(x=_propagator().x[::-1].copy()))
    with pytest.raises(ValueError, match='at most 32 radii, got 33'):
        focus(_propagator(), np.arange(33) * 1e-7)
    for bad, said in (([1e-7, -1e-9], r'radii\[1\] = -1e-09'), ([np.nan], r'radii\[0\] = nan'), ([1e-7, 2e-7, np.inf], r'radii\[2\] = inf')):
        with pytest.raises(ValueError, match='a radius must be finite and >= 0: ' + said):
            focus(_propagator(), bad)
    with pytest.raises(ValueError, match='radii must be a sequence of numbers'):
        focus(_propagator(), [[1e-7, 2e-7]])
    for bad in ((1e-6,), (1e-6, 2e-6, 3e-6), np.zeros((2, 2)), np.zeros((1, 3)), 'centroid', None):
        with pytest.raises(ValueError, match="centre must be 'peak', one"):
            focus(_propagator(), [1e-7], centre=bad)
    with pytest.raises(ValueError, match=r"an array \(3, 2\) - one centre per plane -, got shape \(2, 2\)"):
        focus(_propagator(method='fft-stack', z=np.array([1e-5, 2e-5, 3e-5])), [1e-7], centre=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='a centre must be finite'):
        focus(_propagator(), [1e-7], centre=(np.nan, 0.0))
    for bad in ('field', 'sum', None, 0):
        with pytest.raises(ValueError, match="of must be 'fields' or 'sums'"):
            focus(_propagator(), [1e-7], of=bad)
    # what the checks hand on: the radii ascending and the way back, the centres in index units - a centre on a target is
    # that target -, the planes and the pitches
    p = _propagator(method='fft-stack', z=np.array([1e-5, 2e-5, 3e-5]))
    r, back, c, planes, dx, dy = propagate._check_focus(p, [3e-7, 1e-7, 2e-7, 1e-7], (p.x[4], p.y[0] + 2.25 * 1.3e-7), 'sums')
    assert r.tolist() == [1e-7, 1e-7, 2e-7, 3e-7] and r[back].tolist() == [3e-7, 1e-7, 2e-7, 1e-7]
    assert planes == 3 and c.shape == (3, 2) and (c[:, 0] == 4.0).all() and np.allclose(c[:, 1], 2.25, rtol=1e-9, atol=0)
    assert dx == (p.x[-1] - p.x[0]) / 20 and dy == (p.y[-1] - p.y[0]) / 16
    assert propagate._check_focus(_propagator(), (), 'peak', 'fields')[2:4] == (None, 1)
    per_plane = np.array([[p.x[1], p.y[2]], [p.x[3], p.y[4]], [p.x[5], p.y[6]]])
    assert propagate._check_focus(p, [], per_plane, 'fields')[2].tolist() == [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]


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
    with pytest.raises(ValueError, match='image_radii= needs image='):
        sw.run(src, image_radii=[1e-7])
    with pytest.raises(ValueError, match='image_radii= needs an image with want_h=True'):
        sw.run(src, image=_propagator(ctx=ctx, aperture_shape=(20, 24), shape=(21, 17), want_h=False), image_radii=[1e-7])
    with pytest.raises(ValueError, match='at most 32 radii, got 40'):
        sw.run(src, image=image, image_radii=np.arange(40) * 1e-7)
    with pytest.raises(ValueError, match='a radius must be finite and >= 0'):
        sw.run(src, image=image, image_radii=[-1e-7])
    with pytest.raises(ValueError, match="centre must be 'peak', one"):
        sw.run(src, image=image, image_radii=[1e-7], image_centre=(0.0,))
    with pytest.raises(ValueError, match='not a point list'):
        sw.run(src, image=_propagator(ctx=ctx, aperture_shape=(20, 24), shape=(21,), point_list=True), image_radii=[1e-7])
    with pytest.raises(ValueError, match='context of this sweep'):      # the image's own checks come first, as before
        sw.run(src, image=_propagator(ctx=_NoCalls(), aperture_shape=(20, 24)), image_radii=[1e-7])


def test_entry_in_header_and_binding():
    from metalens_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    decl = re.search(r'int\s+ml_propagate_focus\s*\(([^)]*)\)', code)
    assert decl and len(decl.group(1).split(',')) == 12 and 'ml_propagate_focus' in _lib.SYMBOLS
    lib = _lib.load()
    assert len(lib.ml_propagate_focus.argtypes) == 12
    rec = np.zeros(16)
    assert lib.ml_propagate_focus(None, 0, 2, 2, 1, 1.0, 1.0, None, None, 0, _lib.dptr(rec), 16) != 0    # no context: refused
