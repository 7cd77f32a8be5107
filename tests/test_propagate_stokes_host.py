"""The Stokes records of a propagated image without a GPU: the NumPy twins (``postprocess.stokes_maps``, ``stokes_metrics``,
``analyser_power``) and the yardstick of tests/propagate_stokes_ref.py against a plane worked by hand, the record layout and
the argument checks of csrc/propagate_stokes.h through tools/propagate_stokes_plan.cpp - once more under the address and
undefined-behaviour sanitizers -, every ``ValueError`` of ``PlanePropagator.stokes`` and of ``SourceSweep.run(image_stokes=...)``
before any device call, and the three entries' presence in header and binding."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import propagate_focus_ref as fref
import propagate_stokes_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(21, 17, 5), (70, 61, 32), (13, 11, 0), (182, 181, 9), (1025, 1024, 1), (4096, 4096, 32), (1, 2, 3)]


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('stokes_plan')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'propagate_stokes_plan',
                           out + 'propagate_stokes_plan_san'])

    def run(*args, exe='propagate_stokes_plan'):
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


# ---- the twins ------------------------------------------------------------------------------
def test_maps_on_a_plane_worked_by_hand():
    import metalens_amd as ma
    Ex = np.array([[1 + 2j, 3 + 0j], [0j, 1 - 1j]])
    Ey = np.array([[2 - 1j, 0 + 1j], [2 + 0j, 1 + 1j]])
    Ez = np.array([[0j, 0.5j], [1 + 1j, 0j]])
    M = ma.stokes_maps(Ex, Ey, Ez)
    assert M.shape == (5, 2, 2)
    assert M[0].tolist() == [[10.0, 10.0], [4.0, 4.0]] and M[1].tolist() == [[0.0, 8.0], [-4.0, 0.0]]
    # 2 Re(Ex conj Ey): (1 + 2i)(2 + i) = 5i; 3 (-i); 0; (1 - i)(1 - i) = -2i.   2 Im(conj(Ex) Ey): (1 - 2i)(2 - i) = -5i; 3 i; 0; (1 + i)^2 = 2i
    assert M[2].tolist() == [[0.0, 0.0], [0.0, 0.0]] and M[3].tolist() == [[-10.0, 6.0], [0.0, 4.0]]
    assert M[4].tolist() == [[0.0, 0.25], [2.0, 0.0]]
    # the record's twin: unit pitch, radii about target (0, 1) - itself, then its two neighbours as well, then the plane
    x, y = np.array([0.0, 1.0]), np.array([0.0, 1.0])
    out = ma.stokes_metrics({'Ex': Ex, 'Ey': Ey, 'Ez': Ez}, x, y, [1.0, 0.0, 1.5], centre=(0.0, 1.0))
    assert out['S'].tolist() == [[28.0, 4.0, 0.0, 0.0]] and out['Iz_dA'].tolist() == [2.25]
    assert out['peak_I'].tolist() == [10.25] and out['peak_index'].tolist() == [[0, 1]] and out['centre_index'].tolist() == [[0.0, 1.0]]
    assert out['encircled_S'].tolist() == [[[24.0, 8.0, 0.0, 0.0], [10.0, 8.0, 0.0, 6.0], [28.0, 4.0, 0.0, 0.0]]]
    assert out['encircled_Iz'].tolist() == [[0.25, 0.25, 2.25]]
    assert out['longitudinal_share'].tolist() == [2.25 / 30.25] and out['dop'].tolist() == [4.0 / 28.0]
    assert out['orientation'].tolist() == [0.0] and out['ellipticity'].tolist() == [0.0]
    assert out['encircled_dop'][0, 1] == 1.0 and out['encircled_dop'].shape == (1, 3)          # one coherent pixel
    # from the maps, about the peak, with a stack's leading axis: the same numbers
    again = ma.stokes_metrics(np.stack([M, M], axis=1), x, y, [0.0])
    assert again['S'].tolist() == [[28.0, 4.0, 0.0, 0.0]] * 2 and again['encircled_S'].tolist() == [[[10.0, 8.0, 0.0, 6.0]]] * 2
    # the yardstick agrees with the twin on these exact numbers
    want = sref.record(M, None, 1.0, 1.0, [0.0, 1.0, 1.5], centre=(0.0, 1.0))
    assert want['sums'] == [28.0, 4.0, 0.0, 0.0, 2.25] and want['n_inside'] == [1, 3, 4] and want['peak_index'] == 1
    assert want['enc'][0] == [10.0, 8.0, 0.0, 6.0, 0.25] and want['enc'][1] == [24.0, 8.0, 0.0, 0.0, 0.25]
    assert want['sums_abs'] == [28.0, 12.0, 0.0, 20.0, 2.25]


def test_uniform_states_are_exact():
    import metalens_amd as ma
    rng = np.random.default_rng(5)
    Ex = rng.standard_normal((4, 3)) + 1j * rng.standard_normal((4, 3))
    zero = np.zeros_like(Ex)
    for Ey, state in ((1j * Ex, (0.0, 0.0, 1.0)), (Ex, (0.0, 1.0, 0.0)), (zero, (1.0, 0.0, 0.0)), (-1j * Ex, (0.0, 0.0, -1.0))):
        M = ma.stokes_maps(Ex, Ey, zero)
        assert (M[0] > 0).all()
        for q in range(3):
            assert np.array_equal(M[1 + q] / M[0], np.full(Ex.shape, state[q])), (state, q)


def test_analyser_power():
    import metalens_amd as ma
    Ex, Ey = 0.6 + 0.3j, -0.2 + 0.9j
    S = ma.stokes_maps(Ex, Ey, 0.0)[:4]
    r = np.sqrt(0.5)
    for jones in ((1, 0), (0, 1), (r, r), (r, -r), (r, 1j * r), (r, -1j * r), (3, 3j)):
        a = np.array(jones, dtype=complex)
        want = abs(np.vdot(a, [Ex, Ey])) ** 2 / np.vdot(a, a).real          # |a^dagger E|^2 of the normalised analyser
        assert abs(ma.analyser_power(S, jones) - want) <= 8 * sref.U * S[0], jones
    # an analyser and its orthogonal partner share S0; the circular state of S3 = +S0 passes (1, i) and not (1, -i)
    assert abs(ma.analyser_power(S, (1, 0)) + ma.analyser_power(S, (0, 1)) - S[0]) <= 4 * sref.U * S[0]
    circ = ma.stokes_maps(1.0, 1j, 0.0)[:4]
    assert circ.tolist() == [2.0, 0.0, 0.0, 2.0] and ma.analyser_power(circ, (1, 1j)) == 2.0 and ma.analyser_power(circ, (1, -1j)) == 0.0
    assert ma.analyser_power(np.ones((3, 2, 4)), (1, 0)).shape == (3, 2)
    for bad in ((0, 0), (1,), (np.nan, 1), 'xy'):
        with pytest.raises(ValueError, match='jones must be'):
            ma.analyser_power(S, bad)
    with pytest.raises(ValueError, match='four Stokes parameters'):
        ma.analyser_power(np.ones(3), (1, 0))


def test_degree_of_polarisation():
    import metalens_amd as ma
    x = y = np.array([0.0, 1.0])
    one = {'Ex': np.array([[1 + 1j, 0], [0, 0]]), 'Ey': np.array([[0.5j, 0], [0, 0]]), 'Ez': np.zeros((2, 2))}
    assert abs(ma.stokes_metrics(one, x, y)['dop'][0] - 1) <= 4 * sref.U
    two = {'Ex': np.array([[1.0, 0], [0, 0j]]), 'Ey': np.array([[0, 1j], [0, 0]]), 'Ez': np.zeros((2, 2))}
    out = ma.stokes_metrics(two, x, y, [0.0], centre=(0.0, 0.0))
    assert out['dop'][0] == 0.0 and out['encircled_dop'][0, 0] == 1.0
    two['Ey'][0, 1] = 0.5j
    assert 0 < ma.stokes_metrics(two, x, y)['dop'][0] < 1
    dark = {k: np.zeros((2, 2)) for k in ('Ex', 'Ey', 'Ez')}
    out = ma.stokes_metrics(dark, x, y, [1.0])
    assert np.isnan(out['dop']).all() and np.isnan(out['encircled_dop']).all() and np.isnan(out['longitudinal_share']).all()


# ---- the plan program -----------------------------------------------------------------------
def test_plan_and_layout(tool):
    lines = tool(*[v for s in SHAPES for v in s]).splitlines()
    assert len(lines) == len(SHAPES)
    for (mx, my, K), line in zip(SHAPES, lines):
        focus = fref.plan(mx, my, K)           # the cut is that of the focus metrics
        assert _facts(line) == dict(mx=mx, my=my, P=mx * my, chunk=focus['chunk'], chunks=focus['chunks'], last=focus['last'],
                                    record_doubles=9 + 5 * K, partial_doubles=sref.PARTIAL)
    for K in (0, 5, 32):
        assert _facts(tool('layout', K)) == dict(peak_i=sref.PEAK_I, peak_index=sref.PEAK_INDEX, sums=sref.SUMS, centre=sref.CENTRE,
                                                 enc=sref.ENC, components=5, record_doubles=sref.record_doubles(K) , radii_max=32)
    from metalens_amd import propagate
    assert (propagate._STOKES_SUMS, propagate._STOKES_CENTRE, propagate._STOKES_ENC) == (sref.SUMS, sref.CENTRE, sref.ENC) == (2, 7, 9)


REFUSALS = [   # have_result have_stokes T sets source mx my planes dx dy record_doubles centre radii... -> code, message
    ((0, 0, 357, 0, 0, 21, 17, 1, 1e-7, 1e-7, 9, 'none'), -2, 'ml_propagate has not run on the active propagation plan'),
    ((1, 0, 357, 1, -1, 21, 17, 1, 1e-7, 1e-7, 9, 'none'), -2, 'ml_propagate_accumulate_stokes has not run on the active propagation plan'),
    ((1, 1, 357, 2, 2, 21, 17, 1, 1e-7, 1e-7, 9, 'none'), -1, 'member 2 asked for, the last pass propagated 2 field sets'),
    ((1, 1, 357, 2, -2, 21, 17, 1, 1e-7, 1e-7, 9, 'none'), -1, 'source -2'),
    ((1, 1, 357, 1, 0, 21, 17, 2, 1e-7, 1e-7, 9, 'none'), -1, '2 planes of 21 x 17 targets are 714 targets, the active propagation plan has 357'),
    ((1, 1, 357, 1, 0, 17, 20, 1, 1e-7, 1e-7, 9, 'none'), -1, '1 planes of 17 x 20 targets are 340 targets'),
    ((1, 1, 357, 1, 0, 0, 17, 1, 1e-7, 1e-7, 9, 'none'), -1, '1 planes of 0 x 17 targets'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 0.0, 1e-7, 9, 'none'), -1, 'pitch must be finite and > 0, got dx = 0, dy = 1e-07'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 'nan', 9, 'none'), -1, 'pitch must be finite and > 0'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 9 + 165, '10,8') + tuple(range(33)), -1, '33 radii: 0 to 32 are taken'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 14, 'none', 1e-7), -1, '1 radii asked for, centre is NULL'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 24, '10,8', 1e-7, 3e-7, 2e-7), -1, 'radii[2] = 2e-07 < radii[1] = 3e-07'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 19, '10,8', 1e-7, 'inf'), -1, 'radii[1] = inf: a radius must be finite and >= 0'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 19, '10,8', -1e-7, 1e-7), -1, 'radii[0] = -1e-07'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 14, '10,8', 'nan'), -1, 'radii[0] = nan'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 14, 'nan,3.5', 1e-7), -1, 'the centre of plane 0 is (nan, 3.5)'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 9, '3.5,inf'), -1, 'the centre of plane 0 is (3.5, inf)'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 18, '10,8', 1e-7, 2e-7), -1, 'a record of 2 radii has 19 doubles, record_doubles = 18'),
    ((1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 8, 'none'), -1, 'a record of 0 radii has 9 doubles, record_doubles = 8'),
]
ACCEPTED = [   # repeated radii, a radius of 0, 32 radii, none with and without a centre, a fractional centre, the sums, a longer record
    (1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 24, '10,8', 0.0, 1e-7, 1e-7),
    (1, 1, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 9 + 160, '10,8') + tuple(range(32)),
    (1, 0, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 9, 'none'),
    (1, 0, 357, 1, 0, 21, 17, 1, 1e-7, 1e-7, 9, '3.25,-1.5'),
    (1, 1, 429, 3, -1, 13, 11, 3, 1e-7, 2e-7, 40, '3.25,1.5', 1e-7),
]


def test_refusals_name_the_numbers(tool):
    for args, code, said in REFUSALS:
        out = tool('check', *args)
        assert out.startswith('refused=%d\n' % code) and said in out and 'ml_propagate_focus' not in out, out
    for args in ACCEPTED:
        assert tool('check', *args) == 'ok=1\n'


def test_under_sanitizers(tool):
    """the same program under the address and undefined-behaviour sanitizers: same output, nothing reported"""
    shapes = [v for s in SHAPES for v in s]
    assert tool(*shapes, exe='propagate_stokes_plan_san') == tool(*shapes)
    assert tool('layout', 32, exe='propagate_stokes_plan_san') == tool('layout', 32)
    for args in [r[0] for r in REFUSALS] + ACCEPTED:
        assert tool('check', *args, exe='propagate_stokes_plan_san') == tool('check', *args)


# ---- the Python argument checks -------------------------------------------------------------
def _propagator(**more):
    """what the checks read of a PlanePropagator, without a context"""
    x = 3e-6 + np.arange(21) * 1.3e-7
    y = -2e-6 + np.arange(17) * 1.3e-7
    p = dict(x=x, y=y, z=np.array([2e-5]), point_list=False, method='direct', want_h=True)
    p.update(more)
    return types.SimpleNamespace(**p)


def test_stokes_argument_errors_come_before_any_device_call(no_device):
    from metalens_amd.propagate import PlanePropagator
    stokes = lambda p, *a, **k: PlanePropagator.stokes(p, *a, **k)
    with pytest.raises(ValueError, match=r'stokes\(\) takes a tensor grid of targets, not a point list'):
        stokes(_propagator(point_list=True, y=_propagator().x), [1e-7])
    with pytest.raises(ValueError, match=r'stokes\(\) needs at least 2 targets along y to know their pitch, the axis has 1'):
        stokes(_propagator(y=np.array([0.0])))
    with pytest.raises(ValueError, match='at least 2 targets along x'):
        stokes(_propagator(x=np.array([1e-6])))
    bent = _propagator().x.copy()
    bent[7] += 1e-6 * 1.3e-7
    with pytest.raises(ValueError, match=r'stokes\(\) needs uniform target axes: x\[7\]'):
        stokes(_propagator(x=bent))
    with pytest.raises(ValueError, match=r'stokes\(\) needs an ascending target axis: x runs from'):
        stokes(_propagator(x=_propagator().x[::-1].copy()))
    with pytest.raises(ValueError, match=r'stokes\(\) takes at most 32 radii, got 33'):
        stokes(_propagator(), np.arange(33) * 1e-7)
    for bad, said in (([1e-7, -1e-9], r'radii\[1\] = -1e-09'), ([np.nan], r'radii\[0\] = nan'), ([1e-7, 2e-7, np.inf], r'radii\[2\] = inf')):
        with pytest.raises(ValueError, match='a radius must be finite and >= 0: ' + said):
            stokes(_propagator(), bad)
    with pytest.raises(ValueError, match='radii must be a sequence of numbers'):
        stokes(_propagator(), [[1e-7, 2e-7]])
    for bad in ((1e-6,), (1e-6, 2e-6, 3e-6), np.zeros((2, 2)), 'centroid', None):
        with pytest.raises(ValueError, match="centre must be 'peak', one"):
            stokes(_propagator(), [1e-7], centre=bad)
    with pytest.raises(ValueError, match=r"an array \(3, 2\) - one centre per plane -, got shape \(2, 2\)"):
        stokes(_propagator(method='fft-stack', z=np.array([1e-5, 2e-5, 3e-5])), [1e-7], centre=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='a centre must be finite'):
        stokes(_propagator(), [1e-7], centre=(np.nan, 0.0))
    for bad in ('field', 'sum', None, 0):
        with pytest.raises(ValueError, match="of must be 'fields' or 'sums'"):
            stokes(_propagator(), [1e-7], of=bad)
    # focus() still names itself
    with pytest.raises(ValueError, match=r'focus\(\) takes at most 32 radii, got 33'):
        PlanePropagator.focus(_propagator(), np.arange(33) * 1e-7)


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
    image = _propagator(ctx=ctx, aperture_shape=(20, 24), shape=(21, 17), want_h=False)       # H is not needed
    with pytest.raises(ValueError, match='image_stokes= needs image='):
        sw.run(src, image_stokes=True)
    with pytest.raises(ValueError, match='image_stokes= needs image='):
        sw.run(src, image_stokes=[1e-7])
    with pytest.raises(ValueError, match='at most 32 radii, got 40'):
        sw.run(src, image=image, image_stokes=np.arange(40) * 1e-7)
    with pytest.raises(ValueError, match='a radius must be finite and >= 0'):
        sw.run(src, image=image, image_stokes=[-1e-7])
    with pytest.raises(ValueError, match="centre must be 'peak', one"):
        sw.run(src, image=image, image_stokes=True, image_centre=(0.0,))
    with pytest.raises(ValueError, match="centre must be 'peak', one"):
        sw.run(src, image=image, image_stokes=[1e-7], image_centre=(0.0,))
    with pytest.raises(ValueError, match='not a point list'):
        sw.run(src, image=_propagator(ctx=ctx, aperture_shape=(20, 24), shape=(21,), point_list=True), image_stokes=True)
    with pytest.raises(ValueError, match='context of this sweep'):      # the image's own checks come first, as before
        sw.run(src, image=_propagator(ctx=_NoCalls(), aperture_shape=(20, 24)), image_stokes=True)


def test_entries_in_header_and_binding():
    from metalens_amd import _lib
    import metalens_amd as ma
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = _lib.load()
    for name, n_args in (('ml_propagate_stokes', 12), ('ml_propagate_accumulate_stokes', 4), ('ml_propagate_stokes_sums', 2)):
        decl = re.search(r'int\s+%s\s*\(([^)]*)\)' % name, code)
        assert decl and len(decl.group(1).split(',')) == n_args and name in _lib.SYMBOLS, name
        assert len(getattr(lib, name).argtypes) == n_args
    rec, w = np.zeros(9), np.ones(1)
    assert lib.ml_propagate_stokes(None, 0, 2, 2, 1, 1.0, 1.0, None, None, 0, _lib.dptr(rec), 9) != 0    # no context: refused
    assert lib.ml_propagate_accumulate_stokes(None, _lib.dptr(w), 1, 1) != 0 and lib.ml_propagate_stokes_sums(None, _lib.dptr(rec)) != 0
    # the convention is stated where the issue asks for it
    said = 'counter-clockwise seen looking towards the'
    flat = lambda s: ' '.join(s.replace('*', ' ').replace('//', ' ').split())
    assert said in flat(text) and said in flat(open(os.path.join(ROOT, 'metalens_amd', 'csrc', 'propagate_stokes.h')).read())
    assert said in flat(ma.PlanePropagator.stokes.__doc__) and said in flat(ma.stokes_maps.__doc__)
    assert said in flat(open(os.path.join(ROOT, 'DESIGN.md')).read())
    assert all(hasattr(ma, name) for name in ('stokes_maps', 'stokes_metrics', 'analyser_power'))
