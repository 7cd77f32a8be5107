"""The beam metrics of the far field without a GPU: the argument checks of csrc/farfield_beam.h through
tools/farfield_beam_plan.cpp - every refusal with its wording, once more under the address and undefined-behaviour
sanitizers -, the record's layout against the Python side, ``postprocess.beam_metrics`` against the yardstick
(tests/farfield_beam_ref.py) on seeded maps with NaN corners, every ``ValueError`` of ``FarfieldTransform.beam`` and of
``SourceSweep.run(beam_cones=...)`` before any device call, and the entries' presence in header and binding."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import farfield_beam_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [1, 37, 300, 1024, 1025, 2009, 2048, 77100, 262144, 1 << 20, (1 << 20) + 1, 1049600, 1 << 24, (1 << 31) - 1]


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('beam_plan')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'farfield_beam_plan',
                           out + 'farfield_beam_plan_san'])

    def run(*args, exe='farfield_beam_plan'):
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


# ---- the plan program -----------------------------------------------------------------------
def test_plan_of_the_counts(tool):
    lines = tool(*COUNTS).splitlines()
    assert len(lines) == len(COUNTS)
    for n, line in zip(COUNTS, lines):
        assert _facts(line) == ref.plan(n), n
    assert ref.plan((1 << 31) - 1)['chunks'] == 1024 and ref.plan((1 << 31) - 1)['chunk'] == 1 << 21
    assert ref.plan(1 << 24)['roundings'] == 63 + 6 + 3 + 31 + 31


def test_record_layout(tool):
    f = _facts(tool('layout'))
    assert f == dict(peak_p=ref.PEAK_P, peak_index=ref.PEAK_INDEX, finite=ref.FINITE, mom=ref.MOM, centre=ref.CENTRE, k=ref.K,
                     cone=ref.CONE, record=ref.RECORD, partial=ref.PARTIAL, partial_cone=ref.PARTIAL_CONE, cones_max=ref.CONES_MAX,
                     slots=ref.SLOTS)
    from metalens_amd import postprocess, sweep
    assert (postprocess._BEAM_PEAK_P, postprocess._BEAM_PEAK_INDEX, postprocess._BEAM_FINITE, postprocess._BEAM_MOM,
            postprocess._BEAM_CENTRE, postprocess._BEAM_K, postprocess._BEAM_CONE, postprocess.BEAM_RECORD,
            postprocess.BEAM_CONES_MAX) == (ref.PEAK_P, ref.PEAK_INDEX, ref.FINITE, ref.MOM, ref.CENTRE, ref.K, ref.CONE, ref.RECORD,
                                            ref.CONES_MAX)
    assert sweep.MAX_SLOTS == ref.SLOTS
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    assert re.search(r'#define\s+ML_BEAM_CONES_MAX\s+32\b', text) and re.search(r'#define\s+ML_BEAM_RECORD\s+\(12 \+ ML_BEAM_CONES_MAX\)', text)


# projected scattered n pair_list acc_n acc_pair_list source slot centre cones... -> code, message
REFUSALS = [
    ((0, 0, 0, 0, 0, 0, 0, 0, 'peak', 0.1), -2, 'nothing projected: call ml_farfield_transform and ml_farfield_project first'),
    ((1, 1, 400, 0, 0, 0, 0, 0, 'peak', 0.1), -2, 'the power map is reduce-scattered over the ranks: call ml_farfield_gather before summing it'),
    ((1, 0, 400, 0, 0, 0, -1, 0, 'peak', 0.1), -2, 'this context has no sums yet (ml_farfield_accumulate has not run)'),
    ((1, 0, 400, 0, 300, 0, -1, 0, 'peak', 0.1), -2, 'the sums were started on a plan of 300 directions (tensor grid), the active plan has 400 (tensor grid)'),
    ((1, 0, 400, 1, 400, 0, -1, 0, 'peak', 0.1), -2, 'a plan of 400 directions (tensor grid), the active plan has 400 (pair list)'),
    ((1, 0, 400, 0, 0, 0, 1, 0, 'peak', 0.1), -1, 'source 1: 0 for the current projection or -1 for P_sum'),
    ((1, 0, 400, 0, 0, 0, -2, 0, 'peak', 0.1), -1, 'source -2'),
    ((1, 0, 400, 0, 0, 0, 0, -1, 'peak', 0.1), -1, 'slot -1 out of range [0, 4096)'),
    ((1, 0, 400, 0, 0, 0, 0, 4096, 'peak', 0.1), -1, 'slot 4096 out of range [0, 4096)'),
    ((1, 0, 400, 0, 0, 0, 0, 0, 'peak') + tuple(0.01 * r for r in range(33)), -1, '33 cones: 0 to 32 are taken'),
    ((1, 0, 400, 0, 0, 0, 0, 0, 'peak', 'null:3'), -1, '3 cones asked for, cones is NULL'),
    ((1, 0, 400, 0, 0, 0, 0, 0, 'peak', 'null:-1'), -1, '-1 cones: 0 to 32 are taken'),
    ((1, 0, 400, 0, 0, 0, 0, 0, 'peak', 0.1, -0.2), -1, 'cones[1] = -0.2: the sine of a half-angle must be finite and >= 0'),
    ((1, 0, 400, 0, 0, 0, 0, 0, 'peak', 'nan'), -1, 'cones[0] = nan'),
    ((1, 0, 400, 0, 0, 0, 0, 0, 'peak', 0.1, 'inf'), -1, 'cones[1] = inf'),
    ((1, 0, 400, 0, 0, 0, 0, 0, 'peak', 0.1, 0.3, 0.2), -1, 'the cones must not decrease: cones[2] = 0.2 < cones[1] = 0.3'),
    ((1, 0, 400, 0, 0, 0, 0, 0, '0.1,inf', 0.1), -1, 'the centre is (0.1, inf): it must be finite'),
    ((1, 0, 400, 0, 0, 0, 0, 0, 'nan,0', 0.1), -1, 'the centre is (nan, 0): it must be finite'),
    ((1, 0, 1 << 31, 1, 0, 0, 0, 0, 'peak', 0.1), -1, 'the active plan has 2147483648 directions: 1 to 2147483647 are taken'),
    # an argument error is named before the state: a caller's mistake does not hide behind "nothing projected"
    ((0, 0, 0, 0, 0, 0, 3, 0, 'peak', 0.1), -1, 'source 3'),
]
SLOT_REFUSALS = [((-1, 1), 'first_slot -1 out of range [0, 4096)'), ((4096, 0), 'first_slot 4096 out of range [0, 4096)'),
                 ((0, -1), '-1 slots from slot 0 on'), ((4095, 2), '2 slots from slot 4095 on: the slots are [0, 4096)'),
                 ((1, 4096), '4096 slots from slot 1 on')]
ACCEPTED = [(1, 0, 400, 0, 0, 0, 0, 0, 'peak'), (1, 0, 400, 0, 0, 0, 0, 4095, '0.1,-0.2', 0.0, 0.1, 0.1),
            (1, 0, 400, 0, 400, 0, -1, 7, 'peak') + tuple(0.01 * r for r in range(32)), (1, 0, 400, 1, 400, 1, -1, 0, '0,0', 0.5),
            (1, 0, (1 << 31) - 1, 1, 0, 0, 0, 0, 'peak', 0.1)]


def test_refusals_name_the_numbers(tool):
    for args, code, said in REFUSALS:
        out = tool('check', *args)
        assert out.startswith('refused=%d\n' % code) and said in out, out
    for args in ACCEPTED:
        assert tool('check', *args) == 'ok=1\n', args
    for args, said in SLOT_REFUSALS:
        out = tool('slots', *args)
        assert out.startswith('refused=-1\n') and said in out, out
    for args in ((0, 0), (0, 4096), (4095, 1), (4095, 0), (7, 100)):
        assert tool('slots', *args) == 'ok=1\n'


def test_under_sanitizers(tool):
    """the same program under the address and undefined-behaviour sanitizers: same output, nothing reported"""
    san = 'farfield_beam_plan_san'
    assert tool(*COUNTS, exe=san) == tool(*COUNTS) and tool('layout', exe=san) == tool('layout')
    for args, _code, _said in REFUSALS:
        assert tool('check', *args, exe=san) == tool('check', *args)
    for args in ACCEPTED:
        assert tool('check', *args, exe=san) == 'ok=1\n'
    for args, _said in SLOT_REFUSALS:
        assert tool('slots', *args, exe=san) == tool('slots', *args)


# ---- postprocess.beam_metrics against the yardstick --------------------------------------------
def _seeded_map(shape, ux, uy, pair_list, seed):
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.0, 1.0, shape) ** 4
    if pair_list:
        P[ux ** 2 + uy ** 2 > 1] = np.nan
    else:
        P[ux[:, None] ** 2 + uy[None, :] ** 2 > 1] = np.nan
    return P


# NumPy's pairwise sum: blocks of at most 128 terms in 8 accumulators (16 additions in sequence and 3 to join them), then
# a tree over the blocks - below 2^20 terms at most 19 + 13 roundings; 64 units hold that with room, plus one for fsum
HOST_UNITS = 64


@pytest.mark.parametrize('pair_list, centre', [(False, 'peak'), (False, (0.05, -0.1)), (True, 'peak'), (True, (0.1, 0.0))])
def test_beam_metrics_against_the_yardstick(pair_list, centre):
    from metalens_amd import postprocess
    if pair_list:
        rng = np.random.default_rng(11)
        ux, uy = rng.uniform(-0.8, 0.8, 700), rng.uniform(-0.8, 0.8, 700)
        P = _seeded_map((700,), ux, uy, True, 12)
    else:
        ux, uy = np.linspace(-0.9, 0.9, 61), np.linspace(-0.85, 0.9, 47)
        P = _seeded_map((61, 47), ux, uy, False, 13)
    assert np.isnan(P).any()
    cones = (0.3, 0.05, 0.6, 0.3, 0.0)
    got = postprocess.beam_metrics(P, ux, uy, cones, centre, pair_list=pair_list)
    want = ref.record(P, ux, uy, pair_list, sorted(cones), None if centre == 'peak' else centre)
    assert got['peak_P'] == want['peak'] and got['finite'] == want['finite'] and tuple(got['centre_u']) == want['centre']
    flat = want['index']
    assert got['peak_index'] == (flat if pair_list else (flat // uy.size, flat % uy.size))
    assert tuple(got['peak_u']) == ((ux[flat], uy[flat]) if pair_list else (ux[flat // uy.size], uy[flat % uy.size]))
    assert abs(got['total_P'] - want['mom'][0]) <= HOST_UNITS * ref.U * want['mom_abs'][0]
    back = np.argsort(np.argsort(cones, kind='stable'), kind='stable')
    for r, b in enumerate(back):                          # the caller's order
        assert abs(got['cone_P'][r] - want['cone'][b]) <= HOST_UNITS * ref.U * want['cone_abs'][b], r
    assert got['cone_P'][0] == got['cone_P'][3] and got['cone_P'][4] <= got['cone_P'][1] <= got['cone_P'][0] <= got['cone_P'][2]
    s, sx, sy, sxx, syy, sxy = want['mom']
    assert np.allclose(got['centroid_u'], [want['centre'][0] + sx / s, want['centre'][1] + sy / s], rtol=0, atol=1e-13)
    assert np.allclose(got['second_moments_u'], [sxx / s - (sx / s) ** 2, syy / s - (sy / s) ** 2, sxy / s - sx * sy / s ** 2],
                       rtol=0, atol=1e-13)
    # moments about the centre: the same centroid and width about another centre
    other = postprocess.beam_metrics(P, ux, uy, (), (0.3, 0.3), pair_list=pair_list)
    assert np.allclose(other['centroid_u'], got['centroid_u'], rtol=0, atol=1e-13)
    assert np.allclose(other['second_moments_u'], got['second_moments_u'], rtol=0, atol=1e-13)


def test_beam_metrics_edges():
    from metalens_amd import postprocess
    ux, uy = np.linspace(1.1, 1.3, 5), np.linspace(1.1, 1.3, 4)
    none = postprocess.beam_metrics(np.full((5, 4), np.nan), ux, uy, (0.2,))
    assert np.isnan(none['peak_P']) and none['peak_index'] == (-1, -1) and none['finite'] == 0 and none['total_P'] == 0.0
    assert np.isnan(none['centre_u']).all() and np.isnan(none['centroid_u']).all() and none['cone_P'].tolist() == [0.0]
    given = postprocess.beam_metrics(np.full((5, 4), np.nan), ux, uy, (), (1.2, 1.2))
    assert given['centre_u'].tolist() == [1.2, 1.2] and given['cone_P'].shape == (0,)
    one = postprocess.beam_metrics(np.array([[2.0]]), [0.05], [-0.02], (0.0,))
    assert one['peak_index'] == (0, 0) and one['total_P'] == 2.0 and one['cone_P'].tolist() == [2.0] and one['centroid_u'].tolist() == [0.05, -0.02]
    row = postprocess.beam_metrics(np.ones((1, 3)), [0.05], [0.0, 0.25, 0.5], (0.25,), (0.05, 0.25))
    assert row['total_P'] == 0.75 and row['cone_P'].tolist() == [0.75] and row['second_moments_u'][0] == 0.0
    with pytest.raises(ValueError, match=r'P has shape \(3, 2\), the directions give \(2, 3\)'):
        postprocess.beam_metrics(np.ones((3, 2)), [0.0, 0.1], [0.0, 0.1, 0.2])


# ---- the Python argument checks -------------------------------------------------------------
class _NoCalls:
    """stands in for a Context: touching its library or its handle fails the test"""
    def __getattr__(self, name):
        raise AssertionError('a device call was made before the arguments were checked')


BAD_CONES = [(np.arange(33) * 0.01, 'at most 32 cones, got 33'), ([0.1, -0.2], r'finite and >= 0: cones\[1\] = -0.2'),
             ([np.nan], r'cones\[0\] = nan'), ([0.1, 0.2, np.inf], r'cones\[2\] = inf'), ([[0.1, 0.2]], 'cones must be a sequence of numbers'),
             ('wide', 'cones must be a sequence of numbers'), (0.1, 'cones must be a sequence of numbers')]
BAD_CENTRES = [((0.1,), "centre must be 'peak' or one"), ((0.1, 0.2, 0.3), "centre must be 'peak' or one"), ('centroid', "centre must be 'peak' or one"),
               (None, "centre must be 'peak' or one"), (np.zeros((2, 2)), "centre must be 'peak' or one"), ((np.nan, 0.0), 'a centre must be finite')]


def test_beam_argument_errors_come_before_any_device_call(no_device):
    from metalens_amd import postprocess
    from metalens_amd.nearfield_farfield import FarfieldTransform
    t = types.SimpleNamespace(ctx=_NoCalls(), ux=np.zeros(3), uy=np.zeros(3), pair_list=False, owner=1)
    beam = lambda *a, **k: FarfieldTransform.beam(t, *a, **k)
    for bad, said in BAD_CONES:
        with pytest.raises(ValueError, match=said):
            beam(bad)
        with pytest.raises(ValueError, match=said):
            postprocess.beam_metrics(np.zeros((3, 3)), t.ux, t.uy, bad)
    for bad, said in BAD_CENTRES:
        with pytest.raises(ValueError, match=said):
            beam([0.1], centre=bad)
    for bad in ('sum', 'fields', None, 0):
        with pytest.raises(ValueError, match="of must be 'projection' or 'sums'"):
            beam([0.1], of=bad)
    # what the checks hand on: the cones ascending and the way back, the centre as a pair or None for the peak
    c, back, ce = postprocess._check_beam([0.3, 0.1, 0.2, 0.1], (0.05, -0.1), 'sums')
    assert c.tolist() == [0.1, 0.1, 0.2, 0.3] and c[back].tolist() == [0.3, 0.1, 0.2, 0.1] and ce.tolist() == [0.05, -0.1]
    c, back, ce = postprocess._check_beam((), 'peak')
    assert c.shape == (0,) and back.shape == (0,) and ce is None and c.dtype == np.float64


def test_sweep_argument_errors_come_before_any_device_call(no_device):
    from metalens_amd.sweep import SourceSweep
    sw = SourceSweep.__new__(SourceSweep)
    sw.__dict__.update(ctx=_NoCalls(), x=np.zeros(20), y=np.zeros(24), ux=np.zeros(5), uy=np.zeros(4))
    src = [(0.0, 0.0, -1e-4, 'x')]
    for bad, said in BAD_CONES:
        with pytest.raises(ValueError, match=said):
            sw.run(src, beam_cones=bad)
    for bad, said in BAD_CENTRES:
        with pytest.raises(ValueError, match=said):
            sw.run(src, beam_cones=(0.1,), beam_centre=bad)
    with pytest.raises(ValueError, match='with beam_cones= takes 1 to 4095 sources'):
        sw.run(src * 4096, beam_cones=())
    with pytest.raises(ValueError, match='a sweep takes 1 to 4096 sources, got 4097'):      # as before
        sw.run(src * 4097, beam_cones=())


def test_wavelength_sweep_forwards_the_beam_arguments():
    """WavelengthSweep.run hands beam_cones and beam_centre on to every member's run"""
    from metalens_amd.sweep import WavelengthSweep
    seen = []

    class Member:
        ux = uy = np.zeros(2)

        def run(self, sources, weights=None, **kwargs):
            seen.append(kwargs)
            return {'total_P': np.ones(1), 'power_in': np.ones(1), 'P_sum': np.zeros((2, 2))}
    ws = WavelengthSweep.__new__(WavelengthSweep)
    ws.sweeps, ws.wavelengths = [Member(), Member()], [1.0, 2.0]
    ws.run([(0.0, 0.0, -1e-4, 'x')], beam_cones=(0.1, 0.2), beam_centre=(0.0, 0.1))
    assert seen == [dict(beam_cones=(0.1, 0.2), beam_centre=(0.0, 0.1))] * 2


def test_pass_adds_one_asynchronous_call_and_no_synchronisation():
    """what ``_pass`` calls per member with and without a beam: the one ml_farfield_beam behind ml_farfield_accumulate, into
    the member's slot, and nothing else"""
    from metalens_amd import _lib, sweep

    calls = []

    class Lib:
        def __getattr__(self, name):
            def call(*args):
                calls.append((name,) + tuple(a for a in args[1:] if isinstance(a, (int, float))))
                return 0
            return call
    ctx = types.SimpleNamespace(lib=Lib(), handle=None)
    sw = sweep.SourceSweep.__new__(sweep.SourceSweep)
    sw.__dict__.update(ctx=ctx, x=_lib.f64(np.zeros(4)), y=_lib.f64(np.zeros(4)), wavelength=580e-9, n_glass=1.46, dipole_moment=1.0,
                       c0=3e8, Z0=377.0)
    group = {'pos': (0.0, 0.0, -1e-4), 'members': [(5, 'x'), (6, 'y')], 'positions': [(0.0, 0.0, -1e-4)] * 2}
    weights = np.ones(8)
    sw._pass(group, None, (0.0, 0.0, 0.0), weights)
    plain, calls[:] = list(calls), []
    cones = _lib.f64([0.1, 0.2])
    sw._pass(group, None, (0.0, 0.0, 0.0), weights, None, (cones, None))
    names = [c[0] for c in calls]
    assert [n for n in names if n != 'ml_farfield_beam'] == [c[0] for c in plain]
    assert names.count('ml_farfield_beam') == 2 and 'ml_sync' not in names and 'ml_farfield_beams' not in names
    at = [i for i, n in enumerate(names) if n == 'ml_farfield_beam']
    assert all(names[i - 1] == 'ml_farfield_accumulate' for i in at)
    assert [calls[i][1:] for i in at] == [(0, 2, 5), (0, 2, 6)]          # source 0, two cones, the member's slot


def test_entries_in_header_and_binding():
    from metalens_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, n_args in (('ml_farfield_beam', 6), ('ml_farfield_beams', 4)):
        decl = re.search(r'int\s+%s\s*\(([^)]*)\)' % name, code)
        assert decl and len(decl.group(1).split(',')) == n_args and name in _lib.SYMBOLS
        assert len(getattr(_lib.load(), name).argtypes) == n_args
    lib = _lib.load()
    rec = np.zeros(ref.RECORD)
    assert lib.ml_farfield_beam(None, 0, None, None, 0, 0) != 0 and lib.ml_farfield_beams(None, 0, 1, _lib.dptr(rec)) != 0      # no context
    assert 'ml_abi_version' in code and lib.ml_abi_version() == 1
