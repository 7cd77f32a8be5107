"""The pupil function applied to the near field without a GPU: the plan arithmetic and the argument checks of
csrc/fields_pupil.h through tools/fields_pupil_plan.cpp - what a plan uploads, the monomial coefficients and the line table
against the Python side to the bit, every refusal with its wording, once more under the address and undefined-behaviour
sanitizers -, ``postprocess.pupil_factor`` and ``apply_pupil_host`` against the long-double yardstick (tests/fields_pupil_ref.py)
within its bound, every ``ValueError`` of ``AperturePupil`` before any device call, the entries' presence in header, binding,
export map and Makefile, and the loop measure, correct, measure on the NumPy twins."""
import os
import re
import subprocess

import numpy as np
import pytest

import fields_pupil_ref as ref
import fields_wavefront_ref as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL = 580e-9
P = WL / 2.2


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('pupil_plan')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'fields_pupil_plan', out + 'fields_pupil_plan_san'])

    def run(*args, exe='fields_pupil_plan'):
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


def _list(v):
    return ','.join('%.17g' % t for t in np.ravel(v))


# ---- the plan program -----------------------------------------------------------------------
def test_plan_layout_and_uploads(tool):
    from metalens_amd import postprocess as pp, pupil
    assert tool('layout') == 'order_max=%d nq=%d edges_max=%d sets_max=%d block=64 line_threads=256 phase_limit=%g\n' % (
        pp.ZERNIKE_ORDER_MAX, pp.PUPIL_NQ, pp.ZONES_EDGES_MAX, pupil.SETS_MAX, pp.PUPIL_PHASE_LIMIT)
    shapes = [(1, 1, 0), (130, 129, 7), (4096, 4096, 198), (8192, 8192, 4096)]
    lines = tool(*[v for s in shapes for v in s]).splitlines()
    for (nx, ny, K), line in zip(shapes, lines):
        assert line == 'nx=%d ny=%d edges=%d doubles=%d' % (nx, ny, K, nx * 10 + 2 * ny + 3 * K), line
    assert tool(*[v for s in shapes for v in s], exe='fields_pupil_plan_san').splitlines() == lines


@pytest.mark.parametrize('n_max', [0, 1, 4, 5, 8])
def test_monomials_and_line_table_have_the_twins_bits(tool, n_max):
    """pupil_monomials and pupil_line_table of the header against ``_pupil_monomials`` and ``_pupil_line_table``: the same doubles
    from the same coefficients, plain and sanitized; and the polynomial they state is the phase plate, against the polar form"""
    from metalens_amd import postprocess as pp
    c = ref.seeded_phase(n_max, seed=40 + n_max, scale=2.0)
    B = pp._pupil_monomials(n_max, c)
    xi = np.random.default_rng(n_max).uniform(-1, 1, 7)
    table = pp._pupil_line_table(n_max, B, xi)
    for exe in ('fields_pupil_plan', 'fields_pupil_plan_san'):
        lines = tool('monomials', n_max, _list(c), exe=exe).splitlines()
        want = [(p, q) for p in range(n_max + 1) for q in range(n_max + 1 - p)]
        assert len(lines) == len(want) + 1
        for (p, q), line in zip(want, lines):
            assert line == 'p=%d q=%d B=%.17g' % (p, q, B[p, q]), line
        assert lines[-1] == 'reach=%.17g' % np.abs(B).ravel().cumsum()[-1]
        got = np.array([[float(v) for v in line.split()] for line in tool('table', n_max, _list(c), _list(xi), exe=exe).splitlines()])
        assert got.shape == (7, 9) and got.tobytes() == table.tobytes()
    assert (B[np.add.outer(np.arange(9), np.arange(9)) > n_max] == 0).all() and (table[:, n_max + 1:] == 0).all()
    # the polynomial against sum c_j Z_j in polar form, in long double, at seeded points of the disc
    rng = np.random.default_rng(3)
    rho, phi = np.sqrt(rng.uniform(0, 1, 500)), rng.uniform(-np.pi, np.pi, 500)
    x, e = rho * np.cos(phi), rho * np.sin(phi)
    poly = sum(B[p, q] * x ** p * e ** q for p in range(n_max + 1) for q in range(n_max + 1 - p))
    want = sum(np.longdouble(cj) * wref.zernike_ld(n, m, x, e) for cj, (n, m) in zip(c, wref.terms(n_max)))
    Psi = (np.abs(c) * wref.amplitudes(n_max)).sum()
    assert np.abs(poly - want).max() <= (64 + 5 * n_max) * Psi * ref.U


# n_ranks stop n_max r2 x2 xi y2 eta c e2 g -> message
X2, XI, Y2, ETA = '1,0,1', '-0.5,0,0.5', '4,1,0,1', '-1,-0.5,0,0.5'
OK = (1, 1, 0, 4, X2, XI, Y2, ETA, 'null', 'null', 'null')
NAMES = ('n_ranks', 'stop', 'n_max', 'r2', 'x2', 'xi', 'y2', 'eta', 'c', 'e2', 'g')


def _with(**kw):
    args = dict(zip(NAMES, OK))
    args.update(kw)
    return tuple(args[n] for n in NAMES)


Q = 'ml_fields_pupil_plan: '
REFUSALS = [
    (_with(n_ranks=2), Q + 'this context belongs to a communicator of 2 ranks'),
    (_with(stop=2), Q + 'stop = 2: 0 to leave the samples outside the pupil standing or 1 to clear them'),
    (_with(n_max=-1), Q + 'n_max = -1: radial orders 0 to 8 are taken'),
    (_with(n_max=9), Q + 'n_max = 9: radial orders 0 to 8 are taken'),
    (_with(x2='null', xi='null'), Q + 'the axes have 0 x 4 samples: at least one each'),
    (_with(xi='null'), Q + 'NULL argument'),
    (_with(eta='null'), Q + 'NULL argument'),
    (_with(e2='1,4'), Q + 'NULL argument'),
    (_with(r2=0), Q + 'r2 = 0: the squared radius of the pupil must be finite and > 0'),
    (_with(r2='nan'), Q + 'r2 = nan: the squared radius'),
    (_with(r2='inf'), Q + 'r2 = inf: the squared radius'),
    (_with(x2='1,-1,1'), Q + 'x2[1] = -1: a squared distance must be finite and >= 0'),
    (_with(y2='4,1,nan,1'), Q + 'y2[2] = nan: a squared distance'),
    (_with(xi='0,inf,0'), Q + 'xi[1] = inf: a pupil coordinate must be finite'),
    (_with(eta='0,0,0,nan'), Q + 'eta[3] = nan: a pupil coordinate must be finite'),
    (_with(y2='4,1,2,1'), Q + 'y2 must fall to its minimum y2[1] = 1 and rise again (a y axis in ascending or descending order): '
                              'y2[3] = 1 follows y2[2] = 2'),
    (_with(e2='1,-4', g='1,0,1,0'), Q + 'e2[1] = -4: a squared edge must be finite and >= 0'),
    (_with(e2='4,1', g='1,0,1,0'), Q + 'the edges must not decrease: e2[1] = 1 < e2[0] = 4'),
    (_with(e2='1,4', g='1,0,nan,0'), Q + 'g[1] = (nan, 0): a zone factor must be finite'),
    (_with(e2='1,4', g='1,inf,0,0'), Q + 'g[0] = (1, inf): a zone factor must be finite'),
    (_with(n_max=1, c='0,nan,0'), Q + 'c[1] = nan: a phase coefficient must be finite'),
    (_with(n_max=1, c='0,3e8,3e8'), Q + 'the phase plate can reach 1.2e+09 rad on the unit disc: the phase arithmetic covers up to 1e+09'),
]
ACCEPTED = [(OK, 0.0), (_with(stop=0), 0.0), (_with(n_max=8), 0.0), (_with(e2='1,4', g='1,0,0,1'), 0.0), (_with(y2='0,1,4,9'), 0.0),
            (_with(y2='9,4,1,1'), 0.0), (_with(n_max=1, c='0,2.5e8,2.5e8'), 1e9), (_with(n_max=0, c='-3'), 3.0), (_with(r2=1e-300), 0.0)]

# n_ranks res_nx res_ny res_sets plan_valid plan_nx plan_ny first n_sets -> code, message
A = 'ml_fields_pupil_apply: '
APPLY = [
    ((1, 3, 4, 1, 1, 3, 4, 0, 1), 0, ''),
    ((1, 3, 4, 3, 1, 3, 4, 1, 2), 0, ''),
    ((2, 3, 4, 1, 1, 3, 4, 0, 1), -1, A + 'this context belongs to a communicator of 2 ranks'),
    ((1, 3, 4, 1, 1, 3, 4, 0, 0), -1, A + 'a pass takes 1 to 3 field sets, got 0'),
    ((1, 3, 4, 4, 1, 3, 4, 0, 4), -1, A + 'a pass takes 1 to 3 field sets, got 4'),
    ((1, 3, 4, 1, 0, 0, 0, 0, 1), -2, A + 'no pupil has been planned on this context (ml_fields_pupil_plan)'),
    ((1, 0, 0, 0, 1, 3, 4, 0, 1), -2, 'no resident field set'),
    ((1, 3, 5, 1, 1, 3, 4, 0, 1), -2, A + 'the pupil was planned for 3 x 4 samples, the resident field sets have 3 x 5'),
    ((1, 4, 4, 1, 1, 3, 4, 0, 1), -2, A + 'the pupil was planned for 3 x 4 samples, the resident field sets have 4 x 4'),
    ((1, 3, 4, 1, 1, 3, 4, 1, 1), -1, A + 'field sets 1 ... 1 asked for, 1 resident'),
    ((1, 3, 4, 2, 1, 3, 4, 0, 3), -1, A + 'field sets 0 ... 2 asked for, 2 resident'),
    ((1, 3, 4, 1, 1, 3, 4, -1, 1), -1, A + 'field sets -1 ... -1 asked for, 1 resident'),
]


def test_refusals_name_the_numbers(tool):
    for exe in ('fields_pupil_plan', 'fields_pupil_plan_san'):
        for args, said in REFUSALS:
            out = tool('check', *args, exe=exe)
            assert out.startswith('refused=-1\n') and said in out, (out, said)
        for args, reach in ACCEPTED:
            assert tool('check', *args, exe=exe) == 'ok=1 reach=%.17g\n' % reach, args
        for args, code, said in APPLY:
            out = tool('apply', *args, exe=exe)
            assert out == ('ok=1\n' if code == 0 else 'refused=%d\n%s\n' % (code, said)), (args, out)
    # every refusal has a wording of its own: the messages differ beyond their numbers
    shapes = {re.sub(r'[-+]?(\d+\.?\d*(e[-+]?\d+)?|nan|inf)', '#', tool('check', *a).splitlines()[1]) for a, _s in REFUSALS}
    assert len(shapes) >= 15


# ---- the twins against the yardstick --------------------------------------------------------
def _axes(nx, ny, cx, cy):
    return (np.arange(nx) - cx) * P, (np.arange(ny) - cy) * P


def _zones(R, K, seed):
    """K edges up to 1.1 R and K seeded factors, among them 0 and 1"""
    rng = np.random.default_rng(seed)
    e = np.sort(rng.uniform(0.05, 1.1, K)) * R
    g = rng.uniform(0.2, 1.5, K) * np.exp(2j * np.pi * rng.uniform(0, 1, K))
    g[0] = 1.0
    if K > 1:
        g[K // 2] = 0.0
    return e, g


TWIN_CASES = [
    ('130x129 stop', _axes(130, 129, 64.5, 64), 15e-6, (0.0, 0.0), dict(stop=True)),
    ('130x129 order 4', _axes(130, 129, 64.5, 64), 15e-6, (0.0, 0.0), dict(stop=True, phase=4)),
    ('130x129 order 8 edges 7 no stop', _axes(130, 129, 64.5, 64), 15e-6, (0.0, 0.0), dict(stop=False, phase=8, edges=7)),
    ('70x257 order 5 edges 1', _axes(70, 257, 30.3, 100.7), 9.1e-6, (0.37e-6, -1.21e-6), dict(stop=True, phase=5, edges=1)),
    ('70x257 edges 4096 no stop', _axes(70, 257, 30.3, 100.7), 9.1e-6, (0.37e-6, -1.21e-6), dict(stop=False, edges=4096)),
    ('33x300 descending order 0', (_axes(33, 300, -20.0, -7.4)[0], _axes(33, 300, -20.0, -7.4)[1][::-1]), 30e-6, (0.0, 0.0), dict(stop=False, phase=0)),
    ('identity', _axes(64, 70, 30.5, 33.2), 5e-6, (0.0, 0.0), dict(stop=False)),
]


def _pupil_kw(R, opt, seed):
    kw = dict(stop=opt['stop'])
    if 'phase' in opt:
        kw['phase'] = ref.seeded_phase(opt['phase'], seed)
    if 'edges' in opt:
        kw['edges'], kw['zone_factors'] = _zones(R, opt['edges'], seed + 1)
    return kw


@pytest.mark.parametrize('case', TWIN_CASES, ids=lambda c: c[0].replace(' ', '_'))
def test_twin_against_the_yardstick(case):
    from metalens_amd import postprocess
    name, (x, y), R, centre, opt = case
    kw = _pupil_kw(R, opt, seed=x.size + y.size)
    F = ref.seeded_fields(2, x.size, y.size, seed=x.size * 1000 + y.size)
    got = np.stack(postprocess.apply_pupil_host(F[:, 0], F[:, 1], F[:, 2], F[:, 3], x, y, R, centre=centre, **kw), axis=1)
    want = ref.parts(x, y, R, centre, **kw)
    ref.hold('twin ' + name, got, F, want)
    member, f = postprocess.pupil_factor(x, y, R, centre=centre, **kw)
    assert np.array_equal(member, want['member']) and f.shape == member.shape and (f[want['zero']] == 0).all()
    keep = ~want['zero'] & ~want['touch']
    assert (f[keep] == 1).all()
    err = np.hypot(f.real.astype(ref.LD) - np.where(want['zero'], 0, want['fr']), f.imag.astype(ref.LD) - np.where(want['zero'], 0, want['fi']))
    assert (err <= want['g_abs'] * ((64 + 5 * want['n_max']) * want['Psi'] + 24) * ref.U).all()
    # one set given as 2-D arrays: the same bytes
    one = postprocess.apply_pupil_host(F[1, 0], F[1, 1], F[1, 2], F[1, 3], x, y, R, centre=centre, **kw)
    assert all(one[q].shape == (x.size, y.size) and one[q].tobytes() == got[1, q].tobytes() for q in range(4))
    if name == 'identity':
        assert got.tobytes() == F.tobytes() and not want['touch'].any() and not want['zero'].any()
    else:
        assert want['touch'].any() or want['zero'].any()
    if 'edges' in opt and not opt['stop']:
        assert (want['touch'] & ~want['member']).any()        # non-members left standing take their zone factor


def test_rim_and_edges_on_integers():
    """x = i, y = j: (3, 4), (4, 3), (5, 0) and (0, 5) lie exactly on R = 5 and are inside; edges 3 and 5: (0, 3) and (3, 0) lie on
    the first edge and belong to zone 0, the rim to zone 1"""
    from metalens_amd import postprocess
    x, y = np.arange(16.0), np.arange(70.0)
    member, f = postprocess.pupil_factor(x, y, 5.0, edges=[3.0, 5.0], zone_factors=[2.0, 1j])
    assert member[3, 4] and member[4, 3] and member[5, 0] and member[0, 5] and not member[4, 4] and not member[5, 1] and member.sum() == 26
    assert f[0, 3] == 2 and f[3, 0] == 2 and f[1, 3] == 1j and f[3, 4] == 1j and f[5, 0] == 1j and f[4, 4] == 0 and f[0, 0] == 2
    member, f = postprocess.pupil_factor(x, y, 4.0, stop=False, edges=[3.0, 5.0], zone_factors=[2.0, 1j])
    assert not member[3, 4] and f[3, 4] == 1j and f[4, 4] == 1 and f[5, 1] == 1 and member.sum() == 17


# ---- the Python argument checks -------------------------------------------------------------
AX = np.linspace(-1e-5, 1e-5, 9)
BAD = [
    (dict(xp_list=[[0.0, 1.0]]), 'xp_list must be a sequence of at least one number'),
    (dict(yp_list=[0.0, np.nan]), r'yp_list must be finite: yp_list\[1\] = nan'),
    (dict(yp_list=[0.0, 2.0, 1.0]), r'yp_list must be in ascending or descending order .* yp_list\[2\] = 1 follows yp_list\[1\] = 2'),
    (dict(radius=0.0), 'the radius of the pupil must be finite and > 0, got 0.0'),
    (dict(radius=np.nan), 'the radius of the pupil must be finite and > 0'),
    (dict(radius='wide'), 'radius must be one number'),
    (dict(centre=(0.0,)), r'centre must be one \(xc, yc\)'),
    (dict(centre=(0.0, np.inf)), 'a centre must be finite'),
    (dict(stop=1), 'stop must be True or False, got 1'),
    (dict(phase=[0.0, 1.0]), r'phase must hold the \(n_max \+ 1\)\(n_max \+ 2\) / 2 coefficients .* got an array of shape \(2,\)'),
    (dict(phase=np.zeros(55)), r'1, 3, 6, ... 45 numbers, got an array of shape \(55,\)'),
    (dict(phase='coma'), 'phase must be a sequence of Zernike coefficients in radians'),
    (dict(phase=[0.0, np.inf, 0.0]), r'a phase coefficient must be finite: phase\[1\] = inf'),
    (dict(phase=[0.0, 3e8, 3e8]), r'the phase plate can reach 1\.2e\+09 rad on the unit disc: the phase arithmetic covers up to 1e\+09'),
    (dict(edges=[1e-6]), 'edges and zone_factors go together: one factor per zone, got edges=given and zone_factors=None'),
    (dict(zone_factors=[1.0]), 'edges and zone_factors go together'),
    (dict(edges=[2e-6, 1e-6], zone_factors=[1, 1]), r'the edges must not decrease: edges\[1\] = 1e-06 < edges\[0\] = 2e-06'),
    (dict(edges=[], zone_factors=[]), 'zones take 1 to 4096 edges, got 0'),
    (dict(edges=[1e-6, 2e-6], zone_factors=[1.0]), r'zone_factors must hold one factor per edge: got shape \(1,\) for 2 edges'),
    (dict(edges=[1e-6], zone_factors=[np.nan]), r'a zone factor must be finite: zone_factors\[0\]'),
    (dict(edges=[1e-6], zone_factors=['g']), 'zone_factors must be a sequence of complex numbers'),
]


def test_argument_errors_come_before_any_device_call(no_device):
    import metalens_amd as ma
    from metalens_amd import postprocess
    base = dict(xp_list=AX, yp_list=AX, radius=8e-6)
    F = np.zeros((9, 9), dtype=complex)
    for bad, said in BAD:
        kw = dict(base, **bad)
        with pytest.raises(ValueError, match=said):
            ma.AperturePupil(**kw)
        with pytest.raises(ValueError, match=said):
            ma.apply_pupil(F, F, F, F, **kw)
        x, y, R = kw.pop('xp_list'), kw.pop('yp_list'), kw.pop('radius')
        with pytest.raises(ValueError, match=said):
            postprocess.pupil_factor(x, y, R, **kw)
        with pytest.raises(ValueError, match=said):
            postprocess.apply_pupil_host(F, F, F, F, x, y, R, **kw)
    for first, n, said in ((-1, None, 'first must be a field set index >= 0'), (0, 0, 'takes 1 to 3 field sets per call, got n = 0'), (0, 4, 'got n = 4')):
        with pytest.raises(ValueError, match=said):
            ma.apply_pupil(None, None, None, None, first=first, n=n, **base)
        with pytest.raises(ValueError, match=said):
            ma.AperturePupil.queue(object(), first, n)
    with pytest.raises(ValueError, match=r'Hx has shape \(9, 8\), the axes give \(9, 9\)'):
        postprocess.apply_pupil_host(F, F, F[:, :8], F, AX, AX, 8e-6)
    # what the checks hand on
    z = postprocess._check_pupil(AX, AX[::-1], 8e-6, (1e-6, -2e-6), False, np.arange(6.0) / 10, [1e-6, 3e-6], [1.0, 2j])
    assert np.array_equal(z['x2'], (AX - 1e-6) ** 2) and np.array_equal(z['y2'], (AX[::-1] + 2e-6) ** 2) and z['r2'] == 8e-6 * 8e-6
    assert np.array_equal(z['xi'], (AX - 1e-6) / 8e-6) and np.array_equal(z['eta'], (AX[::-1] + 2e-6) / 8e-6) and z['stop'] == 0
    assert z['n_max'] == 2 and np.array_equal(z['c'], np.arange(6.0) / 10) and np.array_equal(z['e2'], np.array([1e-6, 3e-6]) ** 2)
    assert np.array_equal(z['g'], [[1.0, 0.0], [0.0, 2.0]])
    z = postprocess._check_pupil(AX, AX, 8e-6)
    assert z['stop'] == 1 and z['c'] is None and z['e2'] is None and z['g'] is None


class _Sweep:
    """what SourceSweep._check_pupil reads of a sweep"""
    def __init__(self, ctx, nx, ny):
        self.ctx, self.x, self.y = ctx, np.zeros(nx), np.zeros(ny)


def test_sweep_refuses_a_foreign_pupil_before_any_device_call(no_device):
    from metalens_amd.sweep import SourceSweep

    class _Pupil:
        def __init__(self, ctx, shape):
            self.ctx, self.shape = ctx, shape
    ctx = object()
    assert SourceSweep._check_pupil(_Sweep(ctx, 9, 8), None) is None and SourceSweep._check_pupil(_Sweep(ctx, 9, 8), _Pupil(ctx, (9, 8))) is None
    with pytest.raises(ValueError, match=r'pupil= must be an AperturePupil built on the context of this sweep \(ctx=sweep.ctx\)'):
        SourceSweep._check_pupil(_Sweep(ctx, 9, 8), _Pupil(object(), (9, 8)))
    with pytest.raises(ValueError, match=r"pupil= was built for an aperture of 9 x 9 samples, the sweep's grid has 9 x 8"):
        SourceSweep._check_pupil(_Sweep(ctx, 9, 8), _Pupil(ctx, (9, 9)))


def test_entries_in_header_binding_export_map_and_makefiles():
    import metalens_amd as ma
    from metalens_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    plan = re.search(r'int\s+ml_fields_pupil_plan\s*\(([^)]*)\)', code)
    apply = re.search(r'int\s+ml_fields_pupil_apply\s*\(([^)]*)\)', code)
    assert plan and len(plan.group(1).split(',')) == 14 and apply and len(apply.group(1).split(',')) == 3
    assert 'ml_fields_pupil_plan' in _lib.SYMBOLS and 'ml_fields_pupil_apply' in _lib.SYMBOLS
    assert re.search(r'#define\s+ML_ABI_VERSION\s+1\b', text)
    lib = _lib.load()
    assert len(lib.ml_fields_pupil_plan.argtypes) == 14 and len(lib.ml_fields_pupil_apply.argtypes) == 3
    exports = open(os.path.join(ROOT, 'metalens_amd', 'csrc', 'exports.map')).read()
    assert re.search(r'global:\s*ml_\*;', exports) and 'ml_fields_pupil_plan' in exports and 'ml_fields_pupil_apply' in exports
    import makefile_deps
    assert makefile_deps.header_is_prerequisite('fields_pupil.h', 'fields_pupil')   # (the unit is built, the header rebuilds it)
    tools = open(os.path.join(ROOT, 'tools', 'Makefile')).read()
    assert '$(OUT)fields_pupil_plan:' in tools and '$(OUT)fields_pupil_plan_san:' in tools
    for name in ('AperturePupil', 'apply_pupil', 'apply_pupil_host', 'pupil_factor', 'pupil'):
        assert hasattr(ma, name), name
    assert lib.ml_fields_pupil_plan(None, None, None, 0, None, None, 0, 0.0, 1, 0, None, None, 0, None) != 0        # no context
    assert b'NULL argument' in lib.ml_last_error()
    assert lib.ml_fields_pupil_apply(None, 0, 1) != 0 and b'NULL argument' in lib.ml_last_error()


# ---- measure, correct, measure on the twins -------------------------------------------------
def loop_field(x, y, R, centre):
    """``E = (1 + 0.1 cos 3 xi) exp(i W)``, ``W = 0.3 Z(3, 1) + 0.2 Z(2, 0) - 0.15 Z(2, -2) + 0.1 Z(1, 1)``, as all four fields"""
    from metalens_amd import postprocess
    xi, eta = ((x - centre[0]) / R)[:, None], ((y - centre[1]) / R)[None, :]
    W = (0.3 * postprocess.zernike(3, 1, xi, eta) + 0.2 * postprocess.zernike(2, 0, xi, eta) - 0.15 * postprocess.zernike(2, -2, xi, eta)
         + 0.1 * postprocess.zernike(1, 1, xi, eta))
    E = (1 + 0.1 * np.cos(3 * xi)) * np.exp(1j * W)
    return np.stack([E, E, E, E])


# Both pupils lie wholly inside their grids (70 x 257: the samples reach 8.36 um from the centre along -x, R = 8.3 um).  The
# reading ``wavefront`` takes the terms as orthogonal over the pupil, which a sampled WHOLE disc is to O(pitch / R); a disc the
# grid's edge cuts is not, and the loop then contracts by its non-orthogonality instead (R = 9.1 um on the same grid: ratios
# 0.135, 0.18, 0.38) - a property of the measurement, not of the pupil's application.
LOOP_CASES = {'130x129': (_axes(130, 129, 64.5, 64), 15e-6, (0.0, 0.0)),
              '70x257': (_axes(70, 257, 30.3, 100.7), 8.3e-6, (0.37e-6, -1.21e-6))}


@pytest.mark.parametrize('name', sorted(LOOP_CASES))
def test_measure_correct_measure_converges_on_the_twins(name):
    """three rounds of ``wavefront_metrics`` (order 4) -> ``phase = -wavefront`` (piston left out) -> ``apply_pupil_host``: every round
    brings the rms under 0.2 of the round before and the coherence does not fall.  On 130 x 129, R = 15 um: rms 0.377 ->
    0.0506 -> 0.0045 -> 0.0004, coherence 0.854 -> 0.9934 -> 0.99614 -> 0.99616 (the amplitude ripple keeps it below 1)."""
    from metalens_amd import postprocess
    (x, y), R, centre = LOOP_CASES[name]
    F = loop_field(x, y, R, centre)
    rms, coh = [], []
    for _ in range(4):
        res = postprocess.wavefront_metrics(F[0], F[1], F[2], F[3], x, y, WL, 1.46, R, 4, centre=centre)
        rms.append(float(res['rms'][0, 0]))
        coh.append(float(res['coherence'][0, 0]))
        phase = -res['wavefront'][0, 0]
        phase[0] = 0.0
        F = np.stack(postprocess.apply_pupil_host(F[0], F[1], F[2], F[3], x, y, R, centre=centre, stop=False, phase=phase))
    print('loop %s: rms %s coherence %s' % (name, ' -> '.join('%.4g' % v for v in rms), ' -> '.join('%.5f' % v for v in coh)))
    assert all(b < 0.2 * a for a, b in zip(rms, rms[1:])), rms
    assert all(b >= a for a, b in zip(coh, coh[1:])), coh
    if name == '130x129':
        assert abs(rms[0] - 0.377) < 1e-3 and abs(rms[1] - 0.0506) < 1e-4 and abs(coh[0] - 0.854) < 1e-3 and abs(coh[3] - 0.99616) < 1e-5
