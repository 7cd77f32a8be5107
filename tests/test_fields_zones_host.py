"""The per-zone sums of the near field without a GPU: the plan arithmetic and the argument checks of csrc/fields_zones.h
through tools/fields_zones_plan.cpp - layout and scratch against the Python side, every refusal with its wording, once more
under the address and undefined-behaviour sanitizers -, ``postprocess.zone_metrics`` against the long-double yardstick
(tests/fields_zones_ref.py) within its bounds, ``zone_edges`` against the oracle's ring decisions, every ``ValueError`` of
``ApertureZones`` before any device call, and the entry's presence in header, binding and export map."""
import os
import re
import subprocess

import numpy as np
import pytest

import fields_zones_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1, 1), (1, 3, 64, 2), (1, 3, 65, 2), (2, 64, 3, 1), (1, 64, 70, 4096), (1, 33, 300, 300), (3, 96, 130, 22),
          (3, 4096, 4096, 1000), (3, 8192, 8192, 4096)]


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('zones_plan')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'fields_zones_plan',
                           out + 'fields_zones_plan_san'])

    def run(*args, exe='fields_zones_plan'):
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


def _flat(shapes):
    return [v for s in shapes for v in s]


# ---- the plan program -----------------------------------------------------------------------
def test_plan_of_the_shapes(tool):
    lines = tool(*_flat(SHAPES)).splitlines()
    assert len(lines) == len(SHAPES)
    for (sets, nx, ny, K), line in zip(SHAPES, lines):
        f = _facts(line)
        cap = min(ny, 2 * K)
        assert f == dict(sets=sets, nx=nx, ny=ny, k=K, blocks=-(-ny // 64), capacity=cap, scratch=sets * nx * cap * 64 + nx * 8,
                         bound=sets * nx * min(ny + 2, 2 * K + 2) * 64), line
        assert f['scratch'] <= f['bound']
    assert _facts(lines[-2])['scratch'] == 1572896768          # three sets of 4096^2 with a thousand edges: 1.57 GB


def test_record_layout(tool):
    from metalens_amd import postprocess as pp, zones
    f = _facts(tool('layout'))
    assert f == dict(n=pp._ZONES_N, s=pp._ZONES_S, ix=pp._ZONES_IX, iy=pp._ZONES_IY, cx=pp._ZONES_CX, cy=pp._ZONES_CY,
                     record=pp.ZONES_RECORD, terms=7, run_bytes=64, edges_max=pp.ZONES_EDGES_MAX, sets_max=zones.SETS_MAX, block=64,
                     plane=pp.ZONES_REF_PLANE, focus=pp.ZONES_REF_FOCUS)
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    for name, value in (('ML_ZONES_EDGES_MAX', 4096), ('ML_ZONES_RECORD', 8), ('ML_ZONES_REF_PLANE', 0), ('ML_ZONES_REF_FOCUS', 1)):
        assert re.search(r'#define\s+%s\s+%d\b' % (name, value), text), name
    assert tool('vertex', '4,1,1,2') == 'jv=1\n' and tool('vertex', '3,2,1') == 'jv=2\n' and tool('vertex', '0,1') == 'jv=0\n'


# n_ranks res_nx res_ny res_sets first n_sets ref_mode ref_c k record_doubles x2 y2 e2 ra rb -> code, message
X2, Y2, E2, Z3, Z4 = '1,0,1', '4,1,0,1', '1,2', '0,0,0', '0,0,0,0'
OK = (1, 3, 4, 1, 0, 1, 0, 0, 0, 8, X2, Y2, E2, Z3, Z4)


def _with(**kw):
    names = ('n_ranks', 'res_nx', 'res_ny', 'res_sets', 'first', 'n_sets', 'mode', 'ref_c', 'k', 'rd', 'x2', 'y2', 'e2', 'ra', 'rb')
    args = dict(zip(names, OK))
    args.update(kw)
    return tuple(args[n] for n in names)


REFUSALS = [
    (_with(n_ranks=2), -1, 'ml_fields_zones: this context belongs to a communicator of 2 ranks'),
    (_with(res_nx=0, res_ny=0, res_sets=0), -2, 'no resident field set'),
    (_with(res_nx=4), -1, 'the axes have 3 x 4 samples, the resident field sets 4 x 4'),
    (_with(res_ny=5), -1, 'the axes have 3 x 4 samples, the resident field sets 3 x 5'),
    (_with(n_sets=0), -1, 'a pass takes 1 to 3 field sets, got 0'),
    (_with(n_sets=4, res_sets=4), -1, 'a pass takes 1 to 3 field sets, got 4'),
    (_with(first=1), -1, 'field sets 1 ... 1 asked for, 1 resident'),
    (_with(first=-1), -1, 'field sets -1 ... -1 asked for, 1 resident'),
    (_with(n_sets=3, res_sets=2), -1, 'field sets 0 ... 2 asked for, 2 resident'),
    (_with(e2=','.join(['1'] * 4097)), -1, '4097 edges: 1 to 4096 are taken'),
    (_with(e2='null'), -1, '0 edges: 1 to 4096 are taken'),
    (_with(e2='1,-2'), -1, 'e2[1] = -2: a squared edge must be finite and >= 0'),
    (_with(e2='nan'), -1, 'e2[0] = nan'),
    (_with(e2='1,inf'), -1, 'e2[1] = inf'),
    (_with(e2='1,3,2'), -1, 'the edges must not decrease: e2[2] = 2 < e2[1] = 3'),
    (_with(x2='1,-1,1'), -1, 'x2[1] = -1: a squared distance must be finite and >= 0'),
    (_with(y2='4,1,nan,1'), -1, 'y2[2] = nan: a squared distance'),
    (_with(y2='4,1,2,1'), -1, 'y2 must fall to its minimum y2[1] = 1 and rise again (a y axis in ascending or descending order): '
                              'y2[3] = 1 follows y2[2] = 2'),
    (_with(y2='1,4,0,1'), -1, 'y2[1] = 4 follows y2[0] = 1'),
    (_with(mode=2), -1, 'ref_mode 2: 0 for a plane wave or 1 for a focus'),
    (_with(ra='0,inf,0'), -1, 'ra[1] = inf: a reference phase must be finite'),
    (_with(mode=1, ref_c=1e-3, k=1e7, rb='0,0,-1,0'), -1, 'rb[2] = -1: a squared distance to the focus must be finite and >= 0'),
    (_with(mode=1, ref_c=0, k=1e7), -1, 'ref_c = 0: the focus lies at a finite distance zf != 0'),
    (_with(mode=1, ref_c='nan', k=1e7), -1, 'ref_c = nan'),
    (_with(mode=1, ref_c=1e-3, k=0), -1, 'k = 0: the wave number must be finite and > 0'),
    (_with(mode=1, ref_c=-2e-3, k=1e7, ra='1e6,0,0'), -1, 'the reference phase reaches 1e+10 rad on this grid: the phase arithmetic covers up to 1e+09'),
    (_with(ra='6e8,0,-7e8', rb='6e8,0,0,-4e8'), -1, 'the reference phase reaches 1.2e+09 rad'),
    (_with(rd=7), -1, 'record_doubles = 7: a record has 8 doubles'),
    (_with(x2='null', ra='null', res_nx=0, res_ny=0), -1, 'the axes have 0 x 4 samples: at least one each'),
    (_with(ra='null'), -1, 'NULL argument'),
    # an argument error is named before the state
    (_with(res_nx=0, res_ny=0, res_sets=0, n_sets=5), -1, 'a pass takes 1 to 3 field sets, got 5'),
]
ACCEPTED = [(OK, 0.0), (_with(rd=12), 0.0), (_with(n_sets=3, res_sets=3), 0.0), (_with(first=2, n_sets=1, res_sets=3), 0.0),
            (_with(e2='0'), 0.0), (_with(e2='1,1,2'), 0.0), (_with(y2='0,1,4,9'), 0.0), (_with(y2='9,4,1,1'), 0.0),
            (_with(ra='5e8,0,-5e8', rb='5e8,0,0,-5e8'), 1e9), (_with(mode=1, ref_c=-3.0, k=2.0, ra='16,0,0'), 10.0),
            (_with(e2=','.join(str(v) for v in range(4096))), 0.0)]


def test_refusals_name_the_numbers(tool):
    for args, code, said in REFUSALS:
        out = tool('check', *args)
        assert out.startswith('refused=%d\n' % code) and said in out, (out, said)
    for args, phase in ACCEPTED:
        assert tool('check', *args) == 'ok=1 phase=%.17g\n' % phase, args


def test_under_sanitizers(tool):
    """the same program under the address and undefined-behaviour sanitizers: same output, nothing reported"""
    san = 'fields_zones_plan_san'
    assert tool(*_flat(SHAPES), exe=san) == tool(*_flat(SHAPES)) and tool('layout', exe=san) == tool('layout')
    assert tool('vertex', '4,1,1,2', exe=san) == 'jv=1\n'
    for args, _code, _said in REFUSALS:
        assert tool('check', *args, exe=san) == tool('check', *args)
    for args, phase in ACCEPTED:
        assert tool('check', *args, exe=san) == 'ok=1 phase=%.17g\n' % phase


# ---- postprocess.zone_metrics against the yardstick ---------------------------------------------
@pytest.mark.parametrize('case', ref.cases(), ids=lambda c: c[0].replace(' ', '_'))
def test_zone_metrics_against_the_yardstick(case):
    from metalens_amd import postprocess
    name, x, y, wl, ng, edges, centre, reference = case
    F = ref.seeded_fields(2, x.size, y.size, seed=x.size * 1000 + y.size)
    got = postprocess.zone_metrics(F[:, 0], F[:, 1], F[:, 2], F[:, 3], x, y, wl, ng, edges, centre, reference)
    want = ref.exact(F, x, y, wl, ng, edges, centre, reference)
    assert want['n'].sum() > 0 and want['outside'] > 0
    ref.hold('twin ' + name, got, want)
    # one set given as 2-D arrays: the same numbers with a leading axis of one
    one = postprocess.zone_metrics(F[1, 0], F[1, 1], F[1, 2], F[1, 3], x, y, wl, ng, edges, centre, reference)
    for key in ('P', 'I', 'overlap'):
        assert one[key].shape[0] == 1 and np.array_equal(one[key][0], got[key][1]), key


def test_zone_metrics_edges_and_empty_zones():
    from metalens_amd import postprocess
    # integer axes: the samples (3, 4) and (5, 12) lie exactly on the edges 5 and 13 and belong to the inner zone
    x = y = np.arange(16.0)
    F = ref.seeded_fields(1, 16, 16, seed=3)
    got = postprocess.zone_metrics(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, y, 4.0, 1.0, [5.0, 13.0])
    zone = ref.membership(x, y, [5.0, 13.0], (0.0, 0.0))
    assert zone[3, 4] == 0 and zone[4, 3] == 0 and zone[5, 0] == 0 and zone[5, 12] == 1 and zone[12, 5] == 1 and zone[0, 13] == 1
    assert zone[4, 4] == 1 and zone[5, 13] == 2
    assert got['samples'].tolist() == [int((zone == 0).sum()), int((zone == 1).sum())] and got['outside'] == int((zone == 2).sum())
    # zones closer than the pitch hold nothing: zero sums, NaN coherence, phase 0
    got = postprocess.zone_metrics(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, y, 4.0, 1.0, [2.5, 2.6, 2.7, 6.0])
    assert got['samples'][1:3].tolist() == [0, 0] and (got['P'][0, 1:3] == 0).all() and np.isnan(got['coherence'][0, 1:3]).all()
    assert (got['phase'][0, 1:3] == 0).all() and not np.isnan(got['coherence'][0, [0, 3]]).any()
    with pytest.raises(ValueError, match=r'Hx has shape \(16, 15\), the axes give \(16, 16\)'):
        postprocess.zone_metrics(F[0, 0], F[0, 1], F[0, 2, :, :15], F[0, 3], x, y, 4.0, 1.0, [5.0])
    # a field that follows the reference: coherence 1, piston 0
    k = ref.wave_number(4.0, 1.0)
    w = np.exp(1j * k * (0.3 * x[:, None] - 0.2 * y[None, :]))
    got = postprocess.zone_metrics(w, 2 * w * np.exp(0.5j), w, w, x, y, 4.0, 1.0, [5.0, 13.0], reference=('plane', 0.3, -0.2))
    assert np.allclose(got['coherence'], 1.0, rtol=0, atol=1e-13) and np.allclose(got['phase'][0, :, 0], 0.0, atol=1e-13)
    assert np.allclose(got['phase'][0, :, 1], 0.5, atol=1e-13)


def test_zone_edges_reproduce_the_oracles_rings():
    """on the 30 um, NA 0.5 lens at 240^2 samples the zone of every sample is the oracle's ring + 1, 0 in the centre"""
    import math

    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    from oracle import nearfield_oracle
    wl = 580e-9
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design, radius=30e-6,
                               numerical_aperture=0.5, wavelength=wl, switch_angle=8 * math.pi / 180, num_gratings=8, num_entries=8)
    S = lens['lens_periphery_summary']
    edges = ma.zone_edges(S)
    assert edges.shape == (len(S['r_min_list']) + 1,) and edges[-1] == S['r_max_list'][-1] and (np.diff(edges) > 0).all()
    R = edges[-1]
    x = np.linspace(-R, R, 240)
    seen = {}
    nearfield_oracle.build_nearfield(0.0, 0.0, -lens['source_distance'], 'x', wl, S, lens['lens_center_summary'], lens['hexgridset'],
                                     x_pts=x, y_pts=x, decisions=seen)
    K = edges.size
    want = np.where(seen['in_center'], 0, np.where(seen['ring'] >= 0, seen['ring'] + 1, K))
    got = ref.membership(x, x, edges, (0.0, 0.0))
    assert got.shape == (240, 240) and np.array_equal(got, want)
    assert (np.bincount(got.ravel(), minlength=K + 1) > 0).all()           # the centre, every ring and the outside are met
    from metalens_amd import postprocess
    z = postprocess._check_zones(x, x, wl, 1.46, edges)
    assert np.array_equal(np.searchsorted(z['e2'], z['x2'][:, None] + z['y2'][None, :], side='left'), want)


# ---- the Python argument checks -------------------------------------------------------------
AX = np.linspace(-1e-5, 1e-5, 9)
BAD = [
    (dict(xp_list=[[0.0, 1.0]]), 'xp_list must be a sequence of at least one number'),
    (dict(yp_list=[]), 'yp_list must be a sequence of at least one number'),
    (dict(xp_list='wide'), 'xp_list must be a sequence of numbers'),
    (dict(yp_list=[0.0, np.nan]), r'yp_list must be finite: yp_list\[1\] = nan'),
    (dict(yp_list=[0.0, 2.0, 1.0]), r'yp_list must be in ascending or descending order .* yp_list\[2\] = 1 follows yp_list\[1\] = 2'),
    (dict(wavelength=0.0), 'wavelength and n_glass must be finite and > 0'),
    (dict(n_glass=np.inf), 'wavelength and n_glass must be finite and > 0'),
    (dict(edges=[]), 'zones take 1 to 4096 edges, got 0'),
    (dict(edges=np.arange(4097.0)), 'zones take 1 to 4096 edges, got 4097'),
    (dict(edges=[[1.0, 2.0]]), 'edges must be a sequence of numbers'),
    (dict(edges='rings'), 'edges must be a sequence of numbers'),
    (dict(edges=[1e-6, -2e-6]), r'an edge must be finite and >= 0: edges\[1\] = -2e-06'),
    (dict(edges=[np.nan]), r'edges\[0\] = nan'),
    (dict(edges=[1e-6, 3e-6, 2e-6]), r'the edges must not decrease: edges\[2\] = 2e-06 < edges\[1\] = 3e-06'),
    (dict(centre=(0.0,)), r'centre must be one \(xc, yc\)'),
    (dict(centre='peak'), r'centre must be one \(xc, yc\)'),
    (dict(centre=(0.0, np.inf)), 'a centre must be finite'),
    (dict(reference=('sphere', 0.0, 0.0)), r"reference must be \('plane', ux, uy\) or \('focus', xf, yf, zf\)"),
    (dict(reference=('plane', 0.0)), r"reference must be \('plane', ux, uy\)"),
    (dict(reference=('focus', 0.0, 0.0)), r"reference must be \('plane', ux, uy\)"),
    (dict(reference=None), r"reference must be \('plane', ux, uy\)"),
    (dict(reference=('plane', 0.8, 0.7)), r'a plane-wave reference needs ux\^2 \+ uy\^2 <= 1, got \(0.8, 0.7\)'),
    (dict(reference=('plane', np.nan, 0.0)), 'a plane-wave reference needs'),
    (dict(reference=('focus', 0.0, 0.0, 0.0)), r'a focus reference needs a finite focus \(xf, yf, zf\) with zf != 0, got \(0, 0, 0\)'),
    (dict(reference=('focus', 0.0, np.inf, 1e-3)), 'a focus reference needs a finite focus'),
]


def test_argument_errors_come_before_any_device_call(no_device):
    import metalens_amd as ma
    from metalens_amd import postprocess
    base = dict(xp_list=AX, yp_list=AX, wavelength=580e-9, n_glass=1.46, edges=[2e-6, 5e-6])
    F = np.zeros((9, 9), dtype=complex)
    for bad, said in BAD:
        kw = dict(base, **bad)
        with pytest.raises(ValueError, match=said):
            ma.ApertureZones(**kw)
        with pytest.raises(ValueError, match=said):
            ma.aperture_zones(F, F, F, F, **kw)
        with pytest.raises(ValueError, match=said):
            postprocess.zone_metrics(F, F, F, F, kw.pop('xp_list'), kw.pop('yp_list'), **kw)
    for first, n, said in ((-1, None, 'first must be a field set index >= 0'), (0, 0, 'takes 1 to 3 field sets per call, got n = 0'),
                           (0, 4, 'got n = 4'), (0.5, 1, 'first must be a field set index')):
        with pytest.raises(ValueError, match=said):
            ma.aperture_zones(None, None, None, None, first=first, n=n, **base)
        with pytest.raises(ValueError, match=said):
            ma.ApertureZones.records(object(), first, n)            # (what analyse() calls first)
    # what the checks hand on
    z = postprocess._check_zones(AX, AX[::-1], 580e-9, 1.46, [2e-6, 5e-6], (1e-6, -2e-6), ('focus', 1e-6, 0.0, -3e-5))
    assert np.array_equal(z['x2'], (AX - 1e-6) ** 2) and np.array_equal(z['y2'], (AX[::-1] + 2e-6) ** 2)
    assert z['e2'].tolist() == [2e-6 * 2e-6, 5e-6 * 5e-6] and z['mode'] == 1 and z['ref_c'] == -3e-5 and z['k'] == 2 * np.pi * 1.46 / 580e-9
    assert np.array_equal(z['ra'], (AX - 1e-6) ** 2) and np.array_equal(z['rb'], AX[::-1] ** 2) and z['dA'] == (AX[1] - AX[0]) ** 2
    z = postprocess._check_zones([0.5], AX, 580e-9, 1.46, [1.0], reference=('plane', 0.6, -0.8))
    assert z['mode'] == 0 and np.array_equal(z['ra'], z['k'] * (0.6 * np.array([0.5]))) and np.array_equal(z['rb'], z['k'] * (-0.8 * AX))
    assert z['dA'] == AX[1] - AX[0]


def test_entry_in_header_binding_and_export_map():
    from metalens_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    decl = re.search(r'int\s+ml_fields_zones\s*\(([^)]*)\)', code)
    assert decl and len(decl.group(1).split(',')) == 16 and 'ml_fields_zones' in _lib.SYMBOLS
    lib = _lib.load()
    assert len(lib.ml_fields_zones.argtypes) == 16
    exports = open(os.path.join(ROOT, 'metalens_amd', 'csrc', 'exports.map')).read()
    assert re.search(r'global:\s*ml_\*;', exports) and 'ml_fields_zones' in exports
    import makefile_deps
    assert makefile_deps.header_is_prerequisite('fields_zones.h', 'fields_zones')   # (the unit is built, the header rebuilds it)
    rec = np.zeros(8)
    assert lib.ml_fields_zones(None, 0, 1, None, 0, None, 0, None, 0, 0, None, None, 0.0, 0.0, _lib.dptr(rec), 8) != 0      # no context
    assert b'NULL argument' in lib.ml_last_error()
