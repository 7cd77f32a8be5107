"""The per-zone contributions to the field behind the aperture without a GPU: the plan arithmetic and the argument checks
of csrc/fields_zone_fields.h through tools/fields_zone_fields_plan.cpp - constants and scratch against the Python side,
every refusal with its wording, once more under the address and undefined-behaviour sanitizers -,
``postprocess.zone_fields`` against the long-double yardstick (tests/zone_fields_ref.py) within ``8 e_ref``, its closure
against the direct sum of the unmasked fields, the derived quantities (``gradient``, ``phase``, ``aligned``,
``AperturePupil.from_zone_fields``), every ``ValueError`` of the Python layer before any device call, and the entry's presence
in header, binding and export map."""
import os
import re
import subprocess

import numpy as np
import pytest

import propagate_ref
import zone_fields_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL, NG = 580e-9, 1.46
P = WL / 2.2


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('zone_fields_plan')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'fields_zone_fields_plan',
                           out + 'fields_zone_fields_plan_san'])

    def run(*args, exe='fields_zone_fields_plan'):
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
SHAPES = [(1, 1, 1, 1), (3, 64, 2, 0), (3, 65, 7, 1), (64, 70, 4096, 1), (33, 300, 300, 0), (4096, 4096, 198, 1), (8192, 8192, 4096, 1)]


def test_plan_of_the_shapes(tool):
    from metalens_amd import postprocess as pp
    lines = tool(*[v for s in SHAPES for v in s]).splitlines()
    assert len(lines) == len(SHAPES)
    for (nx, ny, K, h), line in zip(SHAPES, lines):
        f = _facts(line)
        cap, rd = min(ny, 2 * (K + 1)), 1 + pp.ZONE_FIELDS_TG * (12 if h else 6)
        assert f == dict(nx=nx, ny=ny, k=K, h=h, blocks=-(-ny // 64), capacity=cap, run_doubles=rd, scratch=nx * cap * rd * 8 + nx * 8,
                         bound=nx * min(ny + 2, 2 * K + 4) * rd * 8), line
        assert f['scratch'] <= f['bound']
    assert _facts(lines[-2])['scratch'] == 4096 * 398 * 49 * 8 + 4096 * 8          # the benchmark's lens: 0.64 GB


def test_constants_agree(tool):
    from metalens_amd import postprocess as pp, zones
    f = _facts(tool('layout'))
    assert f == dict(targets_max=pp.ZONE_FIELDS_TARGETS_MAX, tg=pp.ZONE_FIELDS_TG, e_doubles=6, eh_doubles=12, edges_max=pp.ZONES_EDGES_MAX,
                     sets_max=zones.SETS_MAX, block=64)
    assert f['targets_max'] == 64
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    assert re.search(r'#define\s+ML_ZONE_FIELDS_TARGETS_MAX\s+64\b', text)
    tg = pp.ZONE_FIELDS_TG
    assert tool('groups', 1) == 'groups=1\n' and tool('groups', tg) == 'groups=1\n' and tool('groups', tg + 1) == 'groups=2\n'
    assert tool('groups', 64) == 'groups=%d\n' % -(-64 // tg)


# n_ranks res_nx res_ny res_sets first n_sets dxp dyp wavelength n_glass Z0 x2 y2 e2 tx ty tz -> code, message
X2, Y2, E2, TX, TY, TZ = '1,0,1', '4,1,0,1', '1,2', '0,1', '0,-1', '1,2'
OK = (1, 3, 4, 1, 0, 1, 1.0, 1.0, 4.0, 1.0, 377.0, X2, Y2, E2, TX, TY, TZ)
NAMES = ('n_ranks', 'res_nx', 'res_ny', 'res_sets', 'first', 'n_sets', 'dxp', 'dyp', 'wl', 'ng', 'Z0', 'x2', 'y2', 'e2', 'tx', 'ty', 'tz')


def _with(**kw):
    args = dict(zip(NAMES, OK))
    args.update(kw)
    return tuple(args[n] for n in NAMES)


T65 = ','.join(['1'] * 65)
REFUSALS = [
    (_with(n_ranks=2), -1, 'ml_fields_zone_fields: this context belongs to a communicator of 2 ranks'),
    (_with(res_nx=0, res_ny=0, res_sets=0), -2, 'no resident field set'),
    (_with(res_nx=4), -1, 'ml_fields_zone_fields: the axes have 3 x 4 samples, the resident field sets 4 x 4'),
    (_with(n_sets=0), -1, 'a pass takes 1 to 3 field sets, got 0'),
    (_with(n_sets=4, res_sets=4), -1, 'a pass takes 1 to 3 field sets, got 4'),
    (_with(first=1), -1, 'field sets 1 ... 1 asked for, 1 resident'),
    (_with(e2=','.join(['1'] * 4097)), -1, '4097 edges: 1 to 4096 are taken'),
    (_with(e2='null'), -1, '0 edges: 1 to 4096 are taken'),
    (_with(e2='1,-2'), -1, 'e2[1] = -2: a squared edge must be finite and >= 0'),
    (_with(e2='1,3,2'), -1, 'the edges must not decrease: e2[2] = 2 < e2[1] = 3'),
    (_with(x2='1,-1,1'), -1, 'x2[1] = -1: a squared distance must be finite and >= 0'),
    (_with(y2='4,1,2,1'), -1, 'y2 must fall to its minimum y2[1] = 1 and rise again'),
    (_with(tx=T65, ty=T65, tz=T65), -1, '65 targets: 1 to 64 are taken'),
    (_with(tx='null', ty='null', tz='null'), -1, '0 targets: 1 to 64 are taken'),
    (_with(ty='null'), -1, 'NULL argument'),
    (_with(tx='0,inf'), -1, "tx[1] = inf: a target's coordinate must be finite"),
    (_with(ty='nan,0'), -1, "ty[0] = nan: a target's coordinate must be finite"),
    (_with(tz='1,inf'), -1, "tz[1] = inf: a target's coordinate must be finite"),
    (_with(tz='1,0'), -1, 'tz[1] = 0: a target lies behind the aperture, z > 0'),
    (_with(tz='-2,1'), -1, 'tz[0] = -2: a target lies behind the aperture, z > 0'),
    (_with(dxp=0), -1, 'dxp = 0: must be finite and > 0'),
    (_with(dyp='nan'), -1, 'dyp = nan: must be finite and > 0'),
    (_with(wl=-1), -1, 'wavelength = -1: must be finite and > 0'),
    (_with(ng='inf'), -1, 'n_glass = inf: must be finite and > 0'),
    (_with(Z0=0), -1, 'Z0 = 0: must be finite and > 0'),
    # an argument error is named before the state, the zones before the targets' values
    (_with(res_nx=0, res_ny=0, res_sets=0, n_sets=5), -1, 'a pass takes 1 to 3 field sets, got 5'),
    (_with(e2='1,-2', tz='0,0'), -1, 'e2[1] = -2'),
]
ACCEPTED = [OK, _with(n_sets=3, res_sets=3), _with(first=2, res_sets=3), _with(e2='0'), _with(y2='0,1,4,9'),
            _with(tx=','.join(['1'] * 64), ty=','.join(['1'] * 64), tz=','.join(['1'] * 64)), _with(tz='1e-300,1')]


def test_refusals_name_the_numbers(tool):
    for args, code, said in REFUSALS:
        out = tool('check', *args)
        assert out.startswith('refused=%d\n' % code) and said in out, (out, said)
    for args in ACCEPTED:
        assert tool('check', *args) == 'ok=1\n', args


def test_under_sanitizers(tool):
    """the same program under the address and undefined-behaviour sanitizers: same output, nothing reported"""
    san = 'fields_zone_fields_plan_san'
    flat = [v for s in SHAPES for v in s]
    assert tool(*flat, exe=san) == tool(*flat) and tool('layout', exe=san) == tool('layout')
    for args, _code, _said in REFUSALS:
        assert tool('check', *args, exe=san) == tool('check', *args)
    for args in ACCEPTED:
        assert tool('check', *args, exe=san) == 'ok=1\n'


# ---- postprocess.zone_fields against the yardstick ---------------------------------------------
def _points(x, y, centre):
    """2 um behind the aperture inside its footprint, a focus-like distance on the centre's axis, well outside laterally"""
    return np.array([[x[len(x) // 3], y[len(y) // 2] + 0.3 * P, 2e-6], [centre[0], centre[1], 25e-6],
                     [x[-1] + 40e-6, y[0] - 15e-6, 12e-6]])


CASES = {
    '40x37': ((np.arange(40) - 19.5) * P, (np.arange(37) - 18) * P, np.linspace(0.8e-6, 5.5e-6, 9), (0.0, 0.0)),
    '22x70 tight': ((np.arange(22) - 8.3) * P, (np.arange(70) - 40.7) * P,
                    np.sort(np.concatenate([np.linspace(0.5e-6, 9e-6, 12), 3e-6 + np.arange(5) * 0.0004e-6])), (0.37e-6, -1.21e-6)),
    '9x80 off grid': ((np.arange(9) + 20.0) * P, (np.arange(80) + 7.4) * P, np.linspace(3e-6, 20e-6, 30), (0.0, 0.0)),
}


@pytest.fixture(scope='module')
def solved():
    """per case: fields, points, the yardstick and the twin's dict - computed once"""
    from metalens_amd import postprocess
    out = {}
    for name, (x, y, edges, centre) in CASES.items():
        F = ref.seeded_fields(2, x.size, y.size, seed=x.size * 1000 + y.size)
        pts = _points(x, y, centre)
        want = ref.yardstick(F, x, y, WL, NG, edges, centre, pts)
        got = postprocess.zone_fields(F[:, 0], F[:, 1], F[:, 2], F[:, 3], x, y, WL, NG, edges, pts, centre=centre, Z0=propagate_ref.Z0_SI)
        out[name] = (F, pts, want, got)
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_twin_against_the_yardstick(solved, name):
    from metalens_amd import postprocess
    x, y, edges, centre = CASES[name]
    F, pts, want, got = solved[name]
    K = len(edges)
    assert got['E'].shape == (2, K, 3, 3) and got['H'].shape == (2, K, 3, 3) and got['outside_E'].shape == (2, 3, 3)
    assert got['samples'].shape == (K,) and got['samples'].dtype == np.int64 and want['n'][-1] > 0 and want['n'][:-1].sum() > 0
    ref.hold('twin ' + name, got, want)
    if name == '22x70 tight':
        assert (want['n'] == 0).any()
    # closure: the slots added up against the direct sum of the unmasked fields, both within 8 e_ref of the truth
    for m in range(2):
        E, H = propagate_ref.direct_sum(F[m, 0], F[m, 1], F[m, 2], F[m, 3], x, y, WL, NG, pts, real=np.longdouble)
        for f, whole in (('E', E), ('H', H)):
            err = np.abs(got['total_' + f][m].astype(np.clongdouble) - whole).max() / np.abs(want[f]).max()
            assert err <= 2 * ref.MARGIN * want['e_ref_' + f], (name, f, float(err))
    # one set given as 2-D arrays, E only, in long double: the same definition
    one = postprocess.zone_fields(F[1, 0], F[1, 1], F[1, 2], F[1, 3], x, y, WL, NG, edges, pts, centre=centre, want_h=False,
                                  Z0=propagate_ref.Z0_SI)
    assert 'H' not in one and np.array_equal(one['E'][0], got['E'][1])
    ld = postprocess.zone_fields(F[1, 0], F[1, 1], F[1, 2], F[1, 3], x, y, WL, NG, edges, pts[:1], centre=centre, Z0=propagate_ref.Z0_SI,
                                 real=np.longdouble)
    assert ld['E'].dtype == np.clongdouble
    assert propagate_ref.max_error(ref.slots(ld)[0, :, :, 0], want['E'][1, :, :, 0]) <= 1e-3 * want['e_ref_E'] + 1e-18


def test_the_yardstick_is_direct_sum_on_the_masked_fields():
    """tests/zone_fields_ref.py forms a target's summands once and masks them: bit for bit ``propagate_ref.direct_sum`` on the
    fields masked to each slot, in both precisions - with an axis of one sample and its ``pitch`` too"""
    x, y, edges, centre = CASES['22x70 tight']
    F = ref.seeded_fields(2, x.size, y.size, seed=9)
    pts = _points(x, y, centre)
    for xx, FF, pitch in ((x, F, None), (x[:1], F[:, :, :1], (P, P))):
        for real in (np.float64, np.longdouble):
            fast = ref.exact(FF, xx, y, WL, NG, edges, centre, pts, real, pitch)
            slow = ref.exact(FF, xx, y, WL, NG, edges, centre, pts, real, pitch, by_direct_sum=True)
            assert fast[0].dtype == slow[0].dtype and np.abs(slow[0]).max() > 0
            assert np.array_equal(fast[0], slow[0]) and np.array_equal(fast[1], slow[1])


# ---- the derived quantities ------------------------------------------------------------------
def test_phase_aligned_and_polarisation(solved):
    from metalens_amd import postprocess
    name = '22x70 tight'
    x, y, edges, centre = CASES[name]
    F, pts, want, got = solved[name]
    tE = got['total_E']
    # the default polarisation is the unit vector along the total field: its projection is |E|, the phases are against it
    p = got['polarisation']
    assert p.shape == tE.shape and np.allclose((np.abs(p) ** 2).sum(axis=1), 1.0, rtol=0, atol=1e-14)
    whole = got['projection'].sum(axis=1) + got['outside_projection']
    norm = np.sqrt((np.abs(tE) ** 2).sum(axis=1))
    assert np.allclose(whole.real, norm, rtol=1e-12, atol=0) and np.allclose(whole.imag, 0, rtol=0, atol=1e-12 * norm.max())
    proj = (np.conj(p)[:, None] * got['E']).sum(axis=2)
    assert np.array_equal(got['projection'], proj)
    empty = got['samples'] == 0
    assert empty.any() and np.isnan(got['phase'][:, empty]).all() and not np.isnan(got['phase'][:, ~empty]).any()
    assert np.array_equal(got['phase'][:, ~empty], np.angle(proj)[:, ~empty])
    # aligned: the sum of the moduli, the ceiling of |p^H sum_z g_z E_z| over unit factors - reached by g_z = exp(-i phase_z)
    assert np.array_equal(got['aligned'], np.abs(proj).sum(axis=1))
    g = np.where(np.isnan(got['phase']), 1.0, np.exp(-1j * np.nan_to_num(got['phase'])))
    reached = np.abs((g * proj).sum(axis=1))
    assert np.allclose(reached, got['aligned'], rtol=1e-13, atol=0) and (np.abs(proj.sum(axis=1)) <= got['aligned'] * (1 + 1e-14)).all()
    # a given polarisation: normalised, the same for every set and target
    fixed = postprocess.zone_fields(F[:, 0], F[:, 1], F[:, 2], F[:, 3], x, y, WL, NG, edges, pts, centre=centre, Z0=propagate_ref.Z0_SI,
                                    polarisation=(3.0, 0.0, 4.0j))
    assert np.allclose(fixed['polarisation'][1, :, 2], [0.6, 0.0, 0.8j], rtol=0, atol=4 * 2.0 ** -53)   # (a square root and a division)
    assert np.allclose(fixed['projection'], 0.6 * got['E'][:, :, 0] - 0.8j * got['E'][:, :, 2], rtol=1e-14, atol=0)
    assert np.array_equal(fixed['E'], got['E']) and np.array_equal(fixed['gradient'], got['gradient'])


def test_gradient_against_a_finite_difference(solved):
    """``gradient[s, z, t]`` is d|E(t)|^2 / d phi_z for a phase phi_z added to zone z.  With zone z's fields multiplied by
    exp(+-i h) the twin gives I(+-h); I(phi) = |E - E_z + e^{i phi} E_z|^2 = const + 2 Re(e^{i phi} conj(E - E_z) . E_z) is a
    sinusoid of amplitude A = 2 |conj(E - E_z) . E_z|, so the central difference (I(h) - I(-h)) / (2 h) = I'(0) sin(h) / h is off
    by at most its truncation term A h^2 / 6.  To that comes the rounding of the two intensities: every slot of the twin is
    within 8 e_ref max|E_z| of the truth (test_twin_against_the_yardstick), the K + 1 slots of a total add up to dE = (K + 1) 8
    e_ref max|E_z| per component, an intensity is off by at most 2 sum_d |E_d| dE <= 6 max|E_d| dE, and the difference of two
    of them divided by 2 h by 6 max|E_d| dE / h.  Nothing here comes from the gradient under test."""
    from metalens_amd import postprocess
    name = '40x37'
    x, y, edges, centre = CASES[name]
    F, pts, want, got = solved[name]
    zone = ref.membership(x, y, edges, centre)
    h = 1e-6
    scale = float(np.abs(want['E']).max())
    for z in (0, 4, len(edges) - 1):
        I = []
        for s in (+1, -1):
            Fz = np.where(zone == z, F[0] * np.exp(1j * s * h), F[0])
            d = postprocess.zone_fields(Fz[0], Fz[1], Fz[2], Fz[3], x, y, WL, NG, edges, pts, centre=centre, want_h=False,
                                        Z0=propagate_ref.Z0_SI)
            I.append((np.abs(d['total_E'][0]) ** 2).sum(axis=0))
        fd = (I[0] - I[1]) / (2 * h)
        Ez, E = got['E'][0, z], got['total_E'][0]
        A = 2 * np.abs((np.conj(E - Ez) * Ez).sum(axis=0))
        dE = (len(edges) + 1) * ref.MARGIN * want['e_ref_E'] * scale
        tol = A * h * h / 6 + 6 * np.abs(E).max() * dE / h
        assert (np.abs(fd - got['gradient'][0, z]) <= tol).all(), (z, fd, got['gradient'][0, z], tol)
        assert (np.abs(got['gradient'][0, z]) > 100 * tol).any(), z            # (the check resolves the gradient)
    assert np.array_equal(got['gradient'], -2 * (np.conj(got['total_E'])[:, None] * got['E']).sum(axis=2).imag)


class _Azf:
    """what from_zone_fields reads of an ApertureZoneFields"""
    def __init__(self, x, y, edges, centre, T):
        self._x, self._y, self._edges, self._centre = x, y, np.asarray(edges, dtype=float), centre
        self.n_zones, self.points, self.ctx = len(edges), np.zeros((T, 3)), 'a context'


def test_from_zone_fields(solved):
    import metalens_amd as ma
    name = '22x70 tight'
    x, y, edges, centre = CASES[name]
    F, pts, want, got = solved[name]
    azf = _Azf(x, y, edges, centre, len(pts))
    seen = {}

    class Pupil(ma.AperturePupil):
        def __init__(self, xp, yp, radius, **kw):
            seen.update(kw, x=xp, y=yp, radius=radius)
    Pupil.from_zone_fields(azf, got, set=1, target=2)
    g, ph = seen['zone_factors'], got['phase'][1, :, 2]
    empty = np.isnan(ph)
    assert empty.any() and (g[empty] == 1).all() and np.allclose(np.abs(g[~empty]), 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(g[~empty], np.exp(-1j * ph[~empty]))
    assert seen['radius'] == edges[-1] and seen['centre'] == centre and seen['ctx'] == 'a context' and np.array_equal(seen['edges'], edges)
    assert seen['x'] is x and seen['y'] is y
    Pupil.from_zone_fields(azf, got, radius=3e-6, stop=False, ctx='another')
    assert seen['radius'] == 3e-6 and seen['stop'] is False and seen['ctx'] == 'another'
    assert np.array_equal(seen['zone_factors'][~empty], np.exp(-1j * got['phase'][0, :, 0][~empty]))
    with pytest.raises(ValueError, match=r'result must be the dict of analyse\(\) of this ApertureZoneFields: phase has shape'):
        Pupil.from_zone_fields(_Azf(x, y, edges[:-1], centre, len(pts)), got)
    with pytest.raises(ValueError, match='for 17 zones and 2 points'):
        Pupil.from_zone_fields(_Azf(x, y, edges, centre, 2), got)
    # the factors applied on the host: every zone's projection turns onto the positive real axis
    from metalens_amd import postprocess
    p = got['polarisation'][1, :, 2]
    out = postprocess.apply_pupil_host(F[1, 0], F[1, 1], F[1, 2], F[1, 3], x, y, edges[-1], centre=centre, edges=edges, zone_factors=g)
    after = postprocess.zone_fields(*out, x, y, WL, NG, edges, pts, centre=centre, Z0=propagate_ref.Z0_SI, polarisation=p)
    pr = after['projection'][0, :, 2]
    assert np.allclose(pr[~empty].imag, 0, rtol=0, atol=1e-12 * np.abs(pr).max()) and (pr[~empty].real > 0).all()
    assert after['outside'] == got['outside'] and (after['outside_E'] == 0).all()
    assert np.allclose(np.abs(pr.sum()), got['aligned'][1, 2], rtol=1e-12, atol=0)


# ---- the Python argument checks -------------------------------------------------------------
AX = np.linspace(-1e-5, 1e-5, 9)
PTS = [[0.0, 0.0, 1e-5]]
BAD = [
    (dict(xp_list=[[0.0, 1.0]]), 'xp_list must be a sequence of at least one number'),
    (dict(yp_list=[0.0, np.nan]), r'yp_list must be finite: yp_list\[1\] = nan'),
    (dict(yp_list=AX[::-1]), r'yp_list must ascend: yp_list\[1\] = .* follows yp_list\[0\]'),
    (dict(xp_list=[0.0, 1e-6, 3e-6]), 'xp_list must be uniform: its steps run from'),
    (dict(xp_list=[0.0]), r'xp_list has one sample and no step of its own: pitch=\(dx, dy\) must give one > 0'),
    (dict(xp_list=[0.0], pitch=(0.0, 1e-6)), r'pitch=\(dx, dy\) must give finite steps > 0, got 0.0 for xp_list'),
    (dict(pitch=3.0), r'pitch must be None or \(dx, dy\)'),
    (dict(wavelength=0.0), 'wavelength and n_glass must be finite and > 0'),
    (dict(edges=[]), 'zones take 1 to 4096 edges, got 0'),
    (dict(edges=[1e-6, 3e-6, 2e-6]), r'the edges must not decrease: edges\[2\] = 2e-06 < edges\[1\] = 3e-06'),
    (dict(centre=(0.0,)), r'centre must be one \(xc, yc\)'),
    (dict(points=[0.0, 0.0, 1.0]), r'points must be an array of shape \(T, 3\), got shape \(3,\)'),
    (dict(points='focus'), r'points must be an array of shape \(T, 3\)'),
    (dict(points=np.zeros((0, 3))), 'zone fields take 1 to 64 points, got 0'),
    (dict(points=np.ones((65, 3))), 'zone fields take 1 to 64 points, got 65'),
    (dict(points=[[0.0, np.inf, 1.0]]), r'a point must be finite: points\[0\]'),
    (dict(points=[[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]), r'every point needs z > 0 .*: points\[1\] has z = 0'),
    (dict(points=[[0.0, 0.0, -1e-6]]), r'points\[0\] has z = -1e-06'),
]


def test_argument_errors_come_before_any_device_call(no_device):
    import metalens_amd as ma
    from metalens_amd import postprocess
    base = dict(xp_list=AX, yp_list=AX, wavelength=WL, n_glass=NG, edges=[2e-6, 5e-6], points=PTS)
    F = np.zeros((9, 9), dtype=complex)
    for bad, said in BAD:
        kw = dict(base, **bad)
        with pytest.raises(ValueError, match=said):
            ma.ApertureZoneFields(**kw)
        with pytest.raises(ValueError, match=said):
            ma.aperture_zone_fields(F, F, F, F, **kw)
        with pytest.raises(ValueError, match=said):
            postprocess.zone_fields(F, F, F, F, kw.pop('xp_list'), kw.pop('yp_list'), **kw)
    with pytest.raises(ValueError, match='Z0 must be finite and > 0'):
        ma.ApertureZoneFields(Z0=-1.0, **base)
    for pol in ((1.0, 0.0), (0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), 'x'):
        with pytest.raises(ValueError, match=r'polarisation must be None or one \(px, py, pz\)'):
            ma.aperture_zone_fields(None, None, None, None, polarisation=pol, **base)
        with pytest.raises(ValueError, match='polarisation must be None or one'):
            postprocess.zone_fields(F, F, F, F, AX, AX, WL, NG, [2e-6], PTS, polarisation=pol)
    for first, n, said in ((-1, None, 'first must be a field set index >= 0'), (0, 0, 'takes 1 to 3 field sets per call, got n = 0'),
                           (0, 4, 'got n = 4')):
        with pytest.raises(ValueError, match=said):
            ma.aperture_zone_fields(None, None, None, None, first=first, n=n, **base)
        with pytest.raises(ValueError, match=said):
            ma.ApertureZoneFields.records(object(), first, n)
    with pytest.raises(ValueError, match=r'Hx has shape \(9, 8\), the axes give \(9, 9\)'):
        postprocess.zone_fields(F, F, F[:, :8], F, AX, AX, WL, NG, [2e-6], PTS)
    # what the checks hand on
    z = postprocess._check_zone_fields(AX, AX[:5], WL, NG, [2e-6, 5e-6], PTS, (1e-6, -2e-6))
    assert np.array_equal(z['x2'], (AX - 1e-6) ** 2) and np.array_equal(z['y2'], (AX[:5] + 2e-6) ** 2) and z['x0'] == AX[0]
    assert z['dxp'] == AX[1] - AX[0] and z['dyp'] == AX[1] - AX[0] and z['points'].shape == (1, 3) and z['p'] is None
    z = postprocess._check_zone_fields([0.5], AX, WL, NG, [1.0], PTS, pitch=(0.25, 7.0))
    assert z['dxp'] == 0.25 and z['dyp'] == 7.0                        # (the steps the caller names are the ones handed on)


def test_sweep_argument_errors_come_before_any_device_call():
    """``SourceSweep.run(zone_fields=...)``: another context, another aperture shape"""
    from metalens_amd import sweep

    class Sweep:
        ctx = 'this'
        x, y = np.zeros(9), np.zeros(8)
    check = sweep.SourceSweep._check_zone_fields

    class Z:
        ctx, shape = 'that', (9, 8)
    with pytest.raises(ValueError, match='zone_fields= must be an ApertureZoneFields built on the context of this sweep'):
        check(Sweep, Z)
    Z.ctx, Z.shape = 'this', (9, 9)
    with pytest.raises(ValueError, match="zone_fields= was built for an aperture of 9 x 9 samples, the sweep's grid has 9 x 8"):
        check(Sweep, Z)
    Z.shape = (9, 8)
    assert check(Sweep, Z) is None and check(Sweep, None) is None
    # ... and run() makes that check in front of everything that touches the device: a stand-in without a context gets that far

    class Bare:
        ctx = 'this'
        x, y = np.zeros(9), np.zeros(8)
        _check_pupil = sweep.SourceSweep._check_pupil
        _check_zone_fields = sweep.SourceSweep._check_zone_fields
    Z.shape = (9, 9)
    with pytest.raises(ValueError, match='zone_fields= was built for an aperture of 9 x 9 samples'):
        sweep.SourceSweep.run(Bare(), [(0.0, 0.0, -1e-4, 'x')], zone_fields=Z)


def test_entry_in_header_binding_and_export_map():
    from metalens_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    decl = re.search(r'int\s+ml_fields_zone_fields\s*\(([^)]*)\)', code)
    assert decl and len(decl.group(1).split(',')) == 23 and 'ml_fields_zone_fields' in _lib.SYMBOLS
    lib = _lib.load()
    assert len(lib.ml_fields_zone_fields.argtypes) == 23
    exports = open(os.path.join(ROOT, 'metalens_amd', 'csrc', 'exports.map')).read()
    assert re.search(r'global:\s*ml_\*;', exports) and 'ml_fields_zone_fields' in exports
    import makefile_deps
    assert makefile_deps.header_is_prerequisite('fields_zone_fields.h', 'fields_zone_fields')
    assert makefile_deps.header_is_prerequisite('propagate_pair.h', 'fields_zone_fields')     # one statement of the pair term,
    assert makefile_deps.header_is_prerequisite('propagate_pair.h', 'propagate')              # for both kernels
    rec, n = np.zeros(24), np.zeros(2, dtype=np.int64)
    assert lib.ml_fields_zone_fields(None, 0, 1, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, None, 0, None, 0, None, 0, None, None, None, 0, 1,
                                     _lib.dptr(rec), n.ctypes.data_as(_lib.POINTER(_lib.c_int64))) != 0      # no context
    assert b'NULL argument' in lib.ml_last_error()
