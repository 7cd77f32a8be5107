"""The Zernike moments of the near field's wavefront without a GPU: the plan arithmetic, the coefficient table, the host
conversion and the argument checks of csrc/fields_wavefront.h through tools/fields_wavefront_plan.cpp - layout and scratch
against the Python side, every refusal with its wording, once more under the address and undefined-behaviour sanitizers -,
``zernike`` against the yardstick's direct polar form and its orthonormality, ``postprocess.wavefront_metrics`` against the
long-double yardstick (tests/fields_wavefront_ref.py) within its bounds, what ``wavefront`` means on a field with one known
aberration, every ``ValueError`` of ``ApertureWavefront`` before any device call, and the entry's presence in header, binding,
export map and Makefile."""
import os
import re
import subprocess

import numpy as np
import pytest

import fields_wavefront_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 0), (1, 3, 4), (2, 64, 5), (3, 300, 8), (3, 4096, 8), (3, 8192, 8), (1, 4096, 4)]


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('wavefront_plan')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'fields_wavefront_plan',
                           out + 'fields_wavefront_plan_san'])

    def run(*args, exe='fields_wavefront_plan'):
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
    from metalens_amd import postprocess as pp
    lines = tool(*_flat(SHAPES)).splitlines()
    assert len(lines) == len(SHAPES)
    for (sets, nx, n_max), line in zip(SHAPES, lines):
        J = (n_max + 1) * (n_max + 2) // 2
        assert _facts(line) == dict(sets=sets, nx=nx, n_max=n_max, terms=J, record=4 + 4 * J, line_record=4 + 4 * (n_max + 1),
                                    scratch=sets * nx * (4 + 4 * (n_max + 1)) * 8), line
        assert len(pp.zernike_terms(n_max)) == J and pp.wavefront_record(n_max) == 4 + 4 * J
    assert _facts(lines[4])['scratch'] == 3932160 < 5e6          # three sets of 4096 lines at order 8: under 5 MB


def test_record_layout(tool):
    from metalens_amd import postprocess as pp, wavefront
    f = _facts(tool('layout'))
    assert f == dict(n=pp._WF_N, s=pp._WF_S, ix=pp._WF_IX, iy=pp._WF_IY, head=pp._WF_HEAD, order_max=pp.ZERNIKE_ORDER_MAX, terms_max=45,
                     sets_max=wavefront.SETS_MAX, block=64, line_threads=256, sum_threads=256, plane=pp.ZONES_REF_PLANE,
                     focus=pp.ZONES_REF_FOCUS)
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    assert re.search(r'#define\s+ML_ZERNIKE_ORDER_MAX\s+8\b', text)
    assert re.search(r'#define\s+ML_ZERNIKE_RECORD\(n_max\)\s+\(4 \+ 2 \* \(\(n_max\) \+ 1\) \* \(\(n_max\) \+ 2\)\)', text)
    # the order of the monomial moments of a set: ascending p, then q
    for n_max in (0, 3, 8):
        want = ['p=%d q=%d at=%d' % (p, q, at) for at, (p, q) in
                enumerate((p, q) for p in range(n_max + 1) for q in range(n_max + 1 - p))]
        assert tool('monomials', n_max).splitlines() == want


def test_coefficient_table(tool):
    """the header's integer table term by term: its checksums are those of the Python table and of the yardstick's, which
    multiplies the polynomials out; OSA/ANSI order; N_j correctly rounded; the conditioning figure"""
    from metalens_amd import postprocess as pp
    lines = tool('table', 8).splitlines()
    terms = pp.zernike_terms(8)
    assert len(lines) == 46 and terms.shape == (45, 2) and terms.tolist() == [list(t) for t in ref.terms(8)]
    worst = 0
    for j, ((n, m), line) in enumerate(zip(terms.tolist(), lines)):
        A = pp._zernike_coefficients(n, m)
        assert A == ref.coefficients(n, m) and all(p + q <= n for p, q in A) and list(A) == sorted(A)
        assert all(isinstance(v, int) and 0 < abs(v) < 2 ** 53 for v in A.values())
        assert j == (n * (n + 2) + m) // 2
        norm = np.sqrt(np.longdouble(n + 1 if m == 0 else 2 * (n + 1)))
        assert line == 'j=%d n=%d m=%d index=%d nonzero=%d sum=%d abs=%d norm=%.17g' % (
            j, n, m, j, len(A), sum(A.values()), sum(abs(v) for v in A.values()), float(norm)), line
        assert pp._zernike_norm(n, m) == float(norm)
        worst = max(worst, sum(abs(v) for v in A.values()))
    assert lines[-1] == 'worst_abs=%d' % worst == 'worst_abs=2641'
    assert tool('table', 4).splitlines()[:-1] == lines[:15]


def test_host_conversion_has_the_twins_bits(tool):
    """wf_convert of the header and ``_wavefront_convert`` of the twin: the same record from the same monomial moments, bit for
    bit, with magnitudes over six decades and both signs"""
    from metalens_amd import postprocess as pp
    rng = np.random.default_rng(11)
    for n_max in (0, 1, 4, 5, 8):
        J = (n_max + 1) * (n_max + 2) // 2
        mono = rng.standard_normal(4 + 4 * J) * 10.0 ** rng.uniform(-3, 3, 4 + 4 * J)
        for exe in ('fields_wavefront_plan', 'fields_wavefront_plan_san'):
            got = np.array([float(v) for v in tool('convert', n_max, ','.join('%.17g' % v for v in mono), exe=exe).split()])
            M = [[None] * (n_max + 1) for _ in range(n_max + 1)]
            at = 0
            for p in range(n_max + 1):
                for q in range(n_max + 1 - p):
                    M[p][q] = mono[None, 4 + 4 * at:8 + 4 * at]
                    at += 1
            want = pp._wavefront_convert(mono[None, :4], M, n_max)[0]
            assert got.shape == want.shape == (4 + 4 * J,) and got.tobytes() == want.tobytes(), n_max


# n_ranks res_nx res_ny res_sets first n_sets n_max ref_mode ref_c k r2 record_doubles x2 xi y2 eta ra rb -> code, message
X2, XI, Y2, ETA, Z3, Z4 = '1,0,1', '-0.5,0,0.5', '4,1,0,1', '-1,-0.5,0,0.5', '0,0,0', '0,0,0,0'
OK = (1, 3, 4, 1, 0, 1, 4, 0, 0, 0, 4, 64, X2, XI, Y2, ETA, Z3, Z4)
NAMES = ('n_ranks', 'res_nx', 'res_ny', 'res_sets', 'first', 'n_sets', 'n_max', 'mode', 'ref_c', 'k', 'r2', 'rd', 'x2', 'xi', 'y2', 'eta',
         'ra', 'rb')


def _with(**kw):
    args = dict(zip(NAMES, OK))
    args.update(kw)
    return tuple(args[n] for n in NAMES)


P = 'ml_fields_zernike: '
REFUSALS = [
    (_with(n_ranks=2), -1, P + 'this context belongs to a communicator of 2 ranks'),
    (_with(res_nx=0, res_ny=0, res_sets=0), -2, 'no resident field set'),
    (_with(res_nx=4), -1, P + 'the axes have 3 x 4 samples, the resident field sets 4 x 4'),
    (_with(res_ny=5), -1, P + 'the axes have 3 x 4 samples, the resident field sets 3 x 5'),
    (_with(n_sets=0), -1, P + 'a pass takes 1 to 3 field sets, got 0'),
    (_with(n_sets=4, res_sets=4), -1, P + 'a pass takes 1 to 3 field sets, got 4'),
    (_with(first=1), -1, P + 'field sets 1 ... 1 asked for, 1 resident'),
    (_with(first=-1), -1, P + 'field sets -1 ... -1 asked for, 1 resident'),
    (_with(n_sets=3, res_sets=2), -1, P + 'field sets 0 ... 2 asked for, 2 resident'),
    (_with(n_max=-1), -1, P + 'n_max = -1: radial orders 0 to 8 are taken'),
    (_with(n_max=9, rd=1000), -1, P + 'n_max = 9: radial orders 0 to 8 are taken'),
    (_with(r2=0), -1, P + 'r2 = 0: the squared radius of the pupil must be finite and > 0'),
    (_with(r2=-1), -1, P + 'r2 = -1: the squared radius'),
    (_with(r2='nan'), -1, P + 'r2 = nan: the squared radius'),
    (_with(r2='inf'), -1, P + 'r2 = inf: the squared radius'),
    (_with(x2='1,-1,1'), -1, P + 'x2[1] = -1: a squared distance must be finite and >= 0'),
    (_with(y2='4,1,nan,1'), -1, P + 'y2[2] = nan: a squared distance'),
    (_with(xi='0,inf,0'), -1, P + 'xi[1] = inf: a pupil coordinate must be finite'),
    (_with(eta='0,0,0,nan'), -1, P + 'eta[3] = nan: a pupil coordinate must be finite'),
    (_with(y2='4,1,2,1'), -1, P + 'y2 must fall to its minimum y2[1] = 1 and rise again (a y axis in ascending or descending order): '
                                  'y2[3] = 1 follows y2[2] = 2'),
    (_with(y2='1,4,0,1'), -1, P + 'y2 must fall to its minimum y2[2] = 0 and rise again'),
    (_with(mode=2), -1, P + 'ref_mode 2: 0 for a plane wave or 1 for a focus'),
    (_with(ra='0,inf,0'), -1, P + 'ra[1] = inf: a reference phase must be finite'),
    (_with(mode=1, ref_c=1e-3, k=1e7, rb='0,0,-1,0'), -1, P + 'rb[2] = -1: a squared distance to the focus must be finite and >= 0'),
    (_with(mode=1, ref_c=0, k=1e7), -1, P + 'ref_c = 0: the focus lies at a finite distance zf != 0'),
    (_with(mode=1, ref_c='nan', k=1e7), -1, P + 'ref_c = nan'),
    (_with(mode=1, ref_c=1e-3, k=0), -1, P + 'k = 0: the wave number must be finite and > 0'),
    (_with(mode=1, ref_c=-2e-3, k=1e7, ra='1e6,0,0'), -1, P + 'the reference phase reaches 1e+10 rad on this grid: the phase arithmetic covers up to 1e+09'),
    (_with(ra='6e8,0,-7e8', rb='6e8,0,0,-4e8'), -1, P + 'the reference phase reaches 1.2e+09 rad'),
    (_with(rd=63), -1, P + 'record_doubles = 63: a record of order 4 has 64 doubles'),
    (_with(n_max=8, rd=183), -1, P + 'record_doubles = 183: a record of order 8 has 184 doubles'),
    (_with(x2='null', xi='null', ra='null', res_nx=0, res_ny=0), -1, P + 'the axes have 0 x 4 samples: at least one each'),
    (_with(ra='null'), -1, P + 'NULL argument'),
    (_with(xi='null'), -1, P + 'NULL argument'),
    (_with(eta='null'), -1, P + 'NULL argument'),
    # an argument error is named before the state
    (_with(res_nx=0, res_ny=0, res_sets=0, n_sets=5), -1, P + 'a pass takes 1 to 3 field sets, got 5'),
]
ACCEPTED = [(OK, 0.0), (_with(rd=70), 0.0), (_with(n_max=0, rd=8), 0.0), (_with(n_max=8, rd=184), 0.0), (_with(n_sets=3, res_sets=3), 0.0),
            (_with(first=2, n_sets=1, res_sets=3), 0.0), (_with(y2='0,1,4,9'), 0.0), (_with(y2='9,4,1,1'), 0.0), (_with(r2=1e-300), 0.0),
            (_with(xi='-1e300,0,1e300'), 0.0), (_with(ra='5e8,0,-5e8', rb='5e8,0,0,-5e8'), 1e9),
            (_with(mode=1, ref_c=-3.0, k=2.0, ra='16,0,0'), 10.0)]


def test_refusals_name_the_numbers(tool):
    said_all = [said for _args, _code, said in REFUSALS]
    for args, code, said in REFUSALS:
        out = tool('check', *args)
        assert out.startswith('refused=%d\n' % code) and said in out, (out, said)
    # every refusal has a wording of its own: the messages differ beyond their numbers
    shapes = {re.sub(r'[-+]?(\d+\.?\d*(e[-+]?\d+)?|nan|inf)', '#', tool('check', *a).splitlines()[1]) for a, _c, _s in REFUSALS}
    assert len(shapes) >= 21 and len(said_all) == len(REFUSALS)
    for args, phase in ACCEPTED:
        assert tool('check', *args) == 'ok=1 phase=%.17g\n' % phase, args


def test_under_sanitizers(tool):
    """the same program under the address and undefined-behaviour sanitizers: same output, nothing reported"""
    san = 'fields_wavefront_plan_san'
    assert tool(*_flat(SHAPES), exe=san) == tool(*_flat(SHAPES)) and tool('layout', exe=san) == tool('layout')
    assert tool('table', 8, exe=san) == tool('table', 8) and tool('monomials', 8, exe=san) == tool('monomials', 8)
    for args, _code, _said in REFUSALS:
        assert tool('check', *args, exe=san) == tool('check', *args)
    for args, phase in ACCEPTED:
        assert tool('check', *args, exe=san) == 'ok=1 phase=%.17g\n' % phase


# ---- the terms ------------------------------------------------------------------------------
def test_zernike_against_the_direct_polar_form():
    """``zernike(n, m, xi, eta)`` - the polynomial in (xi, eta) - against R_n^|m|(rho) cos / sin(m phi) in long double at 2000
    seeded points of the disc, for all 45 terms: within 26 roundings of the sum of the coefficients' magnitudes (a power
    and a product per monomial and at most 25 additions; |xi^p eta^q| <= 1)"""
    import metalens_amd as ma
    rng = np.random.default_rng(5)
    rho, phi = np.sqrt(rng.uniform(0, 1, 2000)), rng.uniform(-np.pi, np.pi, 2000)
    xi, eta = rho * np.cos(phi), rho * np.sin(phi)
    amp = ref.amplitudes(8)
    worst = 0.0
    for j, (n, m) in enumerate(ma.zernike_terms(8)):
        got = ma.zernike(n, m, xi, eta)
        want = ref.zernike_ld(int(n), int(m), xi, eta)
        err = float(np.abs(got - want).max())
        worst = max(worst, err / (amp[j] * ref.U))
        assert err <= (26 + 3 * n) * ref.U * amp[j], (n, m, err)
    print('zernike against the polar form: at most %.2f u amp_j' % worst)
    assert ma.zernike(0, 0, 0.3, -0.2) == 1.0 and ma.zernike(1, 1, 0.25, 0.0) == 0.5 and ma.zernike(1, -1, 0.0, 0.25) == 0.5
    assert ma.zernike(2, 0, xi[:, None], eta[None, :3]).shape == (2000, 3)
    for bad in ((9, 1), (2, 1), (2, 4), (-1, 1), (2.5, 0.5)):
        with pytest.raises(ValueError, match='a Zernike term needs 0 <= n <= 8'):
            ma.zernike(bad[0], bad[1], 0.0, 0.0)


def test_terms_are_orthonormal_on_the_disc():
    """(1 / pi) int Z_j Z_k d^2 rho = delta_jk by a quadrature that is exact for these polynomials: 24 Gauss-Legendre nodes in
    rho (degree 17 with the weight rho) times 64 equidistant angles"""
    import metalens_amd as ma
    t, wt = np.polynomial.legendre.leggauss(24)
    rho, wr = 0.5 * (t + 1), 0.5 * wt
    phi = 2 * np.pi * (np.arange(64) + 0.5) / 64
    xi, eta = rho[:, None] * np.cos(phi)[None, :], rho[:, None] * np.sin(phi)[None, :]
    w = (wr * rho)[:, None] * (2 * np.pi / 64) / np.pi
    Z = np.stack([ma.zernike(n, m, xi, eta) for n, m in ma.zernike_terms(8)])
    G = np.einsum('jab,kab,ab->jk', Z, Z, w)
    assert np.abs(G - np.eye(45)).max() < 1e-11                     # (amp_j amp_k u ~ 8e3^2 1e-16)


# ---- postprocess.wavefront_metrics against the yardstick -------------------------------------
@pytest.mark.parametrize('case', ref.cases(), ids=lambda c: c[0].replace(' ', '_'))
def test_wavefront_metrics_against_the_yardstick(case):
    from metalens_amd import postprocess
    name, x, y, wl, ng, radius, n_max, centre, reference = case
    F = ref.seeded_fields(2, x.size, y.size, seed=x.size * 1000 + y.size)
    got = postprocess.wavefront_metrics(F[:, 0], F[:, 1], F[:, 2], F[:, 3], x, y, wl, ng, radius, n_max, centre, reference)
    want = ref.exact(F, x, y, wl, ng, radius, n_max, centre, reference)
    assert want['n'] > 0 and want['outside'] > 0
    ref.hold('twin ' + name, got, want)
    J = (n_max + 1) * (n_max + 2) // 2
    assert got['moments'].shape == (2, 2, J) and got['wavefront'].shape == (2, 2, J) and got['I'].shape == (2, 2)
    assert got['P'].shape == (2,) and got['rms'].shape == got['piston'].shape == got['coherence'].shape == (2, 2)
    # one set given as 2-D arrays: the same numbers with a leading axis of one
    one = postprocess.wavefront_metrics(F[1, 0], F[1, 1], F[1, 2], F[1, 3], x, y, wl, ng, radius, n_max, centre, reference)
    for key in ('P', 'I', 'moments', 'wavefront'):
        assert one[key].shape[0] == 1 and np.array_equal(one[key][0], got[key][1]), key
    # the terms up to a lower order do not depend on n_max
    if n_max >= 3:
        low = postprocess.wavefront_metrics(F[:, 0], F[:, 1], F[:, 2], F[:, 3], x, y, wl, ng, radius, 2, centre, reference)
        assert np.array_equal(low['moments'], got['moments'][..., :6]) and np.array_equal(low['I'], got['I'])


def test_wavefront_metrics_rim_and_empty_pupil():
    from metalens_amd import postprocess
    # integer axes: the samples (3, 4), (4, 3), (5, 0) and (0, 5) lie exactly on R = 5 and are inside
    x = y = np.arange(16.0)
    F = ref.seeded_fields(1, 16, 16, seed=3)
    got = postprocess.wavefront_metrics(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, y, 4.0, 1.0, 5.0)
    inside = ref.membership(x, y, 5.0, (0.0, 0.0))
    assert inside[3, 4] and inside[5, 0] and not inside[4, 4] and got['samples'] == inside.sum() == 26 and got['outside'] == 256 - 26
    # a pupil between the samples holds nothing: zero sums, NaN coherence, wavefront and rms, piston 0
    got = postprocess.wavefront_metrics(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, y, 4.0, 1.0, 0.3, centre=(2.5, 2.5))
    assert got['samples'] == 0 and got['area'] == 0 and (got['P'] == 0).all() and (got['moments'] == 0).all()
    assert np.isnan(got['coherence']).all() and np.isnan(got['wavefront']).all() and np.isnan(got['rms']).all() and (got['piston'] == 0).all()
    with pytest.raises(ValueError, match=r'Hx has shape \(16, 15\), the axes give \(16, 16\)'):
        postprocess.wavefront_metrics(F[0, 0], F[0, 1], F[0, 2, :, :15], F[0, 3], x, y, 4.0, 1.0, 5.0)
    # a field that follows the reference: coherence 1, piston as given, no aberration
    k = ref.wave_number(4.0, 1.0)
    w = np.exp(1j * k * (0.3 * x[:, None] - 0.2 * y[None, :]))
    got = postprocess.wavefront_metrics(w, 2 * w * np.exp(0.5j), w, w, x, y, 4.0, 1.0, 9.0, centre=(7.0, 8.0), reference=('plane', 0.3, -0.2))
    assert np.allclose(got['coherence'], 1.0, rtol=0, atol=1e-13) and np.allclose(got['piston'][0], [0.0, 0.5], atol=1e-13)
    assert np.abs(got['wavefront']).max() < 1e-12 and got['rms'].max() < 1e-12


# the deviation of the long-double yardstick itself on the grid of the meaning test, measured (see the test's docstring)
YARDSTICK_DEVIATION = {(1, 1): 2.448e-6, (2, 0): 4.436e-6, (3, 1): 3.444e-6, (8, 0): 7.432e-6}


def _aberrated(n, m, eps):
    from metalens_amd import postprocess
    wl, ng = 580e-9, 1.46
    p = wl / 2.2
    x = y = (np.arange(257) - 128) * p
    R = 120 * p
    reference = ('plane', 0.2, -0.1)
    w = np.exp(1j * ref.wave_number(wl, ng) * (0.2 * x[:, None] - 0.1 * y[None, :]))
    E = w * np.exp(1j * eps * postprocess.zernike(n, m, x[:, None] / R, y[None, :] / R))
    return np.stack([E, 2 * E * np.exp(0.5j), w, w])[None], x, y, wl, ng, R, reference


@pytest.mark.parametrize('term', sorted(YARDSTICK_DEVIATION), ids=str)
def test_wavefront_reads_a_known_aberration(term):
    """what ``wavefront`` means: the field ``w exp(i eps Z_k)`` on a 257 x 257 grid, pupil R = 120 samples (45225 members),
    eps = 1e-3, for a tilt (1, 1), defocus (2, 0), coma (3, 1) and Z_8^0, analysed at n_max = 8: ``wavefront[k] = eps`` and the
    other 44 terms are 0, for Ex and for an Ey with twice the amplitude and a piston of 0.5 rad.  The tolerance is twice the
    deviation the long-double yardstick itself shows on that grid - from the grid's non-orthogonality, O(pitch / R), and
    from eps^2 - measured with tests/fields_wavefront_ref.py as max_j |Im(m_j / m_0) - eps delta_jk|:
        tilt 2.448e-06 (own term 3.07e-07)   defocus 4.436e-06 (6.12e-07)   coma 3.444e-06 (9.13e-07)   Z_8^0 7.432e-06 (2.31e-06)
    and the twin's own deviation was the same to four digits.  The tilt's figure is measured again here."""
    from metalens_amd import postprocess
    eps = 1e-3
    F, x, y, wl, ng, R, reference = _aberrated(term[0], term[1], eps)
    got = postprocess.wavefront_metrics(F[:, 0], F[:, 1], F[:, 2], F[:, 3], x, y, wl, ng, R, 8, reference=reference)
    k = ref.terms(8).index(term)
    want = np.zeros(45)
    want[k] = eps
    dev = np.abs(got['wavefront'] - want).max()
    print('wavefront of eps Z(%d, %d): deviation %.4g, yardstick %.4g' % (term[0], term[1], dev, YARDSTICK_DEVIATION[term]))
    assert got['samples'] == 45225 and dev <= 2 * YARDSTICK_DEVIATION[term]
    assert np.allclose(got['piston'][0], [0.0, 0.5], atol=1e-5) and np.allclose(got['rms'], eps, rtol=0, atol=4 * YARDSTICK_DEVIATION[term])
    assert np.allclose(got['coherence'], 1.0, rtol=0, atol=2 * eps * eps)        # Strehl 1 - eps^2
    if term == (1, 1):
        exact = ref.exact(F, x, y, wl, ng, R, 8, reference=reference)
        mom = exact['Zr'] + 1j * exact['Zi']
        own = float(np.abs((mom / mom[..., :1]).imag - want).max())
        assert abs(own - YARDSTICK_DEVIATION[term]) <= 1e-3 * YARDSTICK_DEVIATION[term], own


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
    (dict(radius=0.0), 'the radius of the pupil must be finite and > 0, got 0.0'),
    (dict(radius=-1e-6), 'the radius of the pupil must be finite and > 0'),
    (dict(radius=np.nan), 'the radius of the pupil must be finite and > 0'),
    (dict(radius=np.inf), 'the radius of the pupil must be finite and > 0'),
    (dict(radius=[1e-6, 2e-6]), 'radius must be one number'),
    (dict(radius='wide'), 'radius must be one number'),
    (dict(n_max=9), 'n_max must be a radial order from 0 to 8, got 9'),
    (dict(n_max=-1), 'n_max must be a radial order from 0 to 8, got -1'),
    (dict(n_max=2.5), 'n_max must be a radial order from 0 to 8, got 2.5'),
    (dict(n_max=True), 'n_max must be a radial order from 0 to 8'),
    (dict(centre=(0.0,)), r'centre must be one \(xc, yc\)'),
    (dict(centre='peak'), r'centre must be one \(xc, yc\)'),
    (dict(centre=(0.0, np.inf)), 'a centre must be finite'),
    (dict(reference=('sphere', 0.0, 0.0)), r"reference must be \('plane', ux, uy\) or \('focus', xf, yf, zf\)"),
    (dict(reference=('plane', 0.0)), r"reference must be \('plane', ux, uy\)"),
    (dict(reference=None), r"reference must be \('plane', ux, uy\)"),
    (dict(reference=('plane', 0.8, 0.7)), r'a plane-wave reference needs ux\^2 \+ uy\^2 <= 1, got \(0.8, 0.7\)'),
    (dict(reference=('focus', 0.0, 0.0, 0.0)), r'a focus reference needs a finite focus \(xf, yf, zf\) with zf != 0, got \(0, 0, 0\)'),
]


def test_argument_errors_come_before_any_device_call(no_device):
    import metalens_amd as ma
    from metalens_amd import postprocess
    base = dict(xp_list=AX, yp_list=AX, wavelength=580e-9, n_glass=1.46, radius=8e-6)
    F = np.zeros((9, 9), dtype=complex)
    for bad, said in BAD:
        kw = dict(base, **bad)
        with pytest.raises(ValueError, match=said):
            ma.ApertureWavefront(**kw)
        with pytest.raises(ValueError, match=said):
            ma.aperture_wavefront(F, F, F, F, **kw)
        with pytest.raises(ValueError, match=said):
            postprocess.wavefront_metrics(F, F, F, F, kw.pop('xp_list'), kw.pop('yp_list'), **kw)
    for first, n, said in ((-1, None, 'first must be a field set index >= 0'), (0, 0, 'takes 1 to 3 field sets per call, got n = 0'),
                           (0, 4, 'got n = 4'), (0.5, 1, 'first must be a field set index')):
        with pytest.raises(ValueError, match=said):
            ma.aperture_wavefront(None, None, None, None, first=first, n=n, **base)
        with pytest.raises(ValueError, match=said):
            ma.ApertureWavefront.records(object(), first, n)            # (what analyse() calls first)
    with pytest.raises(ValueError, match='n_max must be a radial order'):
        ma.zernike_terms(9)
    # what the checks hand on
    z = postprocess._check_wavefront(AX, AX[::-1], 580e-9, 1.46, 8e-6, 5, (1e-6, -2e-6), ('focus', 1e-6, 0.0, -3e-5))
    assert np.array_equal(z['x2'], (AX - 1e-6) ** 2) and np.array_equal(z['y2'], (AX[::-1] + 2e-6) ** 2) and z['r2'] == 8e-6 * 8e-6
    assert np.array_equal(z['xi'], (AX - 1e-6) / 8e-6) and np.array_equal(z['eta'], (AX[::-1] + 2e-6) / 8e-6) and z['R'] == 8e-6
    assert z['mode'] == 1 and z['ref_c'] == -3e-5 and z['k'] == 2 * np.pi * 1.46 / 580e-9 and z['n_max'] == 5 and len(z['terms']) == 21
    assert np.array_equal(z['ra'], (AX - 1e-6) ** 2) and np.array_equal(z['rb'], AX[::-1] ** 2) and z['dA'] == (AX[1] - AX[0]) ** 2
    assert 'e2' not in z
    assert ma.zernike_terms(2).tolist() == [[0, 0], [1, -1], [1, 1], [2, -2], [2, 0], [2, 2]] and ma.zernike_terms(0).shape == (1, 2)


def test_entry_in_header_binding_export_map_and_makefiles():
    import metalens_amd as ma
    from metalens_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'metalens_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    decl = re.search(r'int\s+ml_fields_zernike\s*\(([^)]*)\)', code)
    assert decl and len(decl.group(1).split(',')) == 18 and 'ml_fields_zernike' in _lib.SYMBOLS
    lib = _lib.load()
    assert len(lib.ml_fields_zernike.argtypes) == 18
    exports = open(os.path.join(ROOT, 'metalens_amd', 'csrc', 'exports.map')).read()
    assert re.search(r'global:\s*ml_\*;', exports) and 'ml_fields_zernike' in exports
    import makefile_deps
    assert makefile_deps.header_is_prerequisite('fields_wavefront.h', 'fields_wavefront')   # (the unit is built, the header rebuilds it)
    tools = open(os.path.join(ROOT, 'tools', 'Makefile')).read()
    assert '$(OUT)fields_wavefront_plan:' in tools and '$(OUT)fields_wavefront_plan_san:' in tools
    for name in ('ApertureWavefront', 'aperture_wavefront', 'zernike', 'zernike_terms', 'wavefront'):
        assert hasattr(ma, name), name
    rec = np.zeros(64)
    assert lib.ml_fields_zernike(None, 0, 1, None, None, 0, None, None, 0, 0.0, 4, 0, None, None, 0.0, 0.0, _lib.dptr(rec), 64) != 0   # no context
    assert b'NULL argument' in lib.ml_last_error()
