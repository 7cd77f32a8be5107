"""The focus metrics of a propagated image reduced on the GPU (csrc/propagate_focus.hip, ml_propagate_focus,
``PlanePropagator.focus``, ``SourceSweep.run(image_radii=...)``) against the NumPy yardstick of tests/propagate_focus_ref.py on
the fields or sums the same propagator downloads.  Needs an MI355X.

Shapes.  The aperture is 48 x 40 samples carrying a wave that converges on its axis (x- and y-polarised parts), so every
plane has one peak, on a target.  Planes of 21 x 17 targets (357: no multiple of 64 or 256, one chunk, my odd - a 16-byte
load of the sums straddles rows), of 70 x 61 (4270: five chunks of 1024, the last of 174) and a stack of 3 planes of
13 x 11 fine targets at half the pitch (143 a plane: planes 1 and 2 start on unaligned offsets; plane 1 on an odd index).
Methods 'direct', 'fft' and 'fft-stack', with and without H.  Field sets of a synthesis batch: the lens and the dipoles of
tests/test_gpu_propagate_sets.py on a window of 61 x 64 samples.

Bounds, derived (tests/propagate_focus_ref.py): a sum of n terms in any order is within (n + 16) u sum |term| of the exact
sum, u = 2^-53, the 16 for forming I or Sz per target - |term| of Sz taken as (|Ex||Hy| + |Ey||Hx|) / 2 times the geometric
factor; from the sums n u sum |term|.  The worst measured ratio to the bound is printed per case as a ``PARITY ...`` line
(run with -s; they belong in profiles/propagate_parity.txt).  Measured: at most 0.076 of the bound from fields, 0.27 from
the sums - the worst are the discs of 9 to 69 targets, off by an ulp or two of their sum; the sums over a whole plane are
correctly rounded or an ulp off (all eleven of the 70 x 61 plane without H are the correctly rounded ones)."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import propagate_focus_ref as fref
import propagate_grid_fine_ref as fine_ref
import propagate_grid_ref as gref
import propagate_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = fref.U
WL, N_GLASS = gref.WL, gref.N_GLASS
NX, NY = 48, 40
CASES = {   # method, mx, my, want_h
    'direct-21x17-EH': ('direct', 21, 17, True), 'direct-70x61-E': ('direct', 70, 61, False),
    'fft-21x17-E': ('fft', 21, 17, False), 'fft-70x61-EH': ('fft', 70, 61, True),
    'stack-13x11-EH': ('fft-stack', 13, 11, True), 'stack-13x11-E': ('fft-stack', 13, 11, False),
}


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


@pytest.fixture
def ctx():
    from metalens_amd import _lib
    c = _lib.default_context()
    c.set_method('auto')
    c.set_precision('f64')
    return c


@functools.lru_cache(maxsize=None)
def _wave():
    """-> x, y, focal length, (Ex, Ey, Hx, Hy): a wave converging on (0, 0, f) at sin(theta) = 0.5, 48 x 40 samples"""
    x, y = gref.axis(NX), gref.axis(NY)
    a = y.max()
    f = a / np.tan(np.arcsin(0.5))
    r2 = x[:, None] ** 2 + y[None, :] ** 2
    k, Z = 2 * np.pi * N_GLASS / WL, ref.Z0_SI / N_GLASS
    w = np.where(r2 <= a * a, np.exp(-1j * k * np.sqrt(r2 + f * f)), 0)
    Ex, Ey = w, 0.3 * np.exp(0.7j) * w
    return x, y, f, (Ex, Ey, -Ey / Z, Ex / Z)


def _make(ma, ctx, name, F=None, method=None, z=None, case=None, peak_at=None):
    """upload the wave (or F), plan the case -> the propagator; target ``peak_at`` (default: the middle one, (mx // 2,
    my // 2)) lies on the wave's axis.  ``case``: (method, mx, my, want_h) in place of ``CASES[name]``"""
    from test_gpu_fft_mixed import _upload
    from metalens_amd import _lib
    x, y, f, wave = _wave()
    case_method, mx, my, want_h = CASES[name] if case is None else case
    pi, pj = (mx // 2, my // 2) if peak_at is None else peak_at
    _upload(ctx, [_lib.c128(a) for a in (wave if F is None else F)])
    ctx.fields_owner = None
    if case_method == 'fft-stack':
        tx, ty = fine_ref.fine_axis(x, (NX - 1) / 2 - pi / 2, mx, 2), fine_ref.fine_axis(y, (NY - 1) / 2 - pj / 2, my, 2)
        planes = f + np.array([-1.0, 0.0, 1.5]) * WL / N_GLASS
        more = dict(subsample=(2, 2))
        if method == 'fft-fine':
            planes = planes[z]
    else:
        tx, ty = gref.target_axis(x, (NX - 1) / 2 - pi, mx), gref.target_axis(y, (NY - 1) / 2 - pj, my)
        planes, more = f, {}
    return ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, planes, want_h=want_h, ctx=ctx, method=method or case_method, **more)


def _pitch(p):
    return (p.x[-1] - p.x[0]) / (p.x.size - 1), (p.y[-1] - p.y[0]) / (p.y.size - 1)


def _planes(p):
    return p.z.size if p.method == 'fft-stack' else 1


def _raw(p, radii=(), centre=None, source=0):
    """the records of ml_propagate_focus, (planes, 16 + 2 K); centre: None (the peak) or (ci, cj) in index units"""
    from metalens_amd import _lib
    r = _lib.f64(radii)
    planes = _planes(p)
    rec = np.full((planes, fref.record_doubles(r.size)), np.nan)
    c = None if centre is None else _lib.f64(np.broadcast_to(np.asarray(centre, dtype=float), (planes, 2)))
    _lib.check(p.ctx.lib.ml_propagate_focus(p.ctx.handle, source, p.x.size, p.y.size, planes, *_pitch(p), _lib.dptr(c),
                                            _lib.dptr(r) if r.size else None, r.size, _lib.dptr(rec), rec.shape[1]))
    return rec


def _plane_arrays(p, d, want_h):
    """a result dict -> per plane (I, Sz, scale) as 2-D arrays"""
    I, Sz, scale = fref.weights(d, want_h)
    shape = (_planes(p), p.x.size, p.y.size)
    I = I.reshape(shape)
    if not want_h:
        return [(I[q], None, None) for q in range(shape[0])]
    Sz, scale = Sz.reshape(shape), scale.reshape(shape)
    return [(I[q], Sz[q], scale[q]) for q in range(shape[0])]


def _check_record(rec, want, K, want_h, from_sums=False):
    """one plane's record against the yardstick's -> the worst ratio of an error to its bound"""
    extra, worst = (0 if from_sums else 16), 0.0
    assert tuple(rec[fref.CENTRE:fref.CENTRE + 2]) == want['centre']
    for name, at, e_at in (('I', fref.MOM_I, fref.ENC), ('Sz', fref.MOM_SZ, fref.ENC + K)):
        if name == 'Sz' and not want_h:
            assert not rec[at:at + 6].any() and not rec[e_at:e_at + K].any()
            continue
        pairs = [(rec[at + q], want['mom_' + name][q], want['mom_%s_abs' % name][q], want['n']) for q in range(6)]
        pairs += [(rec[e_at + r], want['enc_' + name][r], want['enc_%s_abs' % name][r], want['n_inside'][r]) for r in range(K)]
        for got, exact, mag, n in pairs:
            bound = (n + extra) * U * mag
            assert abs(got - exact) <= bound, (name, got, exact, bound)
            if bound:
                worst = max(worst, abs(got - exact) / bound)
    return worst


def _check_peak(rec, I, from_sums=False, unique=True):
    flat = int(rec[fref.PEAK_INDEX])
    assert flat == rec[fref.PEAK_INDEX] and 0 <= flat < I.size
    if from_sums:
        assert rec[fref.PEAK_I] == I.max() and flat == int(np.argmax(I))
        return
    assert I.ravel()[flat] >= I.max() * (1 - 16 * U) and abs(rec[fref.PEAK_I] - I.ravel()[flat]) <= 16 * U * I.max()
    if unique:   # a precondition on the inputs, on NumPy's values alone: the runner-up lies more than 32 u below the maximum
        runner_up = np.partition(I.ravel(), -2)[-2]
        assert runner_up < I.max() * (1 - 32 * U)
        assert flat == int(np.argmax(I))


def _half_radii(p, count=5, divide=1):
    dx, dy = _pitch(p)
    assert abs(dx - dy) <= 1e-12 * dx          # (q + 1/2)^2 is no sum of two squares: no target on a boundary
    return (np.arange(count) + 0.5) * dx / divide


# ---- sums, peak, radii about the peak: every case -------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_records_against_the_yardstick(ma, ctx, name):
    method, mx, my, want_h = CASES[name]
    p = _make(ma, ctx, name)
    d = p.propagate()
    radii = _half_radii(p)
    rec = _raw(p, radii)
    assert np.array_equal(rec, _raw(p, radii))                      # two calls: the same bits
    arrays = _plane_arrays(p, d, want_h)
    worst, dx_dy = 0.0, _pitch(p)
    for q, (I, Sz, scale) in enumerate(arrays):
        want = fref.record(I, Sz, *dx_dy, radii, scale=scale)
        assert want['n_inside'] == [1, 9, 21, 37, 69][:len(radii)]   # discs about a target, whole inside the plane
        _check_peak(rec[q], I)
        assert (int(rec[q][fref.PEAK_INDEX]) // my, int(rec[q][fref.PEAK_INDEX]) % my) == (mx // 2, my // 2)   # the axis
        worst = max(worst, _check_record(rec[q], want, len(radii), want_h))
    print('PARITY focus %-16s fields: worst error / bound %.4f' % (name, worst))
    # the sums of the same pass with weight 1: the stored doubles are the terms
    p.accumulate([1.0], reset=True)
    I_sum, Sz_sum = p.sums()
    recs = _raw(p, radii, source=-1)
    assert np.array_equal(recs, _raw(p, radii, source=-1))
    shape = (_planes(p), mx, my)
    worst = 0.0
    for q in range(shape[0]):
        I, Sz = I_sum.reshape(shape)[q], (Sz_sum.reshape(shape)[q] if want_h else None)
        _check_peak(recs[q], I, from_sums=True)
        worst = max(worst, _check_record(recs[q], fref.record(I, Sz, *dx_dy, radii), len(radii), want_h, from_sums=True))
    print('PARITY focus %-16s sums:   worst error / bound %.4f' % (name, worst))
    if not want_h:   # the stored I of one member with weight 1 is the number the pass forms from its fields
        assert np.array_equal(recs, rec)


def test_python_dict_is_the_record(ma, ctx):
    """every key of ``focus()`` from the record of the entry, for the stack: shapes, units, the caller's order of radii"""
    p = _make(ma, ctx, 'stack-13x11-EH')
    p.queue_sets(0, 1)
    dx, dy = _pitch(p)
    radii = _half_radii(p, 4)
    caller = radii[[2, 0, 3, 0, 1]]
    out = p.focus(caller)
    rec = _raw(p, radii)
    assert set(out) == {'peak_I', 'peak_index', 'peak_xy', 'I_dA', 'P', 'centroid_I', 'centroid_Sz', 'second_moments_I',
                        'second_moments_Sz', 'centre_index', 'centre_xy', 'encircled_I', 'encircled_P'}
    assert out['peak_index'].shape == (3, 2) and out['peak_index'].dtype.kind == 'i' and (out['peak_index'] == (6, 5)).all()
    assert np.array_equal(out['peak_I'], rec[:, 0]) and np.array_equal(out['peak_xy'], np.tile([p.x[6], p.y[5]], (3, 1)))
    assert np.array_equal(out['centre_index'], np.tile([6.0, 5.0], (3, 1)))
    assert np.array_equal(out['I_dA'], rec[:, fref.MOM_I] * dx * dy) and np.array_equal(out['P'], rec[:, fref.MOM_SZ] * dx * dy)
    assert out['encircled_I'].shape == out['encircled_P'].shape == (3, 5)
    assert np.array_equal(out['encircled_I'], rec[:, fref.ENC:fref.ENC + 4][:, [2, 0, 3, 0, 1]] * dx * dy)
    assert np.array_equal(out['encircled_P'], rec[:, fref.ENC + 4:fref.ENC + 8][:, [2, 0, 3, 0, 1]] * dx * dy)
    for name, at in (('I', fref.MOM_I), ('Sz', fref.MOM_SZ)):
        s, si, sj, sii, sjj, sij = rec[:, at:at + 6].T
        assert np.array_equal(out['centroid_' + name], np.stack([p.x[0] + dx * (si / s), p.y[0] + dy * (sj / s)], axis=1))
        assert np.array_equal(out['second_moments_' + name], np.stack([dx * dx * (sii / s - (si / s) ** 2), dy * dy * (sjj / s - (sj / s) ** 2),
                                                                     dx * dy * (sij / s - (si / s) * (sj / s))], axis=1))
    # the wave is symmetric about its axis: the centroid is the peak to a fraction of a fine step, the spot a few steps wide
    assert np.abs(out['centroid_I'] - out['peak_xy']).max() < 0.5 * dx
    assert (out['second_moments_I'][:, :2] > 0).all() and (out['second_moments_I'][:, :2] < (6 * dx) ** 2).all()
    # without H the Sz keys are absent
    pe = _make(ma, ctx, 'stack-13x11-E')
    pe.queue_sets(0, 1)
    assert set(pe.focus(caller)) == {'peak_I', 'peak_index', 'peak_xy', 'I_dA', 'centroid_I', 'second_moments_I', 'centre_index',
                                     'centre_xy', 'encircled_I'}
    assert pe.focus()['encircled_I'].shape == (3, 0)


# ---- ties and zeros -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['direct-21x17-EH', 'stack-13x11-EH'])
def test_an_all_zero_field(ma, ctx, name):
    zero = [np.zeros((NX, NY), dtype=np.complex128) for _ in range(4)]
    p = _make(ma, ctx, name, F=zero)
    p.queue_sets(0, 1)
    radii = _half_radii(p, 3)
    out = p.focus(radii)
    assert not out['peak_index'].any() and not out['peak_I'].any() and not out['centre_index'].any()
    for key in ('I_dA', 'P', 'encircled_I', 'encircled_P'):
        assert not out[key].any() and not np.isnan(out[key]).any(), key
    for key in ('centroid_I', 'centroid_Sz', 'second_moments_I', 'second_moments_Sz'):
        assert np.isnan(out[key]).all(), key
    rec = _raw(p, radii)
    assert not rec.any()


# ---- radii ----------------------------------------------------------------------------------------------------
def test_radii_and_centres(ma, ctx):
    name = 'fft-70x61-EH'
    method, mx, my, want_h = CASES[name]
    p = _make(ma, ctx, name)
    d = p.propagate()
    (I, Sz, scale), = _plane_arrays(p, d, want_h)
    dx, dy = _pitch(p)
    # a fractional centre, given: no target within 1e-9 (relative) of a boundary, on NumPy's values
    centre, radii = (34.3, 30.55), np.array([0.8, 1.7, 2.9, 4.4, 9.3]) * dx
    for R in radii:
        r2 = fref.inside(I.shape, dx, dy, *centre, R)[1]
        assert (np.abs(r2 - R * R) > 1e-9 * R * R).all()
    rec = _raw(p, radii, centre)
    want = fref.record(I, Sz, dx, dy, radii, centre=centre, scale=scale)
    assert want['n_inside'][0] >= 1 and len(set(want['n_inside'])) == 5
    print('PARITY focus %-16s fractional centre: worst error / bound %.4f' % (name, _check_record(rec[0], want, 5, want_h)))
    assert np.array_equal(rec[0, :fref.CENTRE], _raw(p)[0, :fref.CENTRE])          # peak and moments do not depend on the radii
    # through Python: the same centre in the caller's frame
    out = p.focus(radii, centre=(p.x[0] + 34.3 * dx, p.y[0] + 30.55 * dy))
    assert np.allclose(out['centre_index'], [centre], rtol=1e-12, atol=0)
    if np.array_equal(out['centre_index'][0], centre):
        assert np.array_equal(out['encircled_I'][0], rec[0, fref.ENC:fref.ENC + 5] * dx * dy)
    # a radius of 0 about a target holds that target alone; one beyond the patch holds the plane
    far = 2 * np.hypot(mx * dx, my * dy)
    rec = _raw(p, [0.0, far], (33.0, 31.0))
    want = fref.record(I, Sz, dx, dy, [0.0, far], centre=(33.0, 31.0), scale=scale)
    assert want['n_inside'] == [1, mx * my] and want['enc_I'][0] == I[33, 31]
    _check_record(rec[0], want, 2, want_h)
    assert abs(rec[0, fref.ENC] - I[33, 31]) <= 16 * U * I[33, 31] and abs(rec[0, fref.ENC + 2] - Sz[33, 31]) <= 16 * U * scale[33, 31]
    out = p.focus([0.0, far], centre=(p.x[33], p.y[31]))
    assert np.array_equal(out['centre_index'], [[33.0, 31.0]]) and np.array_equal(out['encircled_I'][0], rec[0, fref.ENC:fref.ENC + 2] * dx * dy)
    assert abs(out['encircled_I'][0, 1] - out['I_dA'][0]) <= 2 * (mx * my + 16) * U * out['I_dA'][0]
    # K = 32: annuli a third of a pitch wide about the peak, some of them empty; K = 0; repeated radii
    thin = _half_radii(p, 32, divide=3)          # ((2 q + 1) / 6)^2 is no sum of two squares either
    rec = _raw(p, thin)
    want = fref.record(I, Sz, dx, dy, thin, scale=scale)
    assert want['n_inside'][0] == 1 and want['n_inside'][-1] == 349 and len(set(want['n_inside'])) == 26      # six annuli are empty
    print('PARITY focus %-16s K = 32: worst error / bound %.4f' % (name, _check_record(rec[0], want, 32, want_h)))
    assert _raw(p).shape == (1, 16) and np.array_equal(_raw(p)[0, :fref.CENTRE], rec[0, :fref.CENTRE])
    twice = np.repeat(_half_radii(p, 3), 2)
    rec = _raw(p, twice)
    assert np.array_equal(rec[0, fref.ENC::2], rec[0, fref.ENC + 1::2]) and np.array_equal(rec[0, fref.ENC:fref.ENC + 6:2], _raw(p, twice[::2])[0, fref.ENC:fref.ENC + 3])
    # an unsorted caller order comes back in the caller's order
    order = [3, 0, 4, 1, 2]
    sorted_out, shuffled = p.focus(_half_radii(p)), p.focus(_half_radii(p)[order])
    for key in ('encircled_I', 'encircled_P'):
        assert np.array_equal(shuffled[key], sorted_out[key][:, order]) and (np.diff(sorted_out[key][0]) != 0).all()
    for key in set(sorted_out) - {'encircled_I', 'encircled_P'}:
        assert np.array_equal(shuffled[key], sorted_out[key]), key


# ---- bit invariances ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['stack-13x11-EH', 'stack-13x11-E'])
def test_a_plane_of_the_stack_has_the_record_of_the_plane_alone(ma, ctx, name):
    p = _make(ma, ctx, name)
    p.queue_sets(0, 1)
    radii = _half_radii(p)
    about_peak, given = _raw(p, radii), _raw(p, radii, (5.25, 4.5))
    p.accumulate([0.75], reset=True)
    of_sums = _raw(p, radii, source=-1)
    assert not np.array_equal(about_peak[0], about_peak[1]) and not np.array_equal(about_peak[1], about_peak[2])
    for q in range(3):
        one = _make(ma, ctx, name, method='fft-fine', z=q)
        one.queue_sets(0, 1)
        assert np.array_equal(_raw(one, radii)[0], about_peak[q]), q
        assert np.array_equal(_raw(one, radii, (5.25, 4.5))[0], given[q]), q
        one.accumulate([0.75], reset=True)
        assert np.array_equal(_raw(one, radii, source=-1)[0], of_sums[q]), q


@functools.lru_cache(maxsize=None)
def _window():
    from test_gpu_propagate_sets import PITCH
    nx, ny, cx, cy = 61, 64, 20.0e-6, -6.0e-6        # straddles the centre disc's edge and the first rings
    return cx + (np.arange(nx) - (nx - 1) / 2) * PITCH, cy + (np.arange(ny) - (ny - 1) / 2) * PITCH


def _dipole_batch(ma, ctx):
    """the x, y, z dipoles of tests/test_gpu_propagate_sets.py synthesised on the window -> x, y, n_glass"""
    from metalens_amd import _lib
    from metalens_amd.nearfield import nearfield_params
    from test_gpu_propagate_sets import DIPOLES, _common, _lens
    lens = _lens()
    x, y = _window()
    _, (sx, sy, _), pols = DIPOLES
    sz = -lens['source_distance']
    n_glass = ma.build_nearfield(sx, sy, sz, pols[0], *_common(lens), x_pts=x, y_pts=y, ctx=ctx, download=False)[7]
    params = (_lib.NearfieldParams * 3)()
    for m, pol in enumerate(pols):
        params[m] = nearfield_params(sx, sy, sz, pol, WL, n_glass, 1e-30, ma.constants.c0, ma.constants.Z0)
    xs, ys = _lib.f64(x), _lib.f64(y)
    _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, 3, _lib.dptr(xs), xs.size, _lib.dptr(ys), ys.size))
    return x, y, n_glass


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_members_of_a_pass(ma, ctx, want_h):
    """members 0 to 2 of a ``propagate_sets`` pass: each against the yardstick on its downloaded fields, and with the record
    of ``propagate()`` on that set alone"""
    from metalens_amd import _lib
    x, y, n_glass = _dipole_batch(ma, ctx)
    tx = x.mean() + (np.arange(21) - 10) * 0.37e-6
    ty = y.mean() + (np.arange(17) - 8) * 0.37e-6
    p = ma.PlanePropagator(x, y, WL, n_glass, tx, ty, 20e-6, want_h=want_h, ctx=ctx)
    sets = p.propagate_sets()
    assert len(sets) == 3
    radii = _half_radii(p)
    dx, dy = _pitch(p)
    recs = [_raw(p, radii, source=m) for m in range(3)]
    assert not np.array_equal(recs[0], recs[1]) and not np.array_equal(recs[1], recs[2])
    worst = 0.0
    for m in range(3):
        (I, Sz, scale), = _plane_arrays(p, sets[m], want_h)
        _check_peak(recs[m][0], I, unique=False)
        centre = divmod(int(recs[m][0, fref.PEAK_INDEX]), 17)
        worst = max(worst, _check_record(recs[m][0], fref.record(I, Sz, dx, dy, radii, centre=centre, scale=scale), 5, want_h))
    print('PARITY focus members %s: worst error / bound %.4f' % ('EH' if want_h else 'E', worst))
    with pytest.raises(_lib.MetalensHipError, match='member 3 asked for, the last pass propagated 3 field sets'):
        p.focus(member=3)
    for m in range(3):
        _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
        p.propagate()
        assert np.array_equal(_raw(p, radii), recs[m]), m
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))


# ---- state ----------------------------------------------------------------------------------------------------
def test_state_and_refusals(ma, ctx):
    from metalens_amd import _lib
    p = _make(ma, ctx, 'direct-21x17-EH')
    with pytest.raises(_lib.MetalensHipError, match='ml_propagate has not run on the active propagation plan'):
        p.focus()
    d = p.propagate()
    with pytest.raises(_lib.MetalensHipError, match='ml_propagate_accumulate has not run on the active propagation plan'):
        p.focus(of='sums')
    p.accumulate([2.0], reset=True)
    sums = p.sums()
    radii = _half_radii(p)
    before, before_sums = p.focus(radii), p.focus(radii, of='sums')
    # refusals of the entry: each leaves result, sums and plan as they were
    rec, r = np.empty((1, 26)), _lib.f64(radii)
    bad = _lib.f64(radii[::-1])
    dx, dy = _pitch(p)
    h = ctx.handle
    for args, said in (((1, 21, 17, 1, dx, dy, None, _lib.dptr(r), 5, _lib.dptr(rec), 26), 'member 1 asked for, the last pass propagated 1'),
                       ((0, 17, 17, 1, dx, dy, None, _lib.dptr(r), 5, _lib.dptr(rec), 26), '289 targets, the active propagation plan has 357'),
                       ((0, 21, 17, 2, dx, dy, None, _lib.dptr(r), 5, _lib.dptr(rec), 26), '2 planes of 21 x 17'),
                       ((0, 21, 17, 1, dx, dy, None, _lib.dptr(bad), 5, _lib.dptr(rec), 26), 'the radii must not decrease'),
                       ((0, 21, 17, 1, dx, dy, None, _lib.dptr(r), 33, _lib.dptr(rec), 26), '33 radii: 0 to 32'),
                       ((0, 21, 17, 1, dx, dy, None, _lib.dptr(r), 5, _lib.dptr(rec), 25), 'record_doubles = 25'),
                       ((0, 21, 17, 1, -dx, dy, None, _lib.dptr(r), 5, _lib.dptr(rec), 26), 'pitch must be finite and > 0')):
        assert ctx.lib.ml_propagate_focus(h, *args) == -1          # ML_EINVAL
        assert said in ctx.lib.ml_last_error().decode()
    with pytest.raises(ValueError, match='at most 32 radii'):
        p.focus(np.arange(33) * dx)
    for key, value in p._download(None).items():
        assert np.array_equal(value, d[key]), key
    for got, want in zip(p.sums(), sums):
        assert np.array_equal(got, want)
    for again, first in ((p.focus(radii), before), (p.focus(radii, of='sums'), before_sums)):
        assert set(again) == set(first) and all(np.array_equal(again[k], first[k]) for k in first)
    assert all(np.array_equal(v, d[k]) for k, v in p.propagate().items())
    # a longer record than needed: filled from its start, the rest left alone
    wide = np.full((1, 40), -7.0)
    _lib.check(ctx.lib.ml_propagate_focus(h, 0, 21, 17, 1, dx, dy, None, _lib.dptr(r), 5, _lib.dptr(wide), 40))
    assert np.array_equal(wide[0, :26], _raw(p, radii)[0]) and (wide[0, 26:] == -7.0).all()
    # another propagator plans: this one's focus is refused, as accumulate is
    other = _make(ma, ctx, 'fft-21x17-E')
    with pytest.raises(RuntimeError, match='another propagator has planned'):
        p.focus()
    with pytest.raises(_lib.MetalensHipError, match='has not run on the active propagation plan'):
        other.focus()


# ---- the sweep ------------------------------------------------------------------------------------------------
def test_through_the_sweep(ma, ctx):
    from test_gpu_propagate_sets import _common, _lens
    lens = _lens()
    x, y = _window()
    u = np.linspace(-0.2, 0.2, 24)
    sw = ma.SourceSweep(*_common(lens), x, y, u, u, ctx=ctx)
    tx = x.mean() + (np.arange(21) - 10) * 0.37e-6
    ty = y.mean() + (np.arange(17) - 8) * 0.37e-6
    p = ma.PlanePropagator(x, y, WL, sw.n_glass, tx, ty, 20e-6, ctx=ctx)
    f = lens['source_distance']
    sources = [(0.3e-6, -0.2e-6, -f, pol) for pol in 'xyz'] + [(-1.0e-6, 0.5e-6, -1.05 * f, 'x')]
    weights = np.array([1.0, 0.5, 2.0, 1.5])
    radii = _half_radii(p)[[1, 0, 4, 2]]
    plain = sw.run(sources, weights=weights, image=p)
    assert set(plain) == {'P_sum', 'power_in', 'total_P', 'efficiency', 'I_sum', 'Sz_sum'}      # today's keys
    got = sw.run(sources, weights=weights, image=p, image_radii=radii)
    assert set(got) == set(plain) | {'image_focus', 'focus_efficiency'}
    for key in plain:
        assert np.array_equal(got[key], plain[key], equal_nan=True), key
    focus = p.focus(radii, of='sums')
    assert set(focus) == set(got['image_focus']) and all(np.array_equal(focus[k], got['image_focus'][k]) for k in focus)
    assert got['focus_efficiency'].shape == (1, 4)
    assert np.array_equal(got['focus_efficiency'], focus['encircled_P'] / float((weights * got['power_in']).sum()))
    assert (got['focus_efficiency'] != 0).all()
    # against the yardstick on the returned maps
    dx, dy = _pitch(p)
    rec = _raw(p, np.sort(radii), source=-1)
    want = fref.record(got['I_sum'], got['Sz_sum'], dx, dy, np.sort(radii))
    _check_peak(rec[0], got['I_sum'], from_sums=True)
    print('PARITY focus sweep sums: worst error / bound %.4f' % _check_record(rec[0], want, 4, True, from_sums=True))
    assert np.array_equal(focus['encircled_P'][0], rec[0, fref.ENC + 4:fref.ENC + 8][[1, 0, 3, 2]] * dx * dy)
    # a given centre, in the caller's frame
    given = sw.run(sources, weights=weights, image=p, image_radii=radii, image_centre=(tx[9], ty[8]))
    assert np.array_equal(given['image_focus']['centre_index'], [[9.0, 8.0]])
    # ... and the record behind it - moments and radii of the sums in one pass about a given centre - against the yardstick
    # on the returned maps
    rec = _raw(p, np.sort(radii), (9.0, 8.0), source=-1)
    want = fref.record(given['I_sum'], given['Sz_sum'], dx, dy, np.sort(radii), centre=(9.0, 8.0))
    assert len(set(want['n_inside'])) == 4 and want['n_inside'][0] == 1          # whole discs about target (9, 8)
    _check_peak(rec[0], given['I_sum'], from_sums=True)
    print('PARITY focus sweep sums, given centre: worst error / bound %.4f' % _check_record(rec[0], want, 4, True, from_sums=True))
    assert np.array_equal(given['image_focus']['encircled_P'][0], rec[0, fref.ENC + 4:fref.ENC + 8][[1, 0, 3, 2]] * dx * dy)
    assert np.array_equal(given['image_focus']['encircled_I'][0], rec[0, fref.ENC:fref.ENC + 4][[1, 0, 3, 2]] * dx * dy)


# ---- the example ----------------------------------------------------------------------------------------------
def test_focus_efficiency_example(ma):
    mods = []
    for name in ('focus_efficiency', 'through_focus'):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'examples', name + '.py'))
        mods.append(importlib.util.module_from_spec(spec))
        spec.loader.exec_module(mods[-1])
    out = mods[0].main(n=64, planes=9, verbose=False)
    want = mods[1].main(n=64, planes=9, verbose=False)
    assert out['brightest_plane'] == want['brightest_plane'] and out['z_brightest'] == want['z_brightest']
    assert out['depth_of_focus'] == want['depth_of_focus']
    assert out['peak_xyz'] == want['peak_xyz']
    enc = out['encircled_fraction']
    # the last radius holds the patch; the sixth, 428 nm - inside the Airy disc of 0.61 lambda / (n sin theta) = 485 nm -, over
    # half of its power
    assert enc.shape == (len(out['radii']),) == (13,) and 0 < enc[0] < enc[5] < 1 and enc[5] > 0.5 and abs(enc[-1] - 1) < 1e-12
