"""The Stokes records of a propagated image reduced on the GPU (csrc/propagate_stokes.hip, ml_propagate_stokes,
``PlanePropagator.stokes`` / ``accumulate_stokes`` / ``stokes_sums``, ``SourceSweep.run(image_stokes=...)``) against the NumPy twin
(``postprocess.stokes_maps``) and the yardstick of tests/propagate_stokes_ref.py on the fields or sums the same propagator
downloads.  Needs an MI355X.

The wave.  The 48 x 40 aperture and the helpers of tests/test_gpu_propagate_focus.py, carrying an x-polarised part converging on
a point half a pitch to one side of the axis and a y-polarised part, 0.8 exp(0.7 i) as strong, converging on a point half a
pitch to the other side (the foci lie 1 pitch apart along x, 0.6 along y): the polarisation varies over every plane, S1, S2
and S3 each take both signs in it (asserted on the downloaded fields), and the peak of I stays on the middle target.

Shapes: 21 x 17 (357 targets, one ragged chunk, odd my), 70 x 61 (five chunks, the last of 174), 182 x 181 (33 chunks, a
second finish tile), 1025 x 1024 by 'direct' without H (the smallest plane that doubles the chunk), stacks of 3 planes of
13 x 11 (T odd: planes and odd components of the sums on odd offsets) and of 37 x 31 (two chunks a plane).

Checks.  Exactness: a radius of 0 about a target returns the five numbers ``stokes_maps`` gives for it, bit for bit - every
formula and the sign of S3, with no tolerance.  Sums: within (n + 16) u sum |term| of the correctly rounded sum from fields, n u
sum |term| from the sums, u = 2^-53, |term| what a component is made of before it cancels (tests/propagate_stokes_ref.py); the
worst ratio is printed per case as a ``PARITY ...`` line (run with -s; they belong in profiles/propagate_parity.txt).  Measured: at
most 0.080 of the bound from fields, 0.22 from the sums.  The accumulated maps are held against the weighted sum formed
in long double."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import propagate_grid_ref as gref
import propagate_ref as ref
import propagate_stokes_ref as sref
import test_gpu_propagate_focus as tf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = sref.U
WL, N_GLASS, NX, NY = tf.WL, tf.N_GLASS, tf.NX, tf.NY
CASES = {   # method, mx, my, want_h
    'direct-21x17-EH': ('direct', 21, 17, True), 'fft-21x17-E': ('fft', 21, 17, False),
    'direct-70x61-E': ('direct', 70, 61, False), 'fft-70x61-EH': ('fft', 70, 61, True),
    'fft-182x181-EH': ('fft', 182, 181, True), 'direct-1025x1024-E': ('direct', 1025, 1024, False),
    'stack-13x11-EH': ('fft-stack', 13, 11, True), 'stack-13x11-E': ('fft-stack', 13, 11, False),
    'stack-37x31-EH': ('fft-stack', 37, 31, True),
}

ma = tf.ma
ctx = tf.ctx


@functools.lru_cache(maxsize=None)
def _two_foci():
    """(Ex, Ey, Hx, Hy) of the aperture: the x part converges on (-d / 2, -0.3 d, f), the y part on (+d / 2, +0.3 d, f)"""
    x, y, f, _ = tf._wave()
    d = gref.PITCH
    a = y.max()
    k, Z = 2 * np.pi * N_GLASS / WL, ref.Z0_SI / N_GLASS
    inside = x[:, None] ** 2 + y[None, :] ** 2 <= a * a

    def part(ox, oy):
        return np.where(inside, np.exp(-1j * k * np.sqrt((x[:, None] - ox) ** 2 + (y[None, :] - oy) ** 2 + f * f)), 0)
    Ex, Ey = part(-0.5 * d, -0.3 * d), 0.8 * np.exp(0.7j) * part(0.5 * d, 0.3 * d)
    return Ex, Ey, -Ey / Z, Ex / Z


def _uniform(ratio):
    """the symmetric wave of tests/test_gpu_propagate_focus.py with Ey = ratio Ex all over the aperture"""
    w = tf._wave()[3][0]
    Z = ref.Z0_SI / N_GLASS
    return w, ratio * w, -ratio * w / Z, w / Z


def _make(ma, ctx, name, F=None, **more):
    return tf._make(ma, ctx, name, F=_two_foci() if F is None else F, case=CASES[name], **more)


def _raw(p, radii=(), centre=None, source=0):
    """the records of ml_propagate_stokes, (planes, 9 + 5 K); centre: None (NULL) or (ci, cj) in index units / (planes, 2)"""
    from metalens_amd import _lib
    r = _lib.f64(radii)
    planes = tf._planes(p)
    rec = np.full((planes, sref.record_doubles(r.size)), np.nan)
    c = None if centre is None else _lib.f64(np.broadcast_to(np.asarray(centre, dtype=float), (planes, 2)))
    _lib.check(p.ctx.lib.ml_propagate_stokes(p.ctx.handle, source, p.x.size, p.y.size, planes, *tf._pitch(p), _lib.dptr(c),
                                             _lib.dptr(r) if r.size else None, r.size, _lib.dptr(rec), rec.shape[1]))
    return rec


def _maps(p, d):
    """a result dict -> (M, mag) of shape (5, planes, mx, my)"""
    M, mag = sref.terms(d)
    shape = (5, tf._planes(p), p.x.size, p.y.size)
    return M.reshape(shape), mag.reshape(shape)


def _half_radii(p, count, divide=1):
    dx, dy = tf._pitch(p)
    assert abs(dx - dy) <= 1e-12 * dx          # (q + 1/2)^2 is no sum of two squares: no target on a boundary
    return (np.arange(count) + 0.5) * dx / divide


# ---- formulas, peak, sums, radii: every shape -----------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_records_against_the_twin(ma, ctx, name):
    method, mx, my, want_h = CASES[name]
    p = _make(ma, ctx, name)
    d = p.propagate()
    M, mag = _maps(p, d)
    planes = M.shape[1]
    dx, dy = tf._pitch(p)
    for q in range(planes):          # the wave does what it is chosen for: each of S1, S2, S3 takes both signs in the plane
        for s in (1, 2, 3):
            assert M[s, q].min() < 0 < M[s, q].max(), (q, s)
    # exactness: a radius of 0 about a target is that target's five numbers, to the bit
    for i, j in ((0, 0), (mx - 1, my - 1), (mx // 2 - 1, my // 3)):
        rec = _raw(p, [0.0], (i, j))
        for q in range(planes):
            assert np.array_equal(rec[q, sref.ENC:sref.ENC + 5], M[:, q, i, j]), (q, i, j)
            assert tuple(rec[q, sref.CENTRE:sref.CENTRE + 2]) == (i, j)
    # the peak is focus()'s, to the bit - through the entry without a centre and through Python
    none = _raw(p)
    focus = p.focus()
    out = p.stokes()
    assert np.array_equal(none[:, 0], focus['peak_I']) and np.array_equal(out['peak_I'], focus['peak_I'])
    assert np.array_equal(out['peak_index'], focus['peak_index']) and np.array_equal(out['centre_index'], focus['peak_index'])
    assert (out['peak_index'] == (mx // 2, my // 2)).all()
    assert np.array_equal(none[:, sref.CENTRE:sref.CENTRE + 2], focus['peak_index'])
    # sums over the plane and inside 10 radii (one of them twice) about the peak's target
    radii = np.sort(np.append(_half_radii(p, 9), _half_radii(p, 3)[2]))
    centre = (mx // 2, my // 2)
    rec = _raw(p, radii, centre)
    assert np.array_equal(rec, _raw(p, radii, centre))                      # two calls: the same bytes
    assert np.array_equal(rec[:, :sref.CENTRE], none[:, :sref.CENTRE])      # peak and plane sums do not depend on the radii
    worst = 0.0
    for q in range(planes):
        want = sref.record(M[:, q], mag[:, q], dx, dy, radii, centre=centre)
        if min(mx // 2, my // 2) >= 9:
            assert want['n_inside'] == [1, 9, 21, 21, 37, 69, 97, 137, 177, 225]   # whole discs inside the plane
        assert rec[q, 0] == want['peak_I'] and rec[q, 1] == want['peak_index']
        worst = max(worst, sref.check_record(rec[q], want, len(radii)))
    print('PARITY stokes %-18s fields: worst error / bound %.4f' % (name, worst))
    # through Python, the radii unsorted and with a repeat, about the peak: two C calls, the same numbers in the caller's order
    order = [4, 0, 9, 2, 3, 7, 1, 8, 5, 6]
    out = p.stokes(radii[order])
    enc = rec[:, sref.ENC:].reshape(planes, 10, 5)[:, order] * dx * dy
    assert np.array_equal(out['encircled_S'], enc[:, :, :4]) and np.array_equal(out['encircled_Iz'], enc[:, :, 4])
    assert np.array_equal(out['S'], rec[:, 2:6] * dx * dy) and np.array_equal(out['Iz_dA'], rec[:, 6] * dx * dy)
    assert out['encircled_dop'].shape == (planes, 10)
    assert (np.abs(out['encircled_dop'][:, 1] - 1) <= 8 * U).all()                     # radius 0: one coherent target
    assert ((out['dop'] > 0) & (out['dop'] < 1)).all() and (out['encircled_dop'][:, 2] < 1).all()   # the state varies over a disc
    # the sums of the same pass with weight 1 hold the maps to the bit; their record: the stored doubles are the terms
    p.accumulate_stokes([1.0], reset=True)
    stored = p.stokes_sums()
    assert stored.shape == (5,) + p.shape and np.array_equal(stored.reshape(M.shape), M)
    recs = _raw(p, radii, centre, source=-1)
    assert np.array_equal(recs, _raw(p, radii, centre, source=-1))
    worst = 0.0
    for q in range(planes):
        want = sref.record(M[:, q], None, dx, dy, radii, centre=centre)
        assert recs[q, 0] == want['peak_I'] and recs[q, 1] == want['peak_index']
        worst = max(worst, sref.check_record(recs[q], want, len(radii), from_sums=True))
    print('PARITY stokes %-18s sums:   worst error / bound %.4f' % (name, worst))
    assert np.array_equal(recs, rec)          # the same terms in the same order, whichever loads bring them


# ---- radii ----------------------------------------------------------------------------------------------------
def test_radii_edges_and_independence(ma, ctx):
    name = 'fft-70x61-EH'
    method, mx, my, want_h = CASES[name]
    p = _make(ma, ctx, name)
    d = p.propagate()
    M, mag = _maps(p, d)
    dx, dy = tf._pitch(p)
    # K = 32 about a fractional centre near a corner: the discs are cut by two edges of the plane
    centre = (1.3, 59.2)
    radii = np.array([0.45 + 0.37 * q for q in range(32)]) * dx
    for R in radii:          # no target within 1e-9 (relative) of a boundary, on NumPy's values
        r2 = sref.inside(M.shape[2:], dx, dy, *centre, R)[1]
        assert (np.abs(r2 - R * R) > 1e-9 * R * R).all()
    rec = _raw(p, radii, centre)
    want = sref.record(M[:, 0], mag[:, 0], dx, dy, radii, centre=centre)
    full = sref.record(M[:, 0], mag[:, 0], dx, dy, radii[-1:], centre=(35.3, 30.2))['n_inside'][0]
    assert want['n_inside'][0] == 1 and want['n_inside'][-1] < 0.5 * full and len(set(want['n_inside'])) >= 28
    print('PARITY stokes %-18s K = 32, disc cut by two edges: worst error / bound %.4f' % (name, sref.check_record(rec[0], want, 32)))
    # a radius alone has the bits it has among 32; so has a pair, and a radius given twice
    for r in (0, 1, 7, 16, 31):
        alone = _raw(p, radii[r:r + 1], centre)
        assert np.array_equal(alone[0, sref.ENC:], rec[0, sref.ENC + 5 * r:sref.ENC + 5 * r + 5]), r
        assert np.array_equal(alone[0, :sref.ENC], rec[0, :sref.ENC])
    some = _raw(p, radii[[3, 3, 20]], centre)[0, sref.ENC:].reshape(3, 5)
    assert np.array_equal(some[0], some[1]) and np.array_equal(some[[0, 2]], rec[0, sref.ENC:].reshape(32, 5)[[3, 20]])
    # no target inside any radius: the radii's part of the record is all zeros (the plane's part is what it was)
    away = _raw(p, radii[:9], (-50.0, -50.0))
    assert not away[0, sref.ENC:].any() and np.array_equal(away[0, :sref.CENTRE], rec[0, :sref.CENTRE])
    assert sref.record(M[:, 0], mag[:, 0], dx, dy, radii[:9], centre=(-50.0, -50.0))['n_inside'] == [0] * 9
    out = p.stokes(radii[:2], centre=(p.x[0] - 50 * dx, p.y[0] - 50 * dy))
    assert not out['encircled_S'].any() and np.isnan(out['encircled_dop']).all()
    # one beyond the patch holds the plane
    far = 2 * np.hypot(mx * dx, my * dy)
    rec = _raw(p, [far], (35.0, 30.0))
    want = sref.record(M[:, 0], mag[:, 0], dx, dy, [far], centre=(35.0, 30.0))
    assert want['n_inside'] == [mx * my]
    sref.check_record(rec[0], want, 1)


@pytest.mark.parametrize('name', ['stack-13x11-EH', 'stack-13x11-E', 'stack-37x31-EH'])
def test_a_plane_of_the_stack_has_the_record_of_the_plane_alone(ma, ctx, name):
    p = _make(ma, ctx, name)
    p.queue_sets(0, 1)
    radii = _half_radii(p, 9)
    given = _raw(p, radii, (5.25, 4.5))
    p.accumulate_stokes([0.75], reset=True)
    of_sums = _raw(p, radii, (5.25, 4.5), source=-1)
    assert not np.array_equal(given[0], given[1]) and not np.array_equal(given[1], given[2])
    for q in range(3):
        one = _make(ma, ctx, name, method='fft-fine', z=q)
        one.queue_sets(0, 1)
        assert np.array_equal(_raw(one, radii, (5.25, 4.5))[0], given[q]), q
        one.accumulate_stokes([0.75], reset=True)
        assert np.array_equal(_raw(one, radii, (5.25, 4.5), source=-1)[0], of_sums[q]), q


# ---- the convention -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ratio, component, sign', [(1j, 3, 1.0), (-1j, 3, -1.0), (1.0, 2, 1.0), (0.0, 1, 1.0)],
                         ids=['Ey=+iEx', 'Ey=-iEx', 'Ey=Ex', 'Ey=0'])
def test_sign_convention(ma, ctx, ratio, component, sign):
    """a uniformly polarised aperture wave, symmetric about the axis, keeps its state at the on-axis target: S3 = +S0 for
    Ey = +i Ex (a sign test, not a precision claim)"""
    p = _make(ma, ctx, 'fft-21x17-E', F=_uniform(ratio))
    p.queue_sets(0, 1)
    rec = _raw(p, [0.0], (10, 8))[0]
    assert rec[1] == 10 * 17 + 8                                     # the axis' target is the peak
    S = rec[sref.ENC:sref.ENC + 4]
    assert S[0] > 0 and abs(S[component] / S[0] - sign) <= 1e-6
    out = p.stokes([0.0], centre=(p.x[10], p.y[8]))
    assert abs(out['encircled_S'][0, 0, component] / out['encircled_S'][0, 0, 0] - sign) <= 1e-6


# ---- accumulation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_accumulation(ma, ctx, want_h):
    x, y, n_glass = tf._dipole_batch(ma, ctx)
    tx = x.mean() + (np.arange(21) - 10) * 0.37e-6
    ty = y.mean() + (np.arange(17) - 8) * 0.37e-6
    p = ma.PlanePropagator(x, y, WL, n_glass, tx, ty, 20e-6, want_h=want_h, ctx=ctx)
    sets = p.propagate_sets()
    assert len(sets) == 3
    terms = [sref.terms(s) for s in sets]
    w = np.array([1.0, 0.5, 2.0])
    p.accumulate(w, reset=True)
    sums_before = p.sums()
    focus_before = p.focus(_half_radii(p, 5))
    focus_sums_before = p.focus(_half_radii(p, 5), of='sums')
    # one member with weight 1 after a reset: exactly its maps
    p.accumulate_stokes([1.0], reset=True)
    assert np.array_equal(p.stokes_sums(), terms[0][0])
    # a batch of three sets, then a second pass on top of it
    p.accumulate_stokes(w, reset=True)
    first = p.stokes_sums()
    p.accumulate_stokes(w, reset=False)
    got = p.stokes_sums()
    for passes, maps in ((1, first), (2, got)):
        exact = passes * sum(np.longdouble(wm) * t[0].astype(np.longdouble) for wm, t in zip(w, terms))   # (11 bits to spare)
        bound = (passes * 3 + 16) * U * passes * sum(abs(wm) * t[1] for wm, t in zip(w, terms))
        assert (np.abs(maps - exact) <= bound).all()
        ratio = (np.abs(maps - exact)[bound > 0] / bound[bound > 0]).astype(float)
        print('PARITY stokes accumulate %s, %d pass(es) of 3 sets: worst error / bound %.4f' % ('EH' if want_h else 'E', passes, ratio.max()))
    # the record of the sums runs on them: the stored doubles are the terms
    radii = _half_radii(p, 9)
    dx, dy = tf._pitch(p)
    rec = _raw(p, radii, (10, 8), source=-1)
    want = sref.record(got, None, dx, dy, radii, centre=(10, 8))
    assert rec[0, 0] == want['peak_I'] and rec[0, 1] == want['peak_index']
    print('PARITY stokes sums of a batch %s: worst error / bound %.4f' % ('EH' if want_h else 'E', sref.check_record(rec[0], want, 9, from_sums=True)))
    out = p.stokes(radii, of='sums')
    assert np.array_equal(out['S'][0], rec[0, 2:6] * dx * dy) and 0 <= out['dop'][0] <= 1 + 64 * U
    # member 2 of the pass
    rec = _raw(p, radii, (10, 8), source=2)
    sref.check_record(rec[0], sref.record(*terms[2], dx, dy, radii, centre=(10, 8)), 9)
    # what the Stokes calls left alone: the sums of accumulate(), focus() of the fields and of the sums
    for got_s, want_s in zip(p.sums(), sums_before):
        assert (got_s is None and want_s is None) or np.array_equal(got_s, want_s)
    for again, before in ((p.focus(_half_radii(p, 5)), focus_before), (p.focus(_half_radii(p, 5), of='sums'), focus_sums_before)):
        assert set(again) == set(before) and all(np.array_equal(again[k], before[k]) for k in before)


# ---- state ----------------------------------------------------------------------------------------------------
def test_state_and_refusals(ma, ctx):
    from metalens_amd import _lib
    p = _make(ma, ctx, 'direct-21x17-EH')
    lib, h = ctx.lib, ctx.handle
    dx, dy = tf._pitch(p)
    rec, w, maps = np.empty((1, 9)), _lib.f64([1.0]), np.empty((5, 21, 17))
    ML_ESTATE = lib.ml_propagate_sums(h, _lib.dptr(maps), None)          # (no sums on a fresh plan: the code of a state error)
    assert ML_ESTATE != 0
    stokes = lambda source=0: lib.ml_propagate_stokes(h, source, 21, 17, 1, dx, dy, None, None, 0, _lib.dptr(rec), 9)
    # before any pass
    assert stokes() == ML_ESTATE and 'ml_propagate has not run on the active propagation plan' in lib.ml_last_error().decode()
    assert lib.ml_propagate_accumulate_stokes(h, _lib.dptr(w), 1, 1) == ML_ESTATE
    with pytest.raises(_lib.MetalensHipError, match='ml_propagate has not run on the active propagation plan'):
        p.stokes()
    d = p.propagate()
    # the sums before an accumulate; a first accumulate without reset
    assert stokes(-1) == ML_ESTATE and 'ml_propagate_accumulate_stokes has not run' in lib.ml_last_error().decode()
    assert lib.ml_propagate_stokes_sums(h, _lib.dptr(maps)) == ML_ESTATE
    assert lib.ml_propagate_accumulate_stokes(h, _lib.dptr(w), 1, 0) == ML_ESTATE and 'the first call needs reset = 1' in lib.ml_last_error().decode()
    with pytest.raises(_lib.MetalensHipError, match='ml_propagate_accumulate_stokes has not run'):
        p.stokes(of='sums')
    p.accumulate([1.0], reset=True)          # the sums of accumulate() are not the Stokes sums
    assert stokes(-1) == ML_ESTATE
    # a member beyond the last pass's sets; more sets than it has
    with pytest.raises(_lib.MetalensHipError, match='member 1 asked for, the last pass propagated 1 field sets'):
        p.stokes(member=1)
    assert lib.ml_propagate_accumulate_stokes(h, _lib.dptr(_lib.f64([1.0, 1.0])), 2, 1) == -1
    assert '2 field sets to add, the last pass propagated 1' in lib.ml_last_error().decode()
    # refusals of the entry, and a centre that is NULL with radii
    r = _lib.f64(_half_radii(p, 5))
    c = _lib.f64([[10.0, 8.0]])
    wide = np.empty((1, 34))
    for args, said in (((0, 17, 17, 1, dx, dy, _lib.dptr(c), _lib.dptr(r), 5, _lib.dptr(wide), 34), '289 targets, the active propagation plan has 357'),
                       ((0, 21, 17, 1, dx, dy, None, _lib.dptr(r), 5, _lib.dptr(wide), 34), '5 radii asked for, centre is NULL'),
                       ((0, 21, 17, 1, dx, dy, _lib.dptr(c), _lib.dptr(_lib.f64(_half_radii(p, 5)[::-1])), 5, _lib.dptr(wide), 34), 'the radii must not decrease'),
                       ((0, 21, 17, 1, dx, dy, _lib.dptr(c), _lib.dptr(r), 5, _lib.dptr(wide), 33), 'record_doubles = 33'),
                       ((0, 21, 17, 1, -dx, dy, _lib.dptr(c), _lib.dptr(r), 5, _lib.dptr(wide), 34), 'pitch must be finite and > 0')):
        assert lib.ml_propagate_stokes(h, *args) == -1          # ML_EINVAL
        assert said in lib.ml_last_error().decode()
    # a longer record than needed: filled from its start, the rest left alone
    wide = np.full((1, 40), -7.0)
    _lib.check(lib.ml_propagate_stokes(h, 0, 21, 17, 1, dx, dy, _lib.dptr(c), _lib.dptr(r), 5, _lib.dptr(wide), 40))
    assert np.array_equal(wide[0, :34], _raw(p, _half_radii(p, 5), (10, 8))[0]) and (wide[0, 34:] == -7.0).all()
    # nothing of this touched the result
    for key, value in p._download(None).items():
        assert np.array_equal(value, d[key]), key
    # a new plan on the context drops the Stokes sums; another propagator's plan makes this one's calls a RuntimeError
    p.accumulate_stokes([1.0], reset=True)
    assert stokes(-1) == 0
    other = _make(ma, ctx, 'fft-21x17-E')
    assert stokes() == ML_ESTATE and stokes(-1) == ML_ESTATE and lib.ml_propagate_stokes_sums(h, _lib.dptr(maps)) == ML_ESTATE
    assert lib.ml_propagate_accumulate_stokes(h, _lib.dptr(w), 1, 0) == ML_ESTATE
    for call in (p.stokes, lambda: p.accumulate_stokes([1.0], reset=True)):
        with pytest.raises(RuntimeError, match='another propagator has planned'):
            call()
    other.propagate()
    assert lib.ml_propagate_accumulate_stokes(h, _lib.dptr(w), 1, 0) == ML_ESTATE          # a direct plan's sums did not survive the FFT plan
    other.accumulate_stokes([1.0], reset=True)
    assert stokes(-1) == 0
    again = _make(ma, ctx, 'direct-21x17-EH')
    again.propagate()
    assert lib.ml_propagate_accumulate_stokes(h, _lib.dptr(w), 1, 0) == ML_ESTATE          # nor the FFT plan's a direct plan


# ---- the sweep ------------------------------------------------------------------------------------------------
def test_through_the_sweep(ma, ctx):
    from test_gpu_propagate_sets import _common, _lens
    lens = _lens()
    x, y = tf._window()
    u = np.linspace(-0.2, 0.2, 24)
    sw = ma.SourceSweep(*_common(lens), x, y, u, u, ctx=ctx)
    tx = x.mean() + (np.arange(21) - 10) * 0.37e-6
    ty = y.mean() + (np.arange(17) - 8) * 0.37e-6
    p = ma.PlanePropagator(x, y, WL, sw.n_glass, tx, ty, 20e-6, ctx=ctx)
    f = lens['source_distance']
    sources = [(0.3e-6, -0.2e-6, -f, pol) for pol in 'xyz']
    weights = np.array([1.0, 0.5, 2.0])
    radii = _half_radii(p, 9)[[1, 0, 8, 2, 4, 3, 7, 6, 5]]
    plain = sw.run(sources, weights=weights, image=p)
    got = sw.run(sources, weights=weights, image=p, image_stokes=radii, keep_each=True)
    assert set(got) == set(plain) | {'image_stokes', 'image_stokes_maps', 'P_each', 'image_each'}
    for key in plain:          # the sums of accumulate() beside it, to the bit
        assert np.array_equal(got[key], plain[key], equal_nan=True), key
    assert set(sw.run(sources, weights=weights, image=p, image_stokes=True)['image_stokes']) == set(got['image_stokes'])
    maps = got['image_stokes_maps']
    assert maps.shape == (5, 21, 17)
    terms = [sref.terms(e) for e in got['image_each']]
    exact = sum(np.longdouble(wm) * t[0].astype(np.longdouble) for wm, t in zip(weights, terms))   # (11 bits to spare)
    bound = (3 + 16) * U * sum(abs(wm) * t[1] for wm, t in zip(weights, terms))
    assert (np.abs(maps - exact) <= bound).all()
    print('PARITY stokes sweep maps: worst error / bound %.4f' % float((np.abs(maps - exact)[bound > 0] / bound[bound > 0]).max()))
    # I_sum is S0 + Iz of the same images, formed apart: within the same bound
    assert (np.abs((maps[0] + maps[4]) - got['I_sum']) <= 2 * (bound[0] + bound[4])).all()
    st = p.stokes(radii, of='sums')
    assert set(st) == set(got['image_stokes']) and all(np.array_equal(st[k], got['image_stokes'][k], equal_nan=True) for k in st)
    assert st['encircled_S'].shape == (1, 9, 4) and (st['dop'] >= 0).all() and (st['dop'] <= 1 + 64 * U).all()
    assert (st['encircled_dop'] >= 0).all() and (st['encircled_dop'] <= 1 + 64 * U).all()
    # the record behind it against the yardstick on the returned maps
    dx, dy = tf._pitch(p)
    centre = tuple(st['centre_index'][0])
    rec = _raw(p, np.sort(radii), centre, source=-1)
    want = sref.record(maps, None, dx, dy, np.sort(radii), centre=centre)
    print('PARITY stokes sweep sums: worst error / bound %.4f' % sref.check_record(rec[0], want, 9, from_sums=True))
    assert np.array_equal(st['encircled_Iz'][0], rec[0, sref.ENC:].reshape(9, 5)[np.argsort(np.argsort(radii)), 4] * dx * dy)


# ---- the example ----------------------------------------------------------------------------------------------
def test_polarisation_purity_example(ma, capsys):
    spec = importlib.util.spec_from_file_location('polarisation_purity', os.path.join(ROOT, 'examples', 'polarisation_purity.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(keep_fields=True)
    printed = capsys.readouterr().out
    line, = [text for text in printed.splitlines() if text.startswith('cross-polarised share ')]
    share = float(line.split()[-1])
    assert share == out['cross_polarised_share']
    # the twin's record of the downloaded field: cross = (S0 - S1) / 2 over S0, each sum within (n + 16) u sum |term|
    M, mag = sref.terms(out['fields'])
    want = sref.record(M, mag, 1.0, 1.0, [])
    n = want['n']
    S0, S1 = want['sums'][0], want['sums'][1]
    twin = ma.analyser_power(np.array(want['sums'][:4]), (0, 1)) / S0
    err = (n + 16) * U * want['sums_abs'][0]                              # of S0, and of S1, whose |term| is S0's
    assert abs(share - twin) <= (err / S0) * (1 + twin) + 8 * U
    assert 0 <= share < 0.5 and twin == 0.5 * (S0 - S1) / S0              # an x-dipole's image is x-polarised, not purely
    assert 0.5 < out['dop'] <= 1 + 64 * U and 0 <= out['dop_unpolarised'] < out['dop']
    assert 'unpolarised emitter' in printed
