"""The transfer function of a propagated image contracted on the GPU (csrc/propagate_otf.hip, ml_propagate_otf,
``PlanePropagator.otf``, ``SourceSweep.run(image_freqs=...)``) against the yardstick of tests/propagate_otf_ref.py on the
fields or sums the same propagator downloads.  Needs an MI355X.

Shapes: the aperture, the wave and the cases of tests/test_gpu_propagate_focus.py - planes of 21 x 17 targets (one
segment of 32 along either axis, my odd), of 70 x 61 (three segments along x, the last of 6; two along y, the last of 29)
and a stack of 3 planes of 13 x 11 (planes 1 and 2 on unaligned offsets, plane 1 on an odd index); 'direct', 'fft' and
'fft-stack', with and without H.  Frequency sets, in cycles per sample: (1, 1) at 0, 5 x 1, 1 x 7, 3 x 64 and 64 x 64, each
with 0, +-0.5, 1/3, a pair f, -f and a repeat among its frequencies.

Bounds, derived (tests/propagate_otf_ref.py): each of re and im within (n + 96) u sum |term| of the yardstick, n = mx my,
u = 2^-53; n + 80 from the sums.  Where a plane times a frequency set has more than 2^20 terms - 70 x 61 under 64 x 64 alone -
the yardstick is computed for the corner values of either axis (0, +-0.5, +-1/3, +-0.1 and the repeat, all of them) and
every k-th of its random frequencies: there 15 x 15 of the 64 x 64 entries, every pairing of two corner values among them;
the other entries of that call are held by the bit tests alone (an entry does not depend on the others of its call, and
the same frequencies are held in full on the smaller planes).
The worst ratio of an error to its bound is printed per case as a ``PARITY otf ...`` line (run with -s; they belong in
profiles/propagate_parity.txt).  The phasors are held on their own: 16 u absolute."""
import numpy as np
import pytest

import propagate_otf_ref as oref
from test_gpu_propagate_focus import CASES, WL, _dipole_batch, _make, _pitch, _plane_arrays, _planes, _window
from test_gpu_propagate_focus import ctx, ma  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

U = oref.U
OTF_PHASOR = 9          # ML_PROBE_OTF_PHASOR
THIRD = 1 / 3


def _axis64(seed):
    """64 frequencies: the corner values, a repeat, and random ones - half of them with a full mantissa (at least 2^-7 in
    size, so that 2^61 holds every numerator), half on a lattice of 2^-40"""
    rng = np.random.default_rng(seed)
    full = rng.uniform(2.0 ** -7, 0.5, 28) * rng.choice([-1.0, 1.0], 28)
    lattice = rng.integers(-2 ** 39, 2 ** 39, 28) / 2.0 ** 40
    f = np.concatenate([[0.0, 0.5, -0.5, THIRD, -THIRD, 0.1, -0.1, THIRD], full, lattice])
    return f[rng.permutation(64)]


FREQS = {
    '1x1': (np.array([0.0]), np.array([0.0])),
    '5x1': (np.array([THIRD, -0.5, 0.0, 0.5, THIRD]), np.array([0.0])),
    '1x7': (np.array([0.0]), np.array([0.5, 0.0, -THIRD, THIRD, -0.5, 0.1, 0.0])),
    '3x64': (np.array([-0.5, 0.0, THIRD]), _axis64(5)),
    '64x64': (_axis64(6), _axis64(7)),
}


def _raw(p, u, v, source=0):
    """ml_propagate_otf -> complex (planes, 2, nu, nv); u, v in cycles per sample"""
    from metalens_amd import _lib
    u, v = _lib.f64(u), _lib.f64(v)
    planes = _planes(p)
    out = np.full((planes, 2, u.size, v.size), np.nan + 1j * np.nan)
    _lib.check(p.ctx.lib.ml_propagate_otf(p.ctx.handle, source, p.x.size, p.y.size, planes, _lib.dptr(u), u.size, _lib.dptr(v), v.size,
                                          _lib.dptr(out)))
    return out


CORNERS = [0.0, 0.5, -0.5, THIRD, -THIRD, 0.1, -0.1]


def _thin(n_targets, u, v):
    """-> index arrays into u and v: all of them, or - so that the yardstick has at most 2^20 terms - the corner values
    (0, +-0.5, +-1/3, +-0.1, the repeat included) wherever they stand and every k-th of the others"""
    k = 1
    while True:
        iu, iv = (np.nonzero(np.isin(f, CORNERS) | (np.arange(len(f)) % k == 0))[0] for f in (u, v))
        if n_targets * iu.size * iv.size <= 2 ** 20 or k > 64:
            return iu, iv
        k += 1


def _check_plane(got, I, Sz, scale, u, v, want_h, from_sums=False):
    """one plane's (2, nu, nv) against the yardstick -> the worst ratio of an error to its bound"""
    iu, iv = _thin(I.size, u, v)
    want = oref.otf(I, Sz if want_h else None, u[iu], v[iv], scale=scale if want_h else None)
    slack, worst = I.size + (80 if from_sums else 96), 0.0
    for w, name in enumerate(('I', 'Sz')):
        g = got[w][np.ix_(iu, iv)]
        if name == 'Sz' and not want_h:
            assert not got[w].any()
            continue
        O, abs_re, abs_im = want[name]
        for err, mag in ((np.abs(g.real - O.real), abs_re), (np.abs(g.imag - O.imag), abs_im)):
            bound = slack * U * mag
            assert (err <= bound).all(), (name, float((err - bound).max()))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    return worst


# ---- parity: every case, every frequency set, fields and sums -------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_entries_against_the_yardstick(ma, ctx, name):
    method, mx, my, want_h = CASES[name]
    p = _make(ma, ctx, name)
    d = p.propagate()
    arrays = _plane_arrays(p, d, want_h)
    fields = {}
    for key, (u, v) in FREQS.items():
        got = fields[key] = _raw(p, u, v)
        assert got.shape == (_planes(p), 2, u.size, v.size) and got.tobytes() == _raw(p, u, v).tobytes()          # two calls: the same bits
        worst = max(_check_plane(got[q], I, Sz, scale, u, v, want_h) for q, (I, Sz, scale) in enumerate(arrays))
        print('PARITY otf %-16s fields %-5s: worst error / bound %.4f' % (name, key, worst))
    # the sums of the same pass with weight 1: the stored doubles are the weights
    p.accumulate([1.0], reset=True)
    I_sum, Sz_sum = p.sums()
    shape = (_planes(p), mx, my)
    for key, (u, v) in FREQS.items():
        got = _raw(p, u, v, source=-1)
        assert got.tobytes() == _raw(p, u, v, source=-1).tobytes()
        worst = max(_check_plane(got[q], I_sum.reshape(shape)[q], Sz_sum.reshape(shape)[q] if want_h else None, None, u, v, want_h,
                                 from_sums=True) for q in range(shape[0]))
        print('PARITY otf %-16s sums   %-5s: worst error / bound %.4f' % (name, key, worst))
        assert np.array_equal(got[:, 0], fields[key][:, 0])          # the stored I of one member with weight 1 is the pass's own


# ---- the phasors ----------------------------------------------------------------------------------------------
def test_phasors_within_16_u(ctx):
    from metalens_amd import _lib
    from test_propagate_otf_host import FRACTION_I, FRACTION_U
    rng = np.random.default_rng(23)
    u = np.concatenate([rng.uniform(-0.5, 0.5, 2 ** 16), np.repeat(FRACTION_U, len(FRACTION_I))])
    i = np.concatenate([rng.integers(0, 2 ** 25, 2 ** 16), np.tile(FRACTION_I, len(FRACTION_U))]).astype(np.int32)
    u = _lib.f64(u)
    s, c = np.full(u.size, np.nan), np.full(u.size, np.nan)
    _lib.check(ctx.lib.ml_math_probe(ctx.handle, OTF_PHASOR, _lib.dptr(u), _lib.iptr(i), u.size, _lib.dptr(s), _lib.dptr(c), None))
    s_w, c_w = oref.phasor(u, i)
    es, ec = np.abs(s - s_w).max(), np.abs(c - c_w).max()
    print('PARITY otf phasor n %d: worst |sin - exact| %.2f u, |cos - exact| %.2f u (held to 16 u)' % (u.size, es / U, ec / U))
    assert es <= 16 * U and ec <= 16 * U
    with pytest.raises(_lib.MetalensHipError, match='needs the indices kq'):
        _lib.check(ctx.lib.ml_math_probe(ctx.handle, OTF_PHASOR, _lib.dptr(u), None, 4, _lib.dptr(s), _lib.dptr(c), None))
    with pytest.raises(_lib.MetalensHipError, match='out1 is NULL'):
        _lib.check(ctx.lib.ml_math_probe(ctx.handle, OTF_PHASOR, _lib.dptr(u), _lib.iptr(i), 4, _lib.dptr(s), None, None))


# ---- bit invariances ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['stack-13x11-EH', 'stack-13x11-E'])
def test_a_plane_of_the_stack_has_the_bits_of_the_plane_alone(ma, ctx, name):
    p = _make(ma, ctx, name)
    p.queue_sets(0, 1)
    of_fields = {key: _raw(p, *FREQS[key]) for key in ('5x1', '3x64', '64x64')}
    p.accumulate([0.75], reset=True)
    of_sums = {key: _raw(p, *FREQS[key], source=-1) for key in of_fields}
    assert not np.array_equal(of_fields['3x64'][0], of_fields['3x64'][1]) and not np.array_equal(of_fields['3x64'][1], of_fields['3x64'][2])
    for q in range(3):
        one = _make(ma, ctx, name, method='fft-fine', z=q)
        one.queue_sets(0, 1)
        for key in of_fields:
            assert _raw(one, *FREQS[key])[0].tobytes() == of_fields[key][q].tobytes(), (q, key)
        one.accumulate([0.75], reset=True)
        for key in of_fields:
            assert _raw(one, *FREQS[key], source=-1)[0].tobytes() == of_sums[key][q].tobytes(), (q, key)


@pytest.mark.parametrize('name', ['fft-70x61-EH', 'direct-21x17-EH', 'stack-13x11-E'])
def test_an_entry_does_not_depend_on_the_others_of_its_call(ma, ctx, name):
    p = _make(ma, ctx, name)
    p.queue_sets(0, 1)
    u, v = FREQS['64x64']
    # (above 8 frequencies along y a workgroup takes four rows, up to 8 one: the calls below cross both launches)
    full = _raw(p, u, v)
    rng = np.random.default_rng(41)
    for a, b in [(0, 0), (63, 63), (17, 40), (5, 63), (63, 2)] + [tuple(rng.integers(0, 64, 2)) for _ in range(3)]:
        assert _raw(p, u[a:a + 1], v[b:b + 1])[:, :, 0, 0].tobytes() == np.ascontiguousarray(full[:, :, a, b]).tobytes(), (a, b)
    pu, pv = rng.permutation(64), rng.permutation(64)
    assert np.array_equal(_raw(p, u[pu], v[pv]), full[:, :, pu][:, :, :, pv])
    sub_u, sub_v = np.array([3, 60, 3, 31, 8]), np.array([9, 1, 50, 22, 63, 9, 40])          # 5 x 7, with repeats
    assert np.array_equal(_raw(p, u[sub_u], v[sub_v]), full[:, :, sub_u][:, :, :, sub_v])
    assert np.array_equal(_raw(p, u[:17], v[:33]), full[:, :, :17, :33])                       # a batch of 32 and one more
    for nv in (8, 9, 16, 17):                                                                   # either side of the two launches
        assert np.array_equal(_raw(p, u[:2], v[:nv]), full[:, :, :2, :nv]), nv


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_members_of_a_pass(ma, ctx, want_h):
    """members 0 to 2 of a ``propagate_sets`` pass: each against the yardstick on its downloaded fields, and with the bits of
    ``propagate()`` on that set alone"""
    from metalens_amd import _lib
    x, y, n_glass = _dipole_batch(ma, ctx)
    tx = x.mean() + (np.arange(21) - 10) * 0.37e-6
    ty = y.mean() + (np.arange(17) - 8) * 0.37e-6
    p = ma.PlanePropagator(x, y, WL, n_glass, tx, ty, 20e-6, want_h=want_h, ctx=ctx)
    sets = p.propagate_sets()
    assert len(sets) == 3
    u, v = FREQS['3x64']
    got = [_raw(p, u, v, source=m) for m in range(3)]
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    worst = 0.0
    for m in range(3):
        (I, Sz, scale), = _plane_arrays(p, sets[m], want_h)
        worst = max(worst, _check_plane(got[m][0], I, Sz, scale, u, v, want_h))
    print('PARITY otf members %s 3x64: worst error / bound %.4f' % ('EH' if want_h else 'E', worst))
    with pytest.raises(_lib.MetalensHipError, match='ml_propagate_otf: member 3 asked for, the last pass propagated 3 field sets'):
        p.otf([0.0], [0.0], member=3)
    for m in range(3):
        _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
        p.propagate()
        assert _raw(p, u, v).tobytes() == got[m].tobytes(), m
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))


# ---- state: nothing else moves --------------------------------------------------------------------------------
def test_state_and_refusals(ma, ctx):
    from metalens_amd import _lib
    from metalens_amd.propagate import plan_info
    p = _make(ma, ctx, 'direct-21x17-EH')
    f = [0.0, 0.1 / _pitch(p)[0]]
    with pytest.raises(_lib.MetalensHipError, match='ml_propagate has not run on the active propagation plan'):
        p.otf(f, f)
    d = p.propagate()
    with pytest.raises(_lib.MetalensHipError, match='ml_propagate_accumulate has not run on the active propagation plan'):
        p.otf(f, f, of='sums')
    p.accumulate([2.0], reset=True)
    sums, info = p.sums(), plan_info(ctx)
    radii = (np.arange(5) + 0.5) * _pitch(p)[0]
    focus, focus_sums = p.focus(radii), p.focus(radii, of='sums')
    u, v = FREQS['3x64']
    before, before_sums = _raw(p, u, v), _raw(p, u, v, source=-1)
    # refusals of the entry: each with its numbers
    out = np.empty((1, 2, 64, 64), dtype=np.complex128)
    du, dv, do = _lib.dptr(_lib.f64(u)), _lib.dptr(_lib.f64(v)), _lib.dptr(out)
    high, odd = _lib.f64([0.0, 0.5000000000000001]), _lib.f64([0.0, 0.1, np.nan])
    h = ctx.handle
    for args, said in (((1, 21, 17, 1, du, 3, dv, 64, do), 'ml_propagate_otf: member 1 asked for, the last pass propagated 1 field sets'),
                       ((-2, 21, 17, 1, du, 3, dv, 64, do), 'source -2'),
                       ((0, 17, 17, 1, du, 3, dv, 64, do), '1 planes of 17 x 17 targets are 289 targets, the active propagation plan has 357'),
                       ((0, 21, 17, 2, du, 3, dv, 64, do), '2 planes of 21 x 17'),
                       ((0, 21, 17, 1, du, 0, dv, 64, do), '0 x 64 frequencies: 1 to 64 are taken per axis'),
                       ((0, 21, 17, 1, du, 3, dv, 65, do), '3 x 65 frequencies'),
                       ((0, 21, 17, 1, None, 3, dv, 64, do), 'NULL argument (u NULL, v given, otf given)'),
                       ((0, 21, 17, 1, du, 3, None, 64, do), 'NULL argument (u given, v NULL, otf given)'),
                       ((0, 21, 17, 1, du, 3, dv, 64, None), 'NULL argument (u given, v given, otf NULL)'),
                       ((0, 21, 17, 1, _lib.dptr(high), 2, dv, 64, do), 'u[1] = 0.50000000000000011: a frequency is finite and within +-0.5'),
                       ((-1, 21, 17, 1, du, 3, _lib.dptr(odd), 3, do), 'v[2] = nan')):
        assert ctx.lib.ml_propagate_otf(h, *args) == -1          # ML_EINVAL
        assert said in ctx.lib.ml_last_error().decode(), said
    with pytest.raises(ValueError, match='lies beyond the Nyquist frequency'):
        p.otf([0.0, 1 / _pitch(p)[0]], f)
    # accepted and refused calls have left the fields, the sums, the focus records, the plan and their own numbers alone
    for key, value in p._download(None).items():
        assert np.array_equal(value, d[key]), key
    for got, want in zip(p.sums(), sums):
        assert np.array_equal(got, want)
    assert plan_info(ctx) == info
    for again, first in ((p.focus(radii), focus), (p.focus(radii, of='sums'), focus_sums)):
        assert set(again) == set(first) and all(np.array_equal(again[k], first[k]) for k in first)
    assert _raw(p, u, v).tobytes() == before.tobytes() and _raw(p, u, v, source=-1).tobytes() == before_sums.tobytes()
    assert all(np.array_equal(value, d[k]) for k, value in p.propagate().items())
    # another propagator plans: this one's otf is refused, as focus and accumulate are
    other = _make(ma, ctx, 'fft-21x17-E')
    with pytest.raises(RuntimeError, match='another propagator has planned'):
        p.otf(f, f)
    with pytest.raises(_lib.MetalensHipError, match='has not run on the active propagation plan'):
        other.otf(f, f)


def test_a_context_of_several_ranks_is_refused(ma, monkeypatch):
    """as every propagation entry: the refusal comes before the state is looked at, so no plan is needed"""
    from metalens_amd import _lib
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        f, out = _lib.f64([0.0]), np.zeros((1, 2, 1, 1), dtype=np.complex128)
        assert c.lib.ml_propagate_otf(c.handle, 0, 21, 17, 1, _lib.dptr(f), 1, _lib.dptr(f), 1, _lib.dptr(out)) == -1          # ML_EINVAL
        assert 'ml_propagate_otf: this context belongs to a communicator of 2 ranks' in c.lib.ml_last_error().decode()
        assert not out.any()
    finally:
        c.close()


# ---- the Python level -----------------------------------------------------------------------------------------
def test_python_dict(ma, ctx):
    name = 'fft-70x61-EH'
    method, mx, my, want_h = CASES[name]
    p = _make(ma, ctx, name)
    p.queue_sets(0, 1)
    dx, dy = _pitch(p)
    u, v = FREQS['5x1'][0], FREQS['1x7'][1]
    fx, fy = u / dx, v / dy
    out = p.otf(fx, fy)
    assert set(out) == {'otf_I', 'mtf_I', 'otf_Sz', 'mtf_Sz', 'fx', 'fy'}
    assert out['otf_I'].shape == out['mtf_Sz'].shape == (1, 5, 7) and out['otf_I'].dtype == np.complex128
    assert np.array_equal(out['fx'], fx) and np.array_equal(out['fy'], fy)
    # the device's numbers scaled (0 is among both axes: nothing is inserted), in the caller's order
    uu, vv = fx * dx, fy * dy
    uu, vv = [np.where(np.abs(np.abs(t) - 0.5) <= 4 * np.spacing(0.5), np.copysign(0.5, t), t) for t in (uu, vv)]
    raw = _raw(p, uu, vv)
    assert np.array_equal(out['otf_I'], raw[:, 0] * (dx * dy)) and np.array_equal(out['otf_Sz'], raw[:, 1] * (dx * dy))
    assert np.array_equal(out['mtf_I'], np.abs(raw[:, 0]) / raw[:, 0, 2, 1].real) and (out['mtf_I'][0, 2, [1, 6]] == 1).all()
    assert (out['mtf_I'] <= 1 + 1e-12).all() and out['mtf_Sz'][0, 2, 1] == 1
    # an axis without 0: it is inserted and stripped - the same bits, by the independence of the entries
    part = p.otf(fx[[1, 4, 0]], fy[[2, 4]])
    assert part['otf_I'].shape == (1, 3, 2) and np.array_equal(part['otf_I'], out['otf_I'][:, [1, 4, 0]][:, :, [2, 4]])
    assert np.array_equal(part['mtf_Sz'], out['mtf_Sz'][:, [1, 4, 0]][:, :, [2, 4]])
    # otf_I(0, 0) is I_dA of focus(): two sums of the same n terms in different orders, each within its bound
    foc = p.focus()
    n = mx * my
    assert abs(out['otf_I'][0, 2, 1].real - foc['I_dA'][0]) <= ((n + 96) + (n + 16) + 8) * U * foc['I_dA'][0] and out['otf_I'][0, 2, 1].imag == 0
    # without H the Sz keys are absent
    pe = _make(ma, ctx, 'fft-21x17-E')
    pe.queue_sets(0, 1)
    assert set(pe.otf(fx, fy)) == {'otf_I', 'mtf_I', 'fx', 'fy'}


def test_centre_removes_the_linear_phase(ma, ctx):
    """About its peak the spot's transfer function has almost no phase at low frequencies.  With phi = 2 pi f (x - xc) over
    the patch, |Im O| <= |sum I phi| + sum I |phi|^3 / 6 and Re O >= sum I (1 - phi^2 / 2); by the moments of ``focus()``,
    sum I phi = 2 pi f S m and sum I phi^2 = (2 pi f)^2 S (s + m^2) with m the centroid's distance from the peak and s the
    central second moment, and |phi|^3 <= phi^2 phi_max with phi_max = 2 pi f L, L the patch's reach from the peak:
        |arg O| <= atan((g |m| + g^2 (s + m^2) phi_max / 6) / (1 - g^2 (s + m^2) / 2)),  g = 2 pi f
    plus 1e-9 for the arithmetic.  At f = 1 / (64 dx), a quarter of the patch's own lowest frequency, that is a few hundredths
    of a radian; about the first target the same entry has the phase -2 pi f (xc - x[0]), half a radian."""
    name = 'stack-13x11-EH'
    p = _make(ma, ctx, name)
    p.queue_sets(0, 1)
    dx, dy = _pitch(p)
    foc = p.focus()
    fx, fy = np.array([0.0, 1 / (64 * dx), -1 / (64 * dx)]), np.array([1 / (64 * dy), 0.0])
    about_peak, about_origin = p.otf(fx, fy, centre='peak'), p.otf(fx, fy)
    assert np.array_equal(about_peak['mtf_I'], about_origin['mtf_I'])
    given = p.otf(fx, fy, centre=foc['peak_xy'])          # (planes, 2)
    assert np.array_equal(given['otf_I'], about_peak['otf_I']) and np.array_equal(given['otf_Sz'], about_peak['otf_Sz'])
    one = p.otf(fx, fy, centre=tuple(foc['peak_xy'][0]))          # every plane's peak lies on the axis
    assert np.array_equal(one['otf_I'], about_peak['otf_I'])
    for q in range(3):
        for (a, b), f, axis, d in (((1, 1), fx[1], 0, dx), ((2, 1), -fx[2], 0, dx), ((0, 0), fy[0], 1, dy)):
            t = (p.x, p.y)[axis]
            g = 2 * np.pi * f
            m = foc['centroid_I'][q, axis] - foc['peak_xy'][q, axis]
            m2 = foc['second_moments_I'][q, axis] + m * m
            reach = max(foc['peak_xy'][q, axis] - t[0], t[-1] - foc['peak_xy'][q, axis])
            tol = np.arctan((g * abs(m) + g * g * m2 * (g * reach) / 6) / (1 - g * g * m2 / 2)) + 1e-9
            assert abs(np.angle(about_peak['otf_I'][q, a, b])) <= tol, (q, a, b)
            turn = 2 * np.pi * f * (foc['peak_xy'][q, axis] - t[0])
            assert turn > 3 * tol and abs(abs(np.angle(about_origin['otf_I'][q, a, b])) - turn) <= tol


def test_through_the_sweep(ma, ctx):
    from test_gpu_propagate_sets import _common, _lens
    lens = _lens()
    x, y = _window()
    uu = np.linspace(-0.2, 0.2, 24)
    sw = ma.SourceSweep(*_common(lens), x, y, uu, uu, ctx=ctx)
    tx = x.mean() + (np.arange(21) - 10) * 0.37e-6
    ty = y.mean() + (np.arange(17) - 8) * 0.37e-6
    p = ma.PlanePropagator(x, y, WL, sw.n_glass, tx, ty, 20e-6, ctx=ctx)
    f = lens['source_distance']
    sources = [(0.3e-6, -0.2e-6, -f, pol) for pol in 'xyz'] + [(-1.0e-6, 0.5e-6, -1.05 * f, 'x')]
    weights = np.array([1.0, 0.5, 2.0, 1.5])
    dx, dy = _pitch(p)
    freqs = (np.array([2e5, 0.0, -1e6, 1 / (2 * dx)]), np.array([3e5, -3e5, 1.1e6]))
    plain = sw.run(sources, weights=weights, image=p)
    got = sw.run(sources, weights=weights, image=p, image_freqs=freqs)
    assert set(got) == set(plain) | {'image_otf'}
    for key in plain:
        assert np.array_equal(got[key], plain[key], equal_nan=True), key
    want = p.otf(*freqs, of='sums', centre='peak')
    assert set(want) == set(got['image_otf']) == {'otf_I', 'mtf_I', 'otf_Sz', 'mtf_Sz', 'fx', 'fy'}
    assert all(got['image_otf'][k].tobytes() == want[k].tobytes() for k in want)
    assert got['image_otf']['otf_I'].shape == (1, 4, 3) and got['image_otf']['mtf_I'][0, 1].max() <= 1
    # against the yardstick on the returned maps, about the first target
    u, v = freqs[0] * dx, freqs[1] * dy
    u[3] = 0.5
    raw = _raw(p, u, np.concatenate([[0.0], v]), source=-1)
    print('PARITY otf sweep sums 4x4: worst error / bound %.4f'
          % _check_plane(raw[0], got['I_sum'], got['Sz_sum'], None, u, np.concatenate([[0.0], v]), True, from_sums=True))
    origin = sw.run(sources, weights=weights, image=p, image_freqs=freqs, image_centre=(tx[0], ty[0]))['image_otf']
    assert np.array_equal(origin['otf_I'], raw[:, 0, :, 1:] * (dx * dy))
    both = sw.run(sources, weights=weights, image=p, image_freqs=iter(freqs), image_radii=[1e-6])          # (taken once)
    assert both['image_otf']['otf_Sz'].tobytes() == want['otf_Sz'].tobytes() and 'focus_efficiency' in both
