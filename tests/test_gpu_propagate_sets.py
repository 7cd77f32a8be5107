"""Several resident field sets propagated to an image plane in ONE pass (csrc/propagate.hip propagate_kernel<WANT_H, NS>,
ml_propagate_sets), their intensity sums kept on the GPU (ml_propagate_accumulate) and ``SourceSweep.run(image=...)``.
Needs an MI355X.

The lens is the one of test_gpu_propagate.test_resident_equals_uploaded (centre disc to r = 21.9 um, rings to
R = 60.6 um).  The aperture WINDOWS are chosen for where the kernel can go wrong:

* ``A``, 96 x 130 samples: one LDS tile of 128 samples plus a tail of 2; x from 38 to 63 um, so it crosses ring
  boundaries and the lens edge - its last rows lie outside the lens altogether, the rows before them carry row
  extents, the others are summed whole;
* ``B``, 61 x 80: less than one tile and an odd row count; it straddles the edge of the centre disc and the first
  rings.

No window of these sizes reaches from the centre disc to outside the lens (38.7 um apart; the windows span 25 x 34 um
at the pitch lambda / 2.2), so the two share the regions between them.

Bounds.  Fields: equality with the single-set path (the pass is required to give its bits).  Against the long-double
sum: the rule of test_gpu_propagate.py, GPU error <= 8 x the plain-fp64 NumPy sum's own.  Sums, with n sources:
|I - I_ref| <= (n + 8) 2^-52 I_ref and |Sz - Sz_ref| <= (n + 8) 2^-52 sum_m w_m (|Ex||Hy| + |Ey||Hx|) / 2, I_ref and
Sz_ref restated in NumPy in the kernel's order of operations from the per-source fields."""
import functools

import numpy as np
import pytest

import propagate_ref as ref
from test_gpu_propagate import _target_set

pytestmark = pytest.mark.gpu

WL = ref.WL
PITCH = WL / 2.2
WINDOWS = {'A': (96, 130, 50.5e-6, 1.0e-6), 'B': (61, 80, 20.0e-6, -6.0e-6)}
DIPOLES = ('dipoles', (0.3e-6, -0.2e-6, None), 'xyz')      # NS = 3 (z: the lens' source distance)
PLANE_WAVES = ('plane waves', (0.0, 0.0, -float('inf')), 'xy')   # NS = 2
# NS = 2 where the lens takes no plane wave: normal incidence lies outside the direction range of the outer rings'
# tables (window A: "need to calculate at smaller ux!", as the reference raises it)
TWO_DIPOLES = ('two dipoles', (0.3e-6, -0.2e-6, None), 'xy')
EPS = 2.0 ** -52


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
def _lens():
    from test_gpu_parity import _synthetic_lens
    return _synthetic_lens(60e-6, 0.4, WL, switch_deg=9.0)


def _common(lens):
    return (WL, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'])


def _window(name):
    nx, ny, cx, cy = WINDOWS[name]
    return cx + (np.arange(nx) - (nx - 1) / 2) * PITCH, cy + (np.arange(ny) - (ny - 1) / 2) * PITCH


def _batch(ma, ctx, window, batch):
    """synthesise the batch on the window: its members become the resident field sets -> x, y, n_glass, n"""
    from metalens_amd import _lib
    from metalens_amd.nearfield import nearfield_params
    lens = _lens()
    x, y = _window(window)
    _, (sx, sy, sz), pols = batch
    sz = -lens['source_distance'] if sz is None else sz
    # tables, layout and the grid's tie answers become resident through the drop-in call
    n_glass = ma.build_nearfield(sx, sy, sz, pols[0], *_common(lens), x_pts=x, y_pts=y, ctx=ctx, download=False)[7]
    params = (_lib.NearfieldParams * len(pols))()
    for m, pol in enumerate(pols):
        params[m] = nearfield_params(sx, sy, sz, pol, WL, n_glass, 1e-30, ma.constants.c0, ma.constants.Z0)
    xs, ys = _lib.f64(x), _lib.f64(y)
    _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, len(pols), _lib.dptr(xs), xs.size,
                                                _lib.dptr(ys), ys.size))
    return x, y, n_glass, len(pols)


def _targets(kind, x, y):
    """'points': the 300-point list of test_gpu_propagate (its second workgroup: 44 live lanes, one live wave, three
    dead ones); 'plane': 80 x 80 = 25 target tiles, splits = 82 < 96 rows - some workgroups sum two rows"""
    if kind == 'points':
        tx, ty, tz, _ = _target_set('points', x, y)
        return (tx, ty, tz), dict(point_list=True)
    return ((x.mean() + np.linspace(-0.6, 0.55, 80) * np.ptp(x), y.mean() + np.linspace(-0.5, 0.6, 80) * np.ptp(y), 20e-6),
            dict(point_list=False))


def _keys(want_h):
    return ('Ex', 'Ey', 'Ez', 'Hx', 'Hy', 'Hz', 'Sz') if want_h else ('Ex', 'Ey', 'Ez', 'I')


def _same(a, b, want_h):
    assert set(a) == set(b) == set(_keys(want_h))
    for key in a:
        assert np.abs(a[key]).max() > 0, key
        assert np.array_equal(a[key], b[key]), key


def _select(ctx, m):
    from metalens_amd import _lib
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('window,kind,batch', [
    ('A', 'points', DIPOLES), ('B', 'points', DIPOLES), ('A', 'plane', DIPOLES),
    ('B', 'points', PLANE_WAVES), ('B', 'plane', PLANE_WAVES),            # plane waves: where the lens admits them
    ('A', 'points', TWO_DIPOLES), ('A', 'plane', TWO_DIPOLES),            # NS = 2 on the 96-row window
], ids=['A-points-xyz', 'B-points-xyz', 'A-plane-xyz', 'B-points-xy-waves', 'B-plane-xy-waves', 'A-points-xy',
        'A-plane-xy'])
def test_sets_equal_singles_bit_for_bit(ma, ctx, window, kind, batch, want_h):
    x, y, n_glass, n = _batch(ma, ctx, window, batch)
    assert x[-1] > _lens()['lens_periphery_summary']['r_max_list'][-1] or window == 'B'   # A: rows outside the lens
    t, kw = _targets(kind, x, y)
    p = ma.PlanePropagator(x, y, WL, n_glass, *t, want_h=want_h, ctx=ctx, **kw)
    sets = p.propagate_sets()
    assert len(sets) == n
    singles = []
    for m in range(n):
        _select(ctx, m)
        singles.append(p.propagate())
        _same(sets[m], singles[m], want_h)
    # members differ (a pass that read one set n times would pass the loop above only if they did not)
    assert not np.array_equal(singles[0]['Ex'], singles[1]['Ex'])
    # the selected set is still the last one selected, and a sub-range starts where it is told to
    again = p.propagate_sets()
    _same(p.propagate(), singles[n - 1], want_h)
    for m in range(n):
        _same(again[m], singles[m], want_h)
    one = p.propagate_sets(first=n - 1, n=1)
    assert len(one) == 1
    _same(one[0], singles[n - 1], want_h)
    if n == 3:
        tail = p.propagate_sets(first=1, n=2)
        assert len(tail) == 2
        _same(tail[0], singles[1], want_h)
        _same(tail[1], singles[2], want_h)
        assert len(p.propagate_sets(first=1)) == 2
    # out of range: refused, nothing propagated
    from metalens_amd import _lib
    for first, count in ((0, n + 1), (n, 1), (-1, 1), (0, 0), (0, 4)):
        with pytest.raises(_lib.MetalensHipError):
            p.propagate_sets(first=first, n=count)
    _select(ctx, 0)


def test_against_the_long_double_direct_sum(ma, ctx):
    """window B, the x / y / z batch, 40 of the 300 points: every set within 8 x e_ref, E and H"""
    from metalens_amd import _lib
    x, y, n_glass, n = _batch(ma, ctx, 'B', DIPOLES)
    tx, ty, tz, _ = _target_set('points', x, y)
    sub = np.arange(0, 300, 7)[:40]
    assert sub.size == 40
    tx, ty, tz = tx[sub], ty[sub], tz[sub]
    pts = np.stack([tx, ty, tz], axis=1)
    p = ma.PlanePropagator(x, y, WL, n_glass, tx, ty, tz, point_list=True, ctx=ctx)
    sets = p.propagate_sets()
    for m in range(n):
        _select(ctx, m)
        F = [np.empty((x.size, y.size), dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
        assert min(np.abs(f).max() for f in F) > 0
        E64, H64 = ref.direct_sum(*F, x, y, WL, n_glass, pts, Z0=p.Z0)
        El, Hl = ref.direct_sum(*F, x, y, WL, n_glass, pts, Z0=p.Z0, real=np.longdouble)
        for name, keys, f64, fl in (('E', ('Ex', 'Ey', 'Ez'), E64, El), ('H', ('Hx', 'Hy', 'Hz'), H64, Hl)):
            e_ref = ref.max_error(f64, fl)
            e_gpu = ref.max_error(np.stack([sets[m][k] for k in keys]), fl)
            print('PARITY sets 61x80 xyz member %d %s: e_ref %.3e gpu %.3e' % (m, name, e_ref, e_gpu))
            assert e_gpu <= 8 * e_ref, (m, name)
    _select(ctx, 0)


def _intensity(d):
    sq = [d[k].real * d[k].real + d[k].imag * d[k].imag for k in ('Ex', 'Ey', 'Ez')]
    return (sq[0] + sq[1]) + sq[2]


def _sz(d):
    return 0.5 * ((d['Ex'].real * d['Hy'].real + d['Ex'].imag * d['Hy'].imag)
                  - (d['Ey'].real * d['Hx'].real + d['Ey'].imag * d['Hx'].imag))


def _sums_ref(passes, want_h):
    """``passes`` = [[(weight, field dict), ...] per pass] -> I, Sz, Sz's scale: the accumulation kernel's order - a
    pass's weighted terms are added in member order, the pass's sum is then added once to the running sum"""
    I = Sz = scale = None
    for members in passes:
        pI = pS = None
        for w, d in members:
            wi = w * _intensity(d)
            pI = wi if pI is None else pI + wi
            if want_h:
                ws = w * _sz(d)
                pS = ws if pS is None else pS + ws
                s = w * 0.5 * (np.abs(d['Ex']) * np.abs(d['Hy']) + np.abs(d['Ey']) * np.abs(d['Hx']))
                scale = s if scale is None else scale + s
        I = pI if I is None else I + pI
        if want_h:
            Sz = pS if Sz is None else Sz + pS
    return I, Sz, scale


def _check_sums(I, Sz, passes, want_h):
    n = sum(len(members) for members in passes)
    I_ref, Sz_ref, scale = _sums_ref(passes, want_h)
    assert I.shape == I_ref.shape and I_ref.min() > 0
    err = np.abs(I - I_ref) / I_ref
    print('SUMS n = %d: I off by %.2f x 2^-52 at most (bound %d)' % (n, err.max() / EPS, n + 8))
    assert (np.abs(I - I_ref) <= (n + 8) * EPS * I_ref).all()
    if want_h:
        assert Sz.shape == Sz_ref.shape and np.abs(Sz_ref).max() > 0
        print('SUMS n = %d: Sz off by %.2f x 2^-52 of its scale at most' % (n, (np.abs(Sz - Sz_ref) / scale).max() / EPS))
        assert (np.abs(Sz - Sz_ref) <= (n + 8) * EPS * scale).all()
    else:
        assert Sz is None


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_sums(ma, ctx, want_h):
    from metalens_amd import _lib
    x, y, n_glass, n = _batch(ma, ctx, 'A', DIPOLES)
    t, kw = _targets('points', x, y)
    p = ma.PlanePropagator(x, y, WL, n_glass, *t, want_h=want_h, ctx=ctx, **kw)
    weights = np.array([1.0, 0.5, 2.0])
    with pytest.raises(_lib.MetalensHipError, match='has not run on the active propagation plan'):
        p.sums()
    sets = p.propagate_sets()
    with pytest.raises(_lib.MetalensHipError, match='reset = 1'):   # nothing to add to yet
        p.accumulate(weights, reset=False)
    p.accumulate(weights, reset=True)
    I1, Sz1 = p.sums()
    _check_sums(I1, Sz1, [list(zip(weights, sets))], want_h)
    # an E-only plan has no Sz to hand out
    if not want_h:
        buf, buf2 = np.empty(p.shape), np.empty(p.shape)
        assert ctx.lib.ml_propagate_sums(ctx.handle, _lib.dptr(buf), _lib.dptr(buf2)) != 0
    # the same pass added a second time: every addend doubles, exactly
    p.accumulate(weights, reset=True)
    p.accumulate(weights, reset=False)
    I2, Sz2 = p.sums()
    assert np.array_equal(I2, 2 * I1)
    if want_h:
        assert np.array_equal(Sz2, 2 * Sz1)
    # reset starts over; fewer members than the pass holds; a second pass on top of the first
    p.accumulate(weights[:2], reset=True)
    I3, Sz3 = p.sums()
    _check_sums(I3, Sz3, [list(zip(weights[:2], sets[:2]))], want_h)
    tail = p.propagate_sets(first=2, n=1)
    p.accumulate(weights[2:], reset=False)
    I4, Sz4 = p.sums()
    _check_sums(I4, Sz4, [list(zip(weights[:2], sets[:2])), [(weights[2], tail[0])]], want_h)
    with pytest.raises(_lib.MetalensHipError):   # the last pass holds one set
        p.accumulate(weights, reset=False)


def _same_far_field(a, b):
    for key in ('P_sum', 'total_P', 'power_in'):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


SWEEP_WEIGHTS = np.array([1.0, 0.5, 2.0, 1.5, 0.7])


def _sweep_sources(lens):
    """five sources: x, y, z at one position (a polarisation batch), then two single sources at two other positions
    (merged into one position batch)"""
    f = lens['source_distance']
    return [(0.3e-6, -0.2e-6, -f, 'x'), (0.3e-6, -0.2e-6, -f, 'y'), (0.3e-6, -0.2e-6, -f, 'z'),
            (-1.0e-6, 0.5e-6, -1.05 * f, 'x'), (0.6e-6, 0.9e-6, -0.97 * f, 'y')]


def _sweep_with_image(ma, ctx):
    lens = _lens()
    x, y = _window('A')
    u = np.linspace(-0.2, 0.2, 24)
    sw = ma.SourceSweep(*_common(lens), x, y, u, u, ctx=ctx)
    t, kw = _targets('points', x, y)
    p = ma.PlanePropagator(x, y, WL, sw.n_glass, *t, ctx=ctx, **kw)
    return sw, p, _sweep_sources(lens), t, kw


def test_through_the_sweep(ma, ctx):
    sw, p, sources, t, kw = _sweep_with_image(ma, ctx)
    weights = SWEEP_WEIGHTS
    groups = sw._group(sources)
    assert [len(g['members']) for g in groups] == [3, 2] and groups[1].get('mixed')
    plain = sw.run(sources, weights=weights)
    assert 'I_sum' not in plain and 'Sz_sum' not in plain
    got = sw.run(sources, weights=weights, image=p, keep_each=True)
    _same_far_field(got, plain)
    each = got['image_each']
    assert len(each) == 5 and got['I_sum'].shape == got['Sz_sum'].shape == p.shape == (300,)
    passes = [[(weights[k], each[k]) for k in (0, 1, 2)], [(weights[k], each[k]) for k in (3, 4)]]
    _check_sums(got['I_sum'], got['Sz_sum'], passes, True)
    # every source's image is what propagate() gives for its field set of the group's batch
    for k in range(5):
        assert set(each[k]) == set(_keys(True)) and np.abs(each[k]['Ex']).max() > 0
    # E only: no Sz_sum; and queue() leaves the sums on the GPU
    x, y = _window('A')
    pe = ma.PlanePropagator(x, y, WL, sw.n_glass, *t, want_h=False, ctx=ctx, **kw)
    got_e = sw.run(sources, weights=weights, image=pe)
    assert 'Sz_sum' not in got_e and 'image_each' not in got_e
    _same_far_field(got_e, plain)
    _check_sums(got_e['I_sum'], None, passes, False)
    sw.queue(sources, image=pe)
    ctx.sync()
    _check_sums(pe.sums()[0], None, [[(1.0, each[k]) for k in (0, 1, 2)], [(1.0, each[k]) for k in (3, 4)]], False)


def test_sweep_images_equal_the_sources_alone(ma, ctx):
    """``image_each[k]`` against a fresh ``build_nearfield(download=False)`` + ``field_at_plane(None, ...)`` of source k
    alone, by ``array_equal``, for all five sources.

    The near field of a member synthesised in its polarisation batch differs from the same source synthesised alone
    (measured here: in 37 751-39 149 of the 4 x 12 480 samples, by up to 4.2e-16 of the field's scale - test_gpu_parity
    allows 1e-14 there and asserts equality only for position batches), which showed as 257-298 of 300 differing
    elements per key, 4.7e-16 ... 2.2e-15 of the peak, in the images of sources 0-2.  With ``image=`` the sweep therefore
    writes such a group's field sets once more through the single-source kernels (ml_nearfield_members_async) before it
    propagates them; the far-field sums and the incident powers stay the batch's (test_through_the_sweep)."""
    sw, p, sources, t, kw = _sweep_with_image(ma, ctx)
    x, y = _window('A')
    each = sw.run(sources, weights=SWEEP_WEIGHTS, image=p, keep_each=True)['image_each']
    alone = []
    for k, (sx, sy, sz, pol) in enumerate(sources):
        res = ma.build_nearfield(sx, sy, sz, pol, *_common(_lens()), x_pts=x, y_pts=y, ctx=ctx, download=False)
        alone.append(ma.field_at_plane(None, None, None, None, res[4], res[5], WL, res[7], *t, ctx=ctx, **kw))
        for key in alone[k]:
            a, b = each[k][key], alone[k][key]
            print('SWEEP source %d %-2s: %3d of %d elements differ, max |diff| / max |.| %.3e'
                  % (k, key, np.count_nonzero(a != b), a.size, np.abs(a - b).max() / np.abs(b).max()))
    for k in (3, 4, 0, 1, 2):
        _same(each[k], alone[k], True)


def test_members_alone_synthesis_gives_the_bits_of_single_calls(ma, ctx):
    """ml_nearfield_members_async on a one-position batch: every field set equals the drop-in call of its member, and
    with keep_powers the incident powers stay those of the batch before it"""
    from metalens_amd import _lib
    from metalens_amd.nearfield import nearfield_params
    lens = _lens()
    x, y, n_glass, n = _batch(ma, ctx, 'B', DIPOLES)
    _, (sx, sy, _), pols = DIPOLES
    sz = -lens['source_distance']
    pw = np.zeros(n)
    _lib.check(ctx.lib.ml_nearfield_powers(ctx.handle, _lib.dptr(pw), n))
    params = (_lib.NearfieldParams * n)()
    for m, pol in enumerate(pols):
        params[m] = nearfield_params(sx, sy, sz, pol, WL, n_glass, 1e-30, ma.constants.c0, ma.constants.Z0)
    xs, ys = _lib.f64(x), _lib.f64(y)
    grid = (_lib.dptr(xs), xs.size, _lib.dptr(ys), ys.size)
    assert ctx.lib.ml_nearfield_members_async(ctx.handle, params, 2, *grid, 1) != 0    # not the resident batch
    _lib.check(ctx.lib.ml_nearfield_members_async(ctx.handle, params, n, *grid, 1))
    kept = np.zeros(n)
    _lib.check(ctx.lib.ml_nearfield_powers(ctx.handle, _lib.dptr(kept), n))
    assert pw.min() > 0 and np.array_equal(kept, pw)
    got = []
    for m in range(n):
        _select(ctx, m)
        F = [np.empty((x.size, y.size), dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
        got.append(F)
    _lib.check(ctx.lib.ml_nearfield_members_async(ctx.handle, params, n, *grid, 0))
    own = np.zeros(n)
    _lib.check(ctx.lib.ml_nearfield_powers(ctx.handle, _lib.dptr(own), n))
    for m, pol in enumerate(pols):
        single = ma.build_nearfield(sx, sy, sz, pol, *_common(lens), x_pts=x, y_pts=y, ctx=ctx)
        for g, w in zip(got[m], single[:4]):
            assert np.abs(w).max() > 0 and np.array_equal(g, w), (m, pol)
        # (the bound test_gpu_parity.test_position_batch_equals_single_sources sets for the same comparison)
        assert abs(own[m] * (x[1] - x[0]) * (y[1] - y[0]) - single[6]) <= 1e-13 * abs(single[6])


def test_the_repeated_first_pass_counts_once(ma, ctx, monkeypatch):
    """an odd symmetric grid (the smallest of test_nearest_cell_ties_follow_ckdtree): nearest-cell ties are reported,
    settled, and the first group's pass runs again - its image must be in the sums once"""
    from metalens_amd import ties
    lens = _lens()
    f = lens['source_distance']
    n = 61
    x = (np.arange(n) - n // 2) * PITCH
    assert x[n // 2] == 0.0
    u = np.linspace(-0.1, 0.1, 16)
    sources = [(0.4e-6, -0.3e-6, -f, pol) for pol in 'xyz']
    weights = np.array([1.0, 0.5, 2.0])
    # a context of its own: no tie answers for this grid are resident yet
    from metalens_amd import _lib
    own = _lib.Context(0)
    try:
        sw = ma.SourceSweep(*_common(lens), x, x, u, u, ctx=own)
        tx, ty, tz, _ = _target_set('points', x, x)
        p = ma.PlanePropagator(x, x, WL, sw.n_glass, tx[:40], ty[:40], tz[:40], point_list=True, ctx=own)
        passes, pending = [], []
        real_pass = sw._pass

        def counted(group, *a, **k):
            out = real_pass(group, *a, **k)
            passes.append(len(group['members']))
            pending.append(ties.pending(own).size)
            return out
        monkeypatch.setattr(sw, '_pass', counted)
        got = sw.run(sources, weights=weights, image=p, keep_each=True)
        assert passes[0] == 3 and len(passes) >= 2 and pending[0] > 0 and pending[-1] == 0   # ties, and a repeat
        each = got['image_each']
        _check_sums(got['I_sum'], got['Sz_sum'], [[(weights[k], each[k]) for k in range(3)]], True)
        twice = 2 * _sums_ref([[(weights[k], each[k]) for k in range(3)]], True)[0]
        assert (np.abs(got['I_sum'] - twice) > 0.4 * twice).all()
    finally:
        own.close()


def test_state_is_left_alone(ma, ctx):
    """the far-field side of a shared context does not notice a pass and its accumulation; sums do not outlive
    their plan"""
    from metalens_amd import _lib
    from test_gpu_fft import fields
    from test_gpu_fft_mixed import _axes, _upload
    nx, ny = 130, 61
    x, y = _axes(nx, ny)
    F = fields(nx, ny, 21)
    ux, uy = np.linspace(-0.3, 0.3, 20), np.linspace(-0.2, 0.22, 24)
    ctx.set_method('gemm')
    t = ma.FarfieldTransform(nx, ny, x[1] - x[0], y[1] - y[0], WL, ref.N_GLASS, ux, uy, ctx=ctx)
    _upload(ctx, F)
    t.transform()
    vectors, proj = t.radiation_vectors(), t.project()
    tx, ty, tz, _ = _target_set('points', x, y)
    p1 = ma.PlanePropagator(x, y, WL, ref.N_GLASS, tx, ty, tz, point_list=True, ctx=ctx)
    sets = p1.propagate_sets()
    assert len(sets) == 1                       # an uploaded field is one set
    _same(sets[0], p1.propagate(), True)
    p1.queue_sets()
    p1.accumulate([1.5], reset=True)
    I, Sz = p1.sums()
    _check_sums(I, Sz, [[(1.5, sets[0])]], True)
    assert ctx.method == 'gemm' and ctx.precision == 'f64' and ctx.plan_owner == t.owner
    after = t.radiation_vectors()
    assert all(np.array_equal(after[k], vectors[k]) for k in vectors)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(t.project(), proj))
    # a second propagator plans: the sums of the first are gone, not stale
    p2 = ma.PlanePropagator(x, y, WL, ref.N_GLASS, tx[:40] + 1e-6, ty[:40], 30e-6, want_h=False, ctx=ctx)
    buf = np.empty(300)
    assert ctx.lib.ml_propagate_sums(ctx.handle, _lib.dptr(buf), None) != 0
    with pytest.raises(_lib.MetalensHipError, match='has not run on the active propagation plan'):
        p1.sums()
    with pytest.raises(RuntimeError, match='another propagator has planned'):
        p1.accumulate([1.0], reset=True)
    assert p2.propagate()['Ex'].shape == (40, 40)
    # ... and the first one plans again when it is asked for fields
    _same(p1.propagate_sets()[0], sets[0], True)
    ctx.set_method('auto')


def test_a_multi_rank_context_refuses(ma, monkeypatch):
    from metalens_amd import _lib
    from test_gpu_fft import fields
    from test_gpu_fft_mixed import _upload
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        x = (np.arange(32) - 15.5) * PITCH
        p = ma.PlanePropagator(x, x, WL, ref.N_GLASS, [0.0], [0.0], 5e-6, ctx=c)   # planned while single-rank
        _upload(c, fields(32, 32, 5))
        assert p.propagate_sets()[0]['Ex'].shape == (1, 1)
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        with pytest.raises(_lib.MetalensHipError, match='ml_propagate_sets: this context belongs to a communicator of 2 ranks'):
            p.propagate_sets()
    finally:
        c.close()
