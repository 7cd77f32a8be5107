"""Per-zone contributions to the field at points behind the aperture on the GPU (csrc/fields_zone_fields.hip,
ml_fields_zone_fields, ``ApertureZoneFields``) against the long-double yardstick (tests/zone_fields_ref.py) within ``8 e_ref``,
their closure against ``PlanePropagator(method='direct', point_list=True)`` on the same context within ``16 e_ref``, and the
byte-level requirements: (a) two calls agree, (b) the records of a set do not depend on the other sets of the call, (c) the
record of a zone does not depend on the other edges, (d) the records of a target do not depend on the other targets - across
the groups of ``ZONE_FIELDS_TG`` targets a walk takes -, (e) the E records do not depend on ``want_h``.  Needs an MI355X.

Fields are seeded random complex arrays through ml_fields_upload.  The shapes are the small cases of
tests/test_gpu_fields_zones.py with ascending uniform axes: a vertex on a block's first lane (130 x 129) and inside the
second block with zones closer than the pitch (70 x 257), lines without a vertex (centre outside the grid), one block
exactly and one sample more, a single sample, more edges than samples, one edge, samples exactly on an edge.  Per case two
to five targets: one 2 um behind the aperture inside its footprint, one at a focus-like distance on the centre's axis, one
well outside the footprint laterally."""
import numpy as np
import pytest

import propagate_ref
import zone_fields_ref as ref

pytestmark = pytest.mark.gpu

WL, NG = 580e-9, 1.46
P = WL / 2.2
Z0 = propagate_ref.Z0_SI


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


def _upload(ctx, F):
    from metalens_amd import _lib
    arrs = [_lib.c128(a) for a in F]
    _lib.check(ctx.lib.ml_fields_upload(ctx.handle, arrs[0].shape[0], arrs[0].shape[1], *[_lib.dptr(a) for a in arrs]))
    ctx.fields_owner = None


def _axes(nx, ny, cx, cy):
    """axes on the pitch with the origin between samples (cx, cy: where 0 lies, in samples)"""
    return (np.arange(nx) - cx) * P, (np.arange(ny) - cy) * P


def _tight_edges():
    """40 edges, ten of them 0.4 nm apart - far closer than the pitch of 0.26 um: empty zones, zones a line skips"""
    return np.sort(np.concatenate([np.linspace(1e-6, 30e-6, 30), 9e-6 + np.arange(10) * 0.0004e-6]))


def _targets(x, y, centre, unit=1e-6):
    """2 um behind the aperture inside its footprint (off every sample), a focus-like distance on the centre's axis, and
    well outside the footprint laterally"""
    return np.array([[x[x.size // 3] + 0.3 * (x[-1] - x[0]) / max(x.size - 1, 1), y[y.size // 2], 2 * unit],
                     [centre[0], centre[1], 30 * unit],
                     [x[-1] + 45 * unit, y[0] - 20 * unit, 12 * unit]])


# name -> (x, y, wavelength, n_glass, edges, centre, pitch, points)
def _case(name):
    pitch = None
    if name == '130x129':      # the centre in the axes' middle: between samples along x, on sample 64 - a block's first lane - along y
        x, y = _axes(130, 129, 64.5, 64)
        edges, centre = np.linspace(2e-6, 17e-6, 12), (0.0, 0.0)
    elif name == '70x257':     # the centre off every sample, the vertex at lane 37 of the second block
        x, y = _axes(70, 257, 30.3, 100.7)
        edges, centre = _tight_edges(), (0.37e-6, -1.21e-6)
    elif name == '33x300':     # the centre outside the grid: every line monotone, the vertex the line's first sample
        x, y = _axes(33, 300, -20.0, -7.4)
        edges, centre = np.linspace(3e-6, 80e-6, 300), (0.0, 0.0)
    elif name in ('1x1', '3x64', '3x65'):
        nx, ny = (int(v) for v in name.split('x'))
        x, y = _axes(nx, ny, (nx - 1) / 2, ny / 3)
        edges, centre = np.linspace(0.0, 12e-6, 7), (0.0, 0.0)
        pitch = (P, P) if name == '1x1' else None      # (one sample has no step of its own)
    elif name == '64x70 K=4096':   # far more zones than samples
        x, y = _axes(64, 70, 30.5, 33.2)
        edges, centre = np.linspace(0.05e-6, 11e-6, 4096), (0.0, 0.0)
    elif name == '64x70 K=1':
        x, y = _axes(64, 70, 30.5, 33.2)
        edges, centre = np.array([6e-6]), (0.0, 0.0)
    elif name == 'integers':   # x = i, y = j: (3, 4) and (5, 12) lie exactly on the edges 5 and 13
        x, y = np.arange(16.0), np.arange(70.0)
        return x, y, 4.0, 1.0, np.array([5.0, 13.0]), (0.0, 0.0), None, _targets(x, y, (0.0, 0.0), unit=4.0)
    else:
        raise KeyError(name)
    pts = _targets(x, y, centre)
    if name == '64x70 K=4096':
        pts = pts[:2]            # (the yardstick takes a direct sum per zone that holds samples)
    if name == '130x129':
        pts = np.concatenate([pts, [[x[5], y[100] + 0.1 * P, 0.5e-6], [-3e-6, 2e-6, 1e-3]]])   # five: one group and one more
    return x, y, WL, NG, edges, centre, pitch, pts


CASES = ['130x129', '70x257', '33x300', '1x1', '3x64', '3x65', '64x70 K=4096', '64x70 K=1', 'integers']


def _azf(ma, ctx, case, **kw):
    x, y, wl, ng, edges, centre, pitch, pts = case
    kw.setdefault('points', pts)
    return ma.ApertureZoneFields(x, y, wl, ng, edges, centre=centre, pitch=pitch, Z0=Z0, ctx=ctx, **kw)


def _direct(ma, ctx, case, pts):
    """the whole field at the points by the direct propagator on the same context -> E, H of shape (3, T)"""
    x, y, wl, ng = case[:4]
    p = ma.PlanePropagator(x, y, wl, ng, pts[:, 0], pts[:, 1], pts[:, 2], point_list=True, Z0=Z0, ctx=ctx, method='direct')
    d = p.propagate()
    return np.stack([d['Ex'], d['Ey'], d['Ez']]), np.stack([d['Hx'], d['Hy'], d['Hz']])


@pytest.mark.parametrize('name', CASES, ids=lambda n: n.replace(' ', '_'))
def test_zone_fields_against_the_yardstick(ma, ctx, name):
    from metalens_amd import postprocess
    case = _case(name)
    x, y, wl, ng, edges, centre, pitch, pts = case
    assert 2 <= len(pts) <= 5
    if name == '130x129':
        assert len(pts) == postprocess.ZONE_FIELDS_TG + 1          # T = TG + 1 (the constant: test_zone_fields_host.py)
    F = ref.seeded_fields(1, x.size, y.size, seed=17 + x.size * 1000 + y.size)
    want = ref.yardstick(F, x, y, wl, ng, edges, centre, pts, pitch)
    _upload(ctx, F[0])
    azf = _azf(ma, ctx, case)
    rec, samples = azf.records(with_samples=True)
    assert rec.shape == (1, len(edges) + 1, len(pts), 12) and np.array_equal(samples, want['n'])
    again = azf.records()
    assert again.tobytes() == rec.tobytes()                                                   # (a)
    got = azf.analyse()
    ref.hold('gpu ' + name, got, want)
    empty = want['n'] == 0
    assert (rec[0][empty] == 0).all() and not np.signbit(rec[0][empty]).any()
    if name == '64x70 K=4096':
        assert empty.sum() > 4096 // 2 and (~empty).sum() > 100          # most zones are empty
    if name == '70x257':
        assert empty[:-1].any() and want['n'][-1] > 0
    if name == '64x70 K=1':
        assert got['samples'].shape == (1,) and got['samples'][0] + got['outside'] == 64 * 70
    if name == 'integers':
        zone = ref.membership(x, y, edges, centre)
        assert zone[3, 4] == 0 and zone[4, 3] == 0 and zone[5, 12] == 1 and zone[12, 5] == 1 and zone[4, 4] == 1 and zone[5, 13] == 2
        assert got['samples'].tolist() == [int((zone == 0).sum()), int((zone == 1).sum())]
    # closure: the slots added up against the direct propagator on the same context
    if x.size > 1 and y.size > 1:          # (PlanePropagator takes its pitch from the axes)
        E, H = _direct(ma, ctx, case, pts)
        for f, whole in (('E', E), ('H', H)):
            err = float(np.abs(got['total_' + f][0] - whole).max() / np.abs(want[f]).max())
            print('PARITY zone fields closure %-18s %s  error %.3e  allowed %.3e' % (name, f, err, 2 * ref.MARGIN * want['e_ref_' + f]))
            assert err <= 2 * ref.MARGIN * want['e_ref_' + f], (name, f, err)
    # the one-shot call on host arrays: the same numbers
    one = ma.aperture_zone_fields(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, y, wl, ng, edges, pts, centre=centre, pitch=pitch, Z0=Z0, ctx=ctx)
    assert all(np.array_equal(one[k], got[k], equal_nan=True) for k in got)


@pytest.fixture(scope='module')
def many():
    """the 70 x 257 case with three field sets and 64 targets: inside, above and around the footprint, from 0.5 um to 1 mm"""
    x, y, wl, ng, edges, centre, pitch, _ = _case('70x257')
    rng = np.random.default_rng(64)
    pts = np.stack([rng.uniform(x[0] - 20e-6, x[-1] + 20e-6, 64), rng.uniform(y[0] - 20e-6, y[-1] + 20e-6, 64),
                    10.0 ** rng.uniform(np.log10(0.5e-6), -3, 64)], axis=1)
    return (x, y, wl, ng, edges, centre, pitch, pts), ref.seeded_fields(3, x.size, y.size, seed=5)


def test_64_targets_and_their_groups(ma, ctx, many):
    """T = 64 against the yardstick, and (d): every target alone, groups that straddle the walks of TG targets and a
    permutation have the bytes of the call of 64"""
    from metalens_amd import postprocess
    case, F = many
    x, y, wl, ng, edges, centre, pitch, pts = case
    tg = postprocess.ZONE_FIELDS_TG
    _upload(ctx, F[0])
    azf = _azf(ma, ctx, case)
    rec = azf.records()
    assert rec.shape == (1, len(edges) + 1, 64, 12) and azf.records().tobytes() == rec.tobytes()          # (a)
    # the yardstick at five of the 64 (a direct sum per zone and target): the first, the last, and around a group's edge
    some = [0, tg - 1, tg, 37, 63]
    want = ref.yardstick(F[:1], x, y, wl, ng, edges, centre, pts[some], pitch)
    got = postprocess._zone_fields_dict(rec[:, :, some], azf.records(with_samples=True)[1], True)
    ref.hold('gpu 64 targets', got, want)
    for t in range(64):                                                                          # (d) each alone
        alone = _azf(ma, ctx, case, points=pts[t:t + 1]).records()
        assert alone[0, :, 0].tobytes() == rec[0, :, t].tobytes(), t
    for lo, hi in ((tg - 1, tg + 1), (1, 2 * tg + 2), (tg, 3 * tg), (61, 64), (2, 63)):        # groups that straddle TG
        part = _azf(ma, ctx, case, points=pts[lo:hi]).records()
        assert np.array_equal(part[0], rec[0, :, lo:hi]), (lo, hi)
    order = np.random.default_rng(1).permutation(64)
    assert np.array_equal(_azf(ma, ctx, case, points=pts[order]).records()[0], rec[0][:, order])


def test_e_does_not_depend_on_h(ma, ctx, many):
    """(e): the E records with want_h = 0 have the bits of those with want_h = 1"""
    case, F = many
    _upload(ctx, F[1])
    pts = case[-1][:9]
    both = _azf(ma, ctx, case, points=pts).records()
    e_only, samples = _azf(ma, ctx, case, points=pts, want_h=False).records(with_samples=True)
    assert e_only.shape == both.shape[:3] + (6,) and e_only.tobytes() == np.ascontiguousarray(both[..., :6]).tobytes()
    assert np.abs(both[..., 6:]).max() > 0 and samples.sum() == 70 * 257
    d = _azf(ma, ctx, case, points=pts, want_h=False).analyse()
    assert 'H' not in d and 'total_H' not in d and d['E'].shape == (1, 40, 3, 9)


def test_a_zone_does_not_depend_on_the_other_edges(ma, ctx, many):
    """(c): the records of zone (e_a, e_b] in the list of 40 edges have the bytes of that zone with edges = [e_a, e_b] alone -
    for the first, a middle and the last zone that holds samples, and for the disc; one more edge cuts a zone in two and
    leaves every other zone's bytes"""
    case, F = many
    x, y, wl, ng, edges, centre, pitch, pts = case
    pts = pts[:6]
    _upload(ctx, F[2])
    rec, n = _azf(ma, ctx, case, points=pts).records(with_samples=True)
    held = np.flatnonzero(n[1:-1] > 0) + 1
    assert held.size >= 3 and (n[:-1] == 0).any()

    def with_edges(e):
        return _azf(ma, ctx, (x, y, wl, ng, e, centre, pitch, pts)).records(with_samples=True)
    for z in (held[0], held[held.size // 2], held[-1]):
        alone, m = with_edges(edges[z - 1:z + 1])
        assert alone.shape == (1, 3, 6, 12) and m[1] == n[z] > 0
        assert alone[0, 1].tobytes() == rec[0, z].tobytes(), z
        assert m.sum() == 70 * 257 and m[2] == n[z + 1:].sum()
    disc, m = with_edges(edges[:1])
    assert disc[0, 0].tobytes() == rec[0, 0].tobytes() and m[0] == n[0] > 0
    last, m = with_edges(edges[-1:])
    assert last[0, 1].tobytes() == rec[0, -1].tobytes() and m[1] == n[-1] > 0                  # the outside is a slot like any other
    z = held[np.argmax(n[held])]                      # (the zone with the most samples: both halves hold some)
    parts, m = with_edges(np.insert(edges, z, 0.5 * (edges[z - 1] + edges[z])))
    assert m[z] + m[z + 1] == n[z] and m[z] > 0 and m[z + 1] > 0
    assert np.array_equal(np.delete(parts[0], [z, z + 1], axis=0), np.delete(rec[0], z, axis=0))


def _download(ctx, m, shape):
    from metalens_amd import _lib
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
    F = [np.empty(shape, dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    return np.stack(F)


def test_three_set_batch(ma, ctx):
    """(b): the x, y, z dipoles of test_gpu_propagate_sets.py's lens on its window A, zones from the layout: one call over the
    three resident sets, every set alone (``first_set`` = 0, 1, 2) and the pairs have its bytes; the batch against the
    yardstick on the fields downloaded afterwards"""
    from metalens_amd import _lib
    from test_gpu_propagate_sets import DIPOLES, _batch, _lens
    x, y, n_glass, n = _batch(ma, ctx, 'A', DIPOLES)
    assert n == 3
    edges = ma.zone_edges(_lens()['lens_periphery_summary'])
    edges = edges[:: max(1, edges.size // 12)]                 # a dozen zones: the yardstick takes a direct sum per zone
    pts = np.array([[x[x.size // 2] + 0.2 * P, y[y.size // 3], 2e-6], [0.0, 0.0, 40e-6], [x[-1] + 30e-6, y[0], 15e-6]])
    azf = ma.ApertureZoneFields(x, y, WL, n_glass, edges, pts, Z0=Z0, ctx=ctx)
    rec = azf.records()
    assert rec.shape == (3, edges.size + 1, 3, 12) and azf.records(0, 3).tobytes() == rec.tobytes()        # (a)
    for m in range(3):
        assert azf.records(m, 1)[0].tobytes() == rec[m].tobytes(), m                                         # (b)
    assert azf.records(1, 2).tobytes() == rec[1:].tobytes() and azf.records(0, 2).tobytes() == rec[:2].tobytes()
    F = np.stack([_download(ctx, m, (x.size, y.size)) for m in range(3)])
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))
    assert all(np.abs(F[m]).max() > 0 for m in range(3)) and not np.array_equal(rec[0], rec[1])
    want = ref.yardstick(F, x, y, WL, n_glass, edges, (0.0, 0.0), pts)
    ref.hold('gpu three-set batch', azf.analyse(), want)


def test_state_is_left_alone(ma, ctx):
    """the fields, the active propagation plan with its result, the zone sums and the pupil's plan do not notice a call"""
    from metalens_amd import _lib
    case = _case('130x129')
    x, y, wl, ng, edges, centre, pitch, pts = case
    F = ref.seeded_fields(1, x.size, y.size, seed=77)
    _upload(ctx, F[0])
    tx, ty = np.linspace(-5e-6, 5e-6, 7), np.linspace(-4e-6, 4e-6, 5)
    p = ma.PlanePropagator(x, y, wl, ng, tx, ty, 25e-6, Z0=Z0, ctx=ctx)
    before = p.propagate()
    p.queue_sets()
    p.accumulate([1.5], reset=True)
    sums = p.sums()
    az = ma.ApertureZones(x, y, wl, ng, edges, centre=centre, ctx=ctx)
    zones = az.records()
    pupil = ma.AperturePupil(x, y, 15e-6, edges=edges, zone_factors=np.exp(1j * np.arange(edges.size)), ctx=ctx)
    pupil.plan()
    owners = (ctx.propagate_owner, ctx.pupil_owner, ctx.fields_owner)
    fields = _download(ctx, 0, (x.size, y.size))
    azf = _azf(ma, ctx, case)
    rec = azf.records()
    assert np.abs(rec).max() > 0
    assert (ctx.propagate_owner, ctx.pupil_owner, ctx.fields_owner) == owners
    assert _download(ctx, 0, (x.size, y.size)).tobytes() == fields.tobytes() == np.stack([_lib.c128(a) for a in F[0]]).tobytes()
    # the plan's result and sums are those of before the call, downloaded without another pass
    after = p._download(0)
    assert all(np.array_equal(after[k], before[k]) for k in before)
    for g, w in zip(p.sums(), sums):
        assert np.array_equal(g, w)
    assert az.records().tobytes() == zones.tobytes()
    pupil.apply()                                     # the plan made before the call is the one applied: no planning again
    want = ma.apply_pupil_host(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, y, 15e-6, edges=edges, zone_factors=np.exp(1j * np.arange(edges.size)))
    assert np.allclose(_download(ctx, 0, (x.size, y.size)), np.stack(want), rtol=1e-14, atol=0)
    assert azf.records().tobytes() != rec.tobytes()   # (the pupil changed the fields; the analysis sees it)


def test_refusals(ma, ctx, monkeypatch):
    """messages only: nothing is launched"""
    from metalens_amd import _lib
    x, y = _axes(20, 24, 9.5, 11.5)
    F = ref.seeded_fields(1, 20, 24, seed=1)
    _upload(ctx, F[0])
    edges, pts = [2e-6, 4e-6], np.array([[0.0, 0.0, 1e-5], [1e-6, 0.0, 2e-6]])
    kw = dict(Z0=Z0, ctx=ctx)
    before = ma.ApertureZoneFields(x, y, WL, NG, edges, pts, **kw).records()
    with pytest.raises(_lib.MetalensHipError, match='ml_fields_zone_fields: the axes have 20 x 23 samples, the resident field sets 20 x 24'):
        ma.ApertureZoneFields(x, y[:-1], WL, NG, edges, pts, **kw).analyse()
    with pytest.raises(_lib.MetalensHipError, match=r'ml_fields_zone_fields: a target can lie 100 m from a sample of the 20 x 24 aperture, '
                                                    r'k R = 1\.58\d*e\+09: the phase arithmetic covers k R up to 1e\+09'):
        ma.ApertureZoneFields(x, y, WL, NG, edges, [[0.0, 0.0, 100.0]], **kw).analyse()
    with pytest.raises(_lib.MetalensHipError, match='field sets 1 ... 1 asked for, 1 resident'):
        ma.ApertureZoneFields(x, y, WL, NG, edges, pts, **kw).analyse(first=1, n=1)
    # tz <= 0 and 65 targets: the Python layer refuses them first, the entry in its own words
    a = ma.ApertureZoneFields(x, y, WL, NG, edges, pts, **kw)
    rec, n = np.zeros((1, 3, 65, 12)), np.zeros(3, dtype=np.int64)

    def call(tx, ty, tz):
        return ctx.lib.ml_fields_zone_fields(ctx.handle, 0, 1, *a._geometry, a.Z0, _lib.dptr(a._x2), 20, _lib.dptr(a._y2), 24, _lib.dptr(a._e2), 2,
                                             _lib.dptr(_lib.f64(tx)), _lib.dptr(_lib.f64(ty)), _lib.dptr(_lib.f64(tz)), len(tx), 1,
                                             _lib.dptr(rec), n.ctypes.data_as(_lib.POINTER(_lib.c_int64)))
    assert call(np.zeros(2), np.zeros(2), np.array([1e-5, 0.0])) != 0
    assert b'ml_fields_zone_fields: tz[1] = 0: a target lies behind the aperture, z > 0' in ctx.lib.ml_last_error()
    assert call(np.zeros(2), np.zeros(2), np.array([-1e-5, 1.0])) != 0 and b'tz[0] = -1e-05' in ctx.lib.ml_last_error()
    assert call(np.zeros(65), np.zeros(65), np.ones(65)) != 0
    assert b'ml_fields_zone_fields: 65 targets: 1 to 64 are taken' in ctx.lib.ml_last_error()
    assert (rec == 0).all() and (n == 0).all()
    assert np.array_equal(ma.ApertureZoneFields(x, y, WL, NG, edges, pts, **kw).records(), before)      # a refused call changes nothing
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        kw = dict(Z0=Z0, ctx=c)
        with pytest.raises(_lib.MetalensHipError, match='no resident field set'):
            ma.ApertureZoneFields(x, y, WL, NG, edges, pts, **kw).analyse(n=1)
        _upload(c, F[0])
        assert np.array_equal(ma.ApertureZoneFields(x, y, WL, NG, edges, pts, **kw).records(), before)
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        with pytest.raises(_lib.MetalensHipError, match='ml_fields_zone_fields: this context belongs to a communicator of 2 ranks'):
            ma.ApertureZoneFields(x, y, WL, NG, edges, pts, **kw).analyse(n=1)
    finally:
        c.close()
