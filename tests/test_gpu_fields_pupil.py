"""The pupil function applied to the resident near field on the GPU (csrc/fields_pupil.hip, ml_fields_pupil_plan /
ml_fields_pupil_apply, ``AperturePupil``) against the long-double yardstick (tests/fields_pupil_ref.py) within its derived
bound, exact zeros and untouched bytes where the definition has them, and the byte-level requirements: two applications
agree, a set does not depend on the other sets of the launch, nothing stale is read by the transform or the propagator
afterwards, a premodulated synthesis is unmodulated first, the loop measure - correct - measure converges on the GPU, and a
``SourceSweep`` with ``pupil=`` gives the bytes of the sequence run by hand.  Needs an MI355X.

Fields are seeded random complex arrays through ml_fields_upload unless said otherwise.  The shapes are those of
test_gpu_fields_wavefront.py, because the line walk is the same: a vertex on a block's first lane (130 x 129) and inside a
block (70 x 257), lines without a vertex (33 x 300, y ascending and descending), one block exactly and one sample more, a
single sample, lines of three samples, lines outside the pupil at both ends (300 x 70), a pupil that holds the whole grid,
one sample or none, samples exactly on the rim and on the edges; crossed with stop on and off, the orders 0, 4, 5 and 8 (both
instantiations of the phase at both ends), and 0, 1, 7 and 4096 edges (more edges than samples) with factors 0 and 1 among
them."""
import numpy as np
import pytest

import fields_pupil_ref as ref
from test_fields_pupil_host import LOOP_CASES, _zones, loop_field
from test_gpu_fields_wavefront import NG, WL, _case, _download, _upload

pytestmark = pytest.mark.gpu


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


def _kw(radius, stop, order, K, seed):
    kw = dict(stop=stop)
    if order is not None:
        kw['phase'] = ref.seeded_phase(order, seed)
    if K:
        kw['edges'], kw['zone_factors'] = _zones(radius, K, seed + 1)
    return kw


# name of test_gpu_fields_wavefront._case, stop, order (None: no phase), edges
CASES = [('130x129', True, None, 0), ('130x129', True, 4, 0), ('130x129', False, 8, 7), ('130x129', True, 5, 198), ('130x129', False, None, 0),
         ('70x257', True, 8, 4096), ('70x257', False, 4, 0), ('70x257', False, None, 4096), ('70x257', True, 0, 1),
         ('33x300', True, 5, 7), ('33x300', False, 0, 1), ('33x300 descending', True, 4, 1), ('33x300 descending', False, 8, 4096),
         ('1x1', True, 8, 7), ('1x1', False, None, 1), ('3x64', True, 4, 0), ('3x64', False, 5, 7), ('3x65', True, 5, 1), ('3x65', False, None, 7),
         ('64x3', True, 8, 4096), ('64x3', False, 0, 0), ('300x70', True, 8, 7), ('300x70', False, 5, 0), ('300x70', True, None, 1),
         ('whole grid', True, 8, 0), ('whole grid', False, 4, 7), ('one sample', True, 5, 7), ('one sample', False, 4, 0),
         ('no sample', True, 4, 7), ('no sample', False, 8, 4096), ('no sample', False, 5, 0)]


@pytest.mark.parametrize('name,stop,order,K', CASES, ids=lambda v: str(v).replace(' ', '_'))
def test_pupil_against_the_yardstick(ma, ctx, name, stop, order, K):
    """(1) against the yardstick; (2) a second application onto the same field, uploaded again, gives the same bytes; and the
    one-shot call on host arrays returns them"""
    x, y, _wl, _ng, radius, centre, _reference = _case(name)
    kw = _kw(radius, stop, order, K, seed=x.size + 3 * y.size)
    F = ref.seeded_fields(1, x.size, y.size, seed=31 + x.size * 1000 + y.size)
    _upload(ctx, F[0])
    ap = ma.AperturePupil(x, y, radius, centre=centre, ctx=ctx, **kw)
    ap.apply()
    got = _download(ctx, 0, (x.size, y.size))[None]
    want = ref.parts(x, y, radius, centre, **kw)
    ref.hold('gpu %s stop %d order %s edges %d' % (name, stop, order, K), got, F, want)
    _upload(ctx, F[0])
    ap.apply(0, 1)
    assert _download(ctx, 0, (x.size, y.size)).tobytes() == got[0].tobytes()                                   # (2)
    one = ma.apply_pupil(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, y, radius, centre=centre, ctx=ctx, **kw)
    assert np.stack(one).tobytes() == got[0].tobytes()
    n, total = int(want['member'].sum()), x.size * y.size
    if name == 'no sample':
        assert n == 0 and (want['zero'].all() if stop else not want['zero'].any())
        if stop:
            assert (got == 0).all()
        elif not K:
            assert got.tobytes() == F.tobytes()
    if name == 'one sample':
        assert n == 1
    if name == 'whole grid':
        assert n == total and not want['zero'].any()
    if name in ('300x70', '70x257', '130x129'):
        assert 0 < n < total
    if name == '300x70':
        held = want['member'].any(axis=1)
        assert not held[0] and not held[-1] and 256 < held.sum() < 300          # lines wholly outside at both ends
    if K and not stop and name != 'no sample':
        assert want['touch'].any()


def test_rim_and_edges_on_integers(ma, ctx):
    """x = i, y = j: (3, 4), (4, 3), (5, 0) and (0, 5) lie exactly on the rim R = 5 and are inside; with E2 = 9, 25 the samples
    (0, 3) and (3, 0) lie on the first edge and belong to zone 0, the rim to zone 1; factors 2 and i are exact in fp64"""
    x, y, _wl, _ng, radius, centre, _reference = _case('integers')
    F = ref.seeded_fields(1, x.size, y.size, seed=5)
    for stop in (True, False):
        _upload(ctx, F[0])
        ma.AperturePupil(x, y, radius, centre=centre, stop=stop, edges=[3.0, 5.0], zone_factors=[2.0, 1j], ctx=ctx).apply()
        got = _download(ctx, 0, (x.size, y.size))
        inside = (x[:, None] ** 2 + y[None, :] ** 2) <= 25
        assert inside.sum() == 26 and inside[3, 4] and inside[5, 0] and not inside[4, 4]
        zone0 = (x[:, None] ** 2 + y[None, :] ** 2) <= 9
        assert zone0[0, 3] and zone0[3, 0] and not zone0[1, 3]
        assert np.array_equal(got[:, zone0], 2 * F[0][:, zone0])
        ring = inside & ~zone0
        assert np.array_equal(got[:, ring].real, -F[0][:, ring].imag) and np.array_equal(got[:, ring].imag, F[0][:, ring].real)
        if stop:
            assert (got[:, ~inside] == 0).all() and not np.signbit(got[:, ~inside].real).any()
        else:
            assert got[:, ~inside].tobytes() == F[0][:, ~inside].tobytes()
        want = ref.parts(x, y, radius, centre, stop=stop, edges=[3.0, 5.0], zone_factors=[2.0, 1j])
        ref.hold('gpu integers stop %d' % stop, got[None], F, want)
    # a phase on the rim: the rim's samples are members and take it
    c = ref.seeded_phase(8, 77)
    _upload(ctx, F[0])
    ma.AperturePupil(x, y, radius, centre=centre, stop=True, phase=c, ctx=ctx).apply()
    ref.hold('gpu integers order 8', _download(ctx, 0, (x.size, y.size))[None], F, ref.parts(x, y, radius, centre, stop=True, phase=c))


def test_identity_pupil_leaves_every_value(ma, ctx):
    """(4) stop=False, no phase, no edges: every value equal under ==, here even every byte: nothing is read or written"""
    x, y, _wl, _ng, radius, centre, _reference = _case('70x257')
    F = ref.seeded_fields(1, x.size, y.size, seed=9)
    _upload(ctx, F[0])
    ma.AperturePupil(x, y, radius, centre=centre, stop=False, ctx=ctx).apply()
    got = _download(ctx, 0, (x.size, y.size))
    assert (got == F[0]).all() and got.tobytes() == F[0].tobytes()
    # factors of exactly 1 given as zone factors, and a zero phase, are multiplied in: equal under ==
    ma.AperturePupil(x, y, radius, centre=centre, stop=False, phase=np.zeros(15), edges=[radius, 2 * radius], zone_factors=[1.0, 1.0], ctx=ctx).apply()
    assert (_download(ctx, 0, (x.size, y.size)) == F[0]).all()


def test_sets_of_a_launch(ma, ctx):
    """(3) the x, y, z dipoles of test_gpu_propagate_sets.py's lens on its window A: ``apply(1, 2)`` changes sets 1 and 2 only, and
    every set of a launch of 1, 2 or 3 sets has the bytes of the same field applied alone"""
    from metalens_amd import _lib
    from test_gpu_propagate_sets import DIPOLES, _batch
    x, y, n_glass, n = _batch(ma, ctx, 'A', DIPOLES)
    assert n == 3
    shape = (x.size, y.size)
    F = np.stack([_download(ctx, m, shape) for m in range(3)])
    centre, radius = (50.5e-6, 1.0e-6), 11e-6
    kw = _kw(radius, True, 8, 7, seed=12)
    ap = ma.AperturePupil(x, y, radius, centre=centre, ctx=ctx, **kw)
    alone = []
    for m in range(3):
        _upload(ctx, F[m])
        ap.apply()
        alone.append(_download(ctx, 0, shape))
        ref.hold('gpu batch set %d alone' % m, alone[m][None], F[m][None], ref.parts(x, y, radius, centre, **kw))
        assert np.abs(alone[m]).max() > 0 and alone[m].tobytes() != F[m].tobytes()
    for first, count in ((1, 2), (0, 3), (2, 1), (0, 2)):
        _batch(ma, ctx, 'A', DIPOLES)
        ap.apply(first, count)
        for m in range(3):
            got = _download(ctx, m, shape)
            assert got.tobytes() == (alone[m] if first <= m < first + count else F[m]).tobytes(), (first, count, m)
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))


def test_nothing_stale_is_read_afterwards(ma, ctx):
    """(5) right after a synthesis and ``apply``: download the modified set, transform it and propagate it ('direct'); then upload
    the downloaded arrays and do the same: ``P``, ``E`` and ``H`` have the same bytes - what the synthesis knew of its own fields
    (row extents, zeros) is not used for fields it no longer wrote"""
    from test_gpu_propagate_sets import DIPOLES, _batch, _targets
    x, y, n_glass, n = _batch(ma, ctx, 'A', DIPOLES)
    shape = (x.size, y.size)
    centre, radius = (50.5e-6, 1.0e-6), 9e-6
    t, tkw = _targets('points', x, y)
    for kw in (_kw(radius, True, 4, 0, seed=3), _kw(radius, False, 5, 7, seed=4)):
        _batch(ma, ctx, 'A', DIPOLES)
        ma.AperturePupil(x, y, radius, centre=centre, ctx=ctx, **kw).apply()
        results = []
        for again in (False, True):
            if again:
                _upload(ctx, G)
            G = _download(ctx, 0, shape)
            P = ma.farfield_from_resident_nearfield(x, y, WL, n_glass, ctx=ctx)[0]
            img = ma.PlanePropagator(x, y, WL, n_glass, *t, ctx=ctx, method='direct', **tkw).propagate()
            results.append((G, P, img))
        (G0, P0, I0), (G1, P1, I1) = results
        assert G0.tobytes() == G1.tobytes() and np.nanmax(P0) > 0 and P0.tobytes() == P1.tobytes()
        assert set(I0) == set(I1) and all(np.abs(I0[key]).max() > 0 and I0[key].tobytes() == I1[key].tobytes() for key in I0)


def test_premodulated_synthesis_is_unmodulated_first(ma, ctx):
    """(6) a synthesis under ml_nearfield_premodulate, set up as in test_gpu_fields_wavefront.py, leaves the resident fields
    modulated: ``apply`` BEFORE any download works on the plain near field - the result of download, upload, apply, to the bit"""
    from metalens_amd import _lib
    from metalens_amd.pipeline import HotPath
    from test_gpu_parity import _synthetic_lens
    lens = _synthetic_lens(40e-6, 0.4, WL, switch_deg=9.0)
    S = lens['lens_periphery_summary']
    R = S['r_max_list'][-1]
    x = np.linspace(-R, R, 384)
    u = (np.arange(96) - 48) * 0.004            # bins -48 .. 47: symmetric about -0.002, so the modulation exists
    kw = _kw(0.8 * R, True, 5, 7, seed=8)

    def synthesise():
        hp = HotPath((0.3e-6, -0.2e-6, -lens['source_distance'], 'y'), WL, S, lens['lens_center_summary'], lens['hexgridset'], x, x, u, u,
                     ctx=ctx, fuse_modulation=True)
        hp.step()
        hp.sync()
    synthesise()
    ap = ma.AperturePupil(x, x, 0.8 * R, ctx=ctx, **kw)
    ap.apply()                                  # before any download
    got = _download(ctx, 0, (x.size, x.size))
    synthesise()
    F = _download(ctx, 0, (x.size, x.size))
    _lib.check(ctx.lib.ml_nearfield_premodulate(ctx.handle, 0))
    _upload(ctx, F)
    ap.apply()
    assert _download(ctx, 0, (x.size, x.size)).tobytes() == got.tobytes() and got.tobytes() != F.tobytes()
    ref.hold('gpu premodulated synthesis', got[None], F[None], ref.parts(x, x, 0.8 * R, (0.0, 0.0), **kw))


@pytest.mark.parametrize('name', sorted(LOOP_CASES))
def test_measure_correct_measure_converges_on_the_gpu(ma, ctx, name):
    """(7) the field of the host loop (test_fields_pupil_host.py) through ``ApertureWavefront`` -> ``from_wavefront`` -> ``apply``, the
    field staying on the GPU: every round brings the rms under 0.2 of the round before and the coherence does not fall"""
    (x, y), R, centre = LOOP_CASES[name]
    _upload(ctx, loop_field(x, y, R, centre))
    aw = ma.ApertureWavefront(x, y, WL, NG, R, n_max=4, centre=centre, ctx=ctx)
    rms, coh = [], []
    for _ in range(4):
        res = aw.analyse()
        rms.append(float(res['rms'][0, 0]))
        coh.append(float(res['coherence'][0, 0]))
        ap = ma.AperturePupil.from_wavefront(aw, res, stop=False)
        assert ap.ctx is ctx and ap.shape == (x.size, y.size) and ap.n_max == 4 and ap._c[0] == 0
        ap.apply()
    print('gpu loop %s: rms %s coherence %s' % (name, ' -> '.join('%.4g' % v for v in rms), ' -> '.join('%.5f' % v for v in coh)))
    assert all(b < 0.2 * a for a, b in zip(rms, rms[1:])), rms
    assert all(b >= a for a, b in zip(coh, coh[1:])), coh


def test_from_zones_flattens_random_pistons(ma, ctx):
    """(7) a unit-amplitude field with a seeded piston in (-1, 1) rad per zone: ``ApertureZones`` -> ``from_zones`` -> ``apply`` leaves
    every populated zone at |phase| <= 1e-12 and coherence >= 1 - 1e-12"""
    (x, y), R, centre = LOOP_CASES['130x129']
    edges = np.linspace(0.1, 1.0, 10) * R
    piston = np.random.default_rng(21).uniform(-1, 1, edges.size)
    r2 = ((x - centre[0]) ** 2)[:, None] + ((y - centre[1]) ** 2)[None, :]
    zone = np.searchsorted(edges * edges, r2, side='left')
    E = np.exp(1j * np.append(piston, 0.0)[zone])
    _upload(ctx, np.stack([E, E, E, E]))
    az = ma.ApertureZones(x, y, WL, NG, edges, centre=centre, ctx=ctx)
    before = az.analyse()
    full = before['samples'] > 0
    assert full.all() and np.abs(before['phase'][0, :, 0] - piston).max() < 1e-12
    ap = ma.AperturePupil.from_zones(az, before, stop=False)
    assert ap.n_zones == edges.size and ap.radius == edges[-1]
    ap.apply()
    after = az.analyse()
    assert (np.abs(after['phase'][0][full]) <= 1e-12).all() and (after['coherence'][0][full] >= 1 - 1e-12).all()
    # a zone without a reading keeps its field: the factor of a NaN phase is 1
    nan = dict(before, phase=np.full_like(before['phase'], np.nan))
    assert (ma.AperturePupil.from_zones(az, nan, stop=False)._g == [1.0, 0.0]).all()


# ---- the sweep ------------------------------------------------------------------------------
def _sweep(ma, ctx):
    from test_gpu_propagate_sets import _common, _lens, _targets, _window
    lens = _lens()
    x, y = _window('A')
    u = np.linspace(-0.2, 0.2, 24)
    sw = ma.SourceSweep(*_common(lens), x, y, u, u, ctx=ctx)
    t, tkw = _targets('points', x, y)
    p = ma.PlanePropagator(x, y, WL, sw.n_glass, *t, ctx=ctx, **tkw)
    ap = ma.AperturePupil(x, y, 10e-6, centre=(50.5e-6, 1.0e-6), ctx=ctx, **_kw(10e-6, True, 5, 7, seed=2))
    return sw, p, ap, lens


def _params(sw, group):
    from metalens_amd import _lib
    from metalens_amd.nearfield import nearfield_params
    n = len(group['members'])
    params = (_lib.NearfieldParams * n)()
    for m, (k, pol) in enumerate(group['members']):
        sx, sy, sz = group['positions'][m]
        params[m] = nearfield_params(sx, sy, sz, pol, sw.wavelength, sw.n_glass, sw.dipole_moment, sw.c0, sw.Z0)
    return params, n


def test_sweep_with_a_pupil_equals_the_sequence_by_hand(ma, ctx):
    """(8) three sources at distinct positions (one position batch) with ``pupil=ap`` and ``keep_each=True``: every map has the bytes of
    ml_nearfield_batch_async, ml_fields_pupil_apply, select, transform, project run by hand; the sweep run twice gives the same
    bytes; a sweep without ``pupil`` afterwards gives the bytes of the sweep before any pupil was applied; ``power_in`` stays the
    incident power"""
    from metalens_amd import _lib
    sw, _p, ap, lens = _sweep(ma, ctx)
    f = lens['source_distance']
    sources = [(0.3e-6, -0.2e-6, -f, 'x'), (-1.0e-6, 0.5e-6, -1.05 * f, 'x'), (0.6e-6, 0.9e-6, -0.97 * f, 'y')]
    fresh = sw.run(sources, keep_each=True, cone=0.1)
    got = sw.run(sources, keep_each=True, cone=0.1, pupil=ap)
    again = sw.run(sources, keep_each=True, cone=0.1, pupil=ap)
    plain = sw.run(sources, keep_each=True, cone=0.1)
    for key in ('P_sum', 'total_P', 'power_in', 'cone_P'):
        assert np.array_equal(got[key], again[key], equal_nan=True), key
        assert np.array_equal(plain[key], fresh[key], equal_nan=True), key
    assert np.array_equal(got['power_in'], fresh['power_in']) and (got['total_P'] < fresh['total_P']).all() and (got['total_P'] > 0).all()
    for k in range(3):
        assert got['P_each'][k].tobytes() == again['P_each'][k].tobytes() and plain['P_each'][k].tobytes() == fresh['P_each'][k].tobytes()
    # by hand
    groups = sw._group(sources)
    assert len(groups) == 1 and groups[0].get('mixed')
    lib = ctx.lib
    sw.prepare()
    params, n = _params(sw, groups[0])
    _lib.check(lib.ml_nearfield_batch_async(ctx.handle, params, n, _lib.dptr(sw.x), sw.x.size, _lib.dptr(sw.y), sw.y.size))
    ap.plan()
    _lib.check(lib.ml_fields_pupil_apply(ctx.handle, 0, n))
    for m in range(n):
        _lib.check(lib.ml_fields_select(ctx.handle, m))
        _lib.check(lib.ml_farfield_transform_async(ctx.handle, 0, 0))
        P = np.empty((sw.ux.size, sw.uy.size))
        _lib.check(lib.ml_farfield_project(ctx.handle, sw.Z0, _lib.dptr(P), None, None))
        assert np.nanmax(P) > 0 and P.tobytes() == got['P_each'][m].tobytes() and P.tobytes() != fresh['P_each'][m].tobytes(), m
    _lib.check(lib.ml_fields_select(ctx.handle, 0))
    # queue(): the same sums without a synchronisation in between
    sw.queue(sources, pupil=ap)
    P_sum, total = np.empty((sw.ux.size, sw.uy.size)), np.zeros(3)
    _lib.check(lib.ml_farfield_sums(ctx.handle, _lib.dptr(P_sum), _lib.dptr(total), _lib.dptr(np.zeros(3)), 3))
    assert np.array_equal(P_sum, got['P_sum'], equal_nan=True) and np.array_equal(total, got['total_P'])


def test_sweep_image_with_a_pupil(ma, ctx):
    """(8) ``image=`` with ``pupil=`` on the five sources of test_gpu_propagate_sets.py - a polarisation batch, whose sets are
    written once more before the image, then a position batch: ``I_sum`` and ``Sz_sum`` equal the propagator run by hand on the
    modified sets, and differ from the image without the pupil"""
    from metalens_amd import _lib
    from test_gpu_propagate_sets import SWEEP_WEIGHTS, _sweep_sources
    sw, p, ap, lens = _sweep(ma, ctx)
    sources = _sweep_sources(lens)
    without = sw.run(sources, weights=SWEEP_WEIGHTS, image=p)
    got = sw.run(sources, weights=SWEEP_WEIGHTS, image=p, pupil=ap)
    assert got['I_sum'].tobytes() != without['I_sum'].tobytes() and np.array_equal(got['power_in'], without['power_in'])
    lib = ctx.lib
    sw.prepare()
    groups = sw._group(sources)
    assert [len(g['members']) for g in groups] == [3, 2]
    for g in groups:
        params, n = _params(sw, g)
        _lib.check(lib.ml_nearfield_batch_async(ctx.handle, params, n, _lib.dptr(sw.x), sw.x.size, _lib.dptr(sw.y), sw.y.size))
        if len(set(g['positions'])) == 1:
            _lib.check(lib.ml_nearfield_members_async(ctx.handle, params, n, _lib.dptr(sw.x), sw.x.size, _lib.dptr(sw.y), sw.y.size, 1))
        ap.queue(0, n)
        p.queue_sets(0, n)
        p.accumulate([SWEEP_WEIGHTS[k] for k, pol in g['members']], reset=g['members'][0][0] == 0)
    I, Sz = p.sums()
    assert I.max() > 0 and I.tobytes() == got['I_sum'].tobytes() and Sz.tobytes() == got['Sz_sum'].tobytes()
    _lib.check(lib.ml_fields_select(ctx.handle, 0))


def test_sweep_refuses_a_foreign_pupil(ma, ctx):
    from metalens_amd import _lib
    sw, _p, ap, lens = _sweep(ma, ctx)
    src = [(0.0, 0.0, -lens['source_distance'], 'x')]
    other = ma.AperturePupil(sw.x[:-1], sw.y, 10e-6, centre=(50.5e-6, 1.0e-6), ctx=ctx)
    with pytest.raises(ValueError, match=r"pupil= was built for an aperture of 95 x 130 samples, the sweep's grid has 96 x 130"):
        sw.run(src, pupil=other)
    c = _lib.Context(0)
    try:
        with pytest.raises(ValueError, match='pupil= must be an AperturePupil built on the context of this sweep'):
            sw.queue(src, pupil=ma.AperturePupil(sw.x, sw.y, 10e-6, centre=(50.5e-6, 1.0e-6), ctx=c))
    finally:
        c.close()


def test_state_errors(ma, ctx, monkeypatch):
    """(9) no plan, no resident set, a shape mismatch and a multi-rank context: ML_ESTATE or ML_EINVAL with their wording, and
    a refused call changes nothing"""
    from metalens_amd import _lib
    x, y = (np.arange(20) - 9.5) * 1e-7, (np.arange(24) - 11.5) * 1e-7
    F = ref.seeded_fields(1, 20, 24, seed=1)
    R = 8e-7
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        assert c.lib.ml_fields_pupil_apply(c.handle, 0, 1) == -4                # ML_ESTATE
        with pytest.raises(_lib.MetalensHipError, match=r'ml_fields_pupil_apply: no pupil has been planned on this context \(ml_fields_pupil_plan\)'):
            _lib.check(c.lib.ml_fields_pupil_apply(c.handle, 0, 1))
        ap = ma.AperturePupil(x, y, R, phase=[0.0, 0.1, 0.2], ctx=c)
        with pytest.raises(_lib.MetalensHipError, match='no resident field set'):
            ap.apply(0, 1)
        _upload(c, F[0])
        with pytest.raises(_lib.MetalensHipError, match='ml_fields_pupil_apply: field sets 1 ... 1 asked for, 1 resident'):
            ap.apply(1, 1)
        with pytest.raises(_lib.MetalensHipError, match='field sets 0 ... 1 asked for, 1 resident'):
            ap.apply(0, 2)
        short = ma.AperturePupil(x, y[:-1], R, ctx=c)
        said = 'ml_fields_pupil_apply: the pupil was planned for 20 x 23 samples, the resident field sets have 20 x 24'
        with pytest.raises(_lib.MetalensHipError, match=said):
            short.apply()
        assert c.lib.ml_fields_pupil_apply(c.handle, 0, 1) == -4 and c.lib.ml_fields_pupil_apply(c.handle, 0, 4) == -1      # ML_ESTATE, ML_EINVAL
        # a refused plan leaves the plan before in place; a refused pass changed nothing
        g = np.array([[np.nan, 0.0]])
        e2 = np.array([1.0])
        rc = c.lib.ml_fields_pupil_plan(c.handle, _lib.dptr(ap._x2), _lib.dptr(ap._xi), 20, _lib.dptr(ap._y2), _lib.dptr(ap._eta), 24, R * R, 1, 0,
                                        None, _lib.dptr(e2), 1, _lib.dptr(g))
        assert rc != 0 and b'g[0] = (nan, 0): a zone factor must be finite' in c.lib.ml_last_error()
        with pytest.raises(_lib.MetalensHipError, match=said):
            _lib.check(c.lib.ml_fields_pupil_apply(c.handle, 0, 1))
        assert _download(c, 0, (20, 24)).tobytes() == F[0].tobytes()
        ap.apply()
        ref.hold('gpu second context', _download(c, 0, (20, 24))[None], F, ref.parts(x, y, R, phase=[0.0, 0.1, 0.2]))
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        with pytest.raises(_lib.MetalensHipError, match='ml_fields_pupil_apply: this context belongs to a communicator of 2 ranks'):
            ap.apply(0, 1)
        with pytest.raises(_lib.MetalensHipError, match='ml_fields_pupil_plan: this context belongs to a communicator of 2 ranks'):
            ma.AperturePupil(x, y, R, ctx=c).apply(0, 1)
    finally:
        c.close()
