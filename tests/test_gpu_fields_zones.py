"""Per-zone sums of the resident near field on the GPU (csrc/fields_zones.hip, ml_fields_zones, ``ApertureZones``) against
the long-double yardstick (tests/fields_zones_ref.py) within its derived bounds, and the byte-level requirements: (a) two
calls agree, (b) the record of a set does not depend on the other sets of the call, (c) the record of a zone does not
depend on the other edges.  Needs an MI355X.

Fields are seeded random complex arrays through ml_fields_upload unless said otherwise.  The shapes are chosen for where
the line kernel can go wrong: a vertex on a block's first lane (130 x 129) and inside a block (70 x 257), lines without a
vertex (centre outside the grid), one block exactly and one sample more, a single line, lines of three samples, more
edges than samples, one edge, samples exactly on an edge."""
import numpy as np
import pytest

import fields_zones_ref as ref

pytestmark = pytest.mark.gpu

WL, NG = 580e-9, 1.46
P = WL / 2.2


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
    """40 edges, ten of them 0.04 um apart - closer than the pitch of 0.26 um: empty zones, zones a line skips"""
    return np.sort(np.concatenate([np.linspace(1e-6, 30e-6, 30), 9e-6 + np.arange(10) * 0.04e-6]))


# name -> (x, y, wavelength, n_glass, edges, centre, reference)
def _case(name):
    if name == '130x129':      # the centre in the axes' middle: between samples along x, on sample 64 - a block's first lane - along y
        x, y = _axes(130, 129, 64.5, 64)
        return x, y, WL, NG, np.linspace(2e-6, 17e-6, 12), (0.0, 0.0), ('focus', 0.0, 0.0, 30e-6)
    if name == '70x257':       # the centre off every sample, the vertex at lane 37 of the second block; oblique plane wave
        x, y = _axes(70, 257, 30.3, 100.7)
        return x, y, WL, NG, _tight_edges(), (0.37e-6, -1.21e-6), ('plane', 0.3, -0.2)
    if name == '33x300':       # the centre outside the grid: every line monotone, the vertex the line's first sample
        x, y = _axes(33, 300, -20.0, -7.4)
        return x, y, WL, NG, np.linspace(3e-6, 80e-6, 300), (0.0, 0.0), ('focus', 2e-6, 1e-6, -50e-6)
    if name == '33x300 descending':   # the same lines walked the other way: the vertex their last sample, side R empty
        x, y = _axes(33, 300, -20.0, -7.4)
        return x, y[::-1], WL, NG, np.linspace(3e-6, 80e-6, 300), (0.0, 0.0), ('plane', -0.5, 0.1)
    if name in ('1x1', '3x64', '3x65', '64x3'):
        nx, ny = (int(v) for v in name.split('x'))
        x, y = _axes(nx, ny, (nx - 1) / 2, ny / 3)
        return x, y, WL, NG, np.linspace(0.0, 12e-6, 7), (0.0, 0.0), ('focus', 0.0, 1e-6, 20e-6)
    if name == '64x70 K=4096':   # far more zones than samples
        x, y = _axes(64, 70, 30.5, 33.2)
        return x, y, WL, NG, np.linspace(0.05e-6, 11e-6, 4096), (0.0, 0.0), ('plane', 0.1, 0.0)
    if name == '64x70 K=1':
        x, y = _axes(64, 70, 30.5, 33.2)
        return x, y, WL, NG, np.array([6e-6]), (0.0, 0.0), ('plane', 0.1, 0.0)
    if name == 'integers':     # x = i, y = j: (3, 4) and (5, 12) lie exactly on the edges 5 and 13
        return np.arange(16.0), np.arange(70.0), 4.0, 1.0, np.array([5.0, 13.0]), (0.0, 0.0), ('plane', 0.6, 0.0)
    raise KeyError(name)


CASES = ['130x129', '70x257', '33x300', '33x300 descending', '1x1', '3x64', '3x65', '64x3', '64x70 K=4096', '64x70 K=1', 'integers']


def _run(ma, ctx, name, F, case):
    """upload, analyse twice (a), hold against the yardstick -> (ApertureZones, records, dict, yardstick)"""
    x, y, wl, ng, edges, centre, reference = case
    _upload(ctx, F[0])
    az = ma.ApertureZones(x, y, wl, ng, edges, centre=centre, reference=reference, ctx=ctx)
    rec = az.records()
    assert rec.shape == (1, len(edges), 8) and np.array_equal(rec, az.records())          # (a)
    got = az.analyse()
    want = ref.exact(F, x, y, wl, ng, edges, centre, reference)
    ref.hold('gpu ' + name, got, want)
    return az, rec, got, want


@pytest.mark.parametrize('name', CASES, ids=lambda n: n.replace(' ', '_'))
def test_zones_against_the_yardstick(ma, ctx, name):
    case = _case(name)
    x, y = case[0], case[1]
    F = ref.seeded_fields(1, x.size, y.size, seed=17 + x.size * 1000 + y.size)
    az, rec, got, want = _run(ma, ctx, name, F, case)
    assert want['n'].sum() > 0
    empty = want['n'] == 0
    # a zone without samples: zero sums, NaN coherence
    assert (rec[0][empty] == 0).all() and np.isnan(got['coherence'][0][empty]).all()
    if name == '64x70 K=4096':
        assert empty.sum() > 4096 // 2 and (~empty).sum() > 100          # most zones are empty
    if name == '70x257':
        assert empty.any() and want['outside'] > 0
    if name == '64x70 K=1':
        assert got['samples'].shape == (1,) and got['samples'][0] + got['outside'] == 64 * 70
    if name == 'integers':
        zone = ref.membership(x, y, case[4], case[5])
        assert zone[3, 4] == 0 and zone[4, 3] == 0 and zone[5, 12] == 1 and zone[12, 5] == 1 and zone[4, 4] == 1 and zone[5, 13] == 2
        assert got['samples'].tolist() == [int((zone == 0).sum()), int((zone == 1).sum())]
    # the one-shot call on host arrays: the same numbers
    one = ma.aperture_zones(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, y, case[2], case[3], case[4], centre=case[5], reference=case[6], ctx=ctx)
    assert all(np.array_equal(one[k], got[k], equal_nan=True) for k in got)


def test_a_zone_does_not_depend_on_the_other_edges(ma, ctx):
    """(c): the record of zone (e_a, e_b] in the list of 40 edges has the bytes of that zone with edges = [e_a, e_b] alone -
    for the first, a middle and the last zone that holds samples, and for the disc"""
    name = '70x257'
    x, y, wl, ng, edges, centre, reference = _case(name)
    F = ref.seeded_fields(1, x.size, y.size, seed=5)
    az, rec, got, want = _run(ma, ctx, name, F, _case(name))
    held = np.flatnonzero(want['n'][1:] > 0) + 1
    assert held.size >= 3
    for z in (held[0], held[held.size // 2], held[-1]):
        alone = ma.ApertureZones(x, y, wl, ng, edges[z - 1:z + 1], centre=centre, reference=reference, ctx=ctx).records()
        assert alone.shape == (1, 2, 8) and alone[0, 1, 0] == want['n'][z] > 0
        assert alone[0, 1].tobytes() == rec[0, z].tobytes(), z
    disc = ma.ApertureZones(x, y, wl, ng, edges[:1], centre=centre, reference=reference, ctx=ctx).records()
    assert disc[0, 0].tobytes() == rec[0, 0].tobytes() and disc[0, 0, 0] > 0
    # ... and a zone cut in two by one more edge: its members add up, and every other zone keeps its bytes
    z = held[held.size // 2]
    cut = np.insert(edges, z, 0.5 * (edges[z - 1] + edges[z]))
    parts = ma.ApertureZones(x, y, wl, ng, cut, centre=centre, reference=reference, ctx=ctx).records()
    assert parts[0, z, 0] + parts[0, z + 1, 0] == rec[0, z, 0]
    assert np.array_equal(np.delete(parts[0], [z, z + 1], axis=0), np.delete(rec[0], z, axis=0))


def test_zero_fields_outside_a_disc(ma, ctx):
    """a field that is exactly zero (of either sign) outside a disc: the zones beyond it have members, zero sums and NaN
    coherence, and the zones inside are what they are without the zeros"""
    name = '130x129'
    case = _case(name)
    x, y = case[0], case[1]
    F = ref.seeded_fields(1, x.size, y.size, seed=23)
    inside = x[:, None] ** 2 + y[None, :] ** 2 <= (8e-6) ** 2
    F0 = np.where(inside, F, -0.0 * F)
    az, rec, got, want = _run(ma, ctx, 'zero outside a disc', F0, case)
    full = ma.aperture_zones(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, y, *case[2:5], centre=case[5], reference=case[6], ctx=ctx)
    beyond = case[4] > 8e-6 + 2e-6
    within = case[4] <= 8e-6
    assert beyond.sum() >= 4 and within.sum() >= 3 and (want['n'][beyond] > 0).all()
    assert (rec[0][beyond][:, 1:] == 0).all() and not np.signbit(rec[0][beyond][:, 1:]).any()
    assert np.isnan(got['coherence'][0][beyond]).all()
    for key in ('P', 'I', 'overlap', 'coherence'):
        assert np.array_equal(got[key][0][within], full[key][0][within]), key


def _download(ctx, m, shape):
    from metalens_amd import _lib
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
    F = [np.empty(shape, dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    return np.stack(F)


def test_three_set_batch(ma, ctx):
    """the x, y, z dipoles of test_gpu_propagate_sets.py's lens on its window A (it crosses ring boundaries and the lens
    edge), zones from the layout: one pass over the three resident sets against the yardstick and the twin on the fields
    downloaded afterwards; (b) every set alone and the pair (1, 2) have the bytes of the batch"""
    from metalens_amd import _lib, postprocess
    from test_gpu_propagate_sets import DIPOLES, _batch, _lens
    x, y, n_glass, n = _batch(ma, ctx, 'A', DIPOLES)
    assert n == 3
    edges = ma.zone_edges(_lens()['lens_periphery_summary'])
    az = ma.ApertureZones(x, y, WL, n_glass, edges, reference=('plane', 0.0, 0.0), ctx=ctx)
    rec = az.records()
    assert rec.shape == (3, edges.size, 8) and np.array_equal(rec, az.records(0, 3))             # (a)
    got = az.analyse()
    for m in range(3):
        assert az.records(m, 1)[0].tobytes() == rec[m].tobytes(), m                           # (b)
    assert az.records(1, 2).tobytes() == rec[1:].tobytes() and az.records(0, 2).tobytes() == rec[:2].tobytes()
    F = np.stack([_download(ctx, m, (x.size, y.size)) for m in range(3)])
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))
    want = ref.exact(F, x, y, WL, n_glass, edges)
    assert (want['n'] > 0).sum() >= 5 and want['outside'] > 0 and all(np.abs(F[m]).max() > 0 for m in range(3))
    ref.hold('gpu three-set batch', got, want)
    twin = postprocess.zone_metrics(F[:, 0], F[:, 1], F[:, 2], F[:, 3], x, y, WL, n_glass, edges)
    ref.hold('twin three-set batch', twin, want)
    assert np.array_equal(twin['samples'], got['samples']) and np.array_equal(rec[0, :, 0], rec[2, :, 0])
    held = want['n'] > 0
    assert np.allclose(twin['coherence'][:, held], got['coherence'][:, held], rtol=1e-9, atol=0)


def test_premodulated_synthesis_is_unmodulated_first(ma, ctx):
    """a synthesis under ml_nearfield_premodulate, set up as in test_gpu_parity.py's test_fused_input_modulation, leaves the
    resident fields modulated: ``analyse`` BEFORE any download sees the plain near field - what the download returns"""
    from metalens_amd import _lib
    from metalens_amd.pipeline import HotPath
    from test_gpu_parity import _synthetic_lens
    lens = _synthetic_lens(40e-6, 0.4, WL, switch_deg=9.0)
    S = lens['lens_periphery_summary']
    R = S['r_max_list'][-1]
    x = np.linspace(-R, R, 384)
    u = (np.arange(96) - 48) * 0.004            # bins -48 .. 47: symmetric about -0.002, so the modulation exists
    hp = HotPath((0.3e-6, -0.2e-6, -lens['source_distance'], 'y'), WL, S, lens['lens_center_summary'], lens['hexgridset'], x, x, u, u,
                 ctx=ctx, fuse_modulation=True)
    hp.step()
    hp.sync()
    edges = ma.zone_edges(S)
    az = ma.ApertureZones(x, x, WL, hp.n_glass, edges, reference=('plane', 0.0, 0.0), ctx=ctx)
    got = az.analyse()                          # before the download
    F = _download(ctx, 0, (x.size, x.size))[None]
    want = ref.exact(F, x, x, WL, hp.n_glass, edges)
    ref.hold('gpu premodulated synthesis', got, want)
    assert np.array_equal(az.records(), az.records()) and (want['n'] > 0).all()
    _lib.check(ctx.lib.ml_nearfield_premodulate(ctx.handle, 0))


def test_refusals(ma, ctx, monkeypatch):
    """messages only: nothing is launched"""
    from metalens_amd import _lib
    x, y = _axes(20, 24, 9.5, 11.5)
    F = ref.seeded_fields(1, 20, 24, seed=1)
    _upload(ctx, F[0])
    edges = [2e-6, 4e-6]
    before = ma.ApertureZones(x, y, WL, NG, edges, ctx=ctx).records()
    with pytest.raises(_lib.MetalensHipError, match='the axes have 20 x 23 samples, the resident field sets 20 x 24'):
        ma.ApertureZones(x, y[:-1], WL, NG, edges, ctx=ctx).analyse()
    with pytest.raises(_lib.MetalensHipError, match=r'the reference phase reaches 1\.58\d*e\+09 rad on this grid: the phase arithmetic covers up to 1e\+09'):
        ma.ApertureZones(x, y, WL, NG, edges, reference=('focus', 0.0, 0.0, 100.0), ctx=ctx).analyse()
    with pytest.raises(_lib.MetalensHipError, match='field sets 1 ... 1 asked for, 1 resident'):
        ma.ApertureZones(x, y, WL, NG, edges, ctx=ctx).analyse(first=1, n=1)
    with pytest.raises(_lib.MetalensHipError, match='field sets 0 ... 1 asked for, 1 resident'):
        ma.ApertureZones(x, y, WL, NG, edges, ctx=ctx).analyse(n=2)
    assert np.array_equal(ma.ApertureZones(x, y, WL, NG, edges, ctx=ctx).records(), before)      # a refused call changes nothing
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.MetalensHipError, match='no resident field set'):
            ma.ApertureZones(x, y, WL, NG, edges, ctx=c).analyse(n=1)
        _upload(c, F[0])
        assert np.array_equal(ma.ApertureZones(x, y, WL, NG, edges, ctx=c).records(), before)
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        with pytest.raises(_lib.MetalensHipError, match='ml_fields_zones: this context belongs to a communicator of 2 ranks'):
            ma.ApertureZones(x, y, WL, NG, edges, ctx=c).analyse(n=1)
    finally:
        c.close()
