"""Zernike moments of the resident near field's wavefront on the GPU (csrc/fields_wavefront.hip, ml_fields_zernike,
``ApertureWavefront``) against the long-double yardstick (tests/fields_wavefront_ref.py) within its derived bounds, and the
byte-level requirements: (a) two calls agree, (b) the record of a set does not depend on the other sets of the call, (c)
the first J' terms of a call of order 8 are those of the call of order 4 to the bit, (d) the one-shot call on host arrays
gives the numbers of the resident call, (e) after a premodulated synthesis the record is that of the downloaded and
re-uploaded fields.  Needs an MI355X.

Fields are seeded random complex arrays through ml_fields_upload unless said otherwise.  The shapes are chosen for where
the kernels can go wrong: a vertex on a block's first lane (130 x 129) and inside a block (70 x 257), lines without a
vertex (centre outside the grid, y ascending and descending), one block exactly and one sample more, a single sample,
lines of three samples, more lines than the sum kernel has lanes (300 x 70), a pupil that holds the whole grid, one sample
or none, a sample exactly on the rim; the orders 0, 4, 5 and 8 reach both instantiations of the line kernel at both ends."""
import numpy as np
import pytest

import fields_wavefront_ref as ref

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


def _download(ctx, m, shape):
    from metalens_amd import _lib
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
    F = [np.empty(shape, dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    return np.stack(F)


def _axes(nx, ny, cx, cy):
    """axes on the pitch with the origin between samples (cx, cy: where 0 lies, in samples)"""
    return (np.arange(nx) - cx) * P, (np.arange(ny) - cy) * P


# name -> (x, y, wavelength, n_glass, radius, centre, reference)
def _case(name):
    if name == '130x129':      # the centre in the axes' middle: between samples along x, on sample 64 - a block's first lane - along y
        x, y = _axes(130, 129, 64.5, 64)
        return x, y, WL, NG, 15e-6, (0.0, 0.0), ('focus', 0.0, 0.0, 30e-6)
    if name == '70x257':       # the centre off every sample, the vertex at lane 37 of the second block; oblique plane wave
        x, y = _axes(70, 257, 30.3, 100.7)
        return x, y, WL, NG, 9.1e-6, (0.37e-6, -1.21e-6), ('plane', 0.3, -0.2)
    if name == '33x300':       # the centre outside the grid: every line monotone, the vertex the line's first sample
        x, y = _axes(33, 300, -20.0, -7.4)
        return x, y, WL, NG, 30e-6, (0.0, 0.0), ('focus', 2e-6, 1e-6, -50e-6)
    if name == '33x300 descending':   # the same lines walked the other way: the vertex their last sample
        x, y = _axes(33, 300, -20.0, -7.4)
        return x, y[::-1], WL, NG, 30e-6, (0.0, 0.0), ('plane', -0.5, 0.1)
    if name in ('1x1', '3x64', '3x65', '64x3'):
        nx, ny = (int(v) for v in name.split('x'))
        x, y = _axes(nx, ny, (nx - 1) / 2, ny / 3)
        return x, y, WL, NG, 7e-6, (0.0, 0.0), ('focus', 0.0, 1e-6, 20e-6)
    if name == '300x70':       # more lines than the sum kernel has lanes; lines outside the pupil at both ends
        x, y = _axes(300, 70, 151.3, 33.2)
        return x, y, WL, NG, 38e-6, (0.0, 0.0), ('plane', 0.1, 0.0)
    if name == 'whole grid':   # every sample is a member
        x, y = _axes(64, 70, 30.5, 33.2)
        return x, y, WL, NG, 20e-6, (0.0, 0.0), ('plane', 0.1, 0.0)
    if name == 'one sample':   # the pupil about sample (31, 40) holds that sample alone
        x, y = _axes(64, 70, 30.5, 33.2)
        return x, y, WL, NG, 0.3 * P, (x[31], y[40]), ('plane', 0.1, 0.0)
    if name == 'no sample':    # the pupil lies between the samples
        x, y = _axes(64, 70, 30.5, 33.5)
        return x, y, WL, NG, 0.3 * P, (0.0, 0.0), ('plane', 0.1, 0.0)
    if name == 'integers':     # x = i, y = j: (3, 4), (4, 3), (5, 0) and (0, 5) lie exactly on R = 5
        return np.arange(16.0), np.arange(70.0), 4.0, 1.0, 5.0, (0.0, 0.0), ('plane', 0.6, 0.0)
    raise KeyError(name)


CASES = [('130x129', 0), ('130x129', 4), ('130x129', 5), ('130x129', 8), ('70x257', 8), ('33x300', 5), ('33x300 descending', 4),
         ('1x1', 8), ('3x64', 4), ('3x65', 5), ('64x3', 8), ('300x70', 8), ('300x70', 3), ('whole grid', 8), ('one sample', 5),
         ('no sample', 4), ('integers', 8)]


def _run(ma, ctx, name, F, case, n_max):
    """upload, analyse twice (a), hold against the yardstick -> (ApertureWavefront, records, dict, yardstick)"""
    x, y, wl, ng, radius, centre, reference = case
    _upload(ctx, F[0])
    aw = ma.ApertureWavefront(x, y, wl, ng, radius, n_max=n_max, centre=centre, reference=reference, ctx=ctx)
    rec = aw.records()
    J = (n_max + 1) * (n_max + 2) // 2
    assert rec.shape == (1, 4 + 4 * J) and rec.tobytes() == aw.records().tobytes()          # (a)
    got = aw.analyse()
    want = ref.exact(F, x, y, wl, ng, radius, n_max, centre, reference)
    ref.hold('gpu %s order %d' % (name, n_max), got, want)
    return aw, rec, got, want


@pytest.mark.parametrize('name,n_max', CASES, ids=lambda v: str(v).replace(' ', '_'))
def test_wavefront_against_the_yardstick(ma, ctx, name, n_max):
    case = _case(name)
    x, y = case[0], case[1]
    F = ref.seeded_fields(1, x.size, y.size, seed=29 + x.size * 1000 + y.size)
    aw, rec, got, want = _run(ma, ctx, name, F, case, n_max)
    assert not (np.signbit(rec) & (rec == 0)).any()                # no sum is ever -0.0
    if name == 'no sample':
        assert want['n'] == 0 and got['samples'] == 0 and got['outside'] == x.size * y.size
        assert (rec == 0).all() and not np.signbit(rec).any()
        assert np.isnan(got['coherence']).all() and np.isnan(got['wavefront']).all() and np.isnan(got['rms']).all()
        assert (got['piston'] == 0).all() and (got['P'] == 0).all()
    else:
        assert want['n'] > 0
    if name == 'one sample':
        assert got['samples'] == 1 and np.allclose(got['coherence'], 1.0, rtol=0, atol=1e-14)
    if name == 'whole grid':
        assert got['samples'] == x.size * y.size and got['outside'] == 0
    if name in ('300x70', '70x257', '130x129'):
        assert want['outside'] > 0
    if name == '300x70':
        held = ref.membership(x, y, case[4], case[5]).any(axis=1)
        assert not held[0] and not held[-1] and 256 < held.sum() < 300          # lines outside at both ends; some lanes add two lines
    if name == 'integers':
        inside = ref.membership(x, y, 5.0, (0.0, 0.0))
        assert inside[3, 4] and inside[4, 3] and inside[5, 0] and inside[0, 5] and not inside[4, 4] and not inside[5, 1]
        assert got['samples'] == int(inside.sum()) == 26
    # (d) the one-shot call on host arrays: the same numbers
    one = ma.aperture_wavefront(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, y, case[2], case[3], case[4], n_max=n_max, centre=case[5],
                                reference=case[6], ctx=ctx)
    assert set(one) == set(got) and all(np.array_equal(one[k], got[k], equal_nan=True) for k in got)


def test_lower_orders_do_not_depend_on_n_max(ma, ctx):
    """(c): the header sums and the first J' terms of the call of order 8 have the bytes of the call of order n', across the two
    instantiations of the line kernel (4 | 5) and inside each (0, 3 | 5, 7)"""
    name = '70x257'
    x, y, wl, ng, radius, centre, reference = _case(name)
    F = ref.seeded_fields(1, x.size, y.size, seed=7)
    _upload(ctx, F[0])
    rec = {n: ma.ApertureWavefront(x, y, wl, ng, radius, n_max=n, centre=centre, reference=reference, ctx=ctx).records() for n in (0, 3, 4, 5, 7, 8)}
    assert rec[8].shape == (1, 184) and rec[8][0, 0] > 1000 and (rec[8][0, 4:] != 0).all()
    for n in (0, 3, 4, 5, 7):
        assert rec[n].tobytes() == rec[8][:, :rec[n].shape[1]].tobytes(), n


def test_three_set_batch(ma, ctx):
    """the x, y, z dipoles of test_gpu_propagate_sets.py's lens on its window A, a pupil that crosses ring boundaries and leaves
    part of the window outside: one pass over the three resident sets against the yardstick on the fields downloaded
    afterwards; (b) every set alone and the pairs have the bytes of the batch, in both instantiations"""
    from metalens_amd import _lib
    from test_gpu_propagate_sets import DIPOLES, _batch
    x, y, n_glass, n = _batch(ma, ctx, 'A', DIPOLES)
    assert n == 3
    centre, radius = (50.5e-6, 1.0e-6), 11e-6
    F = None
    for n_max in (4, 8):
        aw = ma.ApertureWavefront(x, y, WL, n_glass, radius, n_max=n_max, centre=centre, reference=('plane', 0.3, 0.0), ctx=ctx)
        rec = aw.records()
        assert rec.shape == (3, 4 + 2 * (n_max + 1) * (n_max + 2)) and rec.tobytes() == aw.records(0, 3).tobytes()      # (a)
        got = aw.analyse()
        for m in range(3):
            assert aw.records(m, 1)[0].tobytes() == rec[m].tobytes(), m                           # (b)
        assert aw.records(1, 2).tobytes() == rec[1:].tobytes() and aw.records(0, 2).tobytes() == rec[:2].tobytes()
        if F is None:
            F = np.stack([_download(ctx, m, (x.size, y.size)) for m in range(3)])
            _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))
        want = ref.exact(F, x, y, WL, n_glass, radius, n_max, centre, ('plane', 0.3, 0.0))
        assert want['n'] > 1000 and want['outside'] > 0 and all(np.abs(F[m]).max() > 0 for m in range(3))
        ref.hold('gpu three-set batch order %d' % n_max, got, want)
        assert rec[0, 0] == rec[1, 0] == rec[2, 0] == want['n']


def test_premodulated_synthesis_is_unmodulated_first(ma, ctx):
    """(e): a synthesis under ml_nearfield_premodulate, set up as in test_gpu_fields_zones.py, leaves the resident fields
    modulated: ``records`` BEFORE any download sees the plain near field - the record of the downloaded and re-uploaded
    fields, to the bit"""
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
    aw = ma.ApertureWavefront(x, x, WL, hp.n_glass, R, n_max=5, reference=('plane', 0.0, 0.0), ctx=ctx)
    rec = aw.records()                          # before the download
    got = aw.analyse()
    F = _download(ctx, 0, (x.size, x.size))[None]
    want = ref.exact(F, x, x, WL, hp.n_glass, R, 5)
    ref.hold('gpu premodulated synthesis', got, want)
    _lib.check(ctx.lib.ml_nearfield_premodulate(ctx.handle, 0))
    _upload(ctx, F[0])
    assert aw.records().tobytes() == rec.tobytes() and want['n'] > 0 and want['outside'] > 0


def test_small_lens_resident_against_the_twin(ma, ctx):
    """a real small lens from synthetic tables: ``build_nearfield(..., download=False)``, then ``ApertureWavefront`` on the resident
    field against ``wavefront_metrics`` of the download - within the sum of both bounds, that is each within its own against the
    yardstick - for an emitter 2 um off axis and the plane wave its chief ray takes"""
    import math

    from metalens_amd import _lib, layout, postprocess, synthetic
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design, radius=30e-6, numerical_aperture=0.5,
                               wavelength=WL, periphery_orders='physical')
    f, S = lens['source_distance'], lens['lens_periphery_summary']
    x, y, _, n_glass = ma.build_nearfield(2e-6, 0.0, -f, 'x', WL, S, lens['lens_center_summary'], lens['hexgridset'], ctx=ctx,
                                          download=False)[4:8]
    R = float(S['r_max_list'][-1])
    reference = ('plane', -2e-6 / math.sqrt(4e-12 + f * f) / n_glass, 0.0)
    got = ma.ApertureWavefront(x, y, WL, n_glass, R, n_max=4, reference=reference, ctx=ctx).analyse()
    F = _download(ctx, 0, (x.size, y.size))[None]
    twin = postprocess.wavefront_metrics(F[:, 0], F[:, 1], F[:, 2], F[:, 3], x, y, WL, n_glass, R, 4, reference=reference)
    want = ref.exact(F, x, y, WL, n_glass, R, 4, reference=reference)
    ref.hold('gpu small lens', got, want)
    ref.hold('twin small lens', twin, want)
    assert got['samples'] == twin['samples'] > 1000 and (got['coherence'] > 0).all() and np.isfinite(got['rms']).all()
    # both moments lie within the bound B_j of the yardstick's, so to first order the readings m_j / m_0 differ by at most
    # 2 (B_j + |m_j / m_0| B_0) / |m_0|; a quarter more for the higher orders
    B = ref.moment_bound(want).astype(float)
    m0 = np.abs(twin['moments'][..., :1])
    tol = 2.5 * (B + np.abs(twin['moments']) / m0 * B[..., :1]) / m0
    print('small lens: wavefront GPU - twin at most %.3g rad, allowed %.3g; rms %s' % (np.abs(got['wavefront'] - twin['wavefront']).max(), tol.max(), got['rms']))
    assert (np.abs(got['wavefront'] - twin['wavefront']) <= tol).all()
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))


def test_refusals(ma, ctx, monkeypatch):
    """messages only: nothing is launched"""
    from metalens_amd import _lib
    x, y = _axes(20, 24, 9.5, 11.5)
    F = ref.seeded_fields(1, 20, 24, seed=1)
    _upload(ctx, F[0])
    R = 2e-6
    before = ma.ApertureWavefront(x, y, WL, NG, R, ctx=ctx).records()
    with pytest.raises(_lib.MetalensHipError, match='ml_fields_zernike: the axes have 20 x 23 samples, the resident field sets 20 x 24'):
        ma.ApertureWavefront(x, y[:-1], WL, NG, R, ctx=ctx).analyse()
    with pytest.raises(_lib.MetalensHipError, match=r'the reference phase reaches 1\.58\d*e\+09 rad on this grid: the phase arithmetic covers up to 1e\+09'):
        ma.ApertureWavefront(x, y, WL, NG, R, reference=('focus', 0.0, 0.0, 100.0), ctx=ctx).analyse()
    with pytest.raises(_lib.MetalensHipError, match='ml_fields_zernike: field sets 1 ... 1 asked for, 1 resident'):
        ma.ApertureWavefront(x, y, WL, NG, R, ctx=ctx).analyse(first=1, n=1)
    with pytest.raises(_lib.MetalensHipError, match='field sets 0 ... 1 asked for, 1 resident'):
        ma.ApertureWavefront(x, y, WL, NG, R, ctx=ctx).analyse(n=2)
    assert np.array_equal(ma.ApertureWavefront(x, y, WL, NG, R, ctx=ctx).records(), before)      # a refused call changes nothing
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.MetalensHipError, match='no resident field set'):
            ma.ApertureWavefront(x, y, WL, NG, R, ctx=c).analyse(n=1)
        _upload(c, F[0])
        assert np.array_equal(ma.ApertureWavefront(x, y, WL, NG, R, ctx=c).records(), before)
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        with pytest.raises(_lib.MetalensHipError, match='ml_fields_zernike: this context belongs to a communicator of 2 ranks'):
            ma.ApertureWavefront(x, y, WL, NG, R, ctx=c).analyse(n=1)
    finally:
        c.close()
