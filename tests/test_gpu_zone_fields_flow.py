"""The zone contributions in the design flow, on a synthesised lens (needs an MI355X): the contributions of a small
collimator's zones at points behind it against the long-double yardstick on the downloaded field and, added up, against
the direct propagator; ``AperturePupil.from_zone_fields`` applied and analysed again against the host twins
(``apply_pupil_host``, then ``postprocess.zone_fields`` in long double); and ``SourceSweep.run(zone_fields=...)`` for the x, y
and z dipoles of one emitter."""
import numpy as np
import pytest

import propagate_ref
import zone_fields_ref as ref

pytestmark = pytest.mark.gpu

WL = 580e-9
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


def _download(ctx, m, shape):
    from metalens_amd import _lib
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
    F = [np.empty(shape, dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    return np.stack(F)


def _amplitude(d, p):
    """|p^H E| at target 0 of set 0 from the dict of ``analyse``"""
    return float(np.abs((np.conj(p) * d['total_E'][0, :, 0]).sum()))


def test_measure_correct_and_look_again(ma, ctx):
    from metalens_amd import postprocess
    from test_gpu_parity import _synthetic_lens
    lens = _synthetic_lens(40e-6, 0.4, WL, switch_deg=9.0)
    S = lens['lens_periphery_summary']
    R, f = S['r_max_list'][-1], lens['source_distance']
    n = 320
    x = (np.arange(n) - (n - 1) / 2) * (2.1 * R / n)
    assert x[-1] > R and x[1] - x[0] < WL / 2
    n_glass = ma.build_nearfield(0.3e-6, -0.2e-6, -f, 'x', WL, S, lens['lens_center_summary'], lens['hexgridset'], x_pts=x, y_pts=x, ctx=ctx,
                                 download=False)[7]
    edges = ma.zone_edges(S)
    pts = np.array([[0.0, 0.0, f], [1.5e-6, -0.7e-6, 0.5 * f]])            # "the focus": the emitter's mirror point, and one more
    azf = ma.ApertureZoneFields(x, x, WL, n_glass, edges, pts, Z0=Z0, ctx=ctx)
    got = azf.analyse()                       # before any download: the resident synthesis
    F = _download(ctx, 0, (n, n))[None]
    want = ref.yardstick(F, x, x, WL, n_glass, edges, (0.0, 0.0), pts)
    assert (want['n'] > 0).all()
    ref.hold('gpu lens', got, want)
    # closure against the direct propagator at the points
    prop = ma.PlanePropagator(x, x, WL, n_glass, pts[:, 0], pts[:, 1], pts[:, 2], point_list=True, Z0=Z0, ctx=ctx)
    d = prop.propagate()
    for fld, whole in (('E', np.stack([d['Ex'], d['Ey'], d['Ez']])), ('H', np.stack([d['Hx'], d['Hy'], d['Hz']]))):
        err = float(np.abs(got['total_' + fld][0] - whole).max() / np.abs(want[fld]).max())
        assert err <= 2 * ref.MARGIN * want['e_ref_' + fld], (fld, err)
    # the correction: every zone turned onto the polarisation of the field at the focus
    p = got['polarisation'][0, :, 0]
    pupil = ma.AperturePupil.from_zone_fields(azf, got, set=0, target=0)
    g = np.exp(-1j * got['phase'][0, :, 0])
    pupil.apply()
    after = azf.analyse(polarisation=p)
    F2 = np.stack(postprocess.apply_pupil_host(F[0, 0], F[0, 1], F[0, 2], F[0, 3], x, x, edges[-1], edges=edges, zone_factors=g))[None]
    want2 = ref.yardstick(F2, x, x, WL, n_glass, edges, (0.0, 0.0), pts)
    ref.hold('gpu lens, corrected', after, want2)
    twin = postprocess.zone_fields(F2[0, 0], F2[0, 1], F2[0, 2], F2[0, 3], x, x, WL, n_glass, edges, pts, Z0=Z0, polarisation=p, real=np.longdouble)
    for fld in ('E', 'H'):
        err = propagate_ref.max_error(ref.slots(after, fld), ref.slots(twin, fld))
        assert err <= ref.MARGIN * want2['e_ref_' + fld], (fld, err)
    d2 = prop.propagate()                      # the re-propagated field against the twin's total
    for fld, whole in (('E', np.stack([d2['Ex'], d2['Ey'], d2['Ez']])), ('H', np.stack([d2['Hx'], d2['Hy'], d2['Hz']]))):
        err = float(np.abs(whole.astype(np.clongdouble) - twin['total_' + fld][0]).max() / np.abs(want2[fld]).max())
        assert err <= 2 * ref.MARGIN * want2['e_ref_' + fld], (fld, err)
    # the zones are aligned now, and the amplitude along p at the focus is not smaller than before
    held = ~np.isnan(after['phase'][0, :, 0])
    assert held.all() and np.abs(after['phase'][0, held, 0]).max() < 1e-9
    a0, a1 = _amplitude(got, p), _amplitude(after, p)
    print('PARITY zone fields lens  |p^H E| before %.6g after %.6g aligned %.6g' % (a0, a1, got['aligned'][0, 0]))
    assert a1 >= a0 and a1 <= got['aligned'][0, 0] * (1 + 1e-9)
    assert after['outside'] == got['outside'] > 0 and (after['outside_E'] == 0).all()          # the stop cleared the outside


def test_sweep_with_zone_fields(ma, ctx):
    """the x, y and z dipoles of one emitter, one synthesis batch: ``zone_E`` of every source has the bits of the pass run alone
    on that resident set, and the sweep's other results are those of a run without the keyword"""
    from test_gpu_propagate_sets import _common, _lens, _window
    lens = _lens()
    x, y = _window('A')
    u = np.linspace(-0.2, 0.2, 24)
    sw = ma.SourceSweep(*_common(lens), x, y, u, u, ctx=ctx)
    f = lens['source_distance']
    sources = [(0.3e-6, -0.2e-6, -f, pol) for pol in 'xyz']
    edges = ma.zone_edges(lens['lens_periphery_summary'])
    pts = np.array([[x.mean(), y.mean(), 2e-6], [0.0, 0.0, f], [x[0] - 30e-6, y[-1] + 10e-6, 20e-6]])
    azf = ma.ApertureZoneFields(x, y, WL, sw.n_glass, edges, pts, Z0=Z0, ctx=ctx)
    plain = sw.run(sources, cone=0.1)
    out = sw.run(sources, cone=0.1, zone_fields=azf)
    K = edges.size
    assert out['zone_E'].shape == (3, K, 3, 3) and out['zone_H'].shape == (3, K, 3, 3) and out['zone_outside_E'].shape == (3, 3, 3)
    assert set(out) - set(plain) == {'zone_E', 'zone_H', 'zone_outside_E', 'zone_outside_H'}
    for key in plain:
        assert np.array_equal(np.asarray(out[key]), np.asarray(plain[key]), equal_nan=True), key
    for m in range(3):                        # the batch is still resident
        alone = azf.analyse(m, 1)
        assert np.array_equal(alone['E'][0], out['zone_E'][m]) and np.array_equal(alone['H'][0], out['zone_H'][m]), m
        assert np.array_equal(alone['outside_E'][0], out['zone_outside_E'][m]) and np.abs(out['zone_E'][m]).max() > 0
    assert not np.array_equal(out['zone_E'][0], out['zone_E'][1])
    only_e = sw.run(sources, zone_fields=ma.ApertureZoneFields(x, y, WL, sw.n_glass, edges, pts, want_h=False, Z0=Z0, ctx=ctx))
    assert 'zone_H' not in only_e and np.array_equal(only_e['zone_E'], out['zone_E'])
    other = ma.ApertureZoneFields(x, y[:-1], WL, sw.n_glass, edges, pts, Z0=Z0, ctx=ctx)
    with pytest.raises(ValueError, match="zone_fields= was built for an aperture of 96 x 129 samples, the sweep's grid has 96 x 130"):
        sw.run(sources, zone_fields=other)
