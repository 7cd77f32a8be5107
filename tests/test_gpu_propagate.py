"""The finite-distance propagator on the GPU (csrc/propagate.hip, metalens_amd/propagate.py) against the NumPy
restatement of tests/propagate_ref.py, against the reference-pinned far field, and as a guest on a context
that other API objects use.  Needs an MI355X.

Parity bound.  The error of a result is max |difference| over all components and targets / max |E| (resp. |H|)
of the long-double sum.  ``e_ref`` is that error of the plain-fp64 NumPy sum; the GPU must stay within
8 x e_ref: two correct fp64 sums in different order differ by a small multiple of each other's rounding, and a
sincos or a square root that loses digits at k R = 1e4 fails by orders of magnitude.  The measured pairs are
printed as ``PARITY ...`` lines (run with -s; they belong in profiles/propagate_parity.txt)."""
import functools

import numpy as np
import pytest

import propagate_ref as ref
from test_gpu_fft import fields
from test_gpu_fft_mixed import _axes

pytestmark = pytest.mark.gpu

WL, N_GLASS = ref.WL, ref.N_GLASS
APERTURES = [(96, 80), (130, 61)]


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


def _target_set(name, x, y):
    """-> x, y, z, point_list.  'near': a 24 x 17 grid 2 um behind the aperture, inside its footprint; 'far': the
    same grid 1 mm away, reaching well outside the footprint; 'points': 300 points with z of their own from 2 um
    to 1 mm, a third of them up to two aperture widths outside"""
    cx, cy, wx, wy = x.mean(), y.mean(), np.ptp(x), np.ptp(y)
    if name == 'near':
        return cx + np.linspace(-0.4, 0.45, 24) * wx, cy + np.linspace(-0.45, 0.4, 17) * wy, 2e-6, False
    if name == 'far':
        return cx + np.linspace(-2.5, 1.5, 24) * wx, cy + np.linspace(-1.0, 3.0, 17) * wy, 1e-3, False
    rng = np.random.default_rng(7)
    spread = np.where(np.arange(300) % 3 == 0, 2.5, 0.5)
    return (cx + rng.uniform(-1, 1, 300) * spread * wx, cy + rng.uniform(-1, 1, 300) * spread * wy,
            2e-6 * 500 ** rng.uniform(0, 1, 300), True)


def _points(tx, ty, tz, point_list):
    if point_list:
        return np.stack([tx, ty, tz], axis=1)
    TX, TY = np.meshgrid(tx, ty, indexing='ij')
    return np.stack([TX.ravel(), TY.ravel(), np.full(TX.size, tz)], axis=1)


@functools.lru_cache(maxsize=None)
def _reference(nx, ny, name):
    x, y = _axes(nx, ny)
    F = fields(nx, ny, nx + ny)
    pts = _points(*_target_set(name, x, y))
    E64, H64 = ref.direct_sum(*F, x, y, WL, N_GLASS, pts)
    El, Hl = ref.direct_sum(*F, x, y, WL, N_GLASS, pts, real=np.longdouble)
    return F, x, y, El, Hl, ref.max_error(E64, El), ref.max_error(H64, Hl)


def _stack(out, keys, n):
    return np.stack([out[k].reshape(n) for k in keys])


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
@pytest.mark.parametrize('name', ['near', 'far', 'points'])
@pytest.mark.parametrize('nx,ny', APERTURES)
def test_against_the_direct_sum(ma, ctx, nx, ny, name, want_h):
    F, x, y, El, Hl, eE_ref, eH_ref = _reference(nx, ny, name)
    tx, ty, tz, point_list = _target_set(name, x, y)
    out = ma.field_at_plane(*F, x, y, WL, N_GLASS, tx, ty, tz, point_list=point_list, want_h=want_h, ctx=ctx)
    n = El.shape[1]
    assert out['Ex'].shape == ((300,) if point_list else (24, 17))
    eE = ref.max_error(_stack(out, ('Ex', 'Ey', 'Ez'), n), El)
    print('PARITY %dx%d %-6s %-2s E: e_ref %.3e gpu %.3e' % (nx, ny, name, 'EH' if want_h else 'E', eE_ref, eE))
    assert eE <= 8 * eE_ref
    if want_h:
        eH = ref.max_error(_stack(out, ('Hx', 'Hy', 'Hz'), n), Hl)
        print('PARITY %dx%d %-6s EH H: e_ref %.3e gpu %.3e' % (nx, ny, name, eH_ref, eH))
        assert eH <= 8 * eH_ref
        S = ref.poynting(_stack(out, ('Ex', 'Ey', 'Ez'), n), _stack(out, ('Hx', 'Hy', 'Hz'), n))
        assert np.array_equal(out['Sz'].reshape(n), S[2])
    else:
        assert set(out) == {'Ex', 'Ey', 'Ez', 'I'}
        assert np.array_equal(out['I'].reshape(n), (np.abs(_stack(out, ('Ex', 'Ey', 'Ez'), n)) ** 2).sum(axis=0))


def test_far_limit_is_the_reference_pinned_far_field(ma, ctx):
    """rho^2 S_r from field_at_plane at rho = 1 m against farfield_direct's P at the same directions (the 9 x 9 fan
    and the bound of test_propagate_host.py, which the NumPy sum meets on the CPU): signs, the x 2 and Z0 / n_glass
    are those the reference fixtures pin"""
    F, x, beam = ref.tilted_gaussian()
    ux, uy = ref.fan(beam)
    P = ma.farfield_direct(*F, x, x, WL, N_GLASS, ux, uy, ctx=ctx)['P']
    rho = 1.0
    pts, _ = ref.fan_points(ux, uy, rho)
    out = ma.field_at_plane(*F, x, x, WL, N_GLASS, pts[:, 0], pts[:, 1], pts[:, 2], point_list=True, ctx=ctx)
    S = ref.poynting(_stack(out, ('Ex', 'Ey', 'Ez'), 81), _stack(out, ('Hx', 'Hy', 'Hz'), 81))
    S_r = (S * (pts / rho).T).sum(axis=0).reshape(P.shape)
    want = ref.radiant_intensity(P, ux, uy)
    err = np.abs(rho ** 2 * S_r - want).max() / want.max()
    print('PARITY far limit at 1 m: %.3e of the peak' % err)
    assert err <= 1e-8


def _lens_512(ma):
    from test_gpu_parity import _synthetic_lens
    return _synthetic_lens(60e-6, 0.4, WL, switch_deg=9.0)


def test_resident_equals_uploaded(ma, ctx):
    """a synthesised field (row extents: rows and row ends outside the lens are skipped) against the same arrays
    uploaded (no extents: the whole sum).  ACHIEVED: bit-identical - the rows are dealt to the workgroups by the
    sizes alone and a skipped sample is an exact zero, which adds +-0 to every accumulator - so the assertion is
    equality, inside any parity bound"""
    lens = _lens_512(ma)
    n = 512
    x = (np.arange(n) - (n - 1) / 2) * (WL / 2.2)
    assert x[-1] > lens['lens_periphery_summary']['r_max_list'][-1]       # rows outside the lens exist
    args = dict(source_x=0.2e-6, source_y=-0.1e-6, source_z=-lens['source_distance'], source_pol='x', wavelength=WL,
                lens_periphery_summary=lens['lens_periphery_summary'], lens_center_summary=lens['lens_center_summary'],
                hexgridset=lens['hexgridset'], x_pts=x, y_pts=x, ctx=ctx)
    _, _, _, _, xs, ys, _, n_glass = ma.build_nearfield(**args, download=False)
    t = np.linspace(-12e-6, 15e-6, 32)
    resident = ma.field_at_plane(None, None, None, None, xs, ys, WL, n_glass, t, t, 20e-6, ctx=ctx)
    F = ma.build_nearfield(**args)[:4]
    assert max(np.abs(f[0]).max() for f in F) == 0 and np.abs(F[0]).max() > 0
    uploaded = ma.field_at_plane(*F, xs, ys, WL, n_glass, t, t, 20e-6, ctx=ctx)
    for key in ('Ex', 'Ey', 'Ez', 'Hx', 'Hy', 'Hz', 'Sz'):
        assert np.abs(resident[key]).max() > 0
        assert np.array_equal(resident[key], uploaded[key]), key
    with pytest.raises(ValueError, match='resident near field is 512 x 512'):
        ma.field_at_plane(None, None, None, None, xs[:500], ys, WL, n_glass, t, t, 20e-6, ctx=ctx)


def test_a_focus_is_where_it_should_be(ma, ctx):
    """ideal converging wave, sin theta = 0.5 in the medium, f = 91 um: |E|^2 on the plane z = f peaks on the axis
    with the scalar Airy width w = 0.51 lambda / (n sin theta) to 10 % (the NumPy sum: 1.040 w along the
    polarisation, 0.972 w across it), and the on-axis cut peaks at z = f.  Parity of the same 171 points: against
    the long-double sum on every eighth point the 8 x e_ref rule as it stands; against the plain-fp64 sum on all
    of them 9 x that e_ref (the rule plus the fp64 sum's own error, by the triangle inequality)."""
    F, x, f, w = ref.converging_wave()
    assert abs(f - 91e-6) < 1e-6
    t = np.linspace(-1.6 * w, 1.6 * w, 65)
    dof = WL / (N_GLASS * 0.25)
    zs = np.linspace(f - 4 * dof, f + 4 * dof, 41)
    o = np.zeros(65)
    px = np.concatenate([t, o, np.zeros(41)])
    py = np.concatenate([o, t, np.zeros(41)])
    pz = np.concatenate([np.full(130, f), zs])
    out = ma.field_at_plane(*F, x, x, WL, N_GLASS, px, py, pz, point_list=True, want_h=False, ctx=ctx)
    I = out['I']
    Ix, Iy, Iz = I[:65], I[65:130], I[130:]
    assert Ix.argmax() == 32 and Iy.argmax() == 32
    wx, wy = ref.fwhm(t, Ix) / w, ref.fwhm(t, Iy) / w
    print('PARITY focus: FWHM %.3f w along x, %.3f w along y; axial peak at sample %d of 41' % (wx, wy, Iz.argmax()))
    assert abs(wx - 1) <= 0.1 and abs(wy - 1) <= 0.1
    assert Iz.argmax() == 20 and zs[20] == pytest.approx(f, rel=1e-12)
    got = _stack(out, ('Ex', 'Ey', 'Ez'), 171)
    pts = np.stack([px, py, pz], axis=1)
    E64 = ref.direct_sum(*F, x, x, WL, N_GLASS, pts, want_h=False)
    sub = np.arange(0, 171, 8)
    El = ref.direct_sum(*F, x, x, WL, N_GLASS, pts[sub], real=np.longdouble, want_h=False)
    e_ref, e_gpu = ref.max_error(E64[:, sub], El), ref.max_error(got[:, sub], El)
    e_all = ref.max_error(got, E64)
    print('PARITY focus 400x400: e_ref %.3e gpu %.3e (22 points, long double); gpu against fp64 on 171 points %.3e'
          % (e_ref, e_gpu, e_all))
    assert e_gpu <= 8 * e_ref
    assert e_all <= 9 * e_ref


def test_repeatable_and_linear(ma, ctx):
    nx, ny = APERTURES[0]
    x, y = _axes(nx, ny)
    F = fields(nx, ny, 3)
    tx, ty, tz, _ = _target_set('points', x, y)
    p = ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, tz, point_list=True, ctx=ctx)
    from test_gpu_fft_mixed import _upload
    _upload(ctx, F)
    a, b = p.propagate(), p.propagate()
    _upload(ctx, [2 * f for f in F])
    c = p.propagate()
    for key in ('Ex', 'Ey', 'Ez', 'Hx', 'Hy', 'Hz'):
        assert np.abs(a[key]).min() > 0
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(c[key], 2 * a[key]), key


def _sums(ctx, shape):
    from metalens_amd import _lib
    P, total, cone = np.empty(shape), np.zeros(1), np.zeros(1)
    _lib.check(ctx.lib.ml_farfield_sums(ctx.handle, _lib.dptr(P), _lib.dptr(total), _lib.dptr(cone), 1))
    return P, total, cone


def test_state_is_left_alone(ma, ctx, monkeypatch):
    from metalens_amd import _lib
    from test_gpu_fft_mixed import _upload
    nx, ny = APERTURES[1]
    x, y = _axes(nx, ny)
    F = fields(nx, ny, 21)
    ux, uy = np.linspace(-0.3, 0.3, 20), np.linspace(-0.2, 0.22, 24)
    ctx.set_method('gemm')
    t = ma.FarfieldTransform(nx, ny, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux, uy, ctx=ctx)
    _upload(ctx, F)
    t.transform()
    vectors, proj = t.radiation_vectors(), t.project()
    _lib.check(ctx.lib.ml_farfield_accumulate(ctx.handle, 1.0, 0.1, 0.0, 0.0, 0, 1))
    sums = _sums(ctx, proj[0].shape)
    serial = []
    monkeypatch.setattr(t, '_plan', lambda: serial.append('planned again'))
    # two propagators on the context, alternating
    tx, ty, tz, _ = _target_set('points', x, y)
    p1 = ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, tz, point_list=True, ctx=ctx)
    p2 = ma.PlanePropagator(x, y, WL, N_GLASS, tx[:40] + 1e-6, ty[:40], 30e-6, want_h=False, ctx=ctx)
    a1, a2, b1, b2 = p1.propagate(), p2.propagate(), p1.propagate(), p2.propagate()
    assert a1['Ex'].shape == (300,) and a2['Ex'].shape == (40, 40) and 'Hx' not in a2
    for a, b in ((a1, b1), (a2, b2)):
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    alone = ma.field_at_plane(*F, x, y, WL, N_GLASS, tx, ty, tz, point_list=True, ctx=ctx)
    assert all(np.array_equal(alone[key], a1[key]) for key in alone)
    # the far-field side of the context is as it was
    assert ctx.method == 'gemm' and ctx.precision == 'f64' and ctx.plan_owner == t.owner
    for got, want in zip(_sums(ctx, proj[0].shape), sums):
        assert np.array_equal(got, want)
    after = t.radiation_vectors()
    assert all(np.array_equal(after[k], vectors[k]) for k in vectors)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(t.project(), proj))
    t.transform()
    again = t.radiation_vectors()
    assert all(np.array_equal(again[k], vectors[k]) for k in vectors)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(t.project(), proj))
    assert serial == []
    ctx.set_method('auto')


def test_a_multi_rank_context_refuses(ma, monkeypatch):
    from metalens_amd import _lib
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    ident = (_lib.c_uint8 * 128)()
    _lib.check(c.lib.ml_comm_unique_id(ident))
    _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
    x = (np.arange(32) - 15.5) * (WL / 2.2)
    with pytest.raises(_lib.MetalensHipError, match='communicator of 2 ranks'):
        ma.PlanePropagator(x, x, WL, N_GLASS, [0.0], [0.0], 5e-6, ctx=c)
    c.close()
