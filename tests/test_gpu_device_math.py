"""The device arithmetic of csrc/nearfield_math.h on the GPU, one function per lane through ml_math_probe
(csrc/math_probe.hip, built with the library's flags), and the range guards that keep the hot kernels inside what is
tested here.  Needs an MI355X.

- sincos_cw, reduce_pio2, sincos_cw_q: BIT-IDENTICAL to the host restatement (tools/device_math.cpp) on every set of
  tests/device_math_cases.py, signs of zero and quadrant counts included.  No hardware estimate enters them, so a
  difference is a finding about the compiler or the text; the restatement's accuracy (2^-51 against mpmath,
  tests/test_device_math_host.py) is then the kernels'.
- sqrt_exact: bit-identical to np.sqrt (correctly rounded) on every set.
- the bare v_rcp_f64 / v_rsq_f64 estimates: within 2^-22 relative of the long-double value.  That is the largest error
  at which the host model of the three sequences was checked, i.e. the condition under which its conclusions hold on
  this chip - not a tuned number.
- recip, rsqrt_fast: within 2^-52 relative of the long-double value: the final rounding, <= 2^-53; for rsqrt_fast the
  rounding of x y entering e = 1 - (x y) y at half weight, <= 2^-54; the truncation e^3 ~ 2^-70.
- ml_math_probe's refusals; the k R <= 1e9 guards of the propagation plans and of the near field.
The measured figures are printed as ``PARITY ...`` lines (run with -s; they belong in profiles/device_math.txt)."""
import math
import os

import numpy as np
import pytest

import device_math_cases as dc

pytestmark = pytest.mark.gpu

SINCOS, SINCOS_Q, REDUCE, SQRT, RECIP, RSQRT, RAW_RCP, RAW_RSQ = range(8)
LIMIT = 1e9


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


@pytest.fixture(scope='module')
def ctx(ma):
    from metalens_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('device_math')) + os.sep
    return dc.Tool(dc.build_tool(out), out)


def probe_rc(ctx, op, x, kq, n, out0, out1, outk):
    from metalens_amd import _lib
    return ctx.lib.ml_math_probe(ctx.handle, op, _lib.dptr(x), None if kq is None else _lib.iptr(kq), n, _lib.dptr(out0),
                                 _lib.dptr(out1), None if outk is None else _lib.iptr(outk))


def probe(ctx, op, x, kq=None):
    """-> out0, out1, outk of ml_math_probe (what the op does not write is None)"""
    from metalens_amd import _lib
    x = _lib.f64(x)
    out0 = np.full(x.size, np.nan)
    out1 = np.full(x.size, np.nan) if op in (SINCOS, SINCOS_Q) else None
    outk = np.full(x.size, -12345, dtype=np.int32) if op == REDUCE else None
    if kq is not None:
        kq = np.ascontiguousarray(kq, dtype=np.int32)
    _lib.check(probe_rc(ctx, op, x, kq, x.size, out0, out1, outk))
    return out0, out1, outk


def _same_bits(what, got, want, x):
    bad = np.nonzero(dc.bits(got) != dc.bits(want))[0]
    if bad.size:
        print('PARITY %s: %d of %d differ; first x %s gpu %s want %s'
              % (what, bad.size, x.size, [float.hex(float(v)) for v in x[bad[:4]]],
                 [float.hex(float(v)) for v in got[bad[:4]]], [float.hex(float(v)) for v in want[bad[:4]]]))
    return bad.size


@pytest.mark.parametrize('name', dc.SINCOS_SETS)
def test_sincos_and_reduce_have_the_restatement_s_bits(ctx, tool, name):
    x = dc.sincos_set(name)
    s, c, _ = probe(ctx, SINCOS, x)
    s_w, c_w = tool.sincos(x)
    r, _, k = probe(ctx, REDUCE, x)
    r_w, k_w = tool.reduce(x)
    n_bad = (_same_bits('sincos %s sin' % name, s, s_w, x), _same_bits('sincos %s cos' % name, c, c_w, x),
             _same_bits('reduce %s r' % name, r, r_w, x), int(np.sum(k != k_w)))
    print('PARITY sincos_cw / reduce_pio2 %-14s n %7d differing from the restatement: sin %d cos %d r %d k %d'
          % ((name, x.size) + n_bad))
    assert n_bad == (0, 0, 0, 0)


def test_composite_has_the_restatement_s_bits(ctx, tool):
    """x = r + a0, kq as the centre kernels form them, r from the GPU's own reduce_pio2 (which the test above holds to
    the restatement's bits), every kq in -4 ... 7"""
    r, a0, x, kq = dc.composite(lambda big: probe(ctx, REDUCE, big)[::2])
    r_w, _, _, _ = dc.composite(tool.reduce)
    assert np.array_equal(dc.bits(r), dc.bits(r_w))
    s, c, _ = probe(ctx, SINCOS_Q, x, kq)
    s_w, c_w = tool.sincos(x, kq)
    n_bad = (_same_bits('sincos_q sin', s, s_w, x), _same_bits('sincos_q cos', c, c_w, x))
    print('PARITY sincos_cw_q composite n %7d differing from the restatement: sin %d cos %d' % ((x.size,) + n_bad))
    assert n_bad == (0, 0)


@pytest.mark.parametrize('name', dc.SQRT_SETS)
def test_sqrt_exact_is_np_sqrt(ctx, name):
    x = dc.sqrt_set(name)
    got = probe(ctx, SQRT, x)[0]
    n_bad = _same_bits('sqrt_exact %s' % name, got, np.sqrt(x), x)
    print('PARITY sqrt_exact %-10s n %7d differing from np.sqrt: %d' % (name, x.size, n_bad))
    assert n_bad == 0


@pytest.mark.parametrize('op', ['rcp', 'rsq'])
def test_hardware_estimates_are_within_the_modelled_error(ctx, op):
    x = dc.recip_set() if op == 'rcp' else dc.rsqrt_set()
    xl = x.astype(np.longdouble)
    got = probe(ctx, RAW_RCP if op == 'rcp' else RAW_RSQ, x)[0]
    e = dc.rel_error_ld(got, 1 / xl if op == 'rcp' else 1 / np.sqrt(xl))
    print('PARITY v_%s_f64 n %7d max relative error %.3e = 2^%.2f (modelled up to 2^-22 = %.3e)'
          % (op, x.size, e.max(), math.log2(e.max()) if e.max() > 0 else -math.inf, 2.0 ** -22))
    assert e.max() <= 2.0 ** -22


@pytest.mark.parametrize('op', ['recip', 'rsqrt'])
def test_reciprocals_are_within_an_ulp(ctx, op):
    x = dc.recip_set() if op == 'recip' else dc.rsqrt_set()
    xl = x.astype(np.longdouble)
    got = probe(ctx, RECIP if op == 'recip' else RSQRT, x)[0]
    e = dc.rel_error_ld(got, 1 / xl if op == 'recip' else 1 / np.sqrt(xl))
    exact = dc.correctly_rounded_recip(x) if op == 'recip' else dc.correctly_rounded_rsqrt(x)
    print('PARITY %-10s n %7d max relative error %.3e (bound 2^-52 = %.3e), not correctly rounded %.4f %%'
          % ('recip' if op == 'recip' else 'rsqrt_fast', x.size, e.max(), 2.0 ** -52, 100 * np.mean(got != exact)))
    assert e.max() <= 2.0 ** -52


def test_probe_refusals(ctx):
    from metalens_amd import _lib
    x, kq = np.ones(4), np.zeros(4, dtype=np.int32)
    o0, o1, ok = np.empty(4), np.empty(4), np.empty(4, dtype=np.int32)

    def refused(match, *args):
        with pytest.raises(_lib.MetalensHipError, match=match):
            _lib.check(probe_rc(ctx, *args))

    refused('unknown op 8', 8, x, kq, 4, o0, o1, ok)
    refused('unknown op -1', -1, x, kq, 4, o0, o1, ok)
    refused('NULL argument', SQRT, None, None, 4, o0, None, None)
    refused('NULL argument', SQRT, x, None, 4, None, None, None)
    refused('n = 0 values', SQRT, x, None, 0, o0, None, None)
    refused(r'n = 16777217 values, 1 \.\.\. 2\^24', SQRT, x, None, (1 << 24) + 1, o0, None, None)
    refused('needs the quadrants kq', SINCOS_Q, x, None, 4, o0, o1, None)
    refused('out1 is NULL', SINCOS, x, None, 4, o0, None, None)
    refused('outk is NULL', REDUCE, x, None, 4, o0, None, None)
    with pytest.raises(_lib.MetalensHipError, match='NULL argument'):
        _lib.check(ctx.lib.ml_math_probe(None, SQRT, _lib.dptr(x), None, 4, _lib.dptr(o0), None, None))
    # and a refusal leaves the entry usable
    assert np.array_equal(probe(ctx, SQRT, np.array([4.0, 9.0]))[0], [2.0, 3.0])


# ---- the guards: k R <= 1e9 -------------------------------------------------------------------------------------

def _aperture():
    import propagate_ref as ref
    from test_gpu_fft import fields
    from test_gpu_fft_mixed import _axes
    x, y = _axes(96, 80)
    return fields(96, 80, 5), x, y, 2 * np.pi * ref.N_GLASS / ref.WL


def _largest_R(x, y, tx, ty, z):
    """common.h prop_largest_R for the targets' bounding box"""
    dx = max(abs(t - a) for t in (min(tx), max(tx)) for a in (x[0], x[-1]))
    dy = max(abs(t - a) for t in (min(ty), max(ty)) for a in (y[0], y[-1]))
    return math.sqrt(dx * dx + dy * dy + z * z)


def _upload(ctx, F):
    from test_gpu_fft_mixed import _upload as up
    up(ctx, F)


def _raw_plan(ctx, x, y, tx, ty, z):
    import propagate_ref as ref
    from metalens_amd import _lib
    tx, ty, z = _lib.f64(tx), _lib.f64(ty), _lib.f64([z])
    return ctx.lib.ml_propagate_plan(ctx.handle, float(x[0]), float(y[0]), float(x[1] - x[0]), float(y[1] - y[0]), ref.WL,
                                     ref.N_GLASS, _lib.dptr(tx), tx.size, _lib.dptr(ty), ty.size, _lib.dptr(z), 1, 0, 1)


def test_direct_plan_just_inside_the_limit_runs(ma, ctx):
    """three targets whose largest possible k R is 0.9999e9: accepted, and within 8 x e_ref of the long-double direct sum
    as every other target set of tests/test_gpu_propagate.py"""
    import propagate_ref as ref
    F, x, y, k = _aperture()
    tx, ty = x.mean() + np.array([-1e-3, 0.0, 2e-3]), np.array([y.mean()])
    z = 0.9999 * LIMIT / k
    z = math.sqrt(z * z - (_largest_R(x, y, tx, ty, 0.0)) ** 2)
    kR = k * _largest_R(x, y, tx, ty, z)
    assert 0.9998 * LIMIT < kR < LIMIT
    out = ma.field_at_plane(*F, x, y, ref.WL, ref.N_GLASS, tx, ty, z, ctx=ctx)
    pts = np.stack([tx, np.full(3, ty[0]), np.full(3, z)], axis=1)
    E64, H64 = ref.direct_sum(*F, x, y, ref.WL, ref.N_GLASS, pts)
    El, Hl = ref.direct_sum(*F, x, y, ref.WL, ref.N_GLASS, pts, real=np.longdouble)
    for name, keys, got64, want in (('E', ('Ex', 'Ey', 'Ez'), E64, El), ('H', ('Hx', 'Hy', 'Hz'), H64, Hl)):
        got = np.stack([out[key].reshape(3) for key in keys])
        e_ref, e_gpu = ref.max_error(got64, want), ref.max_error(got, want)
        print('PARITY direct plan at k R = %.5e %s: e_ref %.3e gpu %.3e' % (kR, name, e_ref, e_gpu))
        assert np.abs(got).min() > 0 and e_gpu <= 8 * e_ref


def test_direct_plan_outside_the_limit_is_refused_and_the_earlier_plan_still_serves(ma, ctx):
    import propagate_ref as ref
    from metalens_amd import _lib
    F, x, y, k = _aperture()
    tx, ty = x.mean() + np.linspace(-3e-6, 4e-6, 9), y.mean() + np.linspace(-2e-6, 2e-6, 7)
    p = ma.PlanePropagator(x, y, ref.WL, ref.N_GLASS, tx, ty, 40e-6, ctx=ctx)
    _upload(ctx, F)
    before = p.propagate()
    z = 1.0001 * LIMIT / k
    assert LIMIT < k * _largest_R(x, y, tx, ty, z) < 1.0002 * LIMIT
    with pytest.raises(_lib.MetalensHipError, match=r'ml_propagate_plan: a target can lie 63\.2\d* m from a sample of the '
                       r'96 x 80 aperture, k R = 1\.0001\d*e\+09: the phase arithmetic covers k R up to 1e\+09'):
        _lib.check(_raw_plan(ctx, x, y, tx, ty, z))
    _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))      # (no plan call in between: the earlier plan as it was)
    after = p._download(None)
    for key in before:
        assert np.abs(before[key]).max() > 0 and np.array_equal(before[key], after[key]), key


def test_a_pass_refuses_what_the_plan_could_not_know(ma):
    """a plan made while no field set is resident is checked by the pass, against the shape it meets"""
    import propagate_ref as ref
    from metalens_amd import _lib
    F, x, y, k = _aperture()
    c = _lib.Context(0)
    _lib.check(_raw_plan(c, x, y, [x.mean()], [y.mean()], 1.0001 * LIMIT / k))
    _upload(c, F)
    with pytest.raises(_lib.MetalensHipError, match=r'ml_propagate: a target can lie .* 96 x 80 aperture.*up to 1e\+09'):
        _lib.check(c.lib.ml_propagate(c.handle, 376.73))
    c.close()


def _grid_entries(ctx, geometry, tx0, ty0, z):
    """the four FFT-form plan entries for 8 x 6 targets on the pitch (the fine one: on half the pitch)"""
    from metalens_amd import _lib
    lib, h = ctx.lib, ctx.handle
    first_x, first_y = _lib.f64([tx0, tx0 + geometry[2] / 2]), _lib.f64([ty0, ty0 + geometry[3] / 2])
    return {
        'ml_propagate_plan_grid': lambda: lib.ml_propagate_plan_grid(h, *geometry, tx0, ty0, 8, 6, z, 1),
        'ml_propagate_plan_grid_long': lambda: lib.ml_propagate_plan_grid_long(h, *geometry, tx0, ty0, 8, 6, z, 1),
        'ml_propagate_plan_grid_tiled': lambda: lib.ml_propagate_plan_grid_tiled(h, *geometry, tx0, ty0, 8, 6, z, 1, 0, 0),
        'ml_propagate_plan_grid_fine': lambda: lib.ml_propagate_plan_grid_fine(h, *geometry, _lib.dptr(first_x), 2,
                                                                               _lib.dptr(first_y), 2, 8, 6, z, 1, 0, 0, 1),
    }


def test_fft_plans_are_held_to_the_same_limit(ma, ctx):
    import propagate_ref as ref
    from metalens_amd import _lib
    F, x, y, k = _aperture()
    d = (x[1] - x[0], y[1] - y[0])
    geometry = (float(x[0]), float(y[0]), float(d[0]), float(d[1]), ref.WL, ref.N_GLASS)
    tx, ty = x[40] + d[0] * np.arange(8), y[30] + d[1] * np.arange(6)
    p = ma.PlanePropagator(x, y, ref.WL, ref.N_GLASS, tx, ty, 40e-6, ctx=ctx, method='fft')
    _upload(ctx, F)
    before = p.propagate()
    z_out = 1.0001 * LIMIT / k
    for entry, call in _grid_entries(ctx, geometry, float(tx[0]), float(ty[0]), z_out).items():
        with pytest.raises(_lib.MetalensHipError, match=entry + r': a target can lie 63\.2\d* m from a sample of the 96 x 80 '
                           r'aperture, k R = 1\.0001\d*e\+09: the phase arithmetic covers k R up to 1e\+09'):
            _lib.check(call())
        _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))   # the earlier plan, as it was
        after = p._download(None)
        for key in before:
            assert np.abs(before[key]).max() > 0 and np.array_equal(before[key], after[key]), (entry, key)
    # just inside: every entry plans and propagates
    z_in = 0.9999 * LIMIT / k
    z_in = math.sqrt(z_in * z_in - _largest_R(x, y, tx, ty, 0.0) ** 2)
    assert 0.9998 * LIMIT < k * _largest_R(x, y, tx, ty, z_in) < LIMIT
    for entry, call in _grid_entries(ctx, geometry, float(tx[0]), float(ty[0]), z_in).items():
        ctx.propagate_owner = None          # (the Python objects plan again after these raw calls)
        _lib.check(call())
        _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))
        E = np.empty((3, 48), dtype=np.complex128)
        _lib.check(ctx.lib.ml_propagate_download(ctx.handle, _lib.dptr(E), None))
        assert np.isfinite(E.view(np.float64)).all() and np.abs(E).min() > 0, entry


def _small_lens(ma):
    from metalens_amd import layout, synthetic
    return synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design, radius=20e-6,
                               numerical_aperture=0.3, wavelength=580e-9, switch_angle=8 * math.pi / 180, num_gratings=8,
                               num_entries=8)


def test_near_field_source_at_the_limit(ma, ctx):
    """a source 0.9999 of the limit away is synthesised, to the oracle within the bound of smoke() (1e-11 of the field's
    scale: the phase arguments are the reference's bit for bit, and sin / cos are within 2^-51 up to 1e9); one 1.0001 of
    it away is refused, and the resident field set is as it was"""
    from metalens_amd import _lib
    from oracle import nearfield_oracle
    wl = 580e-9
    lens = _small_lens(ma)
    kvac = 2 * np.pi / wl
    r_outer = lens['lens_periphery_summary']['r_max_list'][-1]
    args = dict(source_x=0.3e-6, source_y=-0.2e-6, source_pol='x', wavelength=wl,
                lens_periphery_summary=lens['lens_periphery_summary'], lens_center_summary=lens['lens_center_summary'],
                hexgridset=lens['hexgridset'])
    rho = math.hypot(0.3e-6, 0.2e-6) + r_outer
    z_in, z_out = 0.9999 * LIMIT / kvac, 1.0001 * LIMIT / kvac
    assert 0.9998 * LIMIT < kvac * math.hypot(rho, z_in) < LIMIT < kvac * math.hypot(rho, z_out)
    got = ma.build_nearfield(source_z=-z_in, ctx=ctx, **args)
    want = nearfield_oracle.build_nearfield(source_z=-z_in, **args)
    err = max(np.abs(g - w).max() / np.abs(w).max() for g, w in zip(got[:4], want[:4]))
    print('PARITY near field, source at k R = %.5e: %.3e of the field scale against the oracle' % (kvac * math.hypot(rho, z_in), err))
    assert err < 1e-11
    kept = [np.array(g) for g in got[:4]]
    with pytest.raises(_lib.MetalensHipError, match=r'source 0 lies up to 92\.3\d* m from a sample of the lens, '
                       r'k R = 1\.0001\d*e\+09: the phase arithmetic covers k R up to 1e\+09'):
        ma.build_nearfield(source_z=-z_out, ctx=ctx, **args)
    out = [np.empty_like(a) for a in kept]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in out]))
    assert all(np.array_equal(a, b) for a, b in zip(out, kept))
    # the plane wave has no such phase and is not touched by the guard
    pw = ma.build_nearfield(source_z=-math.inf, ctx=ctx, **args)
    assert np.abs(pw[0]).max() > 0
