"""The finite-distance propagator without a GPU: the NumPy restatement the GPU tests compare with
(tests/propagate_ref.py) passes the two checks that fix its signs and factors, the public names and the C-ABI
entries exist, and argument errors are raised before any device call."""
import numpy as np
import pytest

import propagate_ref as ref


def test_far_limit_is_the_references_far_field():
    """rho^2 S_r at rho = 1 m against P uz / 2 of the reference's formula (nearfield_farfield.py:184-189, with its
    x 2; oracle/farfield_oracle.py, its two regularisers taken out: propagate_ref.radiant_intensity) over a 9 x 9
    fan of directions around the beam (propagate_ref.fan), normalised by the peak: the Fresnel correction there is
    (k w^2 / 2 rho)^2 = 2.4e-9 for the beam's waist, the bound 4 x that.  Ties the signs, the x 2 and Z0 / n_glass
    to what the reference fixtures pin."""
    from oracle import farfield_oracle
    F, x, beam = ref.tilted_gaussian()
    ux, uy = ref.fan(beam)
    P = farfield_oracle.farfield_direct(*F, x, x, ref.WL, ref.N_GLASS, ux, uy)['P']
    rho = 1.0
    pts, uz = ref.fan_points(ux, uy, rho)
    E, H = ref.direct_sum(*F, x, x, ref.WL, ref.N_GLASS, pts)
    S_r = (ref.poynting(E, H) * (pts / rho).T).sum(axis=0).reshape(P.shape)
    want = ref.radiant_intensity(P, ux, uy)
    err = np.abs(rho ** 2 * S_r - want).max() / want.max()
    print('far limit at 1 m: %.3e of the peak' % err)
    assert err <= 1e-8


def test_fields_obey_maxwell():
    """curl E = i k Z H by central differences at (1, 2, 8) um, in the near zone (3e-6: the differences' own accuracy)"""
    F, x, _ = ref.tilted_gaussian()
    k, Z = 2 * np.pi * ref.N_GLASS / ref.WL, ref.Z0_SI / ref.N_GLASS
    r0, h = np.array([1e-6, 2e-6, 8e-6]), ref.WL / 2000
    pts = [r0] + [r0 + s * h * np.eye(3)[j] for j in range(3) for s in (1, -1)]
    E, H = ref.direct_sum(*F, x, x, ref.WL, ref.N_GLASS, np.array(pts))
    dE = [(E[:, 1 + 2 * j] - E[:, 2 + 2 * j]) / (2 * h) for j in range(3)]   # dE / dx_j
    curl = np.array([dE[1][2] - dE[2][1], dE[2][0] - dE[0][2], dE[0][1] - dE[1][0]])
    err = np.abs(curl - 1j * k * Z * H[:, 0]).max() / np.abs(k * Z * H[:, 0]).max()
    print('curl E - i k Z H: %.3e' % err)
    assert err <= 1e-4


def test_long_double_and_e_only_restatements_agree_with_fp64():
    F, x, _ = ref.tilted_gaussian(16)
    pts = np.array([[1e-6, -2e-6, 3e-6], [0.0, 0.0, 1e-3]])
    E, H = ref.direct_sum(*F, x, x, ref.WL, ref.N_GLASS, pts)
    El, Hl = ref.direct_sum(*F, x, x, ref.WL, ref.N_GLASS, pts, real=np.longdouble)
    assert El.dtype == np.clongdouble
    assert ref.max_error(E, El) < 1e-11 and ref.max_error(H, Hl) < 1e-11
    assert np.array_equal(ref.direct_sum(*F, x, x, ref.WL, ref.N_GLASS, pts, want_h=False), E)


def test_public_names_and_cabi_entries():
    import metalens_amd
    from metalens_amd import _lib, propagate
    assert metalens_amd.PlanePropagator is propagate.PlanePropagator
    assert metalens_amd.field_at_plane is propagate.field_at_plane
    for name in ('ml_propagate_plan', 'ml_propagate', 'ml_propagate_download'):
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.load(), name)


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to reach a device fails the test"""
    from metalens_amd import _lib

    def refuse(*a, **k):
        raise AssertionError('a device call was made before the arguments were checked')
    monkeypatch.setattr(_lib, 'default_context', refuse)
    monkeypatch.setattr(_lib, 'Context', refuse)


def test_argument_errors_come_before_any_device_call(no_device):
    import metalens_amd as ma
    x = (np.arange(20) - 9.5) * (ref.WL / 2.2)
    t = np.linspace(-1e-6, 1e-6, 5)
    for z in (0.0, -1e-6, float('nan')):
        with pytest.raises(ValueError, match='z > 0'):
            ma.PlanePropagator(x, x, ref.WL, ref.N_GLASS, t, t, z)
        with pytest.raises(ValueError, match='z > 0'):
            ma.field_at_plane(None, None, None, None, x, x, ref.WL, ref.N_GLASS, t, t, z)
    with pytest.raises(ValueError, match='z > 0'):
        ma.PlanePropagator(x, x, ref.WL, ref.N_GLASS, t, t, [1e-6, 2e-6, 0.0, 1e-6, 1e-6], point_list=True)
    # ragged point lists, and more than one z for a tensor grid
    with pytest.raises(ValueError, match='point list'):
        ma.PlanePropagator(x, x, ref.WL, ref.N_GLASS, t, t[:4], np.full(5, 1e-6), point_list=True)
    with pytest.raises(ValueError, match='point list'):
        ma.field_at_plane(None, None, None, None, x, x, ref.WL, ref.N_GLASS, t, t, [1e-6], point_list=True)
    with pytest.raises(ValueError, match='one plane'):
        ma.PlanePropagator(x, x, ref.WL, ref.N_GLASS, t, t, [1e-6, 2e-6])
    # the axis assertions of farfield_direct: a pitch of lambda / 2 or more, a non-uniform axis
    coarse = (np.arange(20) - 9.5) * (ref.WL / 2)
    for axes in ((coarse, x), (x, coarse), (x ** 3, x)):
        with pytest.raises(AssertionError):
            ma.PlanePropagator(*axes, ref.WL, ref.N_GLASS, t, t, 1e-6)
        with pytest.raises(AssertionError):
            ma.field_at_plane(None, None, None, None, *axes, ref.WL, ref.N_GLASS, t, t, 1e-6)


def test_no_cpu_fallback():
    """valid arguments and no device: MetalensHipError, as everywhere"""
    import ctypes

    import metalens_amd as ma
    from metalens_amd import _lib
    n = ctypes.c_int(0)
    if _lib.load().ml_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip('a GPU is visible here')
    x = (np.arange(20) - 9.5) * (ref.WL / 2.2)
    with pytest.raises(_lib.MetalensHipError):
        ma.field_at_plane(None, None, None, None, x, x, ref.WL, ref.N_GLASS, [0.0], [0.0], 1e-6)
