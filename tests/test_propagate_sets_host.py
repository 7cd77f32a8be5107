"""Several field sets to an image plane in one pass, without a GPU: the C-ABI entries exist, the ``image=`` argument
of ``SourceSweep.run`` / ``queue`` is checked before any device call, and nothing computes on the CPU."""
import types

import numpy as np
import pytest

import propagate_ref as ref

NEW = ('ml_propagate_sets', 'ml_propagate_download_set', 'ml_propagate_accumulate', 'ml_propagate_sums')


def test_cabi_entries_and_python_names():
    from metalens_amd import _lib, propagate, sweep
    lib = _lib.load()
    for name in NEW + ('ml_fields_sets', 'ml_nearfield_members_async'):
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    for name in ('propagate_sets', 'queue_sets', 'accumulate', 'sums'):
        assert callable(getattr(propagate.PlanePropagator, name))
    import inspect
    for f in (sweep.SourceSweep.run, sweep.SourceSweep.queue):
        assert inspect.signature(f).parameters['image'].default is None


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to reach a device fails the test"""
    from metalens_amd import _lib

    def refuse(*a, **k):
        raise AssertionError('a device call was made before the arguments were checked')
    monkeypatch.setattr(_lib, 'default_context', refuse)
    monkeypatch.setattr(_lib, 'Context', refuse)


class _NoCalls:
    """stands in for a context: every attribute access is a device call made too early"""

    def __getattr__(self, name):
        raise AssertionError('ctx.%s was touched before the arguments were checked' % name)


def _bare_sweep(ctx, nx, ny):
    """a SourceSweep that has not been through __init__ (which opens the device): what the checks read"""
    from metalens_amd.sweep import SourceSweep
    sw = object.__new__(SourceSweep)
    sw.ctx = ctx
    sw.x = (np.arange(nx) - (nx - 1) / 2) * (ref.WL / 2.2)
    sw.y = (np.arange(ny) - (ny - 1) / 2) * (ref.WL / 2.2)
    return sw


def test_image_argument_errors_come_before_any_device_call(no_device):
    ctx, other = _NoCalls(), _NoCalls()
    sw = _bare_sweep(ctx, 20, 24)
    src = [(0.0, 0.0, -1e-4, 'x')]
    elsewhere = types.SimpleNamespace(ctx=other, aperture_shape=(20, 24), want_h=True, shape=(5, 5))
    transposed = types.SimpleNamespace(ctx=ctx, aperture_shape=(24, 20), want_h=True, shape=(5, 5))
    for call in (sw.run, sw.queue):
        with pytest.raises(ValueError, match='context of this sweep'):
            call(src, image=elsewhere)
        with pytest.raises(ValueError, match='24 x 20 samples'):
            call(src, image=transposed)
        with pytest.raises(ValueError, match='context of this sweep'):   # before the sources are looked at
            call([], image=elsewhere)


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
        ma.PlanePropagator(x, x, ref.WL, ref.N_GLASS, [0.0], [0.0], 1e-6).propagate_sets()
    with pytest.raises(_lib.MetalensHipError):
        ma.SourceSweep(ref.WL, None, None, None, x, x, [0.0], [0.0]).run([(0.0, 0.0, -1e-4, 'x')], image=None)
    # the entries themselves refuse a NULL context instead of computing anything
    lib = _lib.load()
    w = np.ones(1)
    assert lib.ml_propagate_sets(None, 376.7, 0, 1) != 0
    assert lib.ml_propagate_accumulate(None, _lib.dptr(w), 1, 1) != 0
    assert lib.ml_propagate_sums(None, _lib.dptr(w), None) != 0
    assert lib.ml_propagate_download_set(None, 0, _lib.dptr(w), None) != 0
