"""Axis factors of separable modes on a target axis, for ``PlanePropagator.overlap`` and ``SourceSweep.run(image_modes=...)``:
the Gaussian beam and the Hermite-Gauss orders.  A mode is ``psi_ab(x, y) = mode_x[a](x) mode_y[b](y)``; every function here
returns one factor sampled on an axis ``t``, complex128, in the convention ``exp(-i omega t)`` of the propagator (a wave
travelling towards +z is ``exp(+i k z)``).  The normalisation of a factor is immaterial: the ``norm`` of ``overlap()`` divides it
out of every coupling."""
import numpy as np

HERMITE_ORDER_MAX = 16


def _k(wavelength, n):
    if not (np.isfinite(wavelength) and wavelength > 0 and np.isfinite(n) and n > 0):
        raise ValueError('wavelength and n must be finite and > 0, got %r and %r' % (wavelength, n))
    return 2 * np.pi * n / wavelength


def _waist(w0):
    if not (np.isfinite(w0) and w0 > 0):
        raise ValueError('the waist w0 must be finite and > 0, got %r' % (w0,))
    return float(w0)


def gaussian_axis(t, w0, z=0.0, centre=0.0, tilt=0.0, *, wavelength, n=1.0):
    """The axis factor of a Gaussian beam whose waist ``w0`` (the 1 / e radius of the field) lies a distance ``z`` before the
    plane, centred on ``centre`` and tilted by the angle ``tilt`` (radians, in the medium of index ``n``):

        ``exp(i k (t - c)^2 / (2 q)) exp(i k sin(tilt) t)``,  ``q = z - i k w0^2 / 2``,  ``k = 2 pi n / wavelength``

    - at ``z = 0`` and without tilt ``exp(-(t - c)^2 / w0^2)``.  The common factor ``1 / sqrt(q)`` is left out (the
    normalisation is immaterial, see the module)."""
    t = np.asarray(t, dtype=float)
    k, w0 = _k(wavelength, n), _waist(w0)
    q = z - 0.5j * k * w0 * w0
    s = t - centre
    return np.exp(1j * k * s * s / (2 * q)) * np.exp(1j * k * np.sin(tilt) * t)


def hermite_gauss_axis(order, t, w0, z=0.0, centre=0.0, *, wavelength, n=1.0):
    """The axis factor of the Hermite-Gauss mode of order ``order`` (0 ... 16) of the beam of ``gaussian_axis``:

        ``H_order(sqrt(2) (t - c) / w(z)) exp(i k (t - c)^2 / (2 q)) exp(-i order psi(z))``

    with the physicists' Hermite polynomial, ``w(z) = w0 sqrt(1 + (z / zR)^2)``, ``zR = k w0^2 / 2`` and the Gouy phase ``psi =
    atan(z / zR)`` of its order, which keeps the relative phases of the orders of one beam.  Order 0 is ``gaussian_axis``
    without tilt.  Not normalised (immaterial, see the module); orders of one beam are orthogonal on an axis that holds
    them."""
    try:
        whole = int(order)
    except (TypeError, ValueError):
        whole = None
    if whole is None or whole != order or not 0 <= whole <= HERMITE_ORDER_MAX:
        raise ValueError('the order of a Hermite-Gauss mode is an integer in [0, %d], got %r' % (HERMITE_ORDER_MAX, order))
    order = whole
    t = np.asarray(t, dtype=float)
    k, w0 = _k(wavelength, n), _waist(w0)
    zR = 0.5 * k * w0 * w0
    w = w0 * np.sqrt(1 + (z / zR) ** 2)
    s = t - centre
    c = np.zeros(order + 1)
    c[order] = 1.0
    H = np.polynomial.hermite.hermval(np.sqrt(2.0) * s / w, c)
    return H * np.exp(1j * k * s * s / (2 * (z - 1j * zR))) * np.exp(-1j * order * np.arctan2(z, zR))
