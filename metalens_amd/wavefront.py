"""Zernike moments of the wavefront of the near field resident on the GPU (csrc/fields_wavefront.hip, ml_fields_zernike).

``ApertureZones`` gives one piston per ring - a radial profile; it cannot tell coma from astigmatism or tilt from defocus,
which is what grows when an emitter steps off axis.  Here the resident field sets are reduced against a reference wave
to the moments of the Zernike terms over a circular pupil, where they lie.  ``postprocess.wavefront_metrics`` is the NumPy
twin for host arrays.
"""
import numpy as np

from . import _lib
from .postprocess import _check_wavefront, _wavefront_dict, wavefront_record, zernike, zernike_terms  # noqa: F401
from .zones import SETS_MAX, _check_sets, _resolve_sets, _upload_fields  # noqa: F401


class ApertureWavefront:
    """The wavefront of one aperture geometry over a pupil: ``xp_list`` / ``yp_list`` are the aperture's axes (what
    ``build_nearfield`` returns as ``x_pts`` / ``y_pts``), the pupil the disc of ``radius`` about ``centre``, ``n_max`` the highest
    radial order of the Zernike terms (0 to 8; ``zernike_terms(n_max)`` lists them), ``reference`` the wave the field is
    taken against: ``('plane', ux, uy)`` or ``('focus', xf, yf, zf)``.  Membership, terms and the returned dict:
    ``postprocess.wavefront_metrics``.  Every argument is checked before any device call.

    ``analyse(first, n)`` reduces the resident field sets ``first ... first + n - 1`` (all of them for ``n=None``, at most 3: a
    synthesis batch) in one pass; membership, phase and sincos of a sample are computed once for all sets.  fp64, no
    atomics: a record is repeatable bit for bit, depends neither on the other sets of the call nor - for its terms up to an
    order - on ``n_max``.  The fields, the plans and the sums of the context are not touched; a premodulated synthesis is
    unmodulated first, as a download does.  A context of a multi-rank communicator is refused.

    ``wavefront`` in the returned dict is the small-aberration reading of the complex moments, radians per term to first
    order in the aberration: no phase is unwrapped and nothing is fitted, and on a sampled disc the terms are orthogonal
    to O(pitch / R) only."""

    def __init__(self, xp_list, yp_list, wavelength, n_glass, radius, *, n_max=4, centre=(0.0, 0.0), reference=('plane', 0.0, 0.0),
                 ctx=None):
        z = _check_wavefront(xp_list, yp_list, wavelength, n_glass, radius, n_max, centre, reference)
        self.shape = (z['x2'].size, z['y2'].size)
        self.n_max, self.terms, self.radius, self.dA = z['n_max'], z['terms'], z['R'], z['dA']
        self._mode, self._ref_c, self._k, self._r2 = z['mode'], z['ref_c'], z['k'], z['r2']
        self._x2, self._xi, self._y2, self._eta, self._ra, self._rb = (_lib.f64(z[key]) for key in ('x2', 'xi', 'y2', 'eta', 'ra', 'rb'))
        # the pupil as given: what AperturePupil.from_wavefront builds the correcting pupil on
        self._x, self._y, self._centre = np.array(xp_list, dtype=float), np.array(yp_list, dtype=float), (float(centre[0]), float(centre[1]))
        self.ctx = ctx or _lib.default_context()

    def records(self, first=0, n=None):
        """the records of ml_fields_zernike as they come, shape ``(n, 4 + 4 J)`` (csrc/fields_wavefront.h WF_*)"""
        _check_sets(first, n)
        ctx = self.ctx
        n = _resolve_sets(ctx, first, n)
        doubles = wavefront_record(self.n_max)
        rec = np.zeros((n, doubles))
        _lib.check(ctx.lib.ml_fields_zernike(ctx.handle, int(first), n, _lib.dptr(self._x2), _lib.dptr(self._xi), self.shape[0],
                                             _lib.dptr(self._y2), _lib.dptr(self._eta), self.shape[1], self._r2, self.n_max, self._mode,
                                             _lib.dptr(self._ra), _lib.dptr(self._rb), self._ref_c, self._k, _lib.dptr(rec), doubles))
        return rec

    def analyse(self, first=0, n=None):
        return _wavefront_dict(self.records(first, n), self.dA, self.shape[0] * self.shape[1], self.radius, self.n_max)


def aperture_wavefront(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, radius, **kw):
    """One-shot convenience, modelled on ``aperture_zones``: the wavefront of host arrays ``Ex..Hy`` (or of the field sets
    already resident on the GPU if ``Ex is None``, e.g. after ``build_nearfield(..., download=False)``).  Keywords and the
    returned dict as for ``ApertureWavefront`` and its ``analyse``."""
    first, n = kw.pop('first', 0), kw.pop('n', None)
    _check_sets(first, n)
    a = ApertureWavefront(xp_list, yp_list, wavelength, n_glass, radius, **kw)
    if Ex is not None:
        _upload_fields(a.ctx, a.shape, Ex, Ey, Hx, Hy)
    return a.analyse(first, n)
