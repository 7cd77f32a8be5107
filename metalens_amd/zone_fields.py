"""Per-zone contributions to the field at points behind the lens (csrc/fields_zone_fields.hip, ml_fields_zone_fields).

``ApertureZones`` projects every Fresnel zone of the resident near field onto a scalar reference wave; ``PlanePropagator``
carries the whole aperture to a point with the exact vector kernel.  ``ApertureZoneFields`` is what lies between: the
direct pair sum of the propagator left un-added across the zones, ``E(t) = sum_z E_z(t)`` - how much each ring adds at the
focus and with which phase, with the obliquity factors, the ``Rhat (Rhat . J)`` term, the magnetic current and Ez that the
scalar overlap leaves out.  One pass over the aperture per four points instead of one pupil and one propagation per
zone.  ``postprocess.zone_fields`` is the NumPy twin for host arrays.
"""
import numpy as np

from . import _lib, constants
from .postprocess import ZONE_FIELDS_TG, _check_zone_fields, _zone_fields_dict, _zone_fields_polarisation  # noqa: F401
from .zones import _check_sets, _resolve_sets, _upload_fields


class ApertureZoneFields:
    """The zones of one aperture geometry and the points their contributions are wanted at: ``xp_list`` / ``yp_list`` are the
    aperture's axes, ascending and uniform (what ``build_nearfield`` returns as ``x_pts`` / ``y_pts``; ``pitch=(dx, dy)``: the
    steps as numbers instead of the axes' first steps, needed for an axis of one sample), ``edges`` 1 to 4096 ascending radii
    about ``centre`` (``zone_edges`` of a layout), ``points`` an array ``(T, 3)`` of 1 to 64 points ``(x, y, z)`` with ``z > 0``.
    Sample ``[i][j]`` sits at ``(xp_list[0] + i dx, yp_list[0] + j dy, 0)``, as for ``PlanePropagator``.  Membership, terms and the returned dict:
    ``postprocess.zone_fields``.  Every argument is checked before any device call.

    ``analyse(first, n)`` reduces the resident field sets ``first ... first + n - 1`` (all of them for ``n=None``, at most 3: a
    synthesis batch).  fp64, no atomics: a record is repeatable bit for bit and depends neither on the other sets, nor on the
    other edges, nor on the other points of the call, nor on ``want_h``.  The fields, the plans and the sums of the context
    are not touched; a premodulated synthesis is unmodulated first, as a download does.  A context of a multi-rank
    communicator is refused."""

    def __init__(self, xp_list, yp_list, wavelength, n_glass, edges, points, *, centre=(0.0, 0.0), want_h=True, units=None, Z0=None,
                 pitch=None, ctx=None):
        z = _check_zone_fields(xp_list, yp_list, wavelength, n_glass, edges, points, centre, pitch)
        self.Z0 = float(constants.as_units(units).Z0 if Z0 is None else Z0)
        if not (np.isfinite(self.Z0) and self.Z0 > 0):
            raise ValueError('Z0 must be finite and > 0, got %r' % (Z0,))
        self.shape = (z['x2'].size, z['y2'].size)
        self.n_zones = z['e2'].size
        self.want_h = bool(want_h)
        self.points = z['points']
        self._geometry = (z['x0'], z['y0'], z['dxp'], z['dyp'], float(wavelength), float(n_glass))
        self._x2, self._y2, self._e2 = (_lib.f64(z[key]) for key in ('x2', 'y2', 'e2'))
        self._t = [_lib.f64(np.ascontiguousarray(self.points[:, d])) for d in range(3)]
        # the zones as given: what AperturePupil.from_zone_fields builds the re-phasing pupil on
        self._x, self._y, self._centre = np.array(xp_list, dtype=float), np.array(yp_list, dtype=float), (float(centre[0]), float(centre[1]))
        self._edges = np.array(edges, dtype=float)
        self.ctx = ctx or _lib.default_context()

    def records(self, first=0, n=None, with_samples=False):
        """the records of ml_fields_zone_fields as they come, shape ``(n, K + 1, T, 12)`` (6 without H): Re, Im of Ex, Ey, Ez
        (, Hx, Hy, Hz) per field set, slot - the K zones, then the outside - and point; ``with_samples``: and the members of
        the slots, ``(K + 1,)``"""
        _check_sets(first, n)
        ctx = self.ctx
        n = _resolve_sets(ctx, first, n)
        T = self.points.shape[0]
        rec = np.zeros((n, self.n_zones + 1, T, 12 if self.want_h else 6))
        samples = np.zeros(self.n_zones + 1, dtype=np.int64)
        _lib.check(ctx.lib.ml_fields_zone_fields(
            ctx.handle, int(first), n, *self._geometry, self.Z0, _lib.dptr(self._x2), self.shape[0], _lib.dptr(self._y2), self.shape[1],
            _lib.dptr(self._e2), self.n_zones, _lib.dptr(self._t[0]), _lib.dptr(self._t[1]), _lib.dptr(self._t[2]), T, int(self.want_h),
            _lib.dptr(rec), samples.ctypes.data_as(_lib.POINTER(_lib.c_int64))))
        return (rec, samples) if with_samples else rec

    def analyse(self, first=0, n=None, polarisation=None):
        p = _zone_fields_polarisation(polarisation)
        _check_sets(first, n)
        rec, samples = self.records(first, n, with_samples=True)
        return _zone_fields_dict(rec, samples, self.want_h, p)


def aperture_zone_fields(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, edges, points, **kw):
    """One-shot convenience, modelled on ``aperture_zones``: the zone contributions of host arrays ``Ex..Hy`` (or of the field
    sets already resident on the GPU if ``Ex is None``, e.g. after ``build_nearfield(..., download=False)``).  Keywords and the
    returned dict as for ``ApertureZoneFields`` and its ``analyse``."""
    first, n, polarisation = kw.pop('first', 0), kw.pop('n', None), kw.pop('polarisation', None)
    _check_sets(first, n)
    _zone_fields_polarisation(polarisation)
    a = ApertureZoneFields(xp_list, yp_list, wavelength, n_glass, edges, points, **kw)
    if Ex is not None:
        _upload_fields(a.ctx, a.shape, Ex, Ey, Hx, Hy)
    return a.analyse(first, n, polarisation)
