"""Per-zone power and wavefront overlap of the near field resident on the GPU (csrc/fields_zones.hip, ml_fields_zones).

The reference's lens is a stack of Fresnel zones - one grating ring each - about a hexagonal centre; which of them lose
power or sit off phase is what a designer corrects.  The reference leaves that to the eye; here the
resident field sets are reduced zone by zone where they lie.  ``postprocess.zone_metrics`` is the NumPy twin for host arrays.
"""
import numpy as np

from . import _lib
from .postprocess import ZONES_RECORD, _check_zones, _zones_dict

SETS_MAX = 3   # csrc/fields_pass.h PASS_SETS_MAX: the members of a synthesis batch


def zone_edges(lens_periphery_summary):
    """the edges of a lens layout: every ring's inner radius and the last ring's outer one - zone 0 is the lens centre,
    zone ``z`` ring ``z - 1``"""
    s = lens_periphery_summary
    return np.hstack([np.asarray(s['r_min_list'], dtype=float), np.asarray(s['r_max_list'], dtype=float)[-1]])


def _check_sets(first, n):
    if int(first) != first or first < 0:
        raise ValueError('first must be a field set index >= 0, got %r' % (first,))
    if n is not None and (int(n) != n or not 1 <= n <= SETS_MAX):
        raise ValueError('analyse() takes 1 to %d field sets per call, got n = %r' % (SETS_MAX, n))


def _resolve_sets(ctx, first, n):
    """``n``, or for ``n=None`` the resident field sets from ``first`` on (at least one: the entry names what is missing)"""
    if n is None:
        have = _lib.c_int(0)
        _lib.check(ctx.lib.ml_fields_sets(ctx.handle, _lib.byref(have)))
        n = max(have.value - int(first), 1)
    return int(n)


def _upload_fields(ctx, shape, Ex, Ey, Hx, Hy):
    """make the host arrays the one resident field set of ``ctx``; no object owns the fields then"""
    arrs = [_lib.c128(v) for v in (Ex, Ey, Hx, Hy)]
    if not all(v.shape == shape for v in arrs):
        raise ValueError('the fields have shapes %s, the axes give %s' % ([v.shape for v in arrs], shape))
    _lib.check(ctx.lib.ml_fields_upload(ctx.handle, shape[0], shape[1], *[_lib.dptr(v) for v in arrs]))
    ctx.fields_owner = None


class ApertureZones:
    """The zones of one aperture geometry: ``xp_list`` / ``yp_list`` are the aperture's axes (what ``build_nearfield`` returns
    as ``x_pts`` / ``y_pts``), ``edges`` 1 to 4096 ascending radii about ``centre`` (``zone_edges`` of a layout), ``reference``
    the wave the overlap is taken with: ``('plane', ux, uy)`` or ``('focus', xf, yf, zf)``.  Membership, terms and the
    returned dict: ``postprocess.zone_metrics``.  Every argument is checked before any device call.

    ``analyse(first, n)`` reduces the resident field sets ``first ... first + n - 1`` (all of them for ``n=None``, at most 3: a
    synthesis batch) in one pass; zone, phase and sincos of a sample are computed once for all sets.  fp64, no atomics: a
    record is repeatable bit for bit and depends neither on the other sets of the call nor on the other edges.  The fields,
    the plans and the sums of the context are not touched; a premodulated synthesis is unmodulated first, as a download
    does.  A context of a multi-rank communicator is refused."""

    def __init__(self, xp_list, yp_list, wavelength, n_glass, edges, *, centre=(0.0, 0.0), reference=('plane', 0.0, 0.0),
                 ctx=None):
        z = _check_zones(xp_list, yp_list, wavelength, n_glass, edges, centre, reference)
        self.shape = (z['x2'].size, z['y2'].size)
        self.n_zones = z['e2'].size
        self.dA = z['dA']
        self._mode, self._ref_c, self._k = z['mode'], z['ref_c'], z['k']
        self._x2, self._y2, self._e2, self._ra, self._rb = (_lib.f64(z[key]) for key in ('x2', 'y2', 'e2', 'ra', 'rb'))
        # the zones as given: what AperturePupil.from_zones builds the re-phasing pupil on
        self._x, self._y, self._centre = np.array(xp_list, dtype=float), np.array(yp_list, dtype=float), (float(centre[0]), float(centre[1]))
        self._edges = np.array(edges, dtype=float)
        self.ctx = ctx or _lib.default_context()

    def records(self, first=0, n=None):
        """the records of ml_fields_zones as they come, shape ``(n, K, 8)`` (csrc/fields_zones.h ZONES_*)"""
        _check_sets(first, n)
        ctx = self.ctx
        n = _resolve_sets(ctx, first, n)
        rec = np.zeros((n, self.n_zones, ZONES_RECORD))
        _lib.check(ctx.lib.ml_fields_zones(ctx.handle, int(first), n, _lib.dptr(self._x2), self.shape[0], _lib.dptr(self._y2),
                                           self.shape[1], _lib.dptr(self._e2), self.n_zones, self._mode, _lib.dptr(self._ra),
                                           _lib.dptr(self._rb), self._ref_c, self._k, _lib.dptr(rec), ZONES_RECORD))
        return rec

    def analyse(self, first=0, n=None):
        return _zones_dict(self.records(first, n), self.dA, self.shape[0] * self.shape[1])


def aperture_zones(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, edges, **kw):
    """One-shot convenience, modelled on ``field_at_plane``: the zones of host arrays ``Ex..Hy`` (or of the field sets
    already resident on the GPU if ``Ex is None``, e.g. after ``build_nearfield(..., download=False)``).  Keywords and the
    returned dict as for ``ApertureZones`` and its ``analyse``."""
    first, n = kw.pop('first', 0), kw.pop('n', None)
    _check_sets(first, n)
    a = ApertureZones(xp_list, yp_list, wavelength, n_glass, edges, **kw)
    if Ex is not None:
        _upload_fields(a.ctx, a.shape, Ex, Ey, Hx, Hy)
    return a.analyse(first, n)
