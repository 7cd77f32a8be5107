"""A pupil function applied to the near field resident on the GPU (csrc/fields_pupil.hip, ml_fields_pupil_plan and
ml_fields_pupil_apply).

``ApertureZones`` and ``ApertureWavefront`` measure the resident field sets and change nothing.  ``AperturePupil`` answers what
fixing it would buy: it multiplies the resident sets, where they lie, by an aperture stop, one complex factor per zone and
a Zernike phase plate, and everything downstream - the far-field transform, ``PlanePropagator``, the two analyses, a
``SourceSweep`` - sees the modified aperture.  Correct a field (measure, correct, look again), budget a lens (set a zone's
factor to 0 and see what it contributed), or stop an aperture down.  ``postprocess.pupil_factor`` and
``postprocess.apply_pupil_host`` are the NumPy twins for host arrays.
"""
import numpy as np

from . import _lib
from .postprocess import _check_pupil, apply_pupil_host, pupil_factor  # noqa: F401
from .zones import SETS_MAX, _check_sets, _resolve_sets, _upload_fields


class AperturePupil:
    """The pupil function of one aperture geometry: ``xp_list`` / ``yp_list`` are the aperture's axes (what ``build_nearfield``
    returns as ``x_pts`` / ``y_pts``), the pupil the disc of ``radius`` about ``centre``; a sample on the rim is inside.

    ``stop=True`` clears all four fields of every sample outside the disc; with ``stop=False`` such a sample keeps its field
    (times its zone factor, if it has one).  ``phase``: the coefficients, in radians, of the Zernike terms up to a radial
    order ``n_max <= 8`` in the order of ``zernike_terms(n_max)`` - 1, 3, 6, ... 45 numbers; a member is multiplied by
    ``exp(+i psi)``, ``psi = sum_j phase[j] Z_j``: the pupil ADDS the aberration, so ``phase = -wavefront`` of
    ``ApertureWavefront.analyse()`` flattens what was measured (``from_wavefront``).  ``edges`` with ``zone_factors``: 1 to 4096
    ascending radii and one complex factor per zone, zone 0 the disc inside ``edges[0]``, zone ``z`` the ring ``edges[z - 1] < r
    <= edges[z]`` - the zones of ``ApertureZones``; outside the last edge the factor is exactly 1.  How every value is formed:
    ``postprocess.pupil_factor`` and csrc/fields_pupil.h.  Every argument is checked before any device call.

    ``apply(first, n)`` multiplies the resident field sets ``first ... first + n - 1`` (all of them for ``n=None``, at most 3: a
    synthesis batch) in one launch and synchronises; ``queue(first, n)`` does the same without synchronising.  A premodulated
    synthesis is unmodulated first, as a download does.  The fields then count as supplied by the caller: no object owns
    them.  A context of a multi-rank communicator is refused."""

    def __init__(self, xp_list, yp_list, radius, *, centre=(0.0, 0.0), stop=True, phase=None, edges=None, zone_factors=None, ctx=None):
        z = _check_pupil(xp_list, yp_list, radius, centre, stop, phase, edges, zone_factors)
        self.shape = (z['x2'].size, z['y2'].size)
        self.radius, self.stop, self.n_max = z['R'], bool(z['stop']), z['n_max']
        self.n_zones = 0 if z['e2'] is None else z['e2'].size
        self._r2 = z['r2']
        self._x2, self._xi, self._y2, self._eta = (_lib.f64(z[key]) for key in ('x2', 'xi', 'y2', 'eta'))
        self._c, self._e2, self._g = (None if z[key] is None else _lib.f64(z[key]) for key in ('c', 'e2', 'g'))
        self.owner = _lib.new_owner()
        self.ctx = ctx or _lib.default_context()

    def plan(self):
        """make this pupil the context's plan (a no-op while it is)"""
        ctx = self.ctx
        if ctx.pupil_owner == self.owner:
            return
        ctx.pupil_owner = None
        _lib.check(ctx.lib.ml_fields_pupil_plan(ctx.handle, _lib.dptr(self._x2), _lib.dptr(self._xi), self.shape[0], _lib.dptr(self._y2),
                                                _lib.dptr(self._eta), self.shape[1], self._r2, int(self.stop), self.n_max,
                                                _lib.dptr(self._c), _lib.dptr(self._e2), self.n_zones, _lib.dptr(self._g)))
        ctx.pupil_owner = self.owner

    def queue(self, first=0, n=None):
        """plan if the context's plan is not this object's, then queue the launch; no synchronisation"""
        _check_sets(first, n)
        ctx = self.ctx
        self.plan()
        _lib.check(ctx.lib.ml_fields_pupil_apply(ctx.handle, int(first), _resolve_sets(ctx, first, n)))
        ctx.fields_owner = None

    def apply(self, first=0, n=None):
        self.queue(first, n)
        self.ctx.sync()

    @classmethod
    def from_wavefront(cls, aw, result, set=0, component=0, keep_piston=False, **kw):
        """the pupil that flattens what ``aw.analyse()`` measured: ``phase = -result['wavefront'][set, component]`` (``component``
        0: Ex, 1: Ey) on the pupil of the ``ApertureWavefront`` ``aw``; the piston term is left out unless ``keep_piston``.
        Further keywords (``stop``, ``edges``, ``zone_factors``, ``ctx`` - default: ``aw.ctx``) as for ``AperturePupil``."""
        w = np.asarray(result['wavefront'], dtype=float)
        if w.ndim != 3 or w.shape[2] != len(aw.terms):
            raise ValueError('result must be the dict of analyse() of this ApertureWavefront: wavefront has shape %s for %d terms'
                             % (w.shape, len(aw.terms)))
        phase = -w[set, component]
        if not keep_piston:
            phase[0] = 0.0
        if not np.isfinite(phase).all():
            raise ValueError('the wavefront of set %r, component %r is not finite: the pupil holds no field to measure' % (set, component))
        kw.setdefault('ctx', aw.ctx)
        kw.setdefault('centre', aw._centre)
        return cls(aw._x, aw._y, aw.radius, phase=phase, **kw)

    @classmethod
    def from_zones(cls, az, result, set=0, component=0, **kw):
        """the pupil that re-phases every zone ``az.analyse()`` measured: ``zone_factors = exp(-i result['phase'][set, :,
        component])`` on the edges of the ``ApertureZones`` ``az``; a zone whose phase is NaN (no samples, no field) gets the
        factor 1.  ``radius`` defaults to the last edge; further keywords as for ``AperturePupil`` (``ctx`` defaults to
        ``az.ctx``)."""
        ph = np.asarray(result['phase'], dtype=float)
        if ph.ndim != 3 or ph.shape[1] != az.n_zones:
            raise ValueError('result must be the dict of analyse() of this ApertureZones: phase has shape %s for %d zones'
                             % (ph.shape, az.n_zones))
        p = ph[set, :, component]
        g = np.where(np.isnan(p), 1.0 + 0.0j, np.exp(-1j * np.where(np.isnan(p), 0.0, p)))
        kw.setdefault('ctx', az.ctx)
        kw.setdefault('centre', az._centre)
        radius = kw.pop('radius', az._edges[-1])
        return cls(az._x, az._y, radius, edges=az._edges, zone_factors=g, **kw)

    @classmethod
    def from_zone_fields(cls, azf, result, set=0, target=0, **kw):
        """the pupil that aligns every zone's contribution at a point, as ``azf.analyse()`` measured it with the exact vector
        kernel: ``zone_factors = exp(-i result['phase'][set, :, target])`` on the edges of the ``ApertureZoneFields`` ``azf``; a
        zone whose phase is NaN (no samples) gets the factor 1.  ``radius`` defaults to the last edge; further keywords as for
        ``AperturePupil`` (``ctx`` defaults to ``azf.ctx``)."""
        ph = np.asarray(result['phase'], dtype=float)
        if ph.ndim != 3 or ph.shape[1] != azf.n_zones or ph.shape[2] != azf.points.shape[0]:
            raise ValueError('result must be the dict of analyse() of this ApertureZoneFields: phase has shape %s for %d zones and '
                             '%d points' % (ph.shape, azf.n_zones, azf.points.shape[0]))
        p = ph[set, :, target]
        g = np.where(np.isnan(p), 1.0 + 0.0j, np.exp(-1j * np.where(np.isnan(p), 0.0, p)))
        kw.setdefault('ctx', azf.ctx)
        kw.setdefault('centre', azf._centre)
        radius = kw.pop('radius', azf._edges[-1])
        return cls(azf._x, azf._y, radius, edges=azf._edges, zone_factors=g, **kw)


def apply_pupil(Ex, Ey, Hx, Hy, xp_list, yp_list, radius, **kw):
    """One-shot convenience, modelled on ``aperture_wavefront``: upload the host arrays ``Ex..Hy``, apply the pupil on the GPU
    and return the four modified arrays; with ``Ex is None`` the pupil is applied to the field sets already resident (e.g.
    after ``build_nearfield(..., download=False)``; ``first``, ``n`` choose them) and nothing is returned.  Keywords as for
    ``AperturePupil``."""
    first, n = kw.pop('first', 0), kw.pop('n', None)
    _check_sets(first, n)
    a = AperturePupil(xp_list, yp_list, radius, **kw)
    ctx = a.ctx
    if Ex is None:
        a.apply(first, n)
        return None
    _upload_fields(ctx, a.shape, Ex, Ey, Hx, Hy)
    a.apply(0, 1)
    out = [np.empty(a.shape, dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(v) for v in out]))
    return tuple(out)
