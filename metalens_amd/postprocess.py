"""Power bookkeeping after the far-field projection.

The reference stops at ``total_P`` (nearfield_farfield.py:74: the sum of the finite
``P * dux * duy``) and leaves the rest to the caller; its docstrings describe what callers do
with it (nearfield.py:69-73: an isotropic or Lambertian emitter is the incoherent sum of x-, y-
and z-polarised dipoles; efficiency = far-field power / ``power_passing_through_lens``).  These
are host-side reductions over an M x M map (a few hundred kilobytes): NumPy, no kernel.

``P`` is power per unit (ux, uy) in glass, NaN outside the unit circle, on the tensor grid
``ux[:, None], uy[None, :]`` (what ``farfield_from_nearfield`` and ``FarfieldTransform`` return).
"""
import numpy as np


def total_power(P, dux, duy):
    """sum of the finite ``P * dux * duy`` (nearfield_farfield.py:74)"""
    cell = np.asarray(P, dtype=float) * dux * duy
    return float(cell[np.isfinite(cell)].sum())


def _sin2(ux, uy):
    ux = np.asarray(ux, dtype=float).reshape(-1, 1)
    uy = np.asarray(uy, dtype=float).reshape(1, -1)
    return ux * ux + uy * uy


def encircled_power(P, ux, uy, dux, duy, half_angle=None, sin_max=None, center=(0.0, 0.0)):
    """Power radiated into the cone of half-angle ``half_angle`` [rad] (or direction-cosine
    radius ``sin_max``) about the direction ``center`` = (ux0, uy0): the sum of the finite
    ``P * dux * duy`` over grid points with (ux-ux0)^2 + (uy-uy0)^2 <= sin_max^2."""
    assert (half_angle is None) != (sin_max is None), 'give half_angle or sin_max'
    if sin_max is None:
        sin_max = np.sin(half_angle)
    cell = np.asarray(P, dtype=float) * dux * duy
    inside = _sin2(np.asarray(ux, dtype=float).ravel() - center[0],
                   np.asarray(uy, dtype=float).ravel() - center[1]) <= sin_max * sin_max
    return float(cell[inside & np.isfinite(cell)].sum())


def encircled_power_curve(P, ux, uy, dux, duy, sin_list, center=(0.0, 0.0)):
    """``encircled_power`` for an ascending list of cone radii, one pass over the map"""
    sin_list = np.asarray(sin_list, dtype=float)
    assert np.all(np.diff(sin_list) >= 0)
    cell = np.asarray(P, dtype=float) * dux * duy
    rho2 = _sin2(np.asarray(ux, dtype=float).ravel() - center[0],
                 np.asarray(uy, dtype=float).ravel() - center[1])
    ok = np.isfinite(cell)
    order = np.argsort(rho2[ok], kind='stable')
    cum = np.concatenate(([0.0], np.cumsum(cell[ok][order])))
    return cum[np.searchsorted(rho2[ok][order], sin_list * sin_list, side='right')]


def incoherent_sum(P_maps):
    """Far-field power map of an incoherent source: the plain sum of the maps of its mutually
    incoherent components (x, y and z dipoles of an isotropic emitter, nearfield.py:69-73;
    several wavelengths or positions).  NaN (outside the unit circle) stays NaN."""
    P_maps = [np.asarray(P, dtype=float) for P in P_maps]
    assert P_maps and all(P.shape == P_maps[0].shape for P in P_maps)
    return np.sum(P_maps, axis=0)


def efficiency(P, ux, uy, dux, duy, power_in, half_angle=None, sin_max=None, center=(0.0, 0.0)):
    """Fraction of the power that passed through the lens (``power_passing_through_lens`` of
    ``build_nearfield``, nearfield.py:474-477; summed over the sources for an incoherent sum)
    that ends up in the far field - in the whole map, or inside a cone if one is given."""
    power_in = float(np.sum(power_in))
    if half_angle is None and sin_max is None:
        out = total_power(P, dux, duy)
    else:
        out = encircled_power(P, ux, uy, dux, duy, half_angle, sin_max, center)
    return out / power_in if power_in else float('nan')


BEAM_CONES_MAX = 32     # csrc/farfield_beam.h, ML_BEAM_CONES_MAX
# the record of ml_farfield_beam (csrc/farfield_beam.h BEAM_*)
_BEAM_PEAK_P, _BEAM_PEAK_INDEX, _BEAM_FINITE, _BEAM_MOM, _BEAM_CENTRE, _BEAM_K, _BEAM_CONE = 0, 1, 2, 3, 9, 11, 12
BEAM_RECORD = _BEAM_CONE + BEAM_CONES_MAX


def _check_beam(cones, centre, of='projection'):
    """the argument checks of ``FarfieldTransform.beam``, ``SourceSweep.run(beam_cones=...)`` and ``beam_metrics``, before
    any device call -> (cones ascending as float64, the caller's order as indices into them, the centre as a float64
    pair or None for ``'peak'``)"""
    if of not in ('projection', 'sums'):
        raise ValueError("of must be 'projection' or 'sums', got %r" % (of,))
    try:
        c = np.asarray(cones, dtype=float)
    except (TypeError, ValueError):
        raise ValueError('cones must be a sequence of numbers, got %r' % (cones,)) from None
    if c.ndim != 1:
        raise ValueError('cones must be a sequence of numbers, got an array of shape %s' % (c.shape,))
    if c.size > BEAM_CONES_MAX:
        raise ValueError('beam() takes at most %d cones, got %d' % (BEAM_CONES_MAX, c.size))
    bad = ~(np.isfinite(c) & (c >= 0))
    if bad.any():
        raise ValueError('a cone is the sine of a half-angle, finite and >= 0: cones[%d] = %g' % (int(np.argmax(bad)), c[np.argmax(bad)]))
    order = np.argsort(c, kind='stable')
    back = np.empty(c.size, dtype=int)
    back[order] = np.arange(c.size)
    said = "centre must be 'peak' or one (ux0, uy0), got %r" % (centre,)
    if isinstance(centre, str):
        if centre != 'peak':
            raise ValueError(said)
        return np.ascontiguousarray(c[order]), back, None
    try:
        ce = np.asarray(centre, dtype=float)
    except (TypeError, ValueError):
        raise ValueError(said) from None
    if ce.shape != (2,):
        raise ValueError(said)
    if not np.isfinite(ce).all():
        raise ValueError('a centre must be finite, got %r' % (centre,))
    return np.ascontiguousarray(c[order]), back, np.ascontiguousarray(ce)


def _beam_dict(rec, ux, uy, pair_list, back):
    """records of ml_farfield_beam, shape ``(..., BEAM_RECORD)`` with the cones ascending -> the dict of ``beam()``, every
    entry with the records' leading axes; ``back``: the caller's order of the cones"""
    rec = np.asarray(rec, dtype=float)
    ux, uy = np.asarray(ux, dtype=float).ravel(), np.asarray(uy, dtype=float).ravel()
    flat = rec[..., _BEAM_PEAK_INDEX].astype(np.int64)
    none = flat < 0
    at = np.where(none, 0, flat)
    i, j = (at, at) if pair_list else (at // uy.size, at % uy.size)
    out = {'peak_P': rec[..., _BEAM_PEAK_P].copy()}
    out['peak_index'] = np.where(none, -1, i) if pair_list else np.stack([np.where(none, -1, i), np.where(none, -1, j)], axis=-1)
    out['peak_u'] = np.stack([np.where(none, np.nan, ux[i]), np.where(none, np.nan, uy[j])], axis=-1)
    out['finite'] = rec[..., _BEAM_FINITE].astype(np.int64)
    s, sx, sy, sxx, syy, sxy = (rec[..., _BEAM_MOM + q] for q in range(6))
    out['total_P'] = s.copy()
    out['centre_u'] = rec[..., _BEAM_CENTRE:_BEAM_CENTRE + 2].copy()
    with np.errstate(divide='ignore', invalid='ignore'):
        mx, my = np.where(s != 0, sx / s, np.nan), np.where(s != 0, sy / s, np.nan)
        out['centroid_u'] = out['centre_u'] + np.stack([mx, my], axis=-1)
        out['second_moments_u'] = np.stack([sxx / s - mx * mx, syy / s - my * my, sxy / s - mx * my], axis=-1)
    out['cone_P'] = rec[..., _BEAM_CONE:_BEAM_CONE + back.size][..., back]
    return out


def _beam_single(d, pair_list):
    """the dict of one record: plain numbers where ``_beam_dict`` left arrays of no axis, ``peak_index`` an ``(i, j)`` tuple"""
    d['peak_P'], d['total_P'], d['finite'] = float(d['peak_P']), float(d['total_P']), int(d['finite'])
    d['peak_index'] = int(d['peak_index']) if pair_list else tuple(int(v) for v in d['peak_index'])
    return d


def beam_metrics(P, ux, uy, cones=(), centre='peak', pair_list=False):
    """The beam metrics of a far-field map on the host: what ``FarfieldTransform.beam`` and ``SourceSweep.run(beam_cones=...)``
    reduce on the GPU (``ml_farfield_beam``), for an arbitrary map in NumPy.  ``P``: shape ``(len(ux), len(uy))``, or
    ``(len(ux),)`` at the directions ``(ux[d], uy[d])`` with ``pair_list``; NaN (outside the unit circle) and infinities
    are left out of every sum and of the peak.  ``cones``: up to 32 sines of half-angles in any order; ``centre``:
    ``'peak'`` (the map's own peak direction) or one ``(ux0, uy0)``.

    With ``dx = ux - cx``, ``dy = uy - cy`` and ``cell = dux duy`` (the axes' first steps, 1 for an axis of one direction,
    1 for a pair list) the terms are ``t0 = P cell`` and ``t0 dx``, ``t0 dy``, ``t0 (dx dx)``, ``t0 (dy dy)``, ``t0 (dx dy)``;
    a direction is inside cone ``c`` iff ``dx dx + dy dy <= c c``.  -> dict: ``peak_P``; ``peak_index`` (``(i, j)``, ``i`` of a
    pair list; the lowest of equals, -1 if nothing is finite) and ``peak_u``, its direction; ``finite``, the number of
    finite directions; ``total_P = sum t0``; ``centre_u``, the centre used; ``centroid_u = centre + (sum t1, sum t2) / sum
    t0`` (NaN where the sum is 0) - where the beam points; ``second_moments_u = (xx, yy, xy)``, central - ``xx + yy`` is the
    squared RMS half-width of the beam in direction cosines; ``cone_P``, the power inside each cone, in the caller's order."""
    c, back, ce = _check_beam(cones, centre)
    ux, uy = np.asarray(ux, dtype=float).ravel(), np.asarray(uy, dtype=float).ravel()
    P = np.asarray(P, dtype=float)
    want = (ux.size,) if pair_list else (ux.size, uy.size)
    if P.shape != want or (pair_list and uy.size != ux.size):
        raise ValueError('P has shape %s, the directions give %s' % (P.shape, want))
    cell = 1.0
    if not pair_list:
        cell = (ux[1] - ux[0] if ux.size > 1 else 1.0) * (uy[1] - uy[0] if uy.size > 1 else 1.0)
    ok = np.isfinite(P)
    rec = np.zeros(BEAM_RECORD)
    rec[_BEAM_PEAK_P], rec[_BEAM_PEAK_INDEX], rec[_BEAM_K] = np.nan, -1.0, c.size
    rec[_BEAM_FINITE] = int(ok.sum())
    if ok.any():
        at = int(np.argmax(np.where(ok, P, -np.inf)))           # (the first of equals)
        rec[_BEAM_PEAK_P], rec[_BEAM_PEAK_INDEX] = P.flat[at], at
        if ce is None:
            ce = np.array([ux[at] if pair_list else ux[at // uy.size], uy[at] if pair_list else uy[at % uy.size]])
    elif ce is None:
        ce = np.array([np.nan, np.nan])
    rec[_BEAM_CENTRE:_BEAM_CENTRE + 2] = ce
    if ok.any():
        dx, dy = ux - ce[0], uy - ce[1]
        if not pair_list:
            dx, dy = np.broadcast_to(dx[:, None], P.shape), np.broadcast_to(dy[None, :], P.shape)
        dx, dy, t0 = dx[ok], dy[ok], (P * cell)[ok]
        xx, yy = dx * dx, dy * dy
        for q, t in enumerate((t0, t0 * dx, t0 * dy, t0 * xx, t0 * yy, t0 * (dx * dy))):
            rec[_BEAM_MOM + q] = t.sum()
        rho2 = xx + yy
        for r in range(c.size):
            rec[_BEAM_CONE + r] = t0[rho2 <= c[r] * c[r]].sum()
    return _beam_single(_beam_dict(rec, ux, uy, pair_list, back), pair_list)


ZONES_EDGES_MAX = 4096   # csrc/fields_zones.h, ML_ZONES_EDGES_MAX
# the record of ml_fields_zones per (field set, zone) (csrc/fields_zones.h ZONES_*)
_ZONES_N, _ZONES_S, _ZONES_IX, _ZONES_IY, _ZONES_CX, _ZONES_CY = 0, 1, 2, 3, 4, 6
ZONES_RECORD = 8
ZONES_REF_PLANE, ZONES_REF_FOCUS = 0, 1


def _zones_axis(name, t):
    try:
        t = np.asarray(t, dtype=float)
    except (TypeError, ValueError):
        raise ValueError('%s must be a sequence of numbers, got %r' % (name, t)) from None
    if t.ndim != 1 or t.size < 1:
        raise ValueError('%s must be a sequence of at least one number, got an array of shape %s' % (name, t.shape))
    if not np.isfinite(t).all():
        i = int(np.argmin(np.isfinite(t)))
        raise ValueError('%s must be finite: %s[%d] = %g' % (name, name, i, t[i]))
    return t


def _check_zones(x, y, wavelength, n_glass, edges, centre=(0.0, 0.0), reference=('plane', 0.0, 0.0)):
    """the argument checks of ``ApertureZones``, ``aperture_zones`` and ``zone_metrics``, before any device call, and what the
    host forms for ml_fields_zones -> dict: ``x2 = (x - xc)**2``, ``y2``, ``e2 = edges * edges``, ``mode``, the reference's
    per-axis arrays ``ra``, ``rb`` and scalars ``ref_c``, ``k``, and ``dA``, the area of a sample (an axis of one sample
    counts 1)"""
    x, y = _zones_axis('xp_list', x), _zones_axis('yp_list', y)
    if not (np.isfinite(wavelength) and wavelength > 0 and np.isfinite(n_glass) and n_glass > 0):
        raise ValueError('wavelength and n_glass must be finite and > 0, got %r and %r' % (wavelength, n_glass))
    try:
        e = np.asarray(edges, dtype=float)
    except (TypeError, ValueError):
        raise ValueError('edges must be a sequence of numbers, got %r' % (edges,)) from None
    if e.ndim != 1:
        raise ValueError('edges must be a sequence of numbers, got an array of shape %s' % (e.shape,))
    if not 1 <= e.size <= ZONES_EDGES_MAX:
        raise ValueError('zones take 1 to %d edges, got %d' % (ZONES_EDGES_MAX, e.size))
    bad = ~(np.isfinite(e) & (e >= 0))
    if bad.any():
        raise ValueError('an edge must be finite and >= 0: edges[%d] = %g' % (int(np.argmax(bad)), e[np.argmax(bad)]))
    down = np.diff(e) < 0
    if down.any():
        z = int(np.argmax(down)) + 1
        raise ValueError('the edges must not decrease: edges[%d] = %g < edges[%d] = %g' % (z, e[z], z - 1, e[z - 1]))
    said = 'centre must be one (xc, yc), got %r' % (centre,)
    try:
        c = np.asarray(centre, dtype=float)
    except (TypeError, ValueError):
        raise ValueError(said) from None
    if c.shape != (2,):
        raise ValueError(said)
    if not np.isfinite(c).all():
        raise ValueError('a centre must be finite, got %r' % (centre,))
    said = "reference must be ('plane', ux, uy) or ('focus', xf, yf, zf), got %r" % (reference,)
    try:
        kind, r = reference[0], np.asarray(reference[1:], dtype=float)
    except (TypeError, ValueError, IndexError, KeyError):
        raise ValueError(said) from None
    if not isinstance(kind, str) or kind not in ('plane', 'focus') or r.shape != ((2,) if kind == 'plane' else (3,)):
        raise ValueError(said)
    k = 2 * np.pi * n_glass / wavelength
    if kind == 'plane':
        if not (np.isfinite(r).all() and r[0] * r[0] + r[1] * r[1] <= 1):
            raise ValueError('a plane-wave reference needs ux^2 + uy^2 <= 1, got (%g, %g)' % (r[0], r[1]))
        mode, ra, rb, ref_c = ZONES_REF_PLANE, k * (r[0] * x), k * (r[1] * y), 0.0
    else:
        if not (np.isfinite(r).all() and r[2] != 0):
            raise ValueError('a focus reference needs a finite focus (xf, yf, zf) with zf != 0, got (%g, %g, %g)' % tuple(r))
        mode, ra, rb, ref_c = ZONES_REF_FOCUS, (x - r[0]) ** 2, (y - r[1]) ** 2, float(r[2])
    x2, y2 = (x - c[0]) ** 2, (y - c[1]) ** 2
    jv = int(np.argmin(y2))
    step = np.diff(y2)
    wrong = np.concatenate((step[:jv] > 0, step[jv:] < 0))
    if wrong.any():
        j = int(np.argmax(wrong)) + 1
        raise ValueError('yp_list must be in ascending or descending order - (y - yc)^2 has to fall to one minimum and rise '
                         'again: yp_list[%d] = %.17g follows yp_list[%d] = %.17g' % (j, y[j], j - 1, y[j - 1]))
    dA = (abs(x[1] - x[0]) if x.size > 1 else 1.0) * (abs(y[1] - y[0]) if y.size > 1 else 1.0)
    return dict(x2=x2, y2=y2, e2=e * e, mode=mode, ra=ra, rb=rb, ref_c=ref_c, k=float(k), dA=float(dA))


def _zones_dict(rec, dA, total):
    """records of ml_fields_zones, shape ``(sets, K, ZONES_RECORD)`` -> the dict of ``ApertureZones.analyse``; ``total``: the
    samples of the aperture"""
    rec = np.asarray(rec, dtype=float)
    n = rec[0, :, _ZONES_N]
    out = {'samples': n.astype(np.int64)}
    out['area'] = n * dA
    out['P'] = rec[:, :, _ZONES_S] * dA
    raw_I = rec[:, :, _ZONES_IX:_ZONES_IY + 1]
    raw_C = np.stack([rec[:, :, _ZONES_CX] + 1j * rec[:, :, _ZONES_CX + 1], rec[:, :, _ZONES_CY] + 1j * rec[:, :, _ZONES_CY + 1]], axis=-1)
    out['I'] = raw_I * dA
    out['overlap'] = raw_C * dA
    out['phase'] = np.angle(out['overlap'])
    den = n[None, :, None] * raw_I
    with np.errstate(divide='ignore', invalid='ignore'):
        out['coherence'] = np.where(den != 0, (raw_C.real ** 2 + raw_C.imag ** 2) / den, np.nan)
    out['outside'] = int(total - out['samples'].sum())
    return out


def _zones_phase(z):
    """the reference phase on the grid from the arrays of ``_check_zones``, every operation rounded on its own"""
    u = z['ra'][:, None] + z['rb'][None, :]
    if z['mode'] == ZONES_REF_PLANE:
        return u
    return -np.sign(z['ref_c']) * (z['k'] * np.sqrt(u + z['ref_c'] * z['ref_c']))


def zone_metrics(Ex, Ey, Hx, Hy, x, y, wavelength, n_glass, edges, centre=(0.0, 0.0), reference=('plane', 0.0, 0.0)):
    """Per-zone power and wavefront overlap of a near field on the host: what ``ApertureZones.analyse`` reduces on the GPU
    (``ml_fields_zones``), for host arrays in NumPy.  ``Ex, Ey, Hx, Hy``: complex, shape ``(len(x), len(y))`` or
    ``(sets, len(x), len(y))``; ``edges``: 1 to 4096 radii, ascending; ``centre = (xc, yc)``; ``reference``: ``('plane', ux,
    uy)``, the wave ``exp(i k (ux x + uy y))``, or ``('focus', xf, yf, zf)``, the spherical wave that converges on the point
    ``zf > 0`` behind the aperture (diverges from one in front of it for ``zf < 0``), ``k = 2 pi n_glass / wavelength``.

    Sample ``(i, j)`` has ``r2 = (x[i] - xc)**2 + (y[j] - yc)**2`` and lies in zone ``searchsorted(edges * edges, r2, 'left')``:
    zone 0 is the disc inside ``edges[0]``, zone ``z`` the ring ``edges[z - 1] < r <= edges[z]``; a sample on an edge belongs
    to the inner zone.  With ``edges = zones.zone_edges(lens_periphery_summary)`` zone 0 is the lens centre and zone ``z``
    ring ``z - 1``.  -> dict, the leading axis of every entry but ``samples``, ``area`` and ``outside`` the sets: ``samples``
    ``(K,)``; ``area = samples dx dy``; ``P = sum S dA``, ``S = Re(Ex Hy* - Ey Hx*) / 2``; ``I`` ``(sets, K, 2)``, ``sum |Ex|^2
    dA`` and ``sum |Ey|^2 dA``; ``overlap`` ``(sets, K, 2)``, ``sum E conj(w) dA`` of Ex and Ey; ``phase = angle(overlap)``, the
    piston of the zone against the reference; ``coherence = |sum E conj(w)|^2 / (n sum |E|^2)``, in [0, 1], 1 for a zone
    that follows the reference, NaN for a zone without samples or field; ``outside``, the samples in no zone."""
    z = _check_zones(x, y, wavelength, n_glass, edges, centre, reference)
    F = [np.asarray(a, dtype=np.complex128) for a in (Ex, Ey, Hx, Hy)]
    F = [a[None] if a.ndim == 2 else a for a in F]
    shape = (z['x2'].size, z['y2'].size)
    for name, a in zip(('Ex', 'Ey', 'Hx', 'Hy'), F):
        if a.ndim != 3 or a.shape[1:] != shape or a.shape[0] != F[0].shape[0]:
            raise ValueError('%s has shape %s, the axes give %s' % (name, a.shape[-2:] if a.ndim == 3 else a.shape, shape))
    K = z['e2'].size
    zone = np.searchsorted(z['e2'], z['x2'][:, None] + z['y2'][None, :], side='left')
    inside = zone < K
    zi = zone[inside]
    phi = _zones_phase(z)[inside]
    c, s = np.cos(phi), np.sin(phi)
    rec = np.zeros((F[0].shape[0], K, ZONES_RECORD))
    rec[:, :, _ZONES_N] = np.bincount(zi, minlength=K)
    for m in range(F[0].shape[0]):
        ex, ey, hx, hy = (a[m][inside] for a in F)
        terms = (0.5 * ((ex.real * hy.real + ex.imag * hy.imag) - (ey.real * hx.real + ey.imag * hx.imag)),
                 ex.real * ex.real + ex.imag * ex.imag, ey.real * ey.real + ey.imag * ey.imag,
                 ex.real * c + ex.imag * s, ex.imag * c - ex.real * s, ey.real * c + ey.imag * s, ey.imag * c - ey.real * s)
        for q, t in enumerate(terms):
            rec[m, :, 1 + q] = np.bincount(zi, weights=t, minlength=K)
    return _zones_dict(rec, z['dA'], shape[0] * shape[1])


ZONE_FIELDS_TARGETS_MAX = 64   # csrc/fields_zone_fields.h ZF_TARGETS_MAX, ML_ZONE_FIELDS_TARGETS_MAX
ZONE_FIELDS_TG = 4             # csrc/fields_zone_fields.h ZF_TG: the targets of a walk


def _zone_fields_axis(name, t, pitch):
    """one aperture axis of the zone fields: ascending and uniform (the rule of ``PlanePropagator``: within 1e-9 of the
    step) -> the step the C ABI is given: ``pitch`` where the caller names it, else the axis' first step; an axis of one
    sample has no step of its own and needs ``pitch``"""
    if pitch is not None and not (np.isfinite(pitch) and pitch > 0):
        raise ValueError('pitch=(dx, dy) must give finite steps > 0, got %r for %s' % (pitch, name))
    if t.size == 1:
        if pitch is None:
            raise ValueError('%s has one sample and no step of its own: pitch=(dx, dy) must give one > 0, got %r' % (name, pitch))
        return float(pitch)
    d = np.diff(t)
    if not (d > 0).all():
        i = int(np.argmin(d > 0)) + 1
        raise ValueError('%s must ascend: %s[%d] = %.17g follows %s[%d] = %.17g' % (name, name, i, t[i], name, i - 1, t[i - 1]))
    if d.max() - d.min() > 1e-9 * np.abs(d).max():
        raise ValueError('%s must be uniform: its steps run from %.17g to %.17g' % (name, d.min(), d.max()))
    return float(d[0]) if pitch is None else float(pitch)


def _check_zone_fields(x, y, wavelength, n_glass, edges, points, centre=(0.0, 0.0), pitch=None, polarisation=None):
    """the argument checks of ``ApertureZoneFields``, ``aperture_zone_fields`` and ``zone_fields``, before any device call
    -> the dict of ``_check_zones`` with ``points`` (T, 3), ``x0``, ``y0``, ``dxp``, ``dyp`` and ``p`` (the unit polarisation or
    None) added"""
    z = _check_zones(x, y, wavelength, n_glass, edges, centre)
    xa, ya = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    if pitch is not None:
        try:
            pitch = (float(pitch[0]), float(pitch[1]))
        except (TypeError, ValueError, IndexError):
            raise ValueError('pitch must be None or (dx, dy), got %r' % (pitch,)) from None
    z['dxp'] = _zone_fields_axis('xp_list', xa, None if pitch is None else pitch[0])
    z['dyp'] = _zone_fields_axis('yp_list', ya, None if pitch is None else pitch[1])
    z['x0'], z['y0'] = float(xa[0]), float(ya[0])
    try:
        p = np.asarray(points, dtype=float)
    except (TypeError, ValueError):
        raise ValueError('points must be an array of shape (T, 3), got %r' % (points,)) from None
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError('points must be an array of shape (T, 3), got shape %s' % (p.shape,))
    if not 1 <= p.shape[0] <= ZONE_FIELDS_TARGETS_MAX:
        raise ValueError('zone fields take 1 to %d points, got %d' % (ZONE_FIELDS_TARGETS_MAX, p.shape[0]))
    if not np.isfinite(p).all():
        t = int(np.argmax(~np.isfinite(p).all(axis=1)))
        raise ValueError('a point must be finite: points[%d] = (%g, %g, %g)' % ((t,) + tuple(p[t])))
    if not (p[:, 2] > 0).all():
        t = int(np.argmax(~(p[:, 2] > 0)))
        raise ValueError('every point needs z > 0 (the aperture is the plane z = 0): points[%d] has z = %g' % (t, p[t, 2]))
    z['points'] = p
    z['p'] = _zone_fields_polarisation(polarisation)
    return z


def _zone_fields_polarisation(polarisation):
    """``polarisation=`` -> None or the unit vector (3,) complex"""
    if polarisation is None:
        return None
    said = 'polarisation must be None or one (px, py, pz) that is finite and not zero, got %r' % (polarisation,)
    try:
        p = np.asarray(polarisation, dtype=complex)
    except (TypeError, ValueError):
        raise ValueError(said) from None
    if p.shape != (3,) or not np.isfinite(p).all() or not np.abs(p).max() > 0:
        raise ValueError(said)
    return p / np.sqrt((np.abs(p) ** 2).sum())


def _zone_fields_dict(rec, samples, want_h, p=None):
    """records of ml_fields_zone_fields, shape ``(sets, K + 1, T, 6 or 12)``, and the members ``(K + 1,)`` -> the dict of
    ``ApertureZoneFields.analyse``; ``p``: the unit polarisation (3,), or None for ``total_E / |total_E|`` per set and target"""
    rec = np.asarray(rec)
    K = rec.shape[1] - 1
    out = {'samples': np.asarray(samples[:K]).astype(np.int64), 'outside': int(samples[K])}

    def parts(c0):   # (sets, K + 1, 3, T) complex
        c = rec[..., c0:c0 + 6:2] + 1j * rec[..., c0 + 1:c0 + 6:2]
        return np.moveaxis(c, 2, 3)

    def total(F):    # the zones in ascending order, then the outside
        tot = F[:, 0].copy()
        for zz in range(1, K + 1):
            tot = tot + F[:, zz]
        return tot
    E = parts(0)
    out['E'], out['outside_E'], out['total_E'] = E[:, :K], E[:, K], total(E)
    if want_h:
        H = parts(6)
        out['H'], out['outside_H'], out['total_H'] = H[:, :K], H[:, K], total(H)
    tE = out['total_E']
    if p is None:
        norm = np.sqrt((np.abs(tE) ** 2).sum(axis=1, keepdims=True))
        with np.errstate(divide='ignore', invalid='ignore'):
            pol = np.where(norm > 0, tE / norm, 0)          # (sets, 3, T)
    else:
        pol = np.broadcast_to(np.asarray(p)[None, :, None], tE.shape)
    out['polarisation'] = pol
    out['projection'] = (np.conj(pol)[:, None] * out['E']).sum(axis=2)         # (sets, K, T)
    out['outside_projection'] = (np.conj(pol) * out['outside_E']).sum(axis=1)
    empty = (out['samples'] == 0)[None, :, None]
    out['phase'] = np.where(empty, np.nan, np.angle(out['projection']).astype(float))
    out['gradient'] = -2 * (np.conj(tE)[:, None] * out['E']).sum(axis=2).imag
    out['aligned'] = np.abs(out['projection']).sum(axis=1)                     # (sets, T)
    return out


def zone_fields(Ex, Ey, Hx, Hy, x, y, wavelength, n_glass, edges, points, centre=(0.0, 0.0), want_h=True, units=None, Z0=None,
                pitch=None, polarisation=None, real=np.float64):
    """Per-zone contributions to the field at points behind the aperture, on the host: what ``ApertureZoneFields.analyse``
    reduces on the GPU (``ml_fields_zone_fields``), for host arrays in NumPy.  ``Ex, Ey, Hx, Hy``: complex, shape ``(len(x),
    len(y))`` or ``(sets, len(x), len(y))``; ``x``, ``y``: ascending uniform axes (``pitch=(dx, dy)``: their steps as numbers, needed for an axis of one sample);
    ``edges``, ``centre``: the zones of ``zone_metrics``, the same membership; ``points`` ``(T, 3)``, ``z > 0``.

    Sample ``(i, j)`` sits at ``(x[0] + i dx, y[0] + j dy, 0)`` and adds to the zone it lies in the term of the direct
    Stratton-Chu sum of ``PlanePropagator`` (propagate.py): with ``J = (-Hy, Hx)``, ``M = (Ey, -Ex)``, ``R = r - r'``,
    ``g = exp(ikR) / (4 pi R)``, ``a = 1 + i/(kR) - 1/(kR)^2``, ``b = 1 + 3i/(kR) - 3/(kR)^2``, ``c = ik - 1/R``

        E_z(r) = dx dy sum_{zone z} g { i k Z   [a J - b Rhat (Rhat.J)] - c Rhat x M }
        H_z(r) = dx dy sum_{zone z} g { i (k/Z) [a M - b Rhat (Rhat.M)] + c Rhat x J }

    so that ``E = sum_z E_z`` over the zones and the samples outside every edge.  ``real=np.longdouble`` evaluates the sums in
    long double from the same fp64 inputs.  -> dict, the leading axis the sets: ``E`` ``(sets, K, 3, T)`` (``H`` with
    ``want_h``), ``outside_E`` ``(sets, 3, T)``, ``total_E``: the zones in ascending order, then the outside; ``samples`` ``(K,)``,
    ``outside``; with ``p`` the unit vector ``polarisation`` (default, per set and target: ``total_E / |total_E|``, returned as
    ``polarisation``) ``projection[s, z, t] = sum_d conj(p_d) E[s, z, d, t]``; ``phase = angle(projection)``, NaN for a zone
    without samples; ``gradient[s, z, t] = -2 Im(conj(total_E) . E_z)``, the derivative of ``|E(t)|^2`` with respect to a phase
    added to zone ``z``; ``aligned = sum_z |projection|`` over the K zones, what ``|p^H E|`` becomes when every zone is re-phased
    and the outside is stopped; ``outside_projection``."""
    from . import constants
    z = _check_zone_fields(x, y, wavelength, n_glass, edges, points, centre, pitch, polarisation)
    Z0 = constants.as_units(units).Z0 if Z0 is None else Z0
    F = [np.asarray(a, dtype=np.complex128) for a in (Ex, Ey, Hx, Hy)]
    F = [a[None] if a.ndim == 2 else a for a in F]
    shape = (z['x2'].size, z['y2'].size)
    for name, a in zip(('Ex', 'Ey', 'Hx', 'Hy'), F):
        if a.ndim != 3 or a.shape[1:] != shape or a.shape[0] != F[0].shape[0]:
            raise ValueError('%s has shape %s, the axes give %s' % (name, a.shape[-2:] if a.ndim == 3 else a.shape, shape))
    K, T, sets = z['e2'].size, z['points'].shape[0], F[0].shape[0]
    zi = np.searchsorted(z['e2'], z['x2'][:, None] + z['y2'][None, :], side='left').ravel()
    counts = np.bincount(zi, minlength=K + 1)
    order = np.argsort(zi, kind='stable')
    held = counts > 0
    starts = np.searchsorted(zi[order], np.arange(K + 1), side='left')[held]
    cplx = np.complex128 if real is np.float64 else np.clongdouble

    def by_zone(term):   # the sum of a term over the samples of every slot
        out = np.zeros(K + 1, dtype=cplx)
        out[held] = np.add.reduceat(term.ravel()[order], starts)
        return out

    k, Z = real(2 * np.pi * n_glass / wavelength), real(Z0 / n_glass)
    pi = 4 * np.arctan(real(1))
    dxp, dyp = real(z['dxp']), real(z['dyp'])
    X, Y = np.meshgrid(real(z['x0']) + np.arange(shape[0]).astype(real) * dxp, real(z['y0']) + np.arange(shape[1]).astype(real) * dyp,
                       indexing='ij')
    i = cplx(1j)
    nq = 12 if want_h else 6
    rec = np.zeros((sets, K + 1, T, nq), dtype=real)

    def dyad(a, b, ux, uy, uz, Vx, Vy):      # a V - b Rhat (Rhat . V), V tangential
        dot = ux * Vx + uy * Vy
        return a * Vx - b * ux * dot, a * Vy - b * uy * dot, -b * uz * dot

    def cross(ux, uy, uz, Vx, Vy):           # Rhat x V
        return -uz * Vy, uz * Vx, ux * Vy - uy * Vx

    for m in range(sets):
        ex, ey, hx, hy = (a[m].astype(cplx) for a in F)
        Jx, Jy, Mx, My = -hy, hx, ey, -ex
        for t, (px, py, pz) in enumerate(z['points']):
            Rx, Ry, Rz = real(px) - X, real(py) - Y, real(pz)
            R = np.sqrt(Rx ** 2 + Ry ** 2 + Rz ** 2)
            ux, uy, uz = Rx / R, Ry / R, Rz / R
            kr = k * R
            g = np.exp(i * kr) / (4 * pi * R)
            a = 1 + i / kr - 1 / kr ** 2
            b = 1 + 3 * i / kr - 3 / kr ** 2
            c = i * k - 1 / R
            dJ, cM = dyad(a, b, ux, uy, uz, Jx, Jy), cross(ux, uy, uz, Mx, My)
            for d in range(3):
                v = by_zone(g * (i * k * Z * dJ[d] - c * cM[d])) * dxp * dyp
                rec[m, :, t, 2 * d], rec[m, :, t, 2 * d + 1] = v.real, v.imag
            if want_h:
                dM, cJ = dyad(a, b, ux, uy, uz, Mx, My), cross(ux, uy, uz, Jx, Jy)
                for d in range(3):
                    v = by_zone(g * (i * (k / Z) * dM[d] + c * cJ[d])) * dxp * dyp
                    rec[m, :, t, 6 + 2 * d], rec[m, :, t, 7 + 2 * d] = v.real, v.imag
    return _zone_fields_dict(rec, counts, want_h, z['p'])


ZERNIKE_ORDER_MAX = 8   # csrc/fields_wavefront.h WF_ORDER_MAX, ML_ZERNIKE_ORDER_MAX
# the record of ml_fields_zernike per field set (csrc/fields_wavefront.h WF_*): the header sums, then four doubles per term
_WF_N, _WF_S, _WF_IX, _WF_IY, _WF_HEAD = 0, 1, 2, 3, 4


def zernike_terms(n_max):
    """the ``(J, 2)`` array of ``(n, m)`` of the Zernike terms up to radial order ``n_max`` in OSA/ANSI order, ``j = (n (n + 2) +
    m) / 2`` with ``m = -n, -n + 2, ... n``; ``m < 0`` is the sine term"""
    if isinstance(n_max, bool) or int(n_max) != n_max or not 0 <= n_max <= ZERNIKE_ORDER_MAX:
        raise ValueError('n_max must be a radial order from 0 to %d, got %r' % (ZERNIKE_ORDER_MAX, n_max))
    return np.array([(n, m) for n in range(int(n_max) + 1) for m in range(-n, n + 1, 2)], dtype=np.int64).reshape(-1, 2)


def wavefront_record(n_max):
    """the doubles of a record of ml_fields_zernike: ``4 + 4 J`` (ML_ZERNIKE_RECORD)"""
    return _WF_HEAD + 4 * len(zernike_terms(n_max))


def _zernike_coefficients(n, m):
    """the integer coefficients ``{(p, q): A}`` of ``Z_n^m / N`` as a polynomial in ``xi = rho cos(phi)``, ``eta = rho sin(phi)``,
    from the factorial formula of the radial polynomial and the binomial expansions of ``(xi^2 + eta^2)^t`` and ``(xi + i
    eta)^|m|`` in Python integers (csrc/fields_wavefront.h wf_coefficients)"""
    from math import comb, factorial
    a = abs(m)
    A = {}
    for s in range((n - a) // 2 + 1):
        t = (n - a) // 2 - s
        rad = (-1) ** s * factorial(n - s) // (factorial(s) * factorial((n + a) // 2 - s) * factorial(t))
        for i in range(t + 1):
            for k in range(1 if m < 0 else 0, a + 1, 2):
                key = (2 * i + a - k, 2 * (t - i) + k)
                A[key] = A.get(key, 0) + rad * comb(t, i) * (-1) ** (k // 2) * comb(a, k)
    return {key: v for key, v in sorted(A.items()) if v != 0}


def _zernike_norm(n, m):
    return np.sqrt(float(n + 1) if m == 0 else 2.0 * (n + 1))


def _zernike_check_term(n, m):
    if int(n) != n or int(m) != m or not 0 <= n <= ZERNIKE_ORDER_MAX or abs(m) > n or (n - m) % 2:
        raise ValueError('a Zernike term needs 0 <= n <= %d and m = -n, -n + 2, ... n, got (%r, %r)' % (ZERNIKE_ORDER_MAX, n, m))
    return int(n), int(m)


def zernike(n, m, xi, eta):
    """The Zernike term ``Z_n^m`` at the pupil coordinates ``xi = (x - xc) / R``, ``eta = (y - yc) / R`` (broadcast against
    each other), Noll-normalised: ``sqrt(n + 1) R_n^0(rho)`` for ``m = 0``, ``sqrt(2 (n + 1)) R_n^|m|(rho) cos(m phi)`` for ``m > 0``
    and ``... sin(|m| phi)`` for ``m < 0``, so that ``(1 / pi) int Z_j Z_k = delta_jk`` over the unit disc.  Evaluated as the
    polynomial in ``(xi, eta)`` the moments are formed with; a wavefront map is ``sum_j wavefront[j] zernike(n_j, m_j, xi, eta)``."""
    n, m = _zernike_check_term(n, m)
    xi, eta = np.asarray(xi, dtype=float), np.asarray(eta, dtype=float)
    out = np.zeros(np.broadcast(xi, eta).shape)
    for (p, q), A in _zernike_coefficients(n, m).items():
        out = out + float(A) * (xi ** p * eta ** q)
    return _zernike_norm(n, m) * out


def _check_wavefront(x, y, wavelength, n_glass, radius, n_max, centre=(0.0, 0.0), reference=('plane', 0.0, 0.0)):
    """the argument checks of ``ApertureWavefront``, ``aperture_wavefront`` and ``wavefront_metrics``, before any device call:
    those of ``_check_zones`` with the pupil's radius as the single edge, and what the host forms for ml_fields_zernike
    beside: ``r2 = R R``, ``xi = (x - xc) / R``, ``eta = (y - yc) / R``, ``terms``"""
    try:
        R = float(radius)
    except (TypeError, ValueError):
        raise ValueError('radius must be one number, got %r' % (radius,)) from None
    if not (np.isfinite(R) and R > 0):
        raise ValueError('the radius of the pupil must be finite and > 0, got %r' % (radius,))
    terms = zernike_terms(n_max)
    z = _check_zones(x, y, wavelength, n_glass, [R], centre, reference)
    x, y, c = np.asarray(x, dtype=float), np.asarray(y, dtype=float), np.asarray(centre, dtype=float)
    z.update(R=R, r2=float(z.pop('e2')[0]), xi=(x - c[0]) / R, eta=(y - c[1]) / R, n_max=int(n_max), terms=terms)
    return z


def _wavefront_convert(head, M, n_max):
    """header sums ``(sets, 4)`` and monomial moments ``M[p][q]`` -> ``(sets, 4)`` -> the records of ml_fields_zernike: per term
    ``A M`` over the non-zero coefficients in ascending (p, then q) order onto +0.0, then one multiplication by ``N_j``"""
    terms = zernike_terms(n_max)
    rec = np.zeros((head.shape[0], _WF_HEAD + 4 * len(terms)))
    rec[:, :_WF_HEAD] = head
    for j, (n, m) in enumerate(terms):
        acc = np.zeros((head.shape[0], 4))
        for (p, q), A in _zernike_coefficients(int(n), int(m)).items():
            acc = acc + float(A) * M[p][q]
        rec[:, _WF_HEAD + 4 * j:_WF_HEAD + 4 * j + 4] = _zernike_norm(int(n), int(m)) * acc
    return rec


def _wavefront_dict(rec, dA, total, R, n_max):
    """records of ml_fields_zernike, shape ``(sets, 4 + 4 J)`` -> the dict of ``ApertureWavefront.analyse``; ``total``: the samples
    of the aperture"""
    rec = np.asarray(rec, dtype=float)
    terms = zernike_terms(n_max)
    n = rec[0, _WF_N]
    out = {'terms': terms, 'samples': np.int64(n), 'area': n * dA, 'outside': int(total - n)}
    out['P'] = rec[:, _WF_S] * dA
    raw_I = rec[:, _WF_IX:_WF_IY + 1]
    out['I'] = raw_I * dA
    t = rec[:, _WF_HEAD:].reshape(rec.shape[0], len(terms), 4)
    raw = np.stack([t[:, :, 0] + 1j * t[:, :, 1], t[:, :, 2] + 1j * t[:, :, 3]], axis=1)      # (sets, 2, J)
    out['moments'] = raw * dA / (np.pi * R * R)
    out['piston'] = np.angle(out['moments'][..., 0])
    den = n * raw_I
    c0 = raw[..., 0]
    with np.errstate(divide='ignore', invalid='ignore'):
        out['coherence'] = np.where(den != 0, (c0.real ** 2 + c0.imag ** 2) / den, np.nan)
        w = np.where(c0[..., None] != 0, (out['moments'] / out['moments'][..., :1]).imag, np.nan)
    out['wavefront'] = w
    out['rms'] = np.sqrt((w[..., 1:] ** 2).sum(axis=-1))
    return out


def wavefront_metrics(Ex, Ey, Hx, Hy, x, y, wavelength, n_glass, radius, n_max=4, centre=(0.0, 0.0), reference=('plane', 0.0, 0.0)):
    """Zernike moments of a near field's wavefront on the host: what ``ApertureWavefront.analyse`` reduces on the GPU
    (``ml_fields_zernike``), for host arrays in NumPy, by the same separable route with every operation rounded on its own.
    ``Ex, Ey, Hx, Hy``: complex, shape ``(len(x), len(y))`` or ``(sets, len(x), len(y))``; the pupil is the disc of ``radius``
    about ``centre = (xc, yc)``: sample ``(i, j)`` is a member iff ``(x[i] - xc)**2 + (y[j] - yc)**2 <= radius * radius``, a sample
    on the rim is inside; ``reference`` as for ``zone_metrics``; ``n_max``: the highest radial order, 0 to 8.

    With ``C = E conj(w)`` of a member, ``xi = (x - xc) / R`` and ``eta = (y - yc) / R``, the moments of the Noll-normalised
    terms ``Z_j`` (``zernike_terms``, ``zernike``) come from the monomial moments ``sum_i xi^p sum_j C eta^q`` and the terms'
    integer coefficients.  -> dict, the leading axis of every entry but ``terms``, ``samples``, ``area`` and ``outside`` the
    sets: ``terms`` ``(J, 2)``, the ``(n, m)``; ``samples``, the members; ``area = samples dx dy``; ``outside``; ``P = sum S dA``;
    ``I`` ``(sets, 2)``, ``sum |Ex|^2 dA`` and ``sum |Ey|^2 dA``; ``moments`` ``(sets, 2, J)`` complex, ``sum C Z_j dA / (pi R^2)`` of Ex
    and Ey; ``piston = angle(moments[..., 0])``; ``coherence = |sum C|^2 / (n sum |E|^2)``, in [0, 1], the Strehl ratio of the
    wavefront against the reference, NaN where ``n sum |E|^2`` is 0; ``wavefront = Im(moments / moments[..., :1])``, radians
    per term, NaN where the piston moment is 0; ``rms = sqrt(sum_{j >= 1} wavefront^2)``.

    ``wavefront`` is the small-aberration reading of the complex moments: for a field ``exp(i W)`` with ``W = sum a_j Z_j``
    small it returns ``a_j`` to first order in ``W``.  There is no phase unwrapping and no least-squares fit; and on a
    sampled disc the terms are orthogonal only to O(pitch / R), so a term leaks into the others at that level."""
    z = _check_wavefront(x, y, wavelength, n_glass, radius, n_max, centre, reference)
    F = [np.asarray(a, dtype=np.complex128) for a in (Ex, Ey, Hx, Hy)]
    F = [a[None] if a.ndim == 2 else a for a in F]
    shape = (z['x2'].size, z['y2'].size)
    for name, a in zip(('Ex', 'Ey', 'Hx', 'Hy'), F):
        if a.ndim != 3 or a.shape[1:] != shape or a.shape[0] != F[0].shape[0]:
            raise ValueError('%s has shape %s, the axes give %s' % (name, a.shape[-2:] if a.ndim == 3 else a.shape, shape))
    sets, n_max = F[0].shape[0], z['n_max']
    member = z['x2'][:, None] + z['y2'][None, :] <= z['r2']
    phi = np.where(member, _zones_phase(z), 0.0)
    c, s = np.cos(phi), np.sin(phi)
    held = member.any(axis=1)                                   # the lines that hold members
    xi = np.where(held, z['xi'], 0.0)
    head, T = np.zeros((sets, 4)), np.zeros((sets, 4, shape[0], n_max + 1))
    head[:, _WF_N] = member.sum()
    for m in range(sets):
        ex, ey, hx, hy = (np.where(member, a[m], 0.0) for a in F)
        head[m, _WF_S] = (0.5 * ((ex.real * hy.real + ex.imag * hy.imag) - (ey.real * hx.real + ey.imag * hx.imag))).sum()
        head[m, _WF_IX] = (ex.real * ex.real + ex.imag * ex.imag).sum()
        head[m, _WF_IY] = (ey.real * ey.real + ey.imag * ey.imag).sum()
        C = (ex.real * c + ex.imag * s, ex.imag * c - ex.real * s, ey.real * c + ey.imag * s, ey.imag * c - ey.real * s)
        e = np.where(member, 1.0, 0.0)                          # eta^q by repeated multiplication
        for q in range(n_max + 1):
            for comp in range(4):
                T[m, comp, :, q] = (C[comp] * e).sum(axis=1)
            e = e * np.where(member, z['eta'][None, :], 0.0)
    M = [[None] * (n_max + 1) for _ in range(n_max + 1)]
    pw = np.ones(shape[0])                                      # xi^p by repeated multiplication
    for p in range(n_max + 1):
        for q in range(n_max + 1 - p):
            M[p][q] = (pw[None, None, :] * T[:, :, :, q]).sum(axis=2)
        pw = pw * xi
    return _wavefront_dict(_wavefront_convert(head, M, n_max), z['dA'], shape[0] * shape[1], z['R'], n_max)


PUPIL_NQ = ZERNIKE_ORDER_MAX + 1   # csrc/fields_pupil.h PUPIL_NQ: the entries of a line of the table
PUPIL_PHASE_LIMIT = 1e9            # csrc/fields_pass.h PASS_PHASE_LIMIT


def _check_pupil(x, y, radius, centre=(0.0, 0.0), stop=True, phase=None, edges=None, zone_factors=None):
    """the argument checks of ``AperturePupil``, ``apply_pupil``, ``pupil_factor`` and ``apply_pupil_host``, before any device call,
    and what the host forms for ml_fields_pupil_plan -> dict: ``x2``, ``y2``, ``xi``, ``eta``, ``r2``, ``R`` as ``_check_wavefront``
    forms them, ``stop`` (0 or 1), ``n_max`` and ``c`` (the phase coefficients, or None), ``e2`` and ``g`` (the squared edges and
    the factors as ``(K, 2)`` doubles, or None)"""
    try:
        R = float(radius)
    except (TypeError, ValueError):
        raise ValueError('radius must be one number, got %r' % (radius,)) from None
    if not (np.isfinite(R) and R > 0):
        raise ValueError('the radius of the pupil must be finite and > 0, got %r' % (radius,))
    if not isinstance(stop, (bool, np.bool_)):
        raise ValueError('stop must be True or False, got %r' % (stop,))
    n_max, c = 0, None
    if phase is not None:
        try:
            c = np.array(phase, dtype=float)
        except (TypeError, ValueError):
            raise ValueError('phase must be a sequence of Zernike coefficients in radians, got %r' % (phase,)) from None
        orders = {(n + 1) * (n + 2) // 2: n for n in range(ZERNIKE_ORDER_MAX + 1)}
        if c.ndim != 1 or c.size not in orders:
            raise ValueError('phase must hold the (n_max + 1)(n_max + 2) / 2 coefficients of the terms up to a radial order n_max <= %d '
                             '(zernike_terms): 1, 3, 6, ... 45 numbers, got an array of shape %s' % (ZERNIKE_ORDER_MAX, c.shape))
        if not np.isfinite(c).all():
            j = int(np.argmin(np.isfinite(c)))
            raise ValueError('a phase coefficient must be finite: phase[%d] = %g' % (j, c[j]))
        n_max = orders[c.size]
    if (edges is None) != (zone_factors is None):
        raise ValueError('edges and zone_factors go together: one factor per zone, got edges=%s and zone_factors=%s'
                         % ('None' if edges is None else 'given', 'None' if zone_factors is None else 'given'))
    e = [R] if edges is None else edges
    z = _check_zones(x, y, 1.0, 1.0, e, centre)
    g = None
    if zone_factors is not None:
        try:
            gz = np.array(zone_factors, dtype=complex)
        except (TypeError, ValueError):
            raise ValueError('zone_factors must be a sequence of complex numbers, got %r' % (zone_factors,)) from None
        if gz.shape != z['e2'].shape:
            raise ValueError('zone_factors must hold one factor per edge: got shape %s for %d edges' % (gz.shape, z['e2'].size))
        if not (np.isfinite(gz.real) & np.isfinite(gz.imag)).all():
            k = int(np.argmin(np.isfinite(gz.real) & np.isfinite(gz.imag)))
            raise ValueError('a zone factor must be finite: zone_factors[%d] = %r' % (k, complex(gz[k])))
        g = np.ascontiguousarray(np.stack([gz.real, gz.imag], axis=-1))
    x, y, ce = np.asarray(x, dtype=float), np.asarray(y, dtype=float), np.asarray(centre, dtype=float)
    out = dict(x2=z['x2'], y2=z['y2'], xi=(x - ce[0]) / R, eta=(y - ce[1]) / R, R=R, r2=R * R, stop=int(bool(stop)), n_max=n_max, c=c,
               e2=z['e2'] if edges is not None else None, g=g)
    if c is not None:
        reach = float(np.abs(_pupil_monomials(n_max, c)).sum())
        if not reach <= PUPIL_PHASE_LIMIT:
            raise ValueError('the phase plate can reach %.6g rad on the unit disc: the phase arithmetic covers up to %g'
                             % (reach, PUPIL_PHASE_LIMIT))
    return out


def _pupil_monomials(n_max, c):
    """``B[p, q] = sum_j (c_j N_j) A_j,pq`` over the terms whose coefficient is not 0, ``j`` ascending, onto +0.0: the phase plate
    as a polynomial in ``(xi, eta)``, shape ``(9, 9)`` (csrc/fields_pupil.h pupil_monomials)"""
    B = np.zeros((PUPIL_NQ, PUPIL_NQ))
    for j, (n, m) in enumerate(zernike_terms(n_max)):
        cn = float(c[j]) * _zernike_norm(int(n), int(m))
        for (p, q), A in _zernike_coefficients(int(n), int(m)).items():
            B[p, q] = B[p, q] + cn * float(A)
    return B


def _pupil_line_table(n_max, B, xi):
    """``b[i, q] = sum_p B[p, q] xi[i]^p`` by Horner, ``p`` descending from ``n_max - q``; +0.0 beyond ``n_max`` (csrc/fields_pupil.h
    pupil_line_table)"""
    table = np.zeros((xi.size, PUPIL_NQ))
    for q in range(n_max + 1):
        b = np.full(xi.size, B[n_max - q, q])
        for p in range(n_max - q - 1, -1, -1):
            b = b * xi + B[p, q]
        table[:, q] = b
    return table


def _pupil_parts(z):
    """-> ``member``, ``zero`` (the stopped non-members), ``touch`` (the samples multiplied by a factor) and the factor's parts
    ``fr``, ``fi``, each of shape ``(nx, ny)``, by the route of csrc/fields_pupil.h, every operation rounded on its own"""
    r2 = z['x2'][:, None] + z['y2'][None, :]
    member = r2 <= z['r2']
    zero = ~member & bool(z['stop'])
    gr, gi = np.ones(r2.shape), np.zeros(r2.shape)
    factor = np.zeros(r2.shape, dtype=bool)
    if z['e2'] is not None:
        K = z['e2'].size
        zone = np.searchsorted(z['e2'], r2, side='left')
        factor = (zone < K) & ~zero
        at = np.minimum(zone, K - 1)
        gr, gi = np.where(factor, z['g'][at, 0], 1.0), np.where(factor, z['g'][at, 1], 0.0)
    phased = member & (z['c'] is not None)
    fr, fi = gr, gi
    if z['c'] is not None:
        n_max = z['n_max']
        table = _pupil_line_table(n_max, _pupil_monomials(n_max, z['c']), z['xi'])
        eta = np.where(member, z['eta'][None, :], 0.0)
        psi = np.repeat(table[:, PUPIL_NQ - 1:], z['y2'].size, axis=1)
        for q in range(PUPIL_NQ - 2, -1, -1):
            psi = psi * eta + table[:, q:q + 1]
        cs, sn = np.cos(psi), np.sin(psi)
        fr = np.where(phased, gr * cs - gi * sn, gr)
        fi = np.where(phased, gr * sn + gi * cs, gi)
    return member, zero, ~zero & (factor | phased), fr, fi


def pupil_factor(x, y, radius, centre=(0.0, 0.0), stop=True, phase=None, edges=None, zone_factors=None):
    """The pupil function of ``AperturePupil`` on the host, by the same route with every operation rounded on its own
    (csrc/fields_pupil.h): -> ``(member, f)``, each of shape ``(len(x), len(y))``.  ``member``: ``(x - xc)^2 + (y - yc)^2 <= radius^2``,
    a sample on the rim is inside.  ``f``: the complex factor of every sample - ``g[zone] exp(+i psi)`` on a member, with
    ``psi = sum_j phase[j] Z_j(xi, eta)`` (``zernike_terms`` gives the order) and ``g[zone] = zone_factors[searchsorted(edges^2,
    r^2, 'left')]``, exactly 1 outside every edge and without edges; on a non-member 0 with ``stop`` and its zone factor alone
    without."""
    z = _check_pupil(x, y, radius, centre, stop, phase, edges, zone_factors)
    member, zero, _touch, fr, fi = _pupil_parts(z)
    f = np.empty(member.shape, dtype=np.complex128)
    f.real, f.imag = np.where(zero, 0.0, fr), np.where(zero, 0.0, fi)
    return member, f


def apply_pupil_host(Ex, Ey, Hx, Hy, x, y, radius, centre=(0.0, 0.0), stop=True, phase=None, edges=None, zone_factors=None):
    """What ``AperturePupil.apply`` does to the resident field sets, for host arrays in NumPy: ``Ex, Ey, Hx, Hy`` of shape
    ``(len(x), len(y))`` or ``(sets, len(x), len(y))`` -> the four arrays multiplied by ``pupil_factor`` - ``(E.r f.r - E.i f.i) + i
    (E.r f.i + E.i f.r)`` -, stopped non-members +0.0, and every sample whose factor is exactly 1 (no phase applies to it and
    no zone factor is given for it) with the bytes it had."""
    z = _check_pupil(x, y, radius, centre, stop, phase, edges, zone_factors)
    F = [np.asarray(a, dtype=np.complex128) for a in (Ex, Ey, Hx, Hy)]
    shape = (z['x2'].size, z['y2'].size)
    for name, a in zip(('Ex', 'Ey', 'Hx', 'Hy'), F):
        if a.ndim not in (2, 3) or a.shape[-2:] != shape or a.shape != F[0].shape:
            raise ValueError('%s has shape %s, the axes give %s' % (name, a.shape[-2:] if a.ndim == 3 else a.shape, shape))
    _member, zero, touch, fr, fi = _pupil_parts(z)
    out = []
    for a in F:
        r = a.copy()
        prod_r, prod_i = a.real * fr - a.imag * fi, a.real * fi + a.imag * fr
        r.real = np.where(touch, prod_r, np.where(zero, 0.0, a.real))
        r.imag = np.where(touch, prod_i, np.where(zero, 0.0, a.imag))
        out.append(r)
    return tuple(out)


# ---- overlaps of an image with separable modes: the NumPy twin of PlanePropagator.overlap ---------------------------
def mode_norm(mode_x, mode_y, dx, dy):
    """-> ``(sum_i |mode_x[a, i]|^2 dx) (sum_j |mode_y[b, j]|^2 dy)``, shape ``(nu, nv)``: the integral of ``|psi_ab|^2`` over the
    patch"""
    mode_x, mode_y = np.atleast_2d(mode_x), np.atleast_2d(mode_y)
    return ((np.abs(mode_x) ** 2).sum(axis=1) * dx)[:, None] * ((np.abs(mode_y) ** 2).sum(axis=1) * dy)[None, :]


def mode_coupling(overlaps, norm, Z, power=None, I_dA=None):
    """The power coupled into the x- and the y-polarised mode ``psi_ab`` over a reference power: the one place where
    ``PlanePropagator.overlap``, ``SourceSweep.run(image_modes=...)`` and ``mode_overlaps`` form it.

    ``overlaps``: ``{'Ex', 'Ey'}`` or ``{'Ex', 'Ey', 'Hx', 'Hy'}``, complex ``(..., nu, nv)``, ``sum conj(psi_ab) F dx dy``;
    ``norm`` ``(nu, nv)``; ``Z = Z0 / n_glass``; ``power`` and ``I_dA``: arrays of the leading shape ``(...)``.  The mode is
    paraxial, ``h = z^ x e / Z``, and carries ``norm / (2 Z)``.  With H: ``|O_Ex / Z + O_Hy|^2 Z / (8 norm power)`` and ``|O_Ey /
    Z - O_Hx|^2 Z / (8 norm power)``.  Without H: ``|O_Ex|^2 / (2 Z norm power)`` with a power, ``|O_Ex|^2 / (norm I_dA)``
    without one.  NaN where ``norm`` or the reference is 0.  -> ``(coupling_x, coupling_y)``"""
    if 'Hx' in overlaps:
        if power is None:
            raise ValueError('mode_coupling with H needs a power')
        ax, ay = overlaps['Ex'] / Z + overlaps['Hy'], overlaps['Ey'] / Z - overlaps['Hx']
        scale, ref = Z / 8.0, power
    else:
        ax, ay = overlaps['Ex'], overlaps['Ey']
        if power is None:
            if I_dA is None:
                raise ValueError('mode_coupling without H needs a power or I_dA')
            scale, ref = 1.0, I_dA
        else:
            scale, ref = 1.0 / (2.0 * Z), power
    den = norm * np.asarray(ref, dtype=float)[..., None, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        return tuple(np.where(den != 0, (a.real * a.real + a.imag * a.imag) * scale / den, np.nan) for a in (ax, ay))


def mode_overlaps(fields, x, y, mode_x, mode_y, Z, power=None):
    """The dict of ``PlanePropagator.overlap`` from a DOWNLOADED result dict (``propagate()``, ``propagate_sets()``): ``Ex``,
    ``Ey`` and, for the forms with H, ``Hx``, ``Hy`` of shape ``(len(x), len(y))`` or ``(planes, len(x), len(y))`` on uniform
    axes ``x``, ``y``.  ``mode_x`` ``(nu, len(x))`` or ``(len(x),)``, ``mode_y`` likewise; ``Z = Z0 / n_glass``; ``power``: None
    (with H: ``sum Sz dx dy``; without: the Cauchy-Schwarz form over ``sum |E|^2 dx dy``), a number or ``(planes,)``."""
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    dx, dy = (x[-1] - x[0]) / (x.size - 1), (y[-1] - y[0]) / (y.size - 1)
    mode_x, mode_y = np.atleast_2d(np.asarray(mode_x, dtype=complex)), np.atleast_2d(np.asarray(mode_y, dtype=complex))
    want_h = 'Hx' in fields and 'Hy' in fields
    F = {k: np.asarray(fields[k], dtype=complex).reshape((-1, x.size, y.size)) for k in ('Ex', 'Ey', 'Hx', 'Hy')[:4 if want_h else 2]}
    # separable, as on the GPU: rows first, then columns - two matrix products per plane and component
    O = {k: np.matmul(mode_x.conj()[None], np.matmul(v, mode_y.conj().T[None])) * (dx * dy) for k, v in F.items()}
    planes = F['Ex'].shape[0]
    out = {'overlap_' + k: v for k, v in O.items()}
    out['norm'] = mode_norm(mode_x, mode_y, dx, dy)
    I_dA = None
    if power is not None:
        power = np.broadcast_to(np.asarray(power, dtype=float), (planes,)).copy()
    elif want_h:
        power = (0.5 * np.real(F['Ex'] * F['Hy'].conj() - F['Ey'] * F['Hx'].conj())).sum(axis=(1, 2)) * (dx * dy)
    else:
        E2 = sum(np.abs(np.asarray(fields[k]).reshape((-1, x.size, y.size))) ** 2 for k in ('Ex', 'Ey', 'Ez') if k in fields)
        I_dA = E2.sum(axis=(1, 2)) * (dx * dy)
    out['power'] = I_dA if power is None else power
    out['coupling_x'], out['coupling_y'] = mode_coupling(O, out['norm'], Z, power=power, I_dA=I_dA)
    return out


# ---- Stokes records of an image: the NumPy twin of PlanePropagator.stokes -------------------------------------------
def stokes_maps(Ex, Ey, Ez):
    """-> ``(S0, S1, S2, S3, Iz)`` per target, array ``(5,) + Ex.shape``: the formulas of csrc/propagate_stokes.h line by line,
    every operation rounded on its own, so that the GPU's numbers are these to the bit.  ``S3 = 2 Im(conj(Ex) Ey) = +S0`` for
    ``E`` proportional to ``x^ + i y^``: under the project's ``exp(-i omega t)``, for a wave travelling to +z, that is the field
    rotating counter-clockwise seen looking towards the source (positive helicity)."""
    Ex, Ey, Ez = (np.asarray(v, dtype=complex) for v in (Ex, Ey, Ez))
    a = Ex.real * Ex.real + Ex.imag * Ex.imag
    b = Ey.real * Ey.real + Ey.imag * Ey.imag
    Iz = Ez.real * Ez.real + Ez.imag * Ez.imag
    S0 = a + b
    S1 = a - b
    S2 = 2 * (Ex.real * Ey.real + Ex.imag * Ey.imag)
    S3 = 2 * (Ex.real * Ey.imag - Ex.imag * Ey.real)
    return np.stack([S0, S1, S2, S3, Iz])


def _stokes_state(S, Iz):
    """integrated ``S`` ``(..., 4)`` and ``Iz`` ``(...)`` -> ``(longitudinal_share, dop, orientation, ellipticity)``: the one place
    where ``PlanePropagator.stokes`` and ``stokes_metrics`` form them (NaN where the denominator is 0)"""
    S0, S1, S2, S3 = (S[..., q] for q in range(4))
    pol = np.sqrt(S1 * S1 + S2 * S2 + S3 * S3)
    with np.errstate(divide='ignore', invalid='ignore'):
        share = np.where(S0 + Iz != 0, Iz / (S0 + Iz), np.nan)
        dop = np.where(S0 != 0, pol / S0, np.nan)
        ellipticity = np.where(pol != 0, 0.5 * np.arcsin(np.clip(S3 / pol, -1.0, 1.0)), np.nan)
    return share, dop, 0.5 * np.arctan2(S2, S1), ellipticity


def stokes_metrics(fields_or_maps, x, y, radii=(), centre='peak'):
    """The dict of ``PlanePropagator.stokes`` from a DOWNLOADED result dict (``Ex``, ``Ey``, ``Ez`` of shape ``(len(x), len(y))`` or
    ``(planes, len(x), len(y))``) or from the five maps of ``stokes_maps`` / ``PlanePropagator.stokes_sums()`` (``(5, ...)``), on
    uniform axes ``x``, ``y``.  ``radii`` in any order; ``centre``: ``'peak'`` (every plane's peak of ``S0 + Iz``, the lowest index
    of equals), one ``(xc, yc)`` or ``(planes, 2)``.  Membership of a radius as on the GPU: ``(dx (i - ci))^2 + (dy (j - cj))^2
    <= R^2``."""
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    dx, dy = (x[-1] - x[0]) / (x.size - 1), (y[-1] - y[0]) / (y.size - 1)
    M = stokes_maps(*(fields_or_maps[k] for k in ('Ex', 'Ey', 'Ez'))) if isinstance(fields_or_maps, dict) else np.asarray(fields_or_maps, dtype=float)
    M = M.reshape((5, -1, x.size, y.size))
    planes = M.shape[1]
    I = M[0] + M[4]
    flat = I.reshape(planes, -1).argmax(axis=1)
    peak = np.stack([flat // y.size, flat % y.size], axis=1)
    if isinstance(centre, str):
        if centre != 'peak':
            raise ValueError("centre must be 'peak', one (xc, yc) or an array (planes, 2), got %r" % (centre,))
        c = peak.astype(float)
    else:
        c = np.broadcast_to(np.asarray(centre, dtype=float), (planes, 2))
        c = np.stack([(c[:, 0] - x[0]) / dx, (c[:, 1] - y[0]) / dy], axis=1)
    radii = np.asarray(radii, dtype=float)
    fi, fj = np.meshgrid(np.arange(x.size, dtype=float), np.arange(y.size, dtype=float), indexing='ij')
    enc = np.zeros((planes, radii.size, 5))
    for p in range(planes):
        fx = dx * (fi - c[p, 0])
        fy = dy * (fj - c[p, 1])
        r2 = fx * fx + fy * fy
        for r, R in enumerate(radii):
            enc[p, r] = M[:, p][:, r2 <= R * R].sum(axis=1)
    sums = M.sum(axis=(2, 3)).T * (dx * dy)
    enc *= dx * dy
    out = {'peak_I': I.reshape(planes, -1)[np.arange(planes), flat], 'peak_index': peak,
           'peak_xy': np.stack([x[peak[:, 0]], y[peak[:, 1]]], axis=1), 'centre_index': c.copy(),
           'centre_xy': np.stack([x[0] + dx * c[:, 0], y[0] + dy * c[:, 1]], axis=1), 'S': sums[:, :4], 'Iz_dA': sums[:, 4]}
    out['longitudinal_share'], out['dop'], out['orientation'], out['ellipticity'] = _stokes_state(out['S'], out['Iz_dA'])
    out['encircled_S'], out['encircled_Iz'] = enc[:, :, :4], enc[:, :, 4]
    out['encircled_dop'] = _stokes_state(out['encircled_S'], out['encircled_Iz'])[1]
    return out


def analyser_power(S, jones):
    """The power behind an analyser with Jones vector ``jones = (ax, ay)`` (any normalisation, complex allowed), from Stokes
    parameters ``S`` of shape ``(..., 4)`` - a record of ``PlanePropagator.stokes`` -: ``(S0 + q1 S1 + q2 S2 + q3 S3) / 2`` with the
    analyser's normalised Stokes vector ``q = (|ax|^2 - |ay|^2, 2 Re(ax conj ay), 2 Im(conj(ax) ay)) / (|ax|^2 + |ay|^2)``.
    ``(1, 0)`` passes x, ``(0, 1)`` y - the cross-polarised share of an x-polarised emitter's image is ``analyser_power(S, (0, 1))
    / S[..., 0]`` -, ``(1, 1)`` +45 degrees, ``(1, 1j)`` the circular state of ``S3 = +S0`` (positive helicity in the convention of
    ``stokes_maps``).  Pure host code."""
    S = np.asarray(S, dtype=float)
    try:
        ax, ay = (complex(v) for v in jones)
    except (TypeError, ValueError):
        raise ValueError('jones must be the two components (ax, ay) of a Jones vector, got %r' % (jones,)) from None
    n = abs(ax) ** 2 + abs(ay) ** 2
    if S.shape[-1:] != (4,):
        raise ValueError('S must have the four Stokes parameters as its last axis, got shape %s' % (S.shape,))
    if not (np.isfinite(n) and n > 0):
        raise ValueError('jones must be a finite Jones vector other than (0, 0), got %r' % (jones,))
    q1, q2, q3 = (abs(ax) ** 2 - abs(ay) ** 2) / n, 2 * (ax * ay.conjugate()).real / n, 2 * (ax.conjugate() * ay).imag / n
    return 0.5 * (S[..., 0] + q1 * S[..., 1] + q2 * S[..., 2] + q3 * S[..., 3])
