"""The near field propagated to a plane (or a list of points) at FINITE distance behind the lens.

The reference ends in direction space: everything behind the aperture is a far field ``P(ux, uy)``
(nearfield_farfield.py), which says nothing inside the Fraunhofer distance ``2 D^2 / lambda`` - metres for
a millimetre lens.  ``PlanePropagator`` / ``field_at_plane`` are new (the literal reading of
"focal-plane PSF -> image-plane grid"): the Stratton-Chu / Franz fields of the aperture's tangential
equivalent currents,

    E(r) = dx'dy' sum g { i k Z   [a J - b Rhat (Rhat.J)] - c Rhat x M }
    H(r) = dx'dy' sum g { i (k/Z) [a M - b Rhat (Rhat.M)] + c Rhat x J }

with ``R = |r - r'|``, ``g = exp(ikR) / (4 pi R)``, ``a = 1 + i/(kR) - 1/(kR)^2``, ``b = 1 + 3i/(kR) - 3/(kR)^2``,
``c = ik - 1/R``, in the convention of the reference's far field (nearfield_farfield.py:94-101, 183-185):
``J = (-Hy, Hx)``, ``M = (Ey, -Ex)``, ``k = 2 pi n_glass / wavelength``, ``Z = Z0 / n_glass``, ``exp(-i omega t)``.
The sum runs in the HIP kernel ``propagate_kernel`` (csrc/propagate.hip) as a direct fp64 pair sum over the
GPU-resident near field; for ``R -> infinity`` it reduces to the amplitudes behind ``farfield_direct``'s ``P``:
``rho^2 S_r -> P uz / 2``.  There is no CPU path.

``method='fft'``: for a tensor grid of targets on the aperture's own pitch every factor of a (sample, target) pair
depends on the lag ``(i_t - i_s, j_t - j_s)`` alone, and the same sum runs as a zero-padded circular convolution
(csrc/propagate_grid.hip, propagate_grid_fft.hip): ``O(L^2 log L)`` with ``L >= n + m - 1`` per axis instead of ``n^2 m^2`` pairs.
``method='fft-long'`` is the same with padded axes of up to 16384 instead of 8192 - apertures of 4097 ... 8192 samples a
side - and a workspace of up to 77 GB.  ``method='fft-tiled'`` cuts the aperture into tiles, convolves each at a short
padded length ``L >= m`` and adds the tiles' products in the spectral domain (overlap-add): for ``m << n``.
``method='fft-fine'`` is the tiled form for targets on the pitch divided by integers ``(sx, sy)``: the interleave of
``sx sy`` lattices on the pitch, convolved with the same current spectra - what resolves a focal spot.
``method='fft-stack'`` is the fine form for a stack of planes ``z[0], z[1], ...`` (csrc/propagate_stack.hip): one plan, the
currents transformed once, every plane one more layer of kernel spectra - a through-focus volume.
"""
import numpy as np

from . import _lib, constants
from .nearfield_farfield import _check_axis


def _targets(x, y, z, point_list, stack=False):
    x, y, z = (_lib.f64(np.ravel(np.asarray(v, dtype=float))) for v in (x, y, z))
    if x.size < 1 or y.size < 1 or z.size < 1:
        raise ValueError('no targets: x, y and z need at least one value each')
    if stack:   # the refusals of ml_propagate_plan_grid_stack for the planes
        if z.size > STACK_PLANES_MAX:
            raise ValueError("method='fft-stack' takes 1 to %d planes, got %d" % (STACK_PLANES_MAX, z.size))
        bad = ~(np.isfinite(z) & (z > 0))
        if bad.any():
            p = int(np.argmax(bad))
            raise ValueError("method='fft-stack': plane %d lies at z[%d] = %g: the propagator needs a finite z > 0 (the "
                             "aperture is the plane z = 0)" % (p, p, z[p]))
        if z.size * x.size * y.size > 1 << 26:
            raise ValueError("method='fft-stack': %d targets (%d planes of %d x %d fine targets): at most 2^26 per propagator"
                             % (z.size * x.size * y.size, z.size, x.size, y.size))
        return x, y, z
    if point_list:
        if not x.size == y.size == z.size:
            raise ValueError('a point list needs len(x) == len(y) == len(z), got %d, %d and %d'
                             % (x.size, y.size, z.size))
    elif z.size != 1:
        raise ValueError('a tensor grid of targets lies in one plane: z must be one number, got %d '
                         '(point_list=True takes a z per point)' % z.size)
    if not (z > 0).all():
        raise ValueError('every target needs z > 0 (the aperture is the plane z = 0, the field is propagated '
                         'into the half space behind it); got z = %g' % z[~(z > 0)][0])
    return x, y, z


METHODS = ('direct', 'fft', 'fft-long', 'fft-tiled', 'fft-fine', 'fft-stack')   # in the order of ML_PROPAGATE_* (include/metalens_hip.h)
GRID_L_MIN, GRID_L_MAX = 16, 8192   # csrc/propagate_grid.h
GRID_L_LONG_MAX = 16384
_GRID_CAP = {'fft': GRID_L_MAX, 'fft-long': GRID_L_LONG_MAX}
_GRID_METHODS = ('fft', 'fft-long', 'fft-tiled', 'fft-fine', 'fft-stack')   # a tensor grid of targets on the aperture's pitch (or a fraction)
_FINE_METHODS = ('fft-fine', 'fft-stack')   # targets on the pitch divided by `subsample`
FINE_S_MAX = 8   # csrc/propagate_grid.h GRID_FINE_S_MAX
STACK_PLANES_MAX = 4096   # csrc/propagate_grid.h GRID_STACK_PLANES_MAX


def _padded_length(n, m):
    """the padded length of an axis of n samples and m targets (csrc/propagate_grid.h grid_padded_length)"""
    L = 16
    while L < n + m - 1:
        L *= 2
    return L


def _on_pitch(name, t, pitch, s=1, method='fft-fine'):
    """``method='fft'``: the target axis ``t`` must be ``t[0] + i pitch`` to within 4 spacings of its largest value
    (the deviation changes the phase k x of the direct sum by a few 1e-13 rad at that level); ``method='fft-fine'``:
    ``t[0] + i pitch / s`` (``method``: the one of the two fine methods the message names)"""
    tol = 4 * np.spacing(np.abs(t).max())
    off = np.abs(t - (t[0] + np.arange(t.size) * pitch / s)) > tol
    if off.any():
        i = int(np.argmax(off))
        own = t[1] - t[0]
        if s != 1:
            raise ValueError("method=%r needs the targets on the aperture's pitch / %d: %s[%d] = %.17g is not %s[0] + "
                             "%d x %.17g / %d (the aperture's pitch along %s; the target axis steps by %.17g)"
                             % (method, s, name, i, t[i], name, i, pitch, s, name, own))
        raise ValueError("method='fft' needs the targets on the aperture's pitch: %s[%d] = %.17g is not %s[0] + %d x %.17g "
                         "(the aperture's pitch along %s; the target axis steps by %.17g)"
                         % (name, i, t[i], name, i, pitch, name, own))


def tile_default(n, m):
    """the default tile length of ``method='fft-tiled'`` for an axis of n samples and m <= 8192 targets
    (csrc/propagate_grid.h grid_tile_default): the power of two ``L`` in [16, 8192], ``L >= m``, that minimises the
    padded length ``ceil(n / (L - m + 1)) L`` of the axis times the measured cost of a padded sample at that length
    (1 up to 512, then 9/8, 21/16, 45/32 for 1024, 2048 and beyond); of equals the larger"""
    best = None
    L = GRID_L_MIN
    while L <= GRID_L_MAX:
        if L >= m:
            cost = -(-n // (L - m + 1)) * L * (32 if L <= 512 else 36 if L == 1024 else 42 if L == 2048 else 45)
            if best is None or cost <= best[0]:
                best = (cost, L)
        L *= 2
    return best[1]


def _check_tile(name, n, m, L):
    """the refusals of ml_propagate_plan_grid_tiled for one axis, before a context is touched; L None: the default"""
    if m > GRID_L_MAX:
        raise ValueError("method='fft-tiled' takes at most %d targets per axis: the %s axis of n = %d samples has "
                         "m = %d targets; use method='direct' or fewer targets per propagator" % (GRID_L_MAX, name, n, m))
    if L is None or L == 0:
        return 0
    if L != int(L) or not (GRID_L_MIN <= L <= GRID_L_MAX) or int(L) & (int(L) - 1) or L < m:
        raise ValueError("method='fft-tiled': the tile length of the %s axis of n = %d samples and m = %d targets is "
                         "L = %s: it must be a power of two in [%d, %d] and at least m (None or 0: the default)"
                         % (name, n, m, int(L) if L == int(L) else float(L), GRID_L_MIN, GRID_L_MAX))
    return int(L)


def _check_subsample(subsample, method='fft-fine'):
    """-> (sx, sy), integers in [1, 8]; None: (1, 1)"""
    if subsample is None:
        return 1, 1
    try:
        sx, sy = subsample
    except (TypeError, ValueError):
        raise ValueError('subsample must be None or the two pitch ratios (sx, sy), got %r' % (subsample,)) from None
    for name, v in (('x', sx), ('y', sy)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer, float, np.floating)) or v != int(v) \
                or not 1 <= v <= FINE_S_MAX:
            raise ValueError("method=%r divides the aperture's pitch by an integer in [1, %d]: subsample = %r has "
                             "s = %r along %s" % (method, FINE_S_MAX, tuple(subsample), v, name))
    return int(sx), int(sy)


def _check_fine(name, n, m, s, L, method='fft-fine'):
    """the refusals of ml_propagate_plan_grid_fine for one axis of m fine targets at the ratio s, before a context is
    touched: at most 8192 targets per lattice, the tile length against ``m_c = ceil(m / s)``; L None: the default"""
    m_c = -(-m // s)
    if m_c > GRID_L_MAX:
        raise ValueError("method=%r takes at most %d targets per lattice and axis: the %s axis of n = %d samples has "
                         "m = %d fine targets at s = %d, m_c = %d per lattice; use method='direct' or fewer targets per "
                         "propagator" % (method, GRID_L_MAX, name, n, m, s, m_c))
    if L is None or L == 0:
        return 0
    if L != int(L) or not (GRID_L_MIN <= L <= GRID_L_MAX) or int(L) & (int(L) - 1) or L < m_c:
        raise ValueError("method=%r: the tile length of the %s axis of n = %d samples and m_c = %d targets per "
                         "lattice (m = %d fine targets at s = %d) is L = %s: it must be a power of two in [%d, %d] and at "
                         "least m_c (None or 0: the default)"
                         % (method, name, n, m_c, m, s, int(L) if L == int(L) else float(L), GRID_L_MIN, GRID_L_MAX))
    return int(L)


FOCUS_RADII_MAX = 32   # csrc/propagate_focus.h
# the record of a plane (csrc/propagate_focus.h FOCUS_*): peak, its index, the moments of I and of Sz, the centre, the radii's sums
_FOCUS_MOM_I, _FOCUS_MOM_SZ, _FOCUS_CENTRE, _FOCUS_ENC = 2, 8, 14, 16
# the Stokes record of a plane (csrc/propagate_stokes.h STOKES_*): peak, its index, the five sums, the centre, [radius][component]
_STOKES_SUMS, _STOKES_CENTRE, _STOKES_ENC = 2, 7, 9


def _focus_axis(name, t, who='focus()'):
    """-> (pitch, tolerance in index units) of a target axis of ``focus()``: ``(t[-1] - t[0]) / (len(t) - 1)``, with every
    target within ``4 spacing(max |t|)`` of ``t[0] + i pitch`` (the rule of ``_on_pitch``)"""
    if t.size < 2:
        raise ValueError('%s needs at least 2 targets along %s to know their pitch, the axis has %d' % (who, name, t.size))
    pitch = (t[-1] - t[0]) / (t.size - 1)
    if not (np.isfinite(pitch) and pitch > 0):
        raise ValueError('%s needs an ascending target axis: %s runs from %.17g to %.17g' % (who, name, t[0], t[-1]))
    tol = 4 * np.spacing(np.abs(t).max())
    off = np.abs(t - (t[0] + np.arange(t.size) * pitch)) > tol
    if off.any():
        i = int(np.argmax(off))
        raise ValueError('%s needs uniform target axes: %s[%d] = %.17g is not %s[0] + %d x %.17g (the moments and the '
                         'radii are taken on the lattice of the targets)' % (who, name, i, t[i], name, i, pitch))
    return float(pitch), tol / pitch


def _check_focus(p, radii, centre, of, who='focus()'):
    """the argument checks of ``PlanePropagator.focus`` (and of ``SourceSweep.run(image_radii=...)``), before any device
    call -> (radii ascending, the caller's order as indices into them, centres (planes, 2) in index units or None for
    ``'peak'``, planes, dx, dy)"""
    if of not in ('fields', 'sums'):
        raise ValueError("of must be 'fields' or 'sums', got %r" % (of,))
    if p.point_list:
        raise ValueError('%s takes a tensor grid of targets, not a point list: moments and radii need the lattice' % who)
    dx, tol_i = _focus_axis('x', p.x, who)
    dy, tol_j = _focus_axis('y', p.y, who)
    planes = p.z.size if p.method == 'fft-stack' else 1
    r = np.asarray(radii, dtype=float)
    if r.ndim != 1:
        raise ValueError('radii must be a sequence of numbers, got an array of shape %s' % (r.shape,))
    if r.size > FOCUS_RADII_MAX:
        raise ValueError('%s takes at most %d radii, got %d' % (who, FOCUS_RADII_MAX, r.size))
    bad = ~(np.isfinite(r) & (r >= 0))
    if bad.any():
        raise ValueError('a radius must be finite and >= 0: radii[%d] = %g' % (int(np.argmax(bad)), r[np.argmax(bad)]))
    order = np.argsort(r, kind='stable')
    back = np.empty(r.size, dtype=int)
    back[order] = np.arange(r.size)
    return _lib.f64(r[order]), back, _centre_index(p, centre, planes, dx, dy, tol_i, tol_j), planes, dx, dy


def _centre_index(p, centre, planes, dx, dy, tol_i, tol_j):
    """a centre of ``focus()`` / ``otf()`` -> (planes, 2) in index units, None for ``'peak'``"""
    if isinstance(centre, str):
        if centre != 'peak':
            raise ValueError("centre must be 'peak', one (xc, yc) or an array (planes, 2), got %r" % (centre,))
        return None
    try:
        c = np.asarray(centre, dtype=float)
    except (TypeError, ValueError):
        raise ValueError("centre must be 'peak', one (xc, yc) or an array (planes, 2), got %r" % (centre,)) from None
    if c.shape == (2,):
        c = np.broadcast_to(c, (planes, 2))
    if c.shape != (planes, 2):
        raise ValueError("centre must be 'peak', one (xc, yc) or an array (%d, 2) - one centre per plane -, got shape %s"
                         % (planes, np.shape(centre)))
    if not np.isfinite(c).all():
        raise ValueError('a centre must be finite, got %r' % (centre,))
    # index units; a centre within the axes' own tolerance of a target IS that target (a radius of 0 then holds it)
    ci, cj = (c[:, 0] - p.x[0]) / dx, (c[:, 1] - p.y[0]) / dy
    ci = np.where(np.abs(ci - np.rint(ci)) <= tol_i, np.rint(ci), ci)
    cj = np.where(np.abs(cj - np.rint(cj)) <= tol_j, np.rint(cj), cj)
    return _lib.f64(np.stack([ci, cj], axis=1))


OTF_FREQ_MAX = 64   # csrc/propagate_otf.h, ML_OTF_FREQ_MAX


def _otf_axis(name, f, pitch):
    """one frequency axis of ``otf()``: cycles per length -> (cycles per target sample for the device, frequency 0 put in
    front where the caller has none; where the caller's frequencies lie in that array)"""
    f = np.asarray(f, dtype=float)
    if f.ndim != 1 or f.size < 1:
        raise ValueError('f%s must be a sequence of at least one frequency, got an array of shape %s' % (name, f.shape))
    if not np.isfinite(f).all():
        i = int(np.argmax(~np.isfinite(f)))
        raise ValueError('a frequency must be finite: f%s[%d] = %g' % (name, i, f[i]))
    u = f * pitch
    # 1 / (2 pitch) times the pitch may round to the double above 1/2: that is Nyquist
    u = np.where(np.abs(np.abs(u) - 0.5) <= 4 * np.spacing(0.5), np.copysign(0.5, u), u)
    beyond = np.abs(u) > 0.5
    if beyond.any():
        i = int(np.argmax(beyond))
        raise ValueError('f%s[%d] = %.17g lies beyond the Nyquist frequency 1 / (2 d%s) = %.17g of targets %.17g apart'
                         % (name, i, f[i], name, 0.5 / pitch, pitch))
    has_zero = bool((u == 0).any())
    if u.size + (not has_zero) > OTF_FREQ_MAX:
        raise ValueError('otf() takes at most %d frequencies per axis, %d when 0 is not among them (it is added for the '
                         'normalisation): f%s has %d' % (OTF_FREQ_MAX, OTF_FREQ_MAX - 1, name, u.size))
    if has_zero:
        return _lib.f64(u), np.arange(u.size), int(np.argmax(u == 0))
    return _lib.f64(np.concatenate([[0.0], u])), 1 + np.arange(u.size), 0


def _check_otf(p, fx, fy, centre, of):
    """the argument checks of ``PlanePropagator.otf`` (and of ``SourceSweep.run(image_freqs=...)``), before any device call
    -> ((u, the caller's entries, where 0 lies), the same for v, centres (planes, 2) in index units / ``'peak'`` / None, planes,
    dx, dy)"""
    if of not in ('fields', 'sums'):
        raise ValueError("of must be 'fields' or 'sums', got %r" % (of,))
    if p.point_list:
        raise ValueError('otf() takes a tensor grid of targets, not a point list: the transform needs the lattice')
    dx, tol_i = _focus_axis('x', p.x)
    dy, tol_j = _focus_axis('y', p.y)
    planes = p.z.size if p.method == 'fft-stack' else 1
    ax, ay = _otf_axis('x', fx, dx), _otf_axis('y', fy, dy)
    if centre is not None:
        centre = _centre_index(p, centre, planes, dx, dy, tol_i, tol_j)
        if centre is None:
            centre = 'peak'
    return ax, ay, centre, planes, dx, dy


MODES_MAX = 64                 # csrc/propagate_modes.h, ML_MODES_MAX
MODES_OUT_MAX = 1 << 24        # output entries of all slots of a plan (csrc/propagate_modes.h MODES_OUT_MAX)
_MODE_COMPONENTS = ('Ex', 'Ey', 'Hx', 'Hy')   # the blocks of an output slot


def _mode_table(name, m, n):
    """one axis of ``overlap()``: -> complex128 (modes, n), contiguous; a 1-D array is one mode"""
    try:
        t = np.array(m, dtype=np.complex128)
    except (TypeError, ValueError):
        raise ValueError('mode_%s must be an array of numbers of shape (modes, %d) or (%d,)' % (name, n, n)) from None
    if t.ndim == 1:
        t = t[None, :]
    if t.ndim != 2 or t.shape[1] != n or t.shape[0] < 1:
        raise ValueError('mode_%s must have shape (modes, %d) or (%d,) - one axis factor per mode on the %d targets along %s -, '
                         'got %s' % (name, n, n, n, name, np.shape(m)))
    if t.shape[0] > MODES_MAX:
        raise ValueError('overlap() takes at most %d modes per axis: mode_%s has %d' % (MODES_MAX, name, t.shape[0]))
    bad = ~np.isfinite(t)
    if bad.any():
        a, i = np.argwhere(bad)[0]
        raise ValueError('a mode must be finite: mode_%s[%d][%d] = %r' % (name, a, i, complex(t[a, i])))
    return _lib.c128(t)


def _check_overlap(p, mode_x, mode_y, n_slots=1):
    """the argument checks of ``PlanePropagator.overlap`` (and of ``SourceSweep.run(image_modes=...)``), before any device call
    -> (mode_x (nu, len(x)), mode_y (nv, len(y)), planes, dx, dy)"""
    if p.point_list:
        raise ValueError('overlap() takes a tensor grid of targets, not a point list: separable modes need the lattice')
    dx, _ = _focus_axis('x', p.x)
    dy, _ = _focus_axis('y', p.y)
    planes = p.z.size if p.method == 'fft-stack' else 1
    tx, ty = _mode_table('x', mode_x, p.x.size), _mode_table('y', mode_y, p.y.size)
    entries = n_slots * planes * len(_MODE_COMPONENTS) * tx.shape[0] * ty.shape[0]
    if entries > MODES_OUT_MAX:
        raise ValueError('%d sources x %d planes x 4 x %d x %d modes are %d overlaps, at most 2^24 = %d are held on the GPU'
                         % (n_slots, planes, tx.shape[0], ty.shape[0], entries, MODES_OUT_MAX))
    return tx, ty, planes, dx, dy


def _check_overlap_power(power, planes):
    """``power=`` of ``overlap()``: None, a number or an array (planes,) -> None or a float array (planes,)"""
    if power is None:
        return None
    try:
        w = np.asarray(power, dtype=float)
    except (TypeError, ValueError):
        raise ValueError('power must be None, a number or an array (%d,) - one per plane -, got %r' % (planes, power)) from None
    if w.shape not in ((), (planes,)):
        raise ValueError('power must be None, a number or an array (%d,) - one per plane -, got shape %s' % (planes, w.shape))
    return np.broadcast_to(w, (planes,)).copy()


def _overlap_dict(raw, tx, ty, dx, dy, want_h, Z, power, I_dA=None):
    """the numbers of ``ml_propagate_modes_fetch``, complex (..., planes, 4, nu, nv), -> the dict of ``overlap()``; ``power``
    and ``I_dA``: arrays of shape ``raw.shape[:-3]`` (``I_dA`` is read without H and without a power only)"""
    from .postprocess import mode_coupling, mode_norm
    out = {'overlap_' + name: raw[..., c, :, :] * (dx * dy) for c, name in enumerate(_MODE_COMPONENTS[:4 if want_h else 2])}
    out['norm'] = mode_norm(tx, ty, dx, dy)
    out['power'] = I_dA if (power is None and not want_h) else power
    out['coupling_x'], out['coupling_y'] = mode_coupling({k[8:]: v for k, v in out.items() if k.startswith('overlap_')}, out['norm'],
                                                         Z, power=power, I_dA=I_dA)
    return out


def plan_info(ctx):
    """-> ``{'method', 'Lx', 'Ly', 'workspace_bytes'}`` of the context's active propagation plan
    (ml_propagate_plan_info): the padded lengths are 0 for the direct method.  For ``'fft-tiled'`` they are the tile
    lengths, and the dict has ``'tiles': (cx, cy)``, ``'tile_samples': (bx, by)`` and ``'batch'`` as well
    (ml_propagate_plan_tiles); for ``'fft-fine'`` those and ``'subsample': (sx, sy)``, ``'lattice_targets': (m_cx, m_cy)``
    and ``'cache_kernels'`` (ml_propagate_plan_lattices); for ``'fft-stack'`` those of ``'fft-fine'`` and ``'planes'``
    (ml_propagate_plan_planes)"""
    method, lx, ly, ws = _lib.c_int(0), _lib.c_int(0), _lib.c_int(0), _lib.c_int64(0)
    _lib.check(ctx.lib.ml_propagate_plan_info(ctx.handle, _lib.byref(method), _lib.byref(lx), _lib.byref(ly),
                                              _lib.byref(ws)))
    info = {'method': METHODS[method.value], 'Lx': lx.value, 'Ly': ly.value, 'workspace_bytes': ws.value}
    if info['method'] in ('fft-tiled',) + _FINE_METHODS:
        t = [_lib.c_int(0) for _ in range(5)]
        _lib.check(ctx.lib.ml_propagate_plan_tiles(ctx.handle, *[_lib.byref(v) for v in t]))
        info.update(tiles=(t[0].value, t[1].value), tile_samples=(t[2].value, t[3].value), batch=t[4].value)
    if info['method'] in _FINE_METHODS:
        t = [_lib.c_int(0) for _ in range(5)]
        _lib.check(ctx.lib.ml_propagate_plan_lattices(ctx.handle, *[_lib.byref(v) for v in t]))
        info.update(subsample=(t[0].value, t[1].value), lattice_targets=(t[2].value, t[3].value), cache_kernels=bool(t[4].value))
    if info['method'] == 'fft-stack':
        nz = _lib.c_int(0)
        _lib.check(ctx.lib.ml_propagate_plan_planes(ctx.handle, _lib.byref(nz)))
        info['planes'] = nz.value
    return info


class PlanePropagator:
    """The field of one aperture geometry at one set of targets.

    ``xp_list`` / ``yp_list`` are the aperture's axes (what ``build_nearfield`` returns as ``x_pts`` /
    ``y_pts``), ``x``, ``y``, ``z`` the targets in the same frame and the same length unit: the tensor grid
    ``x[:, None] x y[None, :]`` in the plane ``z`` (one number), or with ``point_list=True`` the ``len(x)``
    points ``(x[d], y[d], z[d])`` - a cut through a focus is a point list.  Every ``z`` must be > 0.

    ``propagate_sets()`` does the same for all field sets of a synthesis batch (the x, y, z dipoles of an emitter)
    in one pass and ``accumulate()`` keeps their weighted intensity sums on the GPU (``SourceSweep.run(image=...)``).
    ``focus()`` reduces the resident image - a field set or the sums - to its focus metrics on the GPU: peak, moments,
    the power inside up to 32 radii, per plane (csrc/propagate_focus.hip).  ``otf()`` contracts it with Fourier phasors and
    ``overlap()`` with the caller's separable modes - the coupling into a fibre mode or a Gaussian beam
    (csrc/propagate_otf.hip, csrc/propagate_modes.hip).  ``stokes()`` reduces it to its polarisation state - the Stokes sums, the
    degree of polarisation, the longitudinal share, per plane and inside radii - and ``accumulate_stokes()`` keeps the Stokes
    maps of a sweep (csrc/propagate_stokes.hip).

    ``propagate()`` sums the field set resident on the GPU (the selected one of a batch) and returns a dict
    with ``Ex, Ey, Ez, Hx, Hy, Hz`` (complex128, shape ``(len(x), len(y))`` or ``(len(x),)``) and
    ``Sz = Re(E x H*)_z / 2``; with ``want_h=False`` ``Ex, Ey, Ez`` and ``I = |E|^2`` only (about 40 % less
    arithmetic).  The far-field plan, the sweep sums, the method and the precision of the context are not
    touched.  A context that belongs to a multi-rank communicator is refused.

    ``method='direct'`` (default) is the pair sum.  ``method='fft'`` computes the same sum as an FFT convolution
    (csrc/propagate_grid*.hip).  It takes a tensor grid only, both of whose axes lie on the aperture's pitch as the C
    ABI defines it (``xp_list[1] - xp_list[0]``, likewise y): ``|x[i] - (x[0] + i dxp)| <= 4 spacing(max |x|)``; one
    target along an axis is accepted, and the origin ``x[0] - xp_list[0]`` is arbitrary (no multiple of the pitch).
    Each axis is padded to ``L`` = the smallest power of two ``>= max(16, n + m - 1)``, at most 8192; the workspace is
    ``(12 + 6 or 3) Lx Ly`` complex128 (``plan_info()``).  Everything else - ``propagate_sets``, ``accumulate``,
    ``sums``, ``SourceSweep.run(image=...)`` - is as for the direct method.  The kernel spectra are computed by the
    first pass and kept while this propagator stays the one that planned last on the context.

    ``method='fft-long'`` is ``'fft'`` with ``L`` of at most 16384 (ml_propagate_plan_grid_long): for apertures of 4097
    ... 8192 samples a side, which ``'fft'`` can give one target per axis at the most.  The same checks, the same
    results - bit for bit where both methods accept a problem; an axis of ``L = 16384`` takes one more pass over the
    planes per transform.  It is a method of its own because of its workspace: ``(12 + 6 or 3) Lx Ly 16`` bytes are up
    to 77 GB (64 GB with ``want_h=False``) where ``'fft'`` never reserves more than 18 GB.  The first pass reserves it
    and raises ``MetalensHipError`` with the bytes asked for if the device cannot give them.

    ``method='fft-tiled'`` is the FFT form for a small patch behind a large aperture (ml_propagate_plan_grid_tiled):
    overlap-add over tiles of the aperture.  Per axis the tile length ``L`` is a power of two in [16, 8192] with
    ``L >= m``; the n samples are cut into ``ceil(n / B)`` tiles of ``B = L - m + 1``, every tile is convolved at the
    padded length ``L`` and the tiles' products are added in the spectral domain in front of one inverse transform.
    The padded length of an axis is ``ceil(n / B) L`` instead of up to ``2 n`` - 8192 samples to 64 targets: 19 tiles of
    512 instead of 16384 - and n is not bounded by it: this is the only FFT form of apertures beyond 8192 samples a
    side.  ``tile=(Lx, Ly)`` sets the tile lengths (None or 0 for an axis: its default); the default (``tile_default``)
    minimises the padded length weighted by the measured cost of a padded sample at that length, the larger ``L`` of
    equals.  The same checks as ``'fft'``; at most 8192 targets per axis.  A plan of one tile - the default where a tile
    of at most 512 holds the axis and shorter tiles would pad it no less - has the bits of ``'fft'``.  The workspace is ``(8 cx cy + 4 batch + 6 or 3) Lx Ly`` complex128; ``plan_info()`` reports the tile
    lengths as ``Lx``, ``Ly`` and adds ``'tiles'``, ``'tile_samples'`` and ``'batch'``.

    ``method='fft-fine'`` is the tiled form for a patch FINER than the aperture's pitch (ml_propagate_plan_grid_fine):
    ``subsample=(sx, sy)``, integers in [1, 8], and ``x``, ``y`` on the pitch divided by them, ``|x[i] - (x[0] + i dxp /
    sx)| <= 4 spacing(max |x|)``.  Per axis the targets ``a, a + s, a + 2 s, ...`` are lattice ``a``, on the pitch with the
    origin ``x[a]``; every lattice is the sum of ``'fft-tiled'`` at that origin with ``m_c = ceil(m / s)`` targets per axis
    - ``tile`` and its default are checked against ``m_c``, at most 8192 - and has its bits where it holds ``m_c`` targets
    per axis.  One plan serves all lattices: the currents are transformed once per field set, tile by tile, the lattices
    are contracted two per read of the current spectra, and the result arrives interleaved, shape ``(len(x), len(y))``
    as for every method, so ``propagate_sets``, ``accumulate``, ``sums`` and ``SourceSweep.run(image=...)`` are unchanged.
    ``cache_kernels=True`` (default) keeps the kernel spectra of all ``A = min(sx, mx) min(sy, my)`` lattices from the
    first pass on, a workspace of ``(8 A cx cy + 4 cx cy + 2 (6 or 3)) Lx Ly`` complex128; ``cache_kernels=False`` fills
    and transforms those of two lattices and one batch of tiles in every pass, ``(16 batch + 4 cx cy + 2 (6 or 3)) Lx
    Ly``, with the same bits.  The first pass reserves the workspace and raises ``MetalensHipError`` with the bytes asked
    for (and ``cache_kernels=0``) if the device cannot give them.  ``subsample=(1, 1)`` has the bits of ``'fft-tiled'``.
    ``plan_info()`` adds ``'subsample'``, ``'lattice_targets'`` and ``'cache_kernels'`` to the keys of ``'fft-tiled'``.
    ``subsample``, and ``cache_kernels=False``, belong to this method and to ``'fft-stack'``.

    ``method='fft-stack'`` is ``'fft-fine'`` for a STACK of planes (ml_propagate_plan_grid_stack): ``z`` is a sequence of
    1 to 4096 planes, each finite and > 0, in any order and with repeats allowed; ``x``, ``y``, ``subsample``, ``tile`` and
    ``cache_kernels`` are those of ``'fft-fine'``, with the same checks.  The fine plan does not depend on z, so one plan
    serves the volume: the currents are transformed once per field set, and every (plane, lattice) is one more layer of
    kernel spectra contracted against them, two per read.  Plane ``p`` has the bits of ``'fft-fine'`` planned at ``z[p]``.
    ``shape`` is ``(len(z), len(x), len(y))`` - 3-D even for one plane - for every returned array, for ``sums()`` and for the
    ``I_sum``, ``Sz_sum`` and ``image_each`` of ``SourceSweep.run(image=...)``; at most 2^26 targets in all.
    ``cache_kernels=True`` keeps the kernel spectra of all ``len(z) A`` layers, ``(8 len(z) A cx cy + 4 cx cy + 2 (6 or 3))
    Lx Ly`` complex128 - 128 B per padded index and layer; ``cache_kernels=False`` takes the streamed workspace of
    ``'fft-fine'`` whatever ``len(z)`` is and fills the kernels of a pair of layers and a batch of tiles in one launch per
    pass.  ``plan_info()`` adds ``'planes'`` to the keys of ``'fft-fine'``.  Several z belong to this method alone: every
    other tensor grid lies in one plane.
    """

    def __init__(self, xp_list, yp_list, wavelength, n_glass, x, y, z, *, point_list=False, want_h=True,
                 units=None, Z0=None, ctx=None, method='direct', tile=None, subsample=None, cache_kernels=True):
        if method not in METHODS:
            raise ValueError('method must be one of %s, got %r' % (METHODS, method))
        if tile is not None and method not in ('fft-tiled',) + _FINE_METHODS:
            raise ValueError("tile=%r: the tile lengths belong to method='fft-tiled', not to method=%r" % (tile, method))
        if subsample is not None and method not in _FINE_METHODS:
            raise ValueError("subsample=%r: the pitch ratios belong to method='fft-fine', not to method=%r" % (subsample, method))
        if cache_kernels is not True and method not in _FINE_METHODS:
            raise ValueError("cache_kernels=%r: the choice belongs to method='fft-fine', not to method=%r" % (cache_kernels, method))
        if tile is not None and len(tile) != 2:
            raise ValueError('tile must be None or the two tile lengths (Lx, Ly), got %r' % (tile,))
        self.method = method
        self.Z0 = constants.as_units(units).Z0 if Z0 is None else Z0
        _check_axis(xp_list, wavelength)
        _check_axis(yp_list, wavelength)
        self.point_list, self.want_h = bool(point_list), bool(want_h)
        if method in _GRID_METHODS and self.point_list:
            raise ValueError("method=%r takes a tensor grid of targets on the aperture's pitch, not a point list" % method)
        self.x, self.y, self.z = _targets(x, y, z, self.point_list, stack=method == 'fft-stack')
        self.shape = (self.x.size,) if self.point_list else (self.x.size, self.y.size)
        if method == 'fft-stack':
            self.shape = (self.z.size,) + self.shape   # 3-D even for one plane
        self.aperture_shape = (len(xp_list), len(yp_list))
        self._geometry = (float(xp_list[0]), float(yp_list[0]), float(xp_list[1] - xp_list[0]),
                          float(yp_list[1] - yp_list[0]), float(wavelength), float(n_glass))
        self.tile = (0, 0)   # 0: the default length
        fine = method if method in _FINE_METHODS else 'fft-fine'   # (the fine method the messages name)
        self.subsample, self.cache_kernels = _check_subsample(subsample, fine), bool(cache_kernels)
        if method in _GRID_METHODS:
            _on_pitch('x', self.x, self._geometry[2], self.subsample[0], fine)
            _on_pitch('y', self.y, self._geometry[3], self.subsample[1], fine)
        if method in _FINE_METHODS:
            Lx, Ly = (None, None) if tile is None else tile   # (None or 0 for an axis: its default)
            self.tile = (_check_fine('x', self.aperture_shape[0], self.x.size, self.subsample[0], Lx, method),
                         _check_fine('y', self.aperture_shape[1], self.y.size, self.subsample[1], Ly, method))
        if method == 'fft-tiled':
            Lx, Ly = (None, None) if tile is None else tile   # (None or 0 for an axis: its default)
            self.tile = (_check_tile('x', self.aperture_shape[0], self.x.size, Lx),
                         _check_tile('y', self.aperture_shape[1], self.y.size, Ly))
        if method in _GRID_CAP:
            cap = _GRID_CAP[method]
            for name, n, m in (('x', self.aperture_shape[0], self.x.size), ('y', self.aperture_shape[1], self.y.size)):
                L = _padded_length(n, m)
                if L > cap:
                    hint = " or, up to L = %d, method='fft-long'" % GRID_L_LONG_MAX if method == 'fft' else ''
                    raise ValueError("method=%r pads the %s axis of n = %d samples and m = %d targets to L = %d > %d; "
                                     "use method='direct' or fewer targets per propagator%s"
                                     % (method, name, n, m, L, cap, hint))
        self.ctx = ctx or _lib.default_context()
        self.owner = _lib.new_owner()
        self._plan()

    def _plan(self):
        ctx = self.ctx
        if self.method == 'fft-stack':
            (sx, sy), mx, my = self.subsample, self.x.size, self.y.size
            first_x, first_y = _lib.f64(self.x[:min(sx, mx)]), _lib.f64(self.y[:min(sy, my)])   # the lattices' origins
            _lib.check(ctx.lib.ml_propagate_plan_grid_stack(
                ctx.handle, *self._geometry, _lib.dptr(first_x), sx, _lib.dptr(first_y), sy, mx, my,
                _lib.dptr(self.z), self.z.size, int(self.want_h), *self.tile, int(self.cache_kernels)))
        elif self.method == 'fft-fine':
            (sx, sy), mx, my = self.subsample, self.x.size, self.y.size
            first_x, first_y = _lib.f64(self.x[:min(sx, mx)]), _lib.f64(self.y[:min(sy, my)])   # the lattices' origins
            _lib.check(ctx.lib.ml_propagate_plan_grid_fine(
                ctx.handle, *self._geometry, _lib.dptr(first_x), sx, _lib.dptr(first_y), sy, mx, my,
                float(self.z[0]), int(self.want_h), *self.tile, int(self.cache_kernels)))
        elif self.method == 'fft-tiled':
            _lib.check(ctx.lib.ml_propagate_plan_grid_tiled(
                ctx.handle, *self._geometry, float(self.x[0]), float(self.y[0]), self.x.size, self.y.size,
                float(self.z[0]), int(self.want_h), *self.tile))
        elif self.method in _GRID_CAP:
            entry = ctx.lib.ml_propagate_plan_grid if self.method == 'fft' else ctx.lib.ml_propagate_plan_grid_long
            _lib.check(entry(
                ctx.handle, *self._geometry, float(self.x[0]), float(self.y[0]), self.x.size, self.y.size,
                float(self.z[0]), int(self.want_h)))
        else:
            _lib.check(ctx.lib.ml_propagate_plan(
                ctx.handle, *self._geometry, _lib.dptr(self.x), self.x.size, _lib.dptr(self.y), self.y.size,
                _lib.dptr(self.z), self.z.size, int(self.point_list), int(self.want_h)))
        ctx.propagate_owner = self.owner

    def plan_info(self):
        """``plan_info(self.ctx)``: of the plan that is active on the context now, whoever made it"""
        return plan_info(self.ctx)

    def _ready(self):
        """the resident field must have the aperture's shape; plans again if another propagator has planned on the
        context since"""
        ctx = self.ctx
        nx, ny = _lib.c_int(0), _lib.c_int(0)
        _lib.check(ctx.lib.ml_fields_shape(ctx.handle, _lib.byref(nx), _lib.byref(ny)))
        if (nx.value, ny.value) != self.aperture_shape:
            raise ValueError('the resident near field is %d x %d but the axes given have %d and %d '
                             'points' % ((nx.value, ny.value) + self.aperture_shape))
        if ctx.propagate_owner != self.owner:
            self._plan()

    def _download(self, member):
        """-> the result dict of member ``member`` of the last pass (``None``: of ``ml_propagate``)"""
        ctx = self.ctx
        E = np.empty((3,) + self.shape, dtype=np.complex128)
        H = np.empty((3,) + self.shape, dtype=np.complex128) if self.want_h else None
        if member is None:
            _lib.check(ctx.lib.ml_propagate_download(ctx.handle, _lib.dptr(E), _lib.dptr(H)))
        else:
            _lib.check(ctx.lib.ml_propagate_download_set(ctx.handle, member, _lib.dptr(E), _lib.dptr(H)))
        out = {'Ex': E[0], 'Ey': E[1], 'Ez': E[2]}
        if self.want_h:
            out.update(Hx=H[0], Hy=H[1], Hz=H[2])
            out['Sz'] = 0.5 * np.real(E[0] * np.conj(H[1]) - E[1] * np.conj(H[0]))
        else:
            out['I'] = (np.abs(E) ** 2).sum(axis=0)
        return out

    def propagate(self):
        """-> dict of the fields at the targets, from the resident near field (plans again if another
        propagator has planned on the context since)"""
        self._ready()
        _lib.check(self.ctx.lib.ml_propagate(self.ctx.handle, self.Z0))
        return self._download(None)

    def queue_sets(self, first=0, n=None):
        """queue ONE pass over the resident field sets ``first ... first + n - 1`` (default: all of them; at most
        three - the members of a synthesis batch) without synchronising; -> n.  The geometry of a (sample, target)
        pair is computed once for all sets; every set's fields have the bits ``propagate()`` gives for it."""
        self._ready()
        ctx = self.ctx
        if n is None:
            resident = _lib.c_int(0)
            _lib.check(ctx.lib.ml_fields_sets(ctx.handle, _lib.byref(resident)))
            n = resident.value - first
        _lib.check(ctx.lib.ml_propagate_sets(ctx.handle, self.Z0, int(first), int(n)))
        return n

    def propagate_sets(self, first=0, n=None):
        """-> list of the dicts ``propagate()`` returns, one per resident field set ``first ... first + n - 1``
        (default: all of them), from one pass over the aperture (``queue_sets``)"""
        n = self.queue_sets(first, n)
        return [self._download(m) for m in range(n)]

    def accumulate(self, weights, reset=False):
        """add the sets of the last ``queue_sets`` / ``propagate_sets`` pass into the sums kept on the GPU:
        ``I += sum_m weights[m] |E_m|^2`` and, with ``want_h``, ``Sz += sum_m weights[m] Sz_m``
        (``reset``: the sums start from zero).  Asynchronous."""
        ctx = self.ctx
        if ctx.propagate_owner != self.owner:
            raise RuntimeError('another propagator has planned on the context since this one propagated')
        w = _lib.f64(np.ravel(np.asarray(weights, dtype=float)))
        _lib.check(ctx.lib.ml_propagate_accumulate(ctx.handle, _lib.dptr(w), w.size, int(bool(reset))))

    def sums(self):
        """-> ``(I_sum, Sz_sum)`` of ``accumulate``, of shape ``self.shape``; ``Sz_sum`` is None without ``want_h``"""
        ctx = self.ctx
        I = np.empty(self.shape)
        Sz = np.empty(self.shape) if self.want_h else None
        _lib.check(ctx.lib.ml_propagate_sums(ctx.handle, _lib.dptr(I), _lib.dptr(Sz)))
        return I, Sz

    def focus(self, radii=(), centre='peak', member=0, of='fields'):
        """The focus metrics of the image that is resident on the GPU, reduced there (``ml_propagate_focus``,
        csrc/propagate_focus.hip): nothing but a record of ``16 + 2 len(radii)`` doubles per plane crosses PCIe.

        ``of='fields'``: of member ``member`` of the last ``propagate()`` / ``queue_sets()`` / ``propagate_sets()`` pass,
        with ``I = |E|^2`` and ``Sz = Re(E x H*)_z / 2``; ``of='sums'``: of the sums of ``accumulate()`` as they are stored
        (``member`` is ignored).  ``radii``: up to 32 radii in the targets' length unit, in any order; ``centre``: ``'peak'``
        (every plane's own peak, read on the device), one ``(xc, yc)`` in the targets' frame, or an array ``(planes, 2)``.
        A target is inside radius ``R`` iff ``(dx (i - ci))^2 + (dy (j - cj))^2 <= R^2`` in index units about the centre
        ``(ci, cj) = ((xc - x[0]) / dx, (yc - y[0]) / dy)`` - a centre within the axes' tolerance of a target is that
        target.  The targets must be a tensor grid with uniform ascending axes of at least 2 targets each,
        ``|x[i] - (x[0] + i dx)| <= 4 spacing(max |x|)`` with ``dx = (x[-1] - x[0]) / (len(x) - 1)``.

        -> dict of arrays whose leading axis is the planes (1 unless ``method='fft-stack'``): ``peak_I``, ``peak_index``
        (``(planes, 2)`` ints, the lowest flat index of equals) and ``peak_xy``; ``I_dA = sum I dx dy``; ``centroid_I =
        (x[0] + dx sum I i / sum I, ...)`` (NaN where the sum is 0) and ``second_moments_I``, central, in length^2, as ``(xx,
        yy, xy)``; ``centre_index`` and ``centre_xy``, the centre used; ``encircled_I`` of shape ``(planes, len(radii))``,
        ``sum I dx dy`` inside each radius, in the caller's order.  With ``want_h``: ``P = sum Sz dx dy``, ``centroid_Sz``,
        ``second_moments_Sz`` and ``encircled_P`` as well.  Bit for bit repeatable; plane ``p`` of a stack has the numbers
        of that plane planned alone.  Synchronises."""
        r, back, c, planes, dx, dy = _check_focus(self, radii, centre, of)
        ctx = self.ctx
        if ctx.propagate_owner != self.owner:
            raise RuntimeError('another propagator has planned on the context since this one propagated')
        K, mx, my = r.size, self.x.size, self.y.size
        rd = _FOCUS_ENC + 2 * K
        rec = np.empty((planes, rd))
        _lib.check(ctx.lib.ml_propagate_focus(ctx.handle, -1 if of == 'sums' else int(member), mx, my, planes, dx, dy,
                                              _lib.dptr(c), _lib.dptr(r) if K else None, K, _lib.dptr(rec), rd))
        flat = rec[:, 1].astype(np.int64)
        out = {'peak_I': rec[:, 0].copy(), 'peak_index': np.stack([flat // my, flat % my], axis=1)}
        out['peak_xy'] = np.stack([self.x[out['peak_index'][:, 0]], self.y[out['peak_index'][:, 1]]], axis=1)
        out['centre_index'] = rec[:, _FOCUS_CENTRE:_FOCUS_CENTRE + 2].copy()
        out['centre_xy'] = np.stack([self.x[0] + dx * rec[:, _FOCUS_CENTRE], self.y[0] + dy * rec[:, _FOCUS_CENTRE + 1]], axis=1)
        for name, total, at, enc, e_at in (('I', 'I_dA', _FOCUS_MOM_I, 'encircled_I', _FOCUS_ENC),
                                           ('Sz', 'P', _FOCUS_MOM_SZ, 'encircled_P', _FOCUS_ENC + K)):
            if name == 'Sz' and not self.want_h:
                continue
            s, si, sj, sii, sjj, sij = (rec[:, at + q] for q in range(6))
            with np.errstate(divide='ignore', invalid='ignore'):
                mi, mj = np.where(s != 0, si / s, np.nan), np.where(s != 0, sj / s, np.nan)
                out['second_moments_' + name] = np.stack([dx * dx * (sii / s - mi * mi), dy * dy * (sjj / s - mj * mj),
                                                          dx * dy * (sij / s - mi * mj)], axis=1)
            out[total] = s * dx * dy
            out['centroid_' + name] = np.stack([self.x[0] + dx * mi, self.y[0] + dy * mj], axis=1)
            out[enc] = rec[:, e_at:e_at + K][:, back] * dx * dy
        return out

    def stokes(self, radii=(), centre='peak', member=0, of='fields'):
        """The polarisation state of the image that is resident on the GPU, reduced there (``ml_propagate_stokes``,
        csrc/propagate_stokes.hip): a record of ``9 + 5 len(radii)`` doubles per plane crosses PCIe, not three complex maps.

        Per target, from ``Ex, Ey, Ez`` alone (``postprocess.stokes_maps`` is the same arithmetic, to the bit): ``S0 = |Ex|^2 +
        |Ey|^2``, ``S1 = |Ex|^2 - |Ey|^2``, ``S2 = 2 Re(Ex conj Ey)``, ``S3 = 2 Im(conj(Ex) Ey)`` and the longitudinal ``Iz =
        |Ez|^2``.  ``S3 = +S0`` for ``E`` proportional to ``x^ + i y^``: under the project's ``exp(-i omega t)``, for a wave
        travelling to +z, that is the field rotating counter-clockwise seen looking towards the source (positive helicity).

        ``of='fields'``: of member ``member`` of the last pass; ``of='sums'``: of the maps of ``accumulate_stokes()`` as they
        are stored (``member`` is ignored) - the incoherent image of an unpolarised emitter.  ``radii``, ``centre``, the
        membership rule and the conditions on the targets are those of ``focus()``; ``centre='peak'`` reads every plane's peak
        with a first call and takes the radii about it with a second.

        -> dict of arrays whose leading axis is the planes (1 unless ``method='fft-stack'``): ``peak_I``, ``peak_index``,
        ``peak_xy``, ``centre_index``, ``centre_xy`` as ``focus()`` gives them (of a member, ``peak_I`` and ``peak_index`` to the
        bit); ``S`` of shape ``(planes, 4)``, ``sum S_q dx dy``; ``Iz_dA``; ``longitudinal_share = Iz / (S0 + Iz)``; ``dop =
        sqrt(S1^2 + S2^2 + S3^2) / S0`` of the integrated values (NaN where ``S0`` is 0); ``orientation = atan2(S2, S1) / 2``;
        ``ellipticity = asin(S3 / sqrt(S1^2 + S2^2 + S3^2)) / 2``; ``encircled_S`` of shape ``(planes, len(radii), 4)``,
        ``encircled_Iz`` and ``encircled_dop`` of shape ``(planes, len(radii))``, in the caller's order.  Repeatable bit for bit;
        plane ``p`` of a stack has the numbers of that plane planned alone, and a radius those it has alone.  ``postprocess.
        analyser_power(out['S'], (ax, ay))`` is the power behind an analyser.  Synchronises."""
        from .postprocess import _stokes_state
        r, back, c, planes, dx, dy = _check_focus(self, radii, centre, of, 'stokes()')
        ctx = self.ctx
        if ctx.propagate_owner != self.owner:
            raise RuntimeError('another propagator has planned on the context since this one propagated')
        K, mx, my = r.size, self.x.size, self.y.size
        source = -1 if of == 'sums' else int(member)

        def call(centres, k):
            rec = np.empty((planes, _STOKES_ENC + 5 * k))
            _lib.check(ctx.lib.ml_propagate_stokes(ctx.handle, source, mx, my, planes, dx, dy, _lib.dptr(centres),
                                                   _lib.dptr(r) if k else None, k, _lib.dptr(rec), rec.shape[1]))
            return rec
        if c is None and K:   # about the peak: read it first
            c = _lib.f64(call(None, 0)[:, _STOKES_CENTRE:_STOKES_CENTRE + 2])
        rec = call(c, K)
        flat = rec[:, 1].astype(np.int64)
        out = {'peak_I': rec[:, 0].copy(), 'peak_index': np.stack([flat // my, flat % my], axis=1)}
        out['peak_xy'] = np.stack([self.x[out['peak_index'][:, 0]], self.y[out['peak_index'][:, 1]]], axis=1)
        out['centre_index'] = rec[:, _STOKES_CENTRE:_STOKES_CENTRE + 2].copy()
        out['centre_xy'] = np.stack([self.x[0] + dx * rec[:, _STOKES_CENTRE], self.y[0] + dy * rec[:, _STOKES_CENTRE + 1]], axis=1)
        out['S'] = rec[:, _STOKES_SUMS:_STOKES_SUMS + 4] * dx * dy
        out['Iz_dA'] = rec[:, _STOKES_SUMS + 4] * dx * dy
        out['longitudinal_share'], out['dop'], out['orientation'], out['ellipticity'] = _stokes_state(out['S'], out['Iz_dA'])
        enc = rec[:, _STOKES_ENC:].reshape(planes, K, 5)[:, back] * dx * dy
        out['encircled_S'], out['encircled_Iz'] = enc[:, :, :4], enc[:, :, 4]
        out['encircled_dop'] = _stokes_state(out['encircled_S'], out['encircled_Iz'])[1]
        return out

    def accumulate_stokes(self, weights, reset=False):
        """add the sets of the last ``queue_sets`` / ``propagate_sets`` pass into the five Stokes maps kept on the GPU:
        ``S_q += sum_m weights[m] S_q of set m`` for ``S0, S1, S2, S3`` and ``Iz`` (``reset``: the maps start from zero; the
        first call needs it).  Beside ``accumulate()``, whose sums it does not touch.  Asynchronous."""
        ctx = self.ctx
        if ctx.propagate_owner != self.owner:
            raise RuntimeError('another propagator has planned on the context since this one propagated')
        w = _lib.f64(np.ravel(np.asarray(weights, dtype=float)))
        _lib.check(ctx.lib.ml_propagate_accumulate_stokes(ctx.handle, _lib.dptr(w), w.size, int(bool(reset))))

    def stokes_sums(self):
        """-> the maps of ``accumulate_stokes``, ``(S0, S1, S2, S3, Iz)``, of shape ``(5,) + self.shape``"""
        ctx = self.ctx
        out = np.empty((5,) + self.shape)
        _lib.check(ctx.lib.ml_propagate_stokes_sums(ctx.handle, _lib.dptr(out)))
        return out

    def otf(self, fx, fy, member=0, of='fields', centre=None):
        """The transfer function of the image that is resident on the GPU - the Fourier transform of ``I = |E|^2`` (and of
        ``Sz`` with ``want_h``) at the frequencies ``fx`` x ``fy`` -, contracted there (``ml_propagate_otf``,
        csrc/propagate_otf.hip): ``2 len(fx) len(fy)`` complex numbers per plane cross PCIe, not the image.

        ``fx``, ``fy``: 1-D sequences in cycles per length unit of the targets, in any order, repeats allowed, none beyond
        the Nyquist frequency ``1 / (2 dx)``; at most 64 per axis, 63 when 0 is not among them (it is added for the
        normalisation and stripped again; an entry does not depend on the other frequencies of a call).  ``member``, ``of``
        and the conditions on the targets are those of ``focus()``.  ``centre`` is the phase reference: None - the first
        target, ``(x[0], y[0])`` -, ``'peak'`` - every plane's own peak, from ``focus()`` -, one ``(xc, yc)`` in the targets'
        frame or an array ``(planes, 2)``; it is applied on the host as ``exp(+2 pi i (fx (xc - x[0]) + fy (yc - y[0])))``.

        -> dict of arrays whose leading axis is the planes (1 unless ``method='fft-stack'``): ``otf_I`` of shape ``(planes,
        len(fx), len(fy))``, ``sum_ij I exp(-2 pi i (fx (x_i - xc) + fy (y_j - yc))) dx dy``; ``mtf_I = |otf_I| / otf_I(0, 0)``
        (NaN where that is 0); with ``want_h`` ``otf_Sz`` and ``mtf_Sz``; ``fx`` and ``fy`` as given.  Repeatable bit for bit;
        plane ``p`` of a stack has the numbers of that plane planned alone.  Synchronises."""
        (u, iu, u0), (v, iv, v0), c, planes, dx, dy = _check_otf(self, fx, fy, centre, of)
        ctx = self.ctx
        if ctx.propagate_owner != self.owner:
            raise RuntimeError('another propagator has planned on the context since this one propagated')
        if isinstance(c, str):
            c = self.focus(member=member, of=of)['peak_index'].astype(float)
        raw = np.empty((planes, 2, u.size, v.size), dtype=np.complex128)
        _lib.check(ctx.lib.ml_propagate_otf(ctx.handle, -1 if of == 'sums' else int(member), self.x.size, self.y.size, planes,
                                            _lib.dptr(u), u.size, _lib.dptr(v), v.size, _lib.dptr(raw)))
        turn = 1.0
        if c is not None:   # the phase reference, with u ci reduced to its fraction first
            px, py = u[None, :] * c[:, :1], v[None, :] * c[:, 1:]
            turn = np.exp(2j * np.pi * (px - np.rint(px)))[:, :, None] * np.exp(2j * np.pi * (py - np.rint(py)))[:, None, :]
        out = {}
        for w, name in enumerate(('I', 'Sz')[:2 if self.want_h else 1]):
            zero = raw[:, w, u0, v0].real[:, None, None]
            with np.errstate(divide='ignore', invalid='ignore'):   # (the modulus is the device's own: no phase reference moves it)
                out['mtf_' + name] = np.where(zero != 0, np.abs(raw[:, w]) / zero, np.nan)[:, iu][:, :, iv]
            out['otf_' + name] = (raw[:, w] * turn)[:, iu][:, :, iv] * (dx * dy)
        out['fx'], out['fy'] = np.array(fx, dtype=float), np.array(fy, dtype=float)
        return out

    def overlap(self, mode_x, mode_y, member=0, power=None):
        """The overlap of the image that is resident on the GPU with separable modes ``psi_ab(x, y) = mode_x[a](x)
        mode_y[b](y)`` - how much of the light enters a single-mode fibre, a Gaussian beam of a given waist, a Hermite-Gauss
        order -, contracted there (``ml_propagate_modes_plan`` / ``_queue`` / ``_fetch``, csrc/propagate_modes.hip): ``4 nu nv``
        complex numbers per plane cross PCIe, not the image.

        ``mode_x``: complex array ``(nu, len(x))`` - the axis factors sampled on the targets' x axis (``metalens_amd.modes``
        has Gaussian and Hermite-Gauss factors) - or ``(len(x),)`` for one mode; likewise ``mode_y`` with ``(nv, len(y))``;
        finite, at most 64 per axis, in any order, repeats allowed.  The tensor product serves Hermite-Gauss orders ``m x
        n``, a grid of lateral fibre offsets, or a scan of waists taken from the diagonal; a mode that is a sum of separable
        terms (LP01) is served by one call with the terms as modes, whose overlaps add.  Their normalisation is immaterial:
        ``norm`` divides it out.  ``member``: of the last ``propagate()`` / ``queue_sets()`` / ``propagate_sets()`` pass (the
        sums of ``accumulate()`` carry no phase).  The targets must be a tensor grid with uniform ascending axes, as for
        ``focus()``.

        The mode model is paraxial: an x-polarised mode has ``e = psi x^``, ``h = z^ x e / Z = psi y^ / Z`` with ``Z = Z0 /
        n_glass``, a y-polarised one ``e = psi y^``, ``h = -psi x^ / Z``; its power is ``norm / (2 Z)``.  The patch of
        targets must hold the mode: what of ``psi`` lies outside it is missing from the overlap and from ``norm`` alike.

        -> dict of arrays whose leading axis is the planes (1 unless ``method='fft-stack'``): ``overlap_Ex``, ``overlap_Ey`` and
        with ``want_h`` ``overlap_Hx``, ``overlap_Hy``, complex ``(planes, nu, nv)``, ``sum_ij conj(psi_ab) F dx dy``; ``norm``
        ``(nu, nv)``, ``(sum_i |mode_x[a, i]|^2 dx) (sum_j |mode_y[b, j]|^2 dy)``; ``power`` ``(planes,)``; ``coupling_x`` and
        ``coupling_y`` ``(planes, nu, nv)``, the power coupled into the x- or y-polarised mode over ``power`` (NaN where
        ``norm`` or ``power`` is 0).  With ``want_h``
            ``coupling_x = |O_Ex / Z + O_Hy|^2 Z / (8 norm power)``,  ``coupling_y = |O_Ey / Z - O_Hx|^2 Z / (8 norm power)``
        and ``power=None`` means ``focus(member=member)['P']``, the power through the patch.  Without H and with
        ``power=None``: ``|O_Ex|^2 / (norm I_dA)``, the Cauchy-Schwarz share of ``I_dA = sum |E|^2 dx dy`` (returned as
        ``power``), at most 1; with a power given ``|O_Ex|^2 / (2 Z norm power)``.  ``power``: a number or an array
        ``(planes,)``, e.g. the incident power.  Repeatable bit for bit; plane ``p`` of a stack has the numbers of that plane
        planned alone; an entry does not depend on the other modes of the call.  Synchronises."""
        tx, ty, planes, dx, dy = _check_overlap(self, mode_x, mode_y)
        power = _check_overlap_power(power, planes)
        ctx = self.ctx
        if ctx.propagate_owner != self.owner:
            raise RuntimeError('another propagator has planned on the context since this one propagated')
        self._modes_plan(tx, ty, planes, 1)
        _lib.check(ctx.lib.ml_propagate_modes_queue(ctx.handle, int(member), 0))
        raw = self._modes_fetch(1, planes, tx.shape[0], ty.shape[0])[0]
        I_dA = None
        if power is None:
            foc = self.focus(member=member)
            power, I_dA = (foc['P'], None) if self.want_h else (None, foc['I_dA'])
        return _overlap_dict(raw, tx, ty, dx, dy, self.want_h, self.Z0 / self._geometry[5], power, I_dA)

    def _modes_plan(self, tx, ty, planes, n_slots):
        """upload the mode tables of ``_check_overlap`` and reserve ``n_slots`` output slots on the active plan"""
        _lib.check(self.ctx.lib.ml_propagate_modes_plan(self.ctx.handle, self.x.size, self.y.size, planes, _lib.dptr(tx), tx.shape[0],
                                                        _lib.dptr(ty), ty.shape[0], int(n_slots)))

    def _modes_fetch(self, n_slots, planes, nu, nv):
        """-> complex (n_slots, planes, 4, nu, nv): the slots 0 ... n_slots - 1"""
        raw = np.empty((n_slots, planes, len(_MODE_COMPONENTS), nu, nv), dtype=np.complex128)
        _lib.check(self.ctx.lib.ml_propagate_modes_fetch(self.ctx.handle, 0, int(n_slots), _lib.dptr(raw)))
        return raw


def field_at_plane(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, x, y, z, *, point_list=False,
                   want_h=True, units=None, Z0=None, ctx=None, method='direct', tile=None, subsample=None,
                   cache_kernels=True):
    """One-shot convenience, modelled on ``farfield_direct``: the field of host arrays ``Ex..Hy`` (or of the
    field set already resident on the GPU if ``Ex is None``, e.g. after ``build_nearfield(..., download=False)``
    or a ``HotPath`` step) at the targets.  Arguments and the returned dict as for ``PlanePropagator``."""
    p = PlanePropagator(xp_list, yp_list, wavelength, n_glass, x, y, z, point_list=point_list, want_h=want_h,
                        units=units, Z0=Z0, ctx=ctx, method=method, tile=tile, subsample=subsample,
                        cache_kernels=cache_kernels)
    ctx = p.ctx
    if Ex is not None:
        arrs = [_lib.c128(a) for a in (Ex, Ey, Hx, Hy)]
        assert arrs[0].shape == arrs[1].shape == arrs[2].shape == arrs[3].shape == (len(xp_list), len(yp_list))
        _lib.check(ctx.lib.ml_fields_upload(ctx.handle, len(xp_list), len(yp_list),
                                            *[_lib.dptr(a) for a in arrs]))
        ctx.fields_owner = None
    return p.propagate()
