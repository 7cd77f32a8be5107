"""Yardstick of the per-zone contributions to the field at points behind the aperture (ml_fields_zone_fields,
``ApertureZoneFields``, ``postprocess.zone_fields``): for every slot - the K zones and the outside - the direct pair sum of
tests/propagate_ref.py on the fields masked to that slot, in plain fp64 and in ``np.longdouble``.  Membership is that of
tests/fields_zones_ref.py.  Nothing here imports the package.

The yardstick is the long-double stack; ``e_ref`` is the error of the fp64 stack against it (``propagate_ref.max_error`` over
all slots, components and targets together), and a result passes within ``MARGIN * e_ref`` - the margin
tests/test_gpu_propagate.py takes for this arithmetic.  A closure (the slots added up against the sum over the unmasked
fields) compares two results that are each within the margin: ``2 * MARGIN * e_ref``."""
import numpy as np

import fields_zones_ref
import propagate_ref

MARGIN = 8
seeded_fields = fields_zones_ref.seeded_fields
membership = fields_zones_ref.membership


def _integrands(F, x, y, wl, ng, point, real, pitch, Z0):
    """the summands of ``propagate_ref.direct_sum`` for one target, expression by expression as it forms them -> six arrays
    (nx, ny): those of Ex, Ey, Ez, Hx, Hy, Hz, and (dx', dy')"""
    cplx = np.complex128 if real is np.float64 else np.clongdouble
    k = real(2 * np.pi * ng / wl)
    Z = real(Z0 / ng)
    pi = 4 * np.arctan(real(1))
    x0, y0 = real(x[0]), real(y[0])
    dxp, dyp = (real(v) for v in propagate_ref._pitches(x, y, pitch))
    X, Y = np.meshgrid(x0 + np.arange(len(x)).astype(real) * dxp, y0 + np.arange(len(y)).astype(real) * dyp, indexing='ij')
    Ex, Ey, Hx, Hy = (np.asarray(f).astype(cplx) for f in F)
    Jx, Jy, Mx, My = -Hy, Hx, Ey, -Ex
    i = cplx(1j)

    def dyad(a, b, ux, uy, uz, Vx, Vy):      # a V - b Rhat (Rhat . V), V tangential
        dot = ux * Vx + uy * Vy
        return a * Vx - b * ux * dot, a * Vy - b * uy * dot, -b * uz * dot

    def cross(ux, uy, uz, Vx, Vy):           # Rhat x V
        return -uz * Vy, uz * Vx, ux * Vy - uy * Vx

    px, py, pz = point
    Rx, Ry, Rz = real(px) - X, real(py) - Y, real(pz)
    R = np.sqrt(Rx ** 2 + Ry ** 2 + Rz ** 2)
    ux, uy, uz = Rx / R, Ry / R, Rz / R
    kr = k * R
    g = np.exp(i * kr) / (4 * pi * R)
    a = 1 + i / kr - 1 / kr ** 2
    b = 1 + 3 * i / kr - 3 / kr ** 2
    c = i * k - 1 / R
    dJ, cM = dyad(a, b, ux, uy, uz, Jx, Jy), cross(ux, uy, uz, Mx, My)
    dM, cJ = dyad(a, b, ux, uy, uz, Mx, My), cross(ux, uy, uz, Jx, Jy)
    return ([g * (i * k * Z * dJ[m] - c * cM[m]) for m in range(3)] + [g * (i * (k / Z) * dM[m] + c * cJ[m]) for m in range(3)]), dxp, dyp


def exact(F, x, y, wl, ng, edges, centre, points, real, pitch=None, Z0=propagate_ref.Z0_SI, by_direct_sum=False):
    """F: (sets, 4, nx, ny) complex128 -> E, H of shape (sets, K + 1, 3, T) in ``real``: slot z is ``propagate_ref.direct_sum``
    of the fields masked to the samples of zone z, slot K of those outside every edge (a slot without samples: zeros, which
    is what the sum over zero fields gives).

    ``by_direct_sum``: literally so, one call per slot - K + 1 times the geometry of every pair.  Otherwise the summands of the
    unmasked fields are formed once per target and masked: every operation of ``direct_sum`` acts sample by sample, a sample
    whose fields are zero has summands of exact zeros and a member's summands do not notice the mask, so the array that is
    summed - and with it the sum, bit for bit - is the same (tests/test_zone_fields_host.py holds the two against each other)."""
    F = np.asarray(F, dtype=np.complex128)
    K, T = len(edges), len(points)
    zone = membership(x, y, edges, centre)
    cplx = np.complex128 if real is np.float64 else np.clongdouble
    E, H = np.zeros((F.shape[0], K + 1, 3, T), dtype=cplx), np.zeros((F.shape[0], K + 1, 3, T), dtype=cplx)
    masks = [(z, zone == z) for z in np.unique(zone)]
    for m in range(F.shape[0]):
        if by_direct_sum:
            for z, mask in masks:
                E[m, z], H[m, z] = propagate_ref.direct_sum(*[np.where(mask, F[m, f], 0) for f in range(4)], x, y, wl, ng, points, Z0,
                                                            real=real, pitch=pitch)
            continue
        for t, point in enumerate(np.asarray(points, dtype=np.float64).reshape(-1, 3)):
            terms, dxp, dyp = _integrands(F[m], x, y, wl, ng, point, real, pitch, Z0)
            for z, mask in masks:
                for d in range(3):
                    E[m, z, d, t] = np.where(mask, terms[d], 0).sum() * dxp * dyp
                    H[m, z, d, t] = np.where(mask, terms[3 + d], 0).sum() * dxp * dyp
    return E, H


def counts(x, y, edges, centre):
    """the members of the K + 1 slots"""
    return np.bincount(membership(x, y, edges, centre).ravel(), minlength=len(edges) + 1)


def yardstick(F, x, y, wl, ng, edges, centre, points, pitch=None):
    """-> dict: ``E``, ``H`` (the long-double stacks), ``e_ref_E``, ``e_ref_H`` (the error of the fp64 stacks against them),
    ``n`` (the members of the K + 1 slots)"""
    E64, H64 = exact(F, x, y, wl, ng, edges, centre, points, np.float64, pitch)
    E, H = exact(F, x, y, wl, ng, edges, centre, points, np.longdouble, pitch)
    return dict(E=E, H=H, e_ref_E=propagate_ref.max_error(E64, E), e_ref_H=propagate_ref.max_error(H64, H),
                n=counts(x, y, edges, centre))


def slots(d, field='E'):
    """the dict of ``analyse`` / ``zone_fields`` -> (sets, K + 1, 3, T): the zones, then the outside"""
    return np.concatenate([d[field], d['outside_' + field][:, None]], axis=1)


def hold(name, got, want, factor=1):
    """print the PARITY line of a case and assert E and H of ``got`` (a dict of ``analyse``) within ``factor * MARGIN * e_ref`` of
    the yardstick ``want``; the members exactly, empty slots exact zeros"""
    assert np.array_equal(got['samples'], want['n'][:-1]) and got['outside'] == want['n'][-1], name
    out = {}
    for f in ('E', 'H'):
        if f not in got:
            continue
        g = slots(got, f)
        err = propagate_ref.max_error(g, want[f])
        out[f] = err
        print('PARITY zone fields %-26s %s  error %.3e  e_ref %.3e  ratio %.2f (allowed %d)'
              % (name, f, err, want['e_ref_' + f], err / want['e_ref_' + f] if want['e_ref_' + f] else np.inf, factor * MARGIN))
        assert err <= factor * MARGIN * want['e_ref_' + f], (name, f, err, want['e_ref_' + f])
        empty = want['n'] == 0
        assert (g[:, empty] == 0).all(), name
    return out
