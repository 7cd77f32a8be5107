"""Yardstick of the pupil function applied to a near field (ml_fields_pupil_plan / ml_fields_pupil_apply, ``AperturePupil``,
``postprocess.pupil_factor`` and ``apply_pupil_host``): a plain-NumPy restatement of the definition.  Membership and zone are
taken in fp64 exactly as the interface states them - ``r2 = (x - xc)^2 + (y - yc)^2``, one rounded addition, a member iff ``r2 <=
R R``, zone ``searchsorted(edges^2, r2, 'left')``.  The phase ``psi = sum_j c_j Z_j`` is evaluated DIRECTLY in ``np.longdouble``: ``Z_j``
from its radial polynomial in ``rho`` and ``cos / sin(m phi)`` (``zernike_ld`` of fields_wavefront_ref.py), with ``xi``, ``eta`` formed
in long double from the fp64 axes - independent of the monomial route the product takes.  The product ``E g exp(i psi)`` is
formed in long double from the fp64 fields and factors.  Nothing here imports the package.

Which samples change (csrc/fields_pupil.h): a stopped non-member becomes +0.0 + 0.0i exactly; a member with a phase, and any
sample left standing in a zone ``z < K``, is multiplied; every other sample keeps its bytes.

Bound per real component of a multiplied sample, with u = 2^-53, ``Psi = sum_j |c_j| amp_j`` and ``amp_j = N_j sum_pq |A_j,pq|``
(``amplitudes`` of fields_wavefront_ref.py), on a member:
    |d| <= |g| |E| ((64 + 5 n_max) Psi + 24) u
First term, the error of psi, each count against ``Psi >= sum_pq |B_pq| >= |psi|`` because |xi^p eta^q| <= 1 on the disc:
  ``B_pq``: the product ``c_j N_j`` (N_j rounded: 2 u), the product by the integer ``A`` (u) and at most 44 additions over the
  terms (44 u): 47 u;  ``xi`` and ``eta`` (a difference and a quotient: 2 u each factor, against the long-double values here) and
  their powers inside the Horner passes: 3 (p + q) u <= 3 n_max u;  the two Horner passes, a product and a sum per step:
  (2 n_max + 2) u.  Together (49 + 5 n_max) u Psi, which 64 + 5 n_max covers.
Second term, on |g| |E|: ``sincos_cw`` is good to 2^-51 = 4 u per component, 4 sqrt(2) u on the unit phasor;  ``f = g (cs + i sn)``
and ``E f`` are two complex products of three roundings per component each, 2 * 3 sqrt(2) u.  Together 10 sqrt(2) u = 14.2 u,
which 24 covers.
A non-member left standing in a zone takes ``g`` alone: one complex product, inside the second term (Psi counts 0 there).
The derivation governs; the bound is never fitted to what the code under test gives.
"""
import numpy as np

import fields_wavefront_ref as wref

U = wref.U
LD = np.longdouble


def parts(x, y, radius, centre=(0.0, 0.0), stop=True, phase=None, edges=None, zone_factors=None):
    """-> dict: ``member``, ``zero`` (stopped non-members), ``touch`` (multiplied samples), ``fr``, ``fi`` (the factor in long double,
    1 + 0i where nothing applies), ``g_abs`` (fp64 modulus of the zone factor in long double), ``Psi`` and ``n_max``"""
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    R = float(radius)
    r2 = ((x - centre[0]) ** 2)[:, None] + ((y - centre[1]) ** 2)[None, :]
    member = r2 <= R * R
    zero = ~member & bool(stop)
    gr, gi = np.ones(r2.shape, dtype=LD), np.zeros(r2.shape, dtype=LD)
    factor = np.zeros(r2.shape, dtype=bool)
    if edges is not None:
        e = np.asarray(edges, dtype=float)
        g = np.asarray(zone_factors, dtype=complex)
        zone = np.searchsorted(e * e, r2, side='left')
        factor = (zone < e.size) & ~zero
        at = np.minimum(zone, e.size - 1)
        gr = np.where(factor, g.real[at].astype(LD), LD(1))
        gi = np.where(factor, g.imag[at].astype(LD), LD(0))
    Psi, n_max = 0.0, 0
    phased = np.zeros(r2.shape, dtype=bool)
    fr, fi = gr, gi
    if phase is not None:
        c = np.asarray(phase, dtype=float)
        n_max = {(n + 1) * (n + 2) // 2: n for n in range(9)}[c.size]
        Psi = float((np.abs(c) * wref.amplitudes(n_max)).sum())
        phased = member
        xi = np.broadcast_to(((x.astype(LD) - LD(float(centre[0]))) / LD(R))[:, None], r2.shape)
        eta = np.broadcast_to(((y.astype(LD) - LD(float(centre[1]))) / LD(R))[None, :], r2.shape)
        psi = np.zeros(r2.shape, dtype=LD)
        if member.any():
            acc = np.zeros(int(member.sum()), dtype=LD)
            for cj, (n, m) in zip(c, wref.terms(n_max)):
                if cj != 0:
                    acc = acc + LD(cj) * wref.zernike_ld(n, m, xi[member], eta[member])
            psi[member] = acc
        cs, sn = np.cos(psi), np.sin(psi)
        fr = np.where(phased, gr * cs - gi * sn, gr)
        fi = np.where(phased, gr * sn + gi * cs, gi)
    return dict(member=member, zero=zero, touch=~zero & (factor | phased), fr=fr, fi=fi, g_abs=np.hypot(gr, gi), Psi=Psi, n_max=n_max)


def hold(name, got, F, want):
    """``got``, ``F``: (sets, 4, nx, ny) complex128, after and before; ``want``: ``parts`` of the pupil.  Prints the PARITY line and
    asserts: exact +0.0 where stopped, the bytes of ``F`` where untouched, the bound where multiplied -> worst error / bound"""
    got, F = np.asarray(got, dtype=np.complex128), np.asarray(F, dtype=np.complex128)
    assert got.shape == F.shape and got.shape[-2:] == want['member'].shape
    zero, touch = want['zero'], want['touch']
    keep = ~zero & ~touch
    z = got[..., zero]
    assert (z.real == 0).all() and (z.imag == 0).all() and not np.signbit(z.real).any() and not np.signbit(z.imag).any(), name
    assert got[..., keep].tobytes() == F[..., keep].tobytes(), name
    worst = 0.0
    if touch.any():
        E = F[..., touch]
        er, ei = E.real.astype(LD), E.imag.astype(LD)
        fr, fi = want['fr'][touch], want['fi'][touch]
        wr, wi = er * fr - ei * fi, er * fi + ei * fr
        psi_term = np.where(want['member'][touch], LD((64 + 5 * want['n_max']) * want['Psi']), LD(0))
        bound = want['g_abs'][touch] * np.hypot(er, ei) * (psi_term + 24) * U
        g = got[..., touch]
        for d in (np.abs(g.real.astype(LD) - wr), np.abs(g.imag.astype(LD) - wi)):
            worst = max(worst, wref._ratio(d, np.broadcast_to(bound, d.shape)))
    print('PARITY pupil %-44s sets %d n_max %d Psi %-8.3g members %6d stopped %6d multiplied %6d untouched %6d  worst error / bound %.4f'
          % (name, got.shape[0], want['n_max'], want['Psi'], int(want['member'].sum()), int(zero.sum()), int(touch.sum()), int(keep.sum()), worst))
    assert worst <= 1, (name, worst)
    return worst


def seeded_fields(sets, nx, ny, seed):
    return wref.seeded_fields(sets, nx, ny, seed)


def seeded_phase(n_max, seed, scale=1.0):
    """J coefficients of a seeded generator in (-scale, scale) rad"""
    return np.random.default_rng(seed).uniform(-scale, scale, (n_max + 1) * (n_max + 2) // 2)
