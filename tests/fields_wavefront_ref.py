"""Yardstick of the Zernike moments of the near field's wavefront (ml_fields_zernike, ``ApertureWavefront``,
``postprocess.wavefront_metrics``): a plain-NumPy restatement of the definitions - membership in fp64, exactly as the
interface states it - and the sums evaluated in ``np.longdouble`` from the same fp64 inputs (``k``, ``x``, ``y``, the centre, the
radius and the reference's parameters are taken as the doubles they are).  ``sum C Z_j`` is evaluated DIRECTLY: ``Z_j`` from its
radial polynomial in ``rho`` and ``cos / sin(m phi)``, ``phi = atan2(eta, xi)``, per member in long double - independent of the
monomial route the product takes.  Nothing here imports the package.

Bounds, with u = 2^-53, n the members of the pupil, Phi = max |phi| over them, and per term ``amp_j = N_j sum_pq |A_j,pq|``
(the integer coefficients of ``Z_j / N_j`` as a polynomial in (xi, eta), expanded here by polynomial multiplication):
  samples, outside   exact
  sum S, sum I       |d| <= (n + 16) u sum |term|, |term| of S taken as (|Ex| |Hy| + |Ey| |Hx|) / 2 (fields_zones_ref.py)
  moments            |d| <= amp_j (4 Phi + n + 64 + n_max) u sum |E| per component (Re, Im).  A member's share of
                     ``A_j,pq M_pq`` is ``A C xi^p eta^q`` with |xi^p eta^q| <= 1, so every relative error below counts against
                     ``|A| |E|`` and the sum over (p, q) gives amp_j:  forming phi, at most 4 roundings of u Phi each;  sincos_cw,
                     2^-51 = 4 u;  the two products and the sum of a component of C, 3 u;  xi and eta (a difference and a
                     quotient: 2 u each factor) and their powers by repeated multiplication (u each): 3 (p + q) u <= 3 n_max u;
                     the products ``C eta^q`` and ``xi^p T_q``, 2 u;  the additions over the samples, n u;  ``A M`` and at most 25
                     additions of a term's non-zero coefficients, 26 u;  N_j and the product by it, 2 u;  dA / (pi R^2) on
                     the way into the dict, 4 u.  Together (4 Phi + n + 41 + 3 n_max) u, which 64 + n_max covers for every
                     n_max <= 8 (41 + 24 = 65 <= 72).
"""
from math import factorial

import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def wave_number(wavelength, n_glass):
    return 2 * np.pi * n_glass / wavelength


def terms(n_max):
    """(n, m) in OSA/ANSI order"""
    return [(n, m) for n in range(n_max + 1) for m in range(-n, n + 1, 2)]


def membership(x, y, radius, centre):
    """-> bool (nx, ny): (x - xc)^2 + (y - yc)^2 <= R R in fp64, one rounded addition"""
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    return ((x - centre[0]) ** 2)[:, None] + ((y - centre[1]) ** 2)[None, :] <= float(radius) * float(radius)


def phase_ld(x, y, wavelength, n_glass, reference):
    """the reference phase on the grid in long double from the fp64 inputs"""
    x, y, k = np.asarray(x, dtype=float).astype(LD), np.asarray(y, dtype=float).astype(LD), LD(wave_number(wavelength, n_glass))
    if reference[0] == 'plane':
        ux, uy = LD(float(reference[1])), LD(float(reference[2]))
        return k * (ux * x)[:, None] + k * (uy * y)[None, :]
    xf, yf, zf = (LD(float(v)) for v in reference[1:])
    return -np.sign(zf) * k * np.sqrt(((x - xf) ** 2)[:, None] + ((y - yf) ** 2)[None, :] + zf * zf)


def zernike_ld(n, m, xi, eta):
    """Z_n^m, Noll-normalised, in long double from the radial polynomial and cos / sin(m phi)"""
    xi, eta = np.asarray(xi, dtype=LD), np.asarray(eta, dtype=LD)
    a = abs(m)
    rho, phi = np.sqrt(xi * xi + eta * eta), np.arctan2(eta, xi)
    R = np.zeros(np.broadcast(xi, eta).shape, dtype=LD)
    for s in range((n - a) // 2 + 1):
        c = (-1) ** s * factorial(n - s) // (factorial(s) * factorial((n + a) // 2 - s) * factorial((n - a) // 2 - s))
        R = R + LD(c) * rho ** (n - 2 * s)
    N = np.sqrt(LD(n + 1)) if m == 0 else np.sqrt(LD(2 * (n + 1)))
    return N * R * (np.cos(LD(m) * phi) if m >= 0 else np.sin(LD(a) * phi))


def _pmul(f, g):
    out = {}
    for (p1, q1), a in f.items():
        for (p2, q2), b in g.items():
            out[(p1 + p2, q1 + q2)] = out.get((p1 + p2, q1 + q2), 0) + a * b
    return out


def coefficients(n, m):
    """{(p, q): A}: Z_n^m / N as a polynomial in (xi, eta), by multiplying polynomials out: rho^2 = xi^2 + eta^2, and
    rho^a cos / sin(a phi) = Re / Im (xi + i eta)^a with Gaussian-integer coefficients"""
    a = abs(m)
    z = {(0, 0): 1}
    for _ in range(a):
        z = _pmul(z, {(1, 0): 1, (0, 1): 1j})
    ang = {key: int(round(complex(v).real if m >= 0 else complex(v).imag)) for key, v in z.items()}
    out = {}
    for s in range((n - a) // 2 + 1):
        c = (-1) ** s * factorial(n - s) // (factorial(s) * factorial((n + a) // 2 - s) * factorial((n - a) // 2 - s))
        r2t = {(0, 0): 1}
        for _ in range((n - a) // 2 - s):
            r2t = _pmul(r2t, {(2, 0): 1, (0, 2): 1})
        for key, v in _pmul(r2t, ang).items():
            out[key] = out.get(key, 0) + c * v
    return {key: v for key, v in sorted(out.items()) if v != 0}


def amplitudes(n_max):
    """amp_j = N_j sum |A_j,pq| per term"""
    return np.array([np.sqrt(n + 1.0 if m == 0 else 2.0 * (n + 1)) * sum(abs(v) for v in coefficients(n, m).values()) for n, m in terms(n_max)])


def exact(F, x, y, wavelength, n_glass, radius, n_max, centre=(0.0, 0.0), reference=('plane', 0.0, 0.0)):
    """F: (sets, 4, nx, ny) complex128, Ex, Ey, Hx, Hy per set -> dict: ``n``, ``outside``, ``S`` (sets,), ``I`` (sets, 2), ``Zr``,
    ``Zi`` (sets, 2, J): Re, Im of sum C Z_j, all long double and WITHOUT the factor dA; ``S_abs`` (sets,), ``E_abs`` (sets, 2): the
    sums of |term| and of |E| the bounds take; ``phi_max``; ``dA``; ``R``; ``n_max``"""
    F = np.asarray(F, dtype=np.complex128)
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    inside = membership(x, y, radius, centre)
    phi = phase_ld(x, y, wavelength, n_glass, reference)[inside]
    c, s = np.cos(phi), np.sin(phi)
    R = LD(float(radius))
    xi = np.broadcast_to(((x.astype(LD) - LD(float(centre[0]))) / R)[:, None], inside.shape)[inside]
    eta = np.broadcast_to(((y.astype(LD) - LD(float(centre[1]))) / R)[None, :], inside.shape)[inside]
    Z = [zernike_ld(n, m, xi, eta) for n, m in terms(n_max)]
    sets, J = F.shape[0], len(Z)
    out = {'n': int(inside.sum()), 'outside': int((~inside).sum()), 'phi_max': float(np.abs(phi).max()) if phi.size else 0.0,
           'R': float(radius), 'n_max': n_max}
    out['S'], out['S_abs'] = np.zeros(sets, LD), np.zeros(sets, LD)
    out['I'], out['E_abs'] = np.zeros((sets, 2), LD), np.zeros((sets, 2), LD)
    out['Zr'], out['Zi'] = np.zeros((sets, 2, J), LD), np.zeros((sets, 2, J), LD)
    for m in range(sets):
        ex, ey, hx, hy = (F[m, f][inside] for f in range(4))
        r = lambda a: a.real.astype(LD)
        i = lambda a: a.imag.astype(LD)
        out['S'][m] = ((r(ex) * r(hy) + i(ex) * i(hy) - r(ey) * r(hx) - i(ey) * i(hx)) / 2).sum()
        out['S_abs'][m] = ((np.abs(ex).astype(LD) * np.abs(hy) + np.abs(ey).astype(LD) * np.abs(hx)) / 2).sum()
        for p, e in enumerate((ex, ey)):
            out['I'][m, p] = (r(e) * r(e) + i(e) * i(e)).sum()
            out['E_abs'][m, p] = np.hypot(r(e), i(e)).sum()
            cr, ci = r(e) * c + i(e) * s, i(e) * c - r(e) * s
            for j in range(J):
                out['Zr'][m, p, j], out['Zi'][m, p, j] = (cr * Z[j]).sum(), (ci * Z[j]).sum()
    out['dA'] = (abs(x[1] - x[0]) if x.size > 1 else 1.0) * (abs(y[1] - y[0]) if y.size > 1 else 1.0)
    return out


def _ratio(err, bound):
    """the worst err / bound; where the bound is 0 the error must be 0 too (-> inf if not)"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    r = np.zeros(err.shape, dtype=LD)
    pos = bound > 0
    r[pos] = err[pos] / bound[pos]
    r[~pos & (err != 0)] = np.inf
    return float(r.max()) if r.size else 0.0


def moment_bound(want):
    """the bound of a component of ``moments`` (sets, 2, J), with the factor dA / (pi R^2) of the dict"""
    n_max, scale = want['n_max'], LD(want['dA']) / (LD(np.pi) * LD(want['R']) * LD(want['R']))
    return (LD(1) * amplitudes(n_max)[None, None, :] * (4 * LD(want['phi_max']) + LD(want['n']) + 64 + n_max) * U
            * want['E_abs'][:, :, None] * scale)


def ratios(got, want):
    """``got``: the dict of ``analyse`` / ``wavefront_metrics``; ``want``: ``exact`` of the same case -> the worst error over its
    bound for S, I and the moments Z.  The integers are asserted here."""
    n_max = want['n_max']
    assert got['samples'].dtype == np.int64 and got['samples'] == want['n'] and got['outside'] == want['outside']
    assert got['terms'].tolist() == [list(t) for t in terms(n_max)]
    assert got['area'] == want['n'] * want['dA']
    dA, n = LD(want['dA']), LD(want['n'])
    out = {'S': _ratio(np.abs(got['P'].astype(LD) - want['S'] * dA), (n + 16) * U * want['S_abs'] * dA),
           'I': _ratio(np.abs(got['I'].astype(LD) - want['I'] * dA), (n + 16) * U * want['I'] * dA)}
    scale = dA / (LD(np.pi) * LD(want['R']) * LD(want['R']))
    bound = moment_bound(want)
    assert got['moments'].shape == want['Zr'].shape
    out['Z'] = max(_ratio(np.abs(got['moments'].real.astype(LD) - want['Zr'] * scale), bound),
                   _ratio(np.abs(got['moments'].imag.astype(LD) - want['Zi'] * scale), bound))
    # for the record, not asserted: the same differences in units of u sum |E|, without the terms' amplitudes
    unit = np.broadcast_to(U * want['E_abs'][:, :, None] * scale, bound.shape)
    out['Zu'] = max(_ratio(np.abs(got['moments'].real.astype(LD) - want['Zr'] * scale), unit),
                    _ratio(np.abs(got['moments'].imag.astype(LD) - want['Zi'] * scale), unit))
    return out


def hold(name, got, want):
    """print the PARITY line of a case and assert the bounds"""
    r = ratios(got, want)
    print('PARITY wavefront %-30s sets %d n_max %d members %6d  worst error / bound: S %.3f  I %.3f  Z %.4f  (Phi %.3g; Z in u sum |E|: %.3g)'
          % (name, got['P'].shape[0], want['n_max'], want['n'], r['S'], r['I'], r['Z'], want['phi_max'], r['Zu']))
    assert r['S'] <= 1 and r['I'] <= 1 and r['Z'] <= 1, (name, r)
    # what follows from the sums: the coherence lies in [0, 1] (Cauchy-Schwarz, to rounding) and is NaN exactly where n sum I is
    # 0; the piston is the angle of the first moment; the wavefront is NaN exactly where that moment is 0
    den = want['n'] * got['I']
    assert np.array_equal(np.isnan(got['coherence']), den == 0)
    ok = ~np.isnan(got['coherence'])
    lim = 1 + 3 * (4 * want['phi_max'] + want['n'] + 64) * U
    assert (got['coherence'][ok] >= 0).all() and (got['coherence'][ok] <= lim).all()
    assert np.array_equal(got['piston'], np.angle(got['moments'][..., 0]))
    gone = got['moments'][..., 0] == 0
    assert np.array_equal(np.isnan(got['wavefront']), np.broadcast_to(gone[..., None], got['wavefront'].shape))
    assert np.array_equal(np.isnan(got['rms']), gone)
    assert (np.abs(got['wavefront'][~gone][:, 0]) <= 4 * U).all()             # (Im(z / z): 0 to the rounding of the division)
    return r


def seeded_fields(sets, nx, ny, seed):
    """(sets, 4, nx, ny) complex fields of a seeded generator, magnitudes over three decades"""
    rng = np.random.default_rng(seed)
    amp = 10.0 ** rng.uniform(-2, 1, (sets, 4, nx, ny))
    return amp * np.exp(2j * np.pi * rng.uniform(0, 1, (sets, 4, nx, ny)))


# the seeded cases of the yardstick: name, x, y, wavelength, n_glass, radius, n_max, centre, reference
def cases():
    wl, ng = 580e-9, 1.46
    p = wl / 2.2
    out = []
    x, y = (np.arange(130) - 64.5) * p, (np.arange(129) - 64) * p
    out.append(('130x129 focus 30 um order 8', x, y, wl, ng, 15e-6, 8, (0.0, 0.0), ('focus', 0.0, 0.0, 30e-6)))
    x, y = (np.arange(70) - 30.3) * p, (np.arange(257) - 100.7) * p
    out.append(('70x257 off axis order 5', x, y, wl, ng, 9.1e-6, 5, (0.37e-6, -1.21e-6), ('focus', 1.1e-6, -0.6e-6, 45e-6)))
    x = y = (np.arange(64) - 31.5) * p
    out.append(('64x64 zf -2 mm order 4', x, y, wl, ng, 7e-6, 4, (0.0, 0.0), ('focus', 0.0, 0.0, -2e-3)))
    x, y = (np.arange(90) - 44.5) * p, (np.arange(75) - 20.0) * p
    out.append(('90x75 plane (0.3, -0.2) order 3', x, y, wl, ng, 8e-6, 3, (0.2e-6, 0.1e-6), ('plane', 0.3, -0.2)))
    x, y = 1e-3 + (np.arange(66) - 30.0) * p, 1e-3 + (np.arange(130) - 64.0) * p
    out.append(('66x130 plane (0.7, 0.7) order 0', x, y, wl, ng, 6e-6, 0, (1e-3, 1e-3), ('plane', 0.7, 0.7)))
    return out
