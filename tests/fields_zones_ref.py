"""Yardstick of the per-zone sums of the near field (ml_fields_zones, ``ApertureZones``, ``postprocess.zone_metrics``): a
plain-NumPy restatement of the definitions - membership in fp64, exactly as the interface states it - and the sums
evaluated in ``np.longdouble`` from the same fp64 inputs (``k``, ``x``, ``y``, the reference's parameters are taken as the
doubles they are).  Nothing here imports the package.

Bounds, with u = 2^-53, n the members of a zone and Phi = max |phi| of the case:
  samples, outside   exact
  sum S, sum I       |d| <= (n + 16) u sum |term|, |term| of S taken as (|Ex| |Hy| + |Ey| |Hx|) / 2 (the bound of
                     test_gpu_propagate_focus.py)
  sum C              |d| <= (4 Phi + n + 64) u sum |E|: at most 4 roundings in forming phi, each u Phi; 2^-51 per value of
                     sincos_cw; the roundings of the products and of the sum
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def wave_number(wavelength, n_glass):
    return 2 * np.pi * n_glass / wavelength


def membership(x, y, edges, centre):
    """-> zone (nx, ny), K for a sample outside every edge"""
    x, y, e = np.asarray(x, dtype=float), np.asarray(y, dtype=float), np.asarray(edges, dtype=float)
    X2, Y2, E2 = (x - centre[0]) ** 2, (y - centre[1]) ** 2, e * e
    return np.searchsorted(E2, X2[:, None] + Y2[None, :], side='left')


def phase_ld(x, y, wavelength, n_glass, reference):
    """the reference phase on the grid in long double from the fp64 inputs"""
    x, y, k = np.asarray(x, dtype=float).astype(LD), np.asarray(y, dtype=float).astype(LD), LD(wave_number(wavelength, n_glass))
    if reference[0] == 'plane':
        ux, uy = LD(float(reference[1])), LD(float(reference[2]))
        return k * (ux * x)[:, None] + k * (uy * y)[None, :]
    xf, yf, zf = (LD(float(v)) for v in reference[1:])
    return -np.sign(zf) * k * np.sqrt(((x - xf) ** 2)[:, None] + ((y - yf) ** 2)[None, :] + zf * zf)


def exact(F, x, y, wavelength, n_glass, edges, centre=(0.0, 0.0), reference=('plane', 0.0, 0.0)):
    """F: (sets, 4, nx, ny) complex128, Ex, Ey, Hx, Hy per set -> dict: ``n`` (K,), ``outside``, ``S`` (sets, K), ``I`` (sets, K,
    2), ``C`` (sets, K, 2) complex, all long double and WITHOUT the factor dA; ``S_abs``, ``E_abs`` (sets, K, 2): the sums of
    |term| and of |E| the bounds take; ``phi_max``; ``dA``"""
    F = np.asarray(F, dtype=np.complex128)
    K = len(edges)
    zone = membership(x, y, edges, centre)
    inside = zone < K
    zi = zone[inside]
    phi = phase_ld(x, y, wavelength, n_glass, reference)
    c, s = np.cos(phi)[inside], np.sin(phi)[inside]
    sets = F.shape[0]
    out = {'n': np.bincount(zi, minlength=K).astype(np.int64), 'outside': int((~inside).sum()), 'phi_max': float(np.abs(phi).max())}
    out['S'], out['S_abs'] = np.zeros((sets, K), LD), np.zeros((sets, K), LD)
    out['I'], out['E_abs'] = np.zeros((sets, K, 2), LD), np.zeros((sets, K, 2), LD)
    Cr, Ci = np.zeros((sets, K, 2), LD), np.zeros((sets, K, 2), LD)
    for m in range(sets):
        ex, ey, hx, hy = (F[m, f][inside] for f in range(4))
        r = lambda a: a.real.astype(LD)
        i = lambda a: a.imag.astype(LD)
        np.add.at(out['S'][m], zi, (r(ex) * r(hy) + i(ex) * i(hy) - r(ey) * r(hx) - i(ey) * i(hx)) / 2)
        np.add.at(out['S_abs'][m], zi, (np.abs(ex).astype(LD) * np.abs(hy) + np.abs(ey).astype(LD) * np.abs(hx)) / 2)
        for p, e in enumerate((ex, ey)):
            np.add.at(out['I'][m, :, p], zi, r(e) * r(e) + i(e) * i(e))
            np.add.at(out['E_abs'][m, :, p], zi, np.abs(e).astype(LD))
            np.add.at(Cr[m, :, p], zi, r(e) * c + i(e) * s)
            np.add.at(Ci[m, :, p], zi, i(e) * c - r(e) * s)
    out['Cr'], out['Ci'] = Cr, Ci
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
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


def ratios(got, want):
    """``got``: the dict of ``analyse`` / ``zone_metrics``; ``want``: ``exact`` of the same case -> the worst error over its
    bound for S, I and C.  The integers are asserted here."""
    assert got['samples'].dtype == np.int64 and np.array_equal(got['samples'], want['n'])
    assert got['outside'] == want['outside']
    dA, n = LD(want['dA']), want['n'].astype(LD)
    assert np.array_equal(got['area'], want['n'] * want['dA'])
    out = {'S': _ratio(np.abs(got['P'].astype(LD) - want['S'] * dA), (n + 16) * U * want['S_abs'] * dA),
           'I': _ratio(np.abs(got['I'].astype(LD) - want['I'] * dA), (n[None, :, None] + 16) * U * want['I'] * dA)}
    d = np.hypot(got['overlap'].real.astype(LD) - want['Cr'] * dA, got['overlap'].imag.astype(LD) - want['Ci'] * dA)
    out['C'] = _ratio(d, (4 * LD(want['phi_max']) + n[None, :, None] + 64) * U * want['E_abs'] * dA)
    return out


def hold(name, got, want):
    """print the PARITY line of a case and assert the bounds"""
    r = ratios(got, want)
    print('PARITY zones %-28s sets %d zones %4d  worst error / bound: S %.3f  I %.3f  C %.3f  (Phi %.3g)'
          % (name, got['P'].shape[0], want['n'].size, r['S'], r['I'], r['C'], want['phi_max']))
    assert r['S'] <= 1 and r['I'] <= 1 and r['C'] <= 1, (name, r)
    # what follows from the sums: the coherence lies in [0, 1] (Cauchy-Schwarz, to rounding) and is NaN exactly where n sum I is 0
    den = want['n'][None, :, None] * got['I']
    assert np.array_equal(np.isnan(got['coherence']), den == 0)
    ok = ~np.isnan(got['coherence'])
    # (|sum C| <= sqrt(n sum I) and sum |E| <= sqrt(n sum I): the bound of C, relative to the root, squared)
    lim = 1 + 3 * (4 * want['phi_max'] + float(want['n'].max()) + 64) * U
    assert (got['coherence'][ok] >= 0).all() and (got['coherence'][ok] <= lim).all()
    assert np.array_equal(got['phase'], np.angle(got['overlap']))
    return r


def seeded_fields(sets, nx, ny, seed):
    """(sets, 4, nx, ny) complex fields of a seeded generator, magnitudes over three decades"""
    rng = np.random.default_rng(seed)
    amp = 10.0 ** rng.uniform(-2, 1, (sets, 4, nx, ny))
    return amp * np.exp(2j * np.pi * rng.uniform(0, 1, (sets, 4, nx, ny)))


# the five seeded cases of the yardstick: name, (nx, ny), x, y, wavelength, n_glass, edges, centre, reference
def cases():
    wl, ng = 580e-9, 1.46
    p = wl / 2.2
    out = []
    x, y = (np.arange(130) - 64.5) * p, (np.arange(129) - 64) * p
    out.append(('130x129 focus 30 um', x, y, wl, ng, np.linspace(2e-6, 17e-6, 12), (0.0, 0.0), ('focus', 0.0, 0.0, 30e-6)))
    x, y = (np.arange(70) - 30.3) * p, (np.arange(257) - 100.7) * p
    e = np.sort(np.concatenate([np.linspace(1e-6, 30e-6, 30), 9e-6 + np.arange(10) * 0.04e-6]))
    out.append(('70x257 off axis', x, y, wl, ng, e, (0.37e-6, -1.21e-6), ('focus', 1.1e-6, -0.6e-6, 45e-6)))
    x = y = (np.arange(64) - 31.5) * p
    out.append(('64x64 zf -2 mm', x, y, wl, ng, np.linspace(1e-6, 10e-6, 9), (0.0, 0.0), ('focus', 0.0, 0.0, -2e-3)))
    x, y = (np.arange(90) - 44.5) * p, (np.arange(75) - 20.0) * p
    out.append(('90x75 plane (0.3, -0.2)', x, y, wl, ng, np.linspace(1e-6, 14e-6, 20), (0.2e-6, 0.1e-6), ('plane', 0.3, -0.2)))
    x, y = 1e-3 + (np.arange(66) - 30.0) * p, 1e-3 + (np.arange(130) - 64.0) * p
    out.append(('66x130 plane (0.7, 0.7)', x, y, wl, ng, np.linspace(0.5e-6, 16e-6, 25), (1e-3, 1e-3), ('plane', 0.7, 0.7)))
    return out
