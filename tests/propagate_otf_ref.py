"""The transfer function of a propagated image (metalens_amd/csrc/propagate_otf.hip, ml_propagate_otf) restated from
downloaded arrays: the yardstick of tests/test_gpu_propagate_otf.py and tests/test_propagate_otf_host.py.

    O_w[a][b] = sum_i sum_j w(i, j) exp(-2 pi i (u[a] i + v[b] j))

The weights come from ``propagate_focus_ref.weights`` (the kernel's order of operations).  The fraction of ``u i + v j`` is
exact: ``fractions.Fraction`` of the doubles gives every frequency as an integer over a power of two, the phase is integer
arithmetic modulo that power, and the fraction in [-1/2, 1/2) is rounded to a double once (the integers are held in int64
where 2^61 holds them, in Python's integers otherwise - the same numbers).  The terms are ``w cos`` and ``-w sin`` of
``2 pi float(fraction)``, with the quarter turns taken off the exact fraction first (``cos_sin``): in doubles cos and sin
of a rounded pi / 2 or pi are 6e-17 and 1.2e-16 where the exact phasor has 0, and at an entry whose frequencies are all 0
or Nyquist such terms would be the whole imaginary part - noise whose sum |term| is no scale for anybody's error.  Every
sum is ``math.fsum`` - correctly rounded, so what a comparison shows is the GPU's arithmetic.  Beside each value stands ``sum |term|`` (for Sz from fields with the ``scale`` of ``weights`` in place of |Sz|).

Bound of an entry, each of re and im: ``(n + 96) u sum |term|`` with ``n = mx my`` and ``u = 2^-53`` - n for a sum in any
order, 16 for forming the weight, 2 x 16 for the two phasors, <= 8 for their product and the product with w, <= 8 for the
yardstick's own cos / sin, rounded up; ``n + 80`` from the sums, whose stored doubles are the weights."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
FREQ_MAX, SEGMENT = 64, 32        # csrc/propagate_otf.h
TILE, FEW, ROWS_MANY, BATCH = 1024, 8, 4, 16


def _last(n, tile):
    """n indices in tiles of ``tile``: -> tiles, segments of the last tile, indices of its last segment"""
    tiles = -(-n // tile)
    last = n - (tiles - 1) * tile
    segments = -(-last // SEGMENT)
    return tiles, segments, last - (segments - 1) * SEGMENT


def plan(mx, my, nv):
    """the launch shapes of the row and the column pass (otf_rows_shape, otf_columns_shape): what ``propagate_otf_plan shape``
    prints"""
    rows = 1 if nv <= FEW else ROWS_MANY
    tile = TILE // rows
    tiles, last_segments, last_segment = _last(my, tile)
    groups = -(-mx // rows)
    col_tiles, col_last_segments, col_last_segment = _last(mx, TILE)
    return dict(rows=rows, tile=tile, tiles=tiles, batch=BATCH if rows == 1 else 2 * BATCH, last_segments=last_segments,
                last_segment=last_segment, groups=groups, last_rows=mx - (groups - 1) * rows, col_tile=TILE, col_tiles=col_tiles,
                col_last_segments=col_last_segments, col_last_segment=col_last_segment)


def _over_power_of_two(freqs):
    """-> integers N, E with freqs[a] = N[a] / 2^E exactly"""
    fr = [Fraction(float(f)) for f in freqs]
    E = max(f.denominator.bit_length() - 1 for f in fr)
    return [f.numerator * ((1 << E) // f.denominator) for f in fr], E


def exact_fraction(u, i):
    """the fraction of u i in [-1/2, 1/2], exactly, as a Fraction (a tie goes to -1/2)"""
    x = Fraction(float(u)) * int(i)
    f = x - math.floor(x)
    return f - 1 if f >= Fraction(1, 2) else f


def _phase_ints(u, v, mx, my):
    """-> N (nu, nv, mx, my), E: the fraction of u[a] i + v[b] j in [-1/2, 1/2) is N / 2^E exactly (int64 where 2^61 holds
    the numerators, Python's integers otherwise - the same numbers); E >= 2"""
    (nu_, Eu), (nv_, Ev) = _over_power_of_two(u), _over_power_of_two(v)
    E = max(Eu, Ev, 2)
    D = 1 << E
    kind = np.int64 if E <= 61 else object
    nx = np.array([[(n << (E - Eu)) * i % D for i in range(mx)] for n in nu_], dtype=kind)
    ny = np.array([[(n << (E - Ev)) * j % D for j in range(my)] for n in nv_], dtype=kind)
    n = (nx[:, None, :, None] + ny[None, :, None, :]) % D
    return n - (n >= D // 2).astype(kind) * D, E


def _to_float(n, E):
    """N / 2^E rounded once: int64 -> double rounds to nearest and the scaling is exact; int / int is correctly rounded"""
    if n.dtype == object:
        return (n / (1 << E)).astype(np.float64)
    return np.ldexp(n.astype(np.float64), -E)


def fractions(u, v, mx, my):
    """-> float array (nu, nv, mx, my): the fraction of u[a] i + v[b] j in [-1/2, 1/2), the exact one rounded once"""
    return _to_float(*_phase_ints(u, v, mx, my))


def cos_sin(u, v, mx, my):
    """-> cos, sin of 2 pi frac(u[a] i + v[b] j), arrays (nu, nv, mx, my): the exact fraction is split into quarter turns and
    a rest of at most 1/8, exactly; the rest is rounded once, and cos / sin of 2 pi float(rest) are turned by the
    quarters - so a fraction of 0, +-1/4, +-1/2 gives exactly 0 or +-1, as the exact phasor is, and not cos / sin of a
    rounded pi"""
    n, E = _phase_ints(u, v, mx, my)
    D = 1 << E
    q = (4 * n + D // 2) // D
    theta = 2 * np.pi * _to_float(n - q * (D // 4), E)
    c0, s0 = np.cos(theta), np.sin(theta)
    q = (q % 4).astype(np.int64)
    c = np.choose(q, [c0, -s0, -c0, s0])
    s = np.choose(q, [s0, c0, -s0, -c0])
    return c + 0.0, s + 0.0          # (-0.0 -> 0.0)


def _fsum(a):
    """fsum over the last two axes of (nu, nv, mx, my)"""
    flat = a.reshape(a.shape[0], a.shape[1], -1)
    return np.array([[math.fsum(flat[p, q].tolist()) for q in range(flat.shape[1])] for p in range(flat.shape[0])])


def otf(I, Sz, u, v, scale=None):
    """one plane (2-D arrays; Sz may be None) -> {'I': (O, abs_re, abs_im), 'Sz': ...}: O complex (nu, nv), the sums of
    |w cos| and |w sin| beside it (for Sz with ``scale`` in place of |Sz| where given)"""
    I = np.asarray(I, dtype=float)
    c, s = cos_sin(u, v, *I.shape)
    out = {}
    for name, w, mag in (('I', I, np.abs(I)), ('Sz', Sz, None if Sz is None else (np.abs(Sz) if scale is None else scale))):
        if w is None:
            continue
        out[name] = (_fsum(w * c) + 1j * _fsum(-(w * s)), _fsum(mag * np.abs(c)), _fsum(mag * np.abs(s)))
    return out


def phasor(u, i):
    """-> sin, cos of 2 pi frac(u i) with the exact fraction, in long double arithmetic (64-bit significand: the values are
    good to 2^-62, far inside the 16 x 2^-53 the device is held to); u, i arrays"""
    assert np.finfo(np.longdouble).nmant >= 63
    hi, lo = np.empty(len(u)), np.empty(len(u))
    for k, (uu, ii) in enumerate(zip(u, i)):
        f = exact_fraction(uu, ii)
        hi[k] = float(f)
        lo[k] = float(f - Fraction(hi[k]))
    angle = (hi.astype(np.longdouble) + lo.astype(np.longdouble)) * TWO_PI_LD
    return np.sin(angle), np.cos(angle)


# 2 pi to 64 bits: 4 atan(1) x 2 in long double
TWO_PI_LD = np.longdouble(8) * np.arctan(np.longdouble(1))
