"""Arguments for the device arithmetic of csrc/nearfield_math.h, shared by tests/test_device_math_host.py (the host
restatement against mpmath) and tests/test_gpu_device_math.py (the GPU against the restatement and exact references).
Test infrastructure; everything is generated from fixed seeds, nothing is stored, every set holds at most 2^20 values.

The ranges are the documented ones: |x| <= 1e9 for the sincos family (|k| < 6.4e8 quadrants), 1e-200 < x < 1e200 for
the square root, the reciprocal and the reciprocal root."""
import functools

import numpy as np

X_MAX = 1e9                  # the contract of sincos_cw / reduce_pio2 (common.h PHASE_LIMIT)
K_MAX = 630_000_000          # quadrants: K_MAX pi/2 + a few ulp stays below X_MAX
N_K = 1 << 17                # multiples of pi/2 whose neighbourhoods are visited
# pi/2 to 60 decimal places, as an integer over 2^200 (correct to 2^-198; a double has 53 bits)
_PIO2_DIGITS = '1.570796326794896619231321691639751442098584699687552910487472'
_SHIFT = 200


def _pio2_scaled():
    from fractions import Fraction
    return int(Fraction(_PIO2_DIGITS) * (1 << _SHIFT))


def _ulp_neighbours(c, reach=2):
    """the doubles c - reach ulp ... c + reach ulp around every (positive or negative, non-zero) c"""
    out = [c]
    lo = hi = c
    for _ in range(reach):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def _multiples(odd_halves):
    """the doubles nearest k pi/2 (or (k + 1/2) pi/2) for N_K values of k, log-uniform in 1 ... K_MAX with K_MAX itself
    and 1 among them, both signs, and their +-1, +-2 ulp neighbours"""
    rng = np.random.default_rng(20 + odd_halves)
    k = np.unique(np.concatenate([[1, 2, 3, K_MAX, K_MAX - 1],
                                  np.floor(np.exp(rng.uniform(0, np.log(K_MAX), N_K // 2))).astype(np.int64)]))
    more = np.setdiff1d(rng.integers(1, K_MAX, N_K), k)          # (half log-uniform, topped up uniformly to N_K)
    k = np.concatenate([k, more[:N_K - k.size]])
    assert k.size == N_K and np.unique(k).size == N_K
    P = _pio2_scaled()
    if odd_halves:
        c = np.array([((2 * int(v) + 1) * P) / (1 << (_SHIFT + 1)) for v in k])   # int / int: correctly rounded
    else:
        c = np.array([(int(v) * P) / (1 << _SHIFT) for v in k])
    c *= np.where(rng.integers(0, 2, c.size) == 1, -1.0, 1.0)
    x = _ulp_neighbours(c)
    assert np.abs(x).max() < X_MAX and x.size <= 1 << 20
    return x


def _propagator_pairs(name):
    """-> R^2 and k R of (a fixed sample of 2^18 of) the (aperture sample, target) pairs the direct propagator forms for
    the `far` and `points` target sets of tests/test_gpu_propagate.py (96 x 80 aperture) and for the 9 x 9 fan at 1 m of
    its far-limit test, in the kernel's order of operations up to contraction"""
    import propagate_ref as ref
    k = 2.0 * np.pi * ref.N_GLASS / ref.WL
    if name == 'fan':
        _, x, beam = ref.tilted_gaussian()
        y = x
        pts, _ = ref.fan_points(*ref.fan(beam), 1.0)
    else:
        from test_gpu_fft_mixed import _axes
        from test_gpu_propagate import _points, _target_set
        x, y = _axes(96, 80)
        pts = _points(*_target_set(name, x, y))
    rng = np.random.default_rng({'far': 31, 'points': 32, 'fan': 33}[name])
    n = 1 << 18
    i, j, t = rng.integers(0, x.size, n), rng.integers(0, y.size, n), rng.integers(0, len(pts), n)
    dxp, dyp = x[1] - x[0], y[1] - y[0]
    dx = (pts[t, 0] - x[0]) - i * dxp
    dy = (pts[t, 1] - y[0]) - j * dyp
    R2 = dy * dy + (dx * dx + pts[t, 2] * pts[t, 2])
    return R2, k * np.sqrt(R2)


def _scaled_randoms(seed, n, signed):
    """random mantissas in [1, 2) times 2^e with 2^e over 1e-200 ... 1e200"""
    rng = np.random.default_rng(seed)
    m = 1.0 + rng.integers(0, 1 << 52, n).astype(np.float64) * 2.0 ** -52
    x = np.ldexp(m, rng.integers(-664, 664, n))          # 2^-664 = 1.3e-200, 2^664 = 7.7e199
    assert x.min() > 1e-200 and x.max() < 1e200
    return x * np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0) if signed else x


@functools.lru_cache(maxsize=None)
def sincos_set(name):
    """the arguments of one sincos set (SINCOS and REDUCE take all of them)"""
    if name == 'loguniform':     # log-uniform |x| in [2^-60, 1e9], both signs
        rng = np.random.default_rng(11)
        x = np.exp(rng.uniform(np.log(2.0 ** -60), np.log(X_MAX), 1 << 18))
        x = np.concatenate([x, [2.0 ** -60, X_MAX]])
        return x * np.where(rng.integers(0, 2, x.size) == 1, -1.0, 1.0)
    if name == 'zeros':
        return np.array([0.0, -0.0])
    if name == 'near_k_pio2':    # worst cancellation: the remainder is a few ulp of x
        return _multiples(0)
    if name == 'near_rint_tie':  # where rint(x 2/pi) changes and |r| = pi/4
        return _multiples(1)
    return _propagator_pairs(name[3:])[1]     # 'kR_far', 'kR_points', 'kR_fan'


SINCOS_SETS = ('loguniform', 'zeros', 'near_k_pio2', 'near_rint_tie', 'kR_far', 'kR_points', 'kR_fan')

KQ_VALUES = tuple(range(-4, 8))


def composite(reduce):
    """what the centre kernels give sincos_cw_q: x = r + a0 with r the remainder `reduce` returns (x -> r, k: the
    restatement's or the GPU's reduce_pio2) for large angles k_vac |r|, a0 uniform in [-8, 8], and every kq of
    KQ_VALUES in turn  ->  r, a0, x, kq (int32)"""
    rng = np.random.default_rng(41)
    n = 12 * (1 << 14)
    big = np.exp(rng.uniform(np.log(1e2), np.log(X_MAX), n))
    big[:4096] = sincos_set('near_rint_tie')[:4096]          # remainders at the ends of [-pi/4, pi/4] too
    r, _ = reduce(big)
    a0 = rng.uniform(-8.0, 8.0, n)
    a0[::97] = 0.0
    kq = np.resize(np.array(KQ_VALUES, dtype=np.int32), n)
    return r, a0, r + a0, kq


@functools.lru_cache(maxsize=None)
def sqrt_set(name):
    if name == 'random':
        return _scaled_randoms(51, 1 << 18, False)
    if name == 'squares':        # exact squares of 26-bit numbers (a 52-bit product) and their +-1 ulp neighbours
        rng = np.random.default_rng(52)
        m = rng.integers(1 << 25, 1 << 26, 1 << 17).astype(np.float64)
        m[:2] = [1 << 25, (1 << 26) - 1]
        sq = m * m
        assert np.array_equal(np.sqrt(sq), m)
        return _ulp_neighbours(sq * np.ldexp(1.0, 2 * rng.integers(-300, 300, sq.size)), 1)
    if name == 'halfway':        # (m + ulp / 2)^2 rounded, and its neighbours: the root lies beside a rounding boundary
        rng = np.random.default_rng(53)
        M = rng.integers(1 << 52, 1 << 53, 1 << 16)
        sq = np.array([float((2 * int(v) + 1) ** 2) for v in M])      # int -> float: correctly rounded
        return _ulp_neighbours(sq * np.ldexp(1.0, -106 + 2 * rng.integers(-300, 300, sq.size)))
    return _propagator_pairs(name[3:])[0]     # 'R2_far', 'R2_points', 'R2_fan'


SQRT_SETS = ('random', 'squares', 'halfway', 'R2_far', 'R2_points', 'R2_fan')


@functools.lru_cache(maxsize=None)
def recip_set():
    """recip and the bare reciprocal estimate: both signs"""
    return _scaled_randoms(61, 1 << 18, True)


@functools.lru_cache(maxsize=None)
def rsqrt_set():
    return _scaled_randoms(62, 1 << 18, False)


# ---- the host tool (tools/device_math.cpp) ----

def build_tool(out_dir, name='device_math'):
    """make the tool in out_dir (with a trailing separator) -> its path"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(['make', '-s', '-C', os.path.join(root, 'tools'), 'OUT=' + out_dir, out_dir + name])
    return out_dir + name


class Tool:
    """the restatement and the model through files in `work`"""

    def __init__(self, path, work):
        self.path, self.work = path, work

    def _run(self, *args):
        import subprocess
        res = subprocess.run([self.path] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr

    def _put(self, name, a, dtype):
        p = self.work + name
        np.ascontiguousarray(a, dtype=dtype).tofile(p)
        return p

    def sincos(self, x, kq=None):
        px, po = self._put('x.bin', x, np.float64), self.work + 'out.bin'
        if kq is None:
            self._run('sincos', px, po)
        else:
            self._run('sincos_q', px, self._put('kq.bin', kq, np.int32), po)
        out = np.fromfile(po, dtype=np.float64)
        assert out.size == 2 * len(x)
        return out[:len(x)], out[len(x):]

    def reduce(self, x):
        px, po = self._put('x.bin', x, np.float64), self.work + 'out.bin'
        self._run('reduce', px, po)
        raw = np.fromfile(po, dtype=np.uint8)
        n = len(x)
        assert raw.size == 12 * n
        return raw[:8 * n].view(np.float64).copy(), raw[8 * n:].view(np.int32).copy()

    def model(self, op, eps, seed, x):
        px, po = self._put('x.bin', x, np.float64), self.work + 'out.bin'
        self._run('model', op, repr(float(eps)), seed, px, po)
        out = np.fromfile(po, dtype=np.float64)
        assert out.size == len(x)
        return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rel_error_ld(got, exact_ld):
    """|got - exact| / |exact| in long double (64-bit mantissa on x86: 2^-64, far below the 2^-52 ... 2^-22 judged)"""
    return np.abs((got.astype(np.longdouble) - exact_ld) / exact_ld).astype(np.float64)


def _settle_ties(x, exact_ld, exact_one):
    """exact_ld rounded to double, with the few results whose long-double value sits within 2^-8 ulp of a double
    rounding boundary (where rounding twice can differ from rounding once) recomputed by `exact_one` in integers"""
    d = exact_ld.astype(np.float64)
    ulp = np.spacing(np.abs(d)).astype(np.longdouble)
    off = np.abs(np.abs(exact_ld - d.astype(np.longdouble)) / ulp - 0.5)
    for i in np.nonzero(off < 2.0 ** -8)[0]:
        d[i] = exact_one(float(x[i]))
    return d


def _recip_one(v):
    from fractions import Fraction
    f = 1 / Fraction(v)
    return f.numerator / f.denominator            # int / int: correctly rounded


def _rsqrt_one(v):
    import math
    from fractions import Fraction
    f = 1 / Fraction(v)                           # 1 / sqrt(v) = sqrt(f); 400 fraction bits settle any double
    root = math.isqrt((f.numerator << 800) // f.denominator)
    return root / (1 << 400)


def correctly_rounded_recip(x):
    return _settle_ties(x, 1 / x.astype(np.longdouble), _recip_one)


def correctly_rounded_rsqrt(x):
    return _settle_ties(x, 1 / np.sqrt(x.astype(np.longdouble)), _rsqrt_one)
