"""The device arithmetic of csrc/nearfield_math.h on the host (tools/device_math.cpp), without a GPU.

sincos_cw, reduce_pio2 and sincos_cw_q are restated there operation by operation; the GPU must match the restatement
bit for bit (tests/test_gpu_device_math.py), so the restatement's accuracy is the kernels'.  Here it goes against
mpmath at 200 bits over every set of tests/device_math_cases.py.

Bound 2^-51 = 4.44e-16 on max(|s - sin x|, |c - cos x|), a budget and not a measurement: two reduction roundings of
<= 2^-53 pi/4 each, the dropped third term of pi/2 (1.5e-33 |k| < 1e-24 for |k| < 6.4e8), and <= 2^-52 for the kernel
polynomials and the final rounding.  The composite x = r + a0, kq of the centre kernels gets 2^-51 + 2^-53 |r + a0|:
the rounding of the sum.  Measured worst per set (printed as ``DEVMATH ...`` lines, run with -s):
    loguniform 1.62e-16   zeros 0   near_k_pio2 5.6e-17   near_rint_tie 1.75e-16
    kR_far 1.72e-16   kR_points 1.70e-16   kR_fan 1.71e-16   composite 9.1e-16 (0.67 of its bound)

sqrt_exact, recip and rsqrt_fast start from a hardware estimate; the tool models them from the exact value perturbed
by up to 2^-22 relative.  With that the square root equals np.sqrt on every input and the two reciprocals stay within
2^-52 relative - the conclusions the GPU test carries over by asserting that the hardware's estimates are within 2^-22."""
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import device_math_cases as dc

BOUND = 2.0 ** -51
EST_ERR = 2.0 ** -22
WORKERS = max(1, min(8, len(os.sched_getaffinity(0))))


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('device_math')) + os.sep
    return dc.Tool(dc.build_tool(out), out)


@pytest.fixture(scope='module')
def pool():
    with ProcessPoolExecutor(WORKERS) as ex:
        yield ex


def _errors(job):
    """worker: max(|s - sin X|, |c - cos X|) per element at 200 bits, X = x (+ a0, exactly) + kq pi/2"""
    pytest.importorskip('mpmath')
    from mpmath import libmp
    x, a0, kq, s, c = job
    prec = 200
    pio2 = libmp.mpf_shift(libmp.mpf_pi(prec + 40), -1)
    f, sub, to = libmp.from_float, libmp.mpf_sub, libmp.to_float
    out = np.empty(len(x))
    for i in range(len(x)):
        X = f(x[i])
        if a0 is not None:
            X = libmp.mpf_add(X, f(a0[i]))                                        # (no precision given: exact)
            X = libmp.mpf_add(X, libmp.mpf_mul_int(pio2, int(kq[i]), prec + 40), prec + 40)
        cm, sm = libmp.mpf_cos_sin(X, prec)
        out[i] = max(abs(to(sub(f(s[i]), sm, 64))), abs(to(sub(f(c[i]), cm, 64))))
    return out


def errors(pool, x, s, c, a0=None, kq=None):
    pytest.importorskip('mpmath')
    cuts = np.linspace(0, len(x), 4 * WORKERS + 1).astype(int)
    lists = [None if a is None else a.tolist() for a in (x, a0, kq, s, c)]
    jobs = [tuple(None if a is None else a[lo:hi] for a in lists) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]
    return np.concatenate(list(pool.map(_errors, jobs)))


@pytest.mark.parametrize('name', dc.SINCOS_SETS)
def test_restatement_against_mpmath(tool, pool, name):
    x = dc.sincos_set(name)
    s, c = tool.sincos(x)
    e = errors(pool, x, s, c)
    print('DEVMATH host sincos %-14s n %7d worst %.3e (bound %.3e)' % (name, x.size, e.max(), BOUND))
    assert e.max() <= BOUND
    if name == 'zeros':
        # (sin(-0) comes out as +0: k = -0, and fma(-k, pi/2, x) = (+0) + (-0) rounds to +0)
        assert np.array_equal(dc.bits(s), dc.bits(np.zeros(2))) and np.array_equal(c, [1.0, 1.0])


def test_reduce_is_the_reduction_of_sincos(tool, pool):
    """x = r + k pi/2 with |r| <= pi/4 (+ the rounding of the product that picks k), r to the reduction's part of the
    budget: |r - (x - k pi/2)| <= 2 x 2^-53 pi/4 + 1e-24, against mpmath"""
    mpmath = pytest.importorskip('mpmath')
    x = np.concatenate([dc.sincos_set(n)[:20000] for n in dc.SINCOS_SETS])
    r, k = tool.reduce(x)
    assert np.abs(r).max() <= np.pi / 4 * (1 + 2.0 ** -50) + np.abs(x).max() * 2.0 ** -52
    mpmath.mp.prec = 200
    pio2 = mpmath.pi / 2
    worst = max(abs(float(mpmath.mpf(float(ri)) - (mpmath.mpf(float(xi)) - int(ki) * pio2)))
                for xi, ri, ki in zip(x[::7], r[::7], k[::7]))
    print('DEVMATH host reduce worst |r - (x - k pi/2)| %.3e' % worst)
    assert worst <= 2 * 2.0 ** -53 * np.pi / 4 + 1e-24


def test_composite_against_mpmath(tool, pool):
    r, a0, x, kq = dc.composite(tool.reduce)
    assert set(kq.tolist()) == set(dc.KQ_VALUES) and np.abs(r).max() <= 0.7854 + 1e-6
    s, c = tool.sincos(x, kq)
    e = errors(pool, r, s, c, a0, kq)
    bound = BOUND + 2.0 ** -53 * np.abs(x)
    print('DEVMATH host sincos_q composite   n %7d worst %.3e, %.3f of its bound' % (x.size, e.max(), (e / bound).max()))
    assert (e <= bound).all()


def test_model_square_root_is_exact(tool):
    for name in dc.SQRT_SETS:
        x = dc.sqrt_set(name)
        got = tool.model('sqrt', EST_ERR, 7, x)
        bad = np.nonzero(dc.bits(got) != dc.bits(np.sqrt(x)))[0]
        print('DEVMATH host model sqrt %-10s n %7d differing %d' % (name, x.size, bad.size))
        assert bad.size == 0, (name, x[bad[:5]])


@pytest.mark.parametrize('op', ['recip', 'rsqrt'])
def test_model_reciprocals(tool, op):
    x = dc.recip_set() if op == 'recip' else dc.rsqrt_set()
    xl = x.astype(np.longdouble)
    got = tool.model(op, EST_ERR, 9, x)
    e = dc.rel_error_ld(got, 1 / xl if op == 'recip' else 1 / np.sqrt(xl))
    exact = dc.correctly_rounded_recip(x) if op == 'recip' else dc.correctly_rounded_rsqrt(x)
    print('DEVMATH host model %-5s n %7d worst rel %.3e (bound %.3e) not correctly rounded %.4f %%'
          % (op, x.size, e.max(), 2.0 ** -52, 100 * np.mean(got != exact)))
    assert e.max() <= 2.0 ** -52


def test_sanitized_tool_agrees(tool, tmp_path):
    san = dc.Tool(dc.build_tool(str(tmp_path) + os.sep, 'device_math_san'), str(tmp_path) + os.sep)
    x = np.concatenate([dc.sincos_set(n)[:3000] for n in dc.SINCOS_SETS])
    kq = np.resize(np.array(dc.KQ_VALUES, dtype=np.int32), x.size)
    for a, b in zip(san.sincos(x) + san.sincos(x, kq) + san.reduce(x), tool.sincos(x) + tool.sincos(x, kq) + tool.reduce(x)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    y = dc.sqrt_set('halfway')[:3000]
    for op in ('sqrt', 'recip', 'rsqrt'):
        assert np.array_equal(dc.bits(san.model(op, EST_ERR, 3, y)), dc.bits(tool.model(op, EST_ERR, 3, y)))
