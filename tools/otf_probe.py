"""Times ``PlanePropagator.otf()`` against what it replaces, on ONE resident result (needs an MI355X):

    python tools/otf_probe.py [--small-only]

* ``otf``: the three launches on the GPU, host clock around ``ml_propagate_otf`` (it ends in the download of the entries and a
  synchronise; ``PlanePropagator.otf()`` as a whole is timed once beside it), at (nu, nv) = (1, 1), (64, 1), (1, 64), (8, 8)
  and (64, 64), from the fields of member 0 and from the sums; the rate is one read of the result over the time;
* ``download + NumPy``: ``_download(0)`` of the same result, the weights and the same separable contraction as two matrix
  products per plane and weight - the parent's way;
* ``accumulate``: ``propagate_accumulate_kernel`` on the same buffer (``accumulate([1], reset=True)`` + synchronise), the
  streaming kernel the pass is held against: it reads the same five components per target and writes two doubles.

Cases: 8 planes of 64^2 targets at half the pitch behind 4096^2 (the README's stack, kernel spectra filled per pass), and
one plane of 4096^2 = 2^24 targets on the pitch behind 64^2 (``method='fft'``).
Bytes: a target costs 80 B from fields with H (Ex, Ey, Ez, Hx, Hy: Hz enters neither |E|^2 nor Sz) and 16 B from the sums.
Every time is the median of 9 calls after 3 warm-up calls (the NumPy way: the better of 2)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from focus_probe import median_ms  # noqa: E402

SHAPES = ((1, 1), (64, 1), (1, 64), (8, 8), (64, 64))


def freqs(n):
    """n frequencies in cycles per sample, 0 first, the rest spread to Nyquist"""
    return np.linspace(0.0, 0.5, n)


def numpy_way(p, u, v, planes):
    """download the volume, contract it on the host -> download ms, arithmetic ms, O_I of plane 0"""
    t0 = time.perf_counter()
    d = p._download(0)
    t1 = time.perf_counter()
    mx, my = p.x.size, p.y.size
    shape = (planes, mx, my)
    I = (np.abs(d['Ex']) ** 2 + np.abs(d['Ey']) ** 2 + np.abs(d['Ez']) ** 2).reshape(shape)
    Sz = d['Sz'].reshape(shape)
    tx = np.exp(-2j * np.pi * np.outer(u, np.arange(mx)))
    ty = np.exp(-2j * np.pi * np.outer(np.arange(my), v))
    first = None
    for q in range(planes):
        for w in (I[q], Sz[q]):
            O = tx @ (w @ ty)
            if first is None:
                first = O
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, first


def entry(p, planes, u, v, source):
    """-> a call of ml_propagate_otf with everything prepared (what ``otf()`` does besides is host arithmetic on the entries)"""
    from metalens_amd import _lib
    u, v = _lib.f64(u), _lib.f64(v)
    out = np.empty((planes, 2, u.size, v.size), dtype=np.complex128)
    args = (p.ctx.handle, source, p.x.size, p.y.size, planes, _lib.dptr(u), u.size, _lib.dptr(v), v.size, _lib.dptr(out))

    def call():
        _lib.check(p.ctx.lib.ml_propagate_otf(*args))
        return out
    return call


def probe(name, p, planes, numpy_shapes=SHAPES):
    ctx = p.ctx
    T = planes * p.x.size * p.y.size
    dx, dy = (p.x[-1] - p.x[0]) / (p.x.size - 1), (p.y[-1] - p.y[0]) / (p.y.size - 1)
    print('== %s: %d planes of %d x %d targets, T = %d, method %r' % (name, planes, p.x.size, p.y.size, T, p.method))
    t0 = time.perf_counter()
    p.queue_sets(0, 1)
    ctx.sync()
    print('first pass (plans, fills, propagates): %.1f ms' % ((time.perf_counter() - t0) * 1e3))
    acc = median_ms(lambda: p.accumulate([1.0], reset=True), ctx.sync)
    acc_rate = T * (80 + 16) / acc[0] * 1e-6
    print('accumulate (reads 80 B, writes 16 B per target): median %.3f ms (min %.3f max %.3f)  %.1f GB/s' % (acc + (acc_rate,)))
    for nu, nv in SHAPES:
        u, v = freqs(nu), freqs(nv)
        for of, per_target in (('fields', 80), ('sums', 16)):
            call = entry(p, planes, u, v, 0 if of == 'fields' else -1)
            ms = median_ms(call, lambda: None)
            gbs = T * per_target / ms[0] * 1e-6
            print('otf %2d x %2d of=%-6s: median %.3f ms (min %.3f max %.3f)  %d B per target, %.1f GB/s, %.2f of accumulate\'s rate'
                  % (nu, nv, of, ms[0], ms[1], ms[2], per_target, gbs, gbs / acc_rate))
        if (nu, nv) in numpy_shapes:
            runs = [numpy_way(p, u, v, planes) for _ in range(2)]
            best = min(runs, key=lambda r: r[0] + r[1])
            t0 = time.perf_counter()
            got = p.otf(u / dx, v / dy)
            print('PlanePropagator.otf %2d x %2d, the whole call with its host arithmetic: %.3f ms' % (nu, nv, (time.perf_counter() - t0) * 1e3))
            print('  plane 0: largest |otf_I - NumPy| / otf_I(0, 0) = %.2e'
                  % (np.abs(got['otf_I'][0] / (dx * dy) - best[2]).max() / abs(best[2][0, 0])))
            print('download + NumPy %2d x %2d: download %.1f ms + contraction %.1f ms = %.1f ms (the better of 2)'
                  % (nu, nv, best[0], best[1], best[0] + best[1]))
    sys.stdout.flush()


def main():
    import metalens_amd as ma
    from metalens_amd import _lib
    wl, n_glass = 580e-9, 1.46
    k, Z = 2 * np.pi * n_glass / wl, ma.constants.Z0 / n_glass
    ctx = _lib.default_context()
    print(ctx.device_info())

    def upload(n):
        x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
        a = x.max()
        f = a / np.tan(np.arcsin(0.5))
        r2 = x[:, None] ** 2 + x[None, :] ** 2
        Ex = np.where(r2 <= a * a, np.exp(-1j * k * np.sqrt(r2 + f * f)), 0)
        zero = np.zeros_like(Ex)
        _lib.check(ctx.lib.ml_fields_upload(ctx.handle, n, n, *[_lib.dptr(_lib.c128(v)) for v in (Ex, zero, zero, Ex / Z)]))
        ctx.fields_owner = None
        return x, f

    x, f = upload(4096)
    d = x[1] - x[0]
    t = (np.arange(64) - 31.5) * d / 2 + d / 4
    z = f + np.linspace(-3, 3, 8) * wl / n_glass
    p = ma.PlanePropagator(x, x, wl, n_glass, t, t, z, method='fft-stack', subsample=(2, 2), cache_kernels=False, ctx=ctx)
    probe('stack 8 x 64^2 at half the pitch behind 4096^2', p, 8)
    if '--small-only' in sys.argv:
        return
    x, f = upload(64)
    d = x[1] - x[0]
    t = x[0] + d / 2 + (np.arange(4096) - 2048) * d
    p = ma.PlanePropagator(x, x, wl, n_glass, t, t, 40 * f, method='fft', ctx=ctx)
    probe('plane 4096^2 on the pitch behind 64^2', p, 1, numpy_shapes=((1, 1), (8, 8), (64, 64)))


if __name__ == '__main__':
    main()
