"""Times ``PlanePropagator.focus()`` against what it replaces, on ONE resident result (needs an MI355X):

    python tools/focus_probe.py [--small-only]

* ``focus``: the pass on the GPU, host clock around ``ml_propagate_focus`` (it ends in the download of the records and a
  synchronise; ``PlanePropagator.focus()`` as a whole is timed once beside it); ``centre='peak'`` (with radii: the moments, then a pass over the radii about the peak, which reads the disc's
  rows only) and a given centre (one pass); from the fields of member 0 and from the sums; the rate is one read of the
  result over the time;
* ``download + NumPy``: ``_download(0)`` of the same result and the reductions of examples/through_focus.py extended to the
  same figures (argmax, the twelve moments, one mask per radius) - the parent's way;
* ``accumulate``: ``propagate_accumulate_kernel`` on the same buffer (``accumulate([1], reset=True)`` + synchronise), the
  streaming kernel the pass is held against: it reads the same five components per target and writes two doubles.

Cases: 8 planes of 64^2 targets at half the pitch behind 4096^2 (the README's stack, kernel spectra filled per pass), and
one plane of 4096^2 = 2^24 targets on the pitch behind 64^2 (``method='fft'``); K = 0, 8 and 32 radii.
Bytes: a target costs 80 B from fields with H (Ex, Ey, Ez, Hx, Hy: Hz enters neither |E|^2 nor Sz), 48 B without, 16 B
from the sums.  Every time is the median of 9 calls after 3 warm-up calls (the NumPy way: the better of 2)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(call, sync, reps=9, warm=3):
    for _ in range(warm):
        call()
    sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def numpy_way(p, radii, planes):
    """download the volume, reduce it on the host -> ms, (peak index, sum I) of plane 0 (to hold against focus())"""
    t0 = time.perf_counter()
    d = p._download(0)
    t1 = time.perf_counter()
    mx, my = p.x.size, p.y.size
    shape = (planes, mx, my)
    I = (np.abs(d['Ex']) ** 2 + np.abs(d['Ey']) ** 2 + np.abs(d['Ez']) ** 2).reshape(shape)
    Sz = d['Sz'].reshape(shape)
    fi, fj = np.arange(mx, dtype=float)[:, None], np.arange(my, dtype=float)[None, :]
    dx, dy = (p.x[-1] - p.x[0]) / (mx - 1), (p.y[-1] - p.y[0]) / (my - 1)
    first = enc = None
    for q in range(planes):
        flat = int(I[q].argmax())
        for w in (I[q], Sz[q]):
            sums = [w.sum(), (w * fi).sum(), (w * fj).sum(), (w * fi * fi).sum(), (w * fj * fj).sum(), (w * fi * fj).sum()]
        r2 = (dx * (fi - flat // my)) ** 2 + (dy * (fj - flat % my)) ** 2
        for R in radii:
            inside = r2 <= R * R
            enc = (I[q][inside].sum(), Sz[q][inside].sum())
        if q == 0:
            first = (flat, float(I[q].sum()))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, first, (sums, enc)


def entry(p, planes, radii, centre, source):
    """-> a call of ml_propagate_focus with everything prepared (what ``focus()`` does besides is host arithmetic on the
    records)"""
    from metalens_amd import _lib
    r = _lib.f64(radii)
    rec = np.empty((planes, 16 + 2 * r.size))
    c = None if centre is None else _lib.f64(np.tile(np.asarray(centre, dtype=float), (planes, 1)))
    dx, dy = (p.x[-1] - p.x[0]) / (p.x.size - 1), (p.y[-1] - p.y[0]) / (p.y.size - 1)
    args = (p.ctx.handle, source, p.x.size, p.y.size, planes, dx, dy, _lib.dptr(c), _lib.dptr(r) if r.size else None, r.size,
            _lib.dptr(rec), rec.shape[1])
    keep = (r, rec, c)

    def call():
        _lib.check(p.ctx.lib.ml_propagate_focus(*args))
        return keep
    return call


def probe(name, p, planes, numpy_radii=(0, 8, 32)):
    ctx = p.ctx
    T = planes * p.x.size * p.y.size
    dx = (p.x[-1] - p.x[0]) / (p.x.size - 1)
    print('== %s: %d planes of %d x %d targets, T = %d, method %r' % (name, planes, p.x.size, p.y.size, T, p.method))
    t0 = time.perf_counter()
    p.queue_sets(0, 1)
    ctx.sync()
    print('first pass (plans, fills, propagates): %.1f ms' % ((time.perf_counter() - t0) * 1e3))
    acc = median_ms(lambda: p.accumulate([1.0], reset=True), ctx.sync)
    acc_bytes = T * (80 + 16)
    print('accumulate (reads 80 B, writes 16 B per target): median %.3f ms (min %.3f max %.3f)  %.1f GB/s'
          % (acc + (acc_bytes / acc[0] * 1e-6,)))
    for K in (0, 8, 32):
        radii = (np.arange(K) + 0.5) * dx * (1 if K <= 8 else 0.25)
        for of, per_target in (('fields', 80), ('sums', 16)):
            for centre in ('peak', 'given'):
                if K == 0 and centre != 'peak':
                    continue
                ms = median_ms(entry(p, planes, radii, None if centre == 'peak' else (p.x.size // 2, p.y.size // 2),
                                     0 if of == 'fields' else -1), lambda: None)
                # one read of the plane: the second pass of centre='peak' reads the targets of the waves that meet the
                # largest radius only (here a disc of at most 8.5 targets' radius)
                gbs = T * per_target / ms[0] * 1e-6
                print('focus K = %2d of=%-6s centre=%-5s: median %.3f ms (min %.3f max %.3f)  %d B per target, %.1f GB/s, '
                      '%.2f of accumulate\'s rate' % (K, of, centre, ms[0], ms[1], ms[2], per_target, gbs,
                                                       gbs / (acc_bytes / acc[0] * 1e-6)))
        if K in numpy_radii:
            runs = [numpy_way(p, radii, planes) for _ in range(2)]
            best = min(runs, key=lambda r: r[0] + r[1])
            t0 = time.perf_counter()
            got = p.focus(radii)
            print('PlanePropagator.focus K = %2d, the whole call with its host arithmetic: %.3f ms' % (K, (time.perf_counter() - t0) * 1e3))
            dy = (p.y[-1] - p.y[0]) / (p.y.size - 1)
            print('  plane 0: peak at %s (NumPy %s), sum I %.15g (NumPy %.15g)'
                  % (tuple(got['peak_index'][0]), divmod(best[2][0], p.y.size), got['I_dA'][0] / (dx * dy), best[2][1]))
            print('download + NumPy K = %2d: download %.1f ms + reductions %.1f ms = %.1f ms (the better of 2)'
                  % (K, best[0], best[1], best[0] + best[1]))
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
    probe('plane 4096^2 on the pitch behind 64^2', p, 1, numpy_radii=(8,))


if __name__ == '__main__':
    main()
