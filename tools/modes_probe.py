"""Times the mode overlaps of a resident image (``ml_propagate_modes_queue``) against what they replace and what they stand
beside, on ONE resident result (needs an MI355X):

    python tools/modes_probe.py [--small-only]

* ``modes``: warm batches of ``ml_propagate_modes_queue`` - BATCH calls into slot 0, then one synchronise; the time per call -
  at (nu, nv) = (1, 1), (8, 8), (64, 1), (1, 64) and (64, 64); the rate is one read of the four components over the time;
* ``accumulate``: ``propagate_accumulate_kernel`` on the same buffer, the streaming kernel the pass is held against: it
  reads 80 B and writes 16 B per target where the mode pass reads 64 B;
* ``otf``: ``ml_propagate_otf`` at the same counts (it ends in a download of its entries and a synchronise);
* ``download + NumPy``: ``_download(0)`` of the same result and ``postprocess.mode_overlaps`` - the parent's way;
* a sweep step with ``image_modes`` against the same step without it.

Cases: one plane of 4096^2 = 2^24 targets on the pitch behind 64^2 (``method='fft'``) and 8 planes of 64^2 targets at half the
pitch behind 4096^2 (the README's stack).  Every time is the median of 9 after 3 warm-up runs (the NumPy way: one run)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from focus_probe import median_ms  # noqa: E402

SHAPES = ((1, 1), (8, 8), (64, 1), (1, 64), (64, 64))
BATCH = 8


def tables(p, nu, nv):
    """nu x nv Gaussian modes on a grid of centres across the patch, waist an eighth of it"""
    import metalens_amd as ma
    wl, n = p._geometry[4], p._geometry[5]
    out = []
    for t, count in ((p.x, nu), (p.y, nv)):
        span = t[-1] - t[0]
        centres = t[0] + span * (np.arange(count) + 0.5) / count
        out.append(np.array([ma.gaussian_axis(t, span / 8, centre=c, wavelength=wl, n=n) for c in centres]))
    return out


def probe(name, p, planes, numpy_shapes):
    from metalens_amd import _lib
    import metalens_amd as ma
    ctx = p.ctx
    T = planes * p.x.size * p.y.size
    Z = p.Z0 / p._geometry[5]
    print('== %s: %d planes of %d x %d targets, T = %d, method %r' % (name, planes, p.x.size, p.y.size, T, p.method))
    t0 = time.perf_counter()
    p.queue_sets(0, 1)
    ctx.sync()
    print('first pass (plans, fills, propagates): %.1f ms' % ((time.perf_counter() - t0) * 1e3))
    acc = median_ms(lambda: p.accumulate([1.0], reset=True), ctx.sync)
    acc_rate = T * (80 + 16) / acc[0] * 1e-6
    print('accumulate (reads 80 B, writes 16 B per target): median %.3f ms (min %.3f max %.3f)  %.1f GB/s' % (acc + (acc_rate,)))
    for nu, nv in SHAPES:
        A, B = tables(p, nu, nv)
        tx, ty = _lib.c128(A), _lib.c128(B)
        t0 = time.perf_counter()
        p._modes_plan(tx, ty, planes, 1)
        plan_ms = (time.perf_counter() - t0) * 1e3

        def batch():
            for _ in range(BATCH):
                _lib.check(ctx.lib.ml_propagate_modes_queue(ctx.handle, 0, 0))
        ms = [v / BATCH for v in median_ms(batch, ctx.sync)]
        gbs = T * 64 / ms[0] * 1e-6
        flops = T * 4 * nv * 8 / ms[0] * 1e-9          # the row pass: 4 components, 8 operations per complex multiply-add
        print('modes %2d x %2d: per call median %.3f ms (min %.3f max %.3f) in batches of %d; plan %.2f ms; 64 B per target %.1f GB/s, %.2f of '
              'accumulate\'s rate; row pass %.2f Tflop/s' % (nu, nv, ms[0], ms[1], ms[2], BATCH, plan_ms, gbs, gbs / acc_rate, flops))
        u, v = _lib.f64(np.linspace(0.0, 0.5, nu)), _lib.f64(np.linspace(0.0, 0.5, nv))
        out = np.empty((planes, 2, nu, nv), dtype=np.complex128)
        otf = median_ms(lambda: _lib.check(ctx.lib.ml_propagate_otf(ctx.handle, 0, p.x.size, p.y.size, planes, _lib.dptr(u), nu, _lib.dptr(v),
                                                                    nv, _lib.dptr(out))), lambda: None)
        print('otf   %2d x %2d: median %.3f ms (min %.3f max %.3f)' % ((nu, nv) + otf))
        if (nu, nv) in numpy_shapes:
            t0 = time.perf_counter()
            got = p.overlap(A, B)
            whole = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            d = p._download(0)
            t1 = time.perf_counter()
            twin = ma.mode_overlaps(d, p.x, p.y, A, B, Z)
            t2 = time.perf_counter()
            scale = np.abs(twin['overlap_Ex']).max()
            print('PlanePropagator.overlap %2d x %2d, the whole call (plan, queue, fetch, focus for the power): %.3f ms' % (nu, nv, whole))
            print('download + NumPy %2d x %2d: download %.1f ms + mode_overlaps %.1f ms = %.1f ms; largest |overlap_Ex - NumPy| / max %.2e'
                  % (nu, nv, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, np.abs(got['overlap_Ex'] - twin['overlap_Ex']).max() / scale))
    sys.stdout.flush()


def sweep_step(ctx):
    """a sweep over 6 emitter positions with and without ``image_modes`` on a synthetic lens of 20 um radius"""
    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    wl = 580e-9
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design, radius=20e-6,
                               numerical_aperture=0.3, wavelength=wl, switch_angle=np.deg2rad(8.0), num_gratings=8, num_entries=8)
    f = lens['source_distance']
    args = (wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'])
    x, y, _, n_glass = ma.build_nearfield(0.0, 0.0, -f, 'x', *args, download=False, ctx=ctx)[4:8]
    u = np.linspace(-0.1, 0.1, 16)
    sw = ma.SourceSweep(*args, x, y, u, u, ctx=ctx)
    tx, ty = x[0] + np.arange(len(x)) * (x[1] - x[0]), y[0] + np.arange(len(y)) * (y[1] - y[0])          # on the pitch
    p = ma.PlanePropagator(x, y, wl, n_glass, tx, ty, 30e-6, method='fft', ctx=ctx)
    sources = [(d, 0.0, -f, 'x') for d in np.linspace(0.0, 1e-6, 6)]
    A, B = tables(p, 8, 8)
    for label, more in (('without image_modes', {}), ('with image_modes 8 x 8', dict(image_modes=(A, B))), ('without image_modes', {}),
                        ('with image_modes 8 x 8', dict(image_modes=(A, B)))):
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            sw.run(sources, image=p, **more)
            times.append((time.perf_counter() - t0) * 1e3)
        print('sweep of %d sources on %d x %d samples, image %d x %d, %s: median %.2f ms (min %.2f), %.3f ms per source'
              % (len(sources), x.size, y.size, p.x.size, p.y.size, label, np.median(times), min(times), np.median(times) / len(sources)))


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
    probe('stack 8 x 64^2 at half the pitch behind 4096^2', p, 8, numpy_shapes=((1, 1), (64, 64)))
    sweep_step(ctx)
    if '--small-only' in sys.argv:
        return
    x, f = upload(64)
    d = x[1] - x[0]
    t = x[0] + d / 2 + (np.arange(4096) - 2048) * d
    p = ma.PlanePropagator(x, x, wl, n_glass, t, t, 40 * f, method='fft', ctx=ctx)
    probe('plane 4096^2 on the pitch behind 64^2', p, 1, numpy_shapes=((8, 8),))


if __name__ == '__main__':
    main()
