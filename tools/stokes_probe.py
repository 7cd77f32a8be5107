"""Times ``PlanePropagator.stokes()`` and ``accumulate_stokes()`` against the existing code's numbers, in one process and on
the same resident buffers (needs an MI355X):

    python tools/stokes_probe.py [--small-only]

* ``stokes``: host clock around ``ml_propagate_stokes`` (it ends in the download of the records and a synchronise), with 0 and
  8 radii about a given centre, and - what ``stokes(centre='peak')`` does - a call without radii for the peak followed by one
  with the radii about it; from the fields of member 0 and from the Stokes sums;
* ``focus``: ``ml_propagate_focus`` with the same radii and centres on the same result (tools/focus_probe.py) - the existing
  pass it is the sibling of;
* ``accumulate`` / ``accumulate_stokes``: ``propagate_accumulate_kernel`` and ``stokes_accumulate_kernel`` on the same sets
  (+ synchronise), for one set and, behind a small lens, for the three sets of an emitter's x, y and z dipoles;
* ``download + NumPy``: ``_download(0)`` of the same result and ``postprocess.stokes_metrics`` on it - the parent's way.

Cases: 8 planes of 64^2 targets at half the pitch behind 4096^2 (the README's stack), one plane of 4096^2 = 2^24 targets on
the pitch behind 64^2 (``method='fft'``, with H), and one plane of 1024^2 behind a synthetic lens with three field sets.
Bytes: the Stokes pass reads Ex, Ey, Ez, 48 B per target, where focus() reads 80 B with H (Hz enters nothing) and 48 B without;
40 B from the Stokes sums against 16 B from the sums.  Every time is the median of 9 calls after 3 warm-up calls (the NumPy way:
once)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from focus_probe import entry as focus_entry, median_ms          # noqa: E402


def stokes_entry(p, planes, radii, centre, source):
    """-> a call of ml_propagate_stokes with everything prepared; centre 'peak': the two calls of ``stokes(centre='peak')``"""
    from metalens_amd import _lib
    r = _lib.f64(radii)
    lib, h = p.ctx.lib, p.ctx.handle
    dx, dy = (p.x[-1] - p.x[0]) / (p.x.size - 1), (p.y[-1] - p.y[0]) / (p.y.size - 1)
    head, rec = np.empty((planes, 9)), np.empty((planes, 9 + 5 * r.size))
    given = None if centre == 'peak' else _lib.f64(np.tile(np.asarray(centre, dtype=float), (planes, 1)))

    def call():
        c = given
        if c is None and r.size:
            _lib.check(lib.ml_propagate_stokes(h, source, p.x.size, p.y.size, planes, dx, dy, None, None, 0, _lib.dptr(head), 9))
            c = _lib.f64(head[:, 7:9])
        _lib.check(lib.ml_propagate_stokes(h, source, p.x.size, p.y.size, planes, dx, dy, _lib.dptr(c), _lib.dptr(r) if r.size else None,
                                           r.size, _lib.dptr(rec), rec.shape[1]))
        return rec
    return call


def line(what, ms, bytes_moved, against=None):
    text = '%-58s median %8.3f ms (min %.3f max %.3f)  %7.1f GB/s' % (what, ms[0], ms[1], ms[2], bytes_moved / ms[0] * 1e-6)
    if against is not None:
        text += '   %.2f x the time of %s' % (ms[0] / against[1][0], against[0])
    print(text)


def probe(name, p, planes, n_sets=1, numpy_way=False):
    import metalens_amd as ma
    ctx = p.ctx
    T = planes * p.x.size * p.y.size
    dx = (p.x[-1] - p.x[0]) / (p.x.size - 1)
    nc = 96 if p.want_h else 48
    print('== %s: %d planes of %d x %d targets, T = %d, method %r, want_h %s, %d set(s)'
          % (name, planes, p.x.size, p.y.size, T, p.method, p.want_h, n_sets))
    t0 = time.perf_counter()
    p.queue_sets(0, n_sets)
    ctx.sync()
    print('first pass (plans, fills, propagates): %.1f ms' % ((time.perf_counter() - t0) * 1e3))
    for n in sorted({1, n_sets}):
        w = [1.0, 0.5, 2.0][:n]
        acc = median_ms(lambda: p.accumulate(w, reset=True), ctx.sync)
        line('accumulate, %d set(s) (reads %d B, writes %d B per target)' % (n, (80 if p.want_h else 48) * n, 16 if p.want_h else 8),
             acc, T * ((80 if p.want_h else 48) * n + (16 if p.want_h else 8)))
        st = median_ms(lambda: p.accumulate_stokes(w, reset=True), ctx.sync)
        line('accumulate_stokes, %d set(s) (reads %d B, writes 40 B per target)' % (n, 48 * n), st, T * (48 * n + 40), ('accumulate', acc))
    mid = (p.x.size // 2, p.y.size // 2)
    for K in (0, 8):
        radii = (np.arange(K) + 0.5) * dx
        for centre in (('peak',) if K == 0 else ('given', 'peak')):
            c = 'peak' if centre == 'peak' else mid
            fo = median_ms(focus_entry(p, planes, radii, None if centre == 'peak' else mid, 0), lambda: None)
            line('focus  K = %d centre=%-5s of=fields (%d B per target)' % (K, centre, 80 if p.want_h else 48), fo, T * (80 if p.want_h else 48))
            so = median_ms(stokes_entry(p, planes, radii, c, 0), lambda: None)
            line('stokes K = %d centre=%-5s of=fields (48 B per target%s)' % (K, centre, ', read twice' if K and centre == 'peak' else ''),
                 so, T * 48 * (2 if K and centre == 'peak' else 1), ('focus', fo))
            fs = median_ms(focus_entry(p, planes, radii, None if centre == 'peak' else mid, -1), lambda: None)
            line('focus  K = %d centre=%-5s of=sums   (%d B per target)' % (K, centre, 16 if p.want_h else 8), fs, T * (16 if p.want_h else 8))
            ss = median_ms(stokes_entry(p, planes, radii, c, -1), lambda: None)
            line('stokes K = %d centre=%-5s of=sums   (40 B per target%s)' % (K, centre, ', read twice' if K and centre == 'peak' else ''),
                 ss, T * 40 * (2 if K and centre == 'peak' else 1), ('focus', fs))
    radii = (np.arange(8) + 0.5) * dx
    t0 = time.perf_counter()
    got = p.stokes(radii)
    print('PlanePropagator.stokes K = 8 about the peak, the whole call with its host arithmetic: %.3f ms' % ((time.perf_counter() - t0) * 1e3))
    if numpy_way:
        t0 = time.perf_counter()
        d = p._download(0)
        t1 = time.perf_counter()
        twin = ma.stokes_metrics(d, p.x, p.y, radii)
        t2 = time.perf_counter()
        print('download + NumPy K = 8: download %.1f ms + stokes_metrics %.1f ms = %.1f ms;  dop %.12g (GPU %.12g)'
              % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, twin['dop'][0], got['dop'][0]))
    print('  result bytes per target: %d; plane 0: peak at %s, dop %.6f, longitudinal share %.4g'
          % (nc, tuple(int(i) for i in got['peak_index'][0]), got['dop'][0], got['longitudinal_share'][0]))
    sys.stdout.flush()


def main():
    import metalens_amd as ma
    from metalens_amd import _lib, layout, synthetic
    from metalens_amd.nearfield import nearfield_params
    wl, n_glass = 580e-9, 1.46
    k, Z = 2 * np.pi * n_glass / wl, ma.constants.Z0 / n_glass
    ctx = _lib.default_context()
    print(ctx.device_info())

    def upload(n):
        """a wave converging on the axis, its y part 0.6 exp(0.9 i) of its x part and tilted against it"""
        x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
        a = x.max()
        f = a / np.tan(np.arcsin(0.5))
        r2 = x[:, None] ** 2 + x[None, :] ** 2
        Ex = np.where(r2 <= a * a, np.exp(-1j * k * np.sqrt(r2 + f * f)), 0)
        Ey = 0.6 * np.exp(0.9j) * Ex * np.exp(1j * k * 0.02 * x[:, None])
        _lib.check(ctx.lib.ml_fields_upload(ctx.handle, n, n, *[_lib.dptr(_lib.c128(v)) for v in (Ex, Ey, -Ey / Z, Ex / Z)]))
        ctx.fields_owner = None
        return x, f

    x, f = upload(4096)
    d = x[1] - x[0]
    t = (np.arange(64) - 31.5) * d / 2 + d / 4
    z = f + np.linspace(-3, 3, 8) * wl / n_glass
    p = ma.PlanePropagator(x, x, wl, n_glass, t, t, z, method='fft-stack', subsample=(2, 2), cache_kernels=False, ctx=ctx)
    probe('stack 8 x 64^2 at half the pitch behind 4096^2', p, 8, numpy_way=True)
    if '--small-only' in sys.argv:
        return
    x, f = upload(64)
    d = x[1] - x[0]
    t = x[0] + d / 2 + (np.arange(4096) - 2048) * d
    p = ma.PlanePropagator(x, x, wl, n_glass, t, t, 40 * f, method='fft', ctx=ctx)
    probe('plane 4096^2 on the pitch behind 64^2', p, 1, numpy_way=True)
    # three field sets: the x, y and z dipoles of an emitter behind a small synthetic lens, synthesised as one batch
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design, radius=20e-6,
                               numerical_aperture=0.3, wavelength=wl, switch_angle=np.deg2rad(8.0), num_gratings=8, num_entries=8)
    fl = lens['source_distance']
    common = (wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'])
    x, y, _, ng = ma.build_nearfield(0.0, 0.0, -fl, 'x', *common, ctx=ctx, download=False)[4:8]
    params = (_lib.NearfieldParams * 3)()
    for m, pol in enumerate('xyz'):
        params[m] = nearfield_params(0.0, 0.0, -fl, pol, wl, ng, 1e-30, ma.constants.c0, ma.constants.Z0)
    xs, ys = _lib.f64(x), _lib.f64(y)
    _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, 3, _lib.dptr(xs), xs.size, _lib.dptr(ys), ys.size))
    dxp, dyp = x[1] - x[0], y[1] - y[0]
    tx, ty = x[0] + (np.arange(1024) - 512 + len(x) // 2) * dxp, y[0] + (np.arange(1024) - 512 + len(y) // 2) * dyp
    p = ma.PlanePropagator(x, y, wl, ng, tx, ty, 30e-6, method='fft', ctx=ctx)
    probe('plane 1024^2 behind a lens of 20 um radius, x + y + z dipoles', p, 1, n_sets=3)


if __name__ == '__main__':
    main()
