"""Times the beam metrics of the far field (``ml_farfield_beam``) against what they replace and against the kernel that
streams the same map, on ONE resident projection (needs an MI355X):

    python tools/beam_probe.py [--small-only] [--kernels-only]

On the projection of a 4096^2 aperture to 512^2 directions (the benchmark's workload), and to the whole 4096^2 lattice:

* (a) the record about a GIVEN centre: two launches (chunks, finish);
* (b) the record about the map's own PEAK: three launches (chunk peaks, chunks, finish) - the map is read twice;
* (c) ``ml_farfield_accumulate`` on the same map: the yardstick - it reads the same 8 B per direction (and writes 8 B of
  P_sum), two launches;
* (d) ``ml_farfield_project`` download + ``postprocess.beam_metrics``: what a caller pays today (``keep_each=True``);

with K = 0, 2 and 32 cones, and a three-source sweep (x, y, z dipoles) at 4096^2 -> 512^2 queued with and without
``beam_cones`` (two cones), alternating.

How the times are taken: the context's stream is its own, so an event recorded on another stream does not bracket its
work; (a), (b), (c) and the sweep are a host clock around ``reps`` calls queued back to back that ends in a device
synchronise, divided by ``reps`` - what a sweep pays per source, launch overhead included.  Every figure is the median
of 7 such batches after 2 warm batches (min and max beside it).  ``--kernels-only`` queues each kind once more for a
``rocprofv3 --kernel-trace --stats`` run of its own, which gives the kernels' own times."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def batch_ms(call, sync, reps, rounds=7, warm=2):
    times = []
    for r in range(warm + rounds):
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        sync()
        if r >= warm:
            times.append((time.perf_counter() - t0) * 1e3 / reps)
    return float(np.median(times)), float(min(times)), float(max(times))


def probe_map(name, ctx, t, Z0, reps, kernels_only):
    from metalens_amd import _lib, postprocess
    lib, h = ctx.lib, ctx.handle
    n = t.ux.size * t.uy.size
    print('== %s: %d x %d = %d directions, %.1f MB' % (name, t.ux.size, t.uy.size, n, n * 8e-6))
    _lib.check(lib.ml_farfield_project_async(h, Z0))
    centre = _lib.f64([t.ux[t.ux.size // 2], t.uy[t.uy.size // 2]])
    acc = lambda: _lib.check(lib.ml_farfield_accumulate(h, 1.0, 0.05, 0.0, 0.0, 0, 1))
    if kernels_only:
        acc()
        for K in (0, 2, 32):
            cones = _lib.f64(np.linspace(0.01, 0.3, K))
            _lib.check(lib.ml_farfield_beam(h, 0, _lib.dptr(centre), _lib.dptr(cones) if K else None, K, 0))
            _lib.check(lib.ml_farfield_beam(h, 0, None, _lib.dptr(cones) if K else None, K, 1))
        ctx.sync()
        return
    c = batch_ms(acc, ctx.sync, reps)
    print('(c) accumulate (reads 8 B, writes 8 B per direction): median %.4f ms (min %.4f max %.4f)  %.1f GB/s read'
          % (c + (n * 8 / c[0] * 1e-6,)))
    for K in (0, 2, 32):
        cones = _lib.f64(np.linspace(0.01, 0.3, K))
        cp = _lib.dptr(cones) if K else None
        a = batch_ms(lambda: _lib.check(lib.ml_farfield_beam(h, 0, _lib.dptr(centre), cp, K, 0)), ctx.sync, reps)
        b = batch_ms(lambda: _lib.check(lib.ml_farfield_beam(h, 0, None, cp, K, 1)), ctx.sync, reps)
        print('(a) record K = %2d, given centre: median %.4f ms (min %.4f max %.4f)  %.1f GB/s, %.2f of the time of (c)'
              % (K, a[0], a[1], a[2], n * 8 / a[0] * 1e-6, a[0] / c[0]))
        print('(b) record K = %2d, about the peak: median %.4f ms (min %.4f max %.4f)  %.1f GB/s (one read), %.2f of the time of (c), '
              '%.2f of (a)' % (K, b[0], b[1], b[2], n * 8 / b[0] * 1e-6, b[0] / c[0], b[0] / a[0]))
        runs = []
        for _ in range(2):
            t0 = time.perf_counter()
            P = np.empty((t.ux.size, t.uy.size))
            _lib.check(lib.ml_farfield_project(h, Z0, _lib.dptr(P), None, None))
            t1 = time.perf_counter()
            host = postprocess.beam_metrics(P, t.ux, t.uy, cones, 'peak')
            runs.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        best = min(runs, key=sum)
        rec = t.beam(cones, 'peak', slot=1)
        print('(d) project + download %.2f ms + postprocess.beam_metrics %.2f ms = %.2f ms (the better of 2); peak at %s (GPU %s), '
              'total_P %.15g (GPU %.15g)' % (best[0], best[1], sum(best), host['peak_index'], rec['peak_index'], host['total_P'],
                                            rec['total_P']))
    sys.stdout.flush()


def main():
    import bench
    import metalens_amd as ma
    from metalens_amd import _lib
    small_only, kernels_only = '--small-only' in sys.argv, '--kernels-only' in sys.argv
    wl = 580e-9
    lens, x, u = bench.build_workload(4096, 512, 1e-3, 0.5, wl, 1.0)
    ctx = _lib.default_context()
    print(ctx.device_info())
    f = lens['source_distance']
    sw = ma.SourceSweep(wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'], x, x, u, u, ctx=ctx)
    batch = [(0.0, 0.0, -f, pol) for pol in 'xyz']
    cones = (float(np.sin(np.radians(1.0))), float(np.sin(np.radians(3.0))))
    res = sw.run(batch, beam_cones=cones)          # priming pass: settles ties; the last projection stays resident
    print('sweep x + y + z, 4096^2 -> 512^2: pointing %s, rms divergence %.5f, cone fractions %s'
          % (res['beam_sum']['centroid_u'], float(np.sqrt(res['beam_sum']['second_moments_u'][:2].sum())),
             res['beam_sum']['cone_P'] / res['power_in'].sum()))
    if not kernels_only:
        for _ in range(20):
            sw.queue(batch)
        ctx.sync()
        rows = {'without': [], 'with': []}
        for _ in range(7):                          # alternating
            for key, kw in (('without', {}), ('with', dict(beam_cones=cones))):
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(10):
                    sw.queue(batch, **kw)
                ctx.sync()
                rows[key].append((time.perf_counter() - t0) * 1e2)
        for key in ('without', 'with'):
            print('sweep step (3 sources) %s beam_cones: median %.4f ms (min %.4f max %.4f)' % (key, np.median(rows[key]), min(rows[key]),
                                                                                              max(rows[key])))
        print('a sweep step with beam_cones costs %+.4f ms (%+.2f %%), %.4f ms per source'
              % (np.median(rows['with']) - np.median(rows['without']), 100 * (np.median(rows['with']) / np.median(rows['without']) - 1),
                 (np.median(rows['with']) - np.median(rows['without'])) / 3))
    t = ma.FarfieldTransform(x.size, x.size, x[1] - x[0], x[1] - x[0], wl, sw.n_glass, u, u, ctx=ctx)
    t.transform()
    probe_map('4096^2 -> 512^2', ctx, t, sw.Z0, 200, kernels_only)
    if small_only:
        return
    full = np.fft.fftshift(ma.fft_direction_cosines(x.size, x[1] - x[0], wl, sw.n_glass))
    t = ma.FarfieldTransform(x.size, x.size, x[1] - x[0], x[1] - x[0], wl, sw.n_glass, full, full, ctx=ctx)
    t.transform()
    probe_map('4096^2 -> the whole lattice of 4096^2', ctx, t, sw.Z0, 20, kernels_only)


if __name__ == '__main__':
    main()
