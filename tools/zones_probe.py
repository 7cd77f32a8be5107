"""Times the per-zone sums of the resident near field (``ml_fields_zones``) against what they replace, on a synthesised
4096^2 lens with that lens's own zone edges (needs an MI355X), and writes what it prints to profiles/zones_probe.txt:

    python tools/zones_probe.py [--small]

* the entry, warm, for the one set of a synthesis and for the three sets of an x + y + z batch: a host clock around calls
  that each end in the entry's own synchronise - upload of the axis arrays, both launches and the download of the records
  included; median of 7 after 2 warm calls, min and max beside it;
* ``64 nx ny sets`` bytes - the four complex fields of every sample, read once - over that time, as a share of the HBM
  bandwidth a copy kernel reaches on this chip (6.29 TB/s measured, 8 TB/s on paper): the whole call over the bytes, not a
  kernel's share of peak;
* ``ml_fields_download`` of one set + ``postprocess.zone_metrics``: what a caller pays today, once;
* the largest difference between the two in units of the yardstick's bound for a double-precision sum.

``--small`` takes a 1024^2 aperture (a rehearsal, not a figure to quote)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_MEASURED, HBM_PAPER = 6.29e12, 8.0e12


def main():
    import bench
    import metalens_amd as ma
    from metalens_amd import _lib, postprocess
    from metalens_amd.nearfield import nearfield_params
    n = 1024 if '--small' in sys.argv else 4096
    wl = 580e-9
    lens, x, _ = bench.build_workload(n, 512, 1e-3 * n / 4096, 0.5, wl, 1.0)
    S, f = lens['lens_periphery_summary'], lens['source_distance']
    common = (wl, S, lens['lens_center_summary'], lens['hexgridset'])
    lines = []

    def say(text):
        print(text)
        sys.stdout.flush()
        lines.append(text)
    ctx = _lib.default_context()
    say('%s' % (ctx.device_info(),))
    edges = ma.zone_edges(S)
    n_glass = ma.build_nearfield(0.0, 0.0, -f, 'x', *common, x_pts=x, y_pts=x, ctx=ctx, download=False)[7]
    az = ma.ApertureZones(x, x, wl, n_glass, edges, ctx=ctx)
    say('aperture %d x %d, %d edges (the centre and %d rings), plane-wave reference along the axis' % (n, n, edges.size, edges.size - 1))

    def timed(sets):
        t = []
        for r in range(9):
            t0 = time.perf_counter()
            az.records(0, sets)
            if r >= 2:
                t.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(t))
        rate = 64.0 * n * n * sets / (med * 1e-3)
        say('ml_fields_zones, %d set(s): median %.3f ms (min %.3f max %.3f) for %.2f GB of fields: %.2f TB/s, %.0f %% of the measured '
            'copy bandwidth, %.0f %% of the paper figure' % (sets, med, min(t), max(t), 64e-9 * n * n * sets, rate * 1e-12,
                                                             100 * rate / HBM_MEASURED, 100 * rate / HBM_PAPER))
    timed(1)
    gpu = az.analyse(0, 1)
    t0 = time.perf_counter()
    F = [np.empty((n, n), dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    t1 = time.perf_counter()
    host = postprocess.zone_metrics(*F, x, x, wl, n_glass, edges)
    t2 = time.perf_counter()
    say('ml_fields_download %.1f ms + postprocess.zone_metrics %.1f ms = %.1f ms' % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3))
    assert np.array_equal(gpu['samples'], host['samples'])
    u = 2.0 ** -53
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.abs(gpu['I'] - host['I']) / ((host['samples'][None, :, None] + 16) * u * host['I'])
    say('GPU against the twin: samples equal; sum I differs by at most %.3f of (n + 16) u sum I' % float(np.nanmax(d)))
    del F
    params = (_lib.NearfieldParams * 3)()
    for m, pol in enumerate('xyz'):
        params[m] = nearfield_params(0.0, 0.0, -f, pol, wl, n_glass, 1e-30, ma.constants.c0, ma.constants.Z0)
    xs = _lib.f64(x)
    _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, 3, _lib.dptr(xs), xs.size, _lib.dptr(xs), xs.size))
    ctx.sync()
    timed(3)
    timed(1)
    if '--small' not in sys.argv:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'zones_probe.txt'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
