"""Times the per-zone contributions to the field behind the lens (``ml_fields_zone_fields``) against its yardsticks, on the
synthesised 4096^2 lens of the benchmark with that lens's own zone edges (needs an MI355X), and writes what it prints to
profiles/zone_fields_probe.txt:

    python tools/zone_fields_probe.py [--small] [--kernels] [--kernel-stats FILE.csv]

All in one process, on the same resident field set, for T = 1, 8 and 64 points around the focus-side mirror point of the
emitter (host clock around calls that end in a synchronise; median of 5 after 1 warm call, min and max beside it):
* the entry, whole: upload of the axis arrays and targets, every walk's two launches, the download of the records;
* ``PlanePropagator(method='direct', point_list=True).propagate()`` on the same points: the same pairs, added over all zones;
* ``ml_fields_zones``: the same line walk with scalar terms;
* the route the entry replaces, K times (a pupil that keeps one zone, then the direct propagator) - measured on 8 zones
  spread over the lens and scaled to K, since every round costs one pupil pass and one whole pair sum whatever the zone.
The pairs of a call are ``nx ny T``; ``--kernels`` runs the GPU calls alone - what a ``rocprofv3 --kernel-trace --stats`` run of
its own wraps; ``--kernel-stats`` adds the kernel lines of that run's ``kernel_stats.csv`` (the line kernel alone).
``--small`` takes a 1024^2 aperture (a rehearsal, not a figure to quote)."""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    import metalens_amd as ma
    from metalens_amd import _lib
    small, kernels_only = '--small' in sys.argv, '--kernels' in sys.argv
    stats = sys.argv[sys.argv.index('--kernel-stats') + 1] if '--kernel-stats' in sys.argv else None
    n = 1024 if small else 4096
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
    K = edges.size
    n_glass = ma.build_nearfield(0.0, 0.0, -f, 'x', *common, x_pts=x, y_pts=x, ctx=ctx, download=False)[7]
    say('aperture %d x %d, %d edges (the centre and %d rings), points about (0, 0, %.1f um); %d targets per walk'
        % (n, n, K, K - 1, f * 1e6, ma.postprocess.ZONE_FIELDS_TG))
    rng = np.random.default_rng(3)
    pts = np.concatenate([[[0.0, 0.0, f]], np.stack([rng.uniform(-2e-6, 2e-6, 63), rng.uniform(-2e-6, 2e-6, 63), f + rng.uniform(-5e-6, 5e-6, 63)], axis=1)])

    def timed(name, call, pairs=None, reps=6):
        t = []
        for r in range(reps):
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if r >= 1:
                t.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(t))
        rate = '' if pairs is None else ': %.1f G pairs/s' % (pairs / (med * 1e-3) * 1e-9)
        say('%-58s median %9.3f ms (min %.3f max %.3f)%s' % (name, med, min(t), max(t), rate))
        return med
    az = ma.ApertureZones(x, x, wl, n_glass, edges, ctx=ctx)
    timed('ml_fields_zones, 1 set', lambda: az.records(0, 1))
    made = {}
    for T in (1, 8, 64):
        p = pts[:T]
        azf = ma.ApertureZoneFields(x, x, wl, n_glass, edges, p, ctx=ctx)
        prop = ma.PlanePropagator(x, x, wl, n_glass, p[:, 0], p[:, 1], p[:, 2], point_list=True, ctx=ctx)
        pairs = float(n) * n * T
        zf = timed('ml_fields_zone_fields T = %2d, E and H, 1 set' % T, lambda: azf.records(0, 1), pairs)
        if T == 64:
            e_only = ma.ApertureZoneFields(x, x, wl, n_glass, edges, p, want_h=False, ctx=ctx)
            timed('ml_fields_zone_fields T = %2d, E only, 1 set' % T, lambda: e_only.records(0, 1), pairs)
        direct = timed('PlanePropagator direct, point list, T = %2d' % T, prop.propagate, pairs)
        say('    the zone pass costs %.2f x the direct sum at T = %d' % (zf / direct, T))
        made[T] = (azf, prop, zf, azf.records(0, 1))
    # the replaced route on 8 zones, behind every other figure: the fields are downloaded once and put back after every
    # round, and an uploaded field carries no row extents
    F = None
    if not kernels_only:
        F = [np.empty((n, n), dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    for T in (() if kernels_only else (1, 8, 64)):
        azf, prop, zf, rec = made[T]
        some = np.unique(np.linspace(0, K - 1, 8).astype(int))
        t_route, worst = [], 0.0
        for z in some:
            g = np.zeros(K, dtype=complex)
            g[z] = 1.0
            one = ma.AperturePupil(x, x, edges[-1], edges=edges, zone_factors=g, ctx=ctx)
            t0 = time.perf_counter()
            one.apply(0, 1)
            d = prop.propagate()
            t_route.append((time.perf_counter() - t0) * 1e3)
            Ez = np.stack([d['Ex'], d['Ey'], d['Ez']])                       # (3, T)
            mine = rec[0, z, :, 0:6:2].T + 1j * rec[0, z, :, 1:6:2].T
            worst = max(worst, float(np.abs(Ez - mine).max() / np.abs(rec[0, :, :, :6]).max()))
            _lib.check(ctx.lib.ml_fields_upload(ctx.handle, n, n, *[_lib.dptr(a) for a in F]))
            ctx.fields_owner = None
        med = float(np.median(t_route))
        say('    T = %2d: one zone by pupil + direct propagator: median %.3f ms per zone, x %d zones = %.1f ms: %.1f x the zone pass; the %d zones '
            'agree with the pass to %.2e of the largest contribution' % (T, med, K, med * K, med * K / zf, some.size, worst))
    del F
    if stats:
        say('kernels alone (rocprofv3 --kernel-trace --stats over `tools/zone_fields_probe.py --kernels`, a run of its own; average, min ... '
            'max in ms):')
        with open(stats) as fh:
            for row in csv.DictReader(fh):
                if any(key in row['Name'] for key in ('zf_', 'zones_', 'propagate_kernel')):
                    say('  %-90s calls %4s  %.3f  (%.3f ... %.3f)' % (row['Name'].replace('void ', '')[:90], row['Calls'], float(row['AverageNs']) * 1e-6,
                                                                      float(row['MinNs']) * 1e-6, float(row['MaxNs']) * 1e-6))
    if not small and not kernels_only:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'zone_fields_probe.txt'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
