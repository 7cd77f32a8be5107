"""Times the Zernike moments of the resident near field's wavefront (``ml_fields_zernike``) against what they replace and
what lies nearest, on the synthesised 4096^2 lens of the benchmark with the lens's outer radius as the pupil (needs an
MI355X), and writes what it prints to profiles/wavefront_probe.txt:

    python tools/wavefront_probe.py [--small] [--kernels] [--kernel-stats FILE.csv]

* the entry, warm, for one set and for the three sets of an x + y + z batch, at n_max = 4 and 8: a host clock around calls
  that each end in the entry's own synchronise - upload of the axis arrays, both launches, the download of the monomial
  moments and the host conversion included; median of 7 after 2 warm calls, min and max beside it;
* (a) ``ml_fields_zones`` on the same grid with that radius as its single edge - the nearest existing capability, the same
  members and the same reference phase - timed the same way in the same run;
* (b) the rate ``propagate_accumulate_kernel`` streams a buffer of the bytes of one field set at (a 3344^2 image behind a
  64^2 aperture: 96 B a target), entry + synchronise;
* (c) ``ml_fields_download`` of one set + ``postprocess.wavefront_metrics``: what a caller pays today, once;
* the largest difference between GPU and twin in units of u sum |E| (u = 2^-53).

``--kernels`` runs the GPU calls alone - what a ``rocprofv3 --kernel-trace --stats`` run of its own wraps; ``--kernel-stats``
takes that run's kernel statistics and prints the two launches' own times beside the calls'.  ``--small`` takes a 1024^2
aperture (a rehearsal, not a figure to quote)."""
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
    from metalens_amd import _lib, postprocess
    from metalens_amd.nearfield import nearfield_params
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
    R = float(S['r_max_list'][-1])
    n_glass = ma.build_nearfield(0.0, 0.0, -f, 'x', *common, x_pts=x, y_pts=x, ctx=ctx, download=False)[7]
    aw = {n_max: ma.ApertureWavefront(x, x, wl, n_glass, R, n_max=n_max, ctx=ctx) for n_max in (4, 8)}
    az = ma.ApertureZones(x, x, wl, n_glass, [R], ctx=ctx)
    members = int(aw[4].records(0, 1)[0, 0])
    say('aperture %d x %d, pupil of radius %.1f um: %d members (%.1f %% of the samples), plane-wave reference along the axis'
        % (n, n, R * 1e6, members, 100.0 * members / (n * n)))

    def timed(name, call, sets):
        t = []
        for r in range(9):
            t0 = time.perf_counter()
            call(0, sets)
            if r >= 2:
                t.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(t))
        rate = 64.0 * members * sets / (med * 1e-3)
        say('%-32s %d set(s): median %.3f ms (min %.3f max %.3f); the members\' fields are %.2f GB: %.2f TB/s'
            % (name, sets, med, min(t), max(t), 64e-9 * members * sets, rate * 1e-12))
        return med

    def round_of(sets):
        for n_max in (4, 8):
            timed('ml_fields_zernike n_max = %d,' % n_max, aw[n_max].records, sets)
        timed('(a) ml_fields_zones, one edge,', az.records, sets)
    round_of(1)
    if not kernels_only:
        gpu = aw[8].analyse(0, 1)
        t0 = time.perf_counter()
        F = [np.empty((n, n), dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
        t1 = time.perf_counter()
        host = postprocess.wavefront_metrics(*F, x, x, wl, n_glass, R, 8)
        t2 = time.perf_counter()
        say('(c) ml_fields_download %.1f ms + postprocess.wavefront_metrics (n_max = 8) %.1f ms = %.1f ms'
            % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3))
        assert gpu['samples'] == host['samples']
        member = (x * x)[:, None] + (x * x)[None, :] <= R * R
        sum_E = np.array([np.abs(F[c][member]).sum() for c in (0, 1)])
        scale = aw[8].dA / (np.pi * R * R)
        with np.errstate(divide='ignore', invalid='ignore'):
            d = np.abs(gpu['moments'] - host['moments'])[0] / (2.0 ** -53 * sum_E[:, None] * scale)
        say('GPU against the twin: members equal; the 45 moments differ by at most %.3g u sum |E| (Ex), %.3g (Ey); rms wavefront %.4f rad, '
            'Strehl %.4f (Ex)' % (float(np.nanmax(d[0])), float(np.nanmax(d[1])), gpu['rms'][0, 0], gpu['coherence'][0, 0]))
        del F
    params = (_lib.NearfieldParams * 3)()
    for m, pol in enumerate('xyz'):
        params[m] = nearfield_params(0.0, 0.0, -f, pol, wl, n_glass, 1e-30, ma.constants.c0, ma.constants.Z0)
    xs = _lib.f64(x)
    _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, 3, _lib.dptr(xs), xs.size, _lib.dptr(xs), xs.size))
    ctx.sync()
    round_of(3)
    round_of(1)
    if not kernels_only:
        # (b) the streaming kernel: a result buffer of the bytes of one field set, 96 B a target (80 read, 16 written)
        side = int(round(np.sqrt(64.0 * n * n / 96.0)))
        xa = (np.arange(64) - 31.5) * (x[1] - x[0])
        Ex = np.exp(-1j * 2 * np.pi * n_glass / wl * np.sqrt(xa[:, None] ** 2 + xa[None, :] ** 2 + 1e-8))
        zero = np.zeros_like(Ex)
        _lib.check(ctx.lib.ml_fields_upload(ctx.handle, 64, 64, *[_lib.dptr(_lib.c128(v)) for v in (Ex, zero, zero, Ex / 377.0)]))
        ctx.fields_owner = None
        t = xa[0] + (x[1] - x[0]) / 2 + (np.arange(side) - side // 2) * (x[1] - x[0])
        p = ma.PlanePropagator(xa, xa, wl, n_glass, t, t, 1e-3, method='fft', ctx=ctx)
        p.queue_sets(0, 1)
        ctx.sync()
        tt = []
        for r in range(12):
            t0 = time.perf_counter()
            p.accumulate([1.0], reset=True)
            ctx.sync()
            if r >= 3:
                tt.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(tt))
        say('(b) propagate_accumulate_kernel on %d^2 targets, %.2f GB moved: median %.3f ms (min %.3f max %.3f): %.2f TB/s'
            % (side, 96e-9 * side * side, med, min(tt), max(tt), 96.0 * side * side / (med * 1e-3) * 1e-12))
    if stats:
        say('kernels alone (rocprofv3 --kernel-trace --stats over `tools/wavefront_probe.py --kernels`, a run of its own; average, min ... max in ms):')
        with open(stats) as fh:
            for row in csv.DictReader(fh):
                if any(key in row['Name'] for key in ('wavefront_', 'zones_')):
                    say('  %-90s calls %3s  %.3f  (%.3f ... %.3f)' % (row['Name'].replace('void ', '')[:90], row['Calls'], float(row['AverageNs']) * 1e-6,
                                                                     float(row['MinNs']) * 1e-6, float(row['MaxNs']) * 1e-6))
    if not small and not kernels_only:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'wavefront_probe.txt'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
