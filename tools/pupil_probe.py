"""Times the pupil function applied to the resident near field (``ml_fields_pupil_apply``) on the synthesised 4096^2 lens of
the benchmark with the lens's outer radius as a stopped pupil (needs an MI355X), and writes what it prints to
profiles/pupil_probe.txt:

    python tools/pupil_probe.py [--small] [--tag TEXT]

* the pass, warm, for one set and for the three sets of an x + y + z batch, in five variants: stop only; a phase plate of
  order 4; of order 8; the lens's own zone edges with unit-modulus factors; phase and edges together.  A host clock around
  batches of 10 queued launches that end in one synchronise (the plan is made before); median of 5 batches after 1 warm
  batch, per launch, min and max beside it.  Every factor has modulus 1, so the fields keep their size over the launches;
* beside them, in the same process, a device-to-device copy of the bytes the members' fields have (64 B read and 64 B
  written per member per set), timed the same way: every variant is given as a share of that copy's rate, counting the
  bytes of what the variant reads and writes;
* the route a caller pays today, once: ``ml_fields_download`` + ``postprocess.apply_pupil_host`` + ``ml_fields_upload``;
* the pass with the far-field transform and projection of the benchmark right behind it, as in a sweep, against the two
  alone.

``--small`` takes a 1024^2 aperture (a rehearsal, not a figure to quote); ``--tag`` is printed in the first line (which build
of the library ran: a comparison run, which leaves profiles/pupil_probe.txt alone)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    import bench
    import metalens_amd as ma
    from metalens_amd import _lib, postprocess
    from metalens_amd.nearfield import nearfield_params
    small = '--small' in sys.argv
    tag = sys.argv[sys.argv.index('--tag') + 1] if '--tag' in sys.argv else ''
    n = 1024 if small else 4096
    wl = 580e-9
    lens, x, u = bench.build_workload(n, 512, 1e-3 * n / 4096, 0.5, wl, 1.0)
    S, f = lens['lens_periphery_summary'], lens['source_distance']
    common = (wl, S, lens['lens_center_summary'], lens['hexgridset'])
    lines = []

    def say(text):
        print(text)
        sys.stdout.flush()
        lines.append(text)
    ctx = _lib.default_context()
    say('%s %s' % (ctx.device_info(), tag))
    R = float(S['r_max_list'][-1])
    edges = ma.zone_edges(S)
    n_glass = ma.build_nearfield(0.0, 0.0, -f, 'x', *common, x_pts=x, y_pts=x, ctx=ctx, download=False)[7]
    r2 = (x * x)[:, None] + (x * x)[None, :]
    members = int((r2 <= R * R).sum())
    total = n * n
    say('aperture %d x %d, stopped pupil of radius %.1f um: %d members (%.1f %% of the samples); %d zone edges'
        % (n, n, R * 1e6, members, 100.0 * members / total, edges.size))
    rng = np.random.default_rng(1)
    g = np.exp(2j * np.pi * rng.uniform(0, 1, edges.size))

    def phase(order):
        c = rng.uniform(-0.05, 0.05, (order + 1) * (order + 2) // 2)
        c[0] = 0.3
        return c
    # name -> (pupil, bytes read + written per set)
    both, stores = 128.0 * members, 64.0 * (total - members)
    variants = [('stop only', dict(), stores),
                ('phase of order 4', dict(phase=phase(4)), both + stores),
                ('phase of order 8', dict(phase=phase(8)), both + stores),
                ('%d edges' % edges.size, dict(edges=edges, zone_factors=g), both + stores),
                ('phase of order 8 and %d edges' % edges.size, dict(phase=phase(8), edges=edges, zone_factors=g), both + stores)]
    pupils = [(name, ma.AperturePupil(x, x, R, stop=True, ctx=ctx, **kw), nbytes) for name, kw, nbytes in variants]

    def batches(call, sync, reps=10):
        t = []
        for r in range(6):
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            sync()
            if r >= 1:
                t.append((time.perf_counter() - t0) * 1e3 / reps)
        return float(np.median(t)), min(t), max(t)

    def copy_rate(sets):
        nbytes = int(64 * members * sets)
        a = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        b = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        a.zero_()
        med, lo, hi = batches(lambda: b.copy_(a), torch.cuda.synchronize)
        rate = 2.0 * nbytes / (med * 1e-3)
        say('device-to-device copy of the members\' fields, %d set(s), %.2f GB read and as much written: median %.3f ms (min %.3f max %.3f): %.2f TB/s'
            % (sets, nbytes * 1e-9, med, lo, hi, rate * 1e-12))
        del a, b
        return rate

    def round_of(sets):
        rate = copy_rate(sets)
        for name, ap, nbytes in pupils:
            ap.plan()
            ctx.sync()
            med, lo, hi = batches(lambda: ap.queue(0, sets), ctx.sync)
            mine = nbytes * sets / (med * 1e-3)
            say('%-34s %d set(s): median %.3f ms per launch (min %.3f max %.3f); %.2f GB read + written: %.2f TB/s, %.0f %% of the copy\'s rate'
                % (name + ',', sets, med, lo, hi, nbytes * sets * 1e-9, mine * 1e-12, 100.0 * mine / rate))
    round_of(1)
    # what a caller pays today, once: download, NumPy, upload
    kw = variants[2][1]
    t0 = time.perf_counter()
    F = [np.empty((n, n), dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    t1 = time.perf_counter()
    G = postprocess.apply_pupil_host(*F, x, x, R, stop=True, **kw)
    t2 = time.perf_counter()
    _lib.check(ctx.lib.ml_fields_upload(ctx.handle, n, n, *[_lib.dptr(_lib.c128(a)) for a in G]))
    t3 = time.perf_counter()
    say('today\'s route, one set, phase of order 8: ml_fields_download %.1f ms + postprocess.apply_pupil_host %.1f ms + ml_fields_upload %.1f ms = %.1f ms'
        % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
    del F, G
    params = (_lib.NearfieldParams * 3)()
    for m, pol in enumerate('xyz'):
        params[m] = nearfield_params(0.0, 0.0, -f, pol, wl, n_glass, 1e-30, ma.constants.c0, ma.constants.Z0)
    xs = _lib.f64(x)
    _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, 3, _lib.dptr(xs), xs.size, _lib.dptr(xs), xs.size))
    ctx.sync()
    round_of(3)
    # who reads next in a sweep: the transform and its projection right behind the pass (one set, the benchmark's 512^2
    # directions), against the transform alone
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))
    t = ma.FarfieldTransform(n, n, x[1] - x[0], x[1] - x[0], wl, n_glass, u, u, ctx=ctx)
    ap = pupils[2][1]

    def transform():
        _lib.check(ctx.lib.ml_farfield_transform_async(ctx.handle, 0, 0))
        _lib.check(ctx.lib.ml_farfield_project_async(ctx.handle, ma.constants.Z0))

    def pair():
        ap.queue(0, 1)
        transform()
    transform()
    ctx.sync()
    alone = batches(transform, ctx.sync)
    pupil_alone = batches(lambda: ap.queue(0, 1), ctx.sync)
    both_t = batches(pair, ctx.sync)
    say('in a sweep, one set: transform + projection alone median %.3f ms (min %.3f max %.3f); phase of order 8 alone %.3f; the pass '
        'with the transform right behind it %.3f (min %.3f max %.3f): %+.3f ms against the sum' % (alone + pupil_alone[:1] + both_t + (both_t[0] - alone[0] - pupil_alone[0],)))
    del t
    if not small and not tag:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'pupil_probe.txt'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
