#!/usr/bin/env python3
"""Time of the finite-distance propagator (csrc/propagate.hip) and what it means in fp64 vector issue.

    python tools/propagate_bench.py [--quick] > profiles/propagate_bench.txt          (needs an MI355X)
    python tools/propagate_bench.py --static                                          (the instruction count only; no GPU)
    python tools/propagate_bench.py --sets >> profiles/propagate_bench.txt            (needs an MI355X)

One JSON line per case: an uploaded ideal converging wave on a circular pupil (no row extents: EVERY sample of
the aperture is summed, pairs = nx ny targets) propagated to an image patch in its focal plane or to an xz cut
through the focus, E + H and E only.  ms = host clock around ml_propagate ... ml_sync, best of three, after
bench.py's priming rule (one pass, then at least 50 ms of further passes).  valu_per_pair = static count of
vector instructions in the kernel's inner loop per aperture sample, from the assembly (hipcc cross-compiles; as
tools/nearfield_phase_instructions.py); issue_fraction = pairs x valu_per_pair x 4 cycles / (CUs x 4 SIMDs x 64
lanes x clock x time) with the clock taken as 2.4 GHz: the share of the chip's fp64 vector issue slots the
loop's instructions account for (a v_fma_f64 holds a SIMD four cycles per wave).

--sets: ONE ml_propagate_sets pass over the three field sets of a synthesised x, y, z dipole batch against THREE
ml_fields_select + ml_propagate calls on the same sets (the single-set kernel, which the NS parameter left as it
was), 2048^2 -> 64^2, E + H and E only, timed as above; ratio = ms of the one pass / ms of the three.  The fields are
a synthetic lens' (row extents: only samples inside the lens circle are summed, in both paths alike).  The static
count covers NS = 1, 2, 3: per (sample, target) pair, all sets of the pass together."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, 'metalens_amd', 'csrc')
CLOCK_HZ = 2.4e9


def inner_loop_valu():
    """{(WANT_H, NS): n}: vector instructions per aperture sample in the innermost loop of propagate_kernel<WANT_H, NS>
    (the loop that holds the reciprocal square root of the distance), for all NS field sets together"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'k.s')
        subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off',
                        '-I' + os.path.join(ROOT, 'include'), '-I' + SRC, '-S', '--cuda-device-only', '-o', out,
                        os.path.join(SRC, 'propagate.hip')], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        s = open(out).read()
    counts = {}
    for want_h, ns in ((h, n) for h in (True, False) for n in (1, 2, 3)):
        tag = 'ILb%dELi%dEE' % (want_h, ns)
        name = re.search(r'^(_ZN2ml16propagate_kernel%s\w*):' % tag, s, re.M).group(1)
        i = s.index('\n' + name + ':')
        body = s[i:s.index('.Lfunc_end', i)].splitlines()
        labels = {m.group(1): k for k, l in enumerate(body) for m in [re.match(r'(\.LBB\d+_\d+):', l)] if m}
        best = None
        for k, l in enumerate(body):           # backward branches = loops; the shortest one that holds a v_rsq_f64
            m = re.match(r'\ts_cbranch_\w+\s+(\.LBB\d+_\d+)', l)
            if m and labels.get(m.group(1), k) < k:
                loop = [x.split()[0] for x in body[labels[m.group(1)]:k + 1] if x.startswith('\t') and not x.strip().startswith(('.', ';'))]
                if 'v_rsq_f64_e32' in loop or 'v_rsq_f64' in loop:
                    if best is None or len(loop) < len(best):
                        best = loop
        samples = sum(op.startswith('v_rsq_f64') for op in best)
        counts[want_h, ns] = sum(op.startswith('v_') for op in best) / samples
    return counts


def best_ms(ctx, call):
    """bench.py's priming rule (one pass, then at least 50 ms of further passes), then the best of three"""
    def one():
        t0 = time.perf_counter()
        call()
        ctx.sync()
        return time.perf_counter() - t0
    t_one = min(one(), one())
    for _ in range(max(1, min(200, int(0.05 / max(t_one, 1e-5))))):
        call()
    ctx.sync()
    return min(one() for _ in range(3)) * 1e3


def sets_against_singles(valu, n=2048, m=64):
    """one pass over three sets against three single-set passes: JSON lines with both times and their ratio"""
    import math

    import numpy as np

    import metalens_amd as ma
    from metalens_amd import _lib, layout, synthetic
    from metalens_amd.nearfield import nearfield_params
    from metalens_amd.propagate import PlanePropagator
    ctx = _lib.default_context()
    wl = 580e-9
    pitch = wl / 2.2
    x = (np.arange(n) - (n - 1) / 2) * pitch
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design,
                               radius=x.max(), numerical_aperture=0.4, wavelength=wl, switch_angle=9 * math.pi / 180,
                               num_gratings=20, num_entries=12, design_kwargs={'wavelength': wl})
    f = lens['source_distance']
    common = (wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'])
    n_glass = ma.build_nearfield(0.0, 0.0, -f, 'x', *common, x_pts=x, y_pts=x, ctx=ctx, download=False)[7]
    params = (_lib.NearfieldParams * 3)()
    for k, pol in enumerate('xyz'):
        params[k] = nearfield_params(0.0, 0.0, -f, pol, wl, n_glass, 1e-30, ma.constants.c0, ma.constants.Z0)
    xs = _lib.f64(x)
    _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, 3, _lib.dptr(xs), xs.size, _lib.dptr(xs), xs.size))
    ctx.sync()
    r_lens = float(lens['lens_periphery_summary']['r_max_list'][-1])
    in_lens = int(np.count_nonzero(x[:, None] ** 2 + x[None, :] ** 2 <= r_lens ** 2))
    t = np.linspace(-4, 4, m) * wl
    for want_h in (True, False):
        p = PlanePropagator(x, x, wl, n_glass, t, t, f, want_h=want_h, ctx=ctx)

        def together():
            _lib.check(ctx.lib.ml_propagate_sets(ctx.handle, p.Z0, 0, 3))

        def singly():
            for k in range(3):
                _lib.check(ctx.lib.ml_fields_select(ctx.handle, k))
                _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))
        ms_singles = best_ms(ctx, singly)
        ms_sets = best_ms(ctx, together)
        print(json.dumps({
            'case': '%d^2 -> %d^2, x + y + z dipoles' % (n, m), 'fields': 'E+H' if want_h else 'E',
            'ms_one_pass_of_three_sets': round(ms_sets, 3), 'ms_three_single_passes': round(ms_singles, 3),
            'ratio': round(ms_sets / ms_singles, 4), 'samples_in_lens': in_lens,
            'valu_per_pair': {'three sets': valu[want_h, 3], 'one set': valu[want_h, 1]},
            'static_ratio': round(valu[want_h, 3] / (3 * valu[want_h, 1]), 4)}), flush=True)
        _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))


def main():
    valu = inner_loop_valu()
    if '--static' in sys.argv:
        print(json.dumps({'valu_per_pair': {'E+H': valu[True, 1], 'E': valu[False, 1]},
                          'valu_per_pair_two_sets': {'E+H': valu[True, 2], 'E': valu[False, 2]},
                          'valu_per_pair_three_sets': {'E+H': valu[True, 3], 'E': valu[False, 3]}}))
        return
    if '--sets' in sys.argv:
        sets_against_singles(valu, *((1024, 64) if '--quick' in sys.argv else ()))
        return
    import numpy as np

    from metalens_amd import _lib, constants
    from metalens_amd.propagate import PlanePropagator
    ctx = _lib.default_context()
    cus = ctx.device_info()['cu_count']
    wl, n_glass = 580e-9, 1.46
    k, Z = 2 * np.pi * n_glass / wl, constants.Z0 / n_glass
    cases = [(2048, 'patch', 64), (4096, 'patch', 64), (4096, 'patch', 256), (4096, 'xz-cut', 4096)]
    if '--quick' in sys.argv:
        cases = [(1024, 'patch', 64), (1024, 'xz-cut', 4096)]
    resident = None
    for n, kind, m in cases:
        x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
        f = x.max() / np.tan(np.arcsin(0.5))
        if resident != n:
            r2 = x[:, None] ** 2 + x[None, :] ** 2
            Ex = np.where(r2 <= x.max() ** 2, np.exp(-1j * k * np.sqrt(r2 + f * f)), 0)
            zero = np.zeros_like(Ex)
            _lib.check(ctx.lib.ml_fields_upload(ctx.handle, n, n, *[_lib.dptr(_lib.c128(a)) for a in (Ex, zero, zero, Ex / Z)]))
            resident = n
            del Ex, zero, r2
        if kind == 'patch':
            t = np.linspace(-4, 4, m) * wl
            args, kw, targets = (t, t, f), {}, m * m
        else:
            t = np.linspace(-8, 8, m) * wl
            args, kw, targets = (t, np.zeros(m), f + t), {'point_list': True}, m
        for want_h in (True, False):
            p = PlanePropagator(x, x, wl, n_glass, *args, want_h=want_h, ctx=ctx, **kw)

            best = best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))) / 1e3
            pairs = n * n * targets
            print(json.dumps({
                'case': '%d^2 -> %s' % (n, '%d^2' % m if kind == 'patch' else '%d-point xz cut' % m),
                'fields': 'E+H' if want_h else 'E', 'ms': round(best * 1e3, 3), 'pairs': pairs,
                'pair_evals_per_s': round(pairs / best, 1), 'valu_per_pair': valu[want_h, 1],
                'issue_fraction': round(pairs * valu[want_h, 1] * 4 / (cus * 4 * 64 * CLOCK_HZ * best), 4),
                'cu_count': cus}), flush=True)


if __name__ == '__main__':
    main()
