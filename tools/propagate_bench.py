#!/usr/bin/env python3
"""Time of the finite-distance propagator (csrc/propagate.hip) and what it means in fp64 vector issue.

    python tools/propagate_bench.py [--quick] > profiles/propagate_bench.txt          (needs an MI355X)
    python tools/propagate_bench.py --static                                          (the instruction count only; no GPU)

One JSON line per case: an uploaded ideal converging wave on a circular pupil (no row extents: EVERY sample of
the aperture is summed, pairs = nx ny targets) propagated to an image patch in its focal plane or to an xz cut
through the focus, E + H and E only.  ms = host clock around ml_propagate ... ml_sync, best of three, after
bench.py's priming rule (one pass, then at least 50 ms of further passes).  valu_per_pair = static count of
vector instructions in the kernel's inner loop per aperture sample, from the assembly (hipcc cross-compiles; as
tools/nearfield_phase_instructions.py); issue_fraction = pairs x valu_per_pair x 4 cycles / (CUs x 4 SIMDs x 64
lanes x clock x time) with the clock taken as 2.4 GHz: the share of the chip's fp64 vector issue slots the
loop's instructions account for (a v_fma_f64 holds a SIMD four cycles per wave)."""
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
    """{True: n, False: n}: vector instructions per aperture sample in the innermost loop of propagate_kernel<WANT_H>
    (the loop that holds the reciprocal square root of the distance)"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'k.s')
        subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off',
                        '-I' + os.path.join(ROOT, 'include'), '-I' + SRC, '-S', '--cuda-device-only', '-o', out,
                        os.path.join(SRC, 'propagate.hip')], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        s = open(out).read()
    counts = {}
    for want_h, tag in ((True, 'ILb1EE'), (False, 'ILb0EE')):
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
        counts[want_h] = sum(op.startswith('v_') for op in best) / samples
    return counts


def main():
    valu = inner_loop_valu()
    if '--static' in sys.argv:
        print(json.dumps({'valu_per_pair': {'E+H': valu[True], 'E': valu[False]}}))
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

            def one():
                t0 = time.perf_counter()
                _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))
                ctx.sync()
                return time.perf_counter() - t0
            t_one = min(one(), one())
            for _ in range(max(1, min(200, int(0.05 / max(t_one, 1e-5))))):
                _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))
            ctx.sync()
            best = min(one() for _ in range(3))
            pairs = n * n * targets
            print(json.dumps({
                'case': '%d^2 -> %s' % (n, '%d^2' % m if kind == 'patch' else '%d-point xz cut' % m),
                'fields': 'E+H' if want_h else 'E', 'ms': round(best * 1e3, 3), 'pairs': pairs,
                'pair_evals_per_s': round(pairs / best, 1), 'valu_per_pair': valu[want_h],
                'issue_fraction': round(pairs * valu[want_h] * 4 / (cus * 4 * 64 * CLOCK_HZ * best), 4),
                'cu_count': cus}), flush=True)


if __name__ == '__main__':
    main()
