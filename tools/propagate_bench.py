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
count covers NS = 1, 2, 3: per (sample, target) pair, all sets of the pass together.

    python tools/propagate_bench.py --method fft [--quick] >> profiles/propagate_bench.txt     (needs an MI355X)

--method fft: ``PlanePropagator(method='fft')`` (csrc/propagate_grid.hip, propagate_grid_fft.hip) against the direct sum on the SAME targets - an
m x m patch on the aperture's pitch around the focus, off its lattice by 0.3 / 0.6 pitch - for 2048^2 -> 64^2, 4096^2 ->
64^2 and 4096^2 -> 256^2, E + H and E only: ms of a pass on cached kernel spectra (timed as above), ms_first = plan +
first pass (workspace, kernel fill and its transform, once), the direct pass, max |E_fft - E_direct| / max |E|, and crossover_targets = the target count
from which the cached FFT pass is the faster one, by the direct sum's time per target (it is linear in the targets).
Then 'fft' alone: 4096^2 -> 4096^2 (L = 8192^2, 18 / 15 GiB of workspace), and the three sets of a synthesised x, y, z
batch in one ml_propagate_sets call, 2048^2 -> 64^2.

    python tools/propagate_bench.py --method fft-long [--quick] >> profiles/propagate_bench.txt     (needs an MI355X)

--method fft-long: ``PlanePropagator(method='fft-long')`` for the 8192^2 aperture (L = 16384^2, 72 / 60 GiB of workspace):
8192^2 -> 64^2 and 8192^2 -> 4096^2 on the pitch, E + H and E only.  ms = a pass on cached kernel spectra, ms_first = plan
+ first pass with the workspace already reserved (kernel fill and the transform of the eight spectra),
ms_first_with_workspace = the same from a context that holds no workspace (the hipMalloc on top).  The direct sum runs
once, on 8192^2 -> 64^2 with E + H (best of two passes): max |E_fft-long - E_direct| / max |E| and crossover_targets as
above.  A workspace the device cannot give is reported with the library's message, and the E-only rows follow.
--quick: 8192^2 -> 64^2, E + H, without the direct sum.

    python tools/propagate_bench.py --method fft-tiled --case N,M [--tile L] [--against fft|fft-long] [--direct T] [--eh-only]

--method fft-tiled: ``PlanePropagator(method='fft-tiled')`` for one case N^2 -> M^2 per process (default 4096,64; --quick:
1024,64), the same converging wave and the same targets as the rows above: ms = a pass on cached kernel spectra, ms_first
= plan + first pass (workspace, the fill of every tile's kernels and their transform), the tile lengths (--tile L: L x L
instead of the default), tiles, batch and workspace; --against: the cached pass of that method on the same targets, its
workspace and max |E_tiled - E_other| / max |E|; --direct T: one direct pass on a T x T corner of the patch, its time per
target and crossover_targets (for apertures no other FFT form takes).  With a diagnostic build of the library
(METALENS_HIP_LIB) ML_GRID_TILE_BATCH_MIB sets the bytes of a batch and is reported as batch_MiB.

    python tools/propagate_bench.py --method fft-fine --case N,M [--subsample S] [--no-direct]

--method fft-fine: ``PlanePropagator(method='fft-fine')`` for one case N^2 -> M^2 fine targets at the pitch / S per process
(default 4096,64 and 2; --quick: 1024,64), E + H, with the kernel spectra kept and filled in every pass, against the loop
of S^2 'fft-tiled' propagators that gives the same targets lattice by lattice and against one direct pass on them
(``fft_fine``).  With a diagnostic build of the library ML_GRID_FINE_PAIR=1 contracts one lattice per read of the current
spectra instead of two and is reported as lattices_per_contraction.

    python tools/propagate_bench.py --method fft-stack --planes N [--case N,M] [--subsample S] [--row ROW]

--method fft-stack: ``PlanePropagator(method='fft-stack')`` for N planes of M^2 fine targets at the pitch / S around the focus
(default 4096,64 and 2; --quick: 1024,64), E + H (``fft_stack``).  --row picks ONE row, so that every row can have a process
of its own: ``stack-streamed``, ``stack-cached`` (a pass on the plan; ms_first = plan + first pass; the workspace),
``loop`` (what gives the same volume without this method: one 'fft-fine' propagator per z, each planned and passed once,
with the default cache_kernels=True), ``loop-streamed`` (the same with cache_kernels=False)
and ``fine`` (one cached 'fft-fine' pass at the first z: the yardstick of N = 1).  Without --row: all four."""
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


def converging_wave(ctx, n, wl, n_glass):
    """upload the ideal converging wave on a circular pupil of n^2 samples -> axis, focal length"""
    import numpy as np

    from metalens_amd import _lib, constants
    k, Z = 2 * np.pi * n_glass / wl, constants.Z0 / n_glass
    x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
    f = x.max() / np.tan(np.arcsin(0.5))
    r2 = x[:, None] ** 2 + x[None, :] ** 2
    Ex = np.where(r2 <= x.max() ** 2, np.exp(-1j * k * np.sqrt(r2 + f * f)), 0)
    zero = np.zeros_like(Ex)
    _lib.check(ctx.lib.ml_fields_upload(ctx.handle, n, n, *[_lib.dptr(_lib.c128(a)) for a in (Ex, zero, zero, Ex / Z)]))
    return x, f


def patch_on_pitch(x, m):
    """m targets per axis on the aperture's pitch around its centre, 0.3 (x) and 0.6 (y) of a pitch off its lattice"""
    import numpy as np
    d = x[1] - x[0]
    first = (x.size - m) // 2
    return x[0] + (first + 0.3) * d + np.arange(m) * d, x[0] + (first + 0.6) * d + np.arange(m) * d


def fft_against_direct(quick):
    import numpy as np

    from metalens_amd import _lib
    from metalens_amd.propagate import PlanePropagator
    ctx = _lib.default_context()
    wl, n_glass = 580e-9, 1.46
    cases = [(1024, 64, True)] if quick else [(2048, 64, True), (4096, 64, True), (4096, 256, True), (4096, 4096, False)]
    resident = None
    for n, m, with_direct in cases:
        if resident != n:
            x, f = converging_wave(ctx, n, wl, n_glass)
            resident = n
        tx, ty = patch_on_pitch(x, m)
        for want_h in (True, False):
            t0 = time.perf_counter()
            p = PlanePropagator(x, x, wl, n_glass, tx, ty, f, want_h=want_h, ctx=ctx, method='fft')
            _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))
            ctx.sync()
            ms_first = (time.perf_counter() - t0) * 1e3
            ms_fft = best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0)))
            info = p.plan_info()
            line = {'case': '%d^2 -> %d^2 on the pitch' % (n, m), 'fields': 'E+H' if want_h else 'E', 'method': 'fft',
                    'ms': round(ms_fft, 3), 'ms_first': round(ms_first, 3), 'L': [info['Lx'], info['Ly']],
                    'workspace_MiB': round(info['workspace_bytes'] / 2 ** 20, 1)}
            if with_direct:
                got = p._download(None)
                pd = PlanePropagator(x, x, wl, n_glass, tx, ty, f, want_h=want_h, ctx=ctx)
                ms_direct = best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate(ctx.handle, pd.Z0)))
                want = pd._download(None)
                diff = max(np.abs(got[c] - want[c]).max() for c in ('Ex', 'Ey', 'Ez')) / max(np.abs(want[c]).max() for c in ('Ex', 'Ey', 'Ez'))
                line.update(ms_direct=round(ms_direct, 3), speedup=round(ms_direct / ms_fft, 2),
                            crossover_targets=int(np.ceil(ms_fft / (ms_direct / (m * m)))),
                            max_E_difference_of_the_methods=float('%.3e' % diff))
            print(json.dumps(line), flush=True)


def fft_long(quick, n=8192):
    import numpy as np

    from metalens_amd import _lib
    from metalens_amd.propagate import PlanePropagator
    ctx = _lib.default_context()
    wl, n_glass = 580e-9, 1.46
    x, f = converging_wave(ctx, n, wl, n_glass)
    one_target = x[:1] + 0.3 * (x[1] - x[0])
    for m in (64,) if quick else (64, 4096):
        tx, ty = patch_on_pitch(x, m)
        for want_h in (True,) if quick else (True, False):
            line = {'case': '%d^2 -> %d^2 on the pitch' % (n, m), 'fields': 'E+H' if want_h else 'E', 'method': 'fft-long'}

            def first_pass():
                t0 = time.perf_counter()
                p = PlanePropagator(x, x, wl, n_glass, tx, ty, f, want_h=want_h, ctx=ctx, method='fft-long')
                _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))
                ctx.sync()
                return p, (time.perf_counter() - t0) * 1e3
            # a direct plan releases the workspace of an FFT plan: the first pass after it reserves it again
            PlanePropagator(x, x, wl, n_glass, one_target, one_target, f, want_h=want_h, ctx=ctx)
            try:
                p, ms_cold = first_pass()
            except _lib.MetalensHipError as e:
                line['error'] = str(e)
                print(json.dumps(line), flush=True)
                continue
            p, ms_first = first_pass()
            ms = best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0)))
            info = p.plan_info()
            line.update(ms=round(ms, 3), ms_first=round(ms_first, 3), ms_first_with_workspace=round(ms_cold, 3),
                        ms_workspace_hipMalloc=round(ms_cold - ms_first, 3), L=[info['Lx'], info['Ly']],
                        workspace_MiB=round(info['workspace_bytes'] / 2 ** 20, 1))
            if m == 64 and want_h and not quick:
                got = p._download(None)
                pd = PlanePropagator(x, x, wl, n_glass, tx, ty, f, want_h=want_h, ctx=ctx)

                def one():
                    t0 = time.perf_counter()
                    _lib.check(ctx.lib.ml_propagate(ctx.handle, pd.Z0))
                    ctx.sync()
                    return (time.perf_counter() - t0) * 1e3
                ms_direct = min(one(), one())
                want = pd._download(None)
                diff = max(np.abs(got[c] - want[c]).max() for c in ('Ex', 'Ey', 'Ez')) / max(np.abs(want[c]).max() for c in ('Ex', 'Ey', 'Ez'))
                line.update(ms_direct=round(ms_direct, 3), speedup=round(ms_direct / ms, 2),
                            crossover_targets=int(np.ceil(ms / (ms_direct / (m * m)))),
                            max_E_difference_of_the_methods=float('%.3e' % diff))
            print(json.dumps(line), flush=True)


def fft_tiled(n, m, tile=None, other=None, want_hs=(True, False), direct_targets=0):
    """``PlanePropagator(method='fft-tiled')`` for n^2 -> m^2 on the pitch: the cached pass, plan + first pass, the
    workspace, and against ``other`` ('fft' or 'fft-long') on the same targets its cached pass and max |dE| / max |E|.
    direct_targets t > 0: the direct sum on a t x t corner of the patch instead - its time per target, and the
    difference of the methods there"""
    import numpy as np

    from metalens_amd import _lib
    from metalens_amd.propagate import PlanePropagator
    ctx = _lib.default_context()
    wl, n_glass = 580e-9, 1.46
    x, f = converging_wave(ctx, n, wl, n_glass)
    tx, ty = patch_on_pitch(x, m)
    keys = ('Ex', 'Ey', 'Ez')
    for want_h in want_hs:
        line = {'case': '%d^2 -> %d^2 on the pitch' % (n, m), 'fields': 'E+H' if want_h else 'E', 'method': 'fft-tiled'}
        if os.environ.get('ML_GRID_TILE_BATCH_MIB'):
            line['batch_MiB'] = int(os.environ['ML_GRID_TILE_BATCH_MIB'])
        try:
            t0 = time.perf_counter()
            p = PlanePropagator(x, x, wl, n_glass, tx, ty, f, want_h=want_h, ctx=ctx, method='fft-tiled', tile=tile)
            _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))
            ctx.sync()
            ms_first = (time.perf_counter() - t0) * 1e3
        except _lib.MetalensHipError as e:
            line['error'] = str(e)
            print(json.dumps(line), flush=True)
            continue
        ms = best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0)))
        info = p.plan_info()
        got = p._download(None)
        # (the plan's own bytes: the buffer only grows, and an earlier plan of the process may have left it larger)
        planes = 8 * info['tiles'][0] * info['tiles'][1] + 4 * info['batch'] + (6 if want_h else 3)
        line.update(ms=round(ms, 3), ms_first=round(ms_first, 3), L=[info['Lx'], info['Ly']], tiles=list(info['tiles']),
                    batch=info['batch'], workspace_MiB=round(planes * info['Lx'] * info['Ly'] * 16 / 2 ** 20, 1))
        if other:
            try:
                po = PlanePropagator(x, x, wl, n_glass, tx, ty, f, want_h=want_h, ctx=ctx, method=other)
                ms_other = best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate(ctx.handle, po.Z0)))
                want, io = po._download(None), po.plan_info()
                diff = max(np.abs(got[c] - want[c]).max() for c in keys) / max(np.abs(want[c]).max() for c in keys)
                line.update(other=other, ms_other=round(ms_other, 3), speedup=round(ms_other / ms, 2),
                            workspace_MiB_other=round(io['workspace_bytes'] / 2 ** 20, 1),
                            max_E_difference_of_the_methods=float('%.3e' % diff))
            except _lib.MetalensHipError as e:
                line['error_other'] = str(e)
        if direct_targets:
            t = direct_targets
            pd = PlanePropagator(x, x, wl, n_glass, tx[:t], ty[:t], f, want_h=want_h, ctx=ctx)
            t0 = time.perf_counter()
            _lib.check(ctx.lib.ml_propagate(ctx.handle, pd.Z0))
            ctx.sync()
            ms_direct = (time.perf_counter() - t0) * 1e3
            want = pd._download(None)
            diff = max(np.abs(got[c][:t, :t] - want[c]).max() for c in keys) / max(np.abs(got[c]).max() for c in keys)
            line.update(direct_targets=t * t, ms_direct_per_target=round(ms_direct / (t * t), 4),
                        crossover_targets=int(np.ceil(ms / (ms_direct / (t * t)))),
                        max_E_difference_of_the_methods_on_them=float('%.3e' % diff))
        print(json.dumps(line), flush=True)


def fft_fine(n, m, s, with_direct=True):
    """``PlanePropagator(method='fft-fine')`` for n^2 -> m^2 fine targets at the pitch / s around the focus, E + H: kernel
    spectra kept and filled in every pass - ms of a pass (timed as above), ms_first = plan + first pass, the plan's
    workspace - against the loop of s^2 'fft-tiled' propagators, one per lattice, each planned and run once (what gives
    the same targets without this method: every plan fills its kernel spectra anew, every pass transforms the currents
    again; best of two loops), and against one direct pass on the same targets"""
    import numpy as np

    from metalens_amd import _lib
    from metalens_amd.propagate import PlanePropagator
    ctx = _lib.default_context()
    wl, n_glass = 580e-9, 1.46
    x, f = converging_wave(ctx, n, wl, n_glass)
    d = x[1] - x[0]
    first = (x.size - m // s) // 2
    tx, ty = x[0] + (first + 0.3) * d + np.arange(m) * d / s, x[0] + (first + 0.6) * d + np.arange(m) * d / s
    keys = ('Ex', 'Ey', 'Ez')
    got = {}
    for cached in (True, False):
        line = {'case': '%d^2 -> %d^2 at pitch / %d' % (n, m, s), 'fields': 'E+H', 'method': 'fft-fine',
                'cache_kernels': cached}
        if os.environ.get('ML_GRID_FINE_PAIR'):
            line['lattices_per_contraction'] = int(os.environ['ML_GRID_FINE_PAIR'])
        try:
            t0 = time.perf_counter()
            p = PlanePropagator(x, x, wl, n_glass, tx, ty, f, ctx=ctx, method='fft-fine', subsample=(s, s), cache_kernels=cached)
            _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))
            ctx.sync()
            ms_first = (time.perf_counter() - t0) * 1e3
        except _lib.MetalensHipError as e:
            line['error'] = str(e)
            print(json.dumps(line), flush=True)
            continue
        ms = best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0)))
        info = p.plan_info()
        got[cached] = p._download(None)
        # (the plan's own bytes: the buffer only grows, and an earlier plan of the process may have left it larger)
        tiles, lattices = info['tiles'][0] * info['tiles'][1], min(s, m) ** 2
        planes = (8 * lattices * tiles if cached else 16 * info['batch']) + 4 * tiles + 12
        line.update(ms=round(ms, 3), ms_first=round(ms_first, 3), L=[info['Lx'], info['Ly']], tiles=list(info['tiles']),
                    lattices=lattices, lattice_targets=list(info['lattice_targets']), batch=info['batch'],
                    workspace_MiB=round(planes * info['Lx'] * info['Ly'] * 16 / 2 ** 20, 1))
        if not cached and True in got:
            line['same_bits_as_cached'] = all(np.array_equal(got[True][c], got[False][c]) for c in got[True])
        print(json.dumps(line), flush=True)
    if not got:
        return
    fine = got[True] if True in got else got[False]

    def loop():
        t0 = time.perf_counter()
        for a in range(min(s, m)):
            for b in range(min(s, m)):
                q = PlanePropagator(x, x, wl, n_glass, tx[a::s], ty[b::s], f, ctx=ctx, method='fft-tiled')
                _lib.check(ctx.lib.ml_propagate(ctx.handle, q.Z0))
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3
    line = {'case': '%d^2 -> %d^2 at pitch / %d' % (n, m, s), 'fields': 'E+H', 'method': "loop of %d 'fft-tiled' plans" % min(s, m) ** 2,
            'ms': round(min(loop(), loop()), 3)}
    print(json.dumps(line), flush=True)
    if with_direct:
        pd = PlanePropagator(x, x, wl, n_glass, tx, ty, f, ctx=ctx)

        def one():
            t0 = time.perf_counter()
            _lib.check(ctx.lib.ml_propagate(ctx.handle, pd.Z0))
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3
        ms_direct = min(one(), one())
        want = pd._download(None)
        diff = max(np.abs(fine[c] - want[c]).max() for c in keys) / max(np.abs(want[c]).max() for c in keys)
        print(json.dumps({'case': '%d^2 -> %d^2 at pitch / %d' % (n, m, s), 'fields': 'E+H', 'method': 'direct',
                          'ms': round(ms_direct, 3), 'max_E_difference_to_fft-fine': float('%.3e' % diff)}), flush=True)


def fft_stack(n, m, s, nz, rows):
    """``PlanePropagator(method='fft-stack')`` for nz planes of m^2 fine targets at the pitch / s around the focus of the
    converging wave, E + H, planes 16 wavelengths around the focal length.  Rows (each timed by ``best_ms`` after a
    priming pass): 'stack-streamed' and 'stack-cached' - a pass on the plan, ms_first = plan + first pass, the plan's
    workspace; 'loop' - one 'fft-fine' propagator per z, planned and passed, with the default cache_kernels=True - the way
    the volume is computed without this method - and 'loop-streamed', the same with cache_kernels=False; 'fine' - a pass of
    one cached 'fft-fine' plan at the first z"""
    import numpy as np

    from metalens_amd import _lib
    from metalens_amd.propagate import PlanePropagator
    ctx = _lib.default_context()
    wl, n_glass = 580e-9, 1.46
    x, f = converging_wave(ctx, n, wl, n_glass)
    d = x[1] - x[0]
    first = (x.size - m // s) // 2
    tx, ty = x[0] + (first + 0.3) * d + np.arange(m) * d / s, x[0] + (first + 0.6) * d + np.arange(m) * d / s
    z = f + (np.linspace(-8, 8, nz) if nz > 1 else np.zeros(1)) * wl
    case = '%d^2 -> %d x %d^2 at pitch / %d' % (n, nz, m, s)
    for row in rows:
        line = {'case': case, 'fields': 'E+H', 'row': row}
        if row in ('stack-streamed', 'stack-cached'):
            cached = row == 'stack-cached'
            try:
                t0 = time.perf_counter()
                p = PlanePropagator(x, x, wl, n_glass, tx, ty, z, ctx=ctx, method='fft-stack', subsample=(s, s), cache_kernels=cached)
                _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0))
                ctx.sync()
                ms_first = (time.perf_counter() - t0) * 1e3
            except _lib.MetalensHipError as e:
                line['error'] = str(e)
                print(json.dumps(line), flush=True)
                continue
            ms = best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate(ctx.handle, p.Z0)))
            info = p.plan_info()
            out = p._download(None)
            I = sum(np.abs(out[c]) ** 2 for c in ('Ex', 'Ey', 'Ez'))
            tiles, layers = info['tiles'][0] * info['tiles'][1], nz * min(s, m) ** 2
            planes = (8 * layers * tiles if cached else 16 * info['batch']) + 4 * tiles + 12   # (the plan's own bytes)
            line.update(ms=round(ms, 3), ms_first=round(ms_first, 3), L=[info['Lx'], info['Ly']], tiles=list(info['tiles']),
                        layers=layers, batch=info['batch'], workspace_MiB=round(planes * info['Lx'] * info['Ly'] * 16 / 2 ** 20, 1),
                        brightest_plane=int(np.argmax(I.reshape(nz, -1).max(axis=1))))
        elif row in ('loop', 'loop-streamed'):
            def loop():
                for zp in z:
                    q = PlanePropagator(x, x, wl, n_glass, tx, ty, zp, ctx=ctx, method='fft-fine', subsample=(s, s),
                                        cache_kernels=row == 'loop')
                    _lib.check(ctx.lib.ml_propagate(ctx.handle, q.Z0))
            line.update(method="loop of %d 'fft-fine' plans, planned and passed" % nz, cache_kernels=row == 'loop',
                        ms=round(best_ms(ctx, loop), 3))
        elif row == 'fine':
            q = PlanePropagator(x, x, wl, n_glass, tx, ty, z[0], ctx=ctx, method='fft-fine', subsample=(s, s))
            line.update(method="one cached 'fft-fine' pass", ms=round(best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate(ctx.handle, q.Z0))), 3))
            # at this size a streamed pair is filled a layer per launch (csrc/propagate_grid.h grid_stack_fill_layers), which
            # no case of the tests reaches: plane 0 of a streamed stack of two planes against this plan, bit for bit
            fine = q._download(None)
            two = PlanePropagator(x, x, wl, n_glass, tx, ty, [z[0], z[0] + wl], ctx=ctx, method='fft-stack', subsample=(s, s),
                                  cache_kernels=False).propagate()
            line['same_bits_as_plane_0_of_a_streamed_stack'] = all(np.array_equal(two[c][0], fine[c]) for c in fine)
        else:
            raise SystemExit('--row: stack-streamed, stack-cached, loop, loop-streamed or fine, got %r' % row)
        print(json.dumps(line), flush=True)


def fft_three_sets(n=2048, m=64):
    """the three sets of a synthesised x, y, z batch through ONE ml_propagate_sets call of an 'fft' plan"""
    import math

    import numpy as np

    import metalens_amd as ma
    from metalens_amd import _lib, layout, synthetic
    from metalens_amd.nearfield import nearfield_params
    from metalens_amd.propagate import PlanePropagator
    ctx = _lib.default_context()
    wl = 580e-9
    x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
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
    tx, ty = patch_on_pitch(x, m)
    for want_h in (True, False):
        p = PlanePropagator(x, x, wl, n_glass, tx, ty, f, want_h=want_h, ctx=ctx, method='fft')
        ms_one = best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate_sets(ctx.handle, p.Z0, 0, 1)))
        ms_three = best_ms(ctx, lambda: _lib.check(ctx.lib.ml_propagate_sets(ctx.handle, p.Z0, 0, 3)))
        print(json.dumps({'case': '%d^2 -> %d^2 on the pitch, x + y + z dipoles' % (n, m), 'fields': 'E+H' if want_h else 'E',
                          'method': 'fft', 'ms_one_pass_of_three_sets': round(ms_three, 3), 'ms_one_set': round(ms_one, 3),
                          'ratio_to_three_single_passes': round(ms_three / (3 * ms_one), 4)}), flush=True)


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    if _option('--method') == 'fft-stack':
        n, m = (int(v) for v in _option('--case', '1024,64' if '--quick' in sys.argv else '4096,64').split(','))
        row = _option('--row')
        fft_stack(n, m, int(_option('--subsample', 2)), int(_option('--planes', 8)),
                  (row,) if row else ('stack-streamed', 'stack-cached', 'loop', 'fine'))
        return
    if _option('--method') == 'fft-fine':
        n, m = (int(v) for v in _option('--case', '1024,64' if '--quick' in sys.argv else '4096,64').split(','))
        fft_fine(n, m, int(_option('--subsample', 2)), with_direct='--no-direct' not in sys.argv)
        return
    if _option('--method') == 'fft-tiled':
        n, m = (int(v) for v in _option('--case', '1024,64' if '--quick' in sys.argv else '4096,64').split(','))
        tile = int(_option('--tile', 0))
        fft_tiled(n, m, tile=(tile, tile) if tile else None, other=_option('--against'),
                  want_hs=(True,) if '--eh-only' in sys.argv else (True, False), direct_targets=int(_option('--direct', 0)))
        return
    if '--method' in sys.argv and sys.argv[sys.argv.index('--method') + 1] == 'fft-long':
        fft_long('--quick' in sys.argv)
        return
    if '--method' in sys.argv and sys.argv[sys.argv.index('--method') + 1] == 'fft':
        quick = '--quick' in sys.argv
        fft_against_direct(quick)
        fft_three_sets(*((1024, 64) if quick else ()))
        return
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
