"""The table of pruned-FFT cases (tests/fft_cases.py) against the launch rules themselves: every row's expected
kernels and launch counts equal what tools/transform_route prints for the row's facts (csrc/transform_route.h
zfft_axis_rule, interleave_block_of, zfft_launch_rule: the functions plan_fft_axis, interleave_block, zfft_run,
zfft_run_tiles and zfft_run_interleaved call), the table reaches every production instantiation zfft.hip's launch code
names, the rules' thresholds sit where DESIGN.md 4.2 says, every axis row's thread programme matches a long-double DFT
on the host, and the oracle's own rounding on each row's inputs stays a tenth of the GPU tolerance.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import fft_cases
from fft_cases import AUTO, STREAMED
from test_transform_route import INTERLEAVED, ROOT, fft_plan, route  # noqa: F401  (route: builds and runs the tool)

CSRC = os.path.join(ROOT, 'metalens_amd', 'csrc')
TOL = 1e-12   # tests/test_gpu_fft.py


def _kernels(r):
    return (r['stage1_kernel'], int(r['stage1_launches']), r['stage2_kernel'], int(r['stage2_launches']))


@pytest.mark.parametrize('name', sorted(fft_cases.ROWS))
def test_every_row_takes_the_kernels_it_names(route, name):
    row = fft_cases.ROWS[name]
    for piece in fft_cases.pieces(row):
        r = route(**fft_cases.plan_facts(row, piece))
        assert (r['stage1'], r['y.ok'], r['x.ok']) == ('fft', '1', '1'), (name, piece)
        assert _kernels(r) == row.expect, (name, piece)
        if row.expect[2] == 'zfft/tiles':
            assert (r['g_layout'], r['stage2']) == ('tiled', 'fft_tiles') and row.expect[0].split('/')[3] == 'p4'
        elif row.shard != 'whole' and row.shard[0] == 'interleaved':
            assert (r['g_layout'], r['stage2']) == ('row_major', 'interleaved')
            assert (int(r['block']), int(r['stuff'])) == fft_cases.INTERLEAVE[name]
        else:   # ('fft-streamed' stores G transposed whatever the size; these apertures are small for `auto` to)
            assert (r['g_layout'], r['stage2']) == ('transposed' if row.method == STREAMED else 'row_major', 'fft')


@pytest.mark.parametrize('name', sorted(fft_cases.ROWS))
def test_every_row_sits_on_the_lattice_the_table_says(route, name):
    """the lattice facts the table hands the tool (fft_cases.n_eff, jstep, the first bin) are what plan_fft_axis
    derives from the row's own axis and direction grid: csrc/transform_route.h zfft_axis_lattice, run by the tool on
    the very doubles the GPU test passes"""
    row = fft_cases.ROWS[name]
    x, y, ux, uy = fft_cases.axes(row)
    for ax, pos, u in ((row.x, x, ux), (row.y, y, uy)):
        args = [str(ax.n), float(pos[1] - pos[0]).hex(), float(fft_cases.WL).hex(), float(fft_cases.N_GLASS).hex()]
        res = subprocess.run([route.exe, 'lattice'] + args + [float(v).hex() for v in u], capture_output=True, text=True,
                             timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        got = dict(kv.split('=') for kv in res.stdout.split())
        want = dict(ok='1', N_eff=str(fft_cases.n_eff(ax)), j0=str(ax.j0), jstep=str(fft_cases.jstep(ax)), N_plain=str(ax.N))
        assert got == want, (name, ax)


def production_zfft():
    """{stage: set of names} of the kernel instantiations zfft.hip's launch code names: the launch_one<...> lines,
    the ML_PASS(...) lines times the three passes ML_PASS hands out, the zfft_multi_kernel<...> launches and the
    three kernels without template arguments"""
    text = open(os.path.join(CSRC, 'zfft.hip')).read()
    ip_max = int(re.search(r'#define ML_ZFFT_IP (\d+)', open(os.path.join(CSRC, 'transform_route.h')).read()).group(1))
    out = {1: set(), 2: set()}
    stage_of = {1: (1,), 2: (2,), 3: (2,), 4: (1,)}
    ones = re.findall(r'return launch_one<(\d+), \d+, \d+, (\d)>\(', text)
    for r3t, p in ones:
        name = 'zfft/one/R%s/p%s%s' % (r3t, p, '/ip' if 0 < int(r3t) <= ip_max else '')
        # (the PASS 1 instantiations also run stage 2 over a transposed G where PASS 3 has none: 3 / 4 residues)
        for stage in stage_of[int(p)]:
            out[stage].add(name)
    body = text[text.index('#define ML_PASS('):text.index('#undef ML_PASS')]
    pass_ids = sorted(set(re.findall(r'launch_pass<R, PP, NBB, 2, (\d)>', body)))
    groups = re.findall(r'^\s*ML_PASS\((\d+), (\d+), (\d+)\)', body, flags=re.M)
    for r3p, p, _nb in groups:
        for ps in pass_ids:
            for stage in stage_of[int(ps)]:
                out[stage].add('zfft/pass/R%sx%s/p%s' % (r3p, p, ps))
    multis = set(re.findall(r'hipLaunchKernelGGL\(zfft_multi_kernel<(\d)>', text))
    for ps in multis:
        out[int(ps)].add('zfft/multi/p' + ps)
    for single in ('tiles', 'interleaved', 'cols128'):
        assert len(re.findall(r'hipLaunchKernelGGL\(zfft_%s_kernel,' % single, text)) == 1, single
        out[2].add('zfft/' + single)
    assert pass_ids == ['1', '2', '3'], pass_ids
    count = len(ones) + len(groups) * len(pass_ids) + len(multis) + 3
    return out, count


def test_the_table_reaches_every_production_kernel():
    production, count = production_zfft()
    assert count == 28 and len(production[1] | production[2]) == 28
    reached = fft_cases.reached()
    for stage in (1, 2):
        missing = sorted(production[stage] - reached[stage])
        assert not missing, 'no row of tests/fft_cases.py runs %s in stage %d' % (missing, stage)
        unknown = sorted(k for k in reached[stage] - production[stage]
                         if not (stage == 2 and k.endswith(('/p1', '/p1/ip'))))   # (PASS 1 over a transposed G)
        assert not unknown, 'tests/fft_cases.py names kernels zfft.hip does not launch: %s' % unknown
    # every shard kind through PASS 2, PASS 3, the tiles and an axis in sub-sequences
    rows = fft_cases.ROWS.values()
    for what, pick in (('p2', lambda r: '/p2' in r.expect[2] and r.expect[3] == 1), ('p3', lambda r: '/p3' in r.expect[2]),
                       ('tiles', lambda r: r.expect[2] == 'zfft/tiles'), ('split', lambda r: r.expect[3] > 1)):
        kinds = {r.shard if r.shard == 'whole' else r.shard[0] for r in rows if pick(r)}
        assert kinds >= {'whole', 'blocks', 'mirrored'}, what
    assert {v[1] for v in fft_cases.INTERLEAVE.values()} == {2, 4, 8}
    # the edges every family gets: bins above the thread count, a window without bin 0, one that wraps round the
    # lattice's end, one sample short of the lattice (of the axis the kernel transforms)
    named = fft_cases.ROWS.items()
    for fam, threads in (('zfft/one/', None), ('zfft/pass/', 512), ('zfft/multi/', 64), ('zfft/tiles', None),
                         ('zfft/interleaved', 64), ('zfft/cols128', 64)):
        axes = [ax for _n, r in named for ax, k in ((r.y, r.expect[0]), (r.x, r.expect[2])) if k.startswith(fam)]
        if threads:
            assert any(ax.M > threads for ax in axes) and any(ax.M < threads for ax in axes), fam
        if fam not in ('zfft/interleaved', 'zfft/cols128', 'zfft/multi/'):
            assert any(ax.j0 > 0 and ax.j0 + ax.M <= ax.N for ax in axes), fam      # no bin 0
            assert any(ax.j0 + ax.M > ax.N for ax in axes), fam                     # wraps
            assert any(ax.n == fft_cases.n_eff(ax) - 1 for ax in axes), fam         # N_eff - 1 samples
    # a stage-1 launch of 4 rows (a one-row block) through the one-level, the pass and the multi kernel
    few = {r.expect[0].split('/')[1] for r in rows if r.shard == ('blocks', 1)}
    assert few == {'one', 'pass', 'multi'}
    assert {fft_cases.jstep(r.y) for r in rows} >= {1, 2, 4, 16}


def _axis(route, n, m, method=AUTO, jstep=1, other='y', **more):
    """route of a tiny aperture with one axis on the lattice of n samples and m wanted bins"""
    small = dict(nx_total=5, nxl=5, mx=4, x_dot_lattice=256) if other == 'y' else \
        dict(ny=12, my=5, y_dot_lattice=256)
    this = dict(ny=n, my=m, y_dot_lattice=n, y_dot_jstep=jstep) if other == 'y' else \
        dict(nx_total=n, nxl=n, mx=m, x_dot_lattice=n, x_dot_jstep=jstep)
    facts = dict(method=method, **small, **this)
    facts.update(more)
    return route(**facts)


def test_pass_kernel_thresholds(route):
    # 8192 samples: two passes of 16 residues up to 512 bins, the one-level kernel beyond
    assert _kernels(_axis(route, 8192, 512))[:2] == ('zfft/pass/R16x2/p1', 1)
    assert _kernels(_axis(route, 8192, 513))[:2] == ('zfft/one/R32/p1', 1)
    # 16384 samples: two passes of 32 residues up to 1024 bins, two sub-sequences beyond
    r = _axis(route, 16384, 1024)
    assert _kernels(r)[:2] == ('zfft/pass/R32x2/p1', 1) and (r['y.split'], r['y.passes']) == ('1', '2')
    r = _axis(route, 16384, 1025)
    assert _kernels(r)[:2] == ('zfft/one/R32/p1', 2) and (r['y.split'], r['y.passes']) == ('2', '0')
    r = _axis(route, 16384, 512)   # (the sub-sequences of a longer lattice take the 8192-sample default)
    assert _kernels(r)[:2] == ('zfft/pass/R32x2/p1', 1)
    assert _kernels(_axis(route, 3 * 8192, 512))[:2] == ('zfft/pass/R16x2/p1', 3)
    assert _kernels(_axis(route, 3 * 8192, 513))[:2] == ('zfft/one/R32/p1', 3)
    for other, p in (('y', 1), ('x', 2)):
        k = _kernels(_axis(route, 8192, 512, other=other))
        assert k[0 if other == 'y' else 2] == 'zfft/pass/R16x2/p%d' % p


def test_multi_and_in_place_thresholds(route):
    assert _kernels(_axis(route, 512, 64))[0] == 'zfft/multi/p1'
    assert _kernels(_axis(route, 768, 64))[0] == 'zfft/one/R0/p1'
    assert _axis(route, 512, 64)['stage1_threads'] == _axis(route, 256, 64)['stage1_threads'] == '64'
    assert _kernels(_axis(route, 4096, 64))[0] == 'zfft/one/R16/p1/ip'
    assert _kernels(_axis(route, 17 * 256, 64))[0] == 'zfft/one/R0/p1'
    assert _kernels(_axis(route, 8192, 600))[0] == 'zfft/one/R32/p1'   # (32 residues: not in place)
    assert _axis(route, 17 * 256, 64)['stage1_threads'] == '272'


def test_auto_leaves_lattices_padded_more_than_four_fold(route):
    r = _axis(route, 3840, 64, jstep=4)
    assert (r['y.ok'], r['stage1']) == ('1', 'fft')
    r = _axis(route, 2 * 3840, 64, jstep=8, fold=1, fold_S=32)
    assert (r['y.ok'], r['stage1']) == ('0', 'folded')
    r = _axis(route, 2 * 3840, 64, jstep=8, method=STREAMED)
    assert (r['y.ok'], r['stage1'], r['stage1_kernel']) == ('1', 'fft', 'zfft/one/R0/p1')


def test_tile_thresholds(route):
    def streamed(ny, my, mx, nx=768):
        r = route(method=STREAMED, nx_total=nx, nxl=nx, ny=ny, mx=mx, my=my, y_dot_lattice=ny, x_dot_lattice=nx)
        return r['g_layout'], r['stage1_kernel'], r['stage2_kernel']
    assert streamed(512, 8, 64) == ('transposed', 'zfft/multi/p1', 'zfft/one/R0/p1')      # 2 residues along y
    assert streamed(768, 8, 64) == ('tiled', 'zfft/one/R0/p4', 'zfft/tiles')              # 3
    assert streamed(4096, 8, 64) == ('tiled', 'zfft/one/R16/p4/ip', 'zfft/tiles')         # 16
    assert streamed(17 * 256, 8, 64) == ('transposed', 'zfft/one/R0/p1', 'zfft/one/R0/p1')
    assert streamed(1024, 12, 64) == ('transposed', 'zfft/one/R4/p1/ip', 'zfft/one/R0/p1')  # my % 8
    assert streamed(1024, 16, 512, 4096) == ('tiled', 'zfft/one/R4/p4/ip', 'zfft/tiles')
    assert streamed(1024, 16, 513, 4096) == ('transposed', 'zfft/one/R4/p1/ip', 'zfft/one/R16/p3/ip')
    assert streamed(1024, 16, 512, 8192) == ('tiled', 'zfft/one/R4/p4/ip', 'zfft/tiles')   # (any residue count along x)
    assert streamed(1024, 16, 512, 16384) == ('transposed', 'zfft/one/R4/p1/ip', 'zfft/pass/R32x2/p3')   # two-pass x


def test_cols128_conditions(route):
    def inter(nx, n_lattice, world, **more):
        r = route(method=AUTO, nx_total=nx, nxl=nx // world, ny=12, mx=40, my=5, y_dot_lattice=256,
                  x_dot_lattice=n_lattice, shard=INTERLEAVED, n_ranks=world, **more)
        return r['stage2_kernel'], int(r['block']), int(r['stuff']), int(r['stage2_threads'])
    assert inter(2048, 2048, 2) == ('zfft/cols128', 8, 2, 64)
    assert inter(8192, 8192, 8) == ('zfft/cols128', 8, 2, 64)        # the 8-rank benchmark configuration
    assert inter(2000, 2048, 2) == ('zfft/cols128', 8, 2, 64)        # 125 of the 128 samples exist
    assert inter(2008, 2048, 2) == ('zfft/interleaved', 4, 1, 64)    # blocks of 4: whole 256-sample transforms
    assert inter(1000, 1024, 2) == ('zfft/interleaved', 4, 2, 64)    # 2-fold stuffed, but 4 transforms per column
    assert inter(6144, 6144, 2) == ('zfft/interleaved', 8, 2, 384)   # 8 transforms, 2-fold, but 768 samples
    assert inter(4096, 4096, 2) == ('zfft/interleaved', 8, 1, 128)
    assert inter(1024, 1024, 2) == ('zfft/interleaved', 8, 4, 128)
    assert inter(2048, 2048, 2, block=4)[0] == 'zfft/interleaved'


@pytest.fixture(scope='module')
def emulators(tmp_path_factory):
    out = tmp_path_factory.mktemp('emul')
    exes = {}
    for name in ('zfft_emul', 'zfft_tiles_emul'):
        exes[name] = str(out / name)
        subprocess.check_call(['g++', '-O2', '-std=c++17', os.path.join(ROOT, 'tools', name + '.cpp'), '-o', exes[name]])
    return exes


@pytest.mark.parametrize('key', sorted(fft_cases.axis_rows()), ids=lambda k: 'R%d-n%d-M%d-j%d-ip%d-s%d-P%d' % k)
def test_thread_programme_of_every_axis_row(emulators, key):
    """the kernel's per-thread functions, thread by thread on the host, against the long-double DFT to the tool's own
    bound (1e-13 of the largest bin)"""
    res = subprocess.run([emulators['zfft_emul']] + [str(v) for v in key], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and '-> OK' in res.stdout, (fft_cases.axis_rows()[key], res.stdout + res.stderr)


@pytest.mark.parametrize('key', sorted(fft_cases.tile_rows()), ids=lambda k: 'R%d-a%d-h%d-M%d-j%d' % k)
def test_tile_programme_of_every_tiled_row(emulators, key):
    res = subprocess.run([emulators['zfft_tiles_emul']] + [str(v) for v in key], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and '-> OK' in res.stdout, (fft_cases.tile_rows()[key], res.stdout + res.stderr)


def _axis_sums(ax, pos_step, u):
    """worst difference, relative to the largest sum, between the per-axis sums the oracle forms from the direction
    grid as given (float64 values, farfield_oracle.axis_twiddles) and the same sums over the exact lattice phases
    -(n - c) (j + j0) / N turns, reduced as integers and evaluated in long double"""
    from oracle import farfield_oracle
    rng = np.random.default_rng(ax.n + ax.M)
    f = rng.standard_normal(ax.n) + 1j * rng.standard_normal(ax.n)
    given = farfield_oracle.axis_twiddles(ax.n, pos_step, u, fft_cases.WL, fft_cases.N_GLASS) @ f
    k = np.arange(ax.n, dtype=np.int64) - (ax.n - ax.n // 2)
    j = np.arange(ax.M, dtype=np.int64) + ax.j0
    turns = ((j[:, None] * k[None, :]) % ax.N).astype(np.longdouble) / np.longdouble(ax.N)
    ang = -2 * np.pi * np.longdouble(1) * turns
    fl = f.real.astype(np.longdouble), f.imag.astype(np.longdouble)
    c, s = np.cos(ang), np.sin(ang)
    re, im = c @ fl[0] - s @ fl[1], c @ fl[1] + s @ fl[0]
    err = np.maximum(np.abs(re - given.real), np.abs(im - given.imag)).max()
    return float(err / np.hypot(re, im).max())


@pytest.mark.parametrize('name', sorted(fft_cases.ROWS))
def test_the_oracle_is_ten_times_finer_than_the_tolerance_on_every_row(name):
    """The oracle sums phases of the axis arrays and direction grids as given; the kernels sum the lattice's.  Where
    the grid's half-ulps, times the turns at the outermost sample, come near the tolerance the comparison measures
    the inputs (tests/mixed_cases.py): every row's inputs keep that a tenth of TOL, per axis."""
    row = fft_cases.ROWS[name]
    x, y, ux, uy = fft_cases.axes(row)
    for ax, pos, u in ((row.x, x, ux), (row.y, y, uy)):
        worst = _axis_sums(ax, pos[1] - pos[0], u)
        assert worst <= TOL / 10, (name, ax, worst)


def test_the_resident_window_has_rows_outside_the_lens(route):
    """what the resident case of test_gpu_fft_cases.py is chosen for, checked on the oracle's near field (no kernel
    runs here): rows at both ends of the window lie wholly outside the lens circle, so both FFT stages work on a
    trimmed row range with a non-zero offset into G; and its three direction grids take the three layouts"""
    import test_gpu_fft_cases as gpu
    _lens, x, y, _ux, _src, nf = gpu.resident_case()
    lit = np.any([f != 0 for f in nf[:4]], axis=0).any(axis=1)           # [row]
    lo, hi = np.flatnonzero(lit)[[0, -1]]
    assert 8 < lo and hi < len(x) - 9 and lit[lo:hi + 1].all()
    assert lo % 8 != 0 and (hi + 1 - lo) % 8 != 0                        # (no whole 8-row patches either)
    for layout, (method, my) in gpu.RESIDENT_LAYOUTS.items():
        r = route(method={'auto': AUTO, 'fft-streamed': STREAMED}[method], nx_total=len(x), nxl=len(x), ny=len(y),
                  mx=gpu.RESIDENT_MX, my=my, y_dot_lattice=len(y), x_dot_lattice=256, row_first=1, trim_lo=int(lo),
                  trim_hi=int(hi) + 1)
        assert (r['g_layout'], r['trim_lo'], r['trim_hi']) == (layout, str(lo), str(hi + 1))
