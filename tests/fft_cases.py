"""The cases of the pruned FFT on lattices of 256 R3 samples (csrc/zfft.hip, DESIGN.md 4.2: what `auto` takes for the
benchmark and for every default grid) that the suite runs, in one table: the aperture, per axis the lattice and the
window of wanted bins, the method, the shard, and the kernel and launch count each stage is expected to take - one of
the production instantiations of zfft_kernel, zfft_pass_kernel and zfft_multi_kernel, or zfft_tiles_kernel,
zfft_interleaved_kernel, zfft_cols128_kernel, in the names tools/transform_route prints:

    zfft/one/R<R3T>/p<PASS>[/ip]   zfft_kernel<R3T, ., ., PASS, IP>; R0: the instantiation for any residue count
    zfft/pass/R<R3P>x<P>/p<PASS>   zfft_pass_kernel<R3P, P, 2, 2, PASS>
    zfft/multi/p<PASS>             zfft_multi_kernel<PASS> (256 and 512 samples)
    zfft/tiles, zfft/interleaved, zfft/cols128

PASS: 1 rows of the aperture, 2 strided columns of a row-major stage-1 result G, 3 contiguous rows of a transposed G,
4 rows of the aperture into a tiled G.  test_fft_cases.py checks `expect` against the launch rules themselves
(csrc/transform_route.h zfft_axis_rule, interleave_block_of, zfft_launch_rule: what the launchers call), that the table
reaches every production instantiation, runs every axis row's thread programme on the host, and checks that the
oracle's own rounding stays a tenth of the tolerance on each row's inputs; test_gpu_fft_cases.py runs every row on the
GPU against the oracle's direct sum.  Plain data and the inputs derived from it; no test collects from here.

The kernel of an axis depends on that axis' lattice alone, so the other axis is tiny (5 rows, or 12 samples): the
oracle's direct sum stays at a fraction of a second.  Windows far off axis stay on short lattices or short apertures:
the oracle sums phases of the direction grid as given, whose values carry half an ulp each - a phase uncertainty of
2 pi (n / 2) (|j| / N) eps / 2 at the outermost sample of n on bin j of N (tests/mixed_cases.py).
"""
import collections
import math

import numpy as np

from gemm_cases import row_block

WL, N_GLASS = 580e-9, 1.459
AUTO, STREAMED = 0, 2                       # include/metalens_hip.h ML_METHOD_AUTO, ML_METHOD_FFT_STREAMED
METHOD_NAMES = {AUTO: 'auto', STREAMED: 'fft-streamed'}

# One axis: n samples, the lattice of N samples its direction grid sits on, M wanted bins from bin j0 of that
# lattice.  A lattice that is no multiple of 256 long runs on the jstep = 256 / gcd(N, 256) times finer one.
Axis = collections.namedtuple('Axis', 'n N M j0')
# x, y: the axes (stage 2 transforms x, stage 1 y).  shard: 'whole' | ('blocks', r1) = rows [0, r1) then [r1, nx)
# accumulated | ('mirrored', world) = every rank's mirrored pairs accumulated | ('interleaved', world) = every rank's
# blocks of rows (ml_farfield_interleave_block) accumulated.
# expect = (stage 1 kernel, its launches, stage 2 kernel, its launches), of every piece of the shard.
Row = collections.namedtuple('Row', 'x y method shard expect')

XS = Axis(5, 256, 4, -2)      # the tiny axes: 20 rows of stage 1 (no multiple of 8) ...
YS = Axis(12, 256, 5, -2)     # ... 20 columns of stage 2; 256 samples: the multi kernel


def jstep(ax):
    return 256 // math.gcd(ax.N, 256)


def n_eff(ax):
    return ax.N * jstep(ax)


def _y(ax, k1, l1=1, method=AUTO):
    """the axis along y, stage 1 (PASS 1) over 20 rows"""
    return Row(XS, ax, method, 'whole', (k1, l1, 'zfft/multi/p2', 1))


def _x(ax, k2, l2=1, shard='whole'):
    """the axis along x, stage 2 over the 20 columns of a row-major G (PASS 2)"""
    return Row(ax, YS, AUTO, shard, ('zfft/multi/p1', 1, k2, l2))


def _xt(ax, k2, shard='whole'):
    """the axis along x, stage 2 over the 20 rows of a transposed G ('fft-streamed'; 256 samples along y: no tiles)"""
    return Row(ax, YS, STREAMED, shard, ('zfft/multi/p1', 1, k2, 1))


def _tiled(x, y, k1, shard='whole'):
    return Row(x, y, STREAMED, shard, (k1, 1, 'zfft/tiles', 1))


# the axes that reach each kernel of a row pass, by lattice: (axis, kernel without its pass, launches)
_AXES = {
    'r1': (Axis(256, 256, 64, -32), 'zfft/multi', 1),
    'r2': (Axis(511, 512, 100, -50), 'zfft/multi', 1),              # one sample short of the lattice, odd
    'r3': (Axis(700, 768, 100, -48), 'zfft/one/R0', 1),             # generic; 100 bins on 48 threads: the bin loop
    'r4': (Axis(1000, 1024, 128, -64), 'zfft/one/R4/ip', 1),        # 128 bins = 2 per thread, the paired form
    'r4m': (Axis(1023, 1024, 200, -100), 'zfft/one/R4/ip', 1),      # 200 bins on 64 threads: the bin loop
    'r8': (Axis(2048, 2048, 100, 7), 'zfft/one/R8/ip', 1),          # a window without bin 0, fewer bins than threads
    'r16': (Axis(4095, 4096, 300, -150), 'zfft/one/R16/ip', 1),     # 300 bins on 256 threads: own0 / own1, unpaired
    'r16w': (Axis(300, 4096, 40, 4080), 'zfft/one/R16/ip', 1),      # wraps round the lattice's end; heavily padded
    'r32': (Axis(3001, 8192, 513, -256), 'zfft/one/R32', 1),        # one bin more than the pass kernel takes
    'r32p': (Axis(3001, 8192, 512, -256), 'zfft/pass/R16x2', 1),
    'r32pn': (Axis(8191, 8192, 100, 7), 'zfft/pass/R16x2', 1),      # one sample short, a window without bin 0
    'r32pw': (Axis(300, 8192, 64, 8160), 'zfft/pass/R16x2', 1),     # wraps round the lattice's end; heavily padded
    'r64p': (Axis(4000, 16384, 1024, -512), 'zfft/pass/R32x2', 1),
    'r64s': (Axis(4000, 16384, 1025, -512), 'zfft/one/R32', 2),     # one bin more: two sub-sequences of 8192
    'r48': (Axis(12288, 12288, 100, -50), 'zfft/one/R0', 2),        # 2 x 24 residues
    'r96': (Axis(20000, 24576, 90, -45), 'zfft/pass/R16x2', 3),     # 3 x 32 residues, each in two passes
    'j2': (Axis(1920, 1920, 64, -32), 'zfft/one/R0', 1),            # on the twice finer lattice of 3840: 15 residues
    'j4': (Axis(959, 960, 70, -30), 'zfft/one/R0', 1),              # four times finer
}


def _with_pass(kernel, p):
    parts = kernel.split('/')
    return '/'.join(parts[:3] + ['p%d' % p] + parts[3:]) if parts[1] != 'multi' else kernel + '/p%d' % p


ROWS = {}
for _name, (_ax, _k, _l) in _AXES.items():
    ROWS['y-' + _name] = _y(_ax, _with_pass(_k, 1), _l)
    ROWS['x-' + _name] = _x(_ax, _with_pass(_k, 2), _l)
ROWS.update({
    # 16 times finer (400 -> 6400 samples, 25 residues): `auto` leaves it to the GEMMs, 'fft-streamed' takes it - and
    # stores G transposed, so stage 2's 256 samples run the multi kernel on contiguous rows
    'y-j16': Row(XS, Axis(400, 400, 64, -32), STREAMED, 'whole', ('zfft/one/R0/p1', 1, 'zfft/multi/p1', 1)),
    # stage 2 over a transposed G (PASS 3 exists for 8, 16, 32 residues; 3 and 4 take the PASS 1 instantiation)
    't-r3': _xt(_AXES['r3'][0], 'zfft/one/R0/p1'),
    't-r4': _xt(_AXES['r4'][0], 'zfft/one/R4/p1/ip'),
    't-r8': _xt(_AXES['r8'][0], 'zfft/one/R8/p3/ip'),
    't-r16': _xt(_AXES['r16'][0], 'zfft/one/R16/p3/ip'),
    't-r32': _xt(_AXES['r32'][0], 'zfft/one/R32/p3'),
    't-r32p': _xt(_AXES['r32p'][0], 'zfft/pass/R16x2/p3'),
    't-r64p': _xt(_AXES['r64p'][0], 'zfft/pass/R32x2/p3'),
    # a tiled G (rows g-y<residues along y>-x<residues along x>): stage 1 stores tiles of 8 bins (PASS 4), stage 2 is
    # the tile column pass.  One tile per plane (8 bins) and three; 1, 3, 5 and 16 residues along x (four per round: ragged last rounds); 512 bins, its limit
    'g-y4-x1': _tiled(Axis(256, 256, 40, -20), Axis(1000, 1024, 8, -4), 'zfft/one/R4/p4/ip'),
    'g-y8-x3': _tiled(Axis(700, 768, 33, -16), Axis(2047, 2048, 24, -12), 'zfft/one/R8/p4/ip'),
    'g-y16-x16': _tiled(Axis(50, 4096, 512, -256), Axis(4096, 4096, 24, -12), 'zfft/one/R16/p4/ip'),
    'g-y5-x5': _tiled(Axis(1270, 1280, 100, -50), Axis(1280, 1280, 8, 3), 'zfft/one/R0/p4'),
    'g-y3-x1': _tiled(Axis(9, 256, 4, -2), Axis(768, 768, 16, -8), 'zfft/one/R0/p4'),
    # the column pass with one sample short of the lattice and a window without bin 0; a window that wraps round the
    # lattice's end (on a short aperture: the oracle's own rounding, see above)
    'g-y4-x3-nobin0': _tiled(Axis(767, 768, 33, 5), Axis(1000, 1024, 8, -4), 'zfft/one/R4/p4/ip'),
    'g-y4-x5-wrap': _tiled(Axis(100, 1280, 40, 1260), Axis(1000, 1024, 8, -4), 'zfft/one/R4/p4/ip'),
    # 513 bins along x: the plain transposed G
    'g-y4-x16-513': Row(Axis(50, 4096, 513, -256), Axis(1000, 1024, 8, -4), STREAMED, 'whole',
                        ('zfft/one/R4/p1/ip', 1, 'zfft/one/R16/p3/ip', 1)),
    # 12 bins along y are no whole tiles
    'g-y4-x3-12': Row(Axis(700, 768, 33, -16), Axis(1000, 1024, 12, -6), STREAMED, 'whole',
                      ('zfft/one/R4/p1/ip', 1, 'zfft/one/R0/p1', 1)),
    # row shards, accumulated: two uneven blocks (the second from row 700 on) and mirrored pairs of three ranks,
    # through PASS 2, PASS 3, the tiles and an axis in two sub-sequences (whose first launch must add to the first
    # block's result)
    'x-r8-blocks': _x(Axis(2048, 2048, 64, -32), 'zfft/one/R8/p2/ip', shard=('blocks', 700)),
    'x-r8-mirrored': _x(Axis(2048, 2048, 64, -32), 'zfft/one/R8/p2/ip', shard=('mirrored', 3)),
    't-r8-blocks': _xt(Axis(2048, 2048, 64, -32), 'zfft/one/R8/p3/ip', shard=('blocks', 700)),
    't-r8-mirrored': _xt(Axis(2048, 2048, 64, -32), 'zfft/one/R8/p3/ip', shard=('mirrored', 3)),
    't-r32p-mirrored': _xt(_AXES['r32p'][0]._replace(n=3000), 'zfft/pass/R16x2/p3', shard=('mirrored', 3)),
    'g-y4-x3-blocks': _tiled(Axis(768, 768, 33, -16), Axis(1000, 1024, 8, -4), 'zfft/one/R4/p4/ip',
                             shard=('blocks', 300)),
    'g-y4-x3-mirrored': _tiled(Axis(768, 768, 33, -16), Axis(1000, 1024, 8, -4), 'zfft/one/R4/p4/ip',
                               shard=('mirrored', 3)),
    'x-r48-blocks': _x(_AXES['r48'][0], 'zfft/one/R0/p2', 2, shard=('blocks', 5000)),
    'x-r48-mirrored': _x(_AXES['r48'][0], 'zfft/one/R0/p2', 2, shard=('mirrored', 3)),
    # a first block of ONE row: stage 1 launches 4 rows, fewer than the 8 row sets they are dealt to (chunk = 1, most
    # of the grid idle; the multi kernel's one group of 4 rows) - one-level, pass and multi kernel
    'y-r16-blocks1': Row(XS, _AXES['r16'][0], AUTO, ('blocks', 1), ('zfft/one/R16/p1/ip', 1, 'zfft/multi/p2', 1)),
    'y-r32p-blocks1': Row(XS, _AXES['r32p'][0], AUTO, ('blocks', 1), ('zfft/pass/R16x2/p1', 1, 'zfft/multi/p2', 1)),
    'y-r1-blocks1': Row(XS, _AXES['r1'][0], AUTO, ('blocks', 1), ('zfft/multi/p1', 1, 'zfft/multi/p2', 1)),
    # interleaved shards (blocks of rows dealt round robin; the short transforms of a column in one workgroup):
    # 128-sample transforms, one wave per column
    # (200 bins on the wave's 64 lanes, 300 on 128 threads, 100 on 64: the bin loops go round; the others 40 bins)
    'i-cols128': Row(Axis(2048, 2048, 200, -100), YS, AUTO, ('interleaved', 2),
                     ('zfft/multi/p1', 1, 'zfft/cols128', 1)),
    'i-cols128-short': Row(Axis(2000, 2048, 40, 5), YS, AUTO, ('interleaved', 2),
                           ('zfft/multi/p1', 1, 'zfft/cols128', 1)),   # 125 of the 128 samples exist
    # 32 samples stuffed 8-fold, 64 stuffed 4-fold, 125 in blocks of 4 rows stuffed 2-fold
    'i-stuff8': Row(Axis(512, 512, 300, -150), YS, AUTO, ('interleaved', 2),
                    ('zfft/multi/p1', 1, 'zfft/interleaved', 1)),
    'i-stuff4': Row(Axis(1024, 1024, 40, 3), YS, AUTO, ('interleaved', 2), ('zfft/multi/p1', 1, 'zfft/interleaved', 1)),
    'i-stuff2': Row(Axis(1000, 1024, 100, -50), YS, AUTO, ('interleaved', 2),
                    ('zfft/multi/p1', 1, 'zfft/interleaved', 1)),
    # 96 samples stuffed 8-fold to 3 residues; an aperture shorter than its lattice (60 of 64 samples, 4-fold)
    'i-r3': Row(Axis(1536, 1536, 40, -20), YS, AUTO, ('interleaved', 2), ('zfft/multi/p1', 1, 'zfft/interleaved', 1)),
    'i-960': Row(Axis(960, 1024, 40, -20), YS, AUTO, ('interleaved', 2), ('zfft/multi/p1', 1, 'zfft/interleaved', 1)),
    # 384 samples stuffed 2-fold to 3 residues: not the one-wave kernel's shape
    'i-r3-stuff2': Row(Axis(6144, 6144, 40, -20), YS, AUTO, ('interleaved', 2),
                       ('zfft/multi/p1', 1, 'zfft/interleaved', 1)),
})

# (block, stuff) of the interleaved rows, as the interleave rule gives them
INTERLEAVE = {'i-cols128': (8, 2), 'i-cols128-short': (8, 2), 'i-stuff8': (8, 8), 'i-stuff4': (8, 4),
              'i-stuff2': (4, 2), 'i-r3': (8, 8), 'i-960': (8, 4), 'i-r3-stuff2': (8, 2)}

# Worst error of the radiation vectors against the oracle per row, relative to each one's largest component - what
# TOL = 1e-12 bounds.  test_gpu_fft_cases.py prints it and records it (ML_RECORD_PARITY).
MEASURED = {
    'g-y16-x16': 1.5e-15, 'g-y3-x1': 1.5e-15, 'g-y4-x1': 2.2e-15, 'g-y4-x16-513': 1.3e-15, 'g-y4-x3-12': 2.3e-15,
    'g-y4-x3-blocks': 2.5e-15, 'g-y4-x3-mirrored': 2.4e-15, 'g-y4-x3-nobin0': 5.0e-15, 'g-y4-x5-wrap': 2.1e-14,
    'g-y5-x5': 7.6e-15, 'g-y8-x3': 2.2e-15, 'i-960': 2.6e-15, 'i-cols128': 1.4e-14, 'i-cols128-short': 6.3e-15,
    'i-r3': 3.1e-15, 'i-r3-stuff2': 4.2e-15, 'i-stuff2': 8.9e-15, 'i-stuff4': 6.7e-15, 'i-stuff8': 2.3e-14,
    't-r16': 2.1e-14, 't-r3': 7.5e-15, 't-r32': 1.7e-14, 't-r32p': 1.7e-14, 't-r32p-mirrored': 1.9e-14,
    't-r4': 9.1e-15, 't-r64p': 2.3e-14, 't-r8': 1.4e-14, 't-r8-blocks': 4.5e-15, 't-r8-mirrored': 4.5e-15,
    'x-j2': 7.8e-15, 'x-j4': 1.1e-14, 'x-r1': 3.4e-15, 'x-r16': 2.1e-14, 'x-r16w': 8.0e-14, 'x-r2': 6.0e-15,
    'x-r3': 7.5e-15, 'x-r32': 1.7e-14, 'x-r32p': 1.7e-14, 'x-r32pn': 1.8e-14, 'x-r32pw': 8.0e-14, 'x-r4': 9.1e-15,
    'x-r48': 7.4e-15, 'x-r48-blocks': 7.4e-15, 'x-r48-mirrored': 7.3e-15, 'x-r4m': 1.9e-14, 'x-r64p': 2.3e-14,
    'x-r64s': 2.3e-14, 'x-r8': 1.4e-14, 'x-r8-blocks': 4.5e-15, 'x-r8-mirrored': 4.5e-15, 'x-r96': 5.5e-15,
    'y-j16': 6.4e-15, 'y-j2': 4.9e-15, 'y-j4': 4.7e-15, 'y-r1': 4.4e-15, 'y-r1-blocks1': 4.4e-15, 'y-r16': 2.0e-14,
    'y-r16-blocks1': 2.0e-14, 'y-r16w': 1.8e-14, 'y-r2': 5.3e-15, 'y-r3': 7.2e-15, 'y-r32': 1.0e-14,
    'y-r32p': 1.0e-14, 'y-r32p-blocks1': 1.0e-14, 'y-r32pn': 1.4e-14, 'y-r32pw': 5.4e-14, 'y-r4': 7.9e-15,
    'y-r48': 6.8e-15, 'y-r4m': 1.6e-14, 'y-r64p': 1.5e-14, 'y-r64s': 1.5e-14, 'y-r8': 1.5e-14, 'y-r96': 5.3e-15,
}


def pieces(row):
    """[(row0, resident rows, kind)] of the row's transform calls, in order; all but the first accumulate.
    kind: 0 a block, 1 mirrored pairs, 2 interleaved blocks (row0 = the rank)"""
    nx = row.x.n
    if row.shard == 'whole':
        return [(0, nx, 0)]
    kind, arg = row.shard
    if kind == 'blocks':
        return [(0, arg, 0), (arg, nx - arg, 0)]
    if kind == 'interleaved':
        return [(rank, nx // arg, 2) for rank in range(arg)]
    out = []
    for rank in range(arg):
        q0, q1 = row_block(nx // 2, arg, rank, 2)
        out.append((q0, 2 * (q1 - q0), 1))
    return out


def piece_rows(row, piece, block=0):
    """the aperture rows a piece holds, in the order they are resident"""
    row0, nxl, kind = piece
    nx = row.x.n
    if kind == 1:
        return np.concatenate((np.arange(row0, row0 + nxl // 2), np.arange(nx - row0 - nxl // 2, nx - row0)))
    if kind == 2:
        world = row.shard[1]
        return (np.arange(nx // (block * world))[:, None] * (block * world) + row0 * block
                + np.arange(block)[None, :]).ravel()
    return np.arange(row0, row0 + nxl)


def plan_facts(row, piece):
    """the arguments of tools/transform_route for one transform call of the row: the sizes, and per axis the lattice
    zfft_commensurate arrives at; the tool applies the axis rule and the interleave rule itself"""
    row0, nxl, kind = piece
    facts = dict(method=row.method, nx_total=row.x.n, ny=row.y.n, mx=row.x.M, my=row.y.M, nxl=nxl, shard=kind,
                 row0=0 if kind == 2 else row0, y_dot_lattice=n_eff(row.y), y_dot_jstep=jstep(row.y),
                 x_dot_lattice=n_eff(row.x), x_dot_jstep=jstep(row.x))
    if kind == 2:
        facts['n_ranks'] = row.shard[1]
    return facts


def lattice(ax, step):
    """the wanted bins of an axis whose samples are `step` apart, as direction cosines"""
    return (np.arange(ax.M) + ax.j0) * ((WL / N_GLASS) / (step * ax.N))


def axes(row):
    """x, y, ux, uy of a row: sample positions with the project's usual odd pitches and offsets, direction grids on
    the lattice of the spacing the arrays actually have (as the reference defines it)"""
    x = (np.arange(row.x.n) - 3.3) * (WL / 2.2)
    y = (np.arange(row.y.n) + 11.1) * (WL / 2.3)
    return x, y, lattice(row.x, x[1] - x[0]), lattice(row.y, y[1] - y[0])


def reached():
    """{stage: set of kernels} the table's rows are expected to launch"""
    out = {1: set(), 2: set()}
    for row in ROWS.values():
        out[1].add(row.expect[0])
        out[2].add(row.expect[2])
    return out


def axis_rows():
    """the distinct (R3, n_valid, M, j0, in place, jstep, passes) of the one-level, pass and multi launches of the
    table, as tools/zfft_emul takes them (j0 in bins of the lattice asked for): {key: a row's name}.  An axis in
    `split` sub-sequences is the geometry of its launches: the lattice of N_eff / split samples, the ceil(n / split)
    samples sub-sequence 0 holds, the same wanted bins (reduced to the short lattice by the tables, as the emulator
    does).  Which rows are resident (shards) is not the emulator's business: a sharded row counts as its axis"""
    out = {}
    for name, row in sorted(ROWS.items()):
        for ax, kernel, split in ((row.y, row.expect[0], row.expect[1]), (row.x, row.expect[2], row.expect[3])):
            fam = kernel.split('/')[1]
            if fam not in ('one', 'pass', 'multi'):
                continue
            key = (n_eff(ax) // 256 // split, -(-ax.n // split), ax.M, ax.j0, int(kernel.endswith('/ip')), jstep(ax),
                   2 if fam == 'pass' else 1)
            out.setdefault(key, name)
    return out


def tile_rows():
    """the distinct (R3, a0, h0, M, j0) of the table's tile column passes, for tools/zfft_tiles_emul"""
    out = {}
    for name, row in sorted(ROWS.items()):
        if row.expect[2] != 'zfft/tiles':
            continue
        for row0, nxl, kind in pieces(row):
            if kind == 0:   # (the emulator holds one run of resident samples)
                out.setdefault((n_eff(row.x) // 256, row0, nxl, row.x.M, row.x.j0), name)
    return out
