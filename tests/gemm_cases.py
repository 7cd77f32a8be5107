"""The cases of the GEMM path (method 'gemm', the fp32 mode, every off-lattice or asymmetric direction grid) that the
suite runs, in one table: the sizes, which direction grids are centre-symmetric, the precision, the shard, and the
kernel and split-K slabs each stage is expected to launch - one of the 12 production instantiations of zfold_kernel
(csrc/zfold.hip: {wide 32 x 128 tile of 1 x 8 waves, narrow 32 x 64} x {f64, f32} x {plain, in_sum, out_t}) or one of
zgemm_kernel's three tiles (csrc/zgemm.hip: 11 = 32 x 32, 10 = 64 x 64, 15 = 128 x 64 of 8 waves).
test_gemm_cases.py checks `expect` against what tools/transform_route prints for the row's plan facts (the launch
rules of csrc/transform_route.h, which the launchers call) and that the table reaches every production kernel in
each stage; test_gpu_gemm_cases.py runs every row on the GPU against the oracle's direct sum.  Plain data, no test
collects from here.

The wide tile is taken from 480 workgroups (tiles x slabs) on: about 1900 aperture rows in stage 1 (M = 4 x rows),
4 my >= 1024 with an 8-fold split in stage 2.  The apertures are therefore a few thousand rows by about a hundred:
the oracle's direct sum stays at a fraction of a second.
"""
import collections

# shape = (nx, ny, mx, my).  sym_x / sym_y: ux / uy centre-symmetric (uniform), else warped (the generic GEMM of that
# stage).  uc0: the symmetric grids are centred on 0 (no input modulation: FoldArgs E, out_E null).
# shard: 'whole' | ('blocks', r1) = rows [0, r1) then [r1, nx) accumulated | ('mirrored', world) = every rank's
# mirrored pairs (dist.mirrored_block, align 2) accumulated.
# expect = (stage 1 kernel, its slabs, stage 2 kernel, its slabs, stage 2 launches), of every piece of the shard.
Row = collections.namedtuple('Row', 'shape sym_x sym_y uc0 precision shard expect')

WIDE, NARROW = 'zfold/wide/', 'zfold/narrow/'


def _folded(shape, uc0, expect, shard='whole', sym_x=True, sym_y=True):
    """the row in both precisions: {name suffix: Row}"""
    return {p: Row(shape, sym_x, sym_y, uc0, p, shard, tuple(e.replace('/P/', '/%s/' % p) if isinstance(e, str) else e
                                                             for e in expect)) for p in ('f64', 'f32')}


_BOTH = {
    # stage 1 wide, 241 x 2 tiles: the second column tile has 2 half-directions (7 of its 8 waves without columns),
    # odd ny (the centre sample has no partner), odd my (jm == jp), 4 nx % 32 = 16
    'w1': _folded((1924, 67, 9, 259), False, (WIDE + 'P/plain', 1, 'zgemm/11', 1, 1), sym_x=False),
    # 240 x 1 tiles, split 2: the second chunk is 2 pairs long; the slabs summed by zsum_slabs_kernel
    'w2': _folded((1920, 131, 9, 200), False, (WIDE + 'P/plain', 2, 'zgemm/11', 1, 1), sym_x=False),
    # stage 1 transposed output with stage 2's input modulation (out_E); stage 2 narrow, 962 rows in 8 slabs
    'wt': _folded((1924, 67, 130, 259), False, (WIDE + 'P/out_t', 1, NARROW + 'P/plain', 8, 1)),
    # stage 1's two transposed slabs summed as the narrow stage 2 loads its tiles
    'wt2': _folded((1920, 131, 130, 200), False, (WIDE + 'P/out_t', 2, NARROW + 'P/in_sum', 8, 1)),
    # stage 2 wide: 64 x 1 tiles (65 half-directions in a 128-wide tile) x 8 slabs; both grids about 0
    'wtw': _folded((1920, 67, 130, 512), True, (WIDE + 'P/out_t', 1, WIDE + 'P/plain', 8, 1)),
    # stage 2 wide and slab-summing: 32 x 2 tiles (the second with 2 half-directions) x 8 slabs
    'wt2w': _folded((1920, 131, 260, 256), False, (WIDE + 'P/out_t', 2, WIDE + 'P/in_sum', 8, 1)),
    # both narrow; all four sizes odd in the second; the first with both grids about 0
    'n': _folded((64, 200, 130, 130), True, (NARROW + 'P/out_t', 2, NARROW + 'P/in_sum', 1, 1)),
    'nodd': _folded((65, 201, 131, 129), False, (NARROW + 'P/out_t', 2, NARROW + 'P/in_sum', 1, 1)),
    # the narrow plain tile in stage 1 too (what the small cases of test_gpu_parity.py run)
    'ns': _folded((45, 33, 18, 12), False, (NARROW + 'P/plain', 1, 'zgemm/11', 1, 1), sym_x=False),
    # a generic stage 1 feeding the folded stage 2 through ztranspose_kernel
    'gt': _folded((130, 37, 130, 130), False, ('zgemm/11', 1, NARROW + 'P/plain', 2, 1), sym_y=False),
    # mirrored shards of three ranks through both folded stages: 22, 22 and 21 row pairs (fold2_E built in two runs)
    'm3': _folded((130, 66, 130, 130), False, (NARROW + 'P/out_t', 1, NARROW + 'P/plain', 1, 1), shard=('mirrored', 3)),
}


def _generic(shape, expect, shard='whole', sym_x=False):
    return Row(shape, sym_x, False, False, 'f64', shard, expect)


ROWS = {'%s-%s' % (name, p): row for name, both in _BOTH.items() for p, row in both.items()}
ROWS.update({
    # zgemm stage 1, K = 37 (not a multiple of BK = 16): 17 x 16 tiles of 128 x 64, 17 x 16 of 64 x 64
    'g1-15': _generic((513, 37, 7, 961), ('zgemm/15', 1, 'zgemm/11', 1, 1)),
    'g1-10': _generic((258, 37, 7, 961), ('zgemm/10', 1, 'zgemm/11', 1, 1)),
    # zgemm stage 2 (batch 4, the negative strideC of the radiation-vector slots): 5 x 13 x 4 tiles of 128 x 64,
    # 5 x 13 x 4 of 64 x 64; whole, as two uneven row blocks (the second accumulating), and as mirrored shards of
    # two ranks (38 rows: the pairs need an even count; 10 and 9 pairs, two launches each)
    'g2-15': _generic((37, 50, 520, 770), ('zgemm/11', 1, 'zgemm/15', 1, 1)),
    'g2-15-blocks': _generic((37, 50, 520, 770), ('zgemm/11', 1, 'zgemm/15', 1, 1), ('blocks', 21)),
    'g2-15-mirrored': _generic((38, 50, 520, 770), ('zgemm/11', 1, 'zgemm/15', 1, 2), ('mirrored', 2)),
    'g2-10': _generic((37, 50, 260, 770), ('zgemm/11', 1, 'zgemm/10', 1, 1)),
    'g2-10-blocks': _generic((37, 50, 260, 770), ('zgemm/11', 1, 'zgemm/10', 1, 1), ('blocks', 21)),
    'g2-10-mirrored': _generic((38, 50, 260, 770), ('zgemm/11', 1, 'zgemm/10', 1, 2), ('mirrored', 2)),
})

# Worst error of the radiation vectors against the oracle per row, relative to each one's largest component - what
# TOL = 1e-12 / TOL_F32 = 1e-4 bound.  test_gpu_gemm_cases.py prints it and records it (ML_RECORD_PARITY); as taken on
# an MI355X.  The rows' bounds are the project's, not these.
MEASURED = {
    'g1-10': 2.1e-15, 'g1-15': 3.2e-15, 'g2-10': 1.0e-15, 'g2-10-blocks': 8.7e-16, 'g2-10-mirrored': 7.8e-16,
    'g2-15': 1.4e-15, 'g2-15-blocks': 1.1e-15, 'g2-15-mirrored': 8.1e-16, 'gt-f32': 4.9e-07, 'gt-f64': 1.7e-14,
    'm3-f32': 2.3e-07, 'm3-f64': 1.8e-14, 'n-f32': 4.2e-07, 'n-f64': 2.0e-15, 'nodd-f32': 4.2e-07,
    'nodd-f64': 2.7e-14, 'ns-f32': 1.1e-07, 'ns-f64': 2.4e-15, 'w1-f32': 1.9e-07, 'w1-f64': 5.6e-15,
    'w2-f32': 3.4e-07, 'w2-f64': 8.1e-15, 'wt-f32': 3.9e-07, 'wt-f64': 2.7e-13, 'wt2-f32': 5.1e-07,
    'wt2-f64': 2.6e-13, 'wt2w-f32': 5.4e-07, 'wt2w-f64': 1.3e-13, 'wtw-f32': 4.4e-07, 'wtw-f64': 2.9e-15,
}

ZFOLD_KERNELS = tuple('zfold/%s/%s/%s' % (t, p, io) for t in ('wide', 'narrow') for p in ('f64', 'f32')
                      for io in ('plain', 'in_sum', 'out_t'))
ZGEMM_KERNELS = ('zgemm/10', 'zgemm/11', 'zgemm/15')


def row_block(n_rows, world, rank, align):
    """metalens_amd/dist.py row_block, restated so that the table needs no package import"""
    edges = [min(n_rows, int(round(n_rows * k / world / align)) * align) for k in range(world + 1)]
    edges[0], edges[-1] = 0, n_rows
    for k in range(1, world + 1):
        edges[k] = max(edges[k], edges[k - 1])
    return edges[rank], edges[rank + 1]


def pieces(row):
    """[(row0, resident rows, mirrored)] of the row's transform calls, in order; all but the first accumulate"""
    nx = row.shape[0]
    if row.shard == 'whole':
        return [(0, nx, False)]
    kind, arg = row.shard
    if kind == 'blocks':
        return [(0, arg, False), (arg, nx - arg, False)]
    out = []
    for rank in range(arg):
        q0, q1 = row_block(nx // 2, arg, rank, 2)
        out.append((q0, 2 * (q1 - q0), True))
    return out


def plan_facts(row, piece):
    """the arguments of tools/transform_route for one transform call of the row: what ml_farfield_plan arrives at
    under method 'gemm' (include/metalens_hip.h ML_METHOD_GEMM = 1: no FFT axis)"""
    nx, ny, mx, my = row.shape
    row0, nxl, mirrored = piece
    return dict(method=1, nx_total=nx, ny=ny, mx=mx, my=my, nxl=nxl, row0=row0, shard=int(mirrored),
                fold=int(row.sym_y), fold_S=(my + 1) // 2 if row.sym_y else 0,
                fold2=int(row.sym_x), fold2_S=(mx + 1) // 2 if row.sym_x else 0, f32=int(row.precision == 'f32'))


def reached():
    """{stage: set of kernels} the table's rows are expected to launch"""
    out = {1: set(), 2: set()}
    for row in ROWS.values():
        out[1].add(row.expect[0])
        out[2].add(row.expect[2])
    return out
