"""The cases of the far-field back end (csrc/farfield_project.hip: project_kernel, unfold_project_kernel;
csrc/farfield_sums.hip: accumulate_kernel, accumulate_finish_kernel; behind ml_farfield_project[_async], ml_farfield_project_reduce, ml_farfield_lattice_power,
ml_farfield_accumulate, ml_farfield_sums, ml_farfield_total_power) in one table: the directions at which a nearly
faithful projection differs from a faithful one, the tensor grid that reaches the fused unfold + projection kernel,
and the sweep-sum rows that reach every branch and loop edge of the two summing kernels.
test_farfield_power_cases.py holds every claim made here in NumPy and through tools/transform_route, without a
GPU; test_gpu_farfield_power_cases.py runs every row on the GPU against tests/farfield_power_ref.py.  Plain data
and NumPy, no package import; no test collects from here.
"""
import collections

import numpy as np

WL, N_GLASS = 580e-9, 1.459
Z0 = 1.25663706212e-6 * 299792458.0

# ---- RIM: directions on, next to and beyond the rim of the unit circle, on and next to the axis ----------------------
# The class of a direction is what NumPy's float64 `1 - ux**2 - uy**2` (the contract, farfield_power_ref._uz) makes
# of it:
#   'uz0'      the expression is exactly 0: P carries 1 / (0 + 1e-5)
#   'tiny'     a positive value below 1e-16 (so sqrt is ~1e-8, at the scale of nothing: P carries 1 / (uz + 1e-5))
#   'nan'      negative: uz, both amplitudes and P are NaN - (0.6, 0.8) by one rounding, the directions outside plainly
#   'zero'     ux == 0 and uy == 0 (of either sign): the (0, 0) rule, the vectors themselves
#   'interior' everything else, among it (0, 0.5) and (0.5, 0) - one cosine zero is NOT the special case - and the
#              directions next to the axis: sin(theta) = 1e-9 is the size of its regulariser, 1e-200 squares to 0
# With ONE fused multiply-add, 1 - ux*ux - uy*uy at (0.28, 0.96) is +4.3e-17 instead of 0 (P moves by 6.5e-4 of itself)
# and at (0.1, sqrt(0.99)) negative (NaN): the rows tell a contracted kernel from a faithful one.
_S99 = 0.99 ** 0.5
_RIM_BASE = (
    ((0.28, 0.96), 'uz0'), ((0.96, 0.28), 'tiny'),
    ((0.1, _S99), 'uz0'), ((_S99, 0.1), 'tiny'),
    ((8 / 17, 15 / 17), 'uz0'), ((15 / 17, 8 / 17), 'tiny'),
    ((0.6, 0.8), 'nan'), ((0.8, 0.6), 'nan'),
)
_RIM_SPECIAL = (
    ((0.0, 0.0), 'zero'), ((-0.0, 0.0), 'zero'),
    ((1.0, 0.0), 'uz0'), ((0.0, 1.0), 'uz0'),
    ((1e-200, 0.0), 'interior'), ((1e-9, 0.0), 'interior'),
    ((0.0, 0.5), 'interior'), ((0.5, 0.0), 'interior'),
    ((1.0, 1e-8), 'nan'), ((1.2, 0.3), 'nan'),
)
RIM_SEEDED = 22


def rim():
    """-> (ux, uy, classes): the pair list, 64 directions"""
    pairs = []
    for (a, b), cls in _RIM_BASE:                       # the sign mirrors (the axis mirrors are rows of the base)
        pairs += [((sa * a, sb * b), cls) for sa in (1, -1) for sb in (1, -1)]
    pairs += list(_RIM_SPECIAL)
    rng = np.random.default_rng(20240917)
    r, phi = 0.97 * np.sqrt(rng.uniform(0.0004, 1, RIM_SEEDED)), rng.uniform(0, 2 * np.pi, RIM_SEEDED)
    pairs += [((float(x), float(y)), 'interior') for x, y in zip(r * np.cos(phi), r * np.sin(phi))]
    ux = np.array([p[0][0] for p in pairs])
    uy = np.array([p[0][1] for p in pairs])
    return ux, uy, [p[1] for p in pairs]


RIM_UX_LEN, RIM_UY_LEN = 19, 261


def rim_axes():
    """-> (ux_list, uy_list) for ml_farfield_lattice_power, which takes any lists: RIM's distinct |ux| with the sign
    mirrors of two pairs, and its distinct uy padded with seeded values to two column blocks of 256, the second with
    5 lanes - which hold rim values again, so that the short block projects the directions that matter"""
    ux = [0.28, 0.96, 0.1, _S99, 8 / 17, 15 / 17, 0.6, 0.8, -0.28, -0.96, -0.6, -0.8,
          0.0, -0.0, 1.0, 1e-200, 1e-9, 0.5, 1.2]
    uy = []
    for v in (0.28, 0.96, 0.1, _S99, 8 / 17, 15 / 17, 0.6, 0.8):
        uy += [v, -v]
    uy += [0.0, -0.0, 1.0, 0.5, 1e-8, 0.3]
    tail = [0.96, 0.28, 0.8, 1.0, _S99]
    rng = np.random.default_rng(20240918)
    uy += list(rng.uniform(-1.0, 1.0, RIM_UY_LEN - len(uy) - len(tail))) + tail
    assert len(ux) == RIM_UX_LEN and len(uy) == RIM_UY_LEN
    return np.array(ux), np.array(uy)


def classify(ux, uy):
    """the class of every direction as NumPy's float64 expressions give it (elementwise)"""
    ux, uy = np.asarray(ux, dtype=float), np.asarray(uy, dtype=float)
    uz2 = 1 - ux ** 2 - uy ** 2
    out = np.full(ux.shape, 'interior', dtype=object)
    out[(uz2 > 0) & (uz2 < 1e-16)] = 'tiny'
    out[uz2 == 0] = 'uz0'
    out[uz2 < 0] = 'nan'
    out[(ux == 0) & (uy == 0)] = 'zero'
    return out


# ---- FOLDED: the tensor grid that reaches unfold_project_kernel under method 'gemm' ----------------------------------
# shape = (nx, ny, mx, my).  Both direction axes exactly antisymmetric and odd (so (0, 0) is a grid point and both
# stages fold), lengths 131 = 16 x 8 + 3 and 133 = 16 x 8 + 5 (ragged 8 x 8 tiles on both sides), |u| up to 0.9 (NaN
# corners).  260 aperture rows = 130 row pairs: the folded stage 2 leaves 3 split-K slabs for the kernel to sum.
# The mirrored pieces are uneven - 80 and 50 row pairs, 2 slabs and 1 - and the second accumulates: the only way to
# `accumulate` in the fused kernel, since a plain block of rows has no mirror partners and takes the generic stage 2
# (transform_route.h), which leaves nothing pending.
Folded = collections.namedtuple('Folded', 'shape u_max pieces blocks expect_whole expect_pieces')
FOLDED = Folded(shape=(260, 37, 131, 133), u_max=0.9,
                pieces=((0, 160), (80, 100)),            # (row0, resident rows) of the mirrored shards
                blocks=((0, 150), (150, 110)),           # ... and of two plain row blocks (generic stage 2)
                expect_whole=('folded', 'folded', 3),   # stage 1, stage 2, stage 2's slabs
                expect_pieces=(('folded', 'folded', 2), ('folded', 'folded', 1)))


def folded_axes():
    mx, my = FOLDED.shape[2:]
    ux, uy = np.linspace(-FOLDED.u_max, FOLDED.u_max, mx), np.linspace(-FOLDED.u_max, FOLDED.u_max, my)
    return 0.5 * (ux - ux[::-1]), 0.5 * (uy - uy[::-1])


def folded_plan_facts(piece=None):
    """the arguments of tools/transform_route for the whole aperture (piece None) or one mirrored piece, as
    gemm_cases.plan_facts forms them"""
    nx, ny, mx, my = FOLDED.shape
    row0, nxl = (0, nx) if piece is None else piece
    return dict(method=1, nx_total=nx, ny=ny, mx=mx, my=my, nxl=nxl, row0=row0, shard=int(piece is not None),
                fold=1, fold_S=(my + 1) // 2, fold2=1, fold2_S=(mx + 1) // 2, f32=0)


def mirrored_rows(nx, row0, nxl):
    return np.concatenate((np.arange(row0, row0 + nxl // 2), np.arange(nx - row0 - nxl // 2, nx - row0)))


# ---- the sum rows -----------------------------------------------------------------------------------------------------
# Each on an aperture of 24 x 20 seeded complex samples under method 'gemm' (every transform is trivial; an axis of
# one direction takes the generic GEMM with M or N = 1, whose loads and stores are bounded per element).
APERTURE = (24, 20)
# kind 'grid': ux, uy = the axes; 'pairs': a pair list.  cone = (radius, centre ux, centre uy).
SumRow = collections.namedtuple('SumRow', 'kind ux uy cone claims')


def _pairs300():
    rng = np.random.default_rng(20240919)
    return rng.uniform(-0.75, 0.75, 300), rng.uniform(-0.75, 0.75, 300)


SUM_ROWS = {
    # 77100 directions = 302 blocks, the last with 44 entries: accumulate_finish_kernel's strided loop runs twice in
    # lanes 0 ... 45 and once in the others; NaN corners
    'two-rounds': SumRow('grid', np.linspace(-0.9, 0.9, 300), np.linspace(-0.9, 0.9, 257), (0.3, 0.05, -0.1),
                         dict(blocks=302, last=44, nan=True)),
    # every quantity a small multiple of 1/64, so the cone test is exact: 81 directions inside, 12 of them ON the edge
    'exact-cone': SumRow('grid', np.arange(-20, 21) / 64, np.arange(-24, 25) / 64, (5 / 64, 1 / 64, -2 / 64),
                         dict(inside=81, on_edge=12, nan=False)),
    # a pair list (cell = 1, i = j = at), some directions outside the circle, two blocks (the second with 44)
    'pairs': SumRow('pairs', *_pairs300(), (0.25, 0.1, -0.05), dict(blocks=2, last=44, nan=True)),
    # one direction on an axis: that axis' factor of the cell is 1
    'one-row': SumRow('grid', np.array([0.05]), np.linspace(-0.6, 0.6, 37), (0.2, 0.0, 0.1), dict(nan=False)),
    'one-column': SumRow('grid', np.linspace(-0.6, 0.6, 41), np.array([-0.02]), (0.2, 0.1, 0.0), dict(nan=False)),
    'one': SumRow('grid', np.array([0.05]), np.array([-0.02]), (0.1, 0.0, 0.0), dict(nan=False)),
}

# 'weights': three maps (three seeded apertures) on one grid with NaN corners; (map, weight, slot, reset) in call order -
# a weight of 0 (0.0 * NaN stays NaN), a negative one, a reset in the middle of the second sequence, the first,
# second and last slot.  Slot 2 is never written and reads 0.
WEIGHTS_GRID = (np.linspace(-0.85, 0.85, 23), np.linspace(-0.8, 0.8, 19))
WEIGHTS_CONE = (0.4, 0.0, 0.0)
WEIGHTS_CALLS = (
    ((0, 1.0, 0, 1), (1, -0.5, 1, 0), (2, 0.0, 4095, 0)),
    ((2, 1.0, 4095, 1), (0, -0.5, 0, 0), (1, 0.25, 1, 1), (2, 0.0, 0, 0)),
)
MAX_SLOTS = 4096

# ---- the inventory: every branch and edge of the back end, and the row that reaches it ----------------------------
# (test_farfield_power_cases.py checks that the rows exist and, in NumPy, that they are what the inventory says)
INVENTORY = {
    'project_point: uz == 0 exactly': ('RIM', 'uz0'),
    'project_point: uz tiny positive': ('RIM', 'tiny'),
    'project_point: uz < 0 by one rounding, NaN': ('RIM', 'nan'),
    'project_point: the (0, 0) rule taken': ('RIM', 'zero'),
    'project_point: the (0, 0) rule not taken with one cosine zero': ('RIM', 'interior'),
    'project_point: pair_list branch (uy[i], my = 1)': ('RIM', 'pairs'),
    'project_point: from_fft (ml_farfield_lattice_power), second column block of 5 lanes': ('RIM', 'axes'),
    'unfold_project_kernel: ragged 8 x 8 tiles, 3 slabs': ('FOLDED', 'whole'),
    'unfold_project_kernel: accumulate': ('FOLDED', 'pieces'),
    'project_kernel on vectors accumulated over row blocks': ('FOLDED', 'blocks'),
    'project_kernel after zunfold_out_kernel (bit-equal to the fused kernel)': ('FOLDED', 'whole'),
    'project stage 1 + stage 2 (ml_farfield_project_reduce, no communicator)': ('FOLDED', 'whole'),
    'accumulate_kernel: isfinite false': ('SUM', 'two-rounds'),
    'accumulate_kernel: isfinite true everywhere': ('SUM', 'exact-cone'),
    'accumulate_kernel: cone edge, <= against <': ('SUM', 'exact-cone'),
    'accumulate_kernel: pair list (cell 1, i = j = at)': ('SUM', 'pairs'),
    'accumulate_kernel: last block partly filled': ('SUM', 'two-rounds'),
    'accumulate_kernel: mx = 1': ('SUM', 'one-row'),
    'accumulate_kernel: my = 1': ('SUM', 'one-column'),
    'accumulate_kernel: one direction': ('SUM', 'one'),
    'accumulate_kernel: reset and add, weight 0 and < 0, NaN stays NaN': ('SUM', 'weights'),
    'accumulate_finish_kernel: more than 256 blocks (strided loop twice)': ('SUM', 'two-rounds'),
    'accumulate_finish_kernel: fewer than 256 blocks': ('SUM', 'exact-cone'),
    'slots 0, 1, 4095 and a slot never written': ('SUM', 'weights'),
    'ml_farfield_total_power: its own slot, P_sum untouched': ('SUM', 'two-rounds'),
}

# Worst error over bound per row (1 = at the bound) as test_gpu_farfield_power_cases.py prints and records it
# (ML_RECORD_PARITY); as taken on an MI355X.  The bounds are those the tests state, not these.
MEASURED = {
    # the projection: the amplitudes had the yardstick's bits in every component of every row (0 of the bound)
    'rim-pairs': 0.27, 'rim-axes': 0.14, 'folded-fused': 0.47, 'folded-separate': 0.47, 'folded-pieces': 0.48,
    'folded-blocks': 0.49,
    # the sums (0: the device's sum is the exactly rounded one)
    'two-rounds': 0.0, 'exact-cone': 0.061, 'pairs': 0.096, 'one-row': 0.0, 'one-column': 0.0, 'one': 0.0,
    'weights-slot0': 0.082, 'weights-slot1': 0.060, 'weights-slot4095': 0.082,
}
