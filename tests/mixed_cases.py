"""The axis cases of the method 'fft-mixed' that the suite runs, in one table: which lattice, how many samples of it
exist, which bins are wanted, and the factorisation N s = A x B x R the production chooser (zfft_core.h mixed_choose)
picks for it.  test_zfft_mixed_emul.py checks `expect` against the chooser itself and runs the host phases of every
row, and checks that the table reaches every kernel; test_gpu_fft_mixed.py runs the 2-D cases below on the GPU
against the oracle's direct sum.  Plain data, no test collects from here.

A 2-D case puts one row on the x axis and one on the y axis (farfield.hip: stage 1 transforms y, stage 2 x):

    stage 1             the y row: zfft_mixed_kernel<A, B, STREAM = true> over the fields' rows
    stage 2 streaming   the x row where y is an FFT axis too: the stage-1 result is stored transposed, in_es == 1
    stage 2 strided     the x row where uy sits on no lattice (y = None): stage 1 is the folded GEMM, its result
                        row-major, in_es == my, STREAM = false
"""
import collections

Row = collections.namedtuple('Row', 'n_samples n_lattice m_bins j0 expect resident')
Row.__new__.__defaults__ = (None,)   # resident: (a0, h0, a1, h1) of a two-run residency (emulator only)

# expect = (s, A, B, R).  Row names: the pair's letter and the lattice length.
# Windows far off axis stay on the short lattices: the oracle sums exp(i 2 pi kappa u x) over the axis arrays as
# given, whose samples carry half an ulp each, i.e. a phase uncertainty of 2 pi |j| eps / 2 per term at bin j - 3e-12
# rad at bin 5000, the size of the tolerance itself (measured on 4960 samples from bin 4930: 6.9e-13 of the 1e-12,
# against 1e-14 around the axis).  There the comparison measures the inputs, not the kernel.
ROWS = {
    # 16 x 10
    'a160': Row(160, 160, 64, -32, (1, 16, 10, 1)),
    'a320': Row(300, 320, 100, 290, (1, 16, 10, 2)),           # wraps round the lattice's end
    'a4960': Row(4960, 4960, 64, -32, (1, 16, 10, 31)),
    'a80': Row(70, 80, 40, -20, (2, 16, 10, 1)),
    'a240': Row(200, 240, 64, 200, (2, 16, 10, 3)),            # s = 2, wraps round the lattice's end
    # 15 x 10
    'b450': Row(450, 450, 128, -64, (1, 15, 10, 3)),
    'b750': Row(700, 750, 96, -48, (1, 15, 10, 5)),
    'b4650': Row(4650, 4650, 64, -32, (1, 15, 10, 31)),
    'b75': Row(75, 75, 40, -20, (2, 15, 10, 1)),
    'b225': Row(180, 225, 64, 40, (2, 15, 10, 3)),             # s = 2, a window without bin 0
    # 12 x 9
    'c108': Row(108, 108, 64, -32, (1, 12, 9, 1)),
    'c540': Row(540, 540, 80, -40, (1, 12, 9, 5)),
    'c1080': Row(1000, 1080, 128, -64, (1, 12, 9, 10)),
    'c3456': Row(3456, 3456, 32, -16, (1, 12, 9, 32)),         # (with many bins 3456 takes 16 x 9 x 24)
    'c54': Row(50, 54, 30, -15, (2, 12, 9, 1)),
    'c270': Row(270, 270, 100, -50, (2, 12, 9, 5)),
    # 16 x 9
    'd144': Row(144, 144, 64, -32, (1, 16, 9, 1)),
    'd288': Row(288, 288, 64, -32, (1, 16, 9, 2)),
    'd576': Row(576, 576, 64, -70, (1, 16, 9, 4)),             # a window without bin 0
    'd4464': Row(4464, 4464, 64, -32, (1, 16, 9, 31)),
    'd72': Row(72, 72, 40, -20, (2, 16, 9, 1)),
    'd504': Row(400, 504, 72, -36, (2, 16, 9, 7)),             # R = 7
    # 16 x 15
    'e720': Row(720, 720, 96, -48, (1, 16, 15, 3)),
    'e7200': Row(7200, 7200, 512, -256, (1, 16, 15, 30)),      # (with few bins 7200 takes 15 x 15 x 32: f7200)
    'e120': Row(100, 120, 64, -32, (2, 16, 15, 1)),
    'e360': Row(360, 360, 90, -45, (2, 16, 15, 3)),
    'e3720': Row(3720, 3720, 200, -100, (2, 16, 15, 31), (200, 1000, 2000, 900)),   # two resident runs at s = 2
    # 15 x 15
    'f675': Row(675, 675, 64, -32, (1, 15, 15, 3)),
    'f900': Row(900, 900, 100, -50, (1, 15, 15, 4)),
    'f1350': Row(1350, 1350, 64, -32, (1, 15, 15, 6)),
    'f7200': Row(7200, 7200, 64, -32, (1, 15, 15, 32)),
    # 9 x 9
    'g81': Row(81, 81, 40, -20, (1, 9, 9, 1)),
    'g162': Row(162, 162, 64, -32, (1, 9, 9, 2)),
    'g243': Row(243, 243, 64, -32, (1, 9, 9, 3)),
    'g2592': Row(2592, 2592, 64, -32, (1, 9, 9, 32)),
    # 10 x 10
    'h100': Row(100, 100, 50, -25, (1, 10, 10, 1)),
    'h700': Row(700, 700, 64, -32, (1, 10, 10, 7)),            # R = 7
    'h3200': Row(3200, 3200, 64, -32, (1, 10, 10, 32)),
    'h50': Row(50, 50, 30, -15, (2, 10, 10, 1)),
    'h1250': Row(1250, 1250, 64, -32, (2, 10, 10, 25)),
}

# (x row, y row or None); a long axis is paired with a short one: the oracle's direct sum is the cost
GPU_CASES = (
    ('a4960', 'c54'), ('b4650', 'd72'), ('c3456', 'a80'), ('d4464', 'b75'), ('e120', 'e7200'), ('f7200', 'h50'),
    ('g2592', 'g81'), ('h3200', 'f675'), ('f900', 'b450'), ('h1250', 'd504'), ('d288', 'c1080'), ('g162', 'a320'),
    ('e360', 'h700'), ('c270', 'b225'), ('a240', 'c540'), ('b750', 'd144'),
    ('a160', None), ('b225', None), ('c108', None), ('d576', None), ('e720', None), ('f1350', None), ('g243', None),
    ('h100', None),
)
OFF_NY, OFF_MY = 60, 24     # the y axis of the cases whose uy sits on no lattice

ROLES = ('stage 1', 'stage 2 streaming', 'stage 2 strided')


def roles():
    """{(A, B): {role: [row name, ...]}} of GPU_CASES"""
    out = collections.defaultdict(lambda: collections.defaultdict(list))
    for xr, yr in GPU_CASES:
        out[ROWS[xr].expect[1:3]]['stage 2 streaming' if yr else 'stage 2 strided'].append(xr)
        if yr:
            out[ROWS[yr].expect[1:3]]['stage 1'].append(yr)
    return out


def wraps(row):
    """the window runs past the last bin of the lattice into its first ones (not merely from negative bins up)"""
    return 0 < row.j0 < row.n_lattice < row.j0 + row.m_bins


def without_bin_0(row):
    return not any((row.j0 + j) % row.n_lattice == 0 for j in range(row.m_bins))
