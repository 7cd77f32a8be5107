"""The cases of the beam metrics of the far field (csrc/farfield_beam.hip: beam_chunk_kernel<false>, beam_chunk_kernel<true>,
beam_finish_kernel behind ml_farfield_beam, and ml_farfield_beams) in one table: the smallest shapes at which these kernels
can go wrong, and an inventory that names every branch and loop edge of them with the row that reaches it.
test_farfield_beam_cases.py holds every claim made here in NumPy and through tools/farfield_beam_plan, without a GPU;
test_gpu_farfield_beam.py runs every row on the GPU against tests/farfield_beam_ref.py.  Each row runs on the APERTURE of
tests/farfield_power_cases.py, 24 x 20 seeded complex samples, under method 'gemm', so every transform is trivial.
Plain data and NumPy, no package import; no test collects from here.
"""
import collections

import numpy as np

from farfield_power_cases import APERTURE, N_GLASS, WL, Z0, _pairs300   # noqa: F401  (the same aperture and constants)

# kind 'grid': ux, uy = the axes; 'pairs': a pair list.  centre: (cx, cy) or None - the map's own peak direction.
# cones: in the caller's order.  of: 'projection', or 'sums' = P_sum after ONE ml_farfield_accumulate with `weight`.
# slot: the record slot the row's first call uses.
Row = collections.namedtuple('Row', 'kind ux uy centre cones of weight slot claims')


def _pairs(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.75, 0.75, n), rng.uniform(-0.75, 0.75, n)


def _row(kind, ux, uy, centre, cones, claims, of='projection', weight=1.0, slot=0):
    return Row(kind, np.asarray(ux, dtype=float), np.asarray(uy, dtype=float), centre, tuple(cones), of, weight, slot, claims)


ROWS = {
    # 77100 directions with NaN corners: 76 chunks, the last with 300 directions (lanes 44 ... 255 of its second step and
    # its last two steps idle), three finish tiles, the last of 12 records; the centre is the peak: three launches
    'many-chunks': _row('grid', np.linspace(-0.9, 0.9, 300), np.linspace(-0.9, 0.9, 257), None, (0.3, 0.1),
                        dict(n=77100, chunks=76, last=300, finish_tiles=3, last_tile=12, nan=True), slot=1),
    # ... and about a given centre: two launches
    'many-chunks-centre': _row('grid', np.linspace(-0.9, 0.9, 300), np.linspace(-0.9, 0.9, 257), (0.05, -0.1), (0.3,),
                               dict(n=77100, chunks=76, last=300, finish_tiles=3, last_tile=12, nan=True)),
    # every quantity a multiple of 1/64, so the cone test is exact: directions ON the edge of every cone; repeated,
    # unsorted and zero cones.  inside / on_edge per cone in the caller's order (the ref counts them)
    'exact-cone': _row('grid', np.arange(-20, 21) / 64, np.arange(-24, 25) / 64, (1 / 64, -2 / 64), (5 / 64, 3 / 64, 5 / 64, 0.0),
                       dict(n=2009, chunks=2, last=985, inside=(81, 29, 81, 1), on_edge=(12, 4, 12, 1), nan=False)),
    # exactly one chunk and exactly two: no lane idles in any step
    'one-chunk': _row('grid', np.linspace(-0.5, 0.5, 32), np.linspace(-0.45, 0.55, 32), None, (0.2,),
                      dict(n=1024, chunks=1, last=1024, nan=False), slot=4095),
    'two-chunks': _row('grid', np.linspace(-0.5, 0.5, 64), np.linspace(-0.45, 0.55, 32), (0.1, 0.1), (0.2, 0.4),
                       dict(n=2048, chunks=2, last=1024, nan=False)),
    # a pair list (cell 1, i = j) one longer than a chunk: the last chunk holds one direction
    'pairs-chunk-plus-one': _row('pairs', *_pairs(1025, 20241020), None, (0.25,), dict(n=1025, chunks=2, last=1, nan=True)),
    # the 300-entry pair list of the sum rows: less than one chunk, some directions outside the circle
    'pairs300': _row('pairs', *_pairs300(), (0.1, -0.05), (0.25, 0.5), dict(n=300, chunks=1, last=300, nan=True), slot=1),
    # one direction on an axis: that axis' factor of the cell is 1, and i or j is 0 throughout
    'one-row': _row('grid', [0.05], np.linspace(-0.6, 0.6, 37), None, (0.2,), dict(n=37, chunks=1, last=37, nan=False)),
    'one-column': _row('grid', np.linspace(-0.6, 0.6, 41), [-0.02], (0.1, 0.0), (0.2,), dict(n=41, chunks=1, last=41, nan=False)),
    'one': _row('grid', [0.05], [-0.02], None, (0.0, 0.1), dict(n=1, chunks=1, last=1, nan=False)),
    # axes wholly beyond the unit circle: nothing finite - NaN, -1, 0, zeros; about the peak (the centre is NaN) and about
    # a given centre (which the record repeats)
    'nothing-finite': _row('grid', np.linspace(1.1, 1.3, 5), np.linspace(1.1, 1.3, 4), None, (0.2, 3.0),
                           dict(n=20, chunks=1, last=20, nan=True, none=True)),
    'nothing-finite-centre': _row('grid', np.linspace(1.1, 1.3, 5), np.linspace(1.1, 1.3, 4), (1.2, 1.2), (0.2, 3.0),
                                  dict(n=20, chunks=1, last=20, nan=True, none=True)),
    # P_sum after one accumulate with weight 0 on a grid with NaN corners: every finite entry is 0.0 (0.0 * NaN stays
    # NaN), so the peak is the lowest FINITE index, which is not index 0; every sum is 0 and the centroid undefined
    'sums-weight-0': _row('grid', np.linspace(-0.85, 0.85, 23), np.linspace(-0.8, 0.8, 19), None, (0.4,),
                          dict(n=437, chunks=1, last=437, nan=True, first_finite=4), of='sums', weight=0.0),
    # P_sum with a weight, about a given centre
    'sums': _row('grid', np.linspace(-0.85, 0.85, 23), np.linspace(-0.8, 0.8, 19), (0.0, 0.1), (0.4, 0.2),
                 dict(n=437, chunks=1, last=437, nan=True), of='sums', weight=-0.5, slot=4095),
    # a pair list of two chunks, the last partly filled (276 directions); the GPU test reorders it after a first run so
    # that its brightest direction is the LAST entry: the peak's index is n - 1, found in the last lane that has work
    'peak-last': _row('pairs', *_pairs(1300, 20241021), None, (0.3,), dict(n=1300, chunks=2, last=276, nan=True)),
    # 32 cones, descending in the caller's order: every cone register of a lane, and the last column of a partial record
    '32-cones': _row('grid', np.linspace(-0.7, 0.7, 41), np.linspace(-0.65, 0.7, 37), None, tuple(np.linspace(0.64, 0.02, 32)),
                     dict(n=1517, chunks=2, last=493, nan=False)),
    # more than 2**20 directions: the chunk doubles to 2048 (a lane adds 8 terms), 513 chunks, 17 finish tiles, the last
    # of one record - 17 x 16 (tile, column) tasks for the 256 lanes of the last launch; the last chunk is half filled
    'chunk-doubles': _row('grid', np.linspace(-0.9, 0.9, 1025), np.linspace(-0.9, 0.9, 1024), None, tuple(np.linspace(0.05, 0.65, 7)),
                          dict(n=1049600, chunk=2048, chunks=513, last=1024, finish_tiles=17, last_tile=1, nan=True), slot=1),
}

SLOTS = (0, 1, 4095)     # the slots the rows use; NEVER_WRITTEN stays untouched in every test that reads it
NEVER_WRITTEN = 2
MAX_SLOTS = 4096

# ---- the inventory: every branch and loop edge of the new kernels, and the row that reaches it -----------------------
# (test_farfield_beam_cases.py checks that the rows exist and, in NumPy and through the plan tool, that they are what
# the inventory says)
INVENTORY = {
    'beam_chunk_kernel: isfinite false (NaN corners)': 'many-chunks',
    'beam_chunk_kernel: isfinite true everywhere': 'exact-cone',
    'beam_chunk_kernel: no finite direction in the map': 'nothing-finite',
    'beam_chunk_kernel: last chunk partly filled, lanes past its end idle': 'many-chunks',
    'beam_chunk_kernel: last chunk of one direction': 'pairs-chunk-plus-one',
    'beam_chunk_kernel: exactly one chunk, every lane busy in every step': 'one-chunk',
    'beam_chunk_kernel: exactly two chunks': 'two-chunks',
    'beam_chunk_kernel: a map shorter than a step (lanes that never have work)': 'one-row',
    'beam_chunk_kernel: pair list (cell 1, i = j = at)': 'pairs300',
    'beam_chunk_kernel: mx = 1': 'one-row',
    'beam_chunk_kernel: my = 1': 'one-column',
    'beam_chunk_kernel: one direction': 'one',
    'beam_chunk_kernel: cone edge, <= against <': 'exact-cone',
    'beam_chunk_kernel: a cone of 0 holds the centre direction alone': 'exact-cone',
    'beam_chunk_kernel: repeated cones have equal sums': 'exact-cone',
    'beam_chunk_kernel: K = 32, every cone register': '32-cones',
    'beam_chunk_kernel: peak of equals is the lowest index (all finite entries 0.0)': 'sums-weight-0',
    'beam_chunk_kernel: peak in the last lane with work of the last chunk': 'peak-last',
    'beam_chunk_kernel: chunk of 2048, eight terms per lane': 'chunk-doubles',
    'beam_chunk_kernel<false> + centre read on the device (three launches)': 'many-chunks',
    'beam_chunk_kernel<true>: centre given (two launches)': 'many-chunks-centre',
    'beam_chunk_kernel<true>: more chunk peaks than lanes (strided loop over 513 peaks)': 'chunk-doubles',
    'beam_chunk_kernel<true>: centre is the peak and no chunk has one (NaN centre)': 'nothing-finite',
    'beam_finish_kernel: one tile of one record': 'one-chunk',
    'beam_finish_kernel: one tile of two records': 'two-chunks',
    'beam_finish_kernel: three tiles, the last ragged (12 records)': 'many-chunks',
    'beam_finish_kernel: 17 tiles, more (tile, column) tasks than lanes, last tile of one record': 'chunk-doubles',
    'beam_finish_kernel: zeros behind K': 'many-chunks-centre',
    'beam_finish_kernel: nothing finite with a given centre (the record repeats it)': 'nothing-finite-centre',
    'source -1: P_sum': 'sums',
    'slots 0, 1 and 4095': ('many-chunks-centre', 'many-chunks', 'one-chunk'),
}

# Worst error over bound per row (1 = at the bound) as test_gpu_farfield_beam.py prints and records it
# (ML_RECORD_PARITY); as taken on an MI355X.  The bound is beam_bound_units(n) 2**-53 sum |term|, not these.
MEASURED = {
    # (0: the device's sums are the exactly rounded ones, or the row has no sum that rounds)
    'many-chunks': 0.032, 'many-chunks-centre': 0.025, 'exact-cone': 0.129, 'one-chunk': 0.065, 'two-chunks': 0.034,
    'pairs-chunk-plus-one': 0.120, 'pairs300': 0.125, 'one-row': 0.100, 'one-column': 0.0, 'one': 0.0, 'nothing-finite': 0.0,
    'nothing-finite-centre': 0.0, 'sums-weight-0': 0.0, 'sums': 0.032, 'peak-last': 0.0, '32-cones': 0.161, 'chunk-doubles': 0.058,
    # the four sources of the sweep test and their P_sum
    'sweep': 0.137,
}
