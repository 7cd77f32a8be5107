"""The cases of the FFT form of the finite-distance propagator (csrc/propagate_grid*.hip with propagate_grid.h; methods
'fft', 'fft-long', 'fft-tiled', 'fft-fine') that the suite runs against a high-precision reference, in one table, and the
launch variants of the product build that the table has to reach.  Plain data and pure functions, no test collects
from here: test_propagate_grid_cases.py holds every row's ``expect`` against the plan the host tools print and the
table against ``INVENTORY``; test_gpu_propagate_grid_cases.py runs the new rows on the GPU.

A row: the method, ``(nx, ny, mx, my)``, ``z``, the target origin in pitches behind the aperture's first sample, ``tile``
and ``subsample`` (None where the method has none; mx, my of 'fft-fine' are the fine targets), ``cache_kernels`` (None
but for 'fft-fine') and ``expect``: the padded or tile lengths ``L = (Lx, Ly)``, the route of each axis as
``(top_stages, lds_len)`` (grid_axis_route: rows run along y with Ly, columns along x with Lx), the tiles per axis, the
batch, the active lattices per axis and the contraction variants the row launches - 'H' in a name stands for WANT_H,
which comes from running every row as EH and as E.

``EXISTING`` names every case of the four ``*_ref`` modules with its ``expect``; sizes, distance and origin stay in the
module that owns the case (``geometry_of``).  ``ROWS`` are the cases of this table, with fields from
``propagate_grid_ref.random_fields(nx, ny, nx + ny)`` on ``propagate_grid_ref.axis``.

How a row's plan facts give its contraction variants (propagate_grid.hip propagate_grid_sets, propagate_grid_tiled.hip
propagate_tile_sets, propagate_grid_fine.hip propagate_fine_sets):
    'fft', 'fft-long':   grid_contract_kernel<H>.
    'fft-tiled':         grid_tile_contract_kernel<H, FIRST>; the first batch of a pass is FIRST = true, always; every later
                         batch is FIRST = false, so that one runs if and only if tiles > batch.
    'fft-fine', cached:  grid_fine_contract_kernel<H, FIRST, G>, one launch over all tiles per pair: FIRST = true only.
    'fft-fine', streamed: a launch per batch of tiles: FIRST = true always, FIRST = false if and only if tiles > batch.
    G:                   the lattices are taken in pairs, a single one last: G = 2 if and only if there are at least two
                         lattices, G = 1 if and only if their count is odd.
The transform kernels follow from the routes: ``grid_rows_kernel`` at Ly, or for Ly = 16384 ``grid_rows_top_kernel<2>``
and ``grid_rows_block_kernel``; ``grid_cols_kernel`` at the columns' lds_len and ``grid_cols_top_kernel<top_stages>`` above
it.  Every row runs each of them forward and back.  The padding is ``grid_pad_kernel`` ('fft', 'fft-long') or
``grid_tile_pad_kernel``; the rows upload their fields, so none has row extents - that variant is run by the tests of
``RESIDENT``, by equality with the uploaded field.

The product build ignores the ML_GRID_* knobs (they exist under -DML_DIAG only): sizes alone reach everything here.
``grid_rows_top_kernel<1>`` is launched only with the diagnostic build's ML_GRID_ROW_BLOCK knob and is no part of the
inventory.  The kernels without variants (grid_fill_kernel, grid_tile_fill_kernel, grid_crop_kernel,
grid_fine_scatter_kernel) run in every row of their method; grid_stack_fill_kernel and grid_stack_scatter_kernel are those of
'fft-stack' (propagate_stack.hip), which has no row here: tests/test_gpu_propagate_grid_stack.py runs them.

The long-double sum of a row of ``ROWS`` is taken on a subset of its targets: the four corners and targets drawn from a
fixed seed, 32 in all - 16 where the aperture holds more than 50 000 samples (the sum is 1.5 us per pair).  The NumPy
restatement of the row's method - ``propagate_grid_ref.grid_sum``, ``propagate_grid_tiled_ref.tiled_sum``,
``propagate_grid_fine_ref.fine_sum`` - is taken on every target.
"""
import collections
import functools

import numpy as np

import propagate_grid_fine_ref as fref
import propagate_grid_long_ref as lref
import propagate_grid_ref as gref
import propagate_grid_tiled_ref as tref
import propagate_ref as ref

WL, N_GLASS = gref.WL, gref.N_GLASS

Expect = collections.namedtuple('Expect', 'L rows cols tiles batch lattices contractions')
Row = collections.namedtuple('Row', 'method sizes z origin tile subsample cache_kernels expect')
# an existing case: the ``*_ref`` module that owns it (its CASES, or LONG of propagate_grid_ref), the method and mode the
# GPU tests run it with against the long-double sum (gpu False: 'g-96x80' is a case of the host test alone)
Named = collections.namedtuple('Named', 'module case method cache_kernels gpu expect')

PLAIN = ('grid_contract_kernel<H>',)
TILE_FIRST, TILE_LATER = 'grid_tile_contract_kernel<H, true>', 'grid_tile_contract_kernel<H, false>'
FINE = 'grid_fine_contract_kernel<H, %s, %d>'   # FIRST, G


def _plain(Lx, Ly, rows, cols):
    return Expect((Lx, Ly), rows, cols, None, None, None, PLAIN)


# ---- the launch variants of the product build, written out from propagate_grid_fft.hip (the transform) and
# propagate_grid.hip, propagate_grid_tiled.hip, propagate_grid_fine.hip (the contractions and the padding) -------------
INVENTORY = frozenset([
    # fft_rows: one launch of grid_rows_kernel for Ly <= 8192 - max(1, 2048 / Ly) rows per workgroup - and fft_rows_long above
    'grid_rows_kernel/16', 'grid_rows_kernel/32', 'grid_rows_kernel/64', 'grid_rows_kernel/128', 'grid_rows_kernel/256',
    'grid_rows_kernel/512', 'grid_rows_kernel/1024', 'grid_rows_kernel/2048', 'grid_rows_kernel/4096', 'grid_rows_kernel/8192',
    'grid_rows_top_kernel<2>', 'grid_rows_block_kernel',
    # fft_cols: blocks of up to 1024 in the LDS, the stages above in one streaming pass
    'grid_cols_kernel/16', 'grid_cols_kernel/32', 'grid_cols_kernel/64', 'grid_cols_kernel/128', 'grid_cols_kernel/256',
    'grid_cols_kernel/512', 'grid_cols_kernel/1024',
    'grid_cols_top_kernel<1>', 'grid_cols_top_kernel<2>', 'grid_cols_top_kernel<3>', 'grid_cols_top_kernel<4>',
    # the contractions: <WANT_H>, <WANT_H, FIRST>, <WANT_H, FIRST, G>
    'grid_contract_kernel<true>', 'grid_contract_kernel<false>',
    'grid_tile_contract_kernel<true, true>', 'grid_tile_contract_kernel<true, false>',
    'grid_tile_contract_kernel<false, true>', 'grid_tile_contract_kernel<false, false>',
    'grid_fine_contract_kernel<true, true, 1>', 'grid_fine_contract_kernel<true, true, 2>',
    'grid_fine_contract_kernel<true, false, 1>', 'grid_fine_contract_kernel<true, false, 2>',
    'grid_fine_contract_kernel<false, true, 1>', 'grid_fine_contract_kernel<false, true, 2>',
    'grid_fine_contract_kernel<false, false, 1>', 'grid_fine_contract_kernel<false, false, 2>',
    # the padding: row_first null (an uploaded field) or the row extents of a synthesised one
    'grid_pad_kernel/uploaded', 'grid_pad_kernel/row-extents', 'grid_tile_pad_kernel/uploaded', 'grid_tile_pad_kernel/row-extents',
])
# the kernels of propagate_grid*.hip and propagate_stack.hip that have no variant of their own, and the launch of the
# diagnostic build
NO_VARIANTS = frozenset(['grid_fill_kernel', 'grid_tile_fill_kernel', 'grid_crop_kernel', 'grid_fine_scatter_kernel',
                         'grid_stack_fill_kernel', 'grid_stack_scatter_kernel'])
DIAGNOSTIC = frozenset(['grid_rows_top_kernel<1>'])

# the padding with row extents: the resident (synthesised) near field of a 512^2 lens against the same arrays uploaded, by
# equality; (test module, test) - they exist already and stay as they are
RESIDENT = {
    'grid_pad_kernel/row-extents': (('test_gpu_propagate_grid', 'test_resident_equals_uploaded'),),
    'grid_tile_pad_kernel/row-extents': (('test_gpu_propagate_grid_tiled', 'test_resident_equals_uploaded'),
                                         ('test_gpu_propagate_grid_fine', 'test_resident_equals_uploaded'),
                                         # the stack pads through the tiled plan's kernel and launch
                                         ('test_gpu_propagate_grid_stack', 'test_resident_equals_uploaded')),
}

# ---- the existing cases ----------------------------------------------------------------------------------------------
_G, _L, _T, _F = 'propagate_grid_ref', 'propagate_grid_long_ref', 'propagate_grid_tiled_ref', 'propagate_grid_fine_ref'
_FIRST_2, _FIRST_1 = FINE % ('true', 2), FINE % ('true', 1)


def _fft(case, expect, gpu=True):
    return Named(_G, case, 'fft', None, gpu, expect)


def _long(case, expect):
    return Named(_L, case, 'fft-long', None, True, expect)


def _tiled(case, L, tiles, batch, rows, cols, contractions=(TILE_FIRST,)):
    return Named(_T, case, 'fft-tiled', None, True, Expect(L, rows, cols, tiles, batch, None, contractions))


def _fine(case, cached, L, tiles, batch, lattices, contractions):
    return Named(_F, case, 'fft-fine', cached, True, Expect(L, (0, L[1]), (0, L[0]), tiles, batch, lattices, contractions))


EXISTING = {
    # test_gpu_propagate_grid.py
    'a-near': _fft('a-near', _plain(128, 128, (0, 128), (0, 128))),
    'b-more-targets': _fft('b-more-targets', _plain(128, 128, (0, 128), (0, 128))),
    'c-far': _fft('c-far', _plain(128, 64, (0, 64), (0, 128))),
    'd-exact-power': _fft('d-exact-power', _plain(64, 128, (0, 128), (0, 64))),
    'e-one-target': _fft('e-one-target', _plain(64, 64, (0, 64), (0, 64))),
    'e-one-row': _fft('e-one-row', _plain(64, 64, (0, 64), (0, 64))),
    'g-96x80': _fft('g-96x80', _plain(128, 128, (0, 128), (0, 128)), gpu=False),
    'f-long': _fft('f-long', _plain(8192, 32, (0, 32), (3, 1024))),
    'f-long-y': _fft('f-long-y', _plain(32, 8192, (0, 8192), (0, 32))),
    # test_gpu_propagate_grid_long.py
    'h-long': _long('h-long', _plain(16384, 32, (0, 32), (4, 1024))),
    'h-long-y': _long('h-long-y', _plain(32, 16384, (2, 4096), (0, 32))),
    'i-5000': _long('i-5000', _plain(16384, 32, (0, 32), (4, 1024))),
    'i-5000-y': _long('i-5000-y', _plain(32, 16384, (2, 4096), (0, 32))),
    'j-both': _long('j-both', _plain(16384, 256, (0, 256), (4, 1024))),
    # test_gpu_propagate_grid_tiled.py
    'ta-near': _tiled('ta-near', (32, 64), (4, 2), 8, (0, 64), (0, 32)),
    'tb-one-target': _tiled('tb-one-target', (16, 16), (3, 3), 9, (0, 16), (0, 16)),
    'tc-far': _tiled('tc-far', (128, 64), (1, 1), 1, (0, 64), (0, 128)),
    'td-many': _tiled('td-many', (32, 32), (33, 10), 64, (0, 32), (0, 32), (TILE_FIRST, TILE_LATER)),
    'tg-default': _tiled('tg-default', (128, 256), (3, 1), 3, (0, 256), (0, 128)),
    'te-cols-top': _tiled('te-cols-top', (2048, 32), (3, 1), 3, (0, 32), (1, 1024)),
    'te-rows-long': _tiled('te-rows-long', (32, 2048), (1, 3), 3, (0, 2048), (0, 32)),
    'tf-beyond': _tiled('tf-beyond', (512, 32), (35, 1), 35, (0, 32), (0, 512)),
    # test_gpu_propagate_grid_fine.py: every case cached; two of them streamed, their tiles in one batch
    'fa-ragged': _fine('fa-ragged', True, (32, 32), (3, 2), 6, (2, 3), (_FIRST_2,)),
    'fa-ragged:streamed': _fine('fa-ragged', False, (32, 32), (3, 2), 6, (2, 3), (_FIRST_2,)),
    'fb-fewer-than-s': _fine('fb-fewer-than-s', True, (16, 16), (3, 3), 9, (3, 1), (_FIRST_2, _FIRST_1)),
    'fb-fewer-than-s:streamed': _fine('fb-fewer-than-s', False, (16, 16), (3, 3), 9, (3, 1), (_FIRST_2, _FIRST_1)),
    'fc-batches': _fine('fc-batches', True, (16, 16), (49, 10), 64, (2, 2), (_FIRST_2,)),
    'fd-eight': _fine('fd-eight', True, (64, 16), (1, 3), 3, (8, 8), (_FIRST_2,)),
    'fe-default': _fine('fe-default', True, (128, 256), (3, 1), 3, (3, 2), (_FIRST_2,)),
}

# ---- the cases of this table -----------------------------------------------------------------------------------------
_FC = fref.CASES['fc-batches']   # 'fc-streamed' is that case in the other mode
ROWS = {
    # Lx = 4096 - what a 2048^2 aperture with a 2048^2 image pads to: two streaming stages above blocks of 1024
    'k-4096x': Row('fft', (2100, 20, 1900, 12), 60e-6, (-950.5, 3.25), None, None, None, _plain(4096, 32, (0, 32), (2, 1024))),
    # rows of 4096: one row per workgroup of 512 threads, twelve stages
    'k-4096y': Row('fft', (20, 2100, 12, 1900), 60e-6, (3.25, -950.5), None, None, None, _plain(32, 4096, (0, 4096), (0, 32))),
    # rows of 1024: two rows per workgroup, ten stages - one left over in front of three groups of three (with the
    # 1024^2 of test_resident_equals_uploaded, which compares GPU with GPU)
    'k-1024y': Row('fft', (20, 600, 12, 400), 40e-6, (3.25, 100.5), None, None, None, _plain(32, 1024, (0, 1024), (0, 32))),
    # rows of 512: four rows per workgroup, nine stages - no group left over
    'k-512y': Row('fft', (40, 300, 12, 200), 30e-6, (3.25, 40.5), None, None, None, _plain(64, 512, (0, 512), (0, 64))),
    # columns of 256
    'k-256x': Row('fft', (150, 40, 100, 12), 30e-6, (-20.5, 3.25), None, None, None, _plain(256, 64, (0, 64), (0, 256))),
    # both axes mid-size at once
    'k-mid': Row('fft', (300, 140, 200, 100), 40e-6, (30.5, -20.25), None, None, None, _plain(512, 256, (0, 256), (0, 512))),
    # GRID_L_MIN under 'fft': 9 of the 128 rows of a workgroup present forward, 8 back
    'k-16': Row('fft', (9, 7, 8, 10), 5e-6, (0.5, -1.25), None, None, None, _plain(16, 16, (0, 16), (0, 16))),
    # the two streaming stages with the batched planes of a tiled plan (the geometry of 'te-cols-top')
    'tk-4096x': Row('fft-tiled', (5000, 20, 100, 12), 200e-6, (-2450.5, 3.25), (4096, 32), None, None,
                    Expect((4096, 32), (0, 32), (2, 1024), (2, 1), 2, None, (TILE_FIRST,))),
    # rows of 4096, batched (the geometry of 'te-rows-long')
    'tk-4096y': Row('fft-tiled', (20, 5000, 12, 100), 200e-6, (3.25, -2450.5), (32, 4096), None, None,
                    Expect((32, 4096), (0, 4096), (0, 32), (1, 2), 2, None, (TILE_FIRST,))),
    # the streamed fine plan across eight batches of tiles: two lattices' kernel spectra refilled per batch, the currents
    # offset by the batch's first tile; two pairs of lattices
    'fc-streamed': Row('fft-fine', _FC[:4], _FC[4], _FC[5:7], _FC[7], _FC[8], False,
                       Expect((16, 16), (0, 16), (0, 16), (49, 10), 64, (2, 2), (FINE % ('true', 2), FINE % ('false', 2)))),
    # the same with an odd count of lattices: a pair and a single one, three batches of tiles (64, 64, 12)
    'fk-odd-streamed': Row('fft-fine', (97, 40, 30, 13), 20e-6, (40.5, 10.25), (16, 16), (3, 1), False,
                           Expect((16, 16), (0, 16), (0, 16), (14, 10), 64, (3, 1),
                                  (FINE % ('true', 2), FINE % ('false', 2), FINE % ('true', 1), FINE % ('false', 1)))),
}


# ---- what a case reaches --------------------------------------------------------------------------------------------
def geometry_of(named):
    """-> (nx, ny, mx, my), tile, subsample of an existing case, from the module that owns it"""
    module = {_G: gref, _L: lref, _T: tref, _F: fref}[named.module]
    case = module.LONG[named.case] if module is gref and named.case in gref.LONG else module.CASES[named.case]
    tile = case[7] if module in (tref, fref) else None
    return tuple(case[:4]), tile, case[8] if module is fref else None


def contractions_by_rule(method, tiles, batch, lattices, cache_kernels):
    """the rule of the module's docstring, from plan facts"""
    if method in ('fft', 'fft-long'):
        return set(PLAIN)
    later = tiles[0] * tiles[1] > batch
    if method == 'fft-tiled':
        return {TILE_FIRST, TILE_LATER} if later else {TILE_FIRST}
    firsts = ['true'] + (['false'] if later and not cache_kernels else [])
    n = lattices[0] * lattices[1]
    return {FINE % (first, G) for first in firsts for G in (2, 1) if (n >= 2 if G == 2 else n % 2 == 1)}


def variants(method, expect):
    """the entries of INVENTORY that a case with this ``expect`` launches, run as EH and as E"""
    (Lx, Ly), (row_top, row_len), (col_top, col_len) = expect.L, expect.rows, expect.cols
    out = {'grid_rows_kernel/%d' % Ly} if row_top == 0 else {'grid_rows_top_kernel<%d>' % row_top, 'grid_rows_block_kernel'}
    out.add('grid_cols_kernel/%d' % col_len)
    if col_top:
        out.add('grid_cols_top_kernel<%d>' % col_top)
    out.add('grid_pad_kernel/uploaded' if method in ('fft', 'fft-long') else 'grid_tile_pad_kernel/uploaded')
    for name in expect.contractions:
        out |= {name.replace('<H', '<' + h) for h in ('true', 'false')}
    return out


def reach(method, expect):
    """the variants and, per method, the axis lengths and whether both axes are 256 or longer at once"""
    out = variants(method, expect) | {(method, 'rows', expect.L[1]), (method, 'columns', expect.L[0])}
    if min(expect.L) >= 256:
        out.add((method, 'both axes of 256 or more'))
    return out


def reached_before():
    """what the existing cases that run on the GPU against a reference reach, together"""
    out = set()
    for named in EXISTING.values():
        if named.gpu:
            out |= reach(named.method, named.expect)
    return out


# ---- the references of the rows --------------------------------------------------------------------------------------
def geometry(name):
    row = ROWS[name]
    nx, ny, mx, my = row.sizes
    x, y = gref.axis(nx), gref.axis(ny)
    if row.method == 'fft-fine':
        sx, sy = row.subsample
        return x, y, fref.fine_axis(x, row.origin[0], mx, sx), fref.fine_axis(y, row.origin[1], my, sy), row.z
    return x, y, gref.target_axis(x, row.origin[0], mx), gref.target_axis(y, row.origin[1], my), row.z


def subset(name):
    """the targets of the long-double sum: the four corners and targets drawn from a fixed seed, none twice"""
    nx, ny, mx, my = ROWS[name].sizes
    count = 16 if nx * ny > 50000 else 32
    corners = tref.corners(mx, my)
    rest = np.setdiff1d(np.arange(mx * my), corners)
    drawn = np.random.default_rng(20245).choice(rest, count - 4, replace=False)
    return np.concatenate([corners, np.sort(drawn)])


@functools.lru_cache(maxsize=None)
def reference(name):
    """as propagate_grid_ref.reference: fields F, axes x, y, targets tx, ty, z, the subset ``sub``, the long-double sum
    El, Hl on it, the NumPy form of the row's method Enp, Hnp on every target, the errors e_ref (E, H) of the plain fp64
    direct sum and e_np (E, H) of the NumPy form on the subset"""
    row = ROWS[name]
    x, y, tx, ty, z = geometry(name)
    F = gref.random_fields(x.size, y.size, x.size + y.size)
    sub = subset(name)
    i, j = sub // ty.size, sub % ty.size
    pts = np.stack([tx[i], ty[j], np.full(sub.size, z)], axis=1)
    E64, H64 = ref.direct_sum(*F, x, y, WL, N_GLASS, pts)
    El, Hl = ref.direct_sum(*F, x, y, WL, N_GLASS, pts, real=np.longdouble)
    if row.method == 'fft':
        Enp, Hnp = gref.grid_sum(*F, x, y, WL, N_GLASS, tx[0], ty[0], tx.size, ty.size, z)
    elif row.method == 'fft-tiled':
        Enp, Hnp = tref.tiled_sum(*F, x, y, WL, N_GLASS, tx[0], ty[0], tx.size, ty.size, z, tile=row.tile)
    else:
        Enp, Hnp = fref.fine_sum(*F, x, y, WL, N_GLASS, tx, ty, z, row.subsample, tile=row.tile)
    assert Enp.shape == (3, tx.size * ty.size)
    return dict(F=F, x=x, y=y, tx=tx, ty=ty, z=z, sub=sub, El=El, Hl=Hl, Enp=Enp, Hnp=Hnp,
                e_ref=(ref.max_error(E64, El), ref.max_error(H64, Hl)),
                e_np=(ref.max_error(Enp[:, sub], El), ref.max_error(Hnp[:, sub], Hl)))
