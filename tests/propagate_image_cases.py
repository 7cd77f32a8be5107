"""The cases of the two reductions of a propagated image - the focus metrics (csrc/propagate_focus.hip with
propagate_focus.h, ml_propagate_focus) and the transfer function (csrc/propagate_otf.hip with propagate_otf.h,
ml_propagate_otf) - that the suite runs against a high-precision yardstick, in one table, and the kernel instantiations,
loops, tiles and chunk edges the table has to reach.  Plain data and pure functions, no test collects from here:
test_propagate_image_cases.py holds every row's ``expect`` against what the two host tools print and the table against
``INVENTORY``; test_gpu_propagate_image_cases.py runs the rows on the GPU.

A row: ``(entry, method, mx, my, planes, want_h, peak_at, expect)``.  ``entry`` is 'focus' or 'otf'; ``want_h`` 'EH', 'E' or
both; ``peak_at`` the target (i, j) that lies on the wave's axis, where the peak is (None: the middle one, (mx // 2,
my // 2)).  The aperture and the wave are those of tests/test_gpu_propagate_focus.py::_wave - 48 x 40 samples, converging on
the axis -, the targets lie on the aperture's pitch ('fft-stack': on half of it), and for 'direct' the origin is whatever
puts ``peak_at`` on the axis.  No plan refused a shape of the table, so aperture and subsampling are the same in every row.

``expect`` of a focus row: the facts of ``propagate_focus_plan`` and its ``finish`` - chunk, chunks, steps (of 512 targets per full chunk), last
(targets of the last chunk), finish_tiles (tiles of 32 partial records in the second launch), last_tile.  Of an otf row:
per frequency set ``(rows, tile, tiles, last_segments, last_segment, groups, last_rows)`` of the row pass and, under
'columns', ``(col_tiles, col_last_segments, col_last_segment)``: the facts of ``propagate_otf_plan shape``.

How a run reaches the instantiations of ``focus_chunk_kernel<FIELDS, MOMENTS, RADII>`` (ml_propagate_focus):
    radii about the peak:        <F, true, false>, then <F, false, true> about the centre the first pass left
    radii about a given centre:  <F, true, true>
    no radii:                    <F, true, false>
with FIELDS = true for a member of the last pass and false for the sums.  ``RUNS`` states per row which of these the GPU
test makes, each compared with the yardstick.  ``otf_rows_kernel<FIELDS, WANT_H, ROWS>`` has ROWS = 1 up to 8
frequencies nv and 4 above; WANT_H is the plan's.

Ties.  The peak of equals is the lowest index: within a wave, between the four waves of a workgroup, between chunks and
between the tiles of the second launch.  ``ZERO_PLANES`` are all-zero fields: every target ties.  No field of the
propagator gives a constant non-zero image, so ties of non-zero values across chunks are held only through zeros.
"""
import collections

Row = collections.namedtuple('Row', 'entry method mx my planes want_h peak_at expect')
# an existing case: the test module and the cases of its CASES it runs (with the runs that are compared with a yardstick)
Named = collections.namedtuple('Named', 'entry method mx my planes want_h peak_at expect runs')

FocusExpect = collections.namedtuple('FocusExpect', 'chunk chunks steps last finish_tiles last_tile')
RowsExpect = collections.namedtuple('RowsExpect', 'rows tile tiles last_segments last_segment groups last_rows')
ColsExpect = collections.namedtuple('ColsExpect', 'col_tiles col_last_segments col_last_segment')

FOCUS_KERNEL = 'focus_chunk_kernel<%s, %s, %s>'      # FIELDS, MOMENTS, RADII
ROWS_KERNEL = 'otf_rows_kernel<%s, %s, %d>'          # FIELDS, WANT_H, ROWS


def _b(flag):
    return 'true' if flag else 'false'


# ---- what has to be reached ------------------------------------------------------------------------------------------
INVENTORY = frozenset(
    # the six instantiations of focus_chunk_kernel, each with its sums compared
    [FOCUS_KERNEL % (_b(f), m, r) for f in (True, False) for m, r in (('true', 'true'), ('true', 'false'), ('false', 'true'))]
    + ['focus: one finish tile', 'focus: finish tiles > 1',
       'focus: chunk 1024', 'focus: chunk > 1024', 'focus: steps per chunk > 2', 'focus: last chunk of whole steps, not a whole chunk',
       'focus: sums read 16 bytes at a time, chunks > 1', 'focus: sums read 8 bytes at a time, chunks > 1',
       'focus: peak on the last target, v1 false', 'focus: peak in a ragged last chunk',
       'focus: peak on the last target of a chunk', 'focus: peak on the first target of a later chunk',
       'focus: discs cut by the plane\'s edge', 'focus: discs whole',
       "focus: result of 'direct'", "focus: result of 'fft'", "focus: result of 'fft-stack'", "focus: result of 'fft-fine'",
       "focus: result of 'fft-tiled'",
       'focus: tie of zeros across waves', 'focus: tie of zeros across chunks', 'focus: tie of zeros across finish tiles']
    # the eight instantiations of otf_rows_kernel, each over one tile and over more
    + [(ROWS_KERNEL % (_b(f), _b(h), rows)) + tiles for f in (True, False) for h in (True, False) for rows in (1, 4)
       for tiles in (', one tile', ', tiles > 1')]
    + ['otf: live rows 1', 'otf: live rows 2', 'otf: live rows 3', 'otf: live rows 4',
       'otf: ragged last segment in a later tile',
       'otf_columns_kernel, one tile', 'otf_columns_kernel, tiles > 1'])

# ---- the runs --------------------------------------------------------------------------------------------------------
# a focus run: (source, centre) with source 'fields' or 'sums' and centre 'peak', 'given' or 'none' (no radii)
PEAK_RUNS = (('fields', 'peak'), ('sums', 'peak'))
GIVEN_RUNS = (('fields', 'given'), ('sums', 'given'))
# an otf run: (source, frequency set)
FREQ_SHAPES = {'1x1': (1, 1), '5x1': (5, 1), '1x7': (1, 7), '2x8': (2, 8), '3x33': (3, 33), '3x64': (3, 64), '64x64': (64, 64)}


def _otf_runs(*sets):
    return tuple((source, key) for source in ('fields', 'sums') for key in sets)


def _focus(chunk, chunks, steps, last, finish_tiles, last_tile):
    return FocusExpect(chunk, chunks, steps, last, finish_tiles, last_tile)


_P182 = _focus(1024, 33, 2, 174, 2, 1)           # 182 x 181 = 32 942 targets
_P357 = _focus(1024, 1, 2, 357, 1, 1)            # 21 x 17
_P4270 = _focus(1024, 5, 2, 174, 1, 5)           # 70 x 61
_P143 = _focus(1024, 1, 2, 143, 1, 1)            # 13 x 11


def _small_otf(mx, my):
    """the expect of a plane of at most 256 targets along y and 1024 along x under every set of FREQ_SHAPES of the existing
    tests: one tile either way"""
    segs, seg = -(-my // 32), my - (-(-my // 32) - 1) * 32
    out = {}
    for key in ('1x1', '5x1', '1x7', '3x64', '64x64'):
        rows = 1 if FREQ_SHAPES[key][1] <= 8 else 4
        groups = -(-mx // rows)
        out[key] = RowsExpect(rows, 1024 // rows, 1, segs, seg, groups, mx - (groups - 1) * rows)
    xs = -(-mx // 32)
    out['columns'] = ColsExpect(1, xs, mx - (xs - 1) * 32)
    return out


ROWS = {
    # second finish tile; the peak on the plane's last target, in the ragged last chunk; discs cut to a quarter by two edges
    'f-tiles': Row('focus', 'direct', 182, 181, 1, ('EH',), (181, 180), _P182),
    # the peak on the last target of chunk 0 (flat 1023) and on the first of chunk 1 (1024)
    'f-seam-a': Row('focus', 'direct', 182, 181, 1, ('E',), (5, 118), _P182),
    'f-seam-b': Row('focus', 'direct', 182, 181, 1, ('E',), (5, 119), _P182),
    # the peak on the last target of an odd plane (flat 356): the lane that owns it has no second target
    'f-odd-last': Row('focus', 'direct', 21, 17, 1, ('EH',), (20, 16), _P357),
    # the smallest plane that doubles the chunk: 1 049 600 targets, 513 chunks of 2048 (four steps), the last of 1024
    'f-double': Row('focus', 'direct', 1025, 1024, 1, ('E',), (1024, 500), _focus(2048, 513, 4, 1024, 17, 1)),
    # 1147 fine targets a plane, odd: two chunks, plane 1 on an odd offset
    'f-stack': Row('focus', 'fft-stack', 37, 31, 3, ('EH', 'E'), None, _focus(1024, 2, 2, 123, 1, 2)),
    # the result buffer of the tiled plan
    'f-tiled': Row('focus', 'fft-tiled', 21, 17, 1, ('EH',), None, _P357),
    # rows of 1100 targets: ROWS = 1 in tiles 1024 + 76 (3 segments, the last of 12), ROWS = 4 in tiles 4 x 256 + 76 with three
    # live rows of four
    'o-long-y': Row('otf', 'direct', 3, 1100, 1, ('EH',), None,
                    {'1x7': RowsExpect(1, 1024, 2, 3, 12, 3, 1), '2x8': RowsExpect(1, 1024, 2, 3, 12, 3, 1),
                     '3x33': RowsExpect(4, 256, 5, 3, 12, 1, 3), '3x64': RowsExpect(4, 256, 5, 3, 12, 1, 3),
                     'columns': ColsExpect(1, 1, 3)}),
    'o-long-y-E': Row('otf', 'direct', 3, 1100, 1, ('E',), None,
                      {'1x7': RowsExpect(1, 1024, 2, 3, 12, 3, 1), '3x64': RowsExpect(4, 256, 5, 3, 12, 1, 3),
                       'columns': ColsExpect(1, 1, 3)}),
    # columns of 1100 rows: the column pass over tiles 1024 + 76
    'o-long-x': Row('otf', 'direct', 1100, 3, 1, ('EH',), None,
                    {'5x1': RowsExpect(1, 1024, 1, 1, 3, 1100, 1), '64x64': RowsExpect(4, 256, 1, 1, 3, 275, 4),
                     'columns': ColsExpect(2, 3, 12)}),
    # a second workgroup along x with one live row, over two tiles (256 + 44: two segments, the last of 12)
    'o-tail': Row('otf', 'direct', 5, 300, 1, ('E',), None,
                  {'3x64': RowsExpect(4, 256, 2, 2, 12, 2, 1), 'columns': ColsExpect(1, 1, 5)}),
}

RUNS = {
    'f-tiles': PEAK_RUNS + GIVEN_RUNS, 'f-seam-a': PEAK_RUNS, 'f-seam-b': PEAK_RUNS, 'f-odd-last': PEAK_RUNS, 'f-double': PEAK_RUNS,
    'f-stack': PEAK_RUNS + GIVEN_RUNS, 'f-tiled': PEAK_RUNS,
    'o-long-y': _otf_runs('1x7', '2x8', '3x33', '3x64'), 'o-long-y-E': _otf_runs('1x7', '3x64'),
    'o-long-x': _otf_runs('5x1', '64x64'), 'o-tail': _otf_runs('3x64'),
}
# the radii of a focus row in pitches of its targets (half-integers: on no target), and the given fractional centres
RADII = {name: (0.5, 1.5, 2.5, 3.5, 4.5) for name, row in ROWS.items() if row.entry == 'focus'}
RADII['f-double'] = (2.5, 40.5)
GIVEN_CENTRE = {'f-tiles': (100.3, 90.55), 'f-stack': (17.3, 14.55)}
GIVEN_RADII = (0.8, 1.7, 2.9, 4.4, 9.3)          # in pitches: those of test_radii_and_centres
# all-zero fields, 'direct' with H: five chunks, and 33 chunks in two finish tiles
ZERO_PLANES = {'z-70x61': (70, 61, _P4270), 'z-182x181': (182, 181, _P182)}

# ---- the existing cases: CASES of tests/test_gpu_propagate_focus.py under both entries ---------------------------------
_CASES = {   # method, mx, my, planes, want_h, focus expect
    'direct-21x17-EH': ('direct', 21, 17, 1, 'EH', _P357), 'direct-70x61-E': ('direct', 70, 61, 1, 'E', _P4270),
    'fft-21x17-E': ('fft', 21, 17, 1, 'E', _P357), 'fft-70x61-EH': ('fft', 70, 61, 1, 'EH', _P4270),
    'stack-13x11-EH': ('fft-stack', 13, 11, 3, 'EH', _P143), 'stack-13x11-E': ('fft-stack', 13, 11, 3, 'E', _P143),
}
EXISTING = {}
for _name, (_method, _mx, _my, _planes, _h, _expect) in _CASES.items():
    # test_records_against_the_yardstick: about the peak, fields and sums; test_radii_and_centres: a given centre, fields
    _runs = PEAK_RUNS + ((('fields', 'given'),) if _name == 'fft-70x61-EH' else ())
    EXISTING['focus:' + _name] = Named('focus', _method, _mx, _my, _planes, (_h,), None, _expect, _runs)
    # test_entries_against_the_yardstick: every set, fields and sums
    EXISTING['otf:' + _name] = Named('otf', _method, _mx, _my, _planes, (_h,), None, _small_otf(_mx, _my),
                                     _otf_runs('1x1', '5x1', '1x7', '3x64', '64x64'))
# test_a_plane_of_the_stack_has_the_record_of_the_plane_alone runs 'fft-fine' by equality with the stack's planes
EXISTING['focus:fine-13x11'] = Named('focus', 'fft-fine', 13, 11, 1, ('EH', 'E'), None, _P143, PEAK_RUNS)
# test_through_the_sweep: the sums of a sweep about the peak and - with the parity check of this table's pull request -
# about a given centre
EXISTING['focus:sweep-21x17-EH'] = Named('focus', 'direct', 21, 17, 1, ('EH',), None, _P357, (('sums', 'peak'), ('sums', 'given')))
# test_an_all_zero_field: 'direct-21x17-EH' and 'stack-13x11-EH', one chunk each
EXISTING_ZERO = {'z-21x17': (21, 17, _P357), 'z-stack-13x11': (13, 11, _P143)}


# ---- what a case reaches ---------------------------------------------------------------------------------------------
def peak_flat(case):
    i, j = (case.mx // 2, case.my // 2) if case.peak_at is None else case.peak_at
    return i * case.my + j


def discs_whole(case, radii):
    """whether the largest disc about the peak lies inside the plane (radii in pitches)"""
    i, j = (case.mx // 2, case.my // 2) if case.peak_at is None else case.peak_at
    reach = int(max(radii))
    return min(i, j, case.mx - 1 - i, case.my - 1 - j) >= reach


def focus_reach(case, runs, radii):
    e, P, T = case.expect, case.mx * case.my, case.mx * case.my * case.planes
    out = {"focus: result of '%s'" % case.method}
    for source, centre in runs:
        fields = _b(source == 'fields')
        if centre == 'given':
            out.add(FOCUS_KERNEL % (fields, 'true', 'true'))
        else:
            out.add(FOCUS_KERNEL % (fields, 'true', 'false'))
            if centre == 'peak':
                out.add(FOCUS_KERNEL % (fields, 'false', 'true'))
    out.add('focus: one finish tile' if e.finish_tiles == 1 else 'focus: finish tiles > 1')
    out.add('focus: chunk 1024' if e.chunk == 1024 else 'focus: chunk > 1024')
    if e.steps > 2:
        out.add('focus: steps per chunk > 2')
    if e.last < e.chunk and e.last % 512 == 0:
        out.add('focus: last chunk of whole steps, not a whole chunk')
    if e.chunks > 1 and any(source == 'sums' for source, _ in runs):
        # plane p starts at p P: I at that index, Sz (with H) T doubles behind it (focus_chunk_kernel: even_i, even_s)
        starts = [p * P for p in range(case.planes)] + ([p * P + T for p in range(case.planes)] if 'EH' in case.want_h else [])
        for s in starts:
            out.add('focus: sums read %d bytes at a time, chunks > 1' % (16 if s % 2 == 0 else 8))
    flat = peak_flat(case)
    if flat == P - 1 and P % 2 == 1:
        out.add('focus: peak on the last target, v1 false')
    if flat >= (e.chunks - 1) * e.chunk and e.last < e.chunk and e.chunks > 1:
        out.add('focus: peak in a ragged last chunk')
    if flat % e.chunk == e.chunk - 1:
        out.add('focus: peak on the last target of a chunk')
    if flat % e.chunk == 0 and flat > 0:
        out.add('focus: peak on the first target of a later chunk')
    if any(centre == 'peak' for _, centre in runs):
        out.add('focus: discs whole' if discs_whole(case, radii) else "focus: discs cut by the plane's edge")
    return out


def zero_reach(expect):
    out = {'focus: tie of zeros across waves'}          # (every plane here has more than 128 targets: two waves at least)
    if expect.chunks > 1:
        out.add('focus: tie of zeros across chunks')
    if expect.finish_tiles > 1:
        out.add('focus: tie of zeros across finish tiles')
    return out


def otf_reach(case, runs):
    out = set()
    for h in case.want_h:
        for source, key in runs:
            r = case.expect[key]
            out.add((ROWS_KERNEL % (_b(source == 'fields'), _b(h == 'EH'), r.rows)) + (', one tile' if r.tiles == 1 else ', tiles > 1'))
            if r.rows == 4:          # (rows = min(ROWS, mx - i0) of the kernel of four rows; the other has one row, always)
                out.add('otf: live rows %d' % r.last_rows)
                if r.groups > 1:
                    out.add('otf: live rows 4')
            if r.tiles > 1 and r.last_segment < 32:
                out.add('otf: ragged last segment in a later tile')
    out.add('otf_columns_kernel, one tile' if case.expect['columns'].col_tiles == 1 else 'otf_columns_kernel, tiles > 1')
    return out


def reach(name, case, runs=None):
    if case.entry == 'focus':
        return focus_reach(case, RUNS[name] if runs is None else runs, RADII.get(name, (0.5, 1.5, 2.5, 3.5, 4.5)))
    return otf_reach(case, RUNS[name] if runs is None else runs)


def reached_before():
    out = set()
    for name, named in EXISTING.items():
        out |= reach(name, named, named.runs)
    for _, _, expect in EXISTING_ZERO.values():
        out |= zero_reach(expect)
    return out


def reached_by_the_table():
    out = set()
    for name, row in ROWS.items():
        out |= reach(name, row)
    for _, _, expect in ZERO_PLANES.values():
        out |= zero_reach(expect)
    return out
