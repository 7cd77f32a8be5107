"""The table of cases of the focus metrics and the transfer function of a propagated image
(tests/propagate_image_cases.py) against the launch-shape arithmetic itself and against the launches of
csrc/propagate_focus.hip and csrc/propagate_otf.hip: every case's ``expect`` equals what tools/propagate_focus_plan and
tools/propagate_otf_plan print for its sizes (csrc/propagate_focus.h, csrc/propagate_otf.h: the functions the kernels and
launchers call) and what the Python restatements give, the existing cases and the rows together reach ``INVENTORY``, the
inventory names every instantiation the sources launch, every row reaches something no existing case reached, and the
preconditions of the GPU assertions that need no device hold.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import propagate_focus_ref as fref
import propagate_image_cases as cases
import propagate_otf_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'metalens_amd', 'csrc')
TESTS = os.path.join(ROOT, 'tests')


@pytest.fixture(scope='module')
def tools(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('image_cases')) + os.sep
    names = ('propagate_focus_plan_san', 'propagate_otf_plan_san')
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out] + [out + n for n in names])

    def run(name, *args):
        res = subprocess.run([out + name] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and res.stderr == '', res.stdout + res.stderr
        return {k: int(v) for k, v in (kv.split('=') for kv in res.stdout.split())}
    return run


def _text(path):
    with open(path) as f:
        return f.read()


def _all_cases():
    return sorted(list(cases.ROWS.items()) + list(cases.EXISTING.items()))


def _focus_plans(tools, mx, my):
    f, r = tools('propagate_focus_plan_san', mx, my, 5), fref.plan(mx, my, 5)
    assert f == r
    more, r = tools('propagate_focus_plan_san', 'finish', mx, my), fref.finish(mx, my)
    assert more == r and more['chunks'] == f['chunks']
    f.update(more)
    return cases.FocusExpect(*(f[k] for k in cases.FocusExpect._fields))


@pytest.mark.parametrize('name', [n for n, c in _all_cases() if c.entry == 'focus'])
def test_every_focus_case_has_the_plan_it_states(tools, name):
    case = dict(_all_cases())[name]
    e = case.expect
    assert _focus_plans(tools, case.mx, case.my) == e
    # each chunk and tile count is as stated: the cut covers the plane, the tiles cover the chunks
    P = case.mx * case.my
    assert (e.chunks - 1) * e.chunk + e.last == P and 1 <= e.last <= e.chunk and e.steps * fref.STEP == e.chunk
    assert (e.finish_tiles - 1) * fref.FINISH_TILE + e.last_tile == e.chunks and 1 <= e.last_tile <= fref.FINISH_TILE
    assert case.planes * P <= 1 << 26 and set(case.want_h) <= {'EH', 'E'} and case.want_h
    assert cases.reach(name, case, getattr(case, 'runs', None)) <= cases.INVENTORY


@pytest.mark.parametrize('name', [n for n, c in _all_cases() if c.entry == 'otf'])
def test_every_otf_case_has_the_plan_it_states(tools, name):
    case = dict(_all_cases())[name]
    runs = case.runs if name in cases.EXISTING else cases.RUNS[name]
    assert {key for _, key in runs} == set(case.expect) - {'columns'} and {source for source, _ in runs} == {'fields', 'sums'}
    for key in set(case.expect) - {'columns'}:
        nu, nv = cases.FREQ_SHAPES[key]
        assert key == '%dx%d' % (nu, nv)
        f, r = tools('propagate_otf_plan_san', 'shape', case.mx, case.my, nv), oref.plan(case.mx, case.my, nv)
        assert f == r
        assert cases.RowsExpect(*(f[k] for k in cases.RowsExpect._fields)) == case.expect[key], (key, f)
        assert cases.ColsExpect(*(f[k] for k in cases.ColsExpect._fields)) == case.expect['columns'], f
        e = case.expect[key]
        assert (e.tiles - 1) * e.tile + (e.last_segments - 1) * oref.SEGMENT + e.last_segment == case.my
        assert (e.groups - 1) * e.rows + e.last_rows == case.mx
    c = case.expect['columns']
    assert (c.col_tiles - 1) * oref.TILE + (c.col_last_segments - 1) * oref.SEGMENT + c.col_last_segment == case.mx
    assert cases.reach(name, case, runs) <= cases.INVENTORY


def test_zero_planes_have_the_plans_they_state(tools):
    for mx, my, expect in list(cases.ZERO_PLANES.values()) + list(cases.EXISTING_ZERO.values()):
        assert _focus_plans(tools, mx, my) == expect and mx * my > 128
    assert sorted((e.chunks, e.finish_tiles) for _, _, e in cases.ZERO_PLANES.values()) == [(5, 1), (33, 2)]
    assert {e.chunks for _, _, e in cases.EXISTING_ZERO.values()} == {1}


def test_table_and_inventory_agree():
    before, table = cases.reached_before(), cases.reached_by_the_table()
    missing = sorted(cases.INVENTORY - before - table)
    assert not missing, 'no case of tests/propagate_image_cases.py runs %s' % missing
    assert before | table == cases.INVENTORY
    assert len(cases.INVENTORY) == 6 + 22 + 16 + 7
    assert not set(cases.ROWS) & set(cases.EXISTING)


# what no case reached before this table, stated outright
UNREACHED_BEFORE = {
    'focus_chunk_kernel<false, true, true>',          # launched by test_through_the_sweep, its sums compared with nothing
    'focus: finish tiles > 1', 'focus: chunk > 1024', 'focus: steps per chunk > 2', 'focus: last chunk of whole steps, not a whole chunk',
    'focus: sums read 8 bytes at a time, chunks > 1',
    'focus: peak on the last target, v1 false', 'focus: peak in a ragged last chunk', 'focus: peak on the last target of a chunk',
    'focus: peak on the first target of a later chunk', "focus: discs cut by the plane's edge", "focus: result of 'fft-tiled'",
    'focus: tie of zeros across chunks', 'focus: tie of zeros across finish tiles',
    'otf: live rows 3', 'otf: ragged last segment in a later tile', 'otf_columns_kernel, tiles > 1',
} | {(cases.ROWS_KERNEL % (f, h, rows)) + ', tiles > 1' for f in ('true', 'false') for h in ('true', 'false') for rows in (1, 4)}


def test_what_was_unreached_before():
    """with the sweep's record about a given centre left uncompared, as it was: the parity check of test_through_the_sweep came
    with this table"""
    before = set()
    for name, named in cases.EXISTING.items():
        runs = tuple(r for r in named.runs if not (name == 'focus:sweep-21x17-EH' and r == ('sums', 'given')))
        before |= cases.reach(name, named, runs)
    for _, _, expect in cases.EXISTING_ZERO.values():
        before |= cases.zero_reach(expect)
    assert cases.INVENTORY - before == UNREACHED_BEFORE
    assert 'focus_chunk_kernel<false, true, true>' in cases.reach('focus:sweep-21x17-EH', cases.EXISTING['focus:sweep-21x17-EH'],
                                                                  cases.EXISTING['focus:sweep-21x17-EH'].runs)
    body = _text(os.path.join(TESTS, 'test_gpu_propagate_focus.py'))
    body = body[body.index('\ndef test_through_the_sweep('):].split('\n\n\n')[0]
    assert "rec = _raw(p, np.sort(radii), (9.0, 8.0), source=-1)" in body and 'centre=(9.0, 8.0))' in body
    assert '_check_record(rec[0], want, 4, True, from_sums=True)' in body.split('image_centre=(tx[9], ty[8])')[1]


@pytest.mark.parametrize('name', sorted(cases.ROWS))
def test_every_new_row_reaches_what_no_existing_case_does(name):
    new = cases.reach(name, cases.ROWS[name]) - cases.reached_before()
    print('CASES %-12s reaches %s' % (name, sorted(new)))
    assert new
    stated = {
        'f-tiles': {'focus: finish tiles > 1', 'focus: peak in a ragged last chunk', "focus: discs cut by the plane's edge"},
        'f-seam-a': {'focus: peak on the last target of a chunk'}, 'f-seam-b': {'focus: peak on the first target of a later chunk'},
        'f-odd-last': {'focus: peak on the last target, v1 false'},
        'f-double': {'focus: chunk > 1024', 'focus: steps per chunk > 2', 'focus: last chunk of whole steps, not a whole chunk'},
        'f-stack': {'focus: sums read 8 bytes at a time, chunks > 1'}, 'f-tiled': {"focus: result of 'fft-tiled'"},
        'o-long-y': {'otf: live rows 3', 'otf: ragged last segment in a later tile'},
        'o-long-y-E': {'otf_rows_kernel<true, false, 1>, tiles > 1', 'otf_rows_kernel<false, false, 4>, tiles > 1'},
        'o-long-x': {'otf_columns_kernel, tiles > 1'}, 'o-tail': {'otf_rows_kernel<true, false, 4>, tiles > 1'},
    }
    assert stated[name] <= new, sorted(stated[name] - new)


def test_the_existing_cases_are_those_of_the_gpu_tests():
    """``EXISTING`` against CASES and FREQS of the two GPU test files, read as text and imported (they import no device)"""
    import test_gpu_propagate_focus as tf
    import test_gpu_propagate_otf as to
    for name, (method, mx, my, want_h) in tf.CASES.items():
        for entry in ('focus', 'otf'):
            n = cases.EXISTING['%s:%s' % (entry, name)]
            assert (n.method, n.mx, n.my, n.want_h) == (method, mx, my, ('EH',) if want_h else ('E',))
            assert n.planes == (3 if method == 'fft-stack' else 1)
    assert {k.split(':', 1)[1] for k in cases.EXISTING} == set(tf.CASES) | {'fine-13x11', 'sweep-21x17-EH'}
    for key, (u, v) in to.FREQS.items():
        assert cases.FREQ_SHAPES[key] == (u.size, v.size)
    for n in cases.EXISTING.values():
        if n.entry == 'otf':
            assert {key for _, key in n.runs} == set(to.FREQS)
    focus, otf = _text(os.path.join(TESTS, 'test_gpu_propagate_focus.py')), _text(os.path.join(TESTS, 'test_gpu_propagate_otf.py'))
    assert "@pytest.mark.parametrize('name', sorted(CASES))\ndef test_records_against_the_yardstick(" in focus
    assert "@pytest.mark.parametrize('name', sorted(CASES))\ndef test_entries_against_the_yardstick(" in otf
    assert "@pytest.mark.parametrize('name', ['direct-21x17-EH', 'stack-13x11-EH'])\ndef test_an_all_zero_field(" in focus
    assert "def test_radii_and_centres(ma, ctx):\n    name = 'fft-70x61-EH'" in focus


def test_the_gpu_test_runs_the_table():
    import test_gpu_propagate_image_cases as tg
    assert {name for name, _ in tg.FOCUS} | set(tg.OTF) == set(cases.ROWS)
    assert sorted(tg.FOCUS) == sorted((name, h) for name, row in cases.ROWS.items() if row.entry == 'focus' for h in row.want_h)
    for key, shape in cases.FREQ_SHAPES.items():
        u, v = tg.FREQS[key]
        assert (u.size, v.size) == shape and np.abs(u).max() <= 0.5 and np.abs(v).max() <= 0.5
    assert set(tg.FREQS) == set(cases.FREQ_SHAPES)
    text = _text(os.path.join(TESTS, 'test_gpu_propagate_image_cases.py'))
    assert 'pytestmark = pytest.mark.gpu' in text
    assert "@pytest.mark.parametrize('name', sorted(cases.ZERO_PLANES))\ndef test_an_all_zero_field_over_several_chunks(" in text
    # the helpers are imported from the two existing files, not copied
    assert not re.search(r'^def (_make|_check_record|_check_peak|_check_plane|_raw|_thin)\(', text, flags=re.M)


def test_the_inventory_names_what_the_sources_launch():
    focus, otf = _text(os.path.join(CSRC, 'propagate_focus.hip')), _text(os.path.join(CSRC, 'propagate_otf.hip'))
    # focus_launch<FIELDS>: three launches, FIELDS from two call sites each way
    got = set(re.findall(r'hipLaunchKernelGGL\(\(focus_chunk_kernel<FIELDS, (\w+), (\w+)>\)', focus))
    assert got == {('true', 'true'), ('true', 'false'), ('false', 'true')}
    assert set(re.findall(r'focus_launch<(\w+)>\(ctx->stream', focus)) == {'true', 'false'}
    assert {cases.FOCUS_KERNEL % (f, m, r) for f in ('true', 'false') for m, r in got} == {v for v in cases.INVENTORY if v.startswith('focus_chunk_kernel')}
    # otf_rows_launch<FIELDS, WANT_H>: ROWS 1 and OTF_ROWS_MANY, four call sites
    assert set(re.findall(r'hipLaunchKernelGGL\(\(otf_rows_kernel<FIELDS, WANT_H, (\w+)>\)', otf)) == {'1', 'OTF_ROWS_MANY'}
    assert set(re.findall(r'otf_rows_launch<(\w+), (\w+)>\(ctx->stream', otf)) == {(f, h) for f in ('true', 'false') for h in ('true', 'false')}
    assert len({v.replace(', one tile', '').replace(', tiles > 1', '') for v in cases.INVENTORY if v.startswith('otf_rows_kernel')}) == 8
    # the constants that decide the loops live in the headers, the kernels and launchers call the shape functions
    fh, oh = _text(os.path.join(CSRC, 'propagate_focus.h')), _text(os.path.join(CSRC, 'propagate_otf.h'))
    for name, value, text, source in (('FOCUS_FINISH_TILE', fref.FINISH_TILE, fh, focus), ('FOCUS_FINISH_THREADS', 256, fh, focus),
                                      ('OTF_TILE', oref.TILE, oh, otf), ('OTF_FEW', oref.FEW, oh, otf),
                                      ('OTF_ROWS_MANY', oref.ROWS_MANY, oh, otf), ('OTF_BATCH', oref.BATCH, oh, otf)):
        assert re.search(r'constexpr int [^;]*\b%s = %d\b' % (name, value), text), name
        assert not re.search(r'constexpr int [^;]*\b%s = ' % name, source), name
    for call, source in (('focus_finish_tiles_of(chunks)', focus), ('focus_finish_tile_chunks(chunks, t)', focus),
                         ('otf_tiles(a.my, TILE)', otf), ('otf_tile_len(a.my, TILE, tile)', otf), ('otf_live_rows(a.mx, ROWS, blockIdx.x)', otf),
                         ('otf_rows_per_group(a.nv)', otf), ('otf_tiles(mx, OTF_TILE)', otf), ('otf_tile_len(mx, OTF_TILE, tile)', otf)):
        assert call in source, call


# ---- the preconditions of the GPU assertions that need no device ---------------------------------------------------
def test_peaks_lie_where_the_table_says():
    flat = {name: cases.peak_flat(row) for name, row in cases.ROWS.items() if row.entry == 'focus'}
    assert flat['f-tiles'] == 182 * 181 - 1 and flat['f-seam-a'] == 1023 and flat['f-seam-b'] == 1024 and flat['f-odd-last'] == 356
    assert flat['f-double'] == 1024 * 1024 + 500 and flat['f-stack'] == 18 * 31 + 15 and flat['f-tiled'] == 10 * 17 + 8
    for name, row in cases.ROWS.items():
        if row.peak_at is not None:
            assert 0 <= row.peak_at[0] < row.mx and 0 <= row.peak_at[1] < row.my


def test_half_integer_radii_lie_on_no_target():
    """(q + 1/2)^2 is no sum of two squares of integers: 4 (i^2 + j^2) = (2 q + 1)^2 would make an odd square a multiple of 4.
    So about a target no target lies on a boundary, and the count inside is that of whole or cut discs, exactly: counted here
    in integers, 4 (i^2 + j^2) < (2 q + 1)^2."""
    a, b = np.meshgrid(np.arange(-41, 42), np.arange(-41, 42), indexing='ij')
    whole = {R: int((4 * (a * a + b * b) < int(2 * R) ** 2).sum()) for R in (0.5, 1.5, 2.5, 3.5, 4.5, 40.5)}
    assert [whole[R] for R in (0.5, 1.5, 2.5, 3.5, 4.5)] == [1, 9, 21, 37, 69]          # what the existing tests assert
    for name, radii in cases.RADII.items():
        row = cases.ROWS[name]
        pi, pj = divmod(cases.peak_flat(row), row.my)
        i, j = np.meshgrid(np.arange(row.mx) - pi, np.arange(row.my) - pj, indexing='ij')
        d4 = 4 * (i * i + j * j)
        for R in radii:
            assert R * 2 == int(R * 2) and int(R * 2) % 2 == 1
            assert not (d4 == int(2 * R) ** 2).any()
            inside = int((d4 < int(2 * R) ** 2).sum())
            assert (inside == whole[R]) == cases.discs_whole(row, [R]), (name, R, inside)
    # two edges cut the discs of 'f-tiles' to a quarter (with the axes through the peak: (n + 2 q + 1) / 4 ... counted above)
    row = cases.ROWS['f-tiles']
    assert not cases.discs_whole(row, cases.RADII['f-tiles']) and cases.discs_whole(cases.ROWS['f-stack'], cases.RADII['f-stack'])


def test_given_centres_keep_every_target_off_the_boundaries():
    """in index units (the pitches along x and y are equal): no target within 1e-9 (relative) of a boundary"""
    for name, (ci, cj) in cases.GIVEN_CENTRE.items():
        row = cases.ROWS[name]
        counts = []
        for R in cases.GIVEN_RADII:
            m, r2 = fref.inside((row.mx, row.my), 1.0, 1.0, ci, cj, R)
            assert (np.abs(r2 - R * R) > 1e-6 * R * R).all()
            counts.append(int(m.sum()))
        assert counts[0] >= 1 and len(set(counts)) == len(counts)
        assert ci != int(ci) and cj != int(cj)
