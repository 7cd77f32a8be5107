"""The table of cases of the FFT form of the finite-distance propagator (tests/propagate_grid_cases.py) against the plan
arithmetic itself and against the launches of csrc/propagate_grid*.hip and propagate_stack.hip: every case's ``expect`` equals what
tools/propagate_grid, propagate_grid_tiled and propagate_grid_fine print for its sizes (csrc/propagate_grid.h: the
functions the launchers call), the table reaches every launch variant of ``INVENTORY``, the inventory names every kernel
the source launches, every row of this table reaches something no earlier case reached, and the NumPy restatement of
every row holds the bound of tests/test_propagate_grid_host.py against the long-double sum.  No GPU.

Bound of the restatement: ``e_np <= 32 e_ref``, the condition of tests/test_propagate_grid_host.py - a cap that keeps the
yardstick of the GPU tests honest, not a measurement."""
import os
import re
import subprocess

import pytest

import propagate_grid_cases as cases
import propagate_grid_fine_ref as fref
import propagate_grid_long_ref as lref
import propagate_grid_ref as gref
import propagate_grid_tiled_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'metalens_amd', 'csrc')
# the files of the FFT form, one per job: the transform, the plain, the tiled and the fine pass, the plans, the stack pass
HIP = [os.path.join(CSRC, name + '.hip') for name in ('propagate_grid_fft', 'propagate_grid', 'propagate_grid_tiled', 'propagate_grid_fine',
                                                     'propagate_grid_plan', 'propagate_stack')]
TESTS = os.path.join(ROOT, 'tests')


@pytest.fixture(scope='module')
def tools(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('grid_cases')) + os.sep
    names = ('propagate_grid_san', 'propagate_grid_tiled_san', 'propagate_grid_fine_san')
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out] + [out + n for n in names])

    def run(name, *args):
        res = subprocess.run([out + name] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        assert not res.stdout.startswith('refused=1'), res.stdout
        return res.stdout
    return run


def _facts(line):
    return dict(kv.split('=') for kv in line.split())


def _routes(tools, nx, ny, mx, my):
    """-> (Lx, Ly), rows, cols of the padded lengths of these sizes: the lines ``propagate_grid ... cap`` prints from
    grid_axis_route.  One sample and L targets pad to L, so (1, 1, Lx, Ly) gives the routes of a tile of Lx x Ly"""
    lines = tools('propagate_grid_san', nx, ny, mx, my, 1, 16384).splitlines()
    plan, rows, cols = _facts(lines[0]), _facts(lines[1][len('route '):]), _facts(lines[2][len('route '):])
    assert (rows['axis'], cols['axis']) == ('rows', 'columns') and (rows['L'], cols['L']) == (plan['Ly'], plan['Lx'])
    return ((int(plan['Lx']), int(plan['Ly'])), (int(rows['top_stages']), int(rows['lds_len'])),
            (int(cols['top_stages']), int(cols['lds_len'])))


def _plan(tools, method, sizes, tile, subsample, cache_kernels, want_h):
    """-> the Expect of these sizes from the host tools, the contractions by the rule of the table"""
    nx, ny, mx, my = sizes
    tiles = batch = lattices = None
    if method in ('fft', 'fft-long'):
        if method == 'fft':   # the cap of 'fft' takes it
            f = _facts(tools('propagate_grid_san', nx, ny, mx, my, want_h))
            assert max(int(f['Lx']), int(f['Ly'])) <= gref.L_MAX
        L, rows, cols = _routes(tools, nx, ny, mx, my)
    else:
        if method == 'fft-tiled':
            f = _facts(tools('propagate_grid_tiled_san', nx, ny, mx, my, want_h, *(tile or ())))
        else:
            f = _facts(tools('propagate_grid_fine_san', nx, ny, mx, my, *subsample, want_h, int(cache_kernels), *(tile or ())))
            assert int(f['cached']) == int(cache_kernels)
            lattices = (int(f['ax']), int(f['ay']))
        tiles, batch = (int(f['cx']), int(f['cy'])), int(f['batch'])
        assert int(f['tiles']) == tiles[0] * tiles[1]
        L, rows, cols = _routes(tools, 1, 1, int(f['Lx']), int(f['Ly']))
        assert L == (int(f['Lx']), int(f['Ly']))
    rule = cases.contractions_by_rule(method, tiles, batch, lattices, cache_kernels)
    return cases.Expect(L, rows, cols, tiles, batch, lattices, rule)


def _same(expect, plan):
    assert len(set(expect.contractions)) == len(expect.contractions)
    return expect._replace(contractions=set(expect.contractions)) == plan


@pytest.mark.parametrize('want_h', [1, 0], ids=['EH', 'E'])
@pytest.mark.parametrize('name', sorted(cases.ROWS))
def test_every_row_has_the_plan_it_states(tools, name, want_h):
    row = cases.ROWS[name]
    assert (row.tile is None) == (row.method in ('fft', 'fft-long')) and (row.subsample is None) == (row.method != 'fft-fine')
    assert (row.cache_kernels is None) == (row.method != 'fft-fine')
    plan = _plan(tools, row.method, row.sizes, row.tile, row.subsample, row.cache_kernels, want_h)
    assert _same(row.expect, plan), plan
    assert plan.rows[1] << plan.rows[0] == plan.L[1] and plan.cols[1] << plan.cols[0] == plan.L[0]
    assert cases.variants(row.method, row.expect) <= cases.INVENTORY


@pytest.mark.parametrize('name', sorted(cases.EXISTING))
def test_every_existing_case_has_the_plan_the_table_states(tools, name):
    named = cases.EXISTING[name]
    sizes, tile, subsample = cases.geometry_of(named)
    for want_h in (1, 0):
        plan = _plan(tools, named.method, sizes, tile, subsample, named.cache_kernels, want_h)
        assert _same(named.expect, plan), plan
    assert cases.variants(named.method, named.expect) <= cases.INVENTORY
    # ... and what the case's own module states of it
    stated = {'propagate_grid_tiled_ref': tref.PLANS, 'propagate_grid_fine_ref': fref.PLANS}
    if named.module == 'propagate_grid_long_ref':
        assert lref.PADDED[named.case] == named.expect.L
    elif named.module in stated:
        s = stated[named.module][named.case]
        assert (s['L'], s['tiles'], s['batch']) == (named.expect.L, named.expect.tiles, named.expect.batch)
        assert named.module != 'propagate_grid_fine_ref' or s['active'] == named.expect.lattices


def _text(module):
    with open(os.path.join(TESTS, module + '.py')) as f:
        return f.read()


def test_the_table_names_every_existing_case_as_the_gpu_tests_run_it():
    owned = {'propagate_grid_ref': set(gref.CASES) | set(gref.LONG), 'propagate_grid_long_ref': set(lref.CASES),
             'propagate_grid_tiled_ref': set(tref.CASES), 'propagate_grid_fine_ref': set(fref.CASES)}
    named = {}
    for key, n in cases.EXISTING.items():
        assert key == n.case + ('' if n.cache_kernels is not False else ':streamed')
        named.setdefault(n.module, set()).add(n.case)
    assert named == owned
    assert not set(cases.ROWS) & (set(cases.EXISTING) | set().union(*owned.values()))
    # 'fft': the tuple of test_gpu_propagate_grid.py; the other three modules run every case of theirs
    line = re.search(r'^PARITY_CASES = \((.*)\)$', _text('test_gpu_propagate_grid'), flags=re.M).group(1)
    on_gpu = {n.case for n in cases.EXISTING.values() if n.module == 'propagate_grid_ref' and n.gpu}
    assert set(re.findall(r"'([^']+)'", line)) == on_gpu == owned['propagate_grid_ref'] - {'g-96x80'}
    for module, cases_of in (('test_gpu_propagate_grid_long', 'lref'), ('test_gpu_propagate_grid_tiled', 'tref'),
                             ('test_gpu_propagate_grid_fine', 'fref')):
        assert "@pytest.mark.parametrize('case', sorted(%s.CASES))\ndef test_against_the_long_double_sum(" % cases_of in _text(module)
    # streamed: the two cases of test_streamed_kernels_give_the_bits_of_cached_ones
    streamed = {n.case for n in cases.EXISTING.values() if n.cache_kernels is False}
    assert ("@pytest.mark.parametrize('case', ['fa-ragged', 'fb-fewer-than-s'])\ndef test_streamed_kernels_give_the_bits_of_cached_ones("
            in _text('test_gpu_propagate_grid_fine')) and streamed == {'fa-ragged', 'fb-fewer-than-s'}
    assert all(n.gpu for n in cases.EXISTING.values() if n.module != 'propagate_grid_ref')


def test_table_and_inventory_agree():
    reached = cases.reached_before()
    for row in cases.ROWS.values():
        reached |= cases.reach(row.method, row.expect)
    launched = {v for v in reached if isinstance(v, str)}
    assert not launched & set(cases.RESIDENT)            # no case of the table has row extents
    missing = sorted(cases.INVENTORY - launched - set(cases.RESIDENT))
    assert not missing, 'no case of tests/propagate_grid_cases.py runs %s' % missing
    assert launched | set(cases.RESIDENT) == cases.INVENTORY and len(cases.INVENTORY) == 12 + 11 + 14 + 4
    for variant, tests in cases.RESIDENT.items():
        for module, test in tests:
            text = _text(module)
            body = text[text.index('\ndef %s(' % test):].split('\n\n\n')[0]
            assert 'pytestmark = pytest.mark.gpu' in text and 'download=False' in body and 'np.array_equal(resident[key], uploaded[key])' in body
            assert ("method='fft'" in body) == variant.startswith('grid_pad_kernel')


def test_the_inventory_names_what_the_source_launches():
    texts = []
    for path in HIP:
        with open(path) as f:
            texts.append(f.read())
    text = '\n'.join(texts)
    defined = [name for t in texts for name in re.findall(r'__global__[^\n]*void (grid_\w+)\(', t)]
    assert len(defined) == len(set(defined)), sorted(defined)                            # every kernel in exactly one file
    launches = re.findall(r'hipLaunchKernelGGL\(\(?(grid_\w+)(?:<([^<>]*)>)?', text)
    kernels = {name for name, _ in launches}
    assert kernels == set(re.findall(r'__global__[^\n]*void (grid_\w+)\(', text))      # every kernel of the file is launched
    assert kernels == {re.split(r'[</]', v)[0] for v in cases.INVENTORY} | cases.NO_VARIANTS
    by_kernel = {}
    for name, args in launches:
        by_kernel.setdefault(name, set()).add(args)
    # direction is a template argument of the launcher: every transform kernel forward and back from one line each
    for name in ('grid_rows_kernel', 'grid_cols_kernel', 'grid_rows_block_kernel'):
        assert by_kernel[name] == {'INV'}
    assert {'grid_cols_top_kernel<%s>' % a.split(',')[0] for a in by_kernel['grid_cols_top_kernel']} \
        == {v for v in cases.INVENTORY if v.startswith('grid_cols_top_kernel')}
    assert {'grid_rows_top_kernel<%s>' % a.split(',')[0] for a in by_kernel['grid_rows_top_kernel']} \
        == {v for v in cases.INVENTORY if v.startswith('grid_rows_top_kernel')} | cases.DIAGNOSTIC
    assert 'diag_int("ML_GRID_ROW_BLOCK", GRID_ROW_BLOCK) == GRID_L_MAX' in text       # the one way to grid_rows_top_kernel<1>
    assert by_kernel['grid_contract_kernel'] == {'true', 'false'}
    assert by_kernel['grid_tile_contract_kernel'] == {'WANT_H, true', 'WANT_H, false'}
    assert by_kernel['grid_fine_contract_kernel'] == {'WANT_H, true, G', 'WANT_H, false, G'}
    assert set(re.findall(r'launch_tile_contract<(\w+)>\(ctx', text)) == {'true', 'false'}
    assert set(re.findall(r'launch_fine_contract<(\w+), (\d)>\(ctx', text)) == {(h, g) for h in ('true', 'false') for g in '12'}
    # the lengths: rows whole in the LDS from GRID_L_MIN to GRID_L_MAX, columns in blocks up to GRID_COL_LDS
    rows = {int(v.split('/')[1]) for v in cases.INVENTORY if v.startswith('grid_rows_kernel/')}
    cols = {int(v.split('/')[1]) for v in cases.INVENTORY if v.startswith('grid_cols_kernel/')}
    assert rows == {1 << e for e in range(4, 14)} and max(rows) == gref.L_MAX and min(rows) == gref.L_MIN
    assert cols == {1 << e for e in range(4, 11)} and max(cols) == lref.COL_LDS


# what no case reached before this table, stated outright
UNREACHED_BEFORE = {
    'grid_rows_kernel/512', 'grid_rows_kernel/1024', 'grid_rows_kernel/4096', 'grid_cols_kernel/256', 'grid_cols_top_kernel<2>',
    'grid_fine_contract_kernel<true, false, 1>', 'grid_fine_contract_kernel<true, false, 2>',
    'grid_fine_contract_kernel<false, false, 1>', 'grid_fine_contract_kernel<false, false, 2>',
}


def test_what_was_unreached_before():
    before = {v for v in cases.reached_before() if isinstance(v, str)}
    assert cases.INVENTORY - before - set(cases.RESIDENT) == UNREACHED_BEFORE


@pytest.mark.parametrize('name', sorted(cases.ROWS))
def test_every_new_row_reaches_what_no_existing_case_does(name):
    row = cases.ROWS[name]
    new = cases.reach(row.method, row.expect) - cases.reached_before()
    print('CASES %-16s reaches %s' % (name, sorted(map(str, new))))
    assert new


@pytest.mark.parametrize('name', sorted(cases.ROWS))
def test_numpy_restatement_against_the_long_double_sum(name):
    r = cases.reference(name)
    mx, my = r['tx'].size, r['ty'].size
    sub = r['sub'].tolist()
    assert {0, my - 1, (mx - 1) * my, mx * my - 1} <= set(sub) and len(set(sub)) == len(sub) and 16 <= len(sub) <= 64
    assert max(sub) < mx * my and r['Enp'].shape == r['Hnp'].shape == (3, mx * my)
    for comp, e_ref, e_np in zip('EH', r['e_ref'], r['e_np']):
        print('GRID %-16s %s: e_ref %.3e e_np %.3e ratio %.2f' % (name, comp, e_ref, e_np, e_np / e_ref))
        assert e_np <= 32 * e_ref
