"""The table of cases of the direct pair sum of the finite-distance propagator (tests/propagate_direct_cases.py) against the
launch arithmetic itself and against csrc/propagate.hip: every row's ``expect`` equals what tools/propagate_direct_plan
prints for its sizes (csrc/propagate_direct.h: the functions propagate_sets calls), plain and under the address and
undefined-behaviour sanitizers; the rows together reach ``INVENTORY``; the plain-fp64 NumPy sum meets the bound per target of
tests/propagate_ref.py at every compared target of every row; the NumPy sums give the closed form of one pair.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import propagate_direct_cases as cases
import propagate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'metalens_amd', 'csrc')
NAMES = sorted(cases.ROWS)


@pytest.fixture(scope='module')
def tools(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('direct_cases')) + os.sep
    names = ('propagate_direct_plan', 'propagate_direct_plan_san')
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out] + [out + n for n in names])

    def run(name, *args, raw=False):
        res = subprocess.run([out + name] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and res.stderr == '', res.stdout + res.stderr
        if raw:
            return [line.split() for line in res.stdout.splitlines()]
        return [{k: int(v) for k, v in (kv.split('=') for kv in line.split())} for line in res.stdout.splitlines()]
    return run


def _text(path):
    with open(path) as f:
        return f.read()


@pytest.mark.parametrize('name', NAMES)
def test_every_row_has_the_plan_it_states(tools, name):
    row = cases.ROWS[name]
    e, T = row.expect, cases.n_targets(row)
    for h in row.want_h:
        want_h = int(h == 'EH')
        plain = tools('propagate_direct_plan', T, row.nx, row.sets, want_h)
        assert plain == tools('propagate_direct_plan_san', T, row.nx, row.sets, want_h) and len(plain) == 1
        f = plain[0]
        assert (f['T'], f['tiles'], f['splits'], f['rows_min'], f['rows_max']) == (T,) + tuple(e[:4]), f
        nq = 12 if want_h else 6
        assert f['partial_bytes'] == e.splits * row.sets * nq * T * 8 and f['result_bytes'] == row.sets * (nq // 2) * T * 16
    assert cases.plan(T, row.nx) == tuple(e[:4])
    # the rows are dealt completely: workgroups of rows_max and of rows_min rows make up nx
    heavy = row.nx - e.rows_min * e.splits
    assert 0 <= heavy <= e.splits and e.rows_max == e.rows_min + (1 if 0 < heavy < e.splits else 0)
    assert e.ny_tiles * cases.TILE + e.ny_tail == row.ny and 0 <= e.ny_tail < cases.TILE
    assert set(row.want_h) <= {'EH', 'E'} and row.want_h and 1 <= row.sets <= 3 and T <= 1 << 26
    assert cases.reach(name) <= cases.INVENTORY


def test_several_shapes_in_one_call_and_the_constants(tools):
    args = []
    for name in NAMES:
        row = cases.ROWS[name]
        args += [cases.n_targets(row), row.nx, row.sets, 1]
    lines = tools('propagate_direct_plan_san', *args)
    assert [(f['tiles'], f['splits'], f['rows_min'], f['rows_max']) for f in lines] == [tuple(cases.ROWS[n].expect[:4]) for n in NAMES]
    c = tools('propagate_direct_plan_san', 'constants')[0]
    assert c == {'threads': cases.THREADS, 'tile': cases.TILE, 'max_sets': 3, 'blocks': cases.BLOCKS, 'target_rows': 5}
    # what the issue's table states for the shapes it names
    by = {n: cases.ROWS[n].expect for n in NAMES}
    assert (by['d-two-rows'].tiles, by['d-two-rows'].splits) == (25, 82) and 48 * 2 + 34 == 130
    assert by['d-three-rows'].splits == 82 and 36 * 3 + 46 * 2 == 200
    assert (by['d-splits-2'].tiles, by['d-splits-2'].splits) == (1024, 2) and (by['d-splits-1'].tiles, by['d-splits-1'].splits) == (2048, 1)
    assert by['d-sets-A-xyz'].splits == 82 < cases.ROWS['d-sets-A-xyz'].nx == 96


def test_a_target_coordinate_is_stored_exactly(tools):
    """prop_two_diff: hi = fl(x - x0) and hi + lo = x - x0 in rationals, for the coordinates of every row's compared targets and
    for pairs of very different size; the near-zone row has targets whose hi alone is off (what lo is for)"""
    import fractions
    F = fractions.Fraction
    pairs = [(1.0, 1e-30), (1e-30, 1.0), (3.0, 3.0), (-2.5e-6, 7.1e-5), (1e300, -1e284), (0.0, 5e-7), (5e-7, 0.0)]
    off = {}
    for name in NAMES:
        x, y, _ = cases.axes(name)
        p = cases.points(name)[cases.compared(name)]
        mine = [(float(v), float(x[0])) for v in p[:, 0]] + [(float(v), float(y[0])) for v in p[:, 1]]
        off[name] = sum(F(a) - F(b) != F(a - b) for a, b in mine)
        pairs += mine
    args = [v.hex() for pair in pairs for v in pair]
    plain, san = tools('propagate_direct_plan', 'diff', *args, raw=True), tools('propagate_direct_plan_san', 'diff', *args, raw=True)
    assert plain == san and len(plain) == len(pairs)
    for (a, b), (hi, lo) in zip(pairs, plain):
        hi, lo = float.fromhex(hi), float.fromhex(lo)
        assert hi == a - b and F(hi) + F(lo) == F(a) - F(b), (a, b)
        assert abs(lo) <= ref.U * abs(hi)
    assert off['d-near'] > 0 and off['d-one'] >= 0


def test_the_source_uses_the_header():
    source, header = _text(os.path.join(CSRC, 'propagate.hip')), _text(os.path.join(CSRC, 'propagate_direct.h'))
    for name, value in (('PROP_THREADS', cases.THREADS), ('PROP_TILE', cases.TILE), ('PROP_MAX_SETS', 3), ('PROP_BLOCKS', cases.BLOCKS)):
        assert re.search(r'constexpr int %s = %d;' % (name, value), header), name
        assert not re.search(r'constexpr int [^;]*\b%s = ' % name, source), name
    assert '#include "propagate_direct.h"' in source and 'hip' not in header.split('#pragma once')[1].lower()
    assert source.count('prop_two_diff(') == 2 and 'fma(-(double)i, a.dxp, tx) + a.tx_lo[tc]' in source
    assert 'fma(-(double)(j0 + s), a.dyp, ty) + ty_lo' in source
    for call in ('prop_tiles(T)', 'prop_splits(T, ctx->fields.nx)', 'prop_partial_bytes(T, ctx->fields.nx, n, pp.want_h)',
                 'prop_result_bytes(T, n, pp.want_h)'):
        assert call in source, call
    # the six instantiations of the inventory are the ones the source launches
    assert set(re.findall(r'hipLaunchKernelGGL\(\(propagate_kernel<WANT_H, (\d)>\)', source)) == {'1', '2', '3'}
    assert set(re.findall(r'launch_pairs<(\w+)>\(ctx->stream', source)) == {'true', 'false'}
    assert propagate_direct_h_in_makefile()


def propagate_direct_h_in_makefile():
    import makefile_deps
    return makefile_deps.header_is_prerequisite('propagate_direct.h', 'propagate')


def test_table_and_inventory_agree():
    reached = cases.reached_by_the_table()
    missing = sorted(cases.INVENTORY - reached)
    assert not missing, 'no row of tests/propagate_direct_cases.py reaches %s' % missing
    assert reached == cases.INVENTORY and len(cases.INVENTORY) == 6 + 5 + 6 + 5 + 1 + 4 + 2
    # every row is compared with the long-double sum (the GPU test runs the whole table, variant by variant)
    import test_gpu_propagate_direct_cases as tg
    assert sorted(tg.CASES) == sorted((name, h) for name in NAMES for h in cases.ROWS[name].want_h)
    text = _text(os.path.join(ROOT, 'tests', 'test_gpu_propagate_direct_cases.py'))
    assert 'pytestmark = pytest.mark.gpu' in text
    # the helpers are imported from the existing files, not copied
    assert not re.search(r'^def (_batch|_lens|_select|_sums_ref|_check_sums|_stack|_upload|_axes|fields)\(', text, flags=re.M)
    stated = {
        'd-one': {'T == 1', 'an axis of one sample'}, 'd-wave-64': {'T == 64', 'splits == nx'}, 'd-wave-65': {'T == 65'},
        'd-tile-256': {'T == 256'}, 'd-tile-257': {'T == 257'}, 'd-ny-1': {'an axis of one sample', 'ny <= 64'},
        'd-ny-64': {'ny <= 64'}, 'd-ny-65': {'64 < ny < 128'}, 'd-ny-128': {'ny == 128'}, 'd-ny-129': {'ny == 129'},
        'd-ny-256': {'ny of exactly two tiles'}, 'd-ny-257': {'ny of two tiles and a tail'},
        'd-two-rows': {'splits < nx, rows_min < rows_max'}, 'd-three-rows': {'rows_max >= 3'}, 'd-splits-2': {'splits == 2'},
        'd-splits-1': {'splits == 1 by the tile count, nx > 1'},
        'd-near': {'target in the near zone, k R < 1', 'target exactly above a sample, dx = dy = 0'},
        'd-sets-A-xyz': {cases.KERNEL % ('true', 3), cases.KERNEL % ('false', 3), cases.LIVE_THEN_SKIP},
        'd-sets-A-xy': {cases.KERNEL % ('true', 2), cases.KERNEL % ('false', 2)},
        'd-skip-first': {cases.SKIP_THEN_LIVE}, 'd-extent-span': {cases.EXTENT_SPAN},
    }
    assert set(stated) == set(NAMES)
    for name in NAMES:
        assert stated[name] <= cases.reach(name), (name, sorted(stated[name] - cases.reach(name)))


@pytest.mark.parametrize('name', NAMES)
def test_the_compared_targets(name):
    row = cases.ROWS[name]
    T, at = cases.n_targets(row), cases.compared(name)
    assert at.size == min(T, cases.MAX_COMPARED) and np.array_equal(at, np.unique(at)) and 0 <= at[0] and at[-1] == T - 1
    assert {t for t in (0, 63, 64, 255, 256, T - 1) if t < T} <= set(at.tolist())
    pts = cases.points(name)
    assert pts.shape == (T, 3) and (pts[:, 2] > 0).all()
    if row.targets[0] == 'plane':
        _, mx, my = row.targets
        assert {0, my - 1, (mx - 1) * my, mx * my - 1} <= set(at.tolist())
        tx, ty, tz, point_list = cases.targets(name)
        assert not point_list and np.array_equal(pts[my - 1], [tx[0], ty[-1], tz[0]]) and np.array_equal(pts[(mx - 1) * my], [tx[-1], ty[0], tz[0]])


def test_window_a_is_the_one_of_the_sets_test():
    import test_gpu_propagate_sets as ts
    for name in ('d-sets-A-xyz', 'd-sets-A-xy'):
        x, y, _ = cases.axes(name)
        wx, wy = ts._window('A')
        assert np.array_equal(x, wx) and np.array_equal(y, wy)
        (px, py, pz), kw = ts._targets('plane', x, y)
        tx, ty, tz, point_list = cases.targets(name)
        assert np.array_equal(tx, px) and np.array_equal(ty, py) and tz[0] == pz and point_list == kw['point_list']
        assert getattr(ts, cases.RESIDENT[name][2])[2] == 'xyz'[:cases.ROWS[name].sets]
    assert cases.ONE_DIPOLE[1] == ts.DIPOLES[1] and cases.PITCH == ts.PITCH and cases.WL == ts.WL
    # the mirrored window: the same rows in the opposite order
    assert np.array_equal(cases.axes('d-skip-first')[0], -cases.axes('d-sets-A-xyz')[0][::-1])


def test_the_stand_in_fields_show_what_the_resident_rows_claim():
    """random fields cut to the lens' disc show the claims of every resident row - the geometry holds them; the GPU test
    asserts them from the synthesised fields"""
    for name, row in cases.ROWS.items():
        if row.state == 'resident':
            assert set(row.claims) <= cases.claims_shown(cases.stand_in_fields(name), row.expect.splits), name
        else:
            assert not row.claims
            assert not cases.claims_shown(cases.uploaded_fields(name), row.expect.splits)


def test_the_near_zone_row():
    assert cases.exactly_above('d-near') == [0, 1, 2, 3]
    kR = cases.nearest_kR('d-near')
    assert 0.25 < kR < 1 and kR == pytest.approx(cases.K * cases.NEAR_Z, rel=1e-12)
    assert len(cases.NEAR) == 40 == len(set(cases.NEAR))
    # every other row stays out of it
    assert all(cases.nearest_kR(n) > 1 for n in NAMES if n != 'd-near' and cases.ROWS[n].state != 'resident')


@pytest.mark.parametrize('name', NAMES)
def test_the_fp64_numpy_sum_meets_the_bound_per_target(name):
    """uploaded rows: the fields the GPU test uploads; resident rows: stand-in fields of the row's shape and extents (the GPU
    test asserts the same for the synthesised fields)"""
    row = cases.ROWS[name]
    F = cases.stand_in_fields(name) if row.state == 'resident' else cases.uploaded_fields(name)
    y = cases.yardstick(name, F)
    print('BOUND direct-case %-14s fp64 NumPy: e_ref E %.3e H %.3e, worst error / bound E %.4f H %.4f, largest q %.3f'
          % (name, y.eE_ref, y.eH_ref, y.ratio_E64, y.ratio_H64, y.q_max))
    assert (y.q_max > 1) == (name == 'd-near')
    assert y.ratio_E64 <= 1 and y.ratio_H64 <= 1
    assert (y.bound_E > 0).all() and (y.bound_H > 0).all()
    # the bound is one of each target's own terms: it follows the targets' amplitudes over the row
    assert (np.abs(y.El).max(axis=0) <= y.bound_E / (ref.BOUND_C0 * ref.U)).all()


def test_one_pair_has_its_closed_form():
    name = 'd-one'
    F = cases.uploaded_fields(name)
    x, y, pitch = cases.axes(name)
    pts = cases.points(name)
    assert pts.shape == (1, 3) and x.size == y.size == 1
    Ec, Hc = ref.one_pair(*[f[0, 0] for f in F], (x[0], y[0]), cases.WL, cases.N_GLASS, pts[0], pitch)
    El, Hl = ref.direct_sum(*F, x, y, cases.WL, cases.N_GLASS, pts, real=np.longdouble, pitch=pitch)
    E64, H64 = ref.direct_sum(*F, x, y, cases.WL, cases.N_GLASS, pts, pitch=pitch)
    assert np.abs(Ec).min() > 0 and np.abs(Hc).min() > 0
    for got, want in ((El[:, 0], Ec), (Hl[:, 0], Hc)):
        assert np.abs(got - want).max() <= 64 * float(np.finfo(np.longdouble).eps) * np.abs(want).max()
    for got, want in ((E64[:, 0], Ec), (H64[:, 0], Hc)):
        assert np.abs(got.astype(np.clongdouble) - want).max() <= 64 * ref.U * np.abs(want).max()
