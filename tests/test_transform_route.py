"""The route of a far-field transform call (metalens_amd/csrc/transform_route.h: stage kinds, layout of the row
transform's result G, allocator, row trim) for the cases DESIGN.md 4.2 / 7 state in words, computed on the host by
tools/transform_route.cpp from the plan facts ml_farfield_plan would arrive at; and the acceptance rule of the folded
GEMMs (transform_route.h fold_split) through the tool's `fold` subcommand.  No GPU."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, GEMM, STREAMED, MIXED = 0, 1, 2, 3     # include/metalens_hip.h ML_METHOD_*
BLOCK, MIRRORED, INTERLEAVED = 0, 1, 2


@pytest.fixture(scope='module')
def route(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('route')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'transform_route'])

    def run(**facts):
        args = ['%s=%d' % (k.replace('_dot_', '.'), v) for k, v in facts.items()]
        res = subprocess.run([out + 'transform_route'] + args, capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        return dict(kv.split('=') for kv in res.stdout.split())
    run.exe = out + 'transform_route'
    return run


def fft_plan(n, m, method=AUTO, passes=0, **more):
    """A square n x n aperture -> m x m directions on its own lattice of n samples (a multiple of 256)."""
    facts = dict(method=method, nx_total=n, ny=n, nxl=n, mx=m, my=m, y_dot_ok=1, y_dot_N=n, x_dot_ok=1, x_dot_N=n,
                 y_dot_passes=passes, x_dot_passes=passes)
    facts.update(more)
    return facts


def test_benchmark_route_is_tiled_in_pieces_and_trimmed(route):
    r = route(**fft_plan(4096, 512, row_first=1, trim_lo=150, trim_hi=3946))
    assert (r['stage1'], r['g_layout'], r['pieces_wanted'], r['stage2']) == ('fft', 'tiled', '1', 'fft_tiles')
    assert (r['g_ld'], r['g_bytes']) == ('4104', str(4 * 512 * 4104 * 16))
    assert (r['trim_lo'], r['trim_hi']) == ('150', '3946')
    # uploaded fields carry no row_first: every resident row
    r = route(**fft_plan(4096, 512, row_first=0, trim_lo=150, trim_hi=3946))
    assert (r['g_layout'], r['trim_lo'], r['trim_hi']) == ('tiled', '0', '4096')


def test_small_aperture_keeps_the_row_major_result(route):
    r = route(**fft_plan(2048, 256))   # 32 MiB of fields + 32 MiB of G: below the 96 MiB threshold
    assert (r['g_transposed'], r['g_layout'], r['pieces_wanted'], r['stage2']) == ('0', 'row_major', '0', 'fft')
    assert r['g_bytes'] == str(4 * 2048 * 256 * 16)


def test_two_pass_rows_are_transposed_over_one_allocation(route):
    r = route(**fft_plan(16384, 1024, passes=2))
    assert (r['g_layout'], r['pieces_wanted'], r['stage2']) == ('transposed', '0', 'fft')


def test_8192_rows_are_transposed_in_pieces(route):
    r = route(**fft_plan(8192, 512))   # 32 residues per thread group: beyond the tile column pass
    assert (r['g_layout'], r['pieces_wanted'], r['stage2']) == ('transposed', '1', 'fft')


def test_no_tiles_for_odd_bin_counts_or_mixed_radix_axes(route):
    r = route(**fft_plan(4096, 512, my=508))
    assert (r['g_layout'], r['stage2']) == ('transposed', 'fft')
    r = route(**fft_plan(3000, 512, method=MIXED, y_dot_A=10, x_dot_A=10))
    assert (r['g_layout'], r['stage2']) == ('transposed', 'fft')


def test_interleaved_shard(route):
    r = route(**fft_plan(4096, 512, nxl=2048, shard=INTERLEAVED, row_first=1, trim_lo=75, trim_hi=1973))
    assert (r['g_layout'], r['pieces_wanted'], r['stage2']) == ('row_major', '0', 'interleaved')
    assert (r['trim_lo'], r['trim_hi']) == ('75', '1973')   # (by local row)


def test_mirrored_shard_is_not_trimmed(route):
    r = route(**fft_plan(4096, 512, nxl=2048, shard=MIRRORED, row_first=1, trim_lo=150, trim_hi=1900))
    assert (r['trim_lo'], r['trim_hi']) == ('0', '2048')
    assert (r['g_layout'], r['stage2']) == ('tiled', 'fft_tiles')


def test_pair_list_takes_the_column_dot(route):
    r = route(nx_total=512, ny=512, nxl=512, mx=100, my=100, pair_list=1)
    assert (r['stage1'], r['g_layout'], r['stage2']) == ('generic', 'row_major', 'coldot')


def test_folded_stages(route):
    sym = dict(method=GEMM, nx_total=4096, ny=4096, mx=512, my=512, fold=1, fold_S=256, fold2=1, fold2_S=256)
    r = route(nxl=4096, **sym)   # 64 x 4 stage-2 tiles
    assert (r['stage1'], r['stage2'], r['gt_direct'], r['want_split1']) == ('folded', 'folded', '1', '1')
    r = route(nxl=2048, row0=0, shard=MIRRORED, **sym)
    assert (r['stage2'], r['gt_direct']) == ('folded', '1')
    r = route(nxl=2048, row0=1024, **sym)   # a block of rows has no mirror partner rows
    assert (r['stage1'], r['stage2'], r['gt_direct']) == ('folded', 'generic', '0')
    r = route(nxl=2048, row0=0, shard=MIRRORED, **dict(sym, fold2=0))
    assert r['stage2'] == 'generic_mirrored'
    # 8 x 1 stage-2 tiles do not fill the chip: the generic GEMM
    r = route(nxl=256, **dict(sym, nx_total=256, ny=256, mx=64, my=64, fold_S=32, fold2_S=32))
    assert (r['stage1'], r['stage2'], r['gt_direct']) == ('folded', 'generic', '0')
    # few rows: 32 x 4 tiles of 64 half-directions, split 5-fold for ~640 workgroups
    r = route(nxl=256, **dict(sym, nx_total=256, ny=256))
    assert (r['want_split1'], r['stage2']) == ('5', 'folded')
    # stage 1 on the lattice, stage 2 off it
    r = route(nxl=4096, **dict(sym, method=AUTO, fold=0, y_dot_ok=1, y_dot_N=4096))
    assert (r['stage1'], r['g_layout'], r['stage2'], r['gt_direct']) == ('fft', 'row_major', 'folded', '0')


@pytest.mark.parametrize('method, layout', [(AUTO, 'row_major'), (STREAMED, 'transposed'), (MIXED, 'transposed')])
def test_streamed_methods_transpose_small_apertures_too(route, method, layout):
    r = route(**fft_plan(512, 64, method=method))   # (2 residues per thread group: below the tile column pass)
    assert (r['g_layout'], r['pieces_wanted']) == (layout, '1' if layout == 'transposed' else '0')


def test_an_axis_in_sub_sequences_keeps_the_row_major_result(route):
    # 16384 samples with more wanted bins than the two-pass kernel takes: two sub-sequences of 8192
    r = route(**fft_plan(16384, 2048, y_dot_split=2, x_dot_split=2))
    assert (r['g_layout'], r['pieces_wanted'], r['stage2']) == ('row_major', '0', 'fft')
    r = route(**fft_plan(16384, 2048, x_dot_split=2))
    assert r['g_layout'] == 'row_major'


def test_diagnostic_knobs_keep_their_meaning(route):
    bench = fft_plan(4096, 512, row_first=1, trim_lo=150, trim_hi=3946)
    r = route(ML_G_TILED=0, **bench)
    assert (r['g_layout'], r['pieces_wanted'], r['stage2']) == ('transposed', '1', 'fft')
    r = route(ML_NO_ROW_TRIM=1, **bench)
    assert (r['g_layout'], r['trim_lo'], r['trim_hi']) == ('tiled', '0', '4096')
    r = route(ML_G_SKEW=4, **bench)
    assert (r['g_ld'], r['g_bytes']) == ('4100', str(4 * 512 * 4100 * 16))
    sym = dict(method=GEMM, nx_total=4096, ny=4096, nxl=4096, mx=512, my=512, fold=1, fold_S=256, fold2=1,
               fold2_S=256)
    r = route(ML_NO_GT_DIRECT=1, **sym)
    assert (r['stage1'], r['stage2'], r['gt_direct']) == ('folded', 'folded', '0')
    r = route(ML_STAGE1_SPLIT=3, **sym)
    assert (r['want_split1'], r['stage2']) == ('3', 'folded')
    r = route(ML_FOLD2_MIN_TILES=257, **sym)   # 64 x 4 stage-2 tiles
    assert (r['stage2'], r['gt_direct']) == ('generic', '0')
    r = route(ML_FOLD2_MIN_TILES=256, **sym)
    assert (r['stage2'], r['gt_direct']) == ('folded', '1')


# ---- fold_split: does a direction axis take the folded GEMM, and the split directions the planner uploads

WL, N_GLASS = 580e-9, 1.459
FOLD_N, FOLD_STEP = 200, 580e-9 / 2.2


@pytest.fixture(scope='module')
def fold(tmp_path_factory):
    """fold(u, n=, step=, exe=) -> (ok, S, has_E, v as floats) from `transform_route fold`, the doubles passed and read
    back as hexadecimal; exe='transform_route_san': the same program under the address and undefined-behaviour
    sanitizers"""
    out = str(tmp_path_factory.mktemp('fold')) + os.sep
    subprocess.check_call(['make', '-s', '-j2', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'transform_route',
                           out + 'transform_route_san'])

    def run(u, n=FOLD_N, step=FOLD_STEP, exe='transform_route'):
        args = [str(n)] + [float(v).hex() for v in (step, WL, N_GLASS)] + [float(v).hex() for v in u]
        res = subprocess.run([out + exe, 'fold'] + args, capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr, res.stderr
        got = dict(kv.split('=') for kv in res.stdout.split())
        v = [float.fromhex(t) for t in got['v'].split(',')] if got['v'] else []
        return int(got['ok']), int(got['S']), int(got['has_E']), v
    return run


def _fits_long_double(q):
    """is the rational q a number of at most 64 significant bits (what an x86 long double carries)?"""
    if q == 0:
        return True
    num, den = abs(q.numerator), q.denominator
    assert den & (den - 1) == 0                 # sums and differences of doubles are dyadic
    return (num >> ((num & -num).bit_length() - 1)).bit_length() <= 64


def _check_pair(hi, lo, exact):
    """(hi, lo) splits `exact`: hi its correctly rounded double, hi + lo within 2^-60 relative of it"""
    assert hi == float(exact)                   # (Fraction -> float rounds correctly)
    assert abs(Fraction(hi) + Fraction(lo) - exact) <= abs(exact) * Fraction(1, 2 ** 60)


def _check_uniform(fold, m, shift):
    """np.linspace over +/- 0.5, shifted: folds over ceil(m / 2) half-directions v_s = (u[m-1-s] - u[s]) / 2 about
    u_c = (u[0] + u[m-1]) / 2.  The grids are chosen so that every difference u[m-1-s] - u[s] and the sum
    u[0] + u[m-1] have at most 64 significant bits (asserted below): the long-double arithmetic of fold_split is
    then exact, and hi must be the correctly rounded exact value, not merely close to it."""
    u = np.linspace(-0.5, 0.5, m) + shift
    ok, S, has_E, v = fold(u)
    assert (ok, S, has_E) == (1, (m + 1) // 2, int(shift != 0))
    assert len(v) == 2 * S + 2
    for s in range(S):
        diff = Fraction(float(u[m - 1 - s])) - Fraction(float(u[s]))
        assert _fits_long_double(diff), (m, shift, s)
        _check_pair(v[s], v[S + s], diff / 2)
    if m % 2:
        assert v[S - 1] == 0 and v[2 * S - 1] == 0      # the middle direction is its own partner
    total = Fraction(float(u[0])) + Fraction(float(u[m - 1]))
    assert _fits_long_double(total)
    _check_pair(v[2 * S], v[2 * S + 1], total / 2)
    if not shift:
        assert v[2 * S] == 0 and v[2 * S + 1] == 0


def _check_warped(fold):
    u = np.linspace(-0.5, 0.5, 40)
    assert fold(u + 0.05 * u * u)[:2] == (0, 0)


def _symmetry_tolerance(u, n, step):
    """transform_route.h symmetry_tolerance, restated: (radians of phase per unit of asymmetry at the aperture's
    edge, the phase allowed) for the axis fold_split tests - p_max = (n - 1) / 2 samples"""
    per_u = 2 * math.pi * (N_GLASS / WL) * 0.5 * (n - 1) * abs(step)
    inherent = per_u * max(abs(float(a)) for a in u) * (2.0 ** -52) * 0.5
    return per_u, max(1e-13, 4 * inherent)


def _check_edge(fold):
    """A grid that is symmetric to the bit, then its upper end moved.  Moving u[m-1] by d moves the centre by d / 2
    while every other pair keeps its midpoint 0: the worst asymmetry is d / 2."""
    half = np.linspace(0.0, 0.5, 21)[1:]
    u = np.concatenate((-half[::-1], half))
    per_u, tol = _symmetry_tolerance(u, FOLD_N, FOLD_STEP)
    assert fold(u)[:3] == (1, 20, 0)
    # one ulp: the phase half an ulp of the largest cosine carries - the tolerance's "inherent" term, of which it
    # allows four
    ulp = np.nextafter(u[-1], 1.0) - u[-1]
    assert per_u * ulp / 2 <= tol / 4 * (1 + 1e-9)
    moved = u.copy()
    moved[-1] += ulp
    assert fold(moved)[:3] == (1, 20, 1)
    # 1000 times the tolerance
    moved[-1] = u[-1] + 2 * 1000 * tol / per_u
    assert per_u * (moved[-1] - u[-1]) / 2 > 999 * tol
    assert fold(moved)[:2] == (0, 0)


def _check_degenerate(fold):
    assert fold([0.25]) == (0, 0, 0, [])
    assert fold(np.linspace(-0.5, 0.5, 8), n=1) == (0, 0, 0, [])
    assert fold(np.linspace(-0.5, 0.5, 8), n=2)[0] == 1


FOLD_CASES = [(_check_uniform, 40, 0.0), (_check_uniform, 33, 0.0), (_check_uniform, 40, 0.1), (_check_uniform, 33, 0.1),
              (_check_warped,), (_check_edge,), (_check_degenerate,)]


@pytest.mark.parametrize('m', [40, 33])
def test_fold_split_of_a_uniform_grid_about_zero(fold, m):
    _check_uniform(fold, m, 0.0)


@pytest.mark.parametrize('m', [40, 33])
def test_fold_split_of_a_shifted_grid_carries_its_centre(fold, m):
    _check_uniform(fold, m, 0.1)


def test_a_warped_grid_does_not_fold(fold):
    _check_warped(fold)


def test_fold_acceptance_edge(fold):
    _check_edge(fold)


def test_degenerate_axes_do_not_fold(fold):
    _check_degenerate(fold)


def test_fold_cases_under_sanitizers(fold):
    """every case above through the same program under the address and undefined-behaviour sanitizers: same results,
    nothing reported (the fixture fails a run whose stderr carries a report)"""
    for check, *args in FOLD_CASES:
        check(lambda *a, **kw: fold(*a, exe='transform_route_san', **kw), *args)
