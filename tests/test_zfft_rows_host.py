"""What the fixed-shape row transform (metalens_amd/csrc/zfft_rows.hip) decides without arithmetic per lane and load,
checked on the host through the functions the kernel calls (csrc/zfft_core.h row_run, piece_lane, RowWalk,
rows_kernel_takes) by tools/zfft_rows_check.cpp, built under the address and undefined-behaviour sanitizers:

- residency: for n_valid in {2048, 1900, 4096, 3793}, every first in [0, n_valid / 2] (and past the half row), every
  (wave, n2) and every lane, the kernel's compare against load_row's predicate min(n, n_valid - 1 - n) >= first, and no
  resident sample at or beyond n_valid;
- rows: for launches of rows = 4 n (n = 24, 40, 23, 37, 3796: chunks that do and do not divide the rows) at several
  grids, every row is visited once, and the incremental (row / d, row % d) of in_rb, out_rb != in_rb, alpha_rb and
  rf_mod equal the plain division at every turn; workgroups with zero, one, an odd and an even number of turns occur;
- selection: the default call is taken, and each condition that must hold declines on its own (two resident runs,
  sub_s = 2, accumulate, other passes and residue counts ...).
No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('rows')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'zfft_rows_check_san'])
    res = subprocess.run([out + 'zfft_rows_check_san'], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr, res.stderr
    return res.stdout


def test_residency_is_load_rows_predicate_lane_by_lane(report):
    m = re.search(r'residency ok: (\d+) lanes, (\d+) loads, (\d+) skipped', report)
    assert m, report
    lanes, loads, skipped = map(int, m.groups())
    assert lanes == 64 * loads and 0 < skipped < loads


def test_rows_and_divisors_follow_the_row_counter(report):
    m = re.search(r'walk ok: (\d+) turns; workgroups with 0 / 1 / odd / even turns: (\d+) (\d+) (\d+) (\d+)', report)
    assert m, report
    assert all(int(v) > 0 for v in m.groups())


def test_only_the_fixed_shape_is_taken(report):
    assert re.search(r'takes ok: 20 calls', report), report
