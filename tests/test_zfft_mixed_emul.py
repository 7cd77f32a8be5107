"""The mixed-radix pruned FFT of the method 'fft-mixed' (metalens_amd/csrc/zfft_core.h mx_*, mixed_choose) emulated
on the host: tools/zfft_mixed_emul.cpp lets the factor chooser pick N s = A x B x R, runs the per-thread phases of
zfft_mixed_kernel thread by thread against a direct DFT in long double on the lattice asked for, and prints the
relative error, the LDS cycles of the chosen padding next to the conflict-free count, and the chooser's answer for
every 2^a 3^b 5^c in [256, 8192].  No GPU.

Error bound: the same programme's 16 x 16 x R3 form on the same kind of input, also run by the emulator, is the
yardstick; the mixed cases stay within twice the larger of its two figures.  Measured (x86-64, long double
reference): 16 x 16 x 16 at 4096 -> 512 bins 4.4e-16, 16 x 16 x 32 at 8192 -> 1024 bins 1.03e-15; mixed cases 2.3e-16
(400) ... 7.6e-16 (3600 -> 3600), worst 1.04e-15 at 3000 = 10 x 10 x 30.  The error follows the length R of the
Horner sum, not the legs: the odd legs' inexact twiddles show no measurable factor (3600 = 16 x 15 x 15 -> 512:
4.1e-16 against 4.4e-16 for 4096 -> 512).  The 1e-15 that test_zfft_tiles_emul.py asserts does not fit (1.04e-15 at
R = 30, as 1.03e-15 at R3 = 32), so the bound asserted is the relative one.

The rows of tests/mixed_cases.py (every leg pair on its own and on the twice finer lattice, R = 1 ... 32, lattices
below 256 samples) go through the same phases in a second run of the emulator (`--case ...`), under the same bound:
worst 9.9e-16 at 4650 = 15 x 10 x 31.  Measured on an x86-64 host: the run without arguments 7.2 s, the 40 table
rows 1.5 s more, the module 9 s with the compilation."""
import os
import re
import subprocess

import pytest

import mixed_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = (400, 800, 1000, 1200, 1440, 1800, 2000, 2400, 2700, 3000, 3600, 4500, 5400, 6000, 7200)
CASES = ((400, 400, 400, -200), (1000, 1000, 256, -128), (1440, 1440, 1440, -720), (2000, 2000, 64, -30),
         (3000, 3000, 300, 100), (3600, 3600, 512, -256), (3600, 3600, 3600, -1800))


# the lattices 2^a 3^b 5^c in [256, 8192], not multiples of 256, for which no pair leaves 32 residues or fewer on the
# lattice itself or the twice finer one (from mixed_choose's rule: N s = A B R, s <= 2, R <= 32, N s <= 8192)
REFUSED = (384, 625, 3125, 3645, 4374, 4860, 5000, 5184, 5832, 6250, 6561, 7290, 7500, 7776, 8000, 8100)


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('emul') / 'zfft_mixed_emul')
    subprocess.check_call(['g++', '-O2', '-std=c++17', os.path.join(ROOT, 'tools', 'zfft_mixed_emul.cpp'),
                           '-o', path])
    return path


@pytest.fixture(scope='module')
def output(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert '-> OK' in out.stdout
    return out.stdout


def _mixed_lines(output):
    return [ln for ln in output.splitlines() if ln.startswith('mixed:')]


def test_mixed_phases_match_a_direct_dft(output):
    base = [float(m) for m in re.findall(r'^base16: .*rel err (\S+)', output, re.M)]
    assert len(base) == 2           # 4096 and 8192 samples
    lines = _mixed_lines(output)
    for n, valid, m, j0 in CASES:
        assert any('N= %d valid= %d ' % (n, valid) in ln and ' M= %d j0= %d ' % (m, j0) in ln for ln in lines), (n, m)
    assert any(int(re.search(r'valid= (\d+)', ln).group(1)) < int(re.search(r'N= (\d+)', ln).group(1))
               and '+ [0, 0)' in ln for ln in lines)          # an aperture shorter than its lattice
    assert any('+ [0, 0)' not in ln for ln in lines)          # a two-run residency
    errs = [float(re.search(r'rel err (\S+)', ln).group(1)) for ln in lines]
    assert len(errs) >= 9 and max(errs) <= 2 * max(base), (max(errs), base)
    # every case ran on the lattice itself or the twice finer one, never on the 256 / gcd multiple
    for ln in lines:
        n, s, a, b, r = (int(re.search(r' %s= (\d+)' % k, ln).group(1)) for k in ('N', 's', 'A', 'B', 'R'))
        assert a * b * r == n * s and s <= 2 and r <= 32, ln


def test_lds_conflicts_of_the_chosen_padding(output):
    """3600 samples -> 512 bins from -256: at most 1.5 x the conflict-free cycles (the cap of the tile test)"""
    line = [ln for ln in _mixed_lines(output) if 'N= 3600 valid= 3600' in ln and ' M= 512 j0= -256 ' in ln][0]
    got, ideal = re.search(r'= (\d+) \(conflict-free (\d+)\)', line).groups()
    assert int(got) <= 1.5 * int(ideal), line


def test_factor_chooser(output):
    choice = {}
    for ln in output.splitlines():
        if ln.startswith('choose:'):
            n = int(re.search(r'N= (\d+)', ln).group(1))
            choice[n] = None if 'none' in ln else tuple(int(re.search(r' %s= (\d+)' % k, ln).group(1)) for k in 'sABR')
    smooth = sorted(2 ** a * 3 ** b * 5 ** c for a in range(14) for b in range(9) for c in range(6)
                    if 256 <= 2 ** a * 3 ** b * 5 ** c <= 8192)
    assert sorted(choice) == smooth
    for n, ch in choice.items():
        if ch is not None:
            s, a, b, r = ch
            assert a * b * r == n * s and 1 <= s <= 2 and 1 <= r <= 32, (n, ch)
    for n in REQUIRED:
        assert choice[n] is not None, n
    # 2 x 3^7 and 3^8: no two legs up to 16 leave 32 residues or fewer
    assert choice[4374] is None and choice[6561] is None


# ---- the case table of tests/mixed_cases.py -----------------------------------------------------------------------

def _pairs_of_the_header(text=None):
    """the (A, B) of the ZF_MX_PAIRS line of zfft_core.h"""
    if text is None:
        with open(os.path.join(ROOT, 'metalens_amd', 'csrc', 'zfft_core.h')) as f:
            text = f.read()
    line = re.search(r'^#define ZF_MX_PAIRS\(X\)(.*)$', text, re.M).group(1)
    pairs = [(int(a), int(b)) for a, b in re.findall(r'X\((\d+), *(\d+)\)', line)]
    assert pairs and len(pairs) == line.count('X(')
    return pairs


def _field(ln, key):
    return int(re.search(r' %s= (-?\d+)' % key, ln).group(1))


@pytest.fixture(scope='module')
def table_lines(exe):
    """{row name: the emulator's `mixed:` line} of every row of the table, one run"""
    args = []
    for row in mixed_cases.ROWS.values():
        a0, h0, a1, h1 = row.resident or (0, row.n_lattice, 0, 0)
        args += ['--case'] + [str(v) for v in (row.n_lattice, row.n_samples, row.m_bins, row.j0, a0, h0, a1, h1)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = _mixed_lines(out.stdout)
    assert len(lines) == len(mixed_cases.ROWS), out.stdout
    for (name, row), ln in zip(mixed_cases.ROWS.items(), lines):
        got = tuple(_field(ln, k) for k in ('N', 'valid', 'M', 'j0'))
        assert got == (row.n_lattice, row.n_samples, row.m_bins, row.j0), (name, ln)
    return dict(zip(mixed_cases.ROWS, lines))


def test_the_table_states_what_the_chooser_picks(table_lines):
    """the GPU test learns from the table which kernel an axis takes: it must be what mixed_choose answers"""
    for name, row in mixed_cases.ROWS.items():
        assert tuple(_field(table_lines[name], k) for k in 'sABR') == row.expect, (name, table_lines[name])
        s, a, b, r = row.expect
        assert a * b * r == row.n_lattice * s and 2 <= row.m_bins <= row.n_lattice >= row.n_samples, name


def _gaps(pairs):
    """what the table lacks to reach every kernel and planner branch of these pairs, as readable lines"""
    rows, roles, gaps = mixed_cases.ROWS, mixed_cases.roles(), []
    on_gpu = {name for case in mixed_cases.GPU_CASES for name in case if name}
    assert on_gpu <= set(rows)
    gpu_rows = [rows[name] for name in sorted(on_gpu)]
    for a, b in pairs:
        for role in mixed_cases.ROLES:
            if not roles.get((a, b), {}).get(role):
                gaps.append('pair %d x %d never runs as %s' % (a, b, role))
        if a * b % 2 == 0 and not any(r.expect == (2, a, b, r.expect[3]) for r in gpu_rows):
            gaps.append('pair %d x %d never runs on the twice finer lattice (s = 2)' % (a, b))
    for what, found in (
            ('R = 1', any(r.expect[3] == 1 for r in gpu_rows)),
            ('R = 32', any(r.expect[3] == 32 for r in gpu_rows)),
            ('an R with a prime factor above 5', any(r.expect[3] % p == 0 for r in gpu_rows for p in (7, 11, 13, 31))),
            ('a lattice below 256 samples', any(r.n_lattice < 256 for r in gpu_rows)),
            ('an aperture shorter than its lattice at s = 2',
             any(r.expect[0] == 2 and r.n_samples < r.n_lattice for r in gpu_rows)),
            ('an s = 2 window that wraps round the lattice', any(r.expect[0] == 2 and mixed_cases.wraps(r) for r in gpu_rows)),
            ('an s = 2 window without bin 0', any(r.expect[0] == 2 and mixed_cases.without_bin_0(r) for r in gpu_rows)),
            ('two resident runs at s = 2', any(r.expect[0] == 2 and r.resident for r in rows.values()))):
        if not found:
            gaps.append('no row with ' + what)
    return gaps


def test_the_table_reaches_every_kernel():
    """every pair of ZF_MX_PAIRS in each of its three roles (2 x 8 kernel instantiations), on the twice finer lattice
    where it can be, and the edges of the residue count and the window; a pair added to the macro fails here until
    it has rows"""
    pairs = _pairs_of_the_header()
    assert len(pairs) == len(set(pairs)) >= 8
    assert _gaps(pairs) == []
    # the check itself: a ninth pair, and a table that has lost one pair's rows, are named
    assert _gaps(pairs + [(12, 10)]) == ['pair 12 x 10 never runs as %s' % r for r in mixed_cases.ROLES] + [
        'pair 12 x 10 never runs on the twice finer lattice (s = 2)']
    assert _pairs_of_the_header('#define ZF_MX_PAIRS(X) X(16, 15) X(12, 10)\n') == [(16, 15), (12, 10)]
    assert {tuple(r.expect[1:3]) for r in mixed_cases.ROWS.values()} == set(pairs)


def test_host_phases_of_every_table_row(output, table_lines):
    """the bound of test_mixed_phases_match_a_direct_dft, on every row"""
    base = [float(m) for m in re.findall(r'^base16: .*rel err (\S+)', output, re.M)]
    assert len(base) == 2
    for name, ln in table_lines.items():
        err = float(re.search(r'rel err (\S+)', ln).group(1))
        assert err <= 2 * max(base), (name, err, base)
    two = [ln for name, ln in table_lines.items() if mixed_cases.ROWS[name].resident]
    assert two and all('+ [0, 0)' not in ln and ' s= 2 ' in ln for ln in two)


def test_factor_chooser_refusals(output):
    """which 2^a 3^b 5^c lattices 'fft-mixed' leaves to what 'fft-streamed' does: exactly these"""
    choice = {int(m.group(1)): m.group(2) for m in re.finditer(r'^choose: N= (\d+) (.*)$', output, re.M)}
    candidates = [n for n in choice if n % 256]
    assert len(candidates) == 97
    assert sorted(n for n in candidates if choice[n] == 'none') == list(REFUSED)
