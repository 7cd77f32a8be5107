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
R = 30, as 1.03e-15 at R3 = 32), so the bound asserted is the relative one."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = (400, 800, 1000, 1200, 1440, 1800, 2000, 2400, 2700, 3000, 3600, 4500, 5400, 6000, 7200)
CASES = ((400, 400, 400, -200), (1000, 1000, 256, -128), (1440, 1440, 1440, -720), (2000, 2000, 64, -30),
         (3000, 3000, 300, 100), (3600, 3600, 512, -256), (3600, 3600, 3600, -1800))


@pytest.fixture(scope='module')
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('emul') / 'zfft_mixed_emul')
    subprocess.check_call(['g++', '-O2', '-std=c++17', os.path.join(ROOT, 'tools', 'zfft_mixed_emul.cpp'),
                           '-o', exe])
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
