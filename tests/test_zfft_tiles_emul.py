"""The tiled stage-1 result and the column pass over it (metalens_amd/csrc/zfft_core.h tile_off, tl_*) emulated on
the host: rows stored into tiles as the row pass stores them, then the per-thread phases of zfft_tiles_kernel run
thread by thread against a direct DFT of every column in long double, plus the LDS cycles of one round.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_column_pass_matches_a_direct_dft(tmp_path):
    exe = str(tmp_path / 'zfft_tiles_emul')
    subprocess.check_call(['g++', '-O2', '-std=c++17', os.path.join(ROOT, 'tools', 'zfft_tiles_emul.cpp'),
                           '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert '-> OK' in out.stdout
    errs = [float(m) for m in re.findall(r'rel err (\S+)', out.stdout)]
    assert len(errs) >= 5 and max(errs) <= 1e-15
    # the benchmark's geometry (4096 samples -> 512 bins): conflict cycles reported, at most 1.5 x conflict-free
    line = [ln for ln in out.stdout.splitlines() if 'N= 4096 resident= [0, 4096) M= 512' in ln][0]
    got, ideal = re.search(r'= (\d+) \(conflict-free (\d+)\)', line).groups()
    assert int(got) <= 1.5 * int(ideal)
