"""The fixed-shape row transform (metalens_amd/csrc/zfft_rows.hip zfft_rows_kernel) against zfft_kernel, which it
replaces for whole contiguous aperture rows in one resident run (csrc/zfft_core.h rows_kernel_takes), bit for bit, and
against the CPU oracle's direct sum within the tolerance of test_gpu_fft_cases.py.  Needs an MI355X.

Which kernel stage 1 takes is the library's choice per process (METALENS_HIP_FIXED_ROWS=0: zfft_kernel for every call;
METALENS_HIP_FIXED_ROWS_GRID: the workgroups of the fixed-shape kernel), read once, so every variant runs in a fresh
child process: this file as a script, which writes the raw radiation vectors of every case.  The cases, on synthesised
fields (only those carry a row_first):

  shapes   2048 samples -> 256 bins with 24 rows per plane (8 residues), 4096 -> 512 with 40 rows (16 residues)
  layouts  of stage 1's result: tiled (zfft_rows_kernel<., true>) and transposed with a plain pitch (<., false>)
  flows    'trimmed': HotPath, stage 1 on the rows that meet the lens circle only (an odd count: rows = 4 x 19 and
           4 x 35 are no multiples of 8, so the last chunk is short); 'mirrored': the whole aperture as mirrored row
           pairs, which are not trimmed - the dark rows reach stage 1 with first = 0x7f7f7f7f and read as zero; its
           stage 2 reads two resident runs and stays with zfft_kernel
  extents  first = 0, first in the middle of a 64-sample piece, exactly on a piece edge (320 = 5 x 64, 192), past the
           half row (the dark rows): test_the_cases_have_the_row_extents checks the grids for them
  turns    default grid: one workgroup per row and some without any (zero and one turn); a grid of 24 workgroups: two
           to six turns per workgroup (odd and even counts: the loop is left from either half)

The launches outside the kernel's conditions that the API reaches - stage 2 over two resident runs (mirrored), an axis
in two sub-sequences (sub_s = 2), accumulating row blocks - run in the same children from tests/fft_cases.py's rows and
must not change either."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL = 580e-9
VECTORS = ('Nx', 'Ny', 'Lx', 'Ly')
# (rows per plane, samples, bins, the window's half width along y in lens radii)
SHAPES = {'r8': (24, 2048, 256, 0.322), 'r16': (40, 4096, 512, 0.305)}
# layout of stage 1's result -> (method, bins along x, lattice along x): 'fft-streamed' stores it transposed, in tiles
# where the column pass over tiles exists (up to 512 bins along x), with a plain pitch beyond
LAYOUTS = {'tiled': ('fft-streamed', 40, 256), 'transposed': ('fft-streamed', 520, 1024)}
FLOWS = ('trimmed', 'mirrored')
OTHER_ROWS = ('x-r8-mirrored', 'x-r48', 'x-r8-blocks', 't-r8-blocks')   # tests/fft_cases.py: outside the conditions
VARIANTS = {'generic': {'METALENS_HIP_FIXED_ROWS': '0'}, 'fixed': {}, 'fixed24': {'METALENS_HIP_FIXED_ROWS_GRID': '24'}}


@functools.lru_cache(maxsize=None)
def lens():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_parity import _synthetic_lens
    return _synthetic_lens(17.5e-6, 0.35, WL, switch_deg=9.0)


def grids(shape, layout):
    """x, y, ux, uy of a case: a window over the lens' edge along x, 0.26 um apart (the oracle wants less than half a
    wavelength) - the first 5 rows lie outside the lens circle, 19 and 35 of the 24 and 40 rows meet it - and so narrow
    along y that the inner rows are lit from sample 0"""
    import fft_cases
    nx, ny, my, sy = SHAPES[shape]
    _, mx, nlat = LAYOUTS[layout]
    R = lens()['lens_periphery_summary']['r_max_list'][-1]
    x = -1.06 * R + np.arange(nx) * 0.26e-6
    y = (np.arange(ny) - (ny - 1) / 2) * (sy * R / ((ny - 1) / 2))
    ux = fft_cases.lattice(fft_cases.Axis(nx, nlat, mx, -mx // 2), x[1] - x[0])
    uy = fft_cases.lattice(fft_cases.Axis(ny, ny, my, -my // 2), y[1] - y[0])
    return x, y, ux, uy


def row_firsts(x, y):
    """row_first as csrc/nearfield.hip row_extent_kernel defines it: per row, the smallest min(j, ny - 1 - j) over the
    samples inside the lens circle; 0x7f7f7f7f for a row outside"""
    R = lens()['lens_periphery_summary']['r_max_list'][-1]
    inside = ~(np.sqrt(x[:, None] ** 2 + y[None, :] ** 2) > R)
    j = np.arange(len(y))
    d = np.minimum(j, len(y) - 1 - j)
    return np.where(inside.any(axis=1), np.where(inside, d[None, :], len(y)).min(axis=1), 0x7f7f7f7f)


SOURCE = (0.4e-6, -0.3e-6, 'y')


def run_cases(out_path):
    """(child process) every case and the rows outside the conditions, raw vectors to out_path"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import fft_cases
    import metalens_amd as ma
    from metalens_amd import _lib
    from metalens_amd.pipeline import HotPath
    ctx = _lib.default_context()
    ctx.set_precision('f64')
    L = lens()
    src = (SOURCE[0], SOURCE[1], -L['source_distance'], SOURCE[2])
    parts = (L['lens_periphery_summary'], L['lens_center_summary'], L['hexgridset'])
    out = {}
    for shape in SHAPES:
        for layout, (method, _, _) in LAYOUTS.items():
            x, y, ux, uy = grids(shape, layout)
            hp = HotPath(src, WL, *parts, x, y, ux, uy, ctx=ctx, method=method)
            hp.step()
            hp.sync()
            got = hp.results()
            assert ctx.plan_kernels() == ('fft', 'fft')
            for key in VECTORS:
                out['%s/%s/trimmed/%s' % (shape, layout, key)] = got[key]
            ctx.set_method(method)
            F = ma.build_nearfield(source_x=src[0], source_y=src[1], source_z=src[2], source_pol=src[3], wavelength=WL,
                                   lens_periphery_summary=parts[0], lens_center_summary=parts[1], hexgridset=parts[2],
                                   x_pts=x, y_pts=y, ctx=ctx)
            t = ma.FarfieldTransform(len(x), len(y), x[1] - x[0], y[1] - y[0], WL, F[7], ux, uy, ctx=ctx)
            t.transform(row0=0, accumulate=False, mirrored=True)
            assert ctx.plan_kernels() == ('fft', 'fft')
            got = t.radiation_vectors()
            for key in VECTORS:
                out['%s/%s/mirrored/%s' % (shape, layout, key)] = got[key]
            out['%s/%s/n_glass' % (shape, layout)] = np.float64(F[7])
    for name in OTHER_ROWS:
        row = fft_cases.ROWS[name]
        x, y, ux, uy = fft_cases.axes(row)
        rng = np.random.default_rng(row.x.n * 1000 + row.y.n)
        F = [rng.standard_normal((row.x.n, row.y.n)) + 1j * rng.standard_normal((row.x.n, row.y.n)) for _ in range(4)]
        ctx.set_method(fft_cases.METHOD_NAMES[row.method])
        if row.shard == 'whole':
            got = ma.farfield_direct(*F, x, y, WL, fft_cases.N_GLASS, ux, uy, ctx=ctx)
        else:
            t = ma.FarfieldTransform(row.x.n, row.y.n, x[1] - x[0], y[1] - y[0], WL, fft_cases.N_GLASS, ux, uy, ctx=ctx)
            for k, piece in enumerate(fft_cases.pieces(row)):
                rows = fft_cases.piece_rows(row, piece)
                part = [np.ascontiguousarray(f[rows]) for f in F]
                _lib.check(ctx.lib.ml_fields_upload(ctx.handle, len(rows), row.y.n, *[_lib.dptr(a) for a in part]))
                t.transform(row0=piece[0], accumulate=k > 0, mirrored=piece[2] == 1)
            got = t.radiation_vectors()
        for key in VECTORS:
            out['other/%s/%s' % (name, key)] = got[key]
    ctx.set_method('auto')
    np.savez(out_path, **out)


if __name__ == '__main__':
    run_cases(sys.argv[1])
    sys.exit(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """{variant: the arrays its child process wrote}; one process at a time"""
    base = {k: v for k, v in os.environ.items() if not k.startswith('METALENS_HIP_FIXED_ROWS')}
    got = {}
    for name, extra in VARIANTS.items():
        path = str(tmp_path_factory.mktemp('rows') / (name + '.npz'))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(base, **extra),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (name, p.stdout[-1000:], p.stderr[-3000:])
        with np.load(path) as z:
            got[name] = {k: z[k] for k in z.files}
    return got


@functools.lru_cache(maxsize=None)
def oracle_vectors(shape, layout, n_glass):
    """the oracle's near field on the case's grid, through the oracle's direct sum; shared, nobody writes to it"""
    from oracle import farfield_oracle, nearfield_oracle
    L = lens()
    x, y, ux, uy = grids(shape, layout)
    nf = nearfield_oracle.build_nearfield(SOURCE[0], SOURCE[1], -L['source_distance'], SOURCE[2], WL,
                                          L['lens_periphery_summary'], L['lens_center_summary'], L['hexgridset'],
                                          x_pts=x, y_pts=y)
    assert nf[7] == n_glass
    want = farfield_oracle.farfield_direct(*nf[:4], x, y, WL, nf[7], ux, uy)
    for a in want.values():
        a.setflags(write=False)
    return want


@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_the_cases_have_the_row_extents(shape):
    """(no GPU work) the grids give stage 1 the row extents the kernel can go wrong at"""
    x, y, _, _ = grids(shape, 'tiled')
    first = row_firsts(x, y)
    ny = len(y)
    lit = first[first < ny]
    assert len(lit) % 2 == 1 and 4 * len(lit) % 8 != 0            # the trimmed range: a short last chunk
    assert (first[:3] > ny).all() and first[-1] == 0             # dark rows first (first past the half row): trim_lo > 0
    assert (lit == 0).any()
    assert ((lit > 0) & (lit % 64 == 0)).any()                    # exactly on a piece edge
    assert ((lit % 64 > 8) & (lit % 64 < 56)).any()               # in the middle of a piece
    print('fft-rows %s: first = %s' % (shape, first.tolist()))


@pytest.mark.parametrize('flow', FLOWS)
@pytest.mark.parametrize('layout', sorted(LAYOUTS))
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_fixed_rows_equal_the_generic_kernel_bit_for_bit(runs, shape, layout, flow):
    from test_gpu_fft import TOL
    want = oracle_vectors(shape, layout, float(runs['generic']['%s/%s/n_glass' % (shape, layout)]))
    for key in VECTORS:
        name = '%s/%s/%s/%s' % (shape, layout, flow, key)
        ref = runs['generic'][name]
        for variant in ('fixed', 'fixed24'):
            got = runs[variant][name]
            assert got.dtype == ref.dtype and got.shape == ref.shape
            assert np.array_equal(got.view(np.float64), ref.view(np.float64)), (variant, name)
        err = np.abs(runs['fixed'][name] - want[key]).max() / np.abs(want[key]).max()
        print('fft-rows %s: rel err against the oracle %.3e' % (name, err))
        assert np.abs(runs['fixed'][name] - want[key]).max() <= TOL * np.abs(want[key]).max(), name


@pytest.mark.parametrize('name', OTHER_ROWS)
def test_calls_outside_the_conditions_keep_the_generic_result(runs, name):
    for key in VECTORS:
        ref = runs['generic']['other/%s/%s' % (name, key)]
        for variant in ('fixed', 'fixed24'):
            got = runs[variant]['other/%s/%s' % (name, key)]
            assert np.array_equal(got.view(np.float64), ref.view(np.float64)), (variant, name, key)
