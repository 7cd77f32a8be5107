"""The pruned FFT on lattices of 256 R3 samples (csrc/zfft.hip: zfft_kernel, zfft_pass_kernel, zfft_multi_kernel,
zfft_tiles_kernel, zfft_interleaved_kernel, zfft_cols128_kernel - 28 production instantiations) with every row of
tests/fft_cases.py on the GPU against the CPU oracle's direct sum: which kernel and how many launches a row takes is
the table's claim, tied to the launch rules by test_fft_cases.py without a GPU; here the numbers.  The rows are small
enough for the oracle to evaluate every direction - the axis under test against a tiny other axis - and sit where the
kernels can go wrong: every residue count with an instantiation of its own and generic ones, row counts that are no
multiple of 8, odd and zero-padded sample counts, bins below and above the thread count, windows that wrap round the
lattice's end or miss bin 0, padded lattices, all three layouts of the stage-1 result, row blocks, mirrored and
interleaved shards accumulating, and the rows a synthesised field lets both stages leave out.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import fft_cases
from fft_cases import N_GLASS, WL
from test_gpu_fft import TOL
from test_gpu_parity import _record, _synthetic_lens

pytestmark = pytest.mark.gpu

VECTORS = ('Nx', 'Ny', 'Lx', 'Ly')


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


@pytest.fixture
def ctx():
    from metalens_amd import _lib
    c = _lib.default_context()
    c.set_precision('f64')
    try:
        yield c
    finally:
        c.set_method('auto')


@functools.lru_cache(maxsize=2)   # (the rows of one aperture follow each other in name order only by chance)
def _case(x_axis, y_axis):
    """fields, axes, direction grids and the oracle's answer for a pair of axes; shared, nobody writes to them"""
    from oracle import farfield_oracle
    row = fft_cases.Row(x_axis, y_axis, 0, 'whole', None)
    x, y, ux, uy = fft_cases.axes(row)
    rng = np.random.default_rng(x_axis.n * 1000 + y_axis.n)
    F = [rng.standard_normal((x_axis.n, y_axis.n)) + 1j * rng.standard_normal((x_axis.n, y_axis.n)) for _ in range(4)]
    want = farfield_oracle.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy)
    for a in F + [x, y, ux, uy] + list(want.values()):
        a.setflags(write=False)
    return F, x, y, ux, uy, want


def _worst(got, want):
    """largest error of the radiation vectors relative to each one's largest component (what TOL bounds)"""
    return max(np.abs(got[key] - want[key]).max() / np.abs(want[key]).max() for key in VECTORS)


@pytest.mark.parametrize('name', sorted(fft_cases.ROWS))
def test_every_row_matches_the_oracle(ma, ctx, name):
    from metalens_amd import _lib
    row = fft_cases.ROWS[name]
    F, x, y, ux, uy, want = _case(row.x, row.y)
    nx, ny = row.x.n, row.y.n
    ctx.set_method(fft_cases.METHOD_NAMES[row.method])
    if row.shard == 'whole':
        got = ma.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy, ctx=ctx)
        assert ctx.plan_kernels() == ('fft', 'fft')
    else:
        t = ma.FarfieldTransform(nx, ny, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux, uy, ctx=ctx)
        assert ctx.plan_kernels() == ('fft', 'fft')
        block = 0
        if row.shard[0] == 'interleaved':
            b = _lib.c_int(0)
            _lib.check(ctx.lib.ml_farfield_interleave_block(ctx.handle, row.shard[1], _lib.byref(b)))
            block = b.value
            assert block == fft_cases.INTERLEAVE[name][0]
        for k, piece in enumerate(fft_cases.pieces(row)):
            rows = fft_cases.piece_rows(row, piece, block)
            part = [np.ascontiguousarray(f[rows]) for f in F]
            _lib.check(ctx.lib.ml_fields_upload(ctx.handle, len(rows), ny, *[_lib.dptr(a) for a in part]))
            if piece[2] == 2:
                _lib.check(ctx.lib.ml_farfield_transform_interleaved_async(ctx.handle, block, row.shard[1], piece[0],
                                                                           int(k > 0)))
            else:
                t.transform(row0=piece[0], accumulate=k > 0, mirrored=piece[2] == 1)
            assert ctx.plan_kernels() == ('fft', 'fft')
        got = t.radiation_vectors()
    worst = _worst(got, want)
    print('fft-case %s x=%s y=%s %s: worst rel err %.3e' % (name, tuple(row.x), tuple(row.y), row.expect, worst))
    _record('fft_case', row=name, stage1=row.expect[0], stage2=row.expect[2], err=worst)
    for key in VECTORS:
        assert np.abs(got[key] - want[key]).max() <= TOL * np.abs(want[key]).max(), key
    if row.shard == 'whole':
        ok = ~np.isnan(want['P'])                   # directions inside the unit circle
        assert np.array_equal(np.isnan(got['P']), ~ok)
        if ok.any():
            for key in ('a_theta', 'a_phi'):
                assert np.abs(got[key][ok] - want[key][ok]).max() <= TOL * np.abs(want[key][ok]).max(), key
            assert np.abs(got['P'][ok] - want['P'][ok]).max() <= 1e-11 * want['P'][ok].max()


# ---- the rows a synthesised field lets both stages leave out (transform_route.h trim_lo / trim_hi, g_view's offset)

RESIDENT_NX, RESIDENT_NY, RESIDENT_MX = 200, 768, 40
# (method, bins along y) -> the layout of the stage-1 result: 3 residues along y, so 16 bins are two tiles of 8
RESIDENT_LAYOUTS = {'row_major': ('auto', 16), 'transposed': ('fft-streamed', 12), 'tiled': ('fft-streamed', 16)}


@functools.lru_cache(maxsize=1)
def resident_case():
    """a lens in a window 1.5 x its diameter wide along x - 200 rows of 768 samples, 34 rows at either end wholly
    outside the lens circle - and the oracle's near field on it"""
    from oracle import nearfield_oracle
    lens = _synthetic_lens(17.5e-6, 0.35, WL, switch_deg=9.0)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    x = (np.arange(RESIDENT_NX) - (RESIDENT_NX - 1) / 2) * (1.5 * R / ((RESIDENT_NX - 1) / 2))
    y = (np.arange(RESIDENT_NY) - (RESIDENT_NY - 1) / 2) * (R / ((RESIDENT_NY - 1) / 2))
    src = (0.4e-6, -0.3e-6, -lens['source_distance'], 'y')
    nf = nearfield_oracle.build_nearfield(*src, WL, lens['lens_periphery_summary'], lens['lens_center_summary'],
                                          lens['hexgridset'], x_pts=x, y_pts=y)
    ux = fft_cases.lattice(fft_cases.Axis(RESIDENT_NX, 256, RESIDENT_MX, -RESIDENT_MX // 2), x[1] - x[0])
    return lens, x, y, ux, src, nf


@pytest.mark.parametrize('layout', sorted(RESIDENT_LAYOUTS))
def test_resident_rows_outside_the_lens_are_left_out(ma, ctx, layout):
    """HotPath on synthesised fields, whose row_first lets stage 1 skip the rows outside the lens circle and stage 2
    read them as zero, through each layout of the stage-1 result.  Against the oracle's flow, and against the same
    fields downloaded and uploaded again, which carry no row_first: every row is transformed"""
    from oracle import farfield_oracle
    from metalens_amd.pipeline import HotPath
    lens, x, y, ux, src, nf = resident_case()
    method, my = RESIDENT_LAYOUTS[layout]
    uy = fft_cases.lattice(fft_cases.Axis(RESIDENT_NY, RESIDENT_NY, my, -my // 2), y[1] - y[0])
    want = farfield_oracle.farfield_direct(*nf[:4], x, y, WL, nf[7], ux, uy)
    hp = HotPath(src, WL, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'],
                 x, y, ux, uy, ctx=ctx, method=method)
    hp.step()
    hp.sync()
    got = hp.results()
    assert ctx.plan_kernels() == ('fft', 'fft')
    worst = _worst(got, want)
    print('fft-resident %s: worst rel err %.3e' % (layout, worst))
    _record('fft_resident', layout=layout, err=worst)
    for key in VECTORS + ('a_theta', 'a_phi'):
        assert np.abs(got[key] - want[key]).max() <= TOL * np.abs(want[key]).max(), key
    F = ma.build_nearfield(source_x=src[0], source_y=src[1], source_z=src[2], source_pol=src[3], wavelength=WL,
                           lens_periphery_summary=lens['lens_periphery_summary'],
                           lens_center_summary=lens['lens_center_summary'], hexgridset=lens['hexgridset'],
                           x_pts=x, y_pts=y, ctx=ctx)
    ctx.set_method(method)
    again = ma.farfield_direct(*F[:4], x, y, WL, F[7], ux, uy, ctx=ctx)
    assert ctx.plan_kernels() == ('fft', 'fft')
    diff = _worst(got, again)
    print('fft-resident %s: resident against uploaded %.3e' % (layout, diff))
    for key in VECTORS:
        assert np.abs(got[key] - again[key]).max() <= 1e-13 * np.abs(again[key]).max(), key
