"""The GEMM path of the far-field transform - the folded even/odd GEMMs (csrc/zfold.hip zfold_kernel, 12 production
instantiations) and the generic complex GEMM (csrc/zgemm.hip zgemm_kernel, three tiles) - with every row of
tests/gemm_cases.py on the GPU against the CPU oracle's direct sum: which kernel and how many split-K slabs a row
takes is the table's claim, tied to the launch rules by test_gemm_cases.py without a GPU; here the numbers.  The
rows are small enough for the oracle to evaluate every direction, and ragged where the kernels can go wrong: the
wide tile's last column tile with 2 half-directions, row counts that are no multiple of 32, odd sample and
direction counts, split-K chunks of 2 pairs, slabs summed on the way in, transposed and modulated output, row
blocks and mirrored shards accumulating.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import gemm_cases
from test_gpu_parity import TOL, TOL_F32, _record, _synthetic_lens

pytestmark = pytest.mark.gpu

WL, N_GLASS = 580e-9, 1.459
VECTORS = ('Nx', 'Ny', 'Lx', 'Ly')

# fp32 rows whose error against the oracle exceeds TOL_F32 get twice the measured value here, with the figure - once
# it has been judged against what fp32 accumulation over the row's reduction length allows, sqrt(K) 2^-24 of the
# maximum with the rotations re-seeded every 64 samples (the convention of test_gpu_parity.py POINTWISE)
ROW_TOL_F32 = {}


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


@pytest.fixture
def ctx():
    from metalens_amd import _lib
    c = _lib.default_context()
    c.set_method('gemm')
    c.set_precision('f64')
    try:
        yield c
    finally:
        c.set_method('auto')
        c.set_precision('f64')


def _grid(m, symmetric, about_zero, lo, hi):
    if symmetric and about_zero:
        u = np.linspace(-hi, hi, m)
        return 0.5 * (u - u[::-1])                  # exactly antisymmetric: no modulation
    u = np.linspace(lo, hi, m)
    if not symmetric:
        u = u + 0.03 * np.linspace(0, 1, m) ** 2    # warped: the generic GEMM of that axis
    return u


@functools.lru_cache(maxsize=2)   # (the fp64 and the fp32 row of a case follow each other)
def _case(shape, sym_x, sym_y, uc0):
    """fields, axes, direction grids and the oracle's answer of a table row; shared, nobody writes to them"""
    from oracle import farfield_oracle
    nx, ny, mx, my = shape
    rng = np.random.default_rng(nx * 1000 + ny)
    F = [rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny)) for _ in range(4)]
    x = (np.arange(nx) - 3.3) * (WL / 2.2)
    y = (np.arange(ny) + 11.1) * (WL / 2.3)
    ux = _grid(mx, sym_x, uc0, -0.61, 0.55)
    uy = _grid(my, sym_y, uc0, -0.3, 0.86)          # (the corners of the grid lie outside the unit circle)
    want = farfield_oracle.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy)
    for a in F + [x, y, ux, uy] + list(want.values()):
        a.setflags(write=False)
    return F, x, y, ux, uy, want


def _worst(got, want):
    """largest error of the radiation vectors relative to each one's largest component (what TOL bounds)"""
    return max(np.abs(got[key] - want[key]).max() / np.abs(want[key]).max() for key in VECTORS)


def _stage_kinds(row):
    return tuple('folded' if k.startswith('zfold') else 'gemm' for k in (row.expect[0], row.expect[2]))


@pytest.mark.parametrize('name', sorted(gemm_cases.ROWS))
def test_every_row_matches_the_oracle(ma, ctx, name):
    from metalens_amd import _lib
    row = gemm_cases.ROWS[name]
    F, x, y, ux, uy, want = _case(row.shape, row.sym_x, row.sym_y, row.uc0)
    nx, ny = row.shape[:2]
    f32 = row.precision == 'f32'
    tol = ROW_TOL_F32.get(name, TOL_F32) if f32 else TOL
    if row.shard == 'whole':
        got = ma.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy, ctx=ctx, precision=row.precision)
        assert ctx.plan_kernels() == _stage_kinds(row)
    else:
        t = ma.FarfieldTransform(nx, ny, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux, uy, ctx=ctx,
                                 precision=row.precision)
        for k, (row0, nxl, mirrored) in enumerate(gemm_cases.pieces(row)):
            rows = np.concatenate((np.arange(row0, row0 + nxl // 2), np.arange(nx - row0 - nxl // 2, nx - row0))) \
                if mirrored else np.arange(row0, row0 + nxl)
            part = [np.ascontiguousarray(f[rows]) for f in F]
            _lib.check(ctx.lib.ml_fields_upload(ctx.handle, len(rows), ny, *[_lib.dptr(a) for a in part]))
            t.transform(row0=row0, accumulate=k > 0, mirrored=mirrored)
            assert ctx.plan_kernels() == _stage_kinds(row)
        got = t.radiation_vectors()
    worst = _worst(got, want)
    print('gemm-case %s %s %s: worst rel err %.3e' % (name, row.shape, row.expect, worst))
    _record('gemm_case', row=name, stage1=row.expect[0], stage2=row.expect[2], err=worst)
    for key in VECTORS:
        assert np.abs(got[key] - want[key]).max() <= tol * np.abs(want[key]).max(), key
    if f32:
        assert worst > 1e-9, 'fp32 mode produced fp64-accurate results: the fp32 kernels did not run'
    if row.shard == 'whole':
        ok = ~np.isnan(want['P'])                   # directions inside the unit circle
        assert ok.any() and not ok.all()
        assert np.array_equal(np.isnan(got['P']), ~ok)
        for key in ('a_theta', 'a_phi'):
            assert np.abs(got[key][ok] - want[key][ok]).max() <= tol * np.abs(want[key][ok]).max(), key
        assert np.abs(got['P'][ok] - want['P'][ok]).max() <= (4 * tol if f32 else 1e-11) * want['P'][ok].max()


RESIDENT_N, RESIDENT_M = 203, 130


@functools.lru_cache(maxsize=1)
def _resident_case():
    """a lens in a window 1.5 x its diameter wide, 203 x 203 samples, and the oracle's flow on it"""
    from oracle import farfield_oracle, nearfield_oracle
    lens = _synthetic_lens(17.5e-6, 0.35, WL, switch_deg=9.0)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    x = (np.arange(RESIDENT_N) - (RESIDENT_N - 1) / 2) * (1.5 * R / ((RESIDENT_N - 1) / 2))
    assert x[1] - x[0] < WL / 2
    u = np.linspace(-0.35, 0.3, RESIDENT_M)
    src = (0.4e-6, -0.3e-6, -lens['source_distance'], 'y')
    nf = nearfield_oracle.build_nearfield(*src, WL, lens['lens_periphery_summary'], lens['lens_center_summary'],
                                          lens['hexgridset'], x_pts=x, y_pts=x)
    want = farfield_oracle.farfield_direct(*nf[:4], x, x, WL, nf[7], u, u)
    return lens, x, u, src, nf, want


def test_the_resident_window_exercises_row_first():
    """what the resident case below is chosen for, checked on the oracle's near field (no kernel runs here): some
    32-row tile of the 4 x 203 stacked rows begins its reduction at a pair >= 64, past a re-seed point of the
    rotations; rows lie wholly outside the lens; a tile straddles two field planes"""
    _lens, _x, _u, _src, nf, _want = _resident_case()
    n, T = RESIDENT_N, (RESIDENT_N + 1) // 2
    lit = np.any([f != 0 for f in nf[:4]], axis=0)                       # [row][sample]
    pair_lit = lit[:, :T] | lit[:, ::-1][:, :T]                           # pair t = samples t and n - 1 - t
    first = np.where(pair_lit.any(axis=1), pair_lit.argmax(axis=1), T)    # row_first: T for a dark row
    assert (first == T).any() and (first < T).any()
    # a plane's 203 rows are no whole number of tiles: tiles straddle two planes (their rows there are dark ones), and
    # the tiles of the later planes take other rows of the window than those of the first
    assert n % 32 != 0 and (4 * n) % 32 != 0
    begins = [first[np.arange(m0, min(m0 + 32, 4 * n)) % n].min() // 32 * 32 for m0 in range(0, 4 * n, 32)]
    assert any(64 <= b < T for b in begins), begins
    assert len({b for b in begins if b < T}) > 1, begins


@pytest.mark.parametrize('precision', ['f64', 'f32'])
def test_resident_rows_start_at_row_first(ma, ctx, precision):
    """HotPath(method='gemm') on synthesised fields: the folded stage 1 starts each tile's reduction at the first
    pair that can be non-zero (FoldArgs row_first).  Against the oracle's flow, and against the same fields
    downloaded and uploaded again, which carry no row_first and run every pair: equal up to the rotation chains'
    different starting seeds"""
    from metalens_amd.pipeline import HotPath
    lens, x, u, src, nf, want = _resident_case()
    f32 = precision == 'f32'
    tol = TOL_F32 if f32 else TOL
    hp = HotPath(src, WL, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'],
                 x, x, u, u, ctx=ctx, method='gemm', precision=precision)
    hp.step()
    hp.sync()
    got = hp.results()
    assert ctx.plan_kernels() == ('folded', 'folded')
    worst = _worst(got, want)
    print('gemm-resident %s: worst rel err %.3e' % (precision, worst))
    _record('gemm_resident', precision=precision, err=worst)
    for key in VECTORS + ('a_theta', 'a_phi'):
        assert np.abs(got[key] - want[key]).max() <= tol * np.abs(want[key]).max(), key
    if f32:
        assert worst > 1e-9, 'fp32 mode produced fp64-accurate results: the fp32 kernels did not run'
    F = ma.build_nearfield(source_x=src[0], source_y=src[1], source_z=src[2], source_pol=src[3], wavelength=WL,
                           lens_periphery_summary=lens['lens_periphery_summary'],
                           lens_center_summary=lens['lens_center_summary'], hexgridset=lens['hexgridset'],
                           x_pts=x, y_pts=x, ctx=ctx)
    ctx.set_method('gemm')
    again = ma.farfield_direct(*F[:4], x, x, WL, F[7], u, u, ctx=ctx, precision=precision)
    assert ctx.plan_kernels() == ('folded', 'folded')
    diff = _worst(got, again)
    print('gemm-resident %s: resident against uploaded %.3e' % (precision, diff))
    for key in VECTORS:
        # (fp32: two evaluations in fp32 differ by what each one's rounding allows)
        assert np.abs(got[key] - again[key]).max() <= (TOL_F32 if f32 else 1e-13) * np.abs(again[key]).max(), key
