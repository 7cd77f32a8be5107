"""The method 'fft-mixed' (csrc/zfft.hip zfft_mixed_kernel): an axis whose direction grid sits on a lattice of
N = 2^a 3^b 5^c samples that is not a multiple of 256 long - what the reference's good_fft_number hands out when the
caller passes no grid (nearfield.py:30-36, 95-102) - runs as an output-pruned FFT on that lattice itself, factored
A x B x R, instead of on the 256 / gcd(N, 256) times finer one.  Checked against the CPU oracle's direct sum and its
restatement of the reference flow, against 'fft-streamed' where no factorisation exists, and for the state the API
objects keep.  The table of tests/mixed_cases.py takes every leg pair through its three roles (stage 1, stage 2
streaming and strided: the 16 instantiations of the kernel), the twice finer lattice, R = 1 ... 32 and lattices
below 256 samples; test_zfft_mixed_emul.py ties the table to the production chooser.  Needs an MI355X."""
import numpy as np
import pytest

import mixed_cases
from test_gpu_fft import N_GLASS, TOL, WL, fields, lattice

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-4   # the fp32 GEMM mode's tolerance (test_gpu_parity.py)


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


@pytest.fixture
def ctx():
    from metalens_amd import _lib
    c = _lib.default_context()
    c.set_method('fft-mixed')
    c.set_precision('f64')
    yield c
    c.set_method('auto')


def _upload(ctx, F):
    from metalens_amd import _lib
    _lib.check(ctx.lib.ml_fields_upload(ctx.handle, F[0].shape[0], F[0].shape[1], *[_lib.dptr(a) for a in F]))


def _axes(nx, ny):
    x = (np.arange(nx) - 3.3) * (WL / 2.2)
    y = (np.arange(ny) + 11.1) * (WL / 2.3)
    return x, y


def _check_against_oracle(got, want):
    for key in ('Nx', 'Ny', 'Lx', 'Ly'):
        assert np.abs(got[key] - want[key]).max() <= TOL * np.abs(want[key]).max(), key
    ok = ~np.isnan(want['P'])                 # directions inside the unit circle
    assert np.array_equal(np.isnan(got['P']), ~ok)
    if ok.any():
        for key in ('a_theta', 'a_phi'):
            assert np.abs(got[key][ok] - want[key][ok]).max() <= TOL * np.abs(want[key][ok]).max(), key
        assert np.abs(got['P'][ok] - want['P'][ok]).max() <= 1e-11 * want['P'][ok].max()


@pytest.mark.parametrize('nx,ny,nex,ney,mx,my,jx,jy,kernels', [
    # both axes mixed: 400 = 10 x 10 x 4, 3600 = 16 x 15 x 15; 1000 = 10 x 10 x 10, 1440 = 16 x 15 x 6
    (400, 3600, 400, 3600, 400, 512, -200, -256, ('fft-mixed', 'fft-mixed')),
    (1000, 1440, 1000, 1440, 256, 1440, -128, -720, ('fft-mixed', 'fft-mixed')),
    # mixed x a multiple of 256 (stage 1 = y, stage 2 = x)
    (2000, 1024, 2000, 1024, 64, 256, -30, -128, ('fft', 'fft-mixed')),
    (512, 3000, 512, 3000, 100, 300, -50, -150, ('fft-mixed', 'fft')),
    # an aperture shorter than its lattice (90 rows on 3600), and a window that does not contain bin 0
    (90, 1000, 3600, 1000, 128, 100, -64, 50, ('fft-mixed', 'fft-mixed')),
    # a zero-padded axis on a mixed lattice, windows far off axis and wrapping around the lattice's end
    (700, 1100, 729, 1200, 60, 90, 700, -1190, ('fft-mixed', 'fft-mixed')),
    # 1920 = 128 x 15 (padded 2-fold by the 256 scheme): 16 x 15 x 8 here; 2400 = 16 x 15 x 10
    (2400, 1920, 2400, 1920, 48, 240, -24, -120, ('fft-mixed', 'fft-mixed')),
])
def test_mixed_lattices_match_the_oracle(ma, ctx, nx, ny, nex, ney, mx, my, jx, jy, kernels):
    from oracle import farfield_oracle
    x, y = _axes(nx, ny)
    ux, uy = lattice(nex, x[1] - x[0], mx, jx), lattice(ney, y[1] - y[0], my, jy)
    F = fields(nx, ny, nx + ny)
    got = ma.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy, ctx=ctx)
    assert ctx.plan_kernels() == kernels
    _check_against_oracle(got, farfield_oracle.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy))


def _worst(got, want):
    """largest error of the radiation vectors relative to each one's largest component (what TOL bounds)"""
    return max(np.abs(got[key] - want[key]).max() / np.abs(want[key]).max() for key in ('Nx', 'Ny', 'Lx', 'Ly'))


@pytest.mark.parametrize('xr,yr', mixed_cases.GPU_CASES, ids=['%s-%s' % (a, b or 'off') for a, b in mixed_cases.GPU_CASES])
def test_every_pair_in_every_role_matches_the_oracle(ma, ctx, xr, yr):
    """one table row per axis: the x row is stage 2 - streaming over a transposed stage-1 result where y is an FFT
    axis, strided over a row-major one where uy sits on no lattice -, the y row stage 1"""
    from oracle import farfield_oracle
    X, Y = mixed_cases.ROWS[xr], mixed_cases.ROWS[yr] if yr else None
    nx, ny = X.n_samples, Y.n_samples if Y else mixed_cases.OFF_NY
    x, y = _axes(nx, ny)
    ux = lattice(X.n_lattice, x[1] - x[0], X.m_bins, X.j0)
    uy = lattice(Y.n_lattice, y[1] - y[0], Y.m_bins, Y.j0) if Y else np.linspace(-0.2, 0.22, mixed_cases.OFF_MY)
    F = fields(nx, ny, nx + ny)
    got = ma.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy, ctx=ctx)
    assert ctx.plan_kernels() == ('fft-mixed' if Y else 'folded', 'fft-mixed')
    want = farfield_oracle.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy)
    print('mixed-case x %s %s y %s %s: worst rel err %.3e' % (xr, X.expect, yr, Y.expect if Y else None,
                                                             _worst(got, want)))
    _check_against_oracle(got, want)


def test_one_axis_mixed_the_other_off_the_lattice(ma, ctx):
    """each axis decides for itself: the mixed-radix FFT where the grid sits on such a lattice, the folded GEMM
    on a uniform grid that sits on none"""
    from oracle import farfield_oracle
    nx, ny, mx, my = 3000, 1000, 50, 60
    x, y = _axes(nx, ny)
    F = fields(nx, ny, 5)
    on_x, on_y = lattice(nx, x[1] - x[0], mx, -25), lattice(ny, y[1] - y[0], my, -30)
    off_x, off_y = np.linspace(-0.3, 0.3, mx), np.linspace(-0.2, 0.22, my)
    for ux, uy, kernels in ((on_x, off_y, ('folded', 'fft-mixed')), (off_x, on_y, ('fft-mixed', 'folded'))):
        got = ma.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy, ctx=ctx)
        assert ctx.plan_kernels() == kernels
        _check_against_oracle(got, farfield_oracle.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy))


@pytest.mark.parametrize('nx,ny,mx,my,jx,jy', [
    (540, 320, 96, 64, -48, -32),     # 12 x 9 x 5 and 16 x 10 x 2
    (360, 450, 96, 64, -48, -32),     # 720 = 16 x 15 x 3: the twice finer lattice along x; 15 x 10 x 3
])
@pytest.mark.parametrize('mirrored', [False, True])
def test_sharded_rows_through_the_mixed_fft(ma, ctx, mirrored, nx, ny, mx, my, jx, jy):
    """test_gpu_fft.py test_sharded_rows_through_the_fft on mixed lattices: row shards (contiguous blocks or mirrored
    pairs: two resident runs a0 / h0 + a1 / h1 of stage 2) accumulate to the whole aperture - and to the oracle's
    sum: two runs of one kernel agreeing says nothing about the kernel"""
    from metalens_amd import _lib, dist
    from oracle import farfield_oracle
    x, y = _axes(nx, ny)
    ux, uy = lattice(nx, x[1] - x[0], mx, jx), lattice(ny, y[1] - y[0], my, jy)
    F = fields(nx, ny, 9)
    whole = ma.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy, ctx=ctx)
    t = ma.FarfieldTransform(nx, ny, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux, uy, ctx=ctx)
    assert ctx.plan_kernels() == ('fft-mixed', 'fft-mixed')
    world = 3
    for rank in range(world):
        if mirrored:
            q0, q1 = dist.mirrored_block(nx, world, rank, align=2)
            rows = dist.mirrored_rows(nx, q0, q1)
        else:
            q0, q1 = dist.row_block(nx, world, rank)
            rows = np.arange(q0, q1)
        part = [np.ascontiguousarray(f[rows]) for f in F]
        _lib.check(ctx.lib.ml_fields_upload(ctx.handle, len(rows), ny, *[_lib.dptr(a) for a in part]))
        t.transform(row0=q0, accumulate=rank > 0, mirrored=mirrored)
    got = t.radiation_vectors()
    assert ctx.plan_kernels() == ('fft-mixed', 'fft-mixed')
    want = farfield_oracle.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy)
    print('mixed-shards %d x %d mirrored %s: worst rel err %.3e (whole aperture %.3e)'
          % (nx, ny, mirrored, _worst(got, want), _worst(whole, want)))
    for key in ('Nx', 'Ny', 'Lx', 'Ly'):
        assert np.abs(got[key] - whole[key]).max() <= 1e-13 * np.abs(whole[key]).max(), key
        assert np.abs(got[key] - want[key]).max() <= TOL * np.abs(want[key]).max(), key
    _check_against_oracle(whole, want)


def _hot_path_lens(ma):
    import math
    from metalens_amd import layout, synthetic
    return synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design,
                               radius=0.14e-3, numerical_aperture=0.5, wavelength=WL,
                               switch_angle=12 * math.pi / 180, num_gratings=20, num_entries=12)


@pytest.mark.parametrize('n,m', [(1000, 100), (360, 90)])   # 10 x 10 x 10; 720 = 16 x 15 x 3 (the twice finer lattice)
def test_hot_path_mixed_equals_gemm_and_the_oracle(ma, ctx, n, m):
    """test_gpu_fft.py test_hot_path_fft_equals_gemm under 'fft-mixed': the resident pipeline (synthesis -> transform
    -> projection) agrees with the GEMM formulation and with the oracle's flow (its near field, its direct sum)"""
    from metalens_amd.pipeline import HotPath
    from oracle import farfield_oracle, nearfield_oracle
    lens = _hot_path_lens(ma)
    x = (np.arange(n) - (n - 1) / 2) * (WL / 2.2)
    u = lattice(n, x[1] - x[0], m, -(m // 2))
    src = (0.4e-6, -0.3e-6, -lens['source_distance'], 'y')
    out = {}
    for method in ('fft-mixed', 'gemm'):
        hp = HotPath(src, WL, lens['lens_periphery_summary'], lens['lens_center_summary'],
                     lens['hexgridset'], x, x, u, u, ctx=ctx, method=method)
        hp.step()
        hp.sync()
        out[method] = hp.results()
        assert ctx.plan_kernels() == (('fft-mixed', 'fft-mixed') if method == 'fft-mixed' else ('folded', 'folded'))
    for key in ('Nx', 'Ny', 'Lx', 'Ly', 'a_theta', 'a_phi', 'P'):
        a, b = out['fft-mixed'][key], out['gemm'][key]
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), key
    assert out['fft-mixed']['power_local_rows'] == out['gemm']['power_local_rows']
    nf = nearfield_oracle.build_nearfield(*src, WL, lens['lens_periphery_summary'], lens['lens_center_summary'],
                                          lens['hexgridset'], x_pts=x, y_pts=x)
    want = farfield_oracle.farfield_direct(*nf[:4], x, x, WL, nf[7], u, u)
    print('mixed-hot-path %d -> %d: worst rel err %.3e' % (n, m, _worst(out['fft-mixed'], want)))
    _check_against_oracle(out['fft-mixed'], want)


def test_source_sweep_mixed_incoherent_sum_vs_oracle(ma):
    """test_gpu_parity.py test_source_sweep_incoherent_sum_vs_oracle with SourceSweep(method='fft-mixed') on a grid
    of 150 samples (300 = 10 x 10 x 3, the twice finer lattice): a polarisation batch of three field sets in one
    pass (alpha_rb, in_rb of the kernel's rows), a single source, a batch of two and a position batch"""
    from metalens_amd import _lib, postprocess
    from oracle import farfield_oracle, nearfield_oracle
    from test_gpu_parity import _synthetic_lens
    wl = 580e-9
    lens = _synthetic_lens(18e-6, 0.35, wl, switch_deg=9.0)
    n, m = 150, 36
    x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
    assert x[-1] >= lens['lens_periphery_summary']['r_max_list'][-1]      # the window holds the lens
    f = lens['source_distance']
    sources = [(0.2e-6, 0.1e-6, -f, 'x'), (0.2e-6, 0.1e-6, -f, 'y'), (0.2e-6, 0.1e-6, -f, 'z'),
               (-1.0e-6, 0.5e-6, -1.05 * f, 'x'),
               (0.0, 0.0, -0.97 * f, 'y'), (0.0, 0.0, -0.97 * f, 'z'),
               (0.5e-6, 0.0, -f, 'x'), (-0.5e-6, 0.3e-6, -1.02 * f, 'y')]
    weights = np.array([1.0, 1.0, 1.0, 0.5, 2.0, 2.0, 1.5, 0.7])
    cone, center = 0.08, (0.01, -0.005)
    near = [nearfield_oracle.build_nearfield(sx, sy, sz, pol, wl, lens['lens_periphery_summary'],
                                             lens['lens_center_summary'], lens['hexgridset'], x_pts=x, y_pts=x)
            for sx, sy, sz, pol in sources]
    u = (np.arange(m) - m // 2) * ((wl / near[0][7]) / ((x[1] - x[0]) * n))
    du = u[1] - u[0]
    ctx = _lib.default_context()
    try:
        sw = ma.SourceSweep(wl, lens['lens_periphery_summary'], lens['lens_center_summary'],
                            lens['hexgridset'], x, x, u, u, method='fft-mixed')
        assert sw.n_glass == near[0][7]
        assert [len(g['members']) for g in sw._group(sources)] == [3, 1, 2, 2]
        got = sw.run(sources, weights=weights, cone=cone, cone_center=center, keep_each=True)
        assert ctx.plan_kernels() == ('fft-mixed', 'fft-mixed')
    finally:
        ctx.set_method('auto')
    P_ref, pin_ref = 0, []
    for k, nf in enumerate(near):
        ff = farfield_oracle.farfield_direct(*nf[:4], x, x, wl, nf[7], u, u)
        print('mixed-sweep source %d: P rel err %.3e' % (k, np.nanmax(np.abs(got['P_each'][k] - ff['P'])) / np.nanmax(ff['P'])))
        assert np.nanmax(np.abs(got['P_each'][k] - ff['P'])) <= 1e-11 * np.nanmax(ff['P'])
        P_ref = P_ref + weights[k] * ff['P']
        pin_ref.append(nf[6])
        want_total = postprocess.total_power(ff['P'], du, du)
        want_cone = postprocess.encircled_power(ff['P'], u, u, du, du, sin_max=cone, center=center)
        assert abs(got['total_P'][k] - want_total) <= 1e-11 * want_total, k
        assert abs(got['cone_P'][k] - want_cone) <= 1e-11 * want_total, k
        assert 0 < want_cone < want_total          # the cone really cuts the map
    assert np.nanmax(np.abs(got['P_sum'] - P_ref)) <= 1e-11 * np.nanmax(P_ref)
    np.testing.assert_allclose(got['power_in'], pin_ref, rtol=1e-12)
    assert abs(got['efficiency'] - got['total_P'].sum() / np.sum(pin_ref)) < 1e-12


@pytest.mark.parametrize('N', [400, 1000, 1440, 2000, 288, 320, 360, 750, 900, 1080])
def test_whole_default_grids_vs_oracle_flow(N):
    """the reference flow on the grids it picks itself: a lens window of N x N samples synthesised resident, every
    lattice direction against the oracle's restatement of the flow (numpy.fft on the host) - ALL N^2 directions with
    the NaN mask.  The rows outside the lens circle are neither read (row_first) nor transformed (the launch
    trimming), on the mixed-radix kernel as on the others"""
    import metalens_amd as ma
    from metalens_amd import _lib
    from oracle import farfield_oracle
    from test_gpu_parity import _synthetic_lens
    wl = 580e-9
    lens = _synthetic_lens(60e-6, 0.4, wl, switch_deg=9.0)
    x = (np.arange(N) - (N - 1) / 2) * (wl / 2.2)
    args = dict(source_x=0.2e-6, source_y=-0.1e-6, source_z=-lens['source_distance'], source_pol='y',
                wavelength=wl, lens_periphery_summary=lens['lens_periphery_summary'],
                lens_center_summary=lens['lens_center_summary'], hexgridset=lens['hexgridset'],
                x_pts=x, y_pts=x)
    ctx = _lib.default_context()
    F = ma.build_nearfield(ctx=ctx, **args)               # host copies for the oracle flow
    ma.build_nearfield(ctx=ctx, download=False, **args)   # and the resident set
    ctx.set_method('fft-mixed')
    try:
        P, total_P, ux, uy, dux, duy = ma.farfield_from_resident_nearfield(x, x, wl, F[7], ctx=ctx)
        assert ctx.plan_kernels() == ('fft-mixed', 'fft-mixed')
    finally:
        ctx.set_method('auto')
    ffts = [np.fft.fft2(np.fft.fftshift(f)) for f in F[:4]]
    want = farfield_oracle.farfield_from_nearfield(*ffts, x, x, wl, F[7])
    assert np.array_equal(np.isnan(P), np.isnan(want[0]))
    ok = ~np.isnan(P)
    assert np.abs(P[ok] - want[0][ok]).max() <= 1e-12 * np.nanmax(want[0])
    assert abs(total_P - want[1]) <= 1e-12 * abs(want[1])
    assert np.array_equal(ux, want[2]) and np.array_equal(uy, want[3])
    assert dux == want[4] and duy == want[5]


@pytest.mark.parametrize('nx,ny,mx,my', [
    (256, 4374, 40, 48),      # 4374 = 2 x 3^7: no A x B x R with R <= 32 (and no 256 R3 lattice either: the GEMMs)
    (1024, 1024, 256, 256),   # multiples of 256 are not the chooser's business
    (64, 6561, 24, 36),       # 3^8
])
def test_without_a_factorisation_it_is_fft_streamed(ma, ctx, nx, ny, mx, my):
    """bit for bit, with the same kernels"""
    x, y = _axes(nx, ny)
    ux, uy = lattice(nx, x[1] - x[0], mx, -(mx // 2)), lattice(ny, y[1] - y[0], my, -(my // 2))
    F = fields(nx, ny, nx + ny + 1)
    a = ma.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy, ctx=ctx)
    ka = ctx.plan_kernels()
    ctx.set_method('fft-streamed')
    b = ma.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy, ctx=ctx)
    assert ctx.plan_kernels() == ka and 'fft-mixed' not in ka
    for key in ('Nx', 'Ny', 'Lx', 'Ly', 'a_theta', 'a_phi', 'P'):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_a_transform_keeps_fft_mixed(ma, ctx):
    """a FarfieldTransform built under 'fft-mixed' keeps it after the context's method has changed and another object
    has planned; afterwards 'auto' on a 400^2 grid still takes the folded GEMMs"""
    nx, ny, mx, my = 400, 1000, 400, 128
    x, y = _axes(nx, ny)
    ux, uy = lattice(nx, x[1] - x[0], mx, -200), lattice(ny, y[1] - y[0], my, -64)
    F = fields(nx, ny, 9)
    want = ma.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy, ctx=ctx)
    assert ctx.plan_kernels() == ('fft-mixed', 'fft-mixed')
    tm = ma.FarfieldTransform(nx, ny, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux, uy, ctx=ctx)
    ctx.set_method('gemm')
    tg = ma.FarfieldTransform(nx, ny, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux, uy, ctx=ctx)
    ctx.set_method('auto')
    x4 = (np.arange(400) - 199.5) * (WL / 2.2)
    u4 = lattice(400, x4[1] - x4[0], 400, -200)
    ma.farfield_direct(*fields(400, 400, 2), x4, x4, WL, N_GLASS, u4, u4, ctx=ctx)   # another object plans
    assert ctx.plan_kernels() == ('folded', 'folded')
    for t, kernels in ((tm, ('fft-mixed', 'fft-mixed')), (tg, ('folded', 'folded')), (tm, ('fft-mixed', 'fft-mixed'))):
        _upload(ctx, F)
        t.transform()
        got = t.radiation_vectors()
        assert ctx.plan_kernels() == kernels
        for key in ('Nx', 'Ny', 'Lx', 'Ly'):
            if kernels[0] == 'fft-mixed':   # the same kernels on the same inputs: the same bits
                assert np.array_equal(got[key], want[key]), key
            else:                           # (another formulation of the sum: twice the tolerance against the oracle)
                assert np.abs(got[key] - want[key]).max() <= 2 * TOL * np.abs(want[key]).max(), key
    assert ctx.method == 'fft-mixed'     # (what the last transform left)
    ctx.set_method('auto')
    ma.farfield_direct(*fields(400, 400, 2), x4, x4, WL, N_GLASS, u4, u4, ctx=ctx)
    assert ctx.plan_kernels() == ('folded', 'folded')


def test_f32_keeps_the_gemms(ma, ctx):
    """precision='f32' is a request for the fp32 matrix-core GEMMs, under 'fft-mixed' as under the other methods"""
    from oracle import farfield_oracle
    nx, ny, mx, my = 400, 1000, 96, 128
    x, y = _axes(nx, ny)
    ux, uy = lattice(nx, x[1] - x[0], mx, -48), lattice(ny, y[1] - y[0], my, -64)
    F = fields(nx, ny, 11)
    got = ma.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy, ctx=ctx, precision='f32')
    assert ctx.plan_kernels() == ('folded', 'folded')
    want = farfield_oracle.farfield_direct(*F, x, y, WL, N_GLASS, ux, uy)
    for key in ('Nx', 'Ny', 'Lx', 'Ly', 'a_theta', 'a_phi'):
        assert np.abs(got[key] - want[key]).max() <= TOL_F32 * np.abs(want[key]).max(), key
    ok = ~np.isnan(want['P'])
    assert np.array_equal(np.isnan(got['P']), ~ok)
    assert np.abs(got['P'][ok] - want['P'][ok]).max() <= 4 * TOL_F32 * want['P'][ok].max()
