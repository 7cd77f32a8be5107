"""Parity of the HIP path (through the C ABI) with the golden fixtures produced by the
reference and with the CPU oracle.  Needs an MI355X: run with ``-m gpu``.

Tolerances (BASELINE.json north_star): complex fields and far-field amplitudes
|dE| / max|E| < 1e-12 in fp64.  Measured values are far below."""
import glob
import os

import numpy as np
import pytest

import golden_io

pytestmark = pytest.mark.gpu

TOL = 1e-12
# lens B: the three-order tables; lens C: the orders characterize() would record (eleven / seven per ring
# collection, three in the centre); lens D: a five-order and a three-order collection, one order in the centre
CASES = sorted(os.path.basename(p) for p in glob.glob(golden_io.golden_path('nearfield_[BCD]_*.npz')))


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


def case_args(case, **override):
    lens = golden_io.load_lens(golden_io.golden_path(str(case['lens'])))
    args = dict(source_x=float(case['source_x']), source_y=float(case['source_y']),
                source_z=float(case['source_z']), source_pol=str(case['source_pol']),
                wavelength=float(case['wavelength']), lens_periphery_summary=lens[0],
                lens_center_summary=lens[1], hexgridset=lens[2],
                x_pts=case['x_pts'], y_pts=case['y_pts'],
                dipole_moment=float(case['dipole_moment']), c0=float(case['c0']), Z0=float(case['Z0']))
    args.update(override)
    return args


def field_errors(got, want):
    """(max |d| / max|want| over samples whose support agrees, number of samples whose
    zero/non-zero support differs = discrete-decision flips)"""
    flips = int(np.count_nonzero((got == 0) != (want == 0)))
    scale = max(np.abs(want).max(), 1e-300)
    return np.abs(got - want).max() / scale, flips


@pytest.mark.parametrize('name', CASES)
def test_nearfield_golden_windows(ma, name):
    case = np.load(golden_io.golden_path(name))
    out = ma.build_nearfield(**case_args(case))
    for got, key in zip(out[:4], ('Ex', 'Ey', 'Hx', 'Hy')):
        err, flips = field_errors(got, case[key])
        assert flips == 0, (key, flips)
        assert err < TOL, (key, err)
    assert abs(out[6] - case['power']) <= 1e-12 * abs(case['power'])
    assert out[7] == case['n_glass']


def test_nearfield_default_grid_golden_and_oracle(ma):
    from oracle import nearfield_oracle
    case = np.load(golden_io.golden_path('nearfield_A_default_grid.npz'))
    args = case_args(case, x_pts=None, y_pts=None)
    out = ma.build_nearfield(**args)
    assert np.array_equal(out[4], case['x_pts']) and np.array_equal(out[5], case['y_pts'])
    s = int(case['stride'])
    sl = (slice(s // 2, None, s), slice(s // 3, None, s))
    for i, key in enumerate(('Ex', 'Ey', 'Hx', 'Hy')):
        assert np.abs(out[i][sl] - case[key]).max() / case['norms'][i] < TOL, key
        assert (out[i] != 0).sum() == case['nonzero'][i]
    assert abs(out[6] - case['power']) <= 1e-12 * abs(case['power'])
    decisions = {}
    want = nearfield_oracle.build_nearfield(decisions=decisions, **args)
    for i in range(4):
        err, flips = field_errors(out[i], want[i])
        assert flips == 0 and err < TOL


def test_big_equals_single(ma):
    case = np.load(golden_io.golden_path('nearfield_B_straddle_offaxis_y.npz'))
    args = case_args(case)
    one = ma.build_nearfield(**args)
    args.pop('dipole_moment')
    big = ma.build_nearfield_big(pts_at_a_time=48 * 7, **args)
    for a, b in zip(one[:4], big[:4]):
        assert np.array_equal(a, b)       # strips are independent: bit-identical
    assert abs(one[6] - big[6]) <= 1e-14 * abs(one[6])


def test_prepared_lens_equals_plain_calls(ma):
    """ma.PreparedLens in place of the periphery summary (hashed and uploaded once): bit-identical
    results, for several sources, with another lens using the context in between, and through the
    strip driver"""
    a = np.load(golden_io.golden_path('nearfield_B_straddle_offaxis_y.npz'))
    b = np.load(golden_io.golden_path('nearfield_A_default_grid.npz'))
    args = case_args(a)
    lens = ma.PreparedLens(args['lens_periphery_summary'], args['lens_center_summary'], args['hexgridset'],
                           args['wavelength'])
    pargs = dict(args, lens_periphery_summary=lens, lens_center_summary=None, hexgridset=None)
    for pol, sx in (('x', 0.0), ('y', 3e-6), ('z', -2e-6)):
        plain = ma.build_nearfield(**dict(args, source_pol=pol, source_x=sx))
        other = ma.build_nearfield(**case_args(b))          # another lens takes the context
        assert other[0].shape == (b['x_pts'].size, b['y_pts'].size)
        got = ma.build_nearfield(**dict(pargs, source_pol=pol, source_x=sx))
        for u, v in zip(plain[:4], got[:4]):
            assert np.array_equal(u, v)
        assert plain[6] == got[6] and plain[7] == got[7]
    pargs.pop('dipole_moment')
    big = ma.build_nearfield_big(pts_at_a_time=48 * 7, **dict(pargs, source_pol='z', source_x=-2e-6))
    for u, v in zip(plain[:4], big[:4]):
        assert np.array_equal(u, v)


def test_empty_window_shortcut(ma):
    case = np.load(golden_io.golden_path('nearfield_B_edge_onaxis_x.npz'))
    far = case['x_pts'] + 400e-6
    out = ma.build_nearfield(**case_args(case, x_pts=far))
    assert all(not o.any() for o in out[:4]) and out[6] == 0 and isinstance(out[6], int)


def test_negative_cases(ma):
    neg = np.load(golden_io.golden_path('negative_cases.npz'))
    base = np.load(golden_io.golden_path('nearfield_B_periphery_onaxis_x.npz'))
    center = np.load(golden_io.golden_path('nearfield_B_center_onaxis_x.npz'))
    um = 1e-6
    wx = base['x_pts']
    overrides = {
        'coarse_pitch': dict(x_pts=wx[::2]),
        'nonuniform': dict(x_pts=np.hstack((wx[:-1], wx[-1] + 1e-9))),
        'source_above': dict(source_z=1e-6),
        'bad_pol': dict(source_pol='s'),
        'plane_z': dict(source_z=-float('inf'), source_pol='z'),
        'ux_overrun': dict(source_x=-180 * um),
        'uy_overrun': dict(source_y=150 * um, source_x=100 * um),
        'plane_wave_overrun': dict(source_z=-float('inf')),
        'center_overrun': dict(source_x=-60 * um, source_z=-60 * um, x_pts=center['x_pts'],
                               y_pts=center['y_pts']),
    }
    for label, ov in overrides.items():
        exc = {'AssertionError': AssertionError, 'ValueError': ValueError}[str(neg[label + '_type'])]
        with pytest.raises(exc) as info:
            ma.build_nearfield(**case_args(base, **ov))
        if exc is ValueError:
            assert info.value.args[0] == str(neg[label + '_msg']), label
            np.testing.assert_allclose([float(v) for v in info.value.args[1:]],
                                       neg[label + '_vals'], rtol=1e-12, err_msg=label)
    from metalens_amd.grating import n_glass
    with pytest.raises(ValueError) as info:
        n_glass(532)
    assert info.value.args[0] == str(neg['bad_wavelength_msg'])


def test_farfield_lattice_golden(ma):
    z = np.load(golden_io.golden_path('farfield_B_periphery_window.npz'))
    nf = np.load(golden_io.golden_path(str(z['nearfield'])))
    P, total_P, ux, uy, dux, duy = ma.farfield_from_nearfield(
        z['fftEx'], z['fftEy'], z['fftHx'], z['fftHy'], nf['x_pts'], nf['y_pts'],
        float(z['wavelength']), float(z['n_glass']), Z0=float(z['Z0']))
    assert np.array_equal(np.isnan(P), np.isnan(z['P'])) and np.isnan(P).any()
    ok = ~np.isnan(P)
    assert np.abs(P[ok] - z['P'][ok]).max() <= 1e-13 * np.nanmax(z['P'])
    assert abs(total_P - z['total_P']) <= 1e-13 * abs(z['total_P'])
    assert np.array_equal(ux, z['ux']) and np.array_equal(uy, z['uy'])
    assert dux == z['dux'] and duy == z['duy']


def test_direct_transform_on_fft_lattice_golden(ma):
    """N, L from the GEMM-cast aperture sum == the reference's fft bin x dA
    (nearfield_farfield.py:135-138) on lattice directions"""
    z = np.load(golden_io.golden_path('farfield_B_periphery_window.npz'))
    nf = np.load(golden_io.golden_path(str(z['nearfield'])))
    wl, n = float(z['wavelength']), float(z['n_glass'])
    x, y = nf['x_pts'], nf['y_pts']
    ux = ma.fft_direction_cosines(len(x), x[1] - x[0], wl, n)
    uy = ma.fft_direction_cosines(len(y), y[1] - y[0], wl, n)
    out = ma.farfield_direct(nf['Ex'], nf['Ey'], nf['Hx'], nf['Hy'], x, y, wl, n, ux, uy,
                             Z0=float(z['Z0']))
    for key in ('Nx', 'Ny', 'Lx', 'Ly'):
        assert np.abs(out[key] - z[key]).max() <= TOL * np.abs(z[key]).max(), key
    # power on the lattice equals the reference's (un-shifted) P
    Pref = np.fft.ifftshift(z['P'])
    ok = ~np.isnan(Pref)
    assert np.array_equal(np.isnan(out['P']), ~ok)
    assert np.abs(out['P'][ok] - Pref[ok]).max() <= 1e-11 * np.nanmax(Pref)


@pytest.mark.parametrize('shape', [(48, 40, 37, 29), (130, 70, 65, 130), (64, 64, 64, 64),
                                   (17, 200, 5, 3), (33, 45, 12, 18), (21, 131, 7, 131),
                                   (40, 257, 9, 2), (45, 33, 18, 12), (131, 21, 131, 7)])
def test_direct_transform_vs_oracle_ragged(ma, shape):
    """off-lattice directions, sizes that are not multiples of any tile"""
    from oracle import farfield_oracle
    nx, ny, mx, my = shape
    rng = np.random.default_rng(nx * 1000 + ny)
    F = [rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny)) for _ in range(4)]
    wl, n = 580e-9, 1.459
    x = (np.arange(nx) - 3.3) * (wl / 2.2)
    y = (np.arange(ny) + 11.1) * (wl / 2.3)
    ux = np.linspace(-0.61, 0.55, mx)
    uy = np.linspace(-0.3, 0.72, my)
    got = ma.farfield_direct(*F, x, y, wl, n, ux, uy)
    want = farfield_oracle.farfield_direct(*F, x, y, wl, n, ux, uy)
    for key in ('Nx', 'Ny', 'Lx', 'Ly', 'a_theta', 'a_phi'):
        assert np.abs(got[key] - want[key]).max() <= TOL * np.abs(want[key]).max(), key
    ok = ~np.isnan(want['P'])
    assert np.array_equal(np.isnan(got['P']), ~ok)
    assert np.abs(got['P'][ok] - want['P'][ok]).max() <= 1e-11 * want['P'][ok].max()


@pytest.mark.parametrize('kind', ['symmetric_about_zero', 'random_unsorted', 'nearly_symmetric'])
def test_direct_transform_direction_grids(ma, kind):
    """the folded (even/odd) stage 1 is used for centre-symmetric uy grids and the generic
    GEMM otherwise; both must agree with the oracle"""
    from oracle import farfield_oracle
    rng = np.random.default_rng(5)
    nx, ny, mx, my = 40, 90, 11, 50
    F = [rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny)) for _ in range(4)]
    wl, n = 580e-9, 1.459
    x = np.arange(nx) * (wl / 2.2)
    y = np.arange(ny) * (wl / 2.2)
    ux = rng.uniform(-0.5, 0.5, mx)
    if kind == 'symmetric_about_zero':
        uy = np.linspace(-0.4, 0.4, my)
        uy = 0.5 * (uy - uy[::-1])                      # exactly antisymmetric: no modulation
    elif kind == 'random_unsorted':
        uy = rng.uniform(-0.6, 0.6, my)                 # generic path
    else:
        uy = np.linspace(-0.2, 0.5, my)
        uy[7] += 3e-9                                   # breaks the symmetry: generic path
    got = ma.farfield_direct(*F, x, y, wl, n, ux, uy)
    want = farfield_oracle.farfield_direct(*F, x, y, wl, n, ux, uy)
    for key in ('Nx', 'Ny', 'Lx', 'Ly', 'a_theta', 'a_phi'):
        assert np.abs(got[key] - want[key]).max() <= TOL * np.abs(want[key]).max(), key


def test_pair_list_vs_oracle(ma):
    from oracle import farfield_oracle
    rng = np.random.default_rng(7)
    nx, ny, D = 50, 66, 300
    F = [rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny)) for _ in range(4)]
    wl, n = 580e-9, 1.459
    x = np.arange(nx) * (wl / 2.2)
    y = np.arange(ny) * (wl / 2.2)
    th = rng.uniform(0, 1.2, D)
    ph = rng.uniform(0, 2 * np.pi, D)
    ux, uy = np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph)
    got = ma.farfield_direct(*F, x, y, wl, n, ux, uy, pair_list=True)
    want = farfield_oracle.radiation_vectors_pairs(*F, x, y, wl, n, ux, uy)
    for g, w, key in zip((got['Nx'], got['Ny'], got['Lx'], got['Ly']), want, 'NNLL'):
        assert g.shape == (D,)
        assert np.abs(g - w).max() <= TOL * np.abs(w).max(), key


def test_sharded_rows_sum_to_whole(ma):
    """linearity: transforming row blocks separately and accumulating equals the whole
    aperture (this is the multi-GPU decomposition, minus the all-reduce)"""
    from metalens_amd import _lib
    rng = np.random.default_rng(3)
    nx, ny, mx, my = 96, 80, 33, 47
    F = [rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny)) for _ in range(4)]
    wl, n = 580e-9, 1.459
    x = np.arange(nx) * (wl / 2.2)
    y = np.arange(ny) * (wl / 2.2)
    ux = np.linspace(-0.4, 0.4, mx)
    uy = np.linspace(-0.5, 0.3, my)
    whole = ma.farfield_direct(*F, x, y, wl, n, ux, uy)
    ctx = _lib.default_context()
    t = ma.FarfieldTransform(nx, ny, x[1] - x[0], y[1] - y[0], wl, n, ux, uy, ctx=ctx)
    first = True
    for r0, r1 in ((0, 31), (31, 64), (64, 96)):
        part = [np.ascontiguousarray(f[r0:r1]) for f in F]
        _lib.check(ctx.lib.ml_fields_upload(ctx.handle, r1 - r0, ny, *[_lib.dptr(a) for a in part]))
        t.transform(row0=r0, accumulate=not first)
        first = False
    got = t.radiation_vectors()
    for key in ('Nx', 'Ny', 'Lx', 'Ly'):
        assert np.abs(got[key] - whole[key]).max() <= 1e-13 * np.abs(whole[key]).max(), key


@pytest.mark.parametrize('nx,ny,mx,my', [(96, 80, 34, 47), (64, 50, 33, 20), (130, 66, 7, 64),
                                         (64, 2100, 520, 2100)])
def test_mirrored_shards_sum_to_whole(ma, nx, ny, mx, my):
    """the multi-GPU decomposition used by HotPath: each rank holds mirrored row pairs so that
    BOTH stages run folded; accumulating the shards must reproduce the unsharded transform and
    the oracle"""
    from metalens_amd import _lib, dist
    from oracle import farfield_oracle
    rng = np.random.default_rng(nx)
    F = [rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny)) for _ in range(4)]
    wl, n = 580e-9, 1.459
    x = np.arange(nx) * (wl / 2.2)
    y = np.arange(ny) * (wl / 2.2)
    ux = np.linspace(-0.45, 0.35, mx)
    uy = np.linspace(-0.5, 0.3, my)
    want = farfield_oracle.radiation_vectors(*F, x, y, wl, n, ux, uy)
    ctx = _lib.default_context()
    t = ma.FarfieldTransform(nx, ny, x[1] - x[0], y[1] - y[0], wl, n, ux, uy, ctx=ctx)
    world = 3
    for rank in range(world):
        q0, q1 = dist.mirrored_block(nx, world, rank, align=2)
        rows = dist.mirrored_rows(nx, q0, q1)
        part = [np.ascontiguousarray(f[rows]) for f in F]
        _lib.check(ctx.lib.ml_fields_upload(ctx.handle, len(rows), ny, *[_lib.dptr(a) for a in part]))
        t.transform(row0=q0, accumulate=rank > 0, mirrored=True)
    got = t.radiation_vectors()
    for key, w in zip(('Nx', 'Ny', 'Lx', 'Ly'), want):
        assert np.abs(got[key] - w).max() <= TOL * np.abs(w).max(), key


@pytest.mark.parametrize('N,world,block,M,diameter,na', [
    (512, 2, 8, 96, 0.2e-3, 0.4), (1024, 2, 8, 96, 0.2e-3, 0.4), (2048, 8, 8, 96, 0.2e-3, 0.4),
    (2048, 2, 8, 96, 0.2e-3, 0.4), (4096, 4, 8, 96, 0.2e-3, 0.4), (1536, 2, 8, 96, 0.2e-3, 0.4),
    (16384, 2, 8, 128, 0.2e-3, 0.4),    # 1024-sample short transforms (R3 = 4), eight per workgroup of 512 threads
    (4000, 8, 4, 96, 0.2e-3, 0.4),      # 4000 rows on the 4096-sample lattice: 125 of 128 samples per short transform
    (960, 4, 8, 96, 0.2e-3, 0.4),       # 960 rows on the 1024-sample lattice
    (8192, 8, 8, 512, 2e-3, 0.94),      # BASELINE configs[2] at size: the 2 mm NA 0.94 lens over 8 ranks
])
def test_interleaved_shards_sum_to_whole(ma, N, world, block, M, diameter, na):
    """Blocks of rows dealt round robin over the ranks (metalens_hip.h ml_farfield_interleave_block):
    every rank's shard through its own synthesis and its SHORT column pass on one GPU, the partial
    radiation vectors added up on the host = the whole aperture in one piece, and the incident power
    likewise.  The block is 8 rows - the synthesis' patch height - wherever the aperture divides;
    the short transforms then have 32 ... 1024 samples and run zero-stuffed below 256 (stuff 8, 4, 2)
    or with R3 = 3 (1536 rows) and 4 (16384 rows over 2 ranks)."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    from metalens_amd import _lib
    from metalens_amd.pipeline import HotPath
    wl = 580e-9
    # (directions = bins of the lattice of the next multiple of 256 samples, zero-padded when the
    # aperture has fewer rows)
    lens, x, u = bench.build_workload(N, M, diameter, na, wl, N / (-(-N // 256) * 256))
    src = (0.2e-6, -0.1e-6, -lens['source_distance'], 'y')
    args = (src, wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'],
            x, x, u, u)
    ctx = _lib.default_context()
    whole = HotPath(*args, ctx=ctx)
    whole.step()
    whole.sync()
    want = whole.results()
    assert ctx.plan_kernels() == ('fft', 'fft')
    total = {k: 0 for k in ('Nx', 'Ny', 'Lx', 'Ly')}
    power = 0.0
    for rank in range(world):
        part = HotPath(*args, ctx=ctx, rank=rank, world=world)
        assert part.interleave == block and part.sharding.startswith('interleaved')
        assert np.array_equal(part.rows[:block], block * rank + np.arange(block))
        part.step_local()
        part.sync()
        vec = [np.empty(part.shape, dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_farfield_download(ctx.handle, *[_lib.dptr(v) for v in vec]))
        for k, v in zip(('Nx', 'Ny', 'Lx', 'Ly'), vec):
            total[k] = total[k] + v
        pw = _lib.c_double(0)
        _lib.check(ctx.lib.ml_nearfield_result(ctx.handle, _lib.byref(pw), None, 0, None))
        power += pw.value * part.dxp * part.dyp
    for key in total:
        assert np.abs(total[key] - want[key]).max() <= 1e-13 * np.abs(want[key]).max(), key
    assert abs(power - want['power_local_rows']) <= 1e-12 * want['power_local_rows']
    # a plan that cannot be dealt this way says so, and 'auto' falls back to mirrored pairs
    off = HotPath(src, wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'],
                  x, x, 0.7 * u, u, ctx=ctx, rank=0, world=world)
    assert off.interleave == 0 and off.sharding.startswith('mirrored')
    with pytest.raises(ValueError):
        HotPath(src, wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'],
                x, x, 0.7 * u, u, ctx=ctx, rank=0, world=world, sharding='interleaved')


def _synthetic_lens(radius, na, wavelength, n_glass=0, switch_deg=12.0, **more):
    import math
    import metalens_amd as ma_
    from metalens_amd import layout, synthetic
    return synthetic.make_lens((ma_.Grating, ma_.GratingCollection, ma_.HexGridSet),
                               layout.make_design, radius=radius, numerical_aperture=na,
                               wavelength=wavelength, switch_angle=switch_deg * math.pi / 180,
                               n_glass=n_glass, num_gratings=20, num_entries=12,
                               design_kwargs={'wavelength': wavelength}, **more)


@pytest.mark.parametrize('pol', ['x', 'y'])
def test_paper_lens_na094_windows_vs_oracle(ma, pol):
    """BASELINE config 3's lens (2 mm diameter, NA 0.94, TE+TM = x and y dipoles run
    separately): ~1200 rings, outer collections at grazing angles.  Windows at the lens edge
    and at mid radius against the CPU oracle."""
    import math
    from oracle import nearfield_oracle
    wl = 580e-9
    lens = _synthetic_lens(1e-3, 0.94, wl)
    assert len(lens['lens_periphery_summary']['r_center_list']) > 1000
    pitch = wl / 2.2
    for cx, cy in ((0.99e-3 * math.cos(0.3), 0.99e-3 * math.sin(0.3)), (-0.5e-3, 0.35e-3)):
        x = cx + (np.arange(72) - 35.5) * pitch
        y = cy + (np.arange(56) - 27.5) * pitch
        args = dict(source_x=0.0, source_y=0.0, source_z=-lens['source_distance'], source_pol=pol,
                    wavelength=wl, lens_periphery_summary=lens['lens_periphery_summary'],
                    lens_center_summary=lens['lens_center_summary'][:64],
                    hexgridset=lens['hexgridset'], x_pts=x, y_pts=y)
        got = ma.build_nearfield(**args)
        want = nearfield_oracle.build_nearfield(**args)
        scale = max(np.abs(w).max() for w in want[:4])
        assert scale > 0
        for g, w in zip(got[:4], want[:4]):
            assert np.count_nonzero((g == 0) != (w == 0)) == 0
            assert np.abs(g - w).max() <= TOL * scale
        assert abs(got[6] - want[6]) <= 1e-12 * abs(want[6])


def test_wavelength_sweep_keeps_every_wavelength_resident(ma):
    """sources x wavelengths on ONE GPU (BASELINE configs[3]'s three colours):
    ``WavelengthSweep`` holds a context per wavelength - tables, layout, geometry records and plan of
    450, 532 and 635 nm resident side by side - and gives, per wavelength, what a ``SourceSweep`` of
    that wavelength alone gives; a second run uploads nothing"""
    from metalens_amd import _lib
    members, alone = [], []
    sources = None
    for wl_nm, n_glass in ((450, 0), (532, 1.4607), (635, 1.457)):
        wl = wl_nm * 1e-9
        lens = _synthetic_lens(30e-6, 0.4, wl, n_glass=n_glass, switch_deg=9.0)
        n = ma.good_fft_number(2 * 31e-6 / (wl / 2.2))
        x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
        u = np.linspace(-0.12, 0.12, 40)
        members.append(dict(wavelength=wl, lens_periphery_summary=lens['lens_periphery_summary'],
                            lens_center_summary=lens['lens_center_summary'], hexgridset=lens['hexgridset'],
                            x_pts=x, y_pts=x, ux=u, uy=u))
        # (one emitter for all colours: at the shortest focal distance of the three lenses)
        f = lens['source_distance']
        sources = sources or [(0.0, 0.0, -f, 'x'), (0.0, 0.0, -f, 'y'), (0.0, 0.0, -f, 'z'), (1e-6, 0.0, -f, 'x')]
    for m in members:
        alone.append(ma.SourceSweep(ctx=_lib.default_context(), **m).run(sources, cone=0.05))
    ws = ma.WavelengthSweep(members)
    got = ws.run(sources, cone=0.05, spectrum=(0.2, 0.5, 0.3))
    tokens = [(c.tables_token, c.layout_token) for c in ws.contexts]
    assert len({id(c) for c in ws.contexts}) == 3 and all(t[0] is not None for t in tokens)
    for a, g in zip(alone, got['per_wavelength']):
        for key in ('P_sum', 'power_in', 'total_P', 'cone_P'):
            assert np.array_equal(a[key], g[key], equal_nan=True), key
    want_eff = (sum(w * a['total_P'].sum() for w, a in zip((0.2, 0.5, 0.3), alone))
                / sum(w * a['power_in'].sum() for w, a in zip((0.2, 0.5, 0.3), alone)))
    assert abs(got['efficiency'] - want_eff) <= 1e-15 * want_eff
    assert np.array_equal(got['P_sum'], sum(w * a['P_sum'] for w, a in zip((0.2, 0.5, 0.3), alone)), equal_nan=True)
    again = ws.run(sources, cone=0.05, spectrum=(0.2, 0.5, 0.3))
    assert [(c.tables_token, c.layout_token) for c in ws.contexts] == tokens     # nothing was uploaded again
    assert np.array_equal(again['P_sum'], got['P_sum'], equal_nan=True)
    ws.close()


@pytest.mark.parametrize('wl_nm,n_glass', [(450, 0), (532, 1.4607), (635, 1.457)])
def test_rgb_wavelengths_vs_oracle(ma, wl_nm, n_glass):
    """BASELINE config 4 (450 / 532 / 635 nm): 532 and 635 nm are not in the reference's glass
    table (grating.py:1277-1288), so those lenses carry an explicit n_glass"""
    from oracle import farfield_oracle, nearfield_oracle
    wl = wl_nm * 1e-9
    lens = _synthetic_lens(30e-6, 0.4, wl, n_glass=n_glass, switch_deg=9.0)
    args = dict(source_x=1e-6, source_y=-0.5e-6, source_z=-lens['source_distance'], source_pol='y',
                wavelength=wl, lens_periphery_summary=lens['lens_periphery_summary'],
                lens_center_summary=lens['lens_center_summary'], hexgridset=lens['hexgridset'])
    got = ma.build_nearfield(**args)
    want = nearfield_oracle.build_nearfield(**args)
    assert got[7] == want[7] == (n_glass or {450: 1.466}[wl_nm])
    scale = max(np.abs(w).max() for w in want[:4])
    for g, w in zip(got[:4], want[:4]):
        assert np.abs(g - w).max() <= TOL * scale
    u = np.linspace(-0.12, 0.12, 40)
    ff = ma.farfield_direct(None, None, None, None, got[4], got[5], wl, got[7], u, u)
    ref = farfield_oracle.farfield_direct(*want[:4], want[4], want[5], wl, want[7], u, u)
    for k in ('a_theta', 'a_phi'):
        assert np.abs(ff[k] - ref[k]).max() <= TOL * np.abs(ref[k]).max()


def test_source_sweep_incoherent_sum_vs_oracle(ma):
    """x + y + z dipoles summed incoherently (the reference's isotropic-emitter recipe,
    nearfield.py:69-73).  Sources at one position are ONE synthesis pass (a polarisation batch
    of 3, then a single, then a batch of 2), two single sources at different positions travel as
    one POSITION batch; P_sum, every total_P and the encircled power are
    accumulated on the GPU and must equal the oracle's maps reduced on the host
    (metalens_amd/postprocess.py, itself pinned on the reference's total_P)."""
    from metalens_amd import postprocess
    from oracle import farfield_oracle, nearfield_oracle
    wl = 580e-9
    lens = _synthetic_lens(18e-6, 0.35, wl, switch_deg=9.0)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    x = np.linspace(-R, R, 150)
    u = np.linspace(-0.2, 0.2, 36)
    du = u[1] - u[0]
    f = lens['source_distance']
    sources = [(0.2e-6, 0.1e-6, -f, 'x'), (0.2e-6, 0.1e-6, -f, 'y'), (0.2e-6, 0.1e-6, -f, 'z'),
               (-1.0e-6, 0.5e-6, -1.05 * f, 'x'),
               (0.0, 0.0, -0.97 * f, 'y'), (0.0, 0.0, -0.97 * f, 'z'),
               (0.5e-6, 0.0, -f, 'x'), (-0.5e-6, 0.3e-6, -1.02 * f, 'y')]   # two positions: one POSITION batch
    weights = np.array([1.0, 1.0, 1.0, 0.5, 2.0, 2.0, 1.5, 0.7])
    cone, center = 0.08, (0.01, -0.005)
    sw = ma.SourceSweep(wl, lens['lens_periphery_summary'], lens['lens_center_summary'],
                        lens['hexgridset'], x, x, u, u)
    groups = sw._group(sources)
    assert [len(g['members']) for g in groups] == [3, 1, 2, 2] and groups[3].get('mixed')
    got = sw.run(sources, weights=weights, cone=cone, cone_center=center, keep_each=True)
    P_ref, pin_ref = 0, []
    for k, (sx, sy, sz, pol) in enumerate(sources):
        nf = nearfield_oracle.build_nearfield(sx, sy, sz, pol, wl, lens['lens_periphery_summary'],
                                              lens['lens_center_summary'], lens['hexgridset'],
                                              x_pts=x, y_pts=x)
        ff = farfield_oracle.farfield_direct(*nf[:4], x, x, wl, nf[7], u, u)
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
    assert 0 < got['cone_efficiency'] < got['efficiency'] < 10


@pytest.mark.parametrize('mixed', [False, True])
def test_polarisation_batch_equals_single_sources(ma, mixed):
    """the batched synthesis (one pass, three resident field sets) against three single-source
    calls of the drop-in function, fields and incident power, dipoles and plane waves; ``mixed``: a lens whose
    ring collections are a narrow simple one, one with an order (0, 1) and a wide simple one - the batch
    instantiations (NP = 2, 3) of the order-list kernels AND of the general kernel in one pass"""
    import math
    from metalens_amd import _lib
    from metalens_amd.nearfield import nearfield_params
    wl = 580e-9
    more = {}
    if mixed:
        more = dict(periphery_orders=(((0, 0), (-1, 0), (1, 0)), ((0, 0), (-1, 0), (0, 1)),
                                      ((-2, 0), (-1, 0), (0, 0), (1, 0), (2, 0))),
                    max_collection_span=5 * math.pi / 180)
    lens = _synthetic_lens(40e-6, 0.4, wl, switch_deg=9.0, **more)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    r_c = float(lens['lens_periphery_summary']['r_min_list'][0])
    ctx = _lib.default_context()
    common = (wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'])
    for (sx, sy, sz), pols, x in (((0.3e-6, -0.2e-6, -lens['source_distance']), 'xyz', np.linspace(-R, R, 384)),
                                  ((0.0, 0.0, -float('inf')), 'xy', np.linspace(-0.6 * r_c, 0.6 * r_c, 160))):
        singles = [ma.build_nearfield(sx, sy, sz, pol, *common, x_pts=x, y_pts=x, ctx=ctx) for pol in pols]
        n = len(pols)
        params = (_lib.NearfieldParams * n)()
        for m, pol in enumerate(pols):
            params[m] = nearfield_params(sx, sy, sz, pol, wl, singles[0][7], 1e-30,
                                         ma.constants.c0, ma.constants.Z0)
        xs = _lib.f64(x)
        _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, n, _lib.dptr(xs), xs.size,
                                                    _lib.dptr(xs), xs.size))
        pw = np.zeros(n)
        _lib.check(ctx.lib.ml_nearfield_powers(ctx.handle, _lib.dptr(pw), n))
        for m in range(n):
            _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
            F = [np.empty((x.size, x.size), dtype=np.complex128) for _ in range(4)]
            _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
            scale = max(np.abs(w).max() for w in singles[m][:4])
            for g, w in zip(F, singles[m][:4]):
                assert np.abs(g - w).max() <= 1e-14 * scale
            assert abs(pw[m] * (x[1] - x[0]) ** 2 - singles[m][6]) <= 1e-13 * abs(singles[m][6])
        assert ctx.nearfield_kernels()['family'] == ('mixed' if mixed else 'orders-along-x')


def test_position_batch_equals_single_sources(ma):
    """f4(b): members of a batch at DIFFERENT source positions (and polarisations) are synthesised back
    to back into their field sets by the same kernels a single call runs: fields bit-identical to
    three drop-in calls, incident powers equal; wavelength / source kind must still agree"""
    from metalens_amd import _lib
    from metalens_amd.nearfield import nearfield_params
    wl = 580e-9
    lens = _synthetic_lens(40e-6, 0.4, wl, switch_deg=9.0)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    f = lens['source_distance']
    ctx = _lib.default_context()
    common = (wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'])
    x = np.linspace(-R, R, 384)
    srcs = [(0.3e-6, -0.2e-6, -f, 'x'), (-1.1e-6, 0.4e-6, -1.03 * f, 'z'), (0.0, 0.9e-6, -0.98 * f, 'y')]
    singles = [ma.build_nearfield(sx, sy, sz, pol, *common, x_pts=x, y_pts=x, ctx=ctx) for sx, sy, sz, pol in srcs]
    params = (_lib.NearfieldParams * 3)()
    for m, (sx, sy, sz, pol) in enumerate(srcs):
        params[m] = nearfield_params(sx, sy, sz, pol, wl, singles[0][7], 1e-30, ma.constants.c0, ma.constants.Z0)
    xs = _lib.f64(x)
    for rep in range(2):       # (the first pass into the three-set buffer also stores the zeros; the second runs from the lists)
        _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, 3, _lib.dptr(xs), xs.size, _lib.dptr(xs), xs.size))
        pw = np.zeros(3)
        _lib.check(ctx.lib.ml_nearfield_powers(ctx.handle, _lib.dptr(pw), 3))
        for m in range(3):
            _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
            F = [np.empty((x.size, x.size), dtype=np.complex128) for _ in range(4)]
            _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
            for g, w in zip(F, singles[m][:4]):
                assert np.array_equal(g, w), (rep, m)
            assert abs(pw[m] * (x[1] - x[0]) ** 2 - singles[m][6]) <= 1e-13 * abs(singles[m][6])
    # a plane wave and a dipole do not share a batch
    bad = (_lib.NearfieldParams * 2)()
    bad[0] = params[0]
    bad[1] = nearfield_params(0.0, 0.0, -float('inf'), 'x', wl, singles[0][7], 1e-30, ma.constants.c0, ma.constants.Z0)
    assert ctx.lib.ml_nearfield_batch_async(ctx.handle, bad, 2, _lib.dptr(xs), xs.size, _lib.dptr(xs), xs.size) != 0


def test_full_size_roundtrip_properties(ma):
    """BASELINE config[1] size (2048^2 -> 256^2): size-independent checks - the direct
    transform of a separable field equals the outer product of 1-D transforms, and is
    linear."""
    from oracle import farfield_oracle
    N, M = 2048, 256
    rng = np.random.default_rng(11)
    wl, n = 580e-9, 1.459
    x = (np.arange(N) - N / 2) * (wl / 2.2)
    fx = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    fy = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    F = np.outer(fx, fy)
    ux = np.linspace(-0.05, 0.05, M)
    uy = np.linspace(-0.04, 0.06, M)
    got = ma.farfield_direct(F, 2 * F, -F, 0.5 * F, x, x, wl, n, ux, uy)
    A = farfield_oracle.axis_twiddles(N, x[1] - x[0], ux, wl, n)
    B = farfield_oracle.axis_twiddles(N, x[1] - x[0], uy, wl, n)
    dA = (x[1] - x[0]) ** 2
    want = np.outer(A @ fx, B @ fy) * dA
    scale = np.abs(want).max()
    assert np.abs(got['Ly'] - (-want)).max() <= TOL * scale      # Ly = -F[Ex]
    assert np.abs(got['Lx'] - 2 * want).max() <= TOL * 2 * scale  # Lx = F[Ey]
    assert np.abs(got['Ny'] - (-want)).max() <= TOL * scale      # Ny = F[Hx]
    assert np.abs(got['Nx'] - (-0.5 * want)).max() <= TOL * scale  # Nx = -F[Hy]


# ---- fp32 GEMM mode (BASELINE.json: |dE|/|E| < 1e-4 for the fp32 path) ---------------------
TOL_F32 = 1e-4


@pytest.fixture
def f32_gemm():
    """switch the default context's far-field GEMMs to fp32 for one test"""
    from metalens_amd import _lib
    ctx = _lib.default_context()
    ctx.set_precision('f32')
    yield ctx
    ctx.set_precision('f64')


@pytest.mark.parametrize('shape', [(48, 40, 37, 29), (130, 70, 65, 130), (64, 64, 64, 64),
                                   (33, 45, 12, 18), (256, 512, 96, 200), (45, 33, 18, 12)])
def test_f32_gemm_vs_oracle(ma, f32_gemm, shape):
    """fp32 matrix-core GEMMs (both stages folded: uniform direction grids, whole aperture)
    against the fp64 oracle at the fp32 tolerance; the error must also be LARGER than fp64
    round-off, i.e. the fp32 kernels really ran"""
    from oracle import farfield_oracle
    nx, ny, mx, my = shape
    rng = np.random.default_rng(nx * 1000 + ny + 7)
    F = [rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny)) for _ in range(4)]
    wl, n = 580e-9, 1.459
    x = (np.arange(nx) - 3.3) * (wl / 2.2)
    y = (np.arange(ny) + 11.1) * (wl / 2.3)
    ux = np.linspace(-0.61, 0.55, mx)
    uy = np.linspace(-0.3, 0.72, my)
    got = ma.farfield_direct(*F, x, y, wl, n, ux, uy, precision='f32')
    want = farfield_oracle.farfield_direct(*F, x, y, wl, n, ux, uy)
    worst = 0.0
    for key in ('Nx', 'Ny', 'Lx', 'Ly', 'a_theta', 'a_phi'):
        err = np.abs(got[key] - want[key]).max() / np.abs(want[key]).max()
        assert err <= TOL_F32, (key, err)
        worst = max(worst, err)
    assert worst > 1e-9, 'fp32 mode produced fp64-accurate results: the fp32 kernels did not run'
    ok = ~np.isnan(want['P'])
    assert np.array_equal(np.isnan(got['P']), ~ok)
    assert np.abs(got['P'][ok] - want['P'][ok]).max() <= 4 * TOL_F32 * want['P'][ok].max()


def test_f32_mode_does_not_leak_into_the_drop_in_transform(ma):
    """HotPath(precision='f32') and a bare ``set_precision('f32')`` on the default context, then
    ``farfield_direct()`` / ``FarfieldTransform`` without a precision argument on the same
    context: they document 1e-12 and must deliver it (precision is set on every construction)"""
    from metalens_amd import _lib
    from metalens_amd.pipeline import HotPath
    from oracle import farfield_oracle
    ctx = _lib.default_context()
    wl, n = 580e-9, 1.459
    try:
        lens = _synthetic_lens(30e-6, 0.4, wl, switch_deg=9.0)
        R = lens['lens_periphery_summary']['r_max_list'][-1]
        xg = np.linspace(-R, R, 256)
        ug = np.linspace(-0.2, 0.2, 64)
        hp = HotPath((0.0, 0.0, -lens['source_distance'], 'x'), wl, lens['lens_periphery_summary'],
                     lens['lens_center_summary'], lens['hexgridset'], xg, xg, ug, ug, ctx=ctx,
                     precision='f32')
        hp.step()
        hp.sync()
        ctx.set_precision('f32')
        rng = np.random.default_rng(3)
        nx, ny = 96, 80
        F = [rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny)) for _ in range(4)]
        x = (np.arange(nx) - 3.3) * (wl / 2.2)
        y = (np.arange(ny) + 11.1) * (wl / 2.3)
        ux = np.linspace(-0.5, 0.5, 40)
        uy = np.linspace(-0.4, 0.4, 36)
        got = ma.farfield_direct(*F, x, y, wl, n, ux, uy)
        want = farfield_oracle.farfield_direct(*F, x, y, wl, n, ux, uy)
        for key in ('Nx', 'Ny', 'Lx', 'Ly', 'a_theta', 'a_phi'):
            assert np.abs(got[key] - want[key]).max() <= TOL * np.abs(want[key]).max(), key
    finally:
        ctx.set_precision('f64')


def test_f32_gemm_hot_path_vs_f64(ma, f32_gemm):
    """the GPU-resident pipeline on a synthetic lens: far-field amplitudes of the fp32-GEMM
    mode against the fp64 mode of the same kernels"""
    from metalens_amd.pipeline import HotPath
    wl = 580e-9
    lens = _synthetic_lens(40e-6, 0.4, wl, switch_deg=9.0)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    N = 384
    x = np.linspace(-R, R, N)
    u = np.linspace(-0.2, 0.2, 96)
    source = (0.3e-6, -0.2e-6, -lens['source_distance'], 'y')
    out = {}
    for prec in ('f32', 'f64'):
        hp = HotPath(source, wl, lens['lens_periphery_summary'], lens['lens_center_summary'],
                     lens['hexgridset'], x, x, u, u, ctx=f32_gemm, precision=prec)
        hp.step()
        hp.sync()
        out[prec] = hp.results()
    for key in ('a_theta', 'a_phi', 'Nx', 'Ly'):
        scale = np.abs(out['f64'][key]).max()
        err = np.abs(out['f32'][key] - out['f64'][key]).max() / scale
        assert 1e-10 < err <= TOL_F32, (key, err)


def test_full_size_nearfield_rows_and_determinism(ma):
    """BASELINE config[1] (2048^2 window of the 1 mm NA 0.5 lens): 24 aperture rows spread over
    the window against the CPU oracle, two runs bit-identical (fixed-order reductions, no float
    atomics), and the incident power equal to the oracle's on those rows' share."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    from metalens_amd import _lib
    from oracle import nearfield_oracle
    wl = 580e-9
    lens, x, u = bench.build_workload(2048, 256, 1e-3, 0.5, wl, 1.0)
    src = (0.0, 0.0, -lens['source_distance'], 'x')
    args = (src[0], src[1], src[2], src[3], wl, lens['lens_periphery_summary'],
            lens['lens_center_summary'], lens['hexgridset'])
    a = ma.build_nearfield(*args, x_pts=x, y_pts=x)
    b = ma.build_nearfield(*args, x_pts=x, y_pts=x)
    for p, q in zip(a[:4], b[:4]):
        assert np.array_equal(p, q)
    assert a[6] == b[6]
    for block in (slice(0, 4), slice(511, 515), slice(1020, 1028), slice(1533, 1537),
                  slice(2044, 2048)):                 # uniform pitch within each block
        want = nearfield_oracle.build_nearfield(*args, x_pts=x[block], y_pts=x)
        scale = max(np.abs(w).max() for w in want[:4]) or 1.0
        for g, w in zip(a[:4], want[:4]):
            assert np.abs(g[block] - w).max() <= TOL * scale
    # the incident power is a sum over samples: the GPU's value for the last block alone
    # (a separate call) equals the oracle's for that block
    c = ma.build_nearfield(*args, x_pts=x[1020:1028], y_pts=x)
    want = nearfield_oracle.build_nearfield(*args, x_pts=x[1020:1028], y_pts=x)
    assert abs(c[6] - want[6]) <= 1e-12 * abs(want[6])


def test_fused_input_modulation(ma):
    """ml_nearfield_premodulate: with a direction grid symmetric about u_c != 0 the synthesis
    kernel applies stage 1's input modulation; the far field must not change, the host must
    still get the plain near field, and a re-plan between synthesis and transform is refused"""
    from metalens_amd import _lib
    from metalens_amd.pipeline import HotPath
    from oracle import nearfield_oracle
    wl = 580e-9
    lens = _synthetic_lens(40e-6, 0.4, wl, switch_deg=9.0)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    u = (np.arange(96) - 48) * 0.004            # bins -48 .. 47: symmetric about -0.002
    r_c = float(lens['lens_periphery_summary']['r_min_list'][0])
    # a dipole over the whole lens; a plane wave over a window inside the centre disc (normal
    # incidence lies outside the periphery tables, as in the reference)
    for source, x in (((0.3e-6, -0.2e-6, -lens['source_distance'], 'y'), np.linspace(-R, R, 384)),
                      ((0.0, 0.0, -float('inf'), 'x'), np.linspace(-0.6 * r_c, 0.6 * r_c, 160))):
        args = (source, wl, lens['lens_periphery_summary'], lens['lens_center_summary'],
                lens['hexgridset'], x, x, u, u)
        out = {}
        for fuse in (False, True):
            hp = HotPath(*args, ctx=_lib.default_context(), fuse_modulation=fuse)
            hp.step()
            hp.sync()
            out[fuse] = hp.results()
        for key in ('a_theta', 'a_phi', 'Nx', 'Ly'):
            scale = np.abs(out[False][key]).max()
            assert np.abs(out[True][key] - out[False][key]).max() <= 1e-13 * scale, key
        # after the fused pass the resident fields are modulated; the download is not
        ctx = _lib.default_context()
        F = [np.empty((x.size, x.size), dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
        want = nearfield_oracle.build_nearfield(source[0], source[1], source[2], source[3], wl,
                                                lens['lens_periphery_summary'],
                                                lens['lens_center_summary'], lens['hexgridset'],
                                                x_pts=x, y_pts=x)
        scale = max(np.abs(w).max() for w in want[:4])
        for g, w in zip(F, want[:4]):
            assert np.abs(g - w).max() <= TOL * scale
    # stale plan: synthesise for one plan, re-plan for OTHER directions, transform -> refused;
    # re-planning the same geometry keeps the plan (and its modulation) and is accepted
    hp = HotPath(*args, ctx=_lib.default_context(), fuse_modulation=True)
    ctx, lib = hp.ctx, hp.ctx.lib
    _lib.check(lib.ml_nearfield_premodulate(ctx.handle, 1))
    u_other = _lib.f64(hp.uy + 0.001)

    def plan(uy):
        return lib.ml_farfield_plan(ctx.handle, x.size, x.size, hp.dxp, hp.dyp, wl, hp.n_glass,
                                    _lib.dptr(hp.ux), hp.ux.size, _lib.dptr(uy), uy.size, 0)

    def synthesise():
        _lib.check(lib.ml_nearfield_async(ctx.handle, _lib.byref(hp.params),
                                          _lib.dptr(hp.x_local), hp.x_local.size,
                                          _lib.dptr(hp.y), hp.y.size))

    _lib.check(plan(hp.uy))
    synthesise()
    _lib.check(plan(hp.uy))
    _lib.check(lib.ml_farfield_transform_async(ctx.handle, 0, 0))
    synthesise()
    _lib.check(plan(u_other))
    assert lib.ml_farfield_transform_async(ctx.handle, 0, 0) != 0
    _lib.check(lib.ml_nearfield_premodulate(ctx.handle, 0))
    ctx.sync()


@pytest.mark.parametrize('kind', ['holes', 'jitter', 'shuffled'])
def test_nearest_cell_on_irregular_cell_sets(ma, kind):
    """the lattice shortcut of the nearest-cell search must not change results: a lattice with
    10 % of its cells removed (empty nodes, shortcut still on), cells jittered off the lattice
    (fit refused -> bins search) and a shuffled cell order (ties go to the lowest ORIGINAL
    index) against the CPU oracle's exact nearest-neighbour search"""
    from oracle import nearfield_oracle
    wl = 580e-9
    lens = _synthetic_lens(40e-6, 0.4, wl, switch_deg=9.0)
    cells = np.array(lens['lens_center_summary'], dtype=float)
    rng = np.random.default_rng({'holes': 1, 'jitter': 2, 'shuffled': 3}[kind])
    if kind == 'holes':
        cells = cells[rng.random(len(cells)) > 0.1]
    elif kind == 'jitter':
        cells[:, :2] += rng.uniform(-0.05, 0.05, (len(cells), 2)) * 320e-9
    else:
        cells = cells[rng.permutation(len(cells))]
    r_c = float(lens['lens_periphery_summary']['r_min_list'][0])
    x = np.linspace(-1.05 * r_c, 1.05 * r_c, 200)     # the centre disc and a rim of periphery
    args = (0.2e-6, -0.1e-6, -lens['source_distance'], 'x', wl, lens['lens_periphery_summary'],
            cells, lens['hexgridset'])
    got = ma.build_nearfield(*args, x_pts=x, y_pts=x)
    decisions = {}
    want = nearfield_oracle.build_nearfield(*args, x_pts=x, y_pts=x, decisions=decisions)
    for g, w in zip(got[:4], want[:4]):
        err, flips = field_errors(g, w)
        assert flips == 0 and err < TOL


def test_zeros_outside_the_lens_survive_repeated_synthesis(ma):
    """Samples outside the lens are zero whatever the source; the synthesis stores them once per
    (buffer, grid, layout) and skips them afterwards.  Repeated calls, another source, and a
    buffer that somebody else has written in between (ml_fields_upload) must all still return
    exact zeros there and the oracle's field inside."""
    from metalens_amd import _lib
    from oracle import nearfield_oracle
    wl = 580e-9
    lens = _synthetic_lens(30e-6, 0.4, wl, switch_deg=9.0)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    x = np.linspace(-1.3 * R, 1.3 * R, 320)          # a window well beyond the lens
    common = (wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'])
    ctx = _lib.Context(0)
    try:
        outside = np.hypot(x[:, None], x[None, :]) > R
        assert outside.sum() > 0.3 * outside.size
        srcs = [(0.0, 0.0, -lens['source_distance'], 'x')] * 2 + [(0.4e-6, -0.3e-6, -0.98 * lens['source_distance'], 'y')]
        for k, src in enumerate(srcs + srcs[:1]):
            if k == 3:   # garbage into the resident buffer: the next synthesis must not trust it
                junk = [np.full((x.size, x.size), 7.0 + 1j, dtype=np.complex128) for _ in range(4)]
                _lib.check(ctx.lib.ml_fields_upload(ctx.handle, x.size, x.size, *[_lib.dptr(a) for a in junk]))
            got = ma.build_nearfield(*src, *common, x_pts=x, y_pts=x, ctx=ctx)
            want = nearfield_oracle.build_nearfield(*src, *common, x_pts=x, y_pts=x)
            for g, w in zip(got[:4], want[:4]):
                assert not g[outside].any()
                err, flips = field_errors(g, w)
                assert flips == 0 and err < TOL, (k, err, flips)
    finally:
        ctx.close()


@pytest.mark.parametrize('nx,ny,shift', [(8, 8, 0.0), (200, 136, 0.8), (1000, 1032, 0.0), (3, 2050, 0.0)])
def test_active_patch_list_matches_full_launch(ma, nx, ny, shift):
    """The first synthesis on a geometry visits every 8 x 8 patch; later ones launch only the
    patches that hold lens samples (a list compacted on the GPU from per-patch flags, in chunks
    of 1024 patches).  Both must give the same fields bit for bit and the same incident power:
    one patch, a window hanging over the lens edge, many chunks with a partial last one, a
    3-row strip."""
    from metalens_amd import _lib
    wl = 580e-9
    lens = _synthetic_lens(30e-6, 0.4, wl, switch_deg=9.0)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    pitch = wl / 2.2
    x = shift * R + (np.arange(nx) - (nx - 1) / 2) * min(pitch, 2.6 * R / max(nx, 2))
    y = (np.arange(ny) - (ny - 1) / 2) * min(pitch, 2.6 * R / max(ny, 2))
    common = (wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'])
    src = (0.2e-6, -0.1e-6, -lens['source_distance'], 'x')
    ctx = _lib.Context(0)
    try:
        first = ma.build_nearfield(*src, *common, x_pts=x, y_pts=y, ctx=ctx)
        for _ in range(2):
            again = ma.build_nearfield(*src, *common, x_pts=x, y_pts=y, ctx=ctx)
            for a, b in zip(first[:4], again[:4]):
                assert np.array_equal(a, b)
            assert first[6] == again[6]          # incident power: same per-patch partials
        assert any(f.any() for f in first[:4])
    finally:
        ctx.close()


def test_reordered_cells_on_one_context_are_a_new_layout(ma):
    """The resident layout is keyed by a content hash of every packed array.  The same cells in
    another ORDER are another layout - tie answers (cKDTree row indices) and the bin-sorted cell
    arrays both depend on the order - so the second call must upload again, and on an odd grid
    (exact ties on the mirror lines) every sample must still follow cKDTree on ITS cell array."""
    from metalens_amd import _lib
    from oracle import nearfield_oracle
    wl = 580e-9
    lens = _synthetic_lens(40e-6, 0.4, wl, switch_deg=9.0)
    cells = np.array(lens['lens_center_summary'], dtype=float)
    n = 61
    x = (np.arange(n) - n // 2) * (wl / 2.2)      # odd and symmetric: ties on the middle row / column
    ctx = _lib.Context(0)
    try:
        tokens = []
        for order in (np.arange(len(cells)), np.random.default_rng(11).permutation(len(cells))):
            args = (0.4e-6, -0.3e-6, -lens['source_distance'], 'y', wl,
                    lens['lens_periphery_summary'], cells[order], lens['hexgridset'])
            dec = {}
            want = nearfield_oracle.build_nearfield(*args, x_pts=x, y_pts=x, decisions=dec)
            assert np.count_nonzero(dec['nearest_tie']) > 0
            got = ma.build_nearfield(*args, x_pts=x, y_pts=x, ctx=ctx)
            tokens.append(ctx.layout_token)
            for g, w in zip(got[:4], want[:4]):
                err, flips = field_errors(g, w)
                assert flips == 0 and err < TOL
        assert tokens[0] != tokens[1]
    finally:
        ctx.close()


@pytest.mark.parametrize('u_steps', [5, 7, 11])
def test_nonuniform_table_axes(ma, u_steps):
    """characterisation tables whose (ux, uy) axes are NOT uniformly spaced take the select-chain
    (<= 5 nodes, <= 8 nodes) or the search-loop (> 8 nodes) cell location instead of the
    arithmetic one: near field of a whole small lens against the oracle"""
    import math
    import metalens_amd as ma_
    from metalens_amd import layout, synthetic
    from oracle import nearfield_oracle
    wl = 580e-9
    lens = synthetic.make_lens((ma_.Grating, ma_.GratingCollection, ma_.HexGridSet),
                               layout.make_design, radius=30e-6, numerical_aperture=0.4,
                               wavelength=wl, switch_angle=9 * math.pi / 180, num_gratings=16,
                               num_entries=10, design_kwargs={'wavelength': wl},
                               axis_warp=0.35, u_steps=u_steps)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    x = np.linspace(-R, R, 230)
    args = (0.4e-6, 0.3e-6, -lens['source_distance'], 'y', wl, lens['lens_periphery_summary'],
            lens['lens_center_summary'], lens['hexgridset'])
    got = ma.build_nearfield(*args, x_pts=x, y_pts=x)
    decisions = {}
    want = nearfield_oracle.build_nearfield(*args, x_pts=x, y_pts=x, decisions=decisions)
    for g, w in zip(got[:4], want[:4]):
        err, flips = field_errors(g, w)
        assert flips == 0 and err < TOL


@pytest.mark.parametrize('N,M', [(383, 95), (385, 96), (384, 97)])
def test_fused_input_modulation_odd_sizes(ma, N, M):
    """odd aperture / direction counts (unpaired centre sample, self-paired centre direction)
    through the GPU-resident pipeline with and without the fused input modulation"""
    from metalens_amd import _lib
    from metalens_amd.pipeline import HotPath
    wl = 580e-9
    lens = _synthetic_lens(40e-6, 0.4, wl, switch_deg=9.0)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    x = np.linspace(-R, R, N)
    u = (np.arange(M) - M // 2) * 0.004
    args = ((0.3e-6, -0.2e-6, -lens['source_distance'], 'y'), wl, lens['lens_periphery_summary'],
            lens['lens_center_summary'], lens['hexgridset'], x, x, u, u)
    out = {}
    for fuse in (False, True):
        hp = HotPath(*args, ctx=_lib.default_context(), fuse_modulation=fuse)
        hp.step()
        hp.sync()
        out[fuse] = hp.results()
    for key in ('a_theta', 'a_phi', 'Nx', 'Ly'):
        assert np.abs(out[True][key] - out[False][key]).max() <= 1e-13 * np.abs(out[False][key]).max()


def test_merged_launches_keep_per_call_semantics(ma):
    """The step's small launches are merged: the bound-violation keys are
    double-buffered and cleared by the synthesis kernel itself, the incident-power partials are
    summed by a spare block of the projection kernel (or on demand), the stage-2 unfold rides in
    the projection kernel, plan tables and row extents are kept while the geometry stands.  What
    a caller sees per call must not change."""
    from metalens_amd import _lib
    from metalens_amd.pipeline import HotPath
    from oracle import nearfield_oracle, farfield_oracle
    base = np.load(golden_io.golden_path('nearfield_B_periphery_onaxis_x.npz'))
    um = 1e-6
    # (1) violations belong to the call that produced them: bad, good, bad, bad, good
    good = ma.build_nearfield(**case_args(base))
    for bad in (True, False, True, True, False):
        if bad:
            with pytest.raises(ValueError):
                ma.build_nearfield(**case_args(base, source_x=-180 * um))
        else:
            out = ma.build_nearfield(**case_args(base))
            for g, w in zip(out[:4], good[:4]):
                assert np.array_equal(g, w)
            assert out[6] == good[6]
    # (2) the power summed inside the projection kernel == the power summed on demand, and the
    # fused unfold + projection == vectors downloaded first (plain unfold) then projected
    wl = 580e-9
    lens = _synthetic_lens(40e-6, 0.4, wl, switch_deg=9.0)
    R = lens['lens_periphery_summary']['r_max_list'][-1]
    x = np.linspace(-R, R, 384)
    source = (0.3e-6, -0.2e-6, -lens['source_distance'], 'x')
    for n_dir in (96, 464):
        u = (np.arange(n_dir) - n_dir // 2) * (0.384 / n_dir)
        args = (source, wl, lens['lens_periphery_summary'], lens['lens_center_summary'],
                lens['hexgridset'], x, x, u, u)
        hp = HotPath(*args, ctx=_lib.default_context())
        for _ in range(3):                      # repeated steps re-use plan tables and row extents
            hp.step()
        hp.sync()
        fused = hp.results()
        ctx, lib = hp.ctx, hp.ctx.lib
        hp.step_local()                         # near field + transform, nothing consumed yet
        power = _lib.c_double(0)
        n_viol = _lib.c_int(0)
        viol = (_lib.BoundViolation * 8)()
        _lib.check(lib.ml_nearfield_result(ctx.handle, _lib.byref(power), viol, 8, _lib.byref(n_viol)))
        assert n_viol.value == 0
        assert power.value * hp.dxp * hp.dyp == fused['power_local_rows']
        vec = [np.empty(hp.shape, dtype=np.complex128) for _ in range(4)]
        _lib.check(lib.ml_farfield_download(ctx.handle, *[_lib.dptr(v) for v in vec]))   # plain unfold
        P = np.empty(hp.shape)
        _lib.check(lib.ml_farfield_project(ctx.handle, hp.Z0, _lib.dptr(P), None, None))
        for v, key in zip(vec, ('Nx', 'Ny', 'Lx', 'Ly')):
            assert np.array_equal(v, fused[key]), key
        assert np.array_equal(P, fused['P'], equal_nan=True)
        # (3) and all of it against the oracle
        want = nearfield_oracle.build_nearfield(source[0], source[1], source[2], source[3], wl,
                                                lens['lens_periphery_summary'],
                                                lens['lens_center_summary'], lens['hexgridset'],
                                                x_pts=x, y_pts=x)
        assert abs(fused['power_local_rows'] - want[6]) <= 1e-12 * abs(want[6])
        N = farfield_oracle.radiation_vectors(want[0], want[1], want[2], want[3], x, x, wl,
                                                     want[7], u, u)
        for got, w in zip((fused['Nx'], fused['Ny'], fused['Lx'], fused['Ly']), N):
            assert np.abs(got - w).max() <= TOL * np.abs(w).max()
    # (4) a different grid on the same context: extents and tables must follow
    x2 = np.linspace(-0.8 * R, 0.9 * R, 300)
    hp2 = HotPath(source, wl, lens['lens_periphery_summary'], lens['lens_center_summary'],
                  lens['hexgridset'], x2, x2, u, u, ctx=_lib.default_context())
    hp2.step()
    hp2.sync()
    got2 = hp2.results()
    want2 = nearfield_oracle.build_nearfield(source[0], source[1], source[2], source[3], wl,
                                             lens['lens_periphery_summary'],
                                             lens['lens_center_summary'], lens['hexgridset'],
                                             x_pts=x2, y_pts=x2)
    N2 = farfield_oracle.radiation_vectors(want2[0], want2[1], want2[2], want2[3], x2, x2,
                                                  wl, want2[7], u, u)
    for got, w in zip((got2['Nx'], got2['Ny'], got2['Lx'], got2['Ly']), N2):
        assert np.abs(got - w).max() <= TOL * np.abs(w).max()
    assert abs(got2['power_local_rows'] - want2[6]) <= 1e-12 * abs(want2[6])


SIMPLE3 = ((0, 0), (-1, 0), (1, 0))
@pytest.mark.parametrize('per,cen,family', [
    (((0, 0), (-1, 0), (1, 0), (0, 1), (-2, 0)), SIMPLE3, 'mixed'),                 # general rings, simple centre
    (SIMPLE3, ((0, 0), (-1, 0), (1, 0), (0, -1), (1, 1)), 'mixed'),                 # simple rings, general centre
    (((0, 0), (-1, 1), (2, -1)), ((0, 0), (0, 1), (-1, -1), (2, 0)), 'general'),    # both general
    # per COLLECTION (cycled over the lens' ring collections): a narrow simple one, one with an order (0, 1) - the
    # general kernel's -, a wide simple one (five orders): every kernel of both families in one lens
    ((SIMPLE3, ((0, 0), (-1, 0), (0, 1)), ((-2, 0), (-1, 0), (0, 0), (1, 0), (2, 0))), SIMPLE3, 'mixed'),
    ((((0, 0), (-1, 0), (0, 1)), ((-2, 0), (-1, 0), (0, 0), (1, 0), (2, 0))), ((0, 0), (1, 1)), 'mixed'),   # no narrow collection, general centre
])
@pytest.mark.parametrize('pol,sz', [('x', -1.0), ('y', -float('inf'))])
def test_general_order_sets_vs_oracle(ma, per, cen, family, pol, sz):
    """Tables with an order oy != 0 (|o| <= 5 in general, grating.lua:406-423) take the GENERAL kernel, which
    evaluates every order's phase argument the reference's way (nearfield.py:268-269,291; :391-409) - PER TABLE:
    the samples of the other ring collections / the centre table of the same lens stay with the kernels that build
    the phasors by products ('mixed').  Windows in the centre, across the switch radius and in the periphery
    (patches with samples of two, three kernels), dipole and plane wave, against the oracle; twice per window, so
    that the full-grid first pass and the listed steady state are both compared."""
    from oracle import nearfield_oracle
    import math
    from metalens_amd import _lib, layout, synthetic
    wl = 580e-9
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design,
                               radius=40e-6, numerical_aperture=0.4, wavelength=wl,
                               switch_angle=9 * math.pi / 180, num_gratings=20, num_entries=12,
                               # (order lists per collection: three ring collections instead of two)
                               max_collection_span=(5 if isinstance(per[0][0], tuple) else 9) * math.pi / 180,
                               design_kwargs={'wavelength': wl}, periphery_orders=per, center_orders=cen)
    if isinstance(per[0][0], tuple):
        assert len(lens['lens_periphery_summary']['gratingcollection_list']) >= len(per)
    rsw = lens['r_for_switch']
    pitch = wl / 2.2
    windows = ((1e-6, -2e-6), (rsw * math.cos(0.7), rsw * math.sin(0.7)), (-30e-6, 12e-6))
    if sz == -float('inf'):
        windows = windows[:1]   # a normally incident plane wave is outside the rings' tables (as in the reference)
    for cx, cy in windows:
        x = cx + (np.arange(40) - 20) * pitch
        y = cy + (np.arange(56) - 28) * pitch
        args = dict(source_x=0.3e-6, source_y=-0.2e-6,
                    source_z=sz if sz == -float('inf') else -lens['source_distance'], source_pol=pol,
                    wavelength=wl, lens_periphery_summary=lens['lens_periphery_summary'],
                    lens_center_summary=lens['lens_center_summary'], hexgridset=lens['hexgridset'],
                    x_pts=x, y_pts=y)
        want = nearfield_oracle.build_nearfield(**args)
        scale = max(np.abs(w).max() for w in want[:4])
        assert scale > 0
        for attempt in range(2):   # (the first synthesis on a geometry runs over the whole grid, the second from the lists)
            got = ma.build_nearfield(**args)
            assert _lib.default_context().nearfield_kernels()['family'] == family
            for g, w in zip(got[:4], want[:4]):
                assert int(np.count_nonzero((g == 0) != (w == 0))) == 0
                assert np.abs(g - w).max() <= TOL * scale
            assert abs(got[6] - want[6]) <= 1e-12 * abs(want[6])


ORDER_LISTS = {
    # what characterize() would record for this lens (grating.lua:417-423): eleven orders in the inner
    # collection, seven in the outer, three in the centre, zero-filled where an order does not propagate
    'physical': ('physical', 'physical'),
    # the review's reading: {-3 ... +1} inside 30 degrees, {-2, -1, 0} outside, (0, 0) in the centre
    'inside-outside': ((((-3, 0), (-2, 0), (-1, 0), (0, 0), (1, 0)), ((-2, 0), (-1, 0), (0, 0))), ((0, 0),)),
    # lists with holes and one-sided lists: no (0, 0) at all; only positive orders; a lone high order
    'holes': ((((-1, 0), (2, 0), (-4, 0)), ((1, 0), (2, 0), (3, 0), (5, 0))), ((-1, 0), (1, 0))),
    'one-order': ((((-5, 0),), ((0, 0), (-1, 0), (1, 0), (-2, 0), (2, 0), (-3, 0), (3, 0), (-4, 0), (4, 0), (-5, 0), (5, 0))),
                  ((0, 0), (-2, 0), (2, 0), (-3, 0))),
}


@pytest.mark.parametrize('which', sorted(ORDER_LISTS))
@pytest.mark.parametrize('pol,sz', [('x', -1.0), ('z', -1.0), ('y', -float('inf'))])
def test_per_collection_order_lists_vs_oracle(ma, which, pol, sz):
    """Tables holding any orders (ox, 0) with |ox| <= 5, every collection its own list, take the
    product-phasor kernels (nearfield_simple.hip) - a collection of three orders runs three, its
    neighbour of eleven runs eleven.  Windows in the centre, across the switch radius, across the
    boundary between two collections of DIFFERENT lists (waves that hold lanes of both) and at the
    rim, dipoles and a plane wave, against the oracle."""
    from oracle import nearfield_oracle
    import math
    from metalens_amd import _lib, layout, synthetic
    wl = 580e-9
    per, cen = ORDER_LISTS[which]
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design,
                               radius=40e-6, numerical_aperture=0.4, wavelength=wl,
                               switch_angle=9 * math.pi / 180, num_gratings=20, num_entries=12,
                               design_kwargs={'wavelength': wl}, periphery_orders=per, center_orders=cen)
    assert len(lens['collections']) == 2
    S = lens['lens_periphery_summary']
    gc_of_ring = np.asarray(S['gratingcollection_index_here_list'])
    first_outer = int(np.argmax(gc_of_ring == 1))
    r_join = float(np.asarray(S['r_min_list'])[first_outer])   # where the second collection starts
    rsw = lens['r_for_switch']
    pitch = wl / 2.2
    windows = ((1e-6, -2e-6), (rsw * math.cos(0.7), rsw * math.sin(0.7)),
               (r_join * math.cos(2.1), r_join * math.sin(2.1)), (-36e-6, 14e-6))
    if sz == -float('inf'):
        windows = windows[:1]   # a normally incident plane wave is outside the rings' tables (as in the reference)
    for cx, cy in windows:
        x = cx + (np.arange(40) - 20) * pitch
        y = cy + (np.arange(56) - 28) * pitch
        args = dict(source_x=0.3e-6, source_y=-0.2e-6,
                    source_z=sz if sz == -float('inf') else -lens['source_distance'], source_pol=pol,
                    wavelength=wl, lens_periphery_summary=lens['lens_periphery_summary'],
                    lens_center_summary=lens['lens_center_summary'], hexgridset=lens['hexgridset'],
                    x_pts=x, y_pts=y)
        got = ma.build_nearfield(**args)
        info = _lib.default_context().nearfield_kernels()
        assert info['family'] == 'orders-along-x', info
        want = nearfield_oracle.build_nearfield(**args)
        # (a normally incident plane wave on a centre table without (0, 0): no order propagates, all zeros)
        scale = max(max(np.abs(w).max() for w in want[:4]), 1e-300)
        for g, w in zip(got[:4], want[:4]):
            assert int(np.count_nonzero((g == 0) != (w == 0))) == 0
            assert np.abs(g - w).max() <= TOL * scale
        assert abs(got[6] - want[6]) <= 1e-12 * abs(want[6])
    # (slots run from a collection's lowest order to its highest: a hole in the list is a slot of zeros)
    spans = [[e['ox'] for g in gc.grating_list for e in g.data] for _, gc in lens['collections']]
    assert info['ring_orders_max'] == max(max(v) - min(v) + 1 for v in spans)


@pytest.mark.parametrize('entries,pols', [(12, 'x'), (27, 'y'), (45, 'xyz'), (5, 'z')])
def test_centre_blocks_many_types_and_straddling_waves(ma, entries, pols):
    """The centre section of the field kernel stages one table cell's nodes x amplitudes x (up to 20)
    cell types per order through LDS and serves a wave in rounds, one per (table cell, group of 20
    types) among its lanes.  Tables of 27 and 45 types (two and three groups), a source just off the
    window's middle (ux = 0 and uy = 0 - table nodes - cross the window, so waves straddle table
    cells) and the three-polarisation batch, against the oracle; every type must occur."""
    from oracle import nearfield_oracle
    import math
    from metalens_amd import layout, synthetic
    wl = 580e-9
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design,
                               radius=40e-6, numerical_aperture=0.4, wavelength=wl,
                               switch_angle=9 * math.pi / 180, num_gratings=20, num_entries=entries,
                               design_kwargs={'wavelength': wl})
    cells = np.array(lens['lens_center_summary'], dtype=float)
    # spread the cell types over the whole table (the design uses what the phase profile needs)
    rng = np.random.default_rng(entries)
    cells[:, 2] = rng.integers(0, entries, size=len(cells))
    assert np.unique(cells[:, 2]).size == entries
    pitch = wl / 2.2
    # (the corners of the window lie beyond the switch radius: waves with centre AND ring samples)
    x = 0.4e-6 + (np.arange(120) - 60) * pitch
    y = -0.3e-6 + (np.arange(112) - 56) * pitch
    assert math.hypot(x[0], y[0]) > lens['r_for_switch'] > 0.5 * abs(x[0])
    common = dict(wavelength=wl, lens_periphery_summary=lens['lens_periphery_summary'],
                  lens_center_summary=cells, hexgridset=lens['hexgridset'], x_pts=x, y_pts=y)
    src = dict(source_x=0.52e-6, source_y=-0.21e-6, source_z=-lens['source_distance'])
    if len(pols) == 1:
        got = {pols: ma.build_nearfield(source_pol=pols, **src, **common)}
    else:
        # the batch kernel (x, y, z in one pass), fields read back member by member
        from metalens_amd import _lib
        from metalens_amd.nearfield import nearfield_params
        ctx = _lib.default_context()
        first = ma.build_nearfield(source_pol=pols[0], ctx=ctx, **src, **common)   # uploads tables and layout
        params = (_lib.NearfieldParams * len(pols))()
        for m, pol in enumerate(pols):
            params[m] = nearfield_params(src['source_x'], src['source_y'], src['source_z'], pol, wl, first[7],
                                         1e-30, ma.constants.c0, ma.constants.Z0)
        xs, ys = _lib.f64(x), _lib.f64(y)
        _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, len(pols), _lib.dptr(xs), xs.size,
                                                    _lib.dptr(ys), ys.size))
        got = {}
        for m, pol in enumerate(pols):
            _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
            F = [np.empty((x.size, y.size), dtype=np.complex128) for _ in range(4)]
            _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(f) for f in F]))
            got[pol] = F
        _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))
    for pol, g in got.items():
        want = nearfield_oracle.build_nearfield(source_pol=pol, **src, **common)
        scale = max(np.abs(w).max() for w in want[:4])
        assert scale > 0
        for gf, w in zip(g[:4], want[:4]):
            assert int(np.count_nonzero((gf == 0) != (w == 0))) == 0
            assert np.abs(gf - w).max() <= TOL * scale


def test_layout_limits_are_refused(ma):
    """what the geometry records cannot hold is refused at upload with a message, not truncated:
    a HexGridSet index outside 0 ... 2047 (11 bits above the ring index) and rings that use more
    than 16 different grating collections (the per-collection descriptors in the kernel arguments)"""
    import copy
    from metalens_amd import _lib, packing
    lens = _synthetic_lens(80e-6, 0.4, 580e-9, switch_deg=9.0)
    S, cells = lens['lens_periphery_summary'], np.array(lens['lens_center_summary'], dtype=float)
    ctx = _lib.Context(0)
    for bad in (2048.0, -1.0):
        c = cells.copy()
        c[5, 2] = bad
        with pytest.raises(_lib.MetalensHipError, match='grating index'):
            packing.upload_layout(ctx, S, c)
    S17 = copy.copy(S)
    n = len(S['r_center_list'])
    assert n >= 17
    S17['gratingcollection_index_here_list'] = [k % 17 for k in range(n)]
    with pytest.raises(_lib.MetalensHipError, match='more than 16 grating collections'):
        packing.upload_layout(ctx, S17, cells)
    packing.upload_layout(ctx, S, cells)   # and the context still takes a good one


@pytest.mark.parametrize('seed,orders', [(5, 'survey'), (6, 'survey'), (7, 'physical')])
def test_random_windows_sweep(ma, seed, orders):
    """random windows, sources and polarisations on two lenses against the oracle
    (tests/extra_random_sweep.py; run that script for hundreds of cases): every discrete decision
    (ring, sector, nearest cell) must agree, fields to 1e-12 - with the three-order tables and with
    the order lists characterize() would record"""
    import extra_random_sweep
    worst, flips, _ties = extra_random_sweep.run(16, seed, orders)
    assert flips == 0
    assert worst < TOL


def _record(name, **values):
    """measured parity figures of a GPU run, one JSON line each, for profiles/ (ML_RECORD_PARITY=file)"""
    path = os.environ.get('ML_RECORD_PARITY')
    if path:
        import json
        with open(path, 'a') as f:
            f.write(json.dumps(dict(name=name, **values)) + '\n')


# |dE| / |E| over the directions above 1e-3 of the PEAK of the far field, GPU against the fp64 oracle on the same
# (GPU-made) near field; north_star: < 1e-12.  The peak is the maximum over the WHOLE direction grid (the GPU's own
# map), and up to 4096^2 the oracle evaluates the whole grid too; beyond, a 16 x 16 sample plus the 3 x 3 directions
# around the peak.  (Until round 6 both the floor and the peak came from the 16 x 16 sample alone, which misses the
# focus: "1e-3 of the peak" then admitted directions ~1e-5 of the true peak and the figures read 1.6e-12 at 2048^2,
# 7e-13 at 4096^2.  tools/parity_isolate.py, profiles/r06_parity_isolate_{2048,4096}.txt: on the whole grid the pruned
# FFT is at 5.5e-13 / 1.6e-13, the folded fp64 GEMMs - cos / sin advanced by rotations between table seeds - at
# 6.2e-13 / 1.3e-12.)  Where everybody stands against long-double sums: tools/oracle_longdouble.py.
# Bounds: 1e-12 for the default (FFT) path at every size; the folded GEMMs ~1.3 x what they measure.
# fp32 GEMM mode: twice the value measured at its size; the 1e-4 of BASELINE.json is met relative to max|E|
# - the normalisation the bench line names.
POINTWISE = {   # (side, precision, method) -> bound; measured GPU vs oracle in the comment
    (2048, 'f64', 'auto'): 1.0e-12,     # 5.5e-13 (whole grid)
    (4096, 'f64', 'auto'): 1.0e-12,     # 1.6e-13 (whole grid)
    (4096, 'f64', 'gemm'): 1.7e-12,     # 1.3e-12 (whole grid)
    (8192, 'f64', 'auto'): 1.0e-12,
    (16384, 'f64', 'auto'): 1.0e-12,
    (16384, 'f64', 'gemm'): 2.1e-12,
    (16384, 'f32', 'auto'): 1.5e-3,     # 7.4e-4
}
FULL_GRID_ORACLE_UP_TO = 4096


def pointwise_rel_err(got, ref, floor=1e-3, peak=None):
    """max |d| / |ref| over the points where |ref| > floor * peak (default: max|ref|) - the far-field
    tolerance of this suite is otherwise normalised by max|E|, which says little about the dim directions"""
    big = np.abs(ref) > floor * (np.abs(ref).max() if peak is None else peak)
    if not big.any():
        return 0.0
    return (np.abs(got - ref)[big] / np.abs(ref)[big]).max()


@pytest.mark.parametrize('side,M,diameter,na,precision,method', [
    (2048, 256, 1e-3, 0.5, 'f64', 'auto'),        # BASELINE configs[0]: the reference's own CPU-runnable case
    (4096, 512, 1e-3, 0.5, 'f64', 'auto'),        # north-star size; both axes run as pruned FFTs
    (4096, 512, 1e-3, 0.5, 'f64', 'gemm'),        # the same through the folded fp64 GEMMs
    (8192, 512, 2e-3, 0.94, 'f64', 'auto'),       # BASELINE configs[2]'s problem on one GPU
    (16384, 1024, 4e-3, 0.5, 'f64', 'auto'),      # BASELINE configs[4]'s size (two-level FFT: lattice > 8192)
    (16384, 1024, 4e-3, 0.5, 'f64', 'gemm'),      # ... through the folded fp64 GEMMs
    (16384, 1024, 4e-3, 0.5, 'f32', 'auto'),      # ... and its fp32 GEMM-cast MFMA path, tolerance 1e-4
])
def test_north_star_size_properties(ma, side, M, diameter, na, precision, method):
    """The north-star size (4096^2 aperture window -> 512^2 directions, fp64), BASELINE
    configs[2]'s problem (8192^2 on the 2 mm NA 0.94 lens) and configs[4]'s (16384^2 -> 1024^2,
    fp64 and the fp32 GEMM mode; read per SURVEY.md D2 as a zoomed DIRECTION grid - the reference
    has no finite-distance propagator, nearfield_farfield.py:97-101) through the GPU-resident
    pipeline, checked by properties that do not need the oracle at that size - determinism, exact
    homogeneity in the dipole moment, additivity over mirrored row shards - plus the oracle on a
    sample: 16 near-field rows and a 16 x 16 sample of the far-field amplitudes evaluated by the
    oracle from the GPU's own near field."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    from metalens_amd import _lib
    from metalens_amd.pipeline import HotPath
    from oracle import farfield_oracle, nearfield_oracle
    wl = 580e-9
    tol = TOL if precision == 'f64' else 1e-4
    lens, x, u = bench.build_workload(side, M, diameter, na, wl, 1.0)
    src = (0.0, 0.0, -lens['source_distance'], 'x')
    args = (src, wl, lens['lens_periphery_summary'], lens['lens_center_summary'],
            lens['hexgridset'], x, x, u, u)
    ctx = _lib.default_context()
    try:
        one = HotPath(*args, ctx=ctx, precision=precision, method=method)
        one.step()
        one.sync()
        r1 = one.results()
        # (lattices beyond 8192 samples run as two-level FFTs; the fp32 mode asks for the GEMMs)
        want_kernels = ('fft', 'fft') if method == 'auto' and precision == 'f64' else ('folded', 'folded')
        assert ctx.plan_kernels() == want_kernels
        # (a) sample against the oracle
        rows = slice(side // 2 - 8, side // 2 + 8)
        F = [np.empty((side, side), dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
        want = nearfield_oracle.build_nearfield(src[0], src[1], src[2], src[3], wl,
                                                lens['lens_periphery_summary'],
                                                lens['lens_center_summary'], lens['hexgridset'],
                                                x_pts=x[rows], y_pts=x)
        scale = max(np.abs(w).max() for w in want[:4])
        assert max(np.abs(g[rows] - w).max() for g, w in zip(F, want[:4])) <= TOL * scale
        # directions the oracle evaluates: all of them up to 4096^2; else a 16 x 16 sample + the 3 x 3 around the peak
        amp = np.abs(r1['a_theta']) ** 2 + np.abs(r1['a_phi']) ** 2
        pi, pj = np.unravel_index(np.argmax(amp), amp.shape)
        if side <= FULL_GRID_ORACLE_UP_TO:
            sel_i = sel_j = np.arange(M)
        else:
            sel_i = np.unique(np.concatenate((np.arange(0, M, M // 16), np.clip([pi - 1, pi, pi + 1], 0, M - 1))))
            sel_j = np.unique(np.concatenate((np.arange(0, M, M // 16), np.clip([pj - 1, pj, pj + 1], 0, M - 1))))
        ref = farfield_oracle.farfield_direct(*F, x, x, wl, one.n_glass, u[sel_i], u[sel_j])
        for key in ('a_theta', 'a_phi'):
            got = r1[key][np.ix_(sel_i, sel_j)]
            peak = np.abs(r1[key]).max()            # of the WHOLE map (the sample alone misses the focus)
            assert np.abs(got - ref[key]).max() <= tol * peak
            # pointwise |dE| / |E| where |E| > 1e-3 of the peak: rounding of an N^2-term sum is absolute
            # (~1e-15 max|E|), so the dimmest of these directions carries up to ~1e-12 relative
            pw = pointwise_rel_err(got, ref[key], peak=peak)
            _record('north_star_pointwise', side=side, precision=precision, method=method, key=key,
                    pointwise=float(pw), rel_to_max=float(np.abs(got - ref[key]).max() / peak),
                    directions=int(sel_i.size * sel_j.size))
            assert pw <= POINTWISE[(side, precision, method)], (pw, POINTWISE[(side, precision, method)])
        if precision == 'f32':   # really the fp32 arithmetic: above fp64 round-off
            assert np.abs(r1['a_theta'][np.ix_(sel_i, sel_j)] - ref['a_theta']).max() > 1e-10 * np.abs(ref['a_theta']).max()
        del F, ref, want
        # (b) determinism: the same step again, bit for bit
        one.step()
        one.sync()
        r1b = one.results()
        for key in ('a_theta', 'a_phi', 'Nx', 'Ly'):
            assert np.array_equal(r1[key], r1b[key]), key
        assert r1['power_local_rows'] == r1b['power_local_rows']
        # (c) homogeneity: twice the dipole moment is an exact power-of-two scaling of every field
        two_p = HotPath(*args, ctx=ctx, dipole_moment=2e-30, precision=precision, method=method)
        two_p.step()
        two_p.sync()
        r2 = two_p.results()
        for key in ('a_theta', 'a_phi', 'Nx', 'Ny', 'Lx', 'Ly'):
            assert np.array_equal(r2[key], 2.0 * r1[key]), key
        assert np.array_equal(r2['P'], 4.0 * r1['P'], equal_nan=True)
        assert r2['power_local_rows'] == 4.0 * r1['power_local_rows']
        # (d) additivity: the aperture as the two mirrored row shards two ranks would own
        total = {k: 0 for k in ('Nx', 'Ny', 'Lx', 'Ly')}
        power = 0.0
        for rank in (0, 1):
            half = HotPath(*args, ctx=ctx, rank=rank, world=2, precision=precision, method=method)
            half.step_local()
            half.sync()
            vec = [np.empty(half.shape, dtype=np.complex128) for _ in range(4)]
            _lib.check(ctx.lib.ml_farfield_download(ctx.handle, *[_lib.dptr(v) for v in vec]))
            for k, v in zip(('Nx', 'Ny', 'Lx', 'Ly'), vec):
                total[k] = total[k] + v
            pw = _lib.c_double(0)
            _lib.check(ctx.lib.ml_nearfield_result(ctx.handle, _lib.byref(pw), None, 0, None))
            power += pw.value * half.dxp * half.dyp
        for key in total:
            assert np.abs(total[key] - r1[key]).max() <= max(1e-13, 10 * tol * (precision == 'f32')) * np.abs(r1[key]).max(), key
        assert abs(power - r1['power_local_rows']) <= 1e-12 * r1['power_local_rows']
    finally:
        ctx.set_precision('f64')
        ctx.set_method('auto')


@pytest.mark.parametrize('N,M', [(2048, 256), (16384, 1024), (65536, 1024)])
def test_large_aperture_plans_take_the_folded_path(ma, N, M):
    """A direction grid computed as (k - M/2) * du in floating point is centre-symmetric only to
    about one ulp; for large apertures that is more than 1e-13 rad of phase at the aperture edge.
    The symmetry test scales with the grid's own rounding (transform_route.h symmetry_tolerance), so
    such grids must still plan the folded kernel (the generic complex GEMM is ~5x slower), while
    a grid perturbed well above its rounding must not."""
    from metalens_amd import _lib
    ctx = _lib.default_context()
    lib = ctx.lib
    wl, n_glass = 580e-9, 1.459
    pitch = wl / 2.2
    du = (wl / n_glass) / (pitch * N)
    u = _lib.f64((np.arange(M) - M // 2) * du)

    def planned_kernel(uy):
        _lib.check(lib.ml_farfield_plan(ctx.handle, N, N, pitch, pitch, wl, n_glass, _lib.dptr(u),
                                        u.size, _lib.dptr(uy), uy.size, 0))
        k = _lib.c_int(-1)
        _lib.check(lib.ml_farfield_plan_info(ctx.handle, _lib.byref(k)))
        return k.value

    try:
        ctx.set_method('gemm')
        assert planned_kernel(u) == 1
        bent = u.copy()
        bent[3] += 1e-9 * du * M      # far above rounding, far below anything a user would notice
        assert planned_kernel(bent) == 0
        # left to itself the plan takes the pruned FFT (one level up to 8192 samples, up to eight
        # interleaved sub-sequences beyond), and the same perturbation sends it back to the GEMMs
        ctx.set_method('auto')
        assert planned_kernel(u) == 2
        assert planned_kernel(bent) == 0
    finally:
        ctx.set_method('auto')
        ctx.sync()


def test_nearest_cell_ties_follow_ckdtree(ma):
    """A symmetric grid with an ODD number of samples has its middle row and column on mirror
    lines of the hexagonal cell lattice: those samples are exactly equidistant from two cells and
    the reference's choice is cKDTree's traversal order.  The kernels report them and the host
    asks cKDTree (metalens_amd/ties.py); every sample, ties included, must then equal the
    oracle.  Also through the resident pipeline, whose first results() settles them."""
    from metalens_amd import _lib, ties
    from metalens_amd.pipeline import HotPath
    from oracle import nearfield_oracle
    wl = 580e-9
    lens = _synthetic_lens(40e-6, 0.4, wl, switch_deg=9.0)
    r_c = float(lens['lens_periphery_summary']['r_min_list'][0])
    R = float(lens['lens_periphery_summary']['r_max_list'][-1])
    src = (0.4e-6, -0.3e-6, -lens['source_distance'], 'y')
    common = (wl, lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'])
    assert r_c > 4e-6 and R > 30e-6
    for n in (61, 251):                            # centre disc only; centre + periphery
        x = (np.arange(n) - n // 2) * (wl / 2.2)   # symmetric, x[n // 2] == 0.0 exactly
        assert x[n // 2] == 0.0
        dec = {}
        want = nearfield_oracle.build_nearfield(*src, *common, x_pts=x, y_pts=x, decisions=dec)
        n_ties = int(np.count_nonzero(dec['nearest_tie']))
        assert n_ties > 0                          # the case really exercises ties
        got = ma.build_nearfield(*src, *common, x_pts=x, y_pts=x)
        for g, w, key in zip(got[:4], want[:4], ('Ex', 'Ey', 'Hx', 'Hy')):
            err, flips = field_errors(g, w)
            assert flips == 0 and err < TOL, (n, key, err, flips, n_ties)
        assert abs(got[6] - want[6]) <= 1e-12 * abs(want[6])
        # nothing is left pending after the drop-in call
        assert ties.pending(_lib.default_context()).size == 0
    # the resident pipeline: the first results() settles the ties and repeats the pass
    u = np.linspace(-0.1, 0.1, 64)
    hp = HotPath(src, *common, x, x, u, u, ctx=_lib.Context(0))
    hp.step()
    hp.sync()
    assert ties.pending(hp.ctx).size > 0
    res = hp.results()
    assert ties.pending(hp.ctx).size == 0
    # which scipy settled them rides with the result (the choice is that library's tree traversal)
    import scipy
    assert res['tie_breaker']['scipy'] == scipy.__version__ and res['tie_breaker']['samples'] > 0
    assert res['tie_breaker']['fixture_scipy'] == ties.FIXTURE_SCIPY
    F = [np.empty((x.size, x.size), dtype=np.complex128) for _ in range(4)]
    _lib.check(hp.ctx.lib.ml_fields_download(hp.ctx.handle, *[_lib.dptr(a) for a in F]))
    scale = max(np.abs(w).max() for w in want[:4])
    assert max(np.abs(g - w).max() for g, w in zip(F, want[:4])) <= TOL * scale
    hp.ctx.close()
