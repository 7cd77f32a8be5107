"""The far-field back end on the GPU, every row of tests/farfield_power_cases.py against the yardsticks of
tests/farfield_power_ref.py: the projection (csrc/farfield_project.hip project_point in project_kernel and in the fused
unfold_project_kernel) POINTWISE - never relative to the brightest direction of the map - at the directions on and
next to the rim of the unit circle and the axis, and the sweep sums (csrc/farfield_sums.hip accumulate_kernel,
accumulate_finish_kernel) at every loop and branch edge.  To isolate the projection from the transform in front of it the yardstick is fed the
GPU's OWN downloaded radiation vectors; the transform rows also hold those vectors against the oracle at the
project's TOL.  What each row is chosen for is the table's claim, held without a GPU by
test_farfield_power_cases.py.  Needs an MI355X.

The bounds, in units of u = 2**-53:

* NaN masks are identical, for P and both amplitudes.
* Amplitudes: kernel and yardstick apply the same correctly rounded operations to the same float64 inputs, so the
  same bits are expected; asserted is |delta| <= 16 u (sum of the magnitudes of the amplitude's four terms) per
  component - at most 8 roundings on either side - so that a signed zero or a library difference does not fail the
  test while a regulariser off by a factor fails by ten orders.  The count of entries that are not bit-identical
  is printed and recorded.
* P against power_from_amplitudes of the GPU's own amplitudes: |delta P| <= C_P u P_ref with C_P = 16, counted from
  project_point: hypot is documented at 1 ulp by the device library and by the host's, so the two moduli differ by at
  most 2 ulp = 4 u relative; the square doubles that and adds a rounding on either side (8 + 2 = 10); the sum of the
  two squares (both >= 0: no cancellation) adds 2 (12), the product with coef 2 (14), the division by uz + 1e-5 -
  the same bits on both sides, sqrt and the sum being correctly rounded - 2 (16); the doubling is exact.
* P through ml_farfield_lattice_power against project_points from the vectors (no amplitudes come back): the bound
  above plus what the amplitudes' own bound allows P to move, 2 |a| d + d d per amplitude with d = 16 u |terms|,
  times the direction's factor 2 coef / (uz + 1e-5).
* Sums: (1 + 8 + (ceil(blocks / 256) - 1) + 8) u of the sum against math.fsum of the float64 products of the
  DOWNLOADED P (one product, the block tree, the strided loop, the finishing tree; all terms >= 0), and 3 units more
  against metalens_amd/postprocess.py, which groups the cell differently.
"""
import functools
import math

import numpy as np
import pytest

import farfield_power_cases as cases
import farfield_power_ref as ref
from test_gpu_parity import TOL, _record

pytestmark = pytest.mark.gpu

WL, N_GLASS, Z0 = cases.WL, cases.N_GLASS, cases.Z0
U = 2.0 ** -53
C_AMP, C_P = 16, 16
VECTORS = ('Nx', 'Ny', 'Lx', 'Ly')


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


@pytest.fixture
def fresh():
    """a context of its own: no earlier test's sums or slots are there"""
    from metalens_amd import _lib
    c = _lib.Context()
    c.set_method('gemm')
    try:
        yield c
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def _aperture(nx, ny, seed=0):
    """seeded complex fields and their axes; shared, nobody writes to them"""
    rng = np.random.default_rng(1000 * nx + ny + seed)
    F = [rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny)) for _ in range(4)]
    x = (np.arange(nx) - 3.3) * (WL / 2.2)
    y = (np.arange(ny) + 11.1) * (WL / 2.3)
    for a in F + [x, y]:
        a.setflags(write=False)
    return F, x, y


def _upload(ctx, F, rows=None):
    from metalens_amd import _lib
    part = [np.ascontiguousarray(f if rows is None else f[rows]) for f in F]
    _lib.check(ctx.lib.ml_fields_upload(ctx.handle, part[0].shape[0], part[0].shape[1], *[_lib.dptr(a) for a in part]))
    ctx.fields_owner = None


def _mesh(ux, uy, pair_list):
    return (ux, uy) if pair_list else np.meshgrid(ux, uy, indexing='ij')


def _bits(a, b):
    """equal bit for bit (the sign of a zero included) up to which NaN it is"""
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    af, bf = np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64)
    ok = ~np.isnan(af)
    return np.array_equal(np.signbit(af[ok]), np.signbit(bf[ok]))


def _check_vectors(V, want, what):
    for key in VECTORS:
        assert np.abs(V[key] - want[key]).max() <= TOL * np.abs(want[key]).max(), (what, key)


def _check_projection(name, V, P, a_theta, a_phi, ux, uy, pair_list):
    """P and both amplitudes of the GPU against the yardstick fed the GPU's own vectors V; -> worst error over bound"""
    UX, UY = _mesh(ux, uy, pair_list)
    P_ref, t_ref, p_ref, mag_t, mag_p = ref.project_points(V['Nx'], V['Ny'], V['Lx'], V['Ly'], UX, UY, WL, N_GLASS, Z0)
    nan = np.isnan(P_ref)
    assert nan.any() and not nan.all()
    for a in (P, a_theta.real, a_theta.imag, a_phi.real, a_phi.imag):
        assert np.array_equal(np.isnan(a), nan), name
    ok = ~nan
    worst, differ = 0.0, 0
    for got, want, mag in ((a_theta, t_ref, mag_t), (a_phi, p_ref, mag_p)):
        for part in ('real', 'imag'):
            g, w, m = getattr(got, part)[ok], getattr(want, part)[ok], getattr(mag, part)[ok]
            differ += int((g != w).sum())
            err, bound = np.abs(g - w), C_AMP * U * m
            assert np.all(err <= bound), (name, part, float((err / np.maximum(bound, 1e-300)).max()))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    P_own = ref.power_from_amplitudes(a_theta, a_phi, UX, UY, WL, N_GLASS, Z0)
    err, bound = np.abs(P[ok] - P_own[ok]), C_P * U * P_own[ok]
    worst_P = float((err[bound > 0] / bound[bound > 0]).max())
    print('power-case %s: amplitudes %d of %d components not bit-identical, worst %.3f of the bound; P worst %.3f of '
          'its bound' % (name, differ, 4 * int(ok.sum()), worst, worst_P))
    _record('farfield_power_case', row=name, amp_differ=differ, amp=worst, P=worst_P)
    assert np.all(err <= bound), (name, 'P', worst_P)
    return max(worst, worst_P)


def test_rim_as_a_pair_list(ma, ctx):
    """project_point's pair_list branch (uy[i], my = 1) at RIM's 64 directions, through project_kernel"""
    from oracle import farfield_oracle
    ux, uy, classes = cases.rim()
    F, x, y = _aperture(*cases.APERTURE)
    _upload(ctx, F)
    t = ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux, uy, pair_list=True, ctx=ctx)
    t.transform()
    V = t.radiation_vectors()
    P, a_theta, a_phi = t.project(Z0)
    _check_vectors(V, dict(zip(VECTORS, farfield_oracle.radiation_vectors_pairs(*F, x, y, WL, N_GLASS, ux, uy))), 'rim')
    assert np.array_equal(np.isnan(P), np.array([c == 'nan' for c in classes]))
    _check_projection('rim-pairs', V, P, a_theta, a_phi, ux, uy, True)
    # the (0, 0) rule: the vectors themselves, of either sign of zero - and not next to the axis
    Z = Z0 / N_GLASS
    for k, c in enumerate(classes):
        assert (a_theta[k] == V['Ly'][k] + Z * V['Nx'][k]) == (c == 'zero'), k


def test_rim_as_tensor_axes_through_lattice_power(ctx):
    """ml_farfield_lattice_power (from_fft) on seeded 'fft' arrays of 19 x 261 with RIM's values as its lists: two
    column blocks of 256, the second with 5 lanes"""
    from metalens_amd import _lib
    ux, uy = cases.rim_axes()
    rng = np.random.default_rng(7)
    fft = [rng.standard_normal((ux.size, uy.size)) + 1j * rng.standard_normal((ux.size, uy.size)) for _ in range(4)]
    fftEx, fftEy, fftHx, fftHy = fft
    dxp, dyp = WL / 2.2, WL / 2.3
    P = np.empty((ux.size, uy.size))
    _lib.check(ctx.lib.ml_farfield_lattice_power(ctx.handle, ux.size, uy.size, *[_lib.dptr(a) for a in fft],
                                                 _lib.dptr(ux), _lib.dptr(uy), dxp, dyp, WL, N_GLASS, Z0, _lib.dptr(P)))
    UX, UY = np.meshgrid(ux, uy, indexing='ij')
    vec = (-fftHy * dxp * dyp, fftHx * dxp * dyp, fftEy * dxp * dyp, -fftEx * dxp * dyp)   # as the reference forms them
    P_ref, a_t, a_p, mag_t, mag_p = ref.project_points(*vec, UX, UY, WL, N_GLASS, Z0)
    nan = np.isnan(P_ref)
    assert np.array_equal(np.isnan(P), nan)
    assert set(cases.classify(UX, UY)[:, 256:].ravel()) >= {'uz0', 'tiny', 'nan'}
    ok = ~nan
    unit = ref.power_from_amplitudes(np.ones_like(P_ref), np.zeros_like(P_ref), UX, UY, WL, N_GLASS, Z0)
    moved = 0.0
    for a, mag in ((a_t, mag_t), (a_p, mag_p)):
        d = C_AMP * U * np.abs(mag)
        moved = moved + 2 * np.abs(a) * d + d * d
    bound = (C_P * U * P_ref + unit * moved)[ok]
    err = np.abs(P - P_ref)[ok]
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    differ = int((P[ok] != P_ref[ok]).sum())
    print('power-case rim-axes: P %d of %d not bit-identical, worst %.3f of the bound' % (differ, int(ok.sum()), worst))
    _record('farfield_power_case', row='rim-axes', P_differ=differ, P=worst)
    assert np.all(err <= bound), worst


@functools.lru_cache(maxsize=1)
def _folded_case():
    from oracle import farfield_oracle
    nx, ny = cases.FOLDED.shape[:2]
    F, x, y = _aperture(nx, ny)
    ux, uy = cases.folded_axes()
    want = dict(zip(VECTORS, farfield_oracle.radiation_vectors(*F, x, y, WL, N_GLASS, ux, uy)))
    return F, x, y, ux, uy, want


def _folded_transform(ma, ctx):
    F, x, y, ux, uy, want = _folded_case()
    _upload(ctx, F)
    t = ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux, uy, ctx=ctx)
    return t, ux, uy, want


def test_folded_fused_and_separate_kernels_give_the_same_bits(ma, ctx):
    """FOLDED under method 'gemm', three ways on the same fields: (a) project with the unfold pending -
    unfold_project_kernel; (b) download the vectors first - zunfold_out_kernel, then project_kernel; (c) two uneven
    mirrored shards, the second accumulating, projected while pending; (d) two uneven plain row blocks, the second
    accumulating.  (a) and (b): the same bits everywhere; all four against the yardstick."""
    F = _folded_case()[0]
    nx = cases.FOLDED.shape[0]
    t, ux, uy, want = _folded_transform(ma, ctx)
    t.transform()
    assert ctx.plan_kernels() == ('folded', 'folded')
    Pa, ta, pa = t.project(Z0)                               # (a): the unfold is still pending
    Va = t.radiation_vectors()
    t.transform()
    Vb = t.radiation_vectors()                               # (b): materialises the vectors
    Pb, tb, pb = t.project(Z0)
    for key in VECTORS:
        assert _bits(Va[key], Vb[key]), key
    assert _bits(Pa, Pb) and _bits(ta, tb) and _bits(pa, pb)
    for k, (row0, nxl) in enumerate(cases.FOLDED.pieces):    # (c)
        _upload(ctx, F, cases.mirrored_rows(nx, row0, nxl))
        t.transform(row0=row0, accumulate=k > 0, mirrored=True)
        assert ctx.plan_kernels() == ('folded', 'folded')
    Pc, tc, pc = t.project(Z0)
    Vc = t.radiation_vectors()
    # (d) two uneven plain row blocks, the second accumulating: no mirror partners, so the generic stage 2 writes the
    # vectors itself and project_kernel runs on sums of two calls
    for k, (row0, nxl) in enumerate(cases.FOLDED.blocks):
        _upload(ctx, F, np.arange(row0, row0 + nxl))
        t.transform(row0=row0, accumulate=k > 0)
        assert ctx.plan_kernels()[0] == 'folded'
    Pd, td, pd = t.project(Z0)
    Vd = t.radiation_vectors()
    for name, V, P, a_t, a_p in (('folded-fused', Va, Pa, ta, pa), ('folded-separate', Vb, Pb, tb, pb),
                                 ('folded-pieces', Vc, Pc, tc, pc), ('folded-blocks', Vd, Pd, td, pd)):
        _check_vectors(V, want, name)
        _check_projection(name, V, P, a_t, a_p, ux, uy, False)
    mx, my = cases.FOLDED.shape[2:]
    Z = Z0 / N_GLASS
    assert ta[mx // 2, my // 2] == Va['Ly'][mx // 2, my // 2] + Z * Va['Nx'][mx // 2, my // 2]   # the (0, 0) rule


@pytest.mark.parametrize('pending', [True, False])
def test_project_reduce_without_a_communicator_is_the_one_pass_projection(ma, ctx, pending):
    """ml_farfield_project_reduce on a context without a communicator runs stage 1 (vectors -> amplitudes) and then
    stage 2 (amplitudes -> power) of project_point: the bits of ml_farfield_project, from a pending unfold (stage 1 in
    the fused kernel) and from materialised vectors"""
    from metalens_amd import _lib
    t, ux, uy, _want = _folded_transform(ma, ctx)
    t.transform()
    if not pending:
        t.radiation_vectors()
    one = t.project(Z0)
    t.transform()
    if not pending:
        t.radiation_vectors()
    _lib.check(ctx.lib.ml_farfield_project_reduce(ctx.handle, Z0))
    two = t.project(Z0)                                      # (the reduce did the projection: this downloads it)
    assert np.isnan(one[0]).any() and not np.isnan(one[0]).all()
    for a, b in zip(one, two):
        assert _bits(a, b)


# ---- the sums ---------------------------------------------------------------------------------------------------------

def _project_row(ma, ctx, ux, uy, pair_list, seed=0):
    """upload the row's aperture, transform, project -> (transform object, vectors, downloaded P)"""
    F, x, y = _aperture(*cases.APERTURE, seed)
    _upload(ctx, F)
    t = ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux, uy, pair_list=pair_list, ctx=ctx)
    t.transform()
    P = t.project(Z0)[0]
    return t, P


def _accumulate(ctx, weight, cone, slot, reset):
    from metalens_amd import _lib
    _lib.check(ctx.lib.ml_farfield_accumulate(ctx.handle, float(weight), cone[0], cone[1], cone[2], slot, int(reset)))


def _sums(ctx, shape, n_slots):
    from metalens_amd import _lib
    P_sum = None if shape is None else np.full(shape, -1.0)
    total, cone = np.full(max(n_slots, 1), -1.0), np.full(max(n_slots, 1), -1.0)
    _lib.check(ctx.lib.ml_farfield_sums(ctx.handle, _lib.dptr(P_sum), _lib.dptr(total), _lib.dptr(cone), n_slots))
    return P_sum, total, cone


def _check_sums(name, row, P, total, cone):
    """a slot's two sums against the yardsticks of the downloaded P; -> worst error over bound"""
    from metalens_amd import postprocess
    pair = row.kind == 'pairs'
    s = ref.sweep_sums(P, row.ux, row.uy, pair, row.cone[0], row.cone[1:])
    units = 1 + ref.sum_bound_units(P.size)
    assert s['total'] > 0 and s['cone'] > 0
    worst = max(abs(total - s['total']) / (units * U * s['total']), abs(cone - s['cone']) / (units * U * s['cone']))
    print('power-case %s: total %.17g cone %.17g, worst %.3f of the bound of %d units' % (name, total, cone, worst, units))
    _record('farfield_power_case', row=name, sums=worst)
    assert abs(total - s['total']) <= units * U * s['total']
    assert abs(cone - s['cone']) <= units * U * s['cone']
    if not pair:
        dux = row.ux[1] - row.ux[0] if row.ux.size > 1 else 1.0
        duy = row.uy[1] - row.uy[0] if row.uy.size > 1 else 1.0
        want_total = postprocess.total_power(P, dux, duy)
        want_cone = postprocess.encircled_power(P, row.ux, row.uy, dux, duy, sin_max=row.cone[0], center=row.cone[1:])
        assert abs(total - want_total) <= (units + 3) * U * want_total
        assert abs(cone - want_cone) <= (units + 3) * U * want_cone
    return worst


@pytest.mark.parametrize('name', sorted(cases.SUM_ROWS))
def test_sum_rows(ma, fresh, name):
    """transform, project, download P, accumulate, ml_farfield_sums: total_P and cone_P against sweep_sums of the
    downloaded P and against postprocess; P_sum of one map with weight 1 is the map.  The vectors against the oracle
    (the rows with one direction on an axis are plans no transform test has used)."""
    from metalens_amd import _lib
    from oracle import farfield_oracle
    row = cases.SUM_ROWS[name]
    pair = row.kind == 'pairs'
    t, P = _project_row(ma, fresh, row.ux, row.uy, pair)
    F, x, y = _aperture(*cases.APERTURE)
    oracle = farfield_oracle.radiation_vectors_pairs if pair else farfield_oracle.radiation_vectors
    _check_vectors(t.radiation_vectors(), dict(zip(VECTORS, oracle(*F, x, y, WL, N_GLASS, row.ux, row.uy))), name)
    assert np.isnan(P).any() == row.claims['nan'] and np.isfinite(P).any()
    if name == 'exact-cone':
        # the 12 directions ON the edge carry a share of cone_P a thousand times the bound: `<` cannot pass
        inside, edge = ref.cone_masks(row.ux, row.uy, False, row.cone[0], row.cone[1:])
        assert (int(inside.sum()), int(edge.sum())) == (81, 12)
        cell = ref.cell_of(row.ux, row.uy, False)
        share = math.fsum((P * cell)[edge])
        bound = (1 + ref.sum_bound_units(P.size)) * U * math.fsum((P * cell)[inside])
        assert share > 1000 * bound
    _accumulate(fresh, 1.0, row.cone, 0, True)
    P_sum, total, cone = _sums(fresh, P.shape, 1)
    assert _bits(P_sum, P)
    _check_sums(name, row, P, total[0], cone[0])
    if name == 'two-rounds':
        # two more slots, then ml_farfield_total_power: the bits of slot 0's total, and nothing else moves
        _accumulate(fresh, 2.0, (0.5, 0.0, 0.0), 1, False)
        _accumulate(fresh, -1.0, (0.1, -0.3, 0.2), 2, False)
        before = _sums(fresh, P.shape, 3)
        assert before[1][0] == total[0] and before[2][0] == cone[0]
        assert before[1][1] == total[0] and before[1][2] == total[0] and len(set(before[2])) == 3
        assert _bits(before[0], ref.p_sum([P, P, P], [1.0, 2.0, -1.0], [1, 0, 0]))
        one = np.full(1, -1.0)
        _lib.check(fresh.lib.ml_farfield_total_power(fresh.handle, _lib.dptr(one)))
        assert one[0] == total[0]
        after = _sums(fresh, P.shape, 3)
        for a, b in zip(before, after):
            assert _bits(a, b)


def test_weights_slots_and_resets(ma, fresh):
    """three maps on one grid with NaN corners through the table's two call sequences: P_sum has the bits of
    p_sum(...) - which entries are NaN and 0.0 * NaN staying NaN included -, slots 0, 1 and 4095 hold the sums of the
    map last accumulated into them, a slot never written reads 0, and the same calls again give the same bits"""
    ux, uy = cases.WEIGHTS_GRID
    row = cases.SumRow('grid', ux, uy, cases.WEIGHTS_CONE, {})

    def run():
        out = []
        in_slot = {}
        for seq in cases.WEIGHTS_CALLS:
            maps = []
            for k, weight, slot, reset in seq:
                _t, P = _project_row(ma, fresh, ux, uy, False, seed=k)
                _accumulate(fresh, weight, cases.WEIGHTS_CONE, slot, reset)
                maps.append(P)
                in_slot[slot] = P
            P_sum, total, cone = _sums(fresh, maps[0].shape, cases.MAX_SLOTS)
            want = ref.p_sum(maps, [c[1] for c in seq], [c[3] for c in seq])
            assert np.isnan(want).any() and _bits(P_sum, want)
            assert np.array_equal(np.isnan(P_sum), np.isnan(maps[0]))
            for slot, P in in_slot.items():
                _check_sums('weights-slot%d' % slot, row, P, total[slot], cone[slot])
            never = np.ones(cases.MAX_SLOTS, dtype=bool)
            never[list(in_slot)] = False
            assert not total[never].any() and not cone[never].any() and never[2]
            out.append((P_sum, total, cone))
        return out

    first, second = run(), run()
    for a, b in zip(first, second):
        for p, q in zip(a, b):
            assert _bits(p, q)


def test_sums_belong_to_the_plan_they_were_started_on(ma, fresh):
    """P_sum is sized by the plan it was accumulated on: adding onto it (reset = 0) before anything was accumulated,
    or under a plan of another direction count or kind, is refused with ML_ESTATE, and so is reading it under such a
    plan; the slot scalars stay readable, and a refused call leaves the sums as they were.  The refusals touch no
    device memory."""
    from metalens_amd import _lib
    estate = 'error -4'
    cone = (0.3, 0.0, 0.0)
    ux_a, uy_a = np.linspace(-0.4, 0.4, 5), np.linspace(-0.3, 0.3, 4)
    ux_b, uy_b = np.linspace(-0.4, 0.4, 7), np.linspace(-0.3, 0.3, 6)
    rng = np.random.default_rng(5)
    ux_c, uy_c = rng.uniform(-0.5, 0.5, 20), rng.uniform(-0.5, 0.5, 20)
    _t, P_a = _project_row(ma, fresh, ux_a, uy_a, False)
    with pytest.raises(_lib.MetalensHipError, match=estate + '.*first call needs reset = 1'):
        _accumulate(fresh, 1.0, cone, 0, False)
    _accumulate(fresh, 1.0, cone, 0, True)
    mine = _sums(fresh, P_a.shape, 2)
    assert _bits(mine[0], P_a) and mine[1][0] > 0 and mine[1][1] == 0
    # a larger plan: neither added onto nor read
    _t, P_b = _project_row(ma, fresh, ux_b, uy_b, False)
    with pytest.raises(_lib.MetalensHipError, match=estate + '.*20 directions.*42'):
        _accumulate(fresh, 1.0, cone, 1, False)
    with pytest.raises(_lib.MetalensHipError, match=estate + '.*ml_farfield_sums.*20 directions.*42'):
        _sums(fresh, P_b.shape, 2)
    scalars = _sums(fresh, None, 2)
    assert _bits(scalars[1], mine[1]) and _bits(scalars[2], mine[2])
    # the same count as a pair list: another kind
    _t, P_c = _project_row(ma, fresh, ux_c, uy_c, True)
    assert P_c.size == P_a.size
    with pytest.raises(_lib.MetalensHipError, match=estate + '.*tensor grid.*pair list'):
        _accumulate(fresh, 1.0, cone, 1, False)
    with pytest.raises(_lib.MetalensHipError, match=estate + '.*tensor grid.*pair list'):
        _sums(fresh, P_c.shape, 2)
    # back on the plan they were started on: as they were, and the sum goes on
    _t, again = _project_row(ma, fresh, ux_a, uy_a, False)
    back = _sums(fresh, P_a.shape, 2)
    for a, b in zip(mine, back):
        assert _bits(a, b)
    _accumulate(fresh, 0.5, cone, 1, False)
    more = _sums(fresh, P_a.shape, 2)
    assert _bits(more[0], ref.p_sum([P_a, again], [1.0, 0.5], [1, 0])) and more[1][1] == more[1][0]
    # a new sum on the pair list takes the buffer over
    _t, P_c = _project_row(ma, fresh, ux_c, uy_c, True)
    _accumulate(fresh, 1.0, cone, 0, True)
    assert _bits(_sums(fresh, P_c.shape, 1)[0], P_c)
