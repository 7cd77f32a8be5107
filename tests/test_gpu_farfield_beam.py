"""The beam metrics of the far field on the GPU (csrc/farfield_beam.hip behind ml_farfield_beam / ml_farfield_beams,
``FarfieldTransform.beam`` and ``SourceSweep.run(beam_cones=...)``), every row of tests/farfield_beam_cases.py against the
yardstick of tests/farfield_beam_ref.py fed the GPU's OWN downloaded map (P, or P_sum).  What each row is chosen for is the
table's claim, held without a GPU by test_farfield_beam_cases.py.  Needs an MI355X.

The bounds:

* peak, its index, the finite count, the centre and K are exact (the peak and the centre are doubles of the map and of the
  axes; NaN where the yardstick has NaN); behind K a record holds zeros.
* every sum: |record - math.fsum(terms)| <= beam_bound_units(n) 2**-53 sum |term|.  Kernel and yardstick form the terms by
  the same correctly rounded operations from the same doubles, so the terms are the same bits and membership of a cone is
  the same set; the units count the roundings of the device's fixed-order sum from the order csrc/farfield_beam.h documents
  (farfield_beam_ref.beam_bound_units), never from device output.
* against ml_farfield_sums' cone_P: the two bounds added (its own: 1 + farfield_power_ref.sum_bound_units(n)).
* the same map reduced twice, into another slot, about the peak passed explicitly, or as a source of a sweep: the same bits.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

import farfield_beam_cases as cases
import farfield_beam_ref as ref
import farfield_power_ref as power_ref
from test_gpu_parity import _record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL, N_GLASS, Z0 = cases.WL, cases.N_GLASS, cases.Z0
U = ref.U
EINVAL, ESTATE = -1, -4


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


@pytest.fixture
def fresh():
    """a context of its own: no earlier test's sums, slots or records are there"""
    from metalens_amd import _lib
    c = _lib.Context()
    c.set_method('gemm')
    try:
        yield c
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def _aperture(seed=0):
    """seeded complex fields and their axes (those of test_gpu_farfield_power_cases.py); shared, nobody writes to them"""
    nx, ny = cases.APERTURE
    rng = np.random.default_rng(1000 * nx + ny + seed)
    F = [rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny)) for _ in range(4)]
    x = (np.arange(nx) - 3.3) * (WL / 2.2)
    y = (np.arange(ny) + 11.1) * (WL / 2.3)
    for a in F + [x, y]:
        a.setflags(write=False)
    return F, x, y


def _project(ma, ctx, ux, uy, pair_list, seed=0):
    """upload the aperture, plan, transform, project -> (transform object, downloaded P)"""
    from metalens_amd import _lib
    F, x, y = _aperture(seed)
    _lib.check(ctx.lib.ml_fields_upload(ctx.handle, x.size, y.size, *[_lib.dptr(np.ascontiguousarray(f)) for f in F]))
    ctx.fields_owner = None
    t = ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux, uy, pair_list=pair_list, ctx=ctx)
    t.transform()
    return t, t.project(Z0)[0]


def _accumulate(ctx, weight, cone, slot, reset):
    from metalens_amd import _lib
    _lib.check(ctx.lib.ml_farfield_accumulate(ctx.handle, float(weight), cone[0], cone[1], cone[2], slot, int(reset)))


def _sums(ctx, shape, n_slots):
    from metalens_amd import _lib
    P_sum = np.full(shape, -1.0)
    total, cone = np.full(n_slots, -1.0), np.full(n_slots, -1.0)
    _lib.check(ctx.lib.ml_farfield_sums(ctx.handle, _lib.dptr(P_sum), _lib.dptr(total), _lib.dptr(cone), n_slots))
    return P_sum, total, cone


def _beam_rc(ctx, source, centre, cones, slot, n_cones=None):
    """ml_farfield_beam as it is -> the return code"""
    from metalens_amd import _lib
    ce = None if centre is None else np.array(centre, dtype=float)
    co = None if cones is None else np.array(cones, dtype=float)
    n = (0 if co is None else co.size) if n_cones is None else n_cones
    return ctx.lib.ml_farfield_beam(ctx.handle, source, _lib.dptr(ce), _lib.dptr(co) if co is not None and co.size else None, n, slot)


def _beam(ctx, source, centre, cones, slot):
    from metalens_amd import _lib
    _lib.check(_beam_rc(ctx, source, centre, cones, slot))


def _beams(ctx, first, n):
    from metalens_amd import _lib
    rec = np.full((n, ref.RECORD), -7.0)
    _lib.check(ctx.lib.ml_farfield_beams(ctx.handle, first, n, _lib.dptr(rec)))
    return rec


def _bits(a, b):
    """equal bit for bit (the sign of a zero included) up to which NaN it is"""
    a, b = np.ascontiguousarray(a, dtype=float), np.ascontiguousarray(b, dtype=float)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(np.signbit(a[ok]), np.signbit(b[ok]))


def _row_map(ma, ctx, row, ux=None, uy=None):
    """the row's map resident on the context -> (transform, the downloaded map the record is taken of, source)"""
    ux, uy = (row.ux, row.uy) if ux is None else (ux, uy)
    t, P = _project(ma, ctx, ux, uy, row.kind == 'pairs')
    if row.of == 'sums':
        _accumulate(ctx, row.weight, (0.0, 0.0, 0.0), 0, True)
        P = _sums(ctx, P.shape, 1)[0]
        return t, P, -1
    return t, P, 0


def _run_row(name, ma, ctx):
    row = cases.ROWS[name]
    pair = row.kind == 'pairs'
    ux, uy = row.ux, row.uy
    if name == 'peak-last':
        # a first run finds the brightest direction; it changes places with the last entry of the list
        _t, P0 = _project(ma, ctx, ux, uy, True)
        at = ref.peak_of(P0)[1]
        order = np.arange(ux.size)
        order[[at, -1]] = order[[-1, at]]
        ux, uy = np.ascontiguousarray(ux[order]), np.ascontiguousarray(uy[order])
    t, P, source = _row_map(ma, ctx, row, ux, uy)
    assert np.isnan(P).any() == row.claims['nan'] and np.isfinite(P).any() != bool(row.claims.get('none'))
    cones = np.sort(np.array(row.cones, dtype=float))
    want = ref.record(P, ux, uy, pair, cones, row.centre)
    _beam(ctx, source, row.centre, cones, row.slot)
    rec = _beams(ctx, row.slot, 1)[0]
    worst = ref.compare(rec, want, P.size)
    print('beam-case %s: n = %d, %d units, worst %.3f of the bound; peak %r at %d, %d finite' % (
        name, P.size, ref.beam_bound_units(P.size), worst, rec[ref.PEAK_P], int(rec[ref.PEAK_INDEX]), int(rec[ref.FINITE])))
    _record('farfield_beam_case', row=name, worst=worst)
    # the same bits: twice, in another slot, and about the peak's direction passed explicitly
    other = 4095 if row.slot != 4095 else 0
    _beam(ctx, source, row.centre, cones, row.slot)
    _beam(ctx, source, row.centre, cones, other)
    assert _bits(_beams(ctx, row.slot, 1)[0], rec) and _bits(_beams(ctx, other, 1)[0], rec)
    if row.centre is None and want['index'] >= 0:
        _beam(ctx, source, want['centre'], cones, other)
        assert _bits(_beams(ctx, other, 1)[0], rec)
    # the Python surface on the same map: the caller's order of the cones, and the same numbers as the NumPy restatement
    got = t.beam(row.cones, 'peak' if row.centre is None else row.centre, of='sums' if source == -1 else 'projection', slot=row.slot)
    back = np.argsort(np.argsort(np.array(row.cones), kind='stable'), kind='stable')
    assert _bits(got['cone_P'], rec[ref.CONE:ref.CONE + cones.size][back]) and got['finite'] == want['finite']
    assert _bits(got['centre_u'], want['centre']) and got['total_P'] == rec[ref.MOM]
    flat = want['index']
    assert got['peak_index'] == (flat if pair else (flat // uy.size, flat % uy.size) if flat >= 0 else (-1, -1))
    from metalens_amd import postprocess
    host = postprocess.beam_metrics(P, ux, uy, row.cones, 'peak' if row.centre is None else row.centre, pair_list=pair)
    assert host['peak_index'] == got['peak_index'] and host['finite'] == got['finite'] and _bits(host['peak_u'], got['peak_u'])
    scale = max(want['mom_abs'][0], 1e-300)
    assert abs(host['total_P'] - got['total_P']) <= (ref.beam_bound_units(P.size) + 64) * U * scale
    return row, P, rec, want


@pytest.mark.parametrize('name', sorted(cases.ROWS))
def test_rows(ma, fresh, name):
    row, P, rec, want = _run_row(name, ma, fresh)
    if name == 'exact-cone':
        back = np.argsort(np.argsort(np.array(row.cones), kind='stable'), kind='stable')
        assert tuple(np.array(want['inside'])[back]) == row.claims['inside']
        assert tuple(np.array(want['on_edge'])[back]) == row.claims['on_edge']
        # the directions ON an edge carry a share of the cone's power far above the bound: `<` cannot pass
        cell = ref.cell_of(row.ux, row.uy, False)
        edge = ref.cone_masks(row.ux, row.uy, False, 5 / 64, row.centre)[1]
        assert (P * cell)[edge].sum() > 1000 * ref.beam_bound_units(P.size) * U * want['cone_abs'][3]
        assert rec[ref.CONE + 2] == rec[ref.CONE + 3] and rec[ref.CONE] == P[21, 22] * cell      # repeated cones; the cone of 0
    if name == 'peak-last':
        assert want['index'] == P.size - 1
    if name == 'sums-weight-0':
        assert want['index'] == row.claims['first_finite'] and want['peak'] == 0.0 and not rec[ref.MOM:ref.MOM + 6].any()
        assert want['finite'] == int(np.isfinite(P).sum()) > 0
    if row.claims.get('none'):
        assert np.isnan(rec[ref.PEAK_P]) and rec[ref.PEAK_INDEX] == -1 and rec[ref.FINITE] == 0
        assert not rec[ref.MOM:ref.MOM + 6].any() and not rec[ref.CONE:].any()
        assert np.isnan(rec[ref.CENTRE:ref.CENTRE + 2]).all() == (row.centre is None)
    if name == 'many-chunks':
        # a slot never written reads zeros, the slots written hold their records
        assert not _beams(fresh, cases.NEVER_WRITTEN, 1).any()
        whole = _beams(fresh, 0, cases.MAX_SLOTS)
        assert _bits(whole[row.slot], rec) and _bits(whole[4095], rec)
        written = np.zeros(cases.MAX_SLOTS, dtype=bool)
        written[[row.slot, 4095]] = True
        assert not whole[~written].any()


def test_slots_before_any_record(fresh):
    assert not _beams(fresh, 0, cases.MAX_SLOTS).any() and not _beams(fresh, 4095, 1).any()


@pytest.mark.parametrize('name', ['many-chunks-centre', 'exact-cone'])
def test_cone_agrees_with_the_sweep_sums(ma, fresh, name):
    """cones = [c] about the sweep's cone_center: cone_P of ml_farfield_sums within the two bounds added, and the total"""
    row = cases.ROWS[name]
    c = max(row.cones)
    t, P = _project(ma, fresh, row.ux, row.uy, False)
    _accumulate(fresh, 1.0, (c,) + tuple(row.centre), 0, True)
    _P_sum, total, cone = _sums(fresh, P.shape, 1)
    _beam(fresh, 0, row.centre, [c], 1)
    rec = _beams(fresh, 1, 1)[0]
    units = ref.beam_bound_units(P.size) + 1 + power_ref.sum_bound_units(P.size)
    assert cone[0] > 0 and abs(rec[ref.CONE] - cone[0]) <= units * U * cone[0]
    assert abs(rec[ref.MOM] - total[0]) <= units * U * total[0]
    # the two membership rules are the same set
    mine = ref.cone_masks(row.ux, row.uy, False, c, row.centre)
    theirs = power_ref.cone_masks(row.ux, row.uy, False, c, row.centre)
    assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
    if name == 'exact-cone':
        assert int(mine[1].sum()) == 12


def _snapshot(ctx, t, shape, skip_slot=None):
    """everything a beam call must leave alone: P_sum and the sweep's scalars, the other record slots, the plan's
    projection and radiation vectors"""
    from metalens_amd import _lib
    as_is = np.zeros(1)      # the fixed-order sum of the resident projection as it lies there, before anything projects again
    _lib.check(ctx.lib.ml_farfield_total_power(ctx.handle, _lib.dptr(as_is)))
    P_sum, total, cone = _sums(ctx, shape, cases.MAX_SLOTS)
    recs = _beams(ctx, 0, cases.MAX_SLOTS)
    if skip_slot is not None:
        recs[skip_slot] = 0.0
    V = t.radiation_vectors()
    P = np.empty(shape)
    _lib.check(ctx.lib.ml_farfield_project(ctx.handle, Z0, _lib.dptr(P), None, None))
    return [as_is, P_sum, total, cone, recs, P] + [V[k].view(np.float64) for k in ('Nx', 'Ny', 'Lx', 'Ly')]


def test_calls_leave_everything_else_as_it_was(ma, fresh):
    """an accepted call writes its own slot and nothing else; a refused one writes nothing"""
    row = cases.ROWS['sums']
    t, P = _project(ma, fresh, row.ux, row.uy, False)
    _accumulate(fresh, 1.0, (0.4, 0.0, 0.0), 0, True)
    _accumulate(fresh, -0.5, (0.2, 0.1, 0.0), 1, False)
    _accumulate(fresh, 2.0, (0.3, 0.0, 0.1), 4095, False)
    _beam(fresh, 0, None, [0.1, 0.2], 0)
    _beam(fresh, -1, (0.0, 0.1), [0.3], 4095)
    before = _snapshot(fresh, t, P.shape)
    assert before[4][0].any() and before[4][4095].any() and not before[4][1].any()
    _beam(fresh, 0, (0.1, 0.1), [0.05, 0.5, 0.5], 7)
    _beam(fresh, -1, None, [], 7)
    after = _snapshot(fresh, t, P.shape, skip_slot=7)
    for a, b in zip(before, after):
        assert _bits(a, b)
    assert _beams(fresh, 7, 1)[0][ref.K] == 0
    before = _snapshot(fresh, t, P.shape)
    for args in ((1, None, [0.1], 7), (0, None, [0.1], 4096), (0, None, [0.2, 0.1], 7), (0, (np.nan, 0.0), [0.1], 7),
                 (-2, None, [], 7), (0, None, [-0.1], 0)):
        assert _beam_rc(fresh, *args) == EINVAL
    for a, b in zip(before, _snapshot(fresh, t, P.shape)):
        assert _bits(a, b)


def test_argument_errors_carry_the_numbers(ma, fresh):
    from metalens_amd import _lib
    row = cases.ROWS['one-column']
    _project(ma, fresh, row.ux, row.uy, False)
    err = lambda: fresh.lib.ml_last_error().decode()
    for args, said in (((1, None, [0.1], 0), 'source 1: 0 for the current projection or -1 for P_sum'),
                       ((-2, None, [0.1], 0), 'source -2'),
                       ((0, None, [0.1], -1), 'slot -1 out of range [0, 4096)'),
                       ((0, None, [0.1], 4096), 'slot 4096 out of range [0, 4096)'),
                       ((0, None, np.arange(33) * 0.01, 0), '33 cones: 0 to 32 are taken'),
                       ((0, None, [0.1, -0.2], 0), 'cones[1] = -0.2: the sine of a half-angle must be finite and >= 0'),
                       ((0, None, [np.nan], 0), 'cones[0] = nan'),
                       ((0, None, [0.1, np.inf], 0), 'cones[1] = inf'),
                       ((0, None, [0.1, 0.3, 0.2], 0), 'the cones must not decrease: cones[2] = 0.2 < cones[1] = 0.3'),
                       ((0, (0.1, np.inf), [0.1], 0), 'the centre is (0.1, inf): it must be finite'),
                       ((0, (np.nan, 0.0), [], 0), 'the centre is (nan, 0): it must be finite')):
        assert _beam_rc(fresh, *args) == EINVAL and said in err(), (args, err())
    assert _beam_rc(fresh, 0, None, None, 0, n_cones=3) == EINVAL and '3 cones asked for, cones is NULL' in err()
    assert _beam_rc(fresh, 0, None, None, 0, n_cones=-1) == EINVAL and '-1 cones' in err()
    rec = np.zeros((2, ref.RECORD))
    for first, n, said in ((-1, 1, 'first_slot -1 out of range [0, 4096)'), (4096, 0, 'first_slot 4096'), (0, -1, '-1 slots from slot 0'),
                           (4095, 2, '2 slots from slot 4095 on: the slots are [0, 4096)')):
        assert fresh.lib.ml_farfield_beams(fresh.handle, first, n, _lib.dptr(rec)) == EINVAL and said in err(), err()
    assert fresh.lib.ml_farfield_beams(fresh.handle, 0, 1, None) == EINVAL and 'records is NULL' in err()
    assert fresh.lib.ml_farfield_beams(fresh.handle, 4095, 0, None) == 0
    assert fresh.lib.ml_farfield_beam(None, 0, None, None, 0, 0) == EINVAL
    # refused calls queued nothing
    assert not _beams(fresh, 0, cases.MAX_SLOTS).any()
    # what is accepted: no cones, repeated cones, a cone of 0, 32 cones, the last slot
    for args in ((0, None, [], 0), (0, (0.0, 0.0), [0.0, 0.1, 0.1], 1), (0, None, np.linspace(0, 0.5, 32), 4095)):
        assert _beam_rc(fresh, *args) == 0
    got = _beams(fresh, 0, cases.MAX_SLOTS)
    assert got[0][ref.K] == 0 and got[1][ref.K] == 3 and got[4095][ref.K] == 32 and got[1][ref.CONE + 1] == got[1][ref.CONE + 2]


def test_state_errors(ma, fresh):
    """ML_ESTATE: nothing projected; source -1 without sums, or with sums of a plan of another direction count or kind"""
    from metalens_amd import _lib
    err = lambda: fresh.lib.ml_last_error().decode()
    assert _beam_rc(fresh, 0, None, [0.1], 0) == ESTATE and 'nothing projected: call ml_farfield_transform and ml_farfield_project first' in err()
    F, x, y = _aperture()
    _lib.check(fresh.lib.ml_fields_upload(fresh.handle, x.size, y.size, *[_lib.dptr(np.ascontiguousarray(f)) for f in F]))
    ux_a, uy_a = np.linspace(-0.4, 0.4, 5), np.linspace(-0.3, 0.3, 4)
    t = ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, N_GLASS, ux_a, uy_a, ctx=fresh)
    assert _beam_rc(fresh, 0, None, [0.1], 0) == ESTATE and 'nothing projected' in err()      # planned, not transformed
    t.transform()
    P_a = t.project(Z0)[0]
    assert _beam_rc(fresh, -1, None, [0.1], 0) == ESTATE and 'this context has no sums yet' in err()
    assert _beam_rc(fresh, 0, None, [0.1], 0) == 0
    _accumulate(fresh, 1.0, (0.3, 0.0, 0.0), 0, True)
    assert _beam_rc(fresh, -1, None, [0.1], 1) == 0
    mine = _beams(fresh, 0, 2)
    assert mine[1][ref.FINITE] == 20 and _bits(mine[0], mine[1])                 # P_sum of one map with weight 1 is the map
    # a larger plan, then the same count as a pair list
    _project(ma, fresh, np.linspace(-0.4, 0.4, 7), np.linspace(-0.3, 0.3, 6), False)
    assert _beam_rc(fresh, -1, None, [0.1], 1) == ESTATE and 'started on a plan of 20 directions (tensor grid), the active plan has 42' in err()
    rng = np.random.default_rng(5)
    _project(ma, fresh, rng.uniform(-0.5, 0.5, 20), rng.uniform(-0.5, 0.5, 20), True)
    assert _beam_rc(fresh, -1, None, [0.1], 1) == ESTATE and '(tensor grid), the active plan has 20 (pair list)' in err()
    assert _bits(_beams(fresh, 0, 2), mine)
    assert _beam_rc(fresh, 0, None, [0.1], 1) == 0                                # the projection of the active plan is fine


# ---- the sweep ---------------------------------------------------------------------------------------------------
def test_through_the_sweep(ma):
    from metalens_amd import _lib
    from test_gpu_propagate_focus import _window
    from test_gpu_propagate_sets import _common, _lens
    ctx = _lib.Context()
    try:
        lens = _lens()
        x, y = _window()
        ux, uy = np.linspace(-0.25, 0.2, 24), np.linspace(-0.2, 0.22, 21)
        sw = ma.SourceSweep(*_common(lens), x, y, ux, uy, ctx=ctx)
        f = lens['source_distance']
        sources = [(0.3e-6, -0.2e-6, -f, pol) for pol in 'xyz'] + [(-1.0e-6, 0.5e-6, -1.05 * f, 'x')]
        weights = np.array([1.0, 0.5, 2.0, 1.5])
        cones = (0.15, 0.05, 0.3)
        order = np.argsort(cones)
        plain = sw.run(sources, weights=weights, cone=0.1, keep_each=True)
        got = sw.run(sources, weights=weights, cone=0.1, keep_each=True, beam_cones=cones)
        assert set(got) == set(plain) | {'beam', 'beam_sum', 'beam_efficiency'}
        for key in plain:      # every earlier key: the same bits
            if key == 'P_each':
                assert all(_bits(a, b) for a, b in zip(got[key], plain[key]))
            else:
                assert _bits(got[key], plain[key]), key
        n = ux.size * uy.size
        raw = _beams(ctx, 0, len(sources) + 1)
        worst = 0.0
        for k in range(len(sources)):
            want = ref.record(got['P_each'][k], ux, uy, False, np.sort(cones))
            worst = max(worst, ref.compare(raw[k], want, n))
            assert _bits(got['beam']['cone_P'][k], raw[k][ref.CONE:ref.CONE + 3][np.argsort(order)])
            assert got['beam']['peak_P'][k] == want['peak'] and tuple(got['beam']['peak_index'][k]) == divmod(want['index'], uy.size)
            assert _bits(got['beam']['peak_u'][k], want['centre']) and _bits(got['beam']['centre_u'][k], want['centre'])
        want = ref.record(got['P_sum'], ux, uy, False, np.sort(cones))
        worst = max(worst, ref.compare(raw[len(sources)], want, n))
        print('beam-case sweep: worst %.3f of the bound of %d units' % (worst, ref.beam_bound_units(n)))
        _record('farfield_beam_case', row='sweep', worst=worst)
        assert got['beam_sum']['peak_index'] == divmod(want['index'], uy.size) and got['beam_sum']['total_P'] == raw[len(sources)][ref.MOM]
        assert got['beam']['cone_P'].shape == (4, 3) and _bits(got['beam_efficiency'], got['beam']['cone_P'] / got['power_in'][:, None])
        assert (got['beam']['cone_P'] > 0).all() and (got['beam']['cone_P'][:, 2] >= got['beam']['cone_P'][:, 0]).all()
        # the record's total is the sweep's total_P within the two bounds added
        units = ref.beam_bound_units(n) + 1 + power_ref.sum_bound_units(n)
        assert np.all(np.abs(got['beam']['total_P'] - got['total_P']) <= units * U * got['total_P'])
        # the centroid and the width are those of the NumPy restatement on the downloaded maps
        from metalens_amd import postprocess
        for k in range(len(sources)):
            host = postprocess.beam_metrics(got['P_each'][k], ux, uy, cones)
            assert np.allclose(host['centroid_u'], got['beam']['centroid_u'][k], rtol=0, atol=1e-12)
            assert np.allclose(host['second_moments_u'], got['beam']['second_moments_u'][k], rtol=0, atol=1e-12)
        # The record of source k is the record of ITS MAP reduced alone - it depends on neither the slot nor the sources
        # around it.  The x, y, z group run alone is synthesised as in the sweep: the same maps, so the same bits.
        group = sw.run(sources[:3], weights=weights[:3], keep_each=True, beam_cones=cones)
        for k in range(3):
            assert _bits(group['P_each'][k], got['P_each'][k]), k
            for key in got['beam']:
                assert _bits(group['beam'][key][k], got['beam'][key][k]), (k, key)
        # Every source run alone: where its map has the bits it has in the sweep the record has them too - the source at a
        # position of its own always does; a member of a polarisation group is synthesised together with the others there
        # and its map differs from the source's alone in the last bits (sweep.py, _pass: the synthesis' granularity, measured
        # here as 1 ulp of the peak), so its record alone is held against the yardstick on its own map instead
        same_map = []
        for k in range(len(sources)):
            alone = sw.run([sources[k]], keep_each=True, beam_cones=cones)
            same_map.append(_bits(alone['P_each'][0], got['P_each'][k]))
            if same_map[-1]:
                for key in got['beam']:
                    assert _bits(alone['beam'][key][0], got['beam'][key][k]), (k, key)
            ref.compare(_beams(ctx, 0, 1)[0], ref.record(alone['P_each'][0], ux, uy, False, np.sort(cones)), n)
            assert np.allclose(alone['beam']['cone_P'][0], got['beam']['cone_P'][k], rtol=1e-12, atol=0)
            assert np.allclose(alone['beam']['centroid_u'][0], got['beam']['centroid_u'][k], rtol=0, atol=1e-12)
        print('beam-case sweep: the map of a source alone has the bits of its map in the sweep for sources', same_map)
        assert same_map[3]
        # a given centre, and no cones at all
        given = sw.run(sources, weights=weights, beam_cones=(), beam_centre=(0.01, -0.02))
        assert given['beam']['cone_P'].shape == (4, 0) and given['beam_efficiency'].shape == (4, 0)
        assert _bits(given['beam']['centre_u'], np.tile([0.01, -0.02], (4, 1))) and _bits(given['beam_sum']['centre_u'], [0.01, -0.02])
        assert _bits(given['beam']['total_P'], got['beam']['total_P']) and _bits(given['P_sum'], got['P_sum'])
    finally:
        ctx.close()


# ---- the example -------------------------------------------------------------------------------------------------
def test_beam_steering_example():
    spec = importlib.util.spec_from_file_location('beam_steering', os.path.join(ROOT, 'examples', 'beam_steering.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(radius=30e-6, positions=3, verbose=False)
    assert out['pointing'].shape == (3, 2) and out['rms_divergence'].shape == (3,) and out['cone_fraction'].shape == (3, 2)
    # A collimator: an emitter dx off the axis in the focal plane sends its beam to the other side, at sin(theta) = dx / f
    # in air by the paraxial estimate, dx / (f n_glass) in the glass the direction cosines are taken in.  The direction
    # grid has a step of du, the design is not paraxial (NA 0.5) and the centroid is taken over a window that holds the
    # uncollimated light too, so: the on-axis peak lies within a step of the axis; each step of the emitter moves the
    # peak to -ux by 0.5 ... 1.5 of the estimate (a step of the grid allowed on either side); the centroid follows in
    # the same order; nothing is steered along y beyond two steps of the grid
    du, est = out['du'], out['offset'] / (out['f'] * out['n_glass'])
    assert est[1] > 4 * du                                                  # (the steps are resolved by the grid)
    assert np.all(np.abs(out['peak_u'][0]) <= du * (1 + 1e-9))
    for k in (1, 2):
        assert -1.5 * est[k] - du <= out['peak_u'][k, 0] <= -0.5 * est[k] + du, (k, out['peak_u'][k], est[k])
    assert out['peak_u'][2, 0] < out['peak_u'][1, 0] < out['peak_u'][0, 0] + du
    assert out['pointing'][2, 0] < out['pointing'][1, 0] < out['pointing'][0, 0] and out['pointing'][1, 0] < 0
    assert np.all(np.abs(out['pointing'][:, 1]) < 2 * du) and np.all(np.abs(out['peak_u'][:, 1]) <= du * (1 + 1e-9))
    assert np.all(out['rms_divergence'] > 0) and np.all(out['rms_divergence'] < 0.16 * np.sqrt(2))      # inside the window
    assert np.all(out['cone_fraction'][:, 1] >= out['cone_fraction'][:, 0]) and np.all(out['cone_fraction'] > 0)
    assert np.all(out['cone_fraction'] <= 1.0 + 1e-12)                      # no more than the incident power
