"""Which launches take the fixed-shape synthesis kernels (csrc/lens_pack.h fixed3_takes), asked of the library's own
predicate through tools/synth_fixed_route.cpp over lenses laid out by tools/lens_pack.cpp; and the census of
tests/synth_cases.py on the windows of tests/synth_fixed_cases.py: each reaches the paths test_gpu_synth_fixed.py runs it
for.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import synth_cases
import synth_fixed_cases
from synth_cases import NA, O1, O3, O4, RADIUS, SPAN_DEG, U_STEPS, Lens
from test_lens_pack import pack_lens, write_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL = 580e-9
LAUNCH = dict(n_pol=1, use_active=1, first_pass=0, plane_wave=0, premod=0)   # the listed steady-state launch of one dipole


@pytest.fixture(scope='module')
def route(tmp_path_factory):
    """route(lens, **launch facts) -> {'lens_ring', 'lens_centre', 'ring', 'centre'}; a lens is laid out once"""
    out = str(tmp_path_factory.mktemp('fixed_route')) + os.sep
    subprocess.check_call(['make', '-s', '-j2', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'lens_pack',
                           out + 'synth_fixed_route', out + 'synth_fixed_route_san'])
    packed = {}

    def pack(key, lens):
        if key not in packed:
            tables, centre, layout = pack_lens(lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'], 580)
            rec = {}
            for prefix, t in [('table%d.' % s, t) for s, t in tables.items()] + [('centre.', centre[0])]:
                for k in range(3):
                    rec[prefix + 'axis%d' % k] = t['axes'][k]
                rec[prefix + 'order_k'] = t['order_k']
                rec[prefix + 'values'] = np.ascontiguousarray(t['values']).view(np.float64)
                rec[prefix + 'bounds'] = t['bounds']
            rec['centre.periods'] = np.asarray(centre[1], np.float64)
            for name, k in (('boundaries', 'B'), ('r_center', 'r_center'), ('period', 'period'), ('lateral', 'lateral'),
                            ('ring_gc', 'ring_gc'), ('cells', 'cells')):
                rec['layout.' + k] = layout[name]
            src, dst = out + 'in%d' % len(packed), out + 'packed%d' % len(packed)
            write_records(src, rec)
            res = subprocess.run([out + 'lens_pack', src, dst], capture_output=True, text=True, timeout=300)
            assert res.returncode == 0 and res.stderr == '', res.stdout + res.stderr
            os.remove(src)
            packed[key] = dst
        return packed[key]

    def run(key, lens, **launch):
        facts = dict(LAUNCH, **launch)
        args = [str(facts[k]) for k in ('n_pol', 'use_active', 'first_pass', 'plane_wave', 'premod')]
        got = None
        for exe in ('synth_fixed_route', 'synth_fixed_route_san'):
            res = subprocess.run([out + exe, pack(key, lens)] + args, capture_output=True, text=True, timeout=60)
            assert res.returncode == 0 and res.stderr == '', (exe, res.stdout + res.stderr)
            words = {k: int(v) for k, v in (kv.split('=') for kv in res.stdout.split())}
            assert got is None or got == words
            got = words
        return got
    return run


def bench_lens():
    """bench.build_workload's lens - its parameters, three-order tables - at 80 um of diameter"""
    import bench
    return bench.build_workload(64, 16, 80e-6, 0.5, WL, 1.0)[0]


def spec_lens(spec):
    return synth_cases.make_lens(spec)


def warped_lens():
    """the three-order tables on axes that are not uniformly spaced"""
    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    return synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design, radius=20e-6,
                               numerical_aperture=0.4, wavelength=WL, switch_angle=9 * math.pi / 180, num_gratings=4,
                               num_entries=4, design_kwargs={'wavelength': WL}, axis_warp=0.2)


def test_three_order_lenses_take_the_fixed_kernels(route):
    want = {'lens_ring': 1, 'lens_centre': 1, 'ring': 1, 'centre': 1}
    assert route('bench', bench_lens()) == want
    assert route('f3', spec_lens(synth_fixed_cases.LENS_F3)) == want
    # neighbouring collections (-2, -1, 0) and (-1, 0, 1): the lowest order is a scalar of the kernel, not its shape
    assert route('f3-lo', spec_lens(synth_fixed_cases.LENS_F3_LO)) == want


def test_the_paper_lens_takes_the_fixed_kernels(route):
    """2 mm of diameter at NA 0.94 with three-order tables (test_gpu_parity.py's lens): ~1200 rings"""
    from test_gpu_parity import _synthetic_lens
    lens = _synthetic_lens(1e-3, 0.94, WL)
    # (the centre cells do not enter the predicate: a few of them keep the layout quick)
    lens = dict(lens, lens_center_summary=lens['lens_center_summary'][:64])
    assert route('paper', lens) == {'lens_ring': 1, 'lens_centre': 1, 'ring': 1, 'centre': 1}


@pytest.mark.parametrize('name, spec', [
    ('n8', synth_cases.LENS_N8),                                         # slots 3, 1, 2
    ('n6', synth_cases.LENS_N6),                                         # a four-slot collection, one with holes
    ('hole', Lens(RADIUS, NA, U_STEPS, SPAN_DEG, (O3, synth_fixed_cases.O3_HOLE), O3)),   # three slots, present = 0b101
    ('two-slot', synth_fixed_cases.LENS_ONE_TWO_SLOT),
])
def test_other_ring_tables_keep_the_general_ring_kernel(route, name, spec):
    got = route(name, spec_lens(spec))
    assert (got['lens_ring'], got['ring']) == (0, 0)
    assert (got['lens_centre'], got['centre']) == (1, 1)   # (the centre table of these lenses holds three orders)


def test_axes_that_are_not_uniform_keep_the_general_kernels(route):
    assert route('warped', warped_lens()) == {'lens_ring': 0, 'lens_centre': 0, 'ring': 0, 'centre': 0}
    # ... and the same lens on uniform axes does not
    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design, radius=20e-6,
                               numerical_aperture=0.4, wavelength=WL, switch_angle=9 * math.pi / 180, num_gratings=4,
                               num_entries=4, design_kwargs={'wavelength': WL})
    assert route('unwarped', lens) == {'lens_ring': 1, 'lens_centre': 1, 'ring': 1, 'centre': 1}


@pytest.mark.parametrize('name, centre', [('centre-1', O1), ('centre-4', O4)])
def test_a_centre_table_of_one_or_four_orders_keeps_the_general_centre_kernel(route, name, centre):
    got = route(name, spec_lens(Lens(RADIUS, NA, U_STEPS, SPAN_DEG, (O3,), centre)))
    assert (got['lens_ring'], got['ring'], got['lens_centre'], got['centre']) == (1, 1, 0, 0)


@pytest.mark.parametrize('launch', [{'n_pol': 2}, {'n_pol': 3}, {'plane_wave': 1}, {'premod': 1}, {'first_pass': 1},
                                    {'use_active': 0}], ids=lambda d: '%s=%d' % next(iter(d.items())))
def test_launches_outside_the_conditions_keep_the_general_kernels(route, launch):
    got = route('bench', bench_lens(), **launch)
    assert got == {'lens_ring': 1, 'lens_centre': 1, 'ring': 0, 'centre': 0}


# ---- the windows of the GPU test reach the paths they claim ------------------------------------------------------------
@pytest.fixture(scope='module')
def rules(tmp_path_factory):
    return synth_cases.staging_rules(tmp_path_factory.mktemp('staging'))


@pytest.mark.parametrize('name', sorted(synth_fixed_cases.CASES))
def test_every_window_reaches_the_paths_it_claims(rules, name):
    case, claims = synth_fixed_cases.CASES[name]
    assert case.shape in ((43, 37), (48, 40)) and case.pitch_div == 2.05 and case.source[:2] != (0, 0)
    args = synth_cases.call_args(case, synth_cases.make_lens(case.lens))
    cen = synth_cases.census(args, rules)
    print(name, synth_cases.figures(cen))
    assert cen.family == 'orders-along-x' and cen.narrow_cap == 8
    assert all((K.kernel, K.n_slots, K.present) == ('narrow', 3, 7) for K in cen.colls.values())
    met = {claim: synth_fixed_cases.confirm(cen, args, claim) for claim in claims}
    short = {claim: n for claim, n in met.items() if n < synth_cases.MARGIN}
    assert not short, 'claimed, but met by fewer than %d patches: %s' % (synth_cases.MARGIN, short)
    if 'narrow:multi-round-partial-patches' in claims:
        assert case.shape[0] % 8 and case.shape[1] % 8


def test_the_windows_cover_the_rounds_and_both_kinds_of_neighbours():
    claimed = set().union(*(claims for _, claims in synth_fixed_cases.CASES.values()))
    assert {'narrow:round-exactly-capacity', 'narrow:second-round-capacity-8', 'narrow:third-round',
            'narrow:two-collections-in-a-wave', 'two-collections-equal-lo', 'narrow:multi-round-partial-patches',
            'ring-and-centre'} <= claimed
