"""The table of synthesis cases (tests/synth_cases.py) against the census: every case reaches the staging rounds and
passes it claims - with margin, by the oracle's own decisions and the rules tools/synth_staging prints from
csrc/synth_staging.h - the table as a whole reaches every branch of synth_cases.TAGS, and the rules are what the
table's lists were chosen for.  And the gap these cases close, kept on record: the suite's lens with the most rings
per patch (test_gpu_parity.py test_paper_lens_na094_windows_vs_oracle) reaches a second round of a few blocks and
nothing beyond.  No GPU."""
import math

import numpy as np
import pytest

import synth_cases
from synth_cases import CASES, MARGIN, TAGS


@pytest.fixture(scope='module')
def rules(tmp_path_factory):
    return synth_cases.staging_rules(tmp_path_factory.mktemp('staging'))


_CENSUS = {}


def census_of(name, rules):
    if name not in _CENSUS:
        case = CASES[name]
        _CENSUS[name] = synth_cases.census(synth_cases.call_args(case, synth_cases.make_lens(case.lens)), rules)
    return _CENSUS[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_case_reaches_the_branches_it_claims(rules, name):
    case = CASES[name]
    assert case.shape[0] <= 64 and case.shape[1] <= 56 and set(case.tags) <= set(TAGS)
    cen = census_of(name, rules)
    print(name, synth_cases.figures(cen))
    assert cen.family == case.family
    met = {tag: synth_cases.confirm(cen, tag) for tag in case.tags}
    short = {tag: n for tag, n in met.items() if n < MARGIN}
    assert not short, 'claimed, but met by fewer than %d patches: %s' % (MARGIN, short)
    if any(tag.endswith('multi-round-partial-patches') for tag in case.tags):
        assert case.shape[0] % 8 and case.shape[1] % 8


def test_the_table_reaches_every_branch(rules):
    confirmed = set()
    for name, case in CASES.items():
        cen = census_of(name, rules)
        confirmed |= {tag for tag in case.tags if synth_cases.confirm(cen, tag) >= MARGIN}
    assert confirmed == set(TAGS), sorted(set(TAGS) - confirmed)
    # one multi-round case per kernel also runs the three-polarisation batch
    for kernel in ('narrow', 'wide', 'general'):
        assert any(c.batch and kernel + ':multi-round-partial-patches' in c.tags for c in CASES.values()), kernel
    # the rules the lists and tags were chosen for: eight blocks per narrow round up to three slots, six with four
    assert [rules['narrow_cap_%d' % n] for n in (1, 2, 3, 4)] == [8, 8, 8, 6]
    assert [rules['narrow_pitch_%d' % n] for n in (1, 2, 3, 4)] == [17, 33, 49, 65]
    assert rules['narrow_slots_max'] == 4 and rules['wide_slots_max'] == 11 and rules['wide_cap'] == 6
    # eleven slots in rounds of 1 ... 6 blocks: 1, 1, 2, 2, 3, 3 passes; eight slots at six blocks: two full passes;
    # five: a pass of four and one of one
    assert [synth_cases.wide_passes(n, 11, rules) for n in range(1, 7)] == [1, 1, 2, 2, 3, 3]
    per6 = rules['wide_slots_per_pass_6']
    assert (synth_cases.wide_passes(6, 8, rules), 8 % per6) == (2, 0)
    assert (synth_cases.wide_passes(6, 5, rules), 5 % per6) == (2, 1)
    assert synth_cases.wide_passes(6, 10, rules) == 3
    # the general kernel: six blocks per round, orders in chunks of four - 4, 5 and 9 orders are one, two and three
    # chunks, the last of the latter two with one order
    assert (rules['general_cap'], rules['general_chunk']) == (6, 4)
    assert synth_cases.round_sizes(13, 6) == [6, 6, 1] and synth_cases.round_sizes(12, 6) == [6, 6]


def test_the_census_counts_blocks_rounds_and_passes(rules):
    """the census' arithmetic on a hand-made patch: collections 0 (wide, 11 slots), 1 (wide, 5), 2 (narrow, 3)"""
    colls, narrow_max, family = synth_cases.classify({0: synth_cases.O11, 1: synth_cases.O5, 2: synth_cases.O3,
                                                      3: synth_cases.O4_HOLE, 4: synth_cases.G5}, synth_cases.O3, rules)
    assert [colls[c].kernel for c in range(5)] == ['wide', 'wide', 'narrow', 'narrow', 'general']
    assert (colls[3].n_slots, colls[3].lo, colls[3].present) == (4, -1, 0b1001) and narrow_max == 4 and family == 'mixed'
    assert synth_cases.classify({0: synth_cases.G4}, synth_cases.G5, rules)[2] == 'general'
    assert synth_cases.classify({0: synth_cases.O3}, None, rules)[2] == 'orders-along-x'
    cen = synth_cases.Census(colls, rules['narrow_cap_%d' % narrow_max], family,
                             [synth_cases.Patch(0, 0, True, {0: 17, 1: 6, 2: 8, 4: 7}, 9, {0: frozenset([(5, 0)]), 1: frozenset([(-1, 0)]),
                                                                                   2: frozenset(), 4: frozenset()})], rules)
    work = synth_cases.patch_work(cen, cen.patches[0])
    assert work['wide'] == [(0, 17, [6, 6, 5], [3, 3, 3]), (1, 6, [6], [2])]
    assert work['narrow'] == [(2, 8, [6, 2], [1, 1])]
    assert work['general'] == [(None, 7, [6, 1], [2, 2])]
    assert synth_cases.confirm(cen, 'wide:11-slots-round-of-5') == 1 and synth_cases.confirm(cen, 'wide:third-round') == 1
    assert synth_cases.confirm(cen, 'wide:5-slots-round-of-6') == 0      # (six blocks: one fewer would not fill the round)
    assert synth_cases.confirm(cen, 'narrow:second-round-capacity-6') == 1
    assert synth_cases.confirm(cen, 'narrow:second-round-capacity-8') == 0
    assert synth_cases.confirm(cen, 'general:second-round') == 0         # (seven blocks: within the margin)
    assert synth_cases.confirm(cen, 'wide:two-collections-in-a-wave') == 1


def test_the_paper_lens_windows_stop_at_a_short_second_round(rules):
    """What these cases are for: the lens of test_paper_lens_na094_windows_vs_oracle (2 mm diameter, NA 0.94, three
    orders, tables of 5 x 5 nodes) has the most rings per patch in test_gpu_parity.py - up to 5 in its two windows, 6
    in a rim window at 45 degrees.  Its uy' axis has a node at 0, which every sector straddles, so a ring is two
    blocks: up to 10 (12) per patch against the narrow round's capacity of 8.  A second round of one to four blocks
    is all that lens reaches - no full second round, no third, nothing of the capacity of 6, and the wide and the
    general kernel's later rounds and passes not at all."""
    from test_gpu_parity import _synthetic_lens
    wl = 580e-9
    lens = _synthetic_lens(1e-3, 0.94, wl)
    pitch = wl / 2.2
    found = []
    for cx, cy in ((0.99e-3 * math.cos(0.3), 0.99e-3 * math.sin(0.3)), (-0.5e-3, 0.35e-3),
                   (0.99e-3 * math.cos(math.pi / 4), 0.99e-3 * math.sin(math.pi / 4))):
        args = dict(source_x=0.0, source_y=0.0, source_z=-lens['source_distance'], source_pol='x', wavelength=wl,
                    lens_periphery_summary=lens['lens_periphery_summary'],
                    lens_center_summary=lens['lens_center_summary'][:64], hexgridset=lens['hexgridset'],
                    x_pts=cx + (np.arange(72) - 35.5) * pitch, y_pts=cy + (np.arange(56) - 27.5) * pitch)
        cen = synth_cases.census(args, rules)
        assert cen.family == 'orders-along-x' and cen.narrow_cap == 8
        assert all(cen.colls[c].kernel == 'narrow' for p in cen.patches for c in p.blocks)
        assert all(sum(p.blocks.values()) <= 2 * p.rings for p in cen.patches)
        found.append((max(p.rings for p in cen.patches), max(n for p in cen.patches for n in p.blocks.values())))
        assert synth_cases.confirm(cen, 'narrow:third-round') == 0
        assert synth_cases.confirm(cen, 'narrow:second-round-capacity-6') == 0
    print('most rings and most blocks of a collection in a patch, per window:', found)
    assert [r for r, b in found[:2]] == [5, 5] and found[2][0] == 6
    assert max(b for r, b in found) <= 12   # a second round of at most four blocks
