"""What tests/farfield_beam_cases.py says of its rows, held without a GPU: in NumPy (which directions are NaN, the counts
inside and exactly on the edge of the exact cones, the lowest finite index) and through tools/farfield_beam_plan.cpp, which
prints the cut csrc/farfield_beam.h makes of each row's direction count (chunks, ragged last chunk, finish tiles)."""
import os
import subprocess

import numpy as np
import pytest

import farfield_beam_cases as cases
import farfield_beam_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('beam_plan')) + os.sep
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'farfield_beam_plan'])

    def run(*args):
        res = subprocess.run([out + 'farfield_beam_plan'] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and res.stderr == '', res.stdout + res.stderr
        return res.stdout
    return run


def _facts(line):
    return {k: int(v) for k, v in (kv.split('=') for kv in line.split())}


def _n(row):
    return row.ux.size if row.kind == 'pairs' else row.ux.size * row.uy.size


def _nan_mask(row):
    """where the projection leaves NaN: the reference's float64 1 - ux**2 - uy**2 is negative"""
    if row.kind == 'pairs':
        return 1 - row.ux ** 2 - row.uy ** 2 < 0
    return 1 - row.ux[:, None] ** 2 - row.uy[None, :] ** 2 < 0


def test_inventory_names_rows_that_exist():
    used = set()
    for what, rows in cases.INVENTORY.items():
        for name in (rows,) if isinstance(rows, str) else rows:
            assert name in cases.ROWS, (what, name)
            used.add(name)
    assert used == set(cases.ROWS)                       # no row without a reason
    assert {cases.ROWS[n].slot for n in cases.INVENTORY['slots 0, 1 and 4095']} == set(cases.SLOTS) == {0, 1, 4095}
    assert cases.NEVER_WRITTEN not in {r.slot for r in cases.ROWS.values()} and cases.MAX_SLOTS == ref.SLOTS
    assert set(cases.MEASURED) <= set(cases.ROWS) | {'sweep'}


def test_the_cut_of_every_row(tool):
    names = sorted(cases.ROWS)
    lines = tool(*[_n(cases.ROWS[name]) for name in names]).splitlines()
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        row, facts = cases.ROWS[name], _facts(line)
        assert facts == ref.plan(_n(row)), name
        assert facts['n'] == row.claims['n'], name
        for key in ('chunk', 'chunks', 'last', 'finish_tiles', 'last_tile'):
            if key in row.claims:
                assert facts[key] == row.claims[key], (name, key)
        # the cut covers the map: full chunks and a last one of 1 ... chunk directions; the tiles cover the chunks
        assert (facts['chunks'] - 1) * facts['chunk'] + facts['last'] == facts['n'] and 1 <= facts['last'] <= facts['chunk']
        assert (facts['finish_tiles'] - 1) * 32 + facts['last_tile'] == facts['chunks'] and 1 <= facts['last_tile'] <= 32
        assert facts['chunks'] <= ref.CHUNKS_MAX and facts['steps'] * ref.THREADS == facts['chunk']
    f = {name: ref.plan(_n(cases.ROWS[name])) for name in names}
    # what the inventory says of the loop edges
    assert f['one-chunk']['chunks'] == 1 and f['one-chunk']['last'] == 1024 and f['two-chunks']['last'] == 1024
    assert f['many-chunks']['last'] % ref.THREADS == 44 and f['many-chunks']['last'] // ref.THREADS == 1      # lanes 44 ... idle in step 1
    assert f['pairs-chunk-plus-one']['last'] == 1 and f['one-row']['n'] < ref.THREADS
    assert f['chunk-doubles']['steps'] == 8 and f['chunk-doubles']['chunks'] > ref.THREADS
    assert f['chunk-doubles']['finish_tiles'] * (ref.PARTIAL_CONE + len(cases.ROWS['chunk-doubles'].cones)) > 256   # (tile, column) tasks > lanes
    assert f['peak-last']['last'] == 276 and (f['peak-last']['n'] - 1) % ref.THREADS == 19
    # the chunk is of n alone, and doubles where 1024 chunks no longer hold the map
    assert ref.chunk_directions(1 << 20) == 1024 and ref.chunk_directions((1 << 20) + 1) == 2048
    assert ref.beam_bound_units(77100) == 3 + 6 + 3 + 31 + 2 + 1 and ref.beam_bound_units(1) == 3 + 6 + 3 + 0 + 0 + 1


def test_nan_claims():
    for name, row in cases.ROWS.items():
        nan = _nan_mask(row)
        assert nan.any() == row.claims['nan'], name
        assert nan.all() == bool(row.claims.get('none')), name
    row = cases.ROWS['sums-weight-0']
    assert int(np.argmin(_nan_mask(row).ravel())) == row.claims['first_finite'] != 0


def test_exact_cone_counts():
    """every quantity of the row is a multiple of 1/64 below 1: offsets, squares and their sums are exact, so the counts
    are those of the integers - 81 lattice points with i^2 + j^2 <= 25 (12 on the circle), 29 with <= 9 (4), 1 at 0"""
    row = cases.ROWS['exact-cone']
    assert row.cones == (5 / 64, 3 / 64, 5 / 64, 0.0) and row.centre == (1 / 64, -2 / 64)
    i, j = np.meshgrid(np.arange(-20, 21) - 1, np.arange(-24, 25) + 2, indexing='ij')
    for c, inside, edge in zip((5, 3, 5, 0), row.claims['inside'], row.claims['on_edge']):
        assert (int((i * i + j * j <= c * c).sum()), int((i * i + j * j == c * c).sum())) == (inside, edge)
        m_in, m_edge = ref.cone_masks(row.ux, row.uy, False, c / 64, row.centre)
        assert (int(m_in.sum()), int(m_edge.sum())) == (inside, edge)
    # ... and the ref's record counts them so, on any finite map
    P = np.random.default_rng(1).uniform(0.5, 1.5, (41, 49))
    want = ref.record(P, row.ux, row.uy, False, sorted(row.cones), row.centre)
    assert want['inside'] == [1, 29, 81, 81] and want['on_edge'] == [1, 4, 12, 12] and want['cone'][2] == want['cone'][3]
    assert want['cone'][0] == P[21, 22] * ref.cell_of(row.ux, row.uy, False)


def test_cones_of_the_rows_are_what_the_inventory_says():
    r = cases.ROWS['32-cones']
    assert len(r.cones) == ref.CONES_MAX == 32 and all(a > b for a, b in zip(r.cones, r.cones[1:]))
    assert all(len(row.cones) <= 32 and all(np.isfinite(c) and c >= 0 for c in row.cones) for row in cases.ROWS.values())
    assert cases.ROWS['many-chunks'].centre is None and cases.ROWS['many-chunks-centre'].centre is not None
    assert cases.ROWS['sums'].of == cases.ROWS['sums-weight-0'].of == 'sums' and cases.ROWS['sums-weight-0'].weight == 0.0


def test_ref_on_a_map_worked_by_hand():
    ux, uy = np.array([0.0, 0.25, 0.5]), np.array([-0.25, 0.0, 0.25, 0.5])
    P = np.arange(1.0, 13.0).reshape(3, 4)
    P[0, 0] = np.nan
    P[2, 3] = np.inf                                    # not finite: left out like NaN
    r = ref.record(P, ux, uy, False, [0.0, 0.25, 0.3], centre=(0.25, 0.0))
    cell = 0.0625
    assert (r['peak'], r['index'], r['finite'], r['k']) == (11.0, 10, 10, 3)
    assert r['mom'][0] == (78 - 1 - 12) * cell and r['inside'] == [1, 5, 5] and r['on_edge'] == [1, 4, 0]
    assert r['cone'] == [6 * cell, (6 + 2 + 5 + 7 + 10) * cell, (6 + 2 + 5 + 7 + 10) * cell]
    # sum t1 = cell 0.25 (-(2 + 3 + 4) + (9 + 10 + 11)), sum t3 = cell 0.0625 (9 + 30)
    assert r['mom'][1] == cell * 0.25 * 21 and r['mom'][3] == cell * 0.0625 * 39
    peak = ref.record(P, ux, uy, False, [0.25])
    assert peak['centre'] == (0.5, 0.25) and peak['inside'] == [3]          # (2, 2) itself, (1, 2), (2, 1); (2, 3) is not finite
    flat = np.full((3, 4), np.nan)
    none = ref.record(flat, ux, uy, False, [0.25])
    assert none['index'] == -1 and none['finite'] == 0 and np.isnan(none['peak']) and np.isnan(none['centre']).all() and none['cone'] == [0.0]
    flat[1, 2] = flat[2, 0] = 0.0
    assert ref.record(flat, ux, uy, False, [])['index'] == 6
    pairs = ref.record(np.array([1.0, 3.0, 3.0]), ux, ux + 0.125, True, [0.2])
    assert pairs['index'] == 1 and pairs['centre'] == (0.25, 0.375) and pairs['mom'][0] == 7.0 and pairs['inside'] == [1]
