"""The table of GEMM-path cases (tests/gemm_cases.py) against the launch rules themselves: every row's expected
kernels and split-K slabs equal what tools/transform_route prints for the row's plan facts (csrc/transform_route.h
zfold_t_chunk, zfold_eff_splits, zfold_take_wide, fold2_want_split, zgemm_tile: the functions the launchers call),
the table reaches every production instantiation the sources name, and the rules' thresholds sit where DESIGN.md and
the sources' comments say.  No GPU."""
import os
import re

import pytest

import gemm_cases
from test_transform_route import GEMM, ROOT, route  # noqa: F401  (route: the fixture that builds and runs the tool)

CSRC = os.path.join(ROOT, 'metalens_amd', 'csrc')


def _kernels(r):
    return (r['stage1_kernel'], int(r['stage1_splits']), r['stage2_kernel'], int(r['stage2_splits']),
            int(r['stage2_launches']))


@pytest.mark.parametrize('name', sorted(gemm_cases.ROWS))
def test_every_row_takes_the_kernels_it_names(route, name):
    row = gemm_cases.ROWS[name]
    for piece in gemm_cases.pieces(row):
        r = route(**gemm_cases.plan_facts(row, piece))
        assert _kernels(r) == row.expect, (name, piece)
        assert r['stage1'] == ('folded' if row.sym_y else 'generic')
        assert r['gt_direct'] == str(int(row.expect[0].endswith('out_t')))


def _production(text):
    """the source without its #ifdef ML_DIAG ... #endif blocks"""
    return re.sub(r'#ifdef ML_DIAG.*?#endif', '', text, flags=re.S)


def production_zfold():
    """the names of the zfold_kernel instantiations zfold.hip builds outside ML_DIAG: the tile shapes zfold_stage1
    hands to launch_fold_io times the I/O flavours launch_fold_io hands on"""
    text = _production(open(os.path.join(CSRC, 'zfold.hip')).read())
    shapes = set(re.findall(r'launch_fold_io<([^<>]*)>\(stream', text))
    tiles = {'32, 128, 1, 8, 1, 32, 4, double': 'wide/f64', '32, 128, 1, 8, 1, 32, 4, float': 'wide/f32',
             '32, 64, 2, 2, 2, 32, 2, double': 'narrow/f64', '32, 64, 2, 4, 1, 32, 4, float': 'narrow/f32'}
    flavours = set(re.findall(r'launch_fold<BM, BN, WM, WN, UNR, BKT, MINB, CT, (\w+), (\w+)>', text))
    ios = {('false', 'false'): 'plain', ('true', 'false'): 'in_sum', ('false', 'true'): 'out_t'}
    unknown = sorted(shapes - set(tiles)) + sorted(set(flavours) - set(ios))
    assert not unknown, 'zfold.hip builds instantiations tests/gemm_cases.py does not know: %s' % unknown
    return {'zfold/%s/%s' % (tiles[s], ios[f]) for s in shapes for f in flavours}


def production_zgemm():
    """the tile ids zgemm() launches outside ML_DIAG"""
    text = _production(open(os.path.join(CSRC, 'zgemm.hip')).read())
    body = text[text.index('switch (pick_tile'):]
    ids = re.findall(r'case (\d+): return launch<', body) + re.findall(r'default: return launch<.*// tile id (\d+)', body)
    return {'zgemm/' + i for i in ids}


def test_the_table_reaches_every_production_kernel():
    zfold, zgemm = production_zfold(), production_zgemm()
    assert zfold == set(gemm_cases.ZFOLD_KERNELS) and len(zfold) == 12
    assert zgemm == set(gemm_cases.ZGEMM_KERNELS)
    reached = gemm_cases.reached()
    missing = sorted(zfold - (reached[1] | reached[2]))
    assert not missing, 'no row of tests/gemm_cases.py runs %s' % missing
    for stage in (1, 2):
        missing = sorted(zgemm - reached[stage])
        assert not missing, 'no row of tests/gemm_cases.py runs %s in stage %d' % (missing, stage)
    # stage 1 cannot sum slabs on the way in, stage 2 never writes transposed: every flavour where it can occur
    for tile_prec in ('wide/f64', 'wide/f32', 'narrow/f64', 'narrow/f32'):
        assert {'zfold/%s/plain' % tile_prec, 'zfold/%s/out_t' % tile_prec} <= reached[1], tile_prec
        assert {'zfold/%s/plain' % tile_prec, 'zfold/%s/in_sum' % tile_prec} <= reached[2], tile_prec
    # both precisions of every folded row, an input modulation present and absent, every shard kind
    rows = gemm_cases.ROWS.values()
    assert any(r.uc0 and r.sym_x and r.sym_y for r in rows) and any(not r.uc0 and r.sym_x and r.sym_y for r in rows)
    for tile in gemm_cases.ZGEMM_KERNELS[::2]:   # 10 and 15 in stage 2: whole, row blocks, mirrored (two launches)
        kinds = {r.shard if r.shard == 'whole' else r.shard[0]: r.expect[4] for r in rows if r.expect[2] == tile}
        assert kinds == {'whole': 1, 'blocks': 1, 'mirrored': 2}, tile


def _folded1(nxl, ny, my, **more):
    return dict(method=GEMM, nx_total=nxl, nxl=nxl, ny=ny, mx=9, my=my, fold=1, fold_S=(my + 1) // 2, **more)


def test_the_wide_tile_starts_at_480_workgroups(route):
    # 4 x 3832 rows = 479 row tiles x 1 column tile, one slab (32 pairs); 3833 rows: 480
    r = route(**_folded1(3832, 64, 256))
    assert (r['want_split1'], r['stage1_kernel'], r['stage1_splits']) == ('2', 'zfold/narrow/f64/plain', '1')
    r = route(**_folded1(3833, 64, 256))
    assert (r['want_split1'], r['stage1_kernel'], r['stage1_splits']) == ('1', 'zfold/wide/f64/plain', '1')
    # 240 row tiles: a 2-way split reaches 480; 239 x 2 = 478 does not
    r = route(**_folded1(1920, 131, 200, f32=1))
    assert (r['want_split1'], r['stage1_kernel'], r['stage1_splits']) == ('2', 'zfold/wide/f32/plain', '2')
    r = route(**_folded1(1912, 131, 200, f32=1))
    assert (r['want_split1'], r['stage1_kernel'], r['stage1_splits']) == ('2', 'zfold/narrow/f32/plain', '2')


def test_slabs_are_whole_multiples_of_64_pairs(route):
    # a wanted split of 2 over T = 64 pairs is one slab of 64; over 65 it is 64 + 1
    r = route(ML_STAGE1_SPLIT=2, **_folded1(64, 128, 100))
    assert (r['want_split1'], r['stage1_splits']) == ('2', '1')
    for ny in (129, 130):
        r = route(ML_STAGE1_SPLIT=2, **_folded1(64, ny, 100))
        assert (r['want_split1'], r['stage1_splits']) == ('2', '2')
    r = route(ML_STAGE1_SPLIT=8, **_folded1(64, 2100, 100))   # 1050 pairs: chunks of 192, 6 slabs
    assert r['stage1_splits'] == '6'


def test_zgemm_tiles_change_at_256_workgroups(route):
    def stage1(nxl, my):
        return route(method=GEMM, nx_total=nxl, nxl=nxl, ny=37, mx=7, my=my)['stage1_kernel']
    assert stage1(512, 1024) == 'zgemm/15'    # 16 x 16 tiles of 128 x 64
    assert stage1(480, 1088) == 'zgemm/10'    # 15 x 17 = 255 of them; 30 x 17 of 64 x 64
    assert stage1(256, 1024) == 'zgemm/10'    # 16 x 16 tiles of 64 x 64
    assert stage1(240, 1088) == 'zgemm/11'    # 15 x 17 = 255
    assert stage1(240, 1089) == 'zgemm/10'    # 15 x 18

    def stage2(mx, my):
        return route(method=GEMM, nx_total=37, nxl=37, ny=50, mx=mx, my=my)['stage2_kernel']
    assert stage2(512, 1024) == 'zgemm/15'    # 4 x 16 x 4 fields
    assert stage2(512, 960) == 'zgemm/10'     # 4 x 15 x 4 = 240; 8 x 15 x 4 of 64 x 64
    assert stage2(256, 1024) == 'zgemm/10'    # 4 x 16 x 4 of 64 x 64
    assert stage2(256, 960) == 'zgemm/11'


def test_the_folded_stage_2_pays_from_32_tiles(route):
    sym = dict(method=GEMM, nx_total=64, nxl=64, ny=50, mx=130, fold2=1, fold2_S=65)
    r = route(my=128, **sym)   # 16 x 2 tiles of 32 rows x 64 half-directions
    assert (r['stage2'], r['stage2_kernel'], r['stage2_splits']) == ('folded', 'zfold/narrow/f64/plain', '1')
    r = route(my=120, **sym)   # 15 x 2
    assert (r['stage2'], r['stage2_kernel']) == ('generic', 'zgemm/11')
    # its wanted split: 1024 / tiles, at most 8 - 962 rows in 8 slabs of 64, 130 in 2
    r = route(my=128, **dict(sym, nx_total=1924, nxl=1924))
    assert r['stage2_splits'] == '8'
    r = route(my=1024, **dict(sym, nx_total=1924, nxl=1924, mx=1030, fold2_S=515))   # 128 x 9 tiles: no split
    assert (r['stage2_kernel'], r['stage2_splits']) == ('zfold/wide/f64/plain', '1')
