"""What the near-field kernels read about a lens, as metalens_amd/csrc/lens_pack.h lays it out on the host: run by
tools/lens_pack.cpp over the arrays packing.pack_table / pack_layout produce and compared with a NumPy restatement of
the layouts documented in lens_pack.h and DESIGN.md 3 - exactly, wherever the layout is a permutation, a zero fill or
the one expression lo * (1 - t) + hi * t.  No GPU.

Not covered: the size limits (ring tables beyond 2^31 block units or 2^40 elements, a table too large for the 24-bit
cell arithmetic) - reaching them needs tables of hundreds of megabytes."""
import math
import os
import subprocess

import numpy as np
import pytest

import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SLOTS, MAX_ORDERS, PACKED_AXIS, UNIT, MAX_SLOTS_SIMPLE, NARROW, GROUP = 32, 32, 8, 16, 11, 4, 20
TYPES = {'f8': np.float64, 'i4': np.int32, 'u1': np.uint8}
ML_EINVAL, ML_ESTATE = -1, -4     # include/metalens_hip.h

# the records of lens_pack.h, field by field
TABLE_DESC = np.dtype([('pointers', '<u8', 4), ('n', '<i4', 4), ('bounds', '<f8', 6), ('center_kx', '<f8', MAX_ORDERS),
                       ('center_ky', '<f8', MAX_ORDERS), ('center_ox', '<i4', MAX_ORDERS), ('center_oy', '<i4', MAX_ORDERS),
                       ('center_g', '<f8', 2), ('packed', '<i4'), ('uniform', '<i4'), ('uni_ax', '<f8', 6),
                       ('ax0', '<f8', PACKED_AXIS), ('inv0', '<f8', PACKED_AXIS), ('ax1', '<f8', PACKED_AXIS),
                       ('inv1', '<f8', PACKED_AXIS)])
COLL_DESC = np.dtype([('uni_ax', '<f8', 6), ('n0', '<i4'), ('n1', '<i4'), ('n_orders', '<i4'), ('flags', '<i4'),
                      ('lim0', '<f8'), ('lim1', '<f8'), ('n_slots', '<i4'), ('ox_lo', '<i4'), ('present', '<i4'),
                      ('pad', '<i4')])
RING_BUCKET = np.dtype([('bm1', '<f8'), ('b0', '<f8'), ('b1', '<f8'), ('first', '<i4'), ('pad', '<i4')])
CELL_REC = np.dtype([('x', '<f8'), ('y', '<f8'), ('which', '<i4'), ('index', '<i4'), ('pad', '<f8')])


def write_records(path, records):
    with open(path, 'wb') as f:
        for name, a in records.items():
            a = np.ascontiguousarray(a)
            kind = {v: k for k, v in TYPES.items()}[a.dtype.type]
            f.write(('%s %s %d\n' % (name, kind, a.size)).encode() + a.tobytes() + b'\n')


def read_records(path):
    out, blob, at = {}, open(path, 'rb').read(), 0
    while at < len(blob):
        end = blob.index(b'\n', at)
        name, kind, count = blob[at:end].decode().split()
        out[name] = np.frombuffer(blob, TYPES[kind], int(count), end + 1)
        at = end + 1 + out[name].nbytes + 1
    return out


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('lens_pack')) + os.sep
    subprocess.check_call(['make', '-s', '-j2', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'lens_pack',
                           out + 'lens_pack_san'])
    count = [0]

    def run(tables, centre, layout, exe='lens_pack', **knobs):
        """tables: {slot: pack_table dict}, centre: (pack_table dict, periods) or None, layout: pack_layout dict"""
        rec = {}
        for prefix, t in [('table%d.' % s, t) for s, t in tables.items()] + ([('centre.', centre[0])] if centre else []):
            for k in range(3):
                rec[prefix + 'axis%d' % k] = t['axes'][k]
            rec[prefix + 'orders'] = np.asarray(t['orders'], np.int32)
            rec[prefix + 'order_k'] = t['order_k']
            rec[prefix + 'values'] = np.ascontiguousarray(t['values']).view(np.float64)
            rec[prefix + 'bounds'] = t['bounds']
        if centre:
            rec['centre.periods'] = np.asarray(centre[1], np.float64)
        for key, name in (('boundaries', 'B'), ('r_center', 'r_center'), ('period', 'period'), ('dphi', 'dphi'),
                          ('lateral', 'lateral'), ('ring_gc', 'ring_gc'), ('cells', 'cells'), ('rot_table', 'rot_table'),
                          ('tie_table', 'tie_table'), ('rot_center', 'rot_center'), ('rot_half', 'rot_half')):
            if key in layout:
                rec['layout.' + name] = layout[key]
        for name, v in knobs.items():
            rec[name] = np.array([v], np.int32)
        count[0] += 1
        src, dst = out + 'in%d' % count[0], out + 'out%d' % count[0]
        write_records(src, rec)
        res = subprocess.run([out + exe, src, dst], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and res.stderr == '', res.stdout + res.stderr
        got = read_records(dst)
        os.remove(src)
        os.remove(dst)
        return got
    return run


# ---- inputs --------------------------------------------------------------------------------
def pack_lens(periphery, cells, hgs, wavelength_in_nm):
    from metalens_amd import packing
    tables = {s: packing.pack_table(gc, wavelength_in_nm) for s, gc in enumerate(periphery['gratingcollection_list'])}
    g0 = hgs.grating_list[0]
    centre = (packing.pack_table(hgs, wavelength_in_nm), (g0.grating_period, g0.lateral_period))
    return tables, centre, packing.pack_layout(periphery, cells)


def golden_lens(name):
    periphery, cells, hgs = golden_io.load_lens(golden_io.golden_path('lens%s.npz' % name))
    return pack_lens(periphery, cells, hgs, sorted(hgs.interpolators)[0][0])


SIMPLE3 = ((0, 0), (-1, 0), (1, 0))
SYNTHETIC = {   # the order sets of test_gpu_parity.py: ORDER_LISTS and test_general_order_sets_vs_oracle
    'physical': ('physical', 'physical'),
    'inside-outside': ((((-3, 0), (-2, 0), (-1, 0), (0, 0), (1, 0)), ((-2, 0), (-1, 0), (0, 0))), ((0, 0),)),
    'holes': ((((-1, 0), (2, 0), (-4, 0)), ((1, 0), (2, 0), (3, 0), (5, 0))), ((-1, 0), (1, 0))),
    'one-order': ((((-5, 0),), ((0, 0), (-1, 0), (1, 0), (-2, 0), (2, 0), (-3, 0), (3, 0), (-4, 0), (4, 0), (-5, 0), (5, 0))),
                  ((0, 0), (-2, 0), (2, 0), (-3, 0))),
    'general-rings': (((0, 0), (-1, 0), (1, 0), (0, 1), (-2, 0)), SIMPLE3),
    'general-centre': (SIMPLE3, ((0, 0), (-1, 0), (1, 0), (0, -1), (1, 1))),
    'both-general': (((0, 0), (-1, 1), (2, -1)), ((0, 0), (0, 1), (-1, -1), (2, 0))),
    'narrow-general-wide': ((SIMPLE3, ((0, 0), (-1, 0), (0, 1)), ((-2, 0), (-1, 0), (0, 0), (1, 0), (2, 0))), SIMPLE3),
    'no-narrow-general-centre': ((((0, 0), (-1, 0), (0, 1)), ((-2, 0), (-1, 0), (0, 0), (1, 0), (2, 0))), ((0, 0), (1, 1))),
}


def synthetic_lens(which):
    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    wl = 580e-9
    per, cen = SYNTHETIC[which]
    more = {}
    if which in ('narrow-general-wide', 'no-narrow-general-centre'):   # three ring collections instead of two
        more['max_collection_span'] = 5 * math.pi / 180
    elif which in ('general-rings', 'general-centre', 'both-general'):
        more['max_collection_span'] = 9 * math.pi / 180
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design, radius=40e-6,
                               numerical_aperture=0.4, wavelength=wl, switch_angle=9 * math.pi / 180, num_gratings=20,
                               num_entries=12, design_kwargs={'wavelength': wl}, periphery_orders=per, center_orders=cen,
                               **more)
    return pack_lens(lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset'], 580)


LENSES = ['A', 'B', 'C', 'D'] + sorted(SYNTHETIC)
_cache = {}


def lens_and_result(tool, name):
    if name not in _cache:
        inputs = golden_lens(name) if len(name) == 1 else synthetic_lens(name)
        _cache[name] = (inputs, tool(*inputs))
    return _cache[name]


def small_table(orders, n0=5, n1=5, n2=4, seed=0, periods=(1.0, 3.0), axis0=None, axis1=None):
    """a hand-made table over the period range `periods`; orders are kept in the order given"""
    rng = np.random.default_rng(seed)
    axes = [np.linspace(-0.5, 0.4, n0) if axis0 is None else np.asarray(axis0, float),
            np.linspace(-0.3, 0.6, n1) if axis1 is None else np.asarray(axis1, float), np.linspace(*periods, n2)]
    shape = (len(orders), axes[0].size, axes[1].size, n2, 4)
    return {'axes': axes, 'orders': np.array(orders, np.int32).reshape(-1, 2),
            'order_k': np.array([[ox * 2 * math.pi, oy * 2 * math.pi] for ox, oy in orders]),
            'values': rng.standard_normal(shape) + 1j * rng.standard_normal(shape),
            'bounds': np.array([-0.5, 0.4, -0.3, 0.6, periods[0], periods[1]])}


def small_layout(ring_gc, periods, cells=None, boundaries=None):
    n = len(ring_gc)
    B = np.arange(1.0, n + 2) if boundaries is None else np.asarray(boundaries, float)
    return {'boundaries': B, 'r_center': 0.5 * (B[:-1] + B[1:]), 'period': np.asarray(periods, float),
            'lateral': np.linspace(0.7, 0.9, n), 'ring_gc': np.asarray(ring_gc, np.int32),
            'cells': np.zeros((0, 3)) if cells is None else np.asarray(cells, float)}


# ---- the documented layouts, restated ------------------------------------------------------
def order_numbers(t):
    return np.rint(t['order_k'] / (2 * math.pi)).astype(int)


def simple_set(t):
    """(lowest ox, slots, present bits, slot -> index in the table's list or -1), None if the order set is not simple:
    orders (ox, 0) with |ox| <= 5, each once, listed ascending"""
    o = order_numbers(t)
    if np.any(o[:, 1] != 0) or np.any(np.abs(o[:, 0]) > 5) or np.any(np.diff(o[:, 0]) <= 0):
        return None
    lo, n = int(o[0, 0]), int(o[-1, 0] - o[0, 0] + 1)
    idx = np.full(n, -1)
    idx[o[:, 0] - lo] = np.arange(len(o))
    return lo, n, int(sum(1 << int(s) for s in o[:, 0] - lo)), idx


def at_period(t, period):
    """the table with its period axis interpolated at `period` (scipy's find_indices location): float [O][n0][n1][4][2]"""
    ax = t['axes'][2]
    i = int(np.clip(np.searchsorted(ax, period, 'right') - 1, 0, ax.size - 2))
    w = (period - ax[i]) / (ax[i + 1] - ax[i])
    v = np.ascontiguousarray(t['values']).view(np.float64).reshape(t['values'].shape + (2,))
    return v[:, :, :, i] * (1 - w) + v[:, :, :, i + 1] * w


def cell_blocks(v, idx):
    """[order][n0][n1][...] -> [i0][i1][slot][node 2 x 2][...] with zeros in the slots of no order"""
    n0, n1 = v.shape[1:3]
    out = np.zeros((n0 - 1, n1 - 1, len(idx), 4) + v.shape[3:])
    for s, o in enumerate(idx):
        for nd in range(4):
            if o >= 0:
                out[:, :, s, nd] = v[o, (nd >> 1):n0 - 1 + (nd >> 1), (nd & 1):n1 - 1 + (nd & 1)]
    return out


def check_uniform(axis, got3):
    step = (axis[-1] - axis[0]) / (axis.size - 1)
    assert np.array_equal(got3, [axis[0], step, 1.0 / step])


def check_lens(inputs, got, force_general=0, force_general_coll=0):
    tables, centre, L = inputs
    ring_gc, period = L['ring_gc'], L['period']
    n_rings = ring_gc.size
    # dense numbering in slot order
    slots = np.unique(ring_gc)
    assert got['n_colls'][0] == slots.size and np.array_equal(got['coll_slot'], slots)
    ring_coll = np.searchsorted(slots, ring_gc)
    assert np.array_equal(got['ring_coll'], ring_coll)
    # who is simple, and the masks
    sets = [None if force_general or (force_general_coll >> c) & 1 else simple_set(tables[s]) for c, s in enumerate(slots)]
    cset = None if not centre or force_general or (force_general_coll >> 16) & 1 else simple_set(centre[0])
    simple = any(s is not None for s in sets) or cset is not None
    bits = lambda which: sum(1 << c for c in range(slots.size) if which(sets[c]))
    assert got['simple_orders'][0] == simple
    assert got['general_mask'][0] == (bits(lambda s: s is None) if simple else 0)
    assert got['centre_general'][0] == (1 if simple and centre and cset is None else 0)
    assert got['narrow_mask'][0] == bits(lambda s: s is not None and s[1] <= NARROW)
    assert got['wide_mask'][0] == bits(lambda s: s is not None and s[1] > NARROW)
    assert got['narrow_exists'][0] == (got['narrow_mask'][0] != 0)
    assert got['narrow_slots_max'][0] == max([1] + [s[1] for s in sets if s is not None and s[1] <= NARROW])
    # table descriptors
    desc = got['table_desc'].view(TABLE_DESC)
    assert desc.size == MAX_SLOTS + 1 and not desc['pointers'].any()
    for s in range(MAX_SLOTS + 1):
        t = centre[0] if s == MAX_SLOTS and centre else tables.get(s)
        d = desc[s]
        if t is None:
            assert not d.tobytes().strip(b'\0')
            continue
        a0, a1 = t['axes'][:2]
        assert list(d['n']) == [a0.size, a1.size, t['axes'][2].size, len(t['order_k'])]
        assert np.array_equal(d['bounds'], t['bounds'], equal_nan=True)
        assert d['packed'] == (0 if max(a0.size, a1.size) > PACKED_AXIS else 1 if max(a0.size, a1.size) <= 5 else 2)
        for ax, node, inv in ((a0, 'ax0', 'inv0'), (a1, 'ax1', 'inv1')):
            if d['packed']:
                assert np.array_equal(d[node][:ax.size - 1], ax[:-1]) and np.all(d[node][ax.size - 1:] == np.inf)
                assert np.array_equal(d[inv][:ax.size - 1], 1.0 / (ax[1:] - ax[:-1])) and not d[inv][ax.size - 1:].any()
            else:
                assert not d[node].any() and not d[inv].any()
        uniform = all(np.abs(ax - np.linspace(ax[0], ax[-1], ax.size)).max() <= 1e-14 * np.abs(ax).max() for ax in (a0, a1))
        assert d['uniform'] == uniform
        if uniform:
            check_uniform(a0, d['uni_ax'][:3])
            check_uniform(a1, d['uni_ax'][3:])
        if s == MAX_SLOTS:
            k, n = t['order_k'], len(t['order_k'])
            assert np.array_equal(d['center_kx'][:n], k[:, 0] / centre[1][0]) and not d['center_kx'][n:].any()
            assert np.array_equal(d['center_ky'][:n], k[:, 1] / centre[1][1]) and not d['center_ky'][n:].any()
            assert np.array_equal(d['center_ox'][:n], order_numbers(t)[:, 0]) and np.array_equal(d['center_oy'][:n], order_numbers(t)[:, 1])
            assert np.array_equal(d['center_g'], [2 * math.pi / centre[1][0], 2 * math.pi / centre[1][1]])
        else:
            assert not d['center_kx'].any() and not d['center_g'].any() and not d['center_ox'].any()
    # collection descriptors and the intersection of the bounds
    coll = got['coll'].view(COLL_DESC)
    assert coll.size == slots.size
    lo_hi = [-np.inf, np.inf, -np.inf, np.inf]
    for c, s in enumerate(slots):
        t, C, d = tables[s], coll[c], desc[s]
        assert (C['n0'], C['n1'], C['n_orders']) == (t['axes'][0].size, t['axes'][1].size, len(t['order_k']))
        assert C['flags'] == d['uniform'] and (C['lim0'], C['lim1'], C['pad']) == (C['n0'] - 2, C['n1'] - 2, 0)
        if C['flags']:
            assert np.array_equal(C['uni_ax'], d['uni_ax'])
        assert (C['ox_lo'], C['n_slots'], C['present']) == (sets[c][:3] if sets[c] else (0, 0, 0))
        for k in range(4):
            b = t['bounds'][k]
            lo_hi[k] = (max, min)[k & 1](lo_hi[k], b) if b == b else (np.inf, -np.inf)[k & 1]
    assert np.array_equal(got['ring_bounds_all'], lo_hi)
    # per-ring tables, ring by ring at the offsets the records name; nothing else in the array
    rec = got['ring_rec'].reshape(n_rings, 4)
    assert np.array_equal(rec[:, 0], L['r_center']) and np.array_equal(rec[:, 1], period)
    assert np.array_equal(rec[:, 2], 2 * math.pi / period)
    word = np.ascontiguousarray(rec[:, 3]).view(np.int64)
    tab = got['ring_tab'].reshape(-1, 2)
    seen = np.zeros(len(tab), bool)
    at = ok_at = 0   # complex elements of ring_tab, doubles of ring_ok before this ring
    for r in range(n_rings):
        t, s = tables[ring_gc[r]], sets[ring_coll[r]]
        outside = period[r] < t['bounds'][4] or period[r] > t['bounds'][5]
        v = at_period(t, period[r])
        if s:
            want = cell_blocks(v, s[3]).reshape(-1, 2)
            at = -(-at // UNIT) * UNIT   # units of 16 complex
            assert word[r] & 0xffffffff == at // UNIT and word[r] >> 32 == outside
        else:
            want = v.reshape(-1, 2)
            assert word[r] & ((1 << 40) - 1) == at and word[r] >> 40 == outside
        assert np.array_equal(tab[at:at + len(want)], want), r
        seen[at:at + len(want)] = True
        at += len(want)
        # order wavenumbers of the ring
        assert got['ring_ok_off'][r] == ok_at
        ok = got['ring_ok'][ok_at:ok_at + 4 * len(t['order_k'])].reshape(-1, 4)
        assert np.array_equal(ok[:, 0], t['order_k'][:, 0] / period[r])
        assert np.array_equal(ok[:, 1], t['order_k'][:, 1] / L['lateral'][r])
        assert np.array_equal(ok[:, 2:], order_numbers(t))
        ok_at += ok.size
    assert got['ring_ok'].size == ok_at
    # the tail: a largest block and one unit of zeros behind the tables of a lens with simple collections
    assert len(tab) == at + ((MAX_SLOTS_SIMPLE + 1) * UNIT if simple else 0)
    assert not tab[~seen].any()
    # centre table
    if centre:
        v = centre[0]['values']
        v = np.ascontiguousarray(v).view(np.float64).reshape(v.shape + (2,))   # [O][n0][n1][K][4][2]
        K = v.shape[3]
        assert (got['center_lo'][0], got['center_n_slots'][0], got['center_present_mask'][0]) == (cset[:3] if cset else (0, 0, 0))
        if cset:
            groups = -(-K // GROUP)
            padded = np.zeros(v.shape[:3] + (groups * GROUP, 4, 2))   # types past K: zeros
            padded[:, :, :, :K] = v
            # [i0][i1][slot][node][group][20][4][2] -> [slot][i0][i1][group][node][amplitude 4][20][2]
            blocks = cell_blocks(padded.reshape(v.shape[:3] + (groups, GROUP, 4, 2)), cset[3])
            want = blocks.transpose(2, 0, 1, 4, 3, 6, 5, 7)
        else:
            want = v.transpose(0, 1, 2, 4, 3, 5)   # [O][n0][n1][4][K]
        assert np.array_equal(got['center_qmajor'], want.reshape(-1))
    else:
        assert 'center_qmajor' not in got and got['center_n_slots'][0] == 0
    return sets, cset


# ---- lenses --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', LENSES)
def test_lens_layout(tool, name):
    inputs, got = lens_and_result(tool, name)
    sets, cset = check_lens(inputs, got)
    kinds = ['general' if s is None else 'narrow' if s[1] <= NARROW else 'wide' for s in sets]
    want = {'A': ['narrow'] * 2, 'B': ['narrow'] * 3, 'C': ['wide'] * 2, 'D': ['wide', 'narrow'],
            'narrow-general-wide': ['narrow', 'general', 'wide', 'narrow'], 'both-general': ['general'] * 2,
            'no-narrow-general-centre': ['general', 'wide', 'general', 'wide'], 'general-rings': ['general'] * 2,
            'one-order': ['narrow', 'wide'], 'holes': ['wide', 'wide']}
    if name in want:   # the cases are what their names say
        assert kinds == want[name], kinds
    assert (cset is None) == (name in ('general-centre', 'both-general', 'no-narrow-general-centre'))
    if name == 'holes':
        assert [s[2] for s in sets] == [0b1001001, 0b10111] and cset[2] == 0b101
    if name == 'D':   # K = 8 is no multiple of 20: twelve zero types behind every amplitude's eight
        cq = got['center_qmajor'].reshape(-1, 16, GROUP, 2)
        assert cq[:, :, :8].any() and not cq[:, :, 8:].any()


def test_forced_general(tool):
    inputs, _ = lens_and_result(tool, 'D')
    for knobs in (dict(force_general=1), dict(force_general_coll=2), dict(force_general_coll=1 << 16)):
        got = tool(*inputs, **knobs)
        sets, cset = check_lens(inputs, got, **knobs)
        general = [s is None for s in sets] + [cset is None]
        assert general == {'force_general': [True] * 3, 2: [False, True, False], 1 << 16: [False, False, True]}[
            knobs.get('force_general_coll', 'force_general')]
    assert got['simple_orders'][0] == 1 and got['centre_general'][0] == 1


def test_small_tables(tool):
    """axes that are not uniform, too long to go inline, inline in the longer form; periods outside the table's range
    under both kinds of record; a NaN bound; order lists the restricted kernels do not take"""
    bent = small_table([(-1, 0), (0, 0), (1, 0)], axis0=[-0.5, -0.2, 0.0, 0.3, 0.4], seed=1)
    long9 = small_table([(0, 0), (1, 0)], n0=9, n1=3, seed=2)
    six_five = small_table([(0, 0), (0, 1)], n0=6, n1=5, seed=3)            # general: an order oy = 1
    descending = small_table([(1, 0), (0, 0), (-1, 0)], seed=4)
    twice = small_table([(0, 0), (1, 0), (1, 0)], seed=5)
    nan_bound = small_table([(0, 0)], seed=6)
    nan_bound['bounds'][2] = np.nan
    tables = {0: bent, 3: long9, 4: six_five, 7: descending, 8: twice, 9: nan_bound}
    centre = (small_table([(0, 0), (1, 0)], n2=23, seed=7), (2.0, 2.5))     # 23 cell types: a full group and three
    # rings below, inside and above the period range [1, 3] of a simple and of a general table
    ring_gc = [0, 0, 0, 4, 4, 4, 3, 7, 8, 9]
    layout = small_layout(ring_gc, [0.9, 1.0, 3.5, 0.5, 2.2, 3.0000001, 2.0, 1.5, 2.5, 1.7])
    got = tool(tables, centre, layout)
    sets, cset = check_lens((tables, centre, layout), got)
    assert [s is None for s in sets] == [False, False, True, True, True, False]
    desc = got['table_desc'].view(TABLE_DESC)
    assert [int(desc[s]['uniform']) for s in (0, 3, 4)] == [0, 1, 1]
    assert [int(desc[s]['packed']) for s in (0, 3, 4)] == [1, 0, 2]
    word = np.ascontiguousarray(got['ring_rec'].reshape(-1, 4)[:, 3]).view(np.int64)
    assert [int(w >> 32) for w in word[:3]] == [1, 0, 1] and [int(w >> 40) for w in word[3:6]] == [1, 0, 1]
    assert list(got['ring_bounds_all']) == [-0.5, 0.4, np.inf, 0.6]         # the empty range along uy'


# ---- ring search ---------------------------------------------------------------------------
def boundaries_below(B, got, r):
    """nearfield_geometry.hip boundaries_below_fast: the bucket record where it settles the search, else the walk from the
    uniform table's entry"""
    n_rings = B.size - 1
    if r > got['r_outer'][0]:
        return n_rings + 1, 'outside'
    q = got['ring_lutrec'].view(RING_BUCKET)[min(max(int(r * got['lutrec_inv_h'][0]), 0), got['lutrec_buckets'][0] - 1)]
    if q['bm1'] < r and not q['b1'] < r:
        return int(q['first']) + int(q['b0'] < r), 'record'
    idx = int(got['ring_lut'][min(max(int(r * got['lut_inv_h'][0]), 0), got['lut_buckets'][0] - 1)])
    start = idx
    while idx <= n_rings and B[idx] < r:
        idx += 1
    while idx > 0 and B[idx - 1] >= r:
        idx -= 1
    return idx, abs(idx - start)


@pytest.mark.parametrize('name', ['A', 'D', 'zero-width'])
def test_ring_search(tool, name):
    if name == 'zero-width':   # two rings, the first of no width
        layout = small_layout([0, 0], [2.0, 2.0], boundaries=[0.25, 0.25, 1.0])
        got = tool({0: small_table([(0, 0)])}, None, layout)
        B = layout['boundaries']
    else:
        inputs, got = lens_and_result(tool, name)
        B = inputs[2]['boundaries']
    assert (got['r_outer'][0], got['r_centre'][0], got['lut_buckets'][0]) == (B[-1], B[0], 16384)
    # the tables themselves: boundaries strictly below each bucket's lower edge, and the boundaries around it
    h = B[-1] / 16384
    assert got['lut_inv_h'][0] == 1.0 / h
    assert np.array_equal(got['ring_lut'], np.searchsorted(B, np.arange(16384) * h, 'left'))
    rec = got['ring_lutrec'].view(RING_BUCKET)
    nb = got['lutrec_buckets'][0]
    assert rec.size == nb and 1024 <= nb <= 65536 and got['lutrec_inv_h'][0] == 1.0 / (B[-1] / nb) and not rec['pad'].any()
    assert np.array_equal(rec['first'], np.searchsorted(B, np.arange(nb) * (B[-1] / nb), 'left'))
    ext = np.concatenate(([-np.inf], B, [np.inf, np.inf]))
    for k, field in enumerate(('bm1', 'b0', 'b1')):
        assert np.array_equal(rec[field], ext[rec['first'] + k])
    # the search: random radii and radii on the boundaries, one ulp below and above them
    rng = np.random.default_rng(5)
    radii = np.concatenate((rng.uniform(0, 1.05 * B[-1], 2000), B, np.nextafter(B, 0), np.nextafter(B, np.inf), [0.0]))
    how = [boundaries_below(B, got, r) for r in radii]
    assert np.array_equal([h_[0] for h_ in how], np.searchsorted(B, radii, 'left'))
    assert sum(h_[1] == 'record' for h_ in how) > 1500     # the one-load answer is the usual one
    assert max([h_[1] for h_ in how if isinstance(h_[1], int)], default=0) <= 2


# ---- centre cells --------------------------------------------------------------------------
def check_bins(cells, got):
    n = len(cells)
    bx, by, h = got['bins_x'][0], got['bins_y'][0], got['bin_h'][0]
    x0, y0 = got['bin_x0'][0], got['bin_y0'][0]
    assert (x0, y0) == (cells[:, 0].min(), cells[:, 1].min())
    index, start = got['cell_index'], got['bin_start']
    assert np.array_equal(np.sort(index), np.arange(n))                       # a permutation of the cells
    assert np.array_equal(got['cell_x'], cells[index, 0]) and np.array_equal(got['cell_y'], cells[index, 1])
    assert np.array_equal(got['cell_xy'].reshape(n, 2), cells[index, :2])
    assert np.array_equal(got['cell_which'], cells[index, 2].astype(np.int32))
    assert np.array_equal(got['slot_of_cell'][index], np.arange(n))           # slot_of_cell inverts index
    # every cell in the bin its coordinates name, the bins in order, the original order kept within a bin
    bin_of = (np.clip(np.floor((cells[:, 0] - x0) / h), 0, bx - 1) * by + np.clip(np.floor((cells[:, 1] - y0) / h), 0, by - 1)).astype(int)
    assert start.size == bx * by + 1 and start[0] == 0
    assert np.array_equal(start[1:], np.cumsum(np.bincount(bin_of, minlength=bx * by)))   # a prefix sum
    assert np.array_equal(index, np.argsort(bin_of, kind='stable'))
    assert (bx - 1) * h <= np.ptp(cells[:, 0]) < bx * h and (by - 1) * h <= np.ptp(cells[:, 1]) < by * h


def hex_cells(n_side=6, pitch=0.4e-6):
    a, b = np.meshgrid(np.arange(n_side), np.arange(n_side), indexing='ij')
    x = pitch * (a + 0.5 * b).ravel() - 1e-6
    y = pitch * (math.sqrt(3) / 2 * b).ravel() + 0.3e-6
    order = np.random.default_rng(3).permutation(x.size)
    return np.column_stack((x, y, np.arange(x.size) % 7))[order]


def run_cells(tool, cells, **more):
    layout = small_layout([0], [2.0], cells=cells)
    return tool({0: small_table([(0, 0)])}, (small_table([(0, 0)], n2=8), (2.0, 2.0)), layout, **more)


def test_cells_of_lens_A_sit_on_their_lattice(tool):
    inputs, got = lens_and_result(tool, 'A')
    cells = inputs[2]['cells']
    check_bins(cells, got)
    assert got['lat_ok'][0] == 1
    inv, na, nb = got['lat_inv'].reshape(2, 2), got['lat_na'][0], got['lat_nb'][0]
    # every cell at its node: (u, v) = inv (p - c0), the map's entry there is the cell's sorted slot
    uv = (cells[:, :2] - [got['lat_c0x'][0], got['lat_c0y'][0]]) @ inv.T
    node = np.rint(uv).astype(int) - [got['lat_amin'][0], got['lat_bmin'][0]]
    assert np.abs(uv - np.rint(uv)).max() < 1e-6 and node.min() >= 0 and node[:, 0].max() < na and node[:, 1].max() < nb
    lat_map = got['cell_lattice_map'].reshape(na, nb)
    assert np.array_equal(lat_map[node[:, 0], node[:, 1]], got['slot_of_cell'])
    assert np.count_nonzero(lat_map >= 0) == len(cells) and lat_map.min() == -1
    # the basis, taken from the cells themselves (the steps from the cell on node (a, b) to those on (a + 1, b) and
    # (a, b + 1)): inv times it is the identity, its metric is g, the accepted radius exceeds half a pitch
    a, b = np.argwhere((lat_map[:-1, :-1] >= 0) & (lat_map[1:, :-1] >= 0) & (lat_map[:-1, 1:] >= 0))[0]
    at = lambda slot: np.array([got['cell_x'][slot], got['cell_y'][slot]])
    b1, b2 = at(lat_map[a + 1, b]) - at(lat_map[a, b]), at(lat_map[a, b + 1]) - at(lat_map[a, b])
    basis = np.column_stack((b1, b2))
    assert np.abs(inv @ basis - np.eye(2)).max() <= 1e-12
    assert np.allclose(got['lat_g'], [b1 @ b1, b1 @ b2, b2 @ b2], rtol=1e-12, atol=0)
    assert got['lat_accept_r2'][0] > (0.5 * math.sqrt(b1 @ b1)) ** 2 and got['lat_guard'][0] > 0
    # the node records: the sorted cell of the node, or an empty record
    rec = got['cell_lattice_rec'].view(CELL_REC)
    full = lat_map.ravel() >= 0
    slot = lat_map.ravel()[full]
    assert rec.size == na * nb and not rec['pad'].any()
    assert np.array_equal(rec['x'][full], got['cell_x'][slot]) and np.array_equal(rec['y'][full], got['cell_y'][slot])
    assert np.array_equal(rec['which'][full], got['cell_which'][slot]) and np.array_equal(rec['index'][full], got['cell_index'][slot])
    assert np.isnan(rec['x'][~full]).all() and np.isnan(rec['y'][~full]).all()
    assert np.all(rec['which'][~full] == -1) and np.all(rec['index'][~full] == -1)


def test_cells_that_are_no_lattice(tool):
    cells = hex_cells()
    got = run_cells(tool, cells)
    check_bins(cells, got)
    assert got['lat_ok'][0] == 1 and np.count_nonzero(got['cell_lattice_map'] >= 0) == 36
    got = run_cells(tool, cells[:15])           # too few to be worth it
    check_bins(cells[:15], got)
    assert got['lat_ok'][0] == 0 and 'cell_lattice_map' not in got
    moved = cells.copy()
    moved[20, 0] += 1e-3 * 0.4e-6               # one cell off its node by 1e-3 of the pitch
    assert run_cells(tool, moved)['lat_ok'][0] == 0
    doubled = np.vstack((cells, cells[7:8]))    # two cells on one node
    got = run_cells(tool, doubled)
    check_bins(doubled, got)
    assert got['lat_ok'][0] == 0


# ---- errors and sanitizers -----------------------------------------------------------------
def error_of(got):
    assert set(got) == {'error_code', 'error_message'}
    return int(got['error_code'][0]), got['error_message'].tobytes().decode()


def test_errors_keep_code_and_message(tool):
    one = small_table([(0, 0)])
    got = tool({0: one}, None, small_layout([0, 2], [2.0, 2.0]))
    assert error_of(got) == (ML_ESTATE, 'ring 1 uses grating collection 2, which has no uploaded table')
    got = tool({s: one for s in range(17)}, None, small_layout(list(range(17)), [2.0] * 17))
    assert error_of(got) == (ML_EINVAL, 'the rings use more than 16 grating collections')
    cells = hex_cells()
    cells[5, 2] = 2048
    got = run_cells(tool, cells)
    assert error_of(got) == (ML_EINVAL, 'centre cell 5 has grating index 2048: 0 ... 2047 are supported')
    got = tool({0: one}, None, small_layout([0, 32], [2.0, 2.0]))
    assert error_of(got) == (ML_EINVAL, 'ring 1 uses grating collection 32: 0 ... 31 are supported')


def test_under_sanitizers(tool):
    """the same program under the address and undefined-behaviour sanitizers: same results, nothing reported"""
    inputs, got = lens_and_result(tool, 'D')
    again = tool(*inputs, exe='lens_pack_san')
    assert set(again) == set(got) and all(np.array_equal(again[k], got[k], equal_nan=True) for k in got)
    moved = hex_cells()
    moved[20, 0] += 1e-3 * 0.4e-6
    assert run_cells(tool, moved, exe='lens_pack_san')['lat_ok'][0] == 0
