"""The overlap of a propagated image with separable modes contracted on the GPU (csrc/propagate_modes.hip,
ml_propagate_modes_plan / _queue / _fetch, ``PlanePropagator.overlap``, ``SourceSweep.run(image_modes=...)``) against the
yardstick of tests/propagate_modes_ref.py on the fields the same propagator downloads.  Needs an MI355X.

Shapes: the aperture, the wave and the cases of tests/test_gpu_propagate_focus.py - planes of 21 x 17 targets (one segment
of 32 along either axis, odd counts), of 70 x 61 (three segments along x, the last of 6; two along y, the last of 29) and a
stack of 3 planes of 13 x 11 (planes 1 and 2 on unaligned offsets); 'direct', 'fft' and 'fft-stack', with and without H.
Mode sets (``_modes``): 1 x 1, 5 x 1, 1 x 7, 3 x 64 and 64 x 64 complex normal tables.  An axis of 64 holds a repeat, an
all-zero mode, the constant 1, a pair m, conj(m), a purely imaginary mode and the delta modes at index 0, 31, 32 (where the
axis has them) and the last index, in a permuted order; the shorter axes hold of these what their count allows (5: m, zero, 1,
conj(m), m again; 7: imaginary, delta 0, delta last, m, conj(m), zero, m again; 3: m, 1, delta last; 1: m).

Bound, derived (tests/propagate_modes_ref.py): each of re and im within (mx + my + 16) u mag of the yardstick, u = 2^-53.
The yardstick is thinned to at most 2^20 (target, entry) pairs per component on the largest plane, 70 x 61, under 64 x 64
modes alone: every special mode of either axis stays, and every k-th of the random ones; the entries left out are held by
the bit tests (an entry does not depend on the others of its call), and the same sets are held in full on the smaller
planes.  The worst ratio of an error to its bound is printed per case as a ``PARITY modes ...`` line (run with -s; they belong
in profiles/propagate_parity.txt)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import propagate_grid_ref as gref
import propagate_modes_ref as mref
import propagate_ref as ref
from test_gpu_propagate_focus import CASES, N_GLASS, NX, NY, ROOT, WL, _dipole_batch, _make, _pitch, _planes, _window
from test_gpu_propagate_focus import ctx, ma  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

U = mref.U
SETS = {'1x1': (1, 1), '5x1': (5, 1), '1x7': (1, 7), '3x64': (3, 64), '64x64': (64, 64)}
ESTATE = -4          # ML_ESTATE
EDGES = (0, 31, 32)          # the first index and either side of a segment's end; the last index comes with the axis


def _delta(n, i):
    d = np.zeros(n, dtype=np.complex128)
    d[i] = 1.0
    return d


@functools.lru_cache(maxsize=None)
def _axis_modes(count, n, seed):
    """-> (complex (count, n), mask of the special modes): see the module docstring"""
    rng = np.random.default_rng(seed)
    normal = lambda k: rng.normal(size=(k, n)) + 1j * rng.normal(size=(k, n))
    m = normal(1)[0]
    zero, one, imag = np.zeros(n, dtype=complex), np.ones(n, dtype=complex), 1j * rng.normal(size=n)
    last = _delta(n, n - 1)
    if count == 1:
        return np.array([m]), np.ones(1, dtype=bool)
    if count == 3:
        return np.array([m, one, last]), np.ones(3, dtype=bool)
    if count == 5:
        return np.array([m, zero, one, m.conj(), m]), np.ones(5, dtype=bool)
    if count == 7:
        return np.array([imag, _delta(n, 0), last, m, m.conj(), zero, m]), np.ones(7, dtype=bool)
    special = [m, zero, one, m.conj(), imag, m, last] + [_delta(n, i) for i in EDGES if i < n - 1]
    table = np.concatenate([np.array(special), normal(count - len(special))])
    mask = np.arange(count) < len(special)
    order = rng.permutation(count)
    return table[order], mask[order]


def _modes(key, mx, my):
    """-> A (nu, mx), B (nv, my), the masks of their special modes"""
    nu, nv = SETS[key]
    (A, sa), (B, sb) = _axis_modes(nu, mx, 100 + nu), _axis_modes(nv, my, 200 + nv)
    return A, B, sa, sb


def _raw(p, A, B, member=0, slot=0, n_slots=None, plan=True):
    """plan (unless ``plan=False``), queue ``member`` into ``slot``, fetch it -> complex (planes, 4, nu, nv)"""
    from metalens_amd import _lib
    A, B = _lib.c128(np.atleast_2d(A)), _lib.c128(np.atleast_2d(B))
    planes, h, lib = _planes(p), p.ctx.handle, p.ctx.lib
    if plan:
        _lib.check(lib.ml_propagate_modes_plan(h, p.x.size, p.y.size, planes, _lib.dptr(A), A.shape[0], _lib.dptr(B), B.shape[0],
                                               slot + 1 if n_slots is None else n_slots))
    _lib.check(lib.ml_propagate_modes_queue(h, member, slot))
    return _fetch(p, slot, 1, A.shape[0], B.shape[0])[0]


def _fetch(p, first, n, nu, nv):
    from metalens_amd import _lib
    out = np.full((n, _planes(p), 4, nu, nv), np.nan + 1j * np.nan)
    _lib.check(p.ctx.lib.ml_propagate_modes_fetch(p.ctx.handle, first, n, _lib.dptr(out)))
    return out


def _components(p, d, want_h):
    """a result dict -> complex (planes, 4 or 2, mx, my)"""
    keys = mref.COMPONENTS[:4 if want_h else 2]
    return np.stack([np.asarray(d[k]).reshape(_planes(p), p.x.size, p.y.size) for k in keys], axis=1)


def _thin(n_targets, sa, sb):
    """-> index arrays into the modes of either axis: the special ones and every k-th of the others, k the smallest that leaves
    at most 2^20 (target, entry) pairs"""
    k = 1
    while True:
        ia, ib = (np.nonzero(s | (np.arange(s.size) % k == 0))[0] for s in (sa, sb))
        if n_targets * ia.size * ib.size <= 2 ** 20 or k > 64:
            return ia, ib
        k += 1


def _check(got, F, A, B, want_h, ia=None, ib=None):
    """(planes, 4, nu, nv) against the yardstick on F (planes, 4 or 2, mx, my) -> the worst ratio of an error to its bound"""
    ia, ib = (np.arange(len(A)) if ia is None else ia), (np.arange(len(B)) if ib is None else ib)
    worst = 0.0
    for q in range(F.shape[0]):
        for c in range(4):
            if c >= F.shape[1]:
                assert not got[q, c].any()          # without H the two H blocks are zeros
                continue
            ratio, ok = mref.worst_ratio(got[q, c][np.ix_(ia, ib)], F[q, c], A[ia], B[ib])
            assert ok, (q, mref.COMPONENTS[c], ratio)
            worst = max(worst, ratio)
    assert want_h == (F.shape[1] == 4)
    return worst


# ---- parity: every case, every mode set ----------------------------------------------------------------------------
@pytest.mark.parametrize('key', list(SETS))
@pytest.mark.parametrize('name', sorted(CASES))
def test_entries_against_the_yardstick(ma, ctx, name, key):
    method, mx, my, want_h = CASES[name]
    p = _make(ma, ctx, name)
    F = _components(p, p.propagate(), want_h)
    A, B, sa, sb = _modes(key, mx, my)
    got = _raw(p, A, B)
    assert got.shape == (_planes(p), 4, len(A), len(B)) and got.tobytes() == _raw(p, A, B).tobytes()          # two calls: the same bits
    ia = ib = None
    if (mx, my) == (70, 61) and key == '64x64':          # the largest plane under 64 x 64 alone
        ia, ib = _thin(mx * my, sa, sb)
        assert sa[ia].sum() == sa.sum() and sb[ib].sum() == sb.sum() and mx * my * ia.size * ib.size <= 2 ** 20
    worst = _check(got, F, A, B, want_h, ia, ib)
    print('PARITY modes %-16s %-5s: worst error / bound %.4f' % (name, key, worst))
    # the zero mode returns zeros
    for a in np.nonzero(~A.any(axis=1))[0]:
        assert not got[:, :, a].any()
    for b in np.nonzero(~B.any(axis=1))[0]:
        assert not got[:, :, :, b].any()


# ---- exactness ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_delta_modes_return_the_stored_field(ma, ctx, name):
    method, mx, my, want_h = CASES[name]
    p = _make(ma, ctx, name)
    F = _components(p, p.propagate(), want_h)
    ii = sorted({i for i in EDGES + (mx - 1,) if i < mx})
    jj = sorted({j for j in EDGES + (my - 1,) if j < my})
    A = np.array([_delta(mx, i) for i in ii] + [np.zeros(mx)])
    B = np.array([np.zeros(my)] + [_delta(my, j) for j in jj])
    got = _raw(p, A, B)
    nc = F.shape[1]
    assert np.array_equal(got[:, :nc, :-1, 1:], F[:, :, ii][:, :, :, jj])
    assert F[:, :, ii][:, :, :, jj].all() and not got[:, :, -1].any() and not got[:, :, :, 0].any() and not got[:, nc:].any()


# ---- bit invariances ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['stack-13x11-EH', 'stack-13x11-E'])
def test_a_plane_of_the_stack_has_the_bits_of_the_plane_alone(ma, ctx, name):
    p = _make(ma, ctx, name)
    p.queue_sets(0, 1)
    of_stack = {key: _raw(p, *_modes(key, 13, 11)[:2]) for key in ('5x1', '3x64', '64x64')}
    assert not np.array_equal(of_stack['3x64'][0], of_stack['3x64'][1]) and not np.array_equal(of_stack['3x64'][1], of_stack['3x64'][2])
    for q in range(3):
        one = _make(ma, ctx, name, method='fft-fine', z=q)
        one.queue_sets(0, 1)
        for key in of_stack:
            assert _raw(one, *_modes(key, 13, 11)[:2])[0].tobytes() == of_stack[key][q].tobytes(), (q, key)


@pytest.mark.parametrize('name', ['fft-70x61-EH', 'direct-21x17-EH', 'stack-13x11-E'])
def test_an_entry_does_not_depend_on_the_others_of_its_call(ma, ctx, name):
    method, mx, my, want_h = CASES[name]
    p = _make(ma, ctx, name)
    p.queue_sets(0, 1)
    A, B = _modes('64x64', mx, my)[:2]
    # (above 8 modes along y a workgroup takes two rows, up to 8 one: the calls below cross both launches)
    full = _raw(p, A, B)
    rng = np.random.default_rng(41)
    for a, b in [(0, 0), (63, 63), (17, 40), (5, 63), (63, 2)] + [tuple(rng.integers(0, 64, 2)) for _ in range(3)]:
        assert _raw(p, A[a], B[b])[:, :, 0, 0].tobytes() == np.ascontiguousarray(full[:, :, a, b]).tobytes(), (a, b)
    pa, pb = rng.permutation(64), rng.permutation(64)
    assert np.array_equal(_raw(p, A[pa], B[pb]), full[:, :, pa][:, :, :, pb])
    sub_a, sub_b = np.array([3, 60, 3, 31, 8]), np.array([9, 1, 50, 22, 63, 9, 40])          # 5 x 7, with repeats
    assert np.array_equal(_raw(p, A[sub_a], B[sub_b]), full[:, :, sub_a][:, :, :, sub_b])
    for nv in (1, 7, 8, 9, 33):          # either side of the two row launches
        assert np.array_equal(_raw(p, A[:2], B[:nv]), full[:, :, :2, :nv]), nv
    # the slot does not enter: slot 5 has the bytes of slot 0, and the slots between them, never written, read zeros
    assert _raw(p, A, B, slot=5, n_slots=7).tobytes() == full.tobytes()
    others = _fetch(p, 0, 7, 64, 64)
    assert others[5].tobytes() == full.tobytes() and not others[:5].any() and not others[6].any()
    assert _raw(p, A, B, slot=0, plan=False).tobytes() == full.tobytes() and _fetch(p, 5, 1, 64, 64)[0].tobytes() == full.tobytes()


@pytest.mark.parametrize('want_h', [True, False], ids=['EH', 'E'])
def test_members_of_a_pass(ma, ctx, want_h):
    """members 0 to 2 of a ``propagate_sets`` pass: each against the yardstick on its downloaded fields, and with the bits of
    ``propagate()`` on that set alone"""
    from metalens_amd import _lib
    x, y, n_glass = _dipole_batch(ma, ctx)
    tx = x.mean() + (np.arange(21) - 10) * 0.37e-6
    ty = y.mean() + (np.arange(17) - 8) * 0.37e-6
    p = ma.PlanePropagator(x, y, WL, n_glass, tx, ty, 20e-6, want_h=want_h, ctx=ctx)
    sets = p.propagate_sets()
    assert len(sets) == 3
    A, B = _modes('3x64', 21, 17)[:2]
    _raw(p, A, B, n_slots=3)
    got = [_raw(p, A, B, member=m, slot=m, plan=False) for m in range(3)]
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    assert np.array_equal(_fetch(p, 0, 3, 3, 64), np.array(got))
    worst = max(_check(got[m], _components(p, sets[m], want_h), A, B, want_h) for m in range(3))
    print('PARITY modes members %s 3x64: worst error / bound %.4f' % ('EH' if want_h else 'E', worst))
    assert ctx.lib.ml_propagate_modes_queue(ctx.handle, 3, 0) == -1          # ML_EINVAL
    assert 'ml_propagate_modes_queue: member 3 asked for, the last pass propagated 3 field sets' in ctx.lib.ml_last_error().decode()
    for m in range(3):
        _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
        p.propagate()
        assert _raw(p, A, B, plan=False).tobytes() == got[m].tobytes(), m          # (a pass keeps the plan's tables)
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))


# ---- state: nothing else moves ---------------------------------------------------------------------------------------
def test_state_and_refusals(ma, ctx):
    from metalens_amd import _lib
    from metalens_amd.propagate import plan_info
    p = _make(ma, ctx, 'direct-21x17-EH')
    lib, h = ctx.lib, ctx.handle
    A, B = _modes('3x64', 21, 17)[:2]
    A, B = _lib.c128(A), _lib.c128(B)
    dA, dB = _lib.dptr(A), _lib.dptr(B)
    said = lambda: lib.ml_last_error().decode()
    # no pass has run: the wording of ml_propagate_download; then no tables on the plan: a wording of its own
    assert lib.ml_propagate_modes_queue(h, 0, 0) == ESTATE and 'ml_propagate has not run on the active propagation plan' in said()
    with pytest.raises(_lib.MetalensHipError, match='ml_propagate has not run on the active propagation plan'):
        p.overlap(A, B)
    p.propagate()
    assert lib.ml_propagate_modes_queue(h, 0, 0) == 0          # (overlap() had planned its tables before its queue was refused)
    p._plan()          # a re-plan drops the result and the tables with it
    assert lib.ml_propagate_modes_queue(h, 0, 0) == ESTATE and 'ml_propagate has not run on the active propagation plan' in said()
    d = p.propagate()
    assert lib.ml_propagate_modes_queue(h, 0, 0) == ESTATE and 'ml_propagate_modes_plan has not run on the active propagation plan' in said()
    out = np.full((1, 1, 4, 3, 64), np.nan + 0j)
    assert lib.ml_propagate_modes_fetch(h, 0, 1, _lib.dptr(out)) == ESTATE and 'ml_propagate_modes_plan has not run' in said()
    assert np.isnan(out).all()
    p.accumulate([2.0], reset=True)
    sums, info = p.sums(), plan_info(ctx)
    radii = (np.arange(5) + 0.5) * _pitch(p)[0]
    focus, f = p.focus(radii), [0.0, 0.1 / _pitch(p)[0]]
    otf = p.otf(f, f)
    before = _raw(p, A, B, slot=1, n_slots=4)
    bad = A.copy()
    bad[2, 20] = complex(1.0, np.inf)
    odd = B.copy()
    odd[63, 0] = complex(np.nan, 0.0)
    for args, text in (((17, 17, 1, dA, 3, dB, 64, 4), '1 planes of 17 x 17 targets are 289 targets, the active propagation plan has 357'),
                       ((21, 17, 2, dA, 3, dB, 64, 4), '2 planes of 21 x 17'),
                       ((21, 17, 1, dA, 0, dB, 64, 4), '0 x 64 modes: 1 to 64 are taken per axis'),
                       ((21, 17, 1, dA, 3, dB, 65, 4), '3 x 65 modes'),
                       ((21, 17, 1, None, 3, dB, 64, 4), 'NULL argument (mode_x NULL, mode_y given)'),
                       ((21, 17, 1, dA, 3, None, 64, 4), 'NULL argument (mode_x given, mode_y NULL)'),
                       ((21, 17, 1, dA, 3, dB, 64, 0), '0 output slots: 1 to 4096 are reserved per plan'),
                       ((21, 17, 1, dA, 3, dB, 64, 4097), '4097 output slots'),
                       ((21, 17, 1, dB, 64, dB, 64, 4096), '4096 slots x 1 planes x 4 x 64 x 64 modes = 67108864 output entries, at most 2^24 = 16777216'),
                       ((21, 17, 1, _lib.dptr(bad), 3, dB, 64, 4), 'mode_x[2][20] = (1, inf): a table entry is finite'),
                       ((21, 17, 1, dA, 3, _lib.dptr(odd), 64, 4), 'mode_y[63][0] = (nan, 0)')):
        assert lib.ml_propagate_modes_plan(h, *args) == -1          # ML_EINVAL
        assert text in said(), (text, said())
    for args, text in (((1, 0), 'member 1 asked for, the last pass propagated 1 field sets'),
                       ((-1, 0), 'source -1: a member of the last pass (>= 0)'),
                       ((0, 4), 'slot 4, the plan reserved the slots 0 ... 3'),
                       ((0, -1), 'slot -1')):
        assert lib.ml_propagate_modes_queue(h, *args) == -1 and text in said(), (text, said())
    big = np.zeros((5, 1, 4, 3, 64), dtype=np.complex128)
    for args, text in (((3, 2, _lib.dptr(big)), 'slots 3 ... 4 asked for, the plan reserved the slots 0 ... 3'),
                       ((-1, 1, _lib.dptr(big)), 'slots -1 ... -1'), ((0, 0, _lib.dptr(big)), 'slots 0 ... -1'),
                       ((0, 4, None), 'NULL argument (out NULL)')):
        assert lib.ml_propagate_modes_fetch(h, *args) == -1 and text in said(), (text, said())
    # the refused calls have left the plan's tables and every slot as they were; an accepted one writes its own slot only
    slots = _fetch(p, 0, 4, 3, 64)
    assert slots[1].tobytes() == before.tobytes() and not slots[[0, 2, 3]].any()
    assert _raw(p, A, B, slot=3, plan=False).tobytes() == before.tobytes()
    slots = _fetch(p, 0, 4, 3, 64)
    assert slots[1].tobytes() == slots[3].tobytes() == before.tobytes() and not slots[[0, 2]].any()
    # accepted and refused calls have left the fields, the sums, the focus records, the transfer function and the plan alone
    for key, value in p._download(None).items():
        assert np.array_equal(value, d[key]), key
    for got, want in zip(p.sums(), sums):
        assert np.array_equal(got, want)
    assert plan_info(ctx) == info
    again, otf_again = p.focus(radii), p.otf(f, f)
    assert set(again) == set(focus) and all(np.array_equal(again[k], focus[k]) for k in focus)
    assert all(np.array_equal(otf_again[k], otf[k]) for k in otf)
    assert p.overlap(A, B)['overlap_Ex'].tobytes() == (before[:, 0] * np.prod(_pitch(p))).tobytes()
    assert all(np.array_equal(value, d[k]) for k, value in p.propagate().items())
    # another propagator plans: the tables are gone with the plan, and this one's overlap is refused as focus and otf are
    other = _make(ma, ctx, 'fft-21x17-E')
    assert lib.ml_propagate_modes_queue(h, 0, 0) == ESTATE and 'ml_propagate has not run on the active propagation plan' in said()
    other.queue_sets(0, 1)
    assert lib.ml_propagate_modes_queue(h, 0, 0) == ESTATE and 'ml_propagate_modes_plan has not run on the active propagation plan' in said()
    assert lib.ml_propagate_modes_fetch(h, 0, 1, _lib.dptr(big)) == ESTATE
    with pytest.raises(RuntimeError, match='another propagator has planned'):
        p.overlap(A, B)
    assert set(other.overlap(A, B)) == {'overlap_Ex', 'overlap_Ey', 'norm', 'power', 'coupling_x', 'coupling_y'}


def test_a_context_of_several_ranks_is_refused(ma, monkeypatch):
    """as every propagation entry: the refusal comes before the state is looked at, so no plan is needed"""
    from metalens_amd import _lib
    monkeypatch.setenv('ML_COMM_BACKEND', 'file')
    c = _lib.Context(0)
    try:
        ident = (_lib.c_uint8 * 128)()
        _lib.check(c.lib.ml_comm_unique_id(ident))
        _lib.check(c.lib.ml_comm_init(c.handle, ident, 2, 0))
        m, out = _lib.c128(np.ones((1, 21))), np.zeros((1, 1, 4, 1, 1), dtype=np.complex128)
        assert c.lib.ml_propagate_modes_plan(c.handle, 21, 21, 1, _lib.dptr(m), 1, _lib.dptr(m), 1, 1) == -1          # ML_EINVAL
        assert 'ml_propagate_modes_plan: this context belongs to a communicator of 2 ranks' in c.lib.ml_last_error().decode()
        assert c.lib.ml_propagate_modes_queue(c.handle, 0, 0) == -1
        assert 'ml_propagate_modes_queue: this context belongs to a communicator of 2 ranks' in c.lib.ml_last_error().decode()
        assert c.lib.ml_propagate_modes_fetch(c.handle, 0, 1, _lib.dptr(out)) == -1
        assert 'ml_propagate_modes_fetch: this context belongs to a communicator of 2 ranks' in c.lib.ml_last_error().decode()
        assert not out.any()
    finally:
        c.close()


# ---- the Python level -----------------------------------------------------------------------------------------
def test_python_dict(ma, ctx):
    from metalens_amd.postprocess import mode_norm
    name = 'fft-70x61-EH'
    method, mx, my, want_h = CASES[name]
    p = _make(ma, ctx, name)
    p.queue_sets(0, 1)
    dx, dy = _pitch(p)
    A, B = _modes('5x1', mx, my)[0], _modes('1x7', mx, my)[1]
    out = p.overlap(A, B)
    assert set(out) == {'overlap_Ex', 'overlap_Ey', 'overlap_Hx', 'overlap_Hy', 'norm', 'power', 'coupling_x', 'coupling_y'}
    assert out['overlap_Ex'].shape == out['coupling_y'].shape == (1, 5, 7) and out['overlap_Hy'].dtype == np.complex128
    assert out['norm'].shape == (5, 7) and out['power'].shape == (1,) and np.array_equal(out['norm'], mode_norm(A, B, dx, dy))
    raw = _raw(p, A, B)
    for c, key in enumerate(mref.COMPONENTS):
        assert np.array_equal(out['overlap_' + key], raw[:, c] * (dx * dy)), key
    assert np.array_equal(out['power'], p.focus()['P'])
    # NaN where the norm is 0 (the zero mode), finite elsewhere; a given power scales
    live = [0, 1, 2, 3, 4, 6]          # (mode 5 of the y axis is the zero mode)
    assert np.isnan(out['coupling_x'][:, 1]).all() and np.isnan(out['coupling_x'][:, :, 5]).all()
    assert np.isfinite(out['coupling_x'][:, [0, 2, 3, 4]][:, :, live]).all()
    half = p.overlap(A, B, power=2 * out['power'])
    assert np.allclose(half['coupling_y'][:, 0, live], out['coupling_y'][:, 0, live] / 2, rtol=1e-15, atol=0)
    assert np.isnan(p.overlap(A, B, power=0.0)['coupling_x']).all()
    # 1-D modes are one mode per axis
    one = p.overlap(A[0], B[3])
    assert one['overlap_Ex'].shape == (1, 1, 1) and one['overlap_Ex'][0, 0, 0] == out['overlap_Ex'][0, 0, 3]
    # without H: the keys, and the Cauchy-Schwarz share of sum |E|^2 dA is at most 1 for any mode
    pe = _make(ma, ctx, 'direct-70x61-E')
    pe.queue_sets(0, 1)
    A64, B64 = _modes('64x64', mx, my)[:2]
    oe = pe.overlap(A64, B64)
    assert set(oe) == {'overlap_Ex', 'overlap_Ey', 'norm', 'power', 'coupling_x', 'coupling_y'}
    assert np.array_equal(oe['power'], pe.focus()['I_dA'])
    for key in ('coupling_x', 'coupling_y'):
        finite = np.isfinite(oe[key])
        assert finite.sum() >= 62 * 62 and (oe[key][finite] <= 1 + 1e-12).all() and (oe[key][finite] >= 0).all()
    given = pe.overlap(A64[:2], B64[:2], power=[3.0])
    assert np.isfinite(given['coupling_x']).any()
    Z = pe.Z0 / N_GLASS
    assert np.allclose(given['coupling_x'], np.abs(given['overlap_Ex']) ** 2 / (2 * Z * given['norm'] * 3.0), rtol=1e-14, atol=0, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _gaussian():
    """the aperture of ``gref.axis`` carrying an x-polarised Gaussian beam at its waist -> x, y, Z, w0, (Ex, Ey, Hx, Hy)"""
    x, y = gref.axis(NX), gref.axis(NY)
    Z, w0 = ref.Z0_SI / N_GLASS, 3 * WL
    psi = np.exp(-(x[:, None] ** 2 + y[None, :] ** 2) / w0 ** 2).astype(np.complex128)
    return x, y, Z, w0, (psi, 0 * psi, 0 * psi, psi / Z)


def _gaussian_case(ma, ctx):
    """-> the propagator of the beam to z = 20e-6 on the centred 70 x 61 patch after its pass, the modes at d = 0, w0 / 2, w0"""
    from metalens_amd import _lib
    from test_gpu_fft_mixed import _upload
    x, y, Z, w0, F = _gaussian()
    _upload(ctx, [_lib.c128(a) for a in F])
    ctx.fields_owner = None
    z = 20e-6
    tx, ty = gref.target_axis(x, (NX - 1) / 2 - 35, 70), gref.target_axis(y, (NY - 1) / 2 - 30, 61)
    p = ma.PlanePropagator(x, y, WL, N_GLASS, tx, ty, z, ctx=ctx, method='fft', Z0=ref.Z0_SI)
    offsets = np.array([0.0, w0 / 2, w0])
    A = np.array([ma.gaussian_axis(tx, w0, z, centre=d, wavelength=WL, n=N_GLASS) for d in offsets])
    B = ma.gaussian_axis(ty, w0, z, wavelength=WL, n=N_GLASS)
    return p, A, B, offsets, w0, Z


def test_a_gaussian_beam_couples_into_itself(ma, ctx):
    """A Gaussian aperture field couples into the same beam, propagated analytically, with efficiency 1, and shifted by d with
    exp(-d^2 / w0^2).  On the CPU reference (tests/propagate_grid_ref.grid_sum + postprocess.mode_overlaps) coupling_x deviates
    from that by 6.6e-7, 3.0e-7 and 1.6e-8 at d = 0, w0 / 2, w0 - the paraxial and truncation error of the model, not
    arithmetic - and the power through the patch exceeds the incident one by 8.8e-7; the GPU is held to 1e-5, a decade over
    that."""
    from metalens_amd.postprocess import mode_coupling
    p, A, B, offsets, w0, Z = _gaussian_case(ma, ctx)
    d = p.propagate()
    out = p.overlap(A, B)
    want = np.exp(-offsets ** 2 / w0 ** 2)
    dev = out['coupling_x'][0, :, 0] - want
    print('PARITY modes gaussian: coupling_x - exp(-d^2 / w0^2) = %s, coupling_y max %.3g' % (dev, out['coupling_y'].max()))
    assert (np.abs(dev) <= 1e-5).all() and (out['coupling_y'] < 1e-6).all()
    x, y, _, _, F = _gaussian()
    P_in = (np.abs(F[0]) ** 2).sum() * (x[1] - x[0]) * (y[1] - y[0]) / (2 * Z)
    incident = p.overlap(A, B, power=P_in)
    assert (np.abs(incident['coupling_x'] / out['coupling_x'] - 1) < 1e-5).all() and incident['power'][0] == P_in
    # the coupling from the GPU's overlaps and from the yardstick's, through the same helper: 1e-10 relative (the entries are
    # large against their bounds here, about 5e-13 of them)
    Fp = _components(p, d, True)
    dA = np.prod(_pitch(p))
    exact = {key: (mref.overlaps(Fp[0, c], A, B[None, :])[0] * dA)[None] for c, key in enumerate(mref.COMPONENTS)}
    cx, cy = mode_coupling(exact, out['norm'], Z, power=out['power'])
    assert np.allclose(out['coupling_x'], cx, rtol=1e-10, atol=0)
    worst = _check(_raw(p, A, B), Fp, A, B[None, :], True)
    print('PARITY modes gaussian 3x1: worst error / bound %.4f' % worst)
    # the NumPy twin on the downloaded fields
    twin = ma.mode_overlaps(d, p.x, p.y, A, B, Z)
    assert set(twin) == set(out)
    # (Ey, Hx and coupling_y are rounding noise of either side here: held on the scale of their partners)
    scale = {'overlap_Ey': np.abs(out['overlap_Ex']).max(), 'overlap_Hx': np.abs(out['overlap_Hy']).max(), 'coupling_y': 1.0}
    for key in out:
        assert np.allclose(twin[key], out[key], rtol=1e-9, atol=1e-9 * scale.get(key, 0.0)), key


def test_through_the_sweep(ma, ctx):
    from test_gpu_propagate_sets import _common, _lens
    lens = _lens()
    x, y = _window()
    uu = np.linspace(-0.2, 0.2, 24)
    sw = ma.SourceSweep(*_common(lens), x, y, uu, uu, ctx=ctx)
    tx = x.mean() + (np.arange(21) - 10) * 0.37e-6
    ty = y.mean() + (np.arange(17) - 8) * 0.37e-6
    p = ma.PlanePropagator(x, y, WL, sw.n_glass, tx, ty, 20e-6, ctx=ctx)
    f = lens['source_distance']
    sources = [(0.3e-6, -0.2e-6, -f, pol) for pol in 'xyz'] + [(-1.0e-6, 0.5e-6, -1.05 * f, 'x')]
    weights = np.array([1.0, 0.5, 2.0, 1.5])
    w0 = 1.2e-6
    A = np.array([ma.gaussian_axis(tx, w0, centre=c, wavelength=WL, n=sw.n_glass) for c in tx[[10, 8, 13]]]
                 + [ma.hermite_gauss_axis(1, tx, w0, centre=tx[10], wavelength=WL, n=sw.n_glass)])
    B = np.array([ma.gaussian_axis(ty, w0, centre=ty[8], wavelength=WL, n=sw.n_glass), _axis_modes(1, 17, 7)[0][0]])
    plain = sw.run(sources, weights=weights, image=p, keep_each=True)
    got = sw.run(sources, weights=weights, image=p, keep_each=True, image_modes=(A, B))
    assert set(got) == set(plain) | {'image_coupling'}
    for key in plain:
        if key in ('P_each', 'image_each'):
            continue
        assert np.array_equal(got[key], plain[key], equal_nan=True), key
    for k in range(4):
        assert np.array_equal(got['P_each'][k], plain['P_each'][k], equal_nan=True)
        assert all(np.array_equal(got['image_each'][k][key], plain['image_each'][k][key]) for key in plain['image_each'][k])
    ic = got['image_coupling']
    assert set(ic) == {'overlap_Ex', 'overlap_Ey', 'overlap_Hx', 'overlap_Hy', 'norm', 'power', 'coupling_x', 'coupling_y'}
    assert ic['overlap_Ex'].shape == ic['coupling_x'].shape == (4, 1, 4, 2) and ic['norm'].shape == (4, 2)
    assert np.array_equal(ic['power'], plain['power_in'][:, None])
    # every source against the yardstick on its own image (the tie-settlement repeat of the first pass left no stale slot),
    # the coupling taken over its power_in
    dA = np.prod(_pitch(p))
    worst = 0.0
    for k in range(4):
        F = _components(p, got['image_each'][k], True)
        raw = np.stack([ic['overlap_' + key][k] for key in mref.COMPONENTS], axis=1) / dA
        worst = max(worst, _check(raw, F, A, B, True))
    print('PARITY modes sweep 4 sources 4x2: worst error / bound %.4f' % worst)
    Z = p.Z0 / sw.n_glass
    want = np.abs(ic['overlap_Ex'] / Z + ic['overlap_Hy']) ** 2 * Z / (8 * ic['norm'] * plain['power_in'][:, None, None, None])
    assert np.allclose(ic['coupling_x'], want, rtol=1e-13, atol=0) and (ic['coupling_x'] >= 0).all() and (ic['coupling_x'] <= 1).all()
    # source 3 alone in its pass is member 0 of the last one: the bytes of overlap() on it
    alone = p.overlap(A, B, member=0)
    for key in mref.COMPONENTS:
        assert alone['overlap_' + key].tobytes() == np.ascontiguousarray(ic['overlap_' + key][3]).tobytes(), key
    # the sources of the polarisation group: the group's pass once more, member by member
    again = sw.run(sources[:3], image=p, image_modes=(A, B))
    for m in range(3):
        one = p.overlap(A, B, member=m)
        for key in mref.COMPONENTS:
            assert one['overlap_' + key].tobytes() == np.ascontiguousarray(again['image_coupling']['overlap_' + key][m]).tobytes()
            assert one['overlap_' + key].tobytes() == np.ascontiguousarray(ic['overlap_' + key][m]).tobytes(), (m, key)
    with pytest.raises(ValueError, match='image_modes= needs image='):
        sw.run(sources, image_modes=(A, B))


def test_example_runs(ma):
    """examples/fibre_coupling.py: one line per (emitter offset, fibre offset); every coupling is a share of the emitted power,
    and the on-axis emitter with the fibre at its aligned position couples best of all positions"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'fibre_coupling.py')], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    rows = [line.split() for line in res.stdout.splitlines() if line.startswith('coupling ')]
    table = {}          # coupling <emitter offset um> <fibre offset um> <value>
    for _, emitter, fibre, value in rows:
        table.setdefault(float(emitter), {})[float(fibre)] = float(value)
    assert len(table) >= 2 and all(len(t) >= 3 for t in table.values())
    values = np.array([v for t in table.values() for v in t.values()])
    assert np.isfinite(values).all() and (values >= 0).all() and (values <= 1 + 1e-6).all()
    on_axis = table[0.0]
    assert max(on_axis, key=on_axis.get) == 0.0 and on_axis[0.0] == values.max()
