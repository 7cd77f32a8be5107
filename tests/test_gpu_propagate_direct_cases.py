"""Every row of tests/propagate_direct_cases.py on the GPU: the direct pair sum (csrc/propagate.hip ``propagate_kernel<WANT_H,
NS>``) on all targets of the row, compared at the row's compared targets (at most 64: flat 0, 63, 64, 255, 256, T - 1, a
plane's corners and an even spread) with the long-double sum of tests/propagate_ref.py.  Needs an MI355X.

Two bounds per row and variant.  Per target: the modulus of the error of every component within (104 + 3 n + 6 Phi[t]) u
A[t] (propagate_ref.term_sums: derived from the kernel's operations, A[t] the sum of the absolute values of the target's own
terms) - a weak target cannot hide behind a strong one.  Per row: the rule of test_gpu_propagate.py, ``max_error`` of the GPU
at most 8 x that of the plain-fp64 NumPy sum (e_ref).  The measured figures are printed as ``PARITY direct-case ...`` lines
(run with -s; they belong in profiles/propagate_parity.txt).

The fields of a resident row are synthesised on the GPU; what the table claims of them - row extents that span more than a
tile, workgroups that skip a row and sum a later one - is asserted from the downloaded fields."""
import functools

import numpy as np
import pytest

import propagate_direct_cases as cases
import propagate_ref as ref
import test_gpu_propagate_sets as ts
from test_gpu_fft_mixed import _upload
from test_gpu_propagate import _stack
from test_gpu_propagate_sets import _batch, _check_sums, _same, _select

pytestmark = pytest.mark.gpu

WL = ref.WL
CASES = [(name, h) for name in sorted(cases.ROWS) for h in cases.ROWS[name].want_h]
E_KEYS, H_KEYS = ('Ex', 'Ey', 'Ez'), ('Hx', 'Hy', 'Hz')


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


@pytest.fixture
def ctx():
    from metalens_amd import _lib
    c = _lib.default_context()
    c.set_method('auto')
    c.set_precision('f64')
    return c


@functools.lru_cache(maxsize=None)
def _uploaded_yardstick(name, Z0):
    return cases.yardstick(name, cases.uploaded_fields(name), Z0)


_RESIDENT_YARDSTICKS = {}


def _resident_yardstick(name, member, F, Z0, n_glass):
    """computed once per (row, member) and shared by the variants: the synthesis must give the same fields each time"""
    key = (name, member)
    if key not in _RESIDENT_YARDSTICKS:
        _RESIDENT_YARDSTICKS[key] = ([f.copy() for f in F], cases.yardstick(name, F, Z0, n_glass))
    kept, y = _RESIDENT_YARDSTICKS[key]
    for a, b in zip(kept, F):
        assert np.array_equal(a, b)
    return y


def _download_fields(ctx, nx, ny):
    from metalens_amd import _lib
    F = [np.empty((nx, ny), dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    return F


def _check(name, h, member, out, y):
    """the two bounds for one result dict, the PARITY line, and Sz or I against its restatement"""
    want_h = h == 'EH'
    T = cases.n_targets(cases.ROWS[name])
    E = _stack(out, E_KEYS, T)
    assert set(out) == set(ts._keys(want_h))
    sides = [('E', E, y.El, y.bound_E, y.eE_ref, y.ratio_E64)]
    if want_h:
        H = _stack(out, H_KEYS, T)
        sides.append(('H', H, y.Hl, y.bound_H, y.eH_ref, y.ratio_H64))
    failed = []
    for side, got, want, bound, e_ref, ratio64 in sides:
        e_gpu, ratio = ref.max_error(got[:, y.at], want), ref.bound_ratio(got[:, y.at], want, bound)
        print('PARITY direct-case %-13s %-2s set %d %s: e_ref %.3e gpu %.3e; worst error / bound per target: gpu %.5f fp64 NumPy %.5f'
              % (name, h, member, side, e_ref, e_gpu, ratio, ratio64))
        assert np.abs(want).min() > 0
        if not (ratio <= 1 and ratio64 <= 1 and e_gpu <= 8 * e_ref):
            failed.append((side, e_ref, e_gpu, ratio, ratio64))
    assert not failed, failed
    if want_h:
        assert np.array_equal(out['Sz'].reshape(T), ref.poynting(E, H)[2])
    else:
        assert np.array_equal(out['I'].reshape(T), (np.abs(E) ** 2).sum(axis=0))


def _equal(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key


class _Raw:
    """the C ABI alone: ml_fields_upload, ml_propagate_plan, ml_propagate, ml_propagate_download - an aperture axis of one
    sample, which the Python class does not take"""

    def __init__(self, ma, ctx, name, want_h):
        from metalens_amd import _lib
        self.lib, self.ctx, self.want_h = _lib, ctx, want_h
        self.Z0 = ma.constants.as_units(None).Z0
        row = cases.ROWS[name]
        x, y, (dxp, dyp) = cases.axes(name)
        tx, ty, tz, point_list = (v if isinstance(v, bool) else _lib.f64(v) for v in cases.targets(name))
        assert point_list
        _upload(ctx, [_lib.c128(f) for f in cases.uploaded_fields(name)])
        ctx.fields_owner = None
        _lib.check(ctx.lib.ml_propagate_plan(ctx.handle, float(x[0]), float(y[0]), dxp, dyp, WL, ref.N_GLASS, _lib.dptr(tx), tx.size,
                                             _lib.dptr(ty), ty.size, _lib.dptr(tz), tz.size, 1, int(want_h)))
        ctx.propagate_owner = None       # whichever propagator planned before plans again
        self.shape = (tx.size,)
        nx, ny = _lib.c_int(0), _lib.c_int(0)
        _lib.check(ctx.lib.ml_fields_shape(ctx.handle, _lib.byref(nx), _lib.byref(ny)))
        assert (nx.value, ny.value) == (row.nx, row.ny)

    def propagate(self):
        self.lib.check(self.ctx.lib.ml_propagate(self.ctx.handle, self.Z0))
        # the dict as the class makes it, from ml_propagate_download
        return self._class()._download(None)

    def _class(self):
        import metalens_amd
        p = object.__new__(metalens_amd.PlanePropagator)
        p.ctx, p.shape, p.want_h = self.ctx, self.shape, self.want_h
        return p

    def accumulate(self, weights, reset):
        w = self.lib.f64(weights)
        self.lib.check(self.ctx.lib.ml_propagate_accumulate(self.ctx.handle, self.lib.dptr(w), w.size, int(reset)))

    def sums(self):
        I, Sz = np.empty(self.shape), np.empty(self.shape) if self.want_h else None
        self.lib.check(self.ctx.lib.ml_propagate_sums(self.ctx.handle, self.lib.dptr(I), self.lib.dptr(Sz)))
        return I, Sz


def _uploaded_row(ma, ctx, name, h):
    row = cases.ROWS[name]
    want_h = h == 'EH'
    if row.state == 'cabi':
        p = _Raw(ma, ctx, name, want_h)
    else:
        x, y, _ = cases.axes(name)
        tx, ty, tz, point_list = cases.targets(name)
        p = ma.PlanePropagator(x, y, WL, ref.N_GLASS, tx, ty, tz, point_list=point_list, want_h=want_h, ctx=ctx)
        _upload(ctx, cases.uploaded_fields(name))
        ctx.fields_owner = None
    out = p.propagate()
    assert out['Ex'].shape == ((cases.n_targets(row),) if row.targets[0] != 'plane' else row.targets[1:])
    _check(name, h, 0, out, _uploaded_yardstick(name, p.Z0))
    if name in cases.REPEATED:
        _equal(p.propagate(), out)
    if name in cases.SUMMED:
        p.accumulate([1.5], reset=True)
        p.accumulate([0.25], reset=False)
        I, Sz = p.sums()
        _check_sums(I, Sz, [[(1.5, out)], [(0.25, out)]], want_h)


def _resident_row(ma, ctx, name, h):
    row = cases.ROWS[name]
    want_h = h == 'EH'
    _, _, batch = cases.RESIDENT[name]
    batch = cases.ONE_DIPOLE if batch == 'ONE_DIPOLE' else getattr(ts, batch)
    wx, wy, _ = cases.axes(name)
    # _batch synthesises on a window of test_gpu_propagate_sets: this row's window under a name of its own
    ts.WINDOWS[name] = (row.nx, row.ny) + cases.RESIDENT[name][:2]
    try:
        x, y, n_glass, n = _batch(ma, ctx, name, batch)
    finally:
        del ts.WINDOWS[name]
    assert n == row.sets and np.array_equal(x, wx) and np.array_equal(y, wy)
    tx, ty, tz, point_list = cases.targets(name)
    p = ma.PlanePropagator(x, y, WL, n_glass, tx, ty, tz, point_list=point_list, want_h=want_h, ctx=ctx)
    sets = p.propagate_sets()
    assert len(sets) == n
    fields = []
    for m in range(n):
        _select(ctx, m)
        fields.append(_download_fields(ctx, row.nx, row.ny))
        _same(p.propagate(), sets[m], want_h)          # every set of the pass equals the single-set pass
    # what the table claims of the field, from the field: the extents belong to the grid and the lens, every member has them
    for F in fields:
        assert set(row.claims) <= cases.claims_shown(F, row.expect.splits), (name, cases.row_firsts(F))
        assert min(np.abs(f).max() for f in F) > 0
    for m in range(n):
        _check(name, h, m, sets[m], _resident_yardstick(name, m, fields[m], p.Z0, n_glass))
    # the same fields uploaded (no extents: every sample is read) give the bits of the resident ones
    for m in range(n):
        _upload(ctx, fields[m])
        ctx.fields_owner = None
        _same(p.propagate(), sets[m], want_h)


@pytest.mark.parametrize('name,h', CASES, ids=['%s-%s' % c for c in CASES])
def test_row_against_the_long_double_sum(ma, ctx, name, h):
    if cases.ROWS[name].state == 'resident':
        _resident_row(ma, ctx, name, h)
    else:
        _uploaded_row(ma, ctx, name, h)
