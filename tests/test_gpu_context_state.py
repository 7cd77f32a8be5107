"""API objects taking turns on ONE context.

Every object built without ``ctx=`` shares ``_lib.default_context()``, and what a context keeps
between calls - tables, layout, far-field plan, resident fields, precision, method, the C-side
geometry / zero / trim / fold keys - is what makes the library fast.  The tests here run sequences
of operations on one long-lived context and compare every result with THE SAME OPERATION ON A
FRESH CONTEXT (``_lib.Context(0)``, closed afterwards), memoised by a description of the
operation.  The comparison is bit identity: ``np.array_equal`` with NaN positions equal, scalars
``==`` (the kernels are deterministic: fixed-order sums, no float atomics).  The first occurrence of
each operation kind in the random walk is also compared with the CPU oracle, so that the fresh
reference cannot be wrong in the same way."""
import functools

import numpy as np
import pytest

import golden_io
from test_gpu_parity import TOL, _synthetic_lens, field_errors

pytestmark = pytest.mark.gpu

WL = 580e-9
PITCH = WL / 2.2
F_KEYS = ('Ex', 'Ey', 'Hx', 'Hy')
FF_KEYS = ('Nx', 'Ny', 'Lx', 'Ly', 'P', 'a_theta', 'a_phi')


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


# ---- lenses, grids, directions, sources (all 30-60 um lenses, grids <= 320^2, directions <= 64^2) ----

@functools.lru_cache(None)
def lens(name):
    """'A': three orders per table; 'B': the orders characterize() would record ('physical'); 'G', 'M': lens A's
    layout with an order (0, 1) in every ring table / in the second of its two collections' tables only"""
    if name == 'A':
        return _synthetic_lens(20e-6, 0.35, WL, switch_deg=9.0)
    if name in ('G', 'M'):
        simple, general = ((0, 0), (-1, 0), (1, 0)), ((0, 0), (-1, 0), (0, 1))
        return _synthetic_lens(20e-6, 0.35, WL, switch_deg=9.0,
                               periphery_orders=general if name == 'G' else (simple, general))
    return _synthetic_lens(16e-6, 0.4, WL, switch_deg=9.0, periphery_orders='physical',
                           center_orders='physical')


def lens_args(name):
    L = lens(name)
    return L['lens_periphery_summary'], L['lens_center_summary'], L['hexgridset']


@functools.lru_cache(None)
def grid(name):
    """aperture sample axes (x, y)"""
    if name == 'sq':          # a 256^2 window around the lens (the FFT lattice path: 256 rows)
        x = (np.arange(256) - 127.5) * PITCH
        return x, x.copy()
    if name == 'w320':
        x = (np.arange(320) - 159.5) * PITCH
        return x, x.copy()
    if name == 'off':         # 200 x 136, off centre, different pitches
        return (4e-6 + (np.arange(200) - 99.5) * PITCH,
                -2.5e-6 + (np.arange(136) - 67.5) * 0.97 * PITCH)
    if name == 'tie':         # 61^2, symmetric with x[30] == 0.0 exactly: samples on mirror lines of the cell lattice
        x = (np.arange(61) - 30) * PITCH
        return x, x.copy()
    if name == 'strip':       # 3 x 2050
        return 0.3e-6 + (np.arange(3) - 1.0) * PITCH, (np.arange(2050) - 1024.5) * 0.05e-6
    raise KeyError(name)


def lattice(axis, m, ng):
    m = min(m, axis.size)
    return (np.arange(m) - m // 2) * ((WL / ng) / ((axis[1] - axis[0]) * axis.size))


@functools.lru_cache(None)
def directions(name, g, ng=1.459):
    """(ux, uy, pair_list): 'lat' on the aperture's FFT lattice, 'sym' off the lattice and
    symmetric (folded GEMMs), 'asym' asymmetric (generic GEMMs), 'pairs' a pair list"""
    x, y = grid(g)
    if name == 'lat':
        return lattice(x, 48, ng), lattice(y, 48, ng), False
    if name == 'sym':
        u = np.linspace(-0.2, 0.2, 40)
        return u, u.copy(), False
    if name == 'big':
        u = np.linspace(-0.25, 0.25, 64)
        return u, u.copy(), False
    if name == 'asym':
        return np.linspace(-0.3, 0.12, 37), np.linspace(-0.05, 0.25, 29), False
    if name == 'pairs':
        rng = np.random.default_rng(4)
        th = np.arcsin(rng.uniform(0, 0.3, 50))
        ph = rng.uniform(0, 2 * np.pi, 50)
        return np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), True
    raise KeyError(name)


def source(lens_name, k=0):
    f = lens(lens_name)['source_distance']
    return ((0.3e-6, -0.2e-6, -f, 'x'), (-0.5e-6, 0.4e-6, -1.03 * f, 'y'), (0.0, 0.0, -0.98 * f, 'z'))[k]


SOURCE_LISTS = {
    # a polarisation batch of 3, then a single source, then a position batch of 2
    'mixed': lambda L: [source(L, 0)[:3] + (p,) for p in 'xyz'] + [source(L, 1)] +
                       [(0.5e-6, 0.0, source(L, 0)[2], 'x'), (-0.5e-6, 0.3e-6, source(L, 1)[2], 'y')],
    'single': lambda L: [source(L, 2)],
}


@functools.lru_cache(None)
def host_fields(g, seed=1):
    x, y = grid(g)
    rng = np.random.default_rng(seed)
    return tuple(np.ascontiguousarray(rng.standard_normal((x.size, y.size)) + 1j * rng.standard_normal((x.size, y.size)))
                 for _ in range(4))


# ---- operations: a description (hashable) -> a dict of results -----------------------------------------

def _upload(ctx, F):
    from metalens_amd import _lib
    _lib.check(ctx.lib.ml_fields_upload(ctx.handle, F[0].shape[0], F[0].shape[1], *[_lib.dptr(a) for a in F]))


def _pooled(pool, key, make):
    if key not in pool:
        pool[key] = make()
    return pool[key]


def make_hotpath(ma, ctx, L, g, d, precision='f64', method='auto', fuse=True, src=0, world=1, rank=0,
                 sharding='auto'):
    x, y = grid(g)
    ux, uy, pairs = directions(d, g)
    return ma.HotPath(source(L, src), WL, *lens_args(L), x, y, ux, uy, pair_list=pairs, ctx=ctx,
                      precision=precision, method=method, fuse_modulation=fuse, world=world, rank=rank,
                      sharding=sharding, reduce='none')


def make_sweep(ma, ctx, L, g, d):
    x, y = grid(g)
    ux, uy, _ = directions(d, g)
    return ma.SourceSweep(WL, *lens_args(L), x, y, ux, uy, ctx=ctx)


def run_op(ma, ctx, pool, desc):
    """run the operation ``desc`` on ``ctx``; ``pool`` keeps the objects built on this context
    (a pooled HotPath / SourceSweep / PreparedLens is built on first use and re-used)"""
    from metalens_amd import _lib
    kind = desc[0]
    if kind == 'nf':                                  # build_nearfield, with / without download
        _, L, g, src, download = desc
        x, y = grid(g)
        out = ma.build_nearfield(*source(L, src), WL, *lens_args(L), x_pts=x, y_pts=y, ctx=ctx,
                                 download=download)
        res = {'power': out[6]}
        if download:
            res.update((k, np.array(v)) for k, v in zip(F_KEYS, out[:4]))
        return res
    if kind == 'pl':                                  # build_nearfield through a PreparedLens
        _, L, g, src = desc
        x, y = grid(g)
        p = _pooled(pool, ('pl', L), lambda: ma.PreparedLens(*lens_args(L), WL, ctx=ctx))
        out = ma.build_nearfield(*source(L, src), WL, p, None, None, x_pts=x, y_pts=y)
        return dict({'power': out[6]}, **{k: np.array(v) for k, v in zip(F_KEYS, out[:4])})
    if kind == 'ffd':                                 # farfield_direct on host fields (inherits the method)
        _, g, d, seed, method = desc
        x, y = grid(g)
        ux, uy, pairs = directions(d, g)
        out = ma.farfield_direct(*host_fields(g, seed), x, y, WL, 1.459, ux, uy, pair_list=pairs, ctx=ctx)
        return {k: out[k] for k in FF_KEYS}
    if kind == 'ffres':                               # synthesis left resident + the whole-lattice far field
        _, L, g, src, method = desc
        x, y = grid(g)
        out = ma.build_nearfield(*source(L, src), WL, *lens_args(L), x_pts=x, y_pts=y, ctx=ctx, download=False)
        P, total, *_ = ma.farfield_from_resident_nearfield(x, y, WL, out[7], ctx=ctx)
        return {'P': np.array(P), 'total_P': total, 'power': out[6]}
    if kind == 'hp':                                  # a step of a pooled HotPath
        args = desc[1:]
        hp = _pooled(pool, desc, lambda: make_hotpath(ma, ctx, *args))
        hp.step()
        hp.sync()
        r = hp.results()
        return {k: r[k] for k in FF_KEYS + ('power_local_rows',)}
    if kind == 'shard':                               # one rank's rows of a sharded HotPath (partial sums)
        _, L, g, d, world, rank, sharding = desc
        hp = _pooled(pool, desc, lambda: make_hotpath(ma, ctx, L, g, d, world=world, rank=rank,
                                                      sharding=sharding))
        hp.step_local()
        hp.sync()
        vec = [np.empty(hp.shape, dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_farfield_download(ctx.handle, *[_lib.dptr(v) for v in vec]))
        power = _lib.c_double(0)
        _lib.check(ctx.lib.ml_nearfield_result(ctx.handle, _lib.byref(power), None, 0, None))
        return dict({'power': power.value, 'sharding': hp.sharding}, **dict(zip(FF_KEYS[:4], vec)))
    if kind == 'sw':                                  # SourceSweep.run with mixed pol / position batches
        _, L, g, d, which = desc
        sw = _pooled(pool, desc, lambda: make_sweep(ma, ctx, L, g, d))
        r = sw.run(SOURCE_LISTS[which](L), cone=0.05)
        return {k: r[k] for k in ('P_sum', 'power_in', 'total_P', 'cone_P')}
    if kind == 'junk':                                # junk fields of another shape
        _, nx, ny = desc
        rng = np.random.default_rng(nx * 7 + ny)
        _upload(ctx, [np.ascontiguousarray(1e3 * rng.standard_normal((nx, ny)) + 0j) for _ in range(4)])
        return None
    if kind == 'method':
        ctx.set_method(desc[1])
        return None
    if kind == 'precision':
        ctx.set_precision(desc[1])
        return None
    raise KeyError(kind)


# operations whose result depends on the context's method at the time of the call (the drop-ins
# inherit it): their description ends with that method, and the fresh reference sets it first
INHERITS_METHOD = ('ffd', 'ffres')
_REFERENCE = {}


def reference(ma, desc):
    """the operation on a fresh context, memoised by its description"""
    if desc not in _REFERENCE:
        from metalens_amd import _lib
        ctx = _lib.Context(0)
        try:
            if desc[0] in INHERITS_METHOD:
                ctx.set_method(desc[-1])
            _REFERENCE[desc] = run_op(ma, ctx, {}, desc)
        finally:
            ctx.close()
    return _REFERENCE[desc]


def assert_same(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            assert g.shape == w.shape, (what, k, g.shape, w.shape)
            if not np.array_equal(g, w, equal_nan=True):
                ok = np.isfinite(w)
                err = np.abs(g[ok] - w[ok]).max() / max(np.abs(w[ok]).max(), 1e-300) if ok.any() else np.inf
                raise AssertionError('%s: %s differs from the fresh context (max rel %.3e, NaN positions '
                                     'equal: %s)' % (what, k, err, np.array_equal(np.isnan(g), np.isnan(w))))
        else:
            assert g == w, (what, k, g, w)


def check(ma, ctx, pool, desc):
    """run on the shared context, compare with the fresh one"""
    got = run_op(ma, ctx, pool, desc)
    if got is not None:
        assert_same(got, reference(ma, desc), desc)
    return got


# ---- the oracle: the first occurrence of each operation kind ------------------------------------------

def oracle_check(desc, got):
    from oracle import farfield_oracle, nearfield_oracle
    kind = desc[0]

    def nf(L, g, src):
        x, y = grid(g)
        return nearfield_oracle.build_nearfield(*source(L, src), WL, *lens_args(L), x_pts=x, y_pts=y)

    def rel(a, b):
        ok = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), ok)
        return np.abs(a[ok] - b[ok]).max() / np.abs(b[ok]).max()

    if kind in ('nf', 'pl'):
        want = nf(*desc[1:4])
        assert abs(got['power'] - want[6]) <= 1e-12 * abs(want[6]), desc
        if 'Ex' in got:
            for k, w in zip(F_KEYS, want[:4]):
                err, flips = field_errors(got[k], w)
                assert flips == 0 and err < TOL, (desc, k, err, flips)
    elif kind == 'ffd':
        _, g, d, seed, _m = desc
        x, y = grid(g)
        ux, uy, pairs = directions(d, g)
        F = host_fields(g, seed)
        if pairs:
            vec = farfield_oracle.radiation_vectors_pairs(*F, x, y, WL, 1.459, ux, uy)
            for k, w in zip(FF_KEYS[:4], vec):
                assert rel(got[k], w) < TOL, (desc, k)
        else:
            want = farfield_oracle.farfield_direct(*F, x, y, WL, 1.459, ux, uy)
            for k in FF_KEYS:
                assert rel(got[k], want[k]) < TOL, (desc, k)
    elif kind == 'ffres':
        _, L, g, src, _m = desc
        x, y = grid(g)
        want = nf(L, g, src)
        fft = [np.fft.fft2(np.fft.fftshift(a)) for a in want[:4]]
        P, total = farfield_oracle.farfield_from_nearfield(*fft, x, y, WL, want[7])[:2]
        assert rel(got['P'], P) < 1e-11, desc
        assert abs(got['total_P'] - total) <= 1e-11 * abs(total), desc
    elif kind == 'hp':
        _, L, g, d, precision = desc[:5]
        x, y = grid(g)
        ux, uy, pairs = directions(d, g)
        want = nf(L, g, desc[7] if len(desc) > 7 else 0)
        if pairs:
            vec = farfield_oracle.radiation_vectors_pairs(*want[:4], x, y, WL, want[7], ux, uy)
            for k, w in zip(FF_KEYS[:4], vec):
                assert rel(got[k], w) < (TOL if precision == 'f64' else 1e-4), (desc, k)
        else:
            ff = farfield_oracle.farfield_direct(*want[:4], x, y, WL, want[7], ux, uy)
            for k in ('Nx', 'Ny', 'Lx', 'Ly', 'a_theta', 'a_phi'):
                assert rel(got[k], ff[k]) < (TOL if precision == 'f64' else 1e-4), (desc, k)
    elif kind == 'sw':
        _, L, g, d, which = desc
        x, y = grid(g)
        ux, uy, _ = directions(d, g)
        P_sum = 0
        for sx, sy, sz, pol in SOURCE_LISTS[which](L):
            want = nearfield_oracle.build_nearfield(sx, sy, sz, pol, WL, *lens_args(L), x_pts=x, y_pts=y)
            P_sum = P_sum + farfield_oracle.farfield_direct(*want[:4], x, y, WL, want[7], ux, uy)['P']
        assert rel(got['P_sum'], P_sum) < 1e-11, desc


# ---- targeted sequences ----------------------------------------------------------------------------

@pytest.fixture
def ctx():
    from metalens_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def test_two_hotpaths_on_two_lenses_take_turns(ma, ctx):
    """HotPaths on different lenses (three orders / 'physical' orders) and different grids,
    stepped A, B, A, B: each step synthesises ITS lens (HotPath re-asserts its tables and layout
    when the context's tokens are not the ones it left)"""
    pool = {}
    a = ('hp', 'A', 'sq', 'sym')
    b = ('hp', 'B', 'off', 'asym')
    for desc in (a, b, a, b):
        check(ma, ctx, pool, desc)


def test_precision_and_method_follow_each_object(ma, ctx):
    """a FarfieldTransform built first (fp64), then HotPaths in fp64 / fp32 / 'gemm' and a
    SourceSweep, interleaved: every call gives its own object's result (each object re-asserts its
    precision and method).  All share one aperture grid and one direction grid."""
    from metalens_amd import _lib
    g, d = 'sq', 'sym'
    x, y = grid(g)
    ux, uy, _ = directions(d, g)
    F = host_fields(g, 2)

    def transform(c, t):
        _upload(c, F)
        t.transform()
        out = t.radiation_vectors()
        out['P'], out['a_theta'], out['a_phi'] = t.project()
        return out

    fresh = _lib.Context(0)
    try:
        want_t = transform(fresh, ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, 1.459,
                                                       ux, uy, ctx=fresh))
    finally:
        fresh.close()
    t = ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, 1.459, ux, uy, ctx=ctx)
    pool = {}
    ops = [('hp', 'A', g, d, 'f64', 'auto'), ('hp', 'A', g, d, 'f32', 'auto'), ('hp', 'A', g, d, 'f64', 'gemm'),
           ('sw', 'A', g, d, 'single')]
    for desc in ops:                     # every object exists before any of them runs
        if desc[0] == 'hp':
            pool[desc] = make_hotpath(ma, ctx, *desc[1:])
        else:
            pool[desc] = make_sweep(ma, ctx, *desc[1:4])
    for desc in (ops[1], 't', ops[0], ops[3], ops[1], ops[2], 't', ops[1], ops[3], 't'):
        if desc == 't':
            assert_same(transform(ctx, t), want_t, 'FarfieldTransform after ' + repr(prev))
        else:
            check(ma, ctx, pool, desc)
        prev = desc


def test_a_transform_keeps_the_method_of_its_construction(ma, ctx):
    """FarfieldTransform / farfield_direct inherit the method the context had when they were BUILT:
    one built under 'fft-streamed' keeps it after the context's method has changed"""
    from metalens_amd import _lib
    g, d = 'sq', 'lat'
    x, y = grid(g)
    ux, uy, _ = directions(d, g)
    F = host_fields(g, 3)
    want = {}
    for method in ('fft-streamed', 'gemm'):
        fresh = _lib.Context(0)
        try:
            fresh.set_method(method)
            _upload(fresh, F)
            t = ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, 1.459, ux, uy, ctx=fresh)
            t.transform()
            want[method] = t.radiation_vectors()
            assert fresh.plan_kernels() == (('fft', 'fft') if method != 'gemm' else ('folded', 'folded'))
        finally:
            fresh.close()
    ctx.set_method('fft-streamed')
    ts = ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, 1.459, ux, uy, ctx=ctx)
    ctx.set_method('gemm')
    tg = ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, 1.459, ux, uy, ctx=ctx)
    ctx.set_method('auto')
    check(ma, ctx, {}, ('hp', 'A', g, 'sym'))
    for t, method in ((ts, 'fft-streamed'), (tg, 'gemm'), (ts, 'fft-streamed')):
        _upload(ctx, F)
        t.transform()
        assert_same(t.radiation_vectors(), want[method], method)
        assert ctx.plan_kernels() == (('fft', 'fft') if method != 'gemm' else ('folded', 'folded'))
    assert ctx.method == 'fft-streamed'     # (what the last transform left)


@pytest.mark.parametrize('first,second', [('small', 'big'), ('big', 'small'), ('pairs', 'big')])
def test_stale_transform_plans_again_and_never_overruns(ma, ctx, first, second):
    """t1 = FarfieldTransform(40 x 36 directions, or a pair list), t2 = FarfieldTransform(64 x 64)
    built after it: t1.transform() and its downloads give t1's own result; downloads after the
    OTHER object has planned are refused (the library copies as many elements as the active plan
    has - never into an array sized for fewer)"""
    from metalens_amd import _lib
    g = 'off'
    x, y = grid(g)
    dirs = {'small': (np.linspace(-0.3, 0.3, 40), np.linspace(-0.25, 0.2, 36), False),
            'big': directions('big', g), 'pairs': directions('pairs', g)}
    F = host_fields(g, 4)

    def make(c, which):
        ux, uy, pairs = dirs[which]
        return ma.FarfieldTransform(x.size, y.size, x[1] - x[0], y[1] - y[0], WL, 1.459, ux, uy,
                                    pair_list=pairs, ctx=c)

    def run(t):
        t.transform()
        out = t.radiation_vectors()
        out['P'], out['a_theta'], out['a_phi'] = t.project()
        return out

    want = {}
    for which in (first, second):
        fresh = _lib.Context(0)
        try:
            _upload(fresh, F)
            want[which] = run(make(fresh, which))
        finally:
            fresh.close()
    _upload(ctx, F)
    t1 = make(ctx, first)
    t2 = make(ctx, second)
    assert_same(run(t1), want[first], first)
    assert_same(run(t2), want[second], second)
    t1.transform()
    t2.transform()
    for fn in (t1.radiation_vectors, t1.project, lambda: t1.transform(accumulate=True)):
        with pytest.raises(RuntimeError, match='no longer this FarfieldTransform'):
            fn()
    assert_same(run(t1), want[first], first + ' again')
    assert_same(t1.radiation_vectors(), {k: want[first][k] for k in FF_KEYS[:4]}, first + ' download')


def test_hotpath_results_after_another_object_stepped(ma, ctx):
    """``hpA.step(); hpB.step(); hpA.results()`` returns A's own result (HotPath.results runs A's
    step again when the context's plan or near field is another object's); the transform half of
    a step after another object synthesised is refused"""
    pool = {}
    a = ('hp', 'A', 'off', 'big')
    b = ('hp', 'B', 'sq', 'asym')
    hpA = _pooled(pool, a, lambda: make_hotpath(ma, ctx, *a[1:]))
    hpB = _pooled(pool, b, lambda: make_hotpath(ma, ctx, *b[1:]))
    for first, second, desc in ((hpA, hpB, a), (hpB, hpA, b)):
        first.step()
        second.step()
        first.sync()
        r = first.results()
        assert_same({k: r[k] for k in FF_KEYS + ('power_local_rows',)}, reference(ma, desc), desc)
    hpA.queue_synthesis()
    hpB.queue_synthesis()
    with pytest.raises(RuntimeError, match='used by another object'):
        hpA.queue_transform()
    hpB.queue_transform()
    hpB.sync()
    r = hpB.results()
    assert_same({k: r[k] for k in FF_KEYS + ('power_local_rows',)}, reference(ma, b), b)


def test_one_context_through_grid_batch_and_plan_transitions(ma, ctx):
    """one context, one lens: grids (320^2 window, 200 x 136 off centre, 3 x 2050 strip, the
    320^2 window again), batches (polarisation batch, single source, position batch, single),
    junk fields between a synthesis and a resident transform, shards (mirrored, interleaved over
    two ranks, the whole aperture), plans (FFT, GEMM, a fused-premodulation HotPath, then the plain
    resident flow).  Pins the C-side zero / row-first / trim / interleave / fold keys and the
    premodulation serial through their transitions."""
    pool = {}
    seq = [('nf', 'A', 'w320', 0, True), ('nf', 'A', 'off', 0, True), ('nf', 'A', 'strip', 1, True),
           ('nf', 'A', 'w320', 0, True),
           ('sw', 'A', 'off', 'sym', 'mixed'), ('sw', 'A', 'off', 'sym', 'single'),
           ('sw', 'A', 'off', 'sym', 'mixed'), ('sw', 'A', 'off', 'sym', 'single'),
           ('nf', 'A', 'sq', 0, False), ('junk', 64, 48), ('ffres', 'A', 'sq', 0, 'auto'),
           ('junk', 300, 7), ('ffres', 'A', 'off', 1, 'auto'),
           ('shard', 'A', 'sq', 'sym', 2, 0, 'mirrored'), ('shard', 'A', 'sq', 'lat', 2, 1, 'interleaved'),
           ('shard', 'A', 'sq', 'sym', 1, 0, 'auto'), ('shard', 'A', 'sq', 'sym', 2, 1, 'mirrored'),
           ('shard', 'A', 'sq', 'lat', 2, 0, 'interleaved'),
           ('hp', 'A', 'sq', 'lat', 'f64', 'auto'), ('hp', 'A', 'sq', 'lat', 'f64', 'gemm'),
           ('hp', 'A', 'sq', 'sym', 'f64', 'auto', True), ('ffres', 'A', 'sq', 0, 'auto'),
           ('hp', 'A', 'sq', 'sym', 'f64', 'auto', True), ('nf', 'A', 'sq', 0, True)]
    for desc in seq:
        got = check(ma, ctx, pool, desc)
        if desc[0] == 'shard':
            assert got['sharding'].startswith({'mirrored': 'mirrored', 'interleaved': 'interleaved',
                                               'auto': 'whole'}[desc[6]]), (desc, got['sharding'])


def test_lens_class_and_tie_answers_between_syntheses(ma, ctx):
    """the lens-class edge: ONE layout (lens A's) and one grid, the ring tables' order sets changed under it -
    simple (every table the order-list kernels'), an order (0, 1) in every ring table (the rings through the general
    kernel), one collection of each, simple again.  Neither the grid nor the layout serial moves, so only the class
    event (synth_caches.h lens_class_changed) drops the patch lists and the zeros outside the lens.  Then the tie edge:
    a grid with exact nearest-cell ties (answered inside build_nearfield), another grid, the tie grid again - the
    answers are dropped with their (grid, layout) and given anew."""
    from oracle import nearfield_oracle
    assert len(lens('A')['lens_periphery_summary']['gratingcollection_list']) == 2
    pool, infos, tokens = {}, [], []
    for L in ('A', 'G', 'M', 'A'):
        for _ in range(2):               # (the second finds the zeros stored and launches the patch lists)
            check(ma, ctx, pool, ('nf', L, 'off', 0, True))
        infos.append(ctx.nearfield_kernels())
        tokens.append(ctx.layout_token)
    assert [i['family'] for i in infos] == ['orders-along-x', 'mixed', 'mixed', 'orders-along-x'], infos
    assert [i['ring_orders_max'] for i in infos] == [3, 0, 3, 3], infos     # (all rings general; one collection simple)
    assert tokens[0] is not None and len(set(tokens)) == 1, tokens       # the layout was not uploaded again
    dec = {}
    x, y = grid('tie')
    nearfield_oracle.build_nearfield(*source('A', 0), WL, *lens_args('A'), x_pts=x, y_pts=y, decisions=dec)
    assert np.count_nonzero(dec['nearest_tie']) > 0     # the grid really has ties
    for g in ('tie', 'off', 'tie', 'tie'):
        check(ma, ctx, pool, ('nf', 'A', g, 0, True))


def _as_table_object(ns, centre):
    """the fixture's table (tests/golden_io.py keeps the packed grids and the ORDER SET of the
    characterisation records, not the records) as this package's GratingCollection / HexGridSet:
    one record per order, zero amplitudes - build_nearfield reads the orders from the records and
    every value from the packed grids, which the file carries as they are"""
    from metalens_amd.grating import Grating, GratingCollection
    from metalens_amd.lens_center import HexGridSet
    g0 = ns.grating_list[0]
    wl_nm = sorted(ns.interpolators)[0][0]
    recs = [dict({'wavelength_in_nm': float(wl_nm), 'ux': 0.0, 'uy': 0.0, 'ox': e['ox'], 'oy': e['oy'],
                  'x_or_y': 'x'}, **{a: 0j for a in ('ampfy', 'ampfx', 'ampry', 'amprx')}) for e in g0.data]
    g = Grating(lateral_period=g0.lateral_period, cyl_height=0.0, grating_period=g0.grating_period,
                n_glass=g0.n_glass, data=recs)
    if centre:
        obj = HexGridSet(sep=g0.lateral_period, cyl_height=0.0, n_glass=g0.n_glass, grating_list=[g])
    else:
        obj = GratingCollection(target_wavelength=wl_nm * 1e-9, lateral_period=g0.lateral_period,
                                lens_type='round', grating_list=[g])
    obj.interpolators = dict(ns.interpolators)
    obj.interpolator_bounds = ns.interpolator_bounds
    return obj


@pytest.mark.parametrize('warm', [True, False])
def test_tables_read_back_from_the_table_file(ma, tmp_path, warm):
    """lens B's collections and centre set written with tablefile.save and read back with
    tablefile.load drive build_nearfield on three golden windows to the golden fields (1e-12, no
    flips).  On a context where the original objects are resident this is a content hit: the
    tables token does not change (no upload)."""
    from metalens_amd import _lib, tablefile
    from test_gpu_parity import case_args
    names = ('nearfield_B_center_offaxis_z.npz', 'nearfield_B_periphery_onaxis_x.npz',
             'nearfield_B_straddle_plane_y.npz')
    cases = [np.load(golden_io.golden_path(n)) for n in names]
    S, cells, hgs = golden_io.load_lens(golden_io.golden_path(str(cases[0]['lens'])))
    paths = []
    for k, gc in enumerate(S['gratingcollection_list']):
        paths.append(str(tmp_path / ('gc%d.npz' % k)))
        tablefile.save(paths[-1], _as_table_object(gc, centre=False))
    tablefile.save(str(tmp_path / 'hgs.npz'), _as_table_object(hgs, centre=True))
    S2 = dict(S)
    S2['gratingcollection_list'] = [tablefile.load(p) for p in paths]
    hgs2 = tablefile.load(str(tmp_path / 'hgs.npz'))
    ctx = _lib.Context(0)
    try:
        if warm:
            ma.build_nearfield(**case_args(cases[0], ctx=ctx))
            token = ctx.tables_token
            assert token is not None
        for case in cases:
            out = ma.build_nearfield(**case_args(case, lens_periphery_summary=S2, hexgridset=hgs2, ctx=ctx))
            if warm:
                assert ctx.tables_token == token
            for got, key in zip(out[:4], F_KEYS):
                err, flips = field_errors(got, case[key])
                assert flips == 0, (key, flips)
                assert err < TOL, (key, err)
            assert abs(out[6] - case['power']) <= 1e-12 * abs(case['power'])
    finally:
        ctx.close()


def _sweep_sums(ctx, n, shape):
    from metalens_amd import _lib
    ctx.sync()
    P = np.empty(shape)
    total = np.zeros(n)
    _lib.check(ctx.lib.ml_farfield_sums(ctx.handle, _lib.dptr(P), _lib.dptr(total), None, n))
    return {'P_sum': P, 'total_P': total}


def test_in_place_table_edit(ma, ctx):
    """one table of a resident lens edited in place: build_nearfield sees the new content and equals
    a fresh context on the edited lens; a PreparedLens and SourceSweep.queue do NOT see it until
    refresh() / prepare() (their documented contract), and then they do"""
    from metalens_amd import _lib
    L = _synthetic_lens(20e-6, 0.35, WL, switch_deg=9.0)     # a private copy: edited below
    args = (L['lens_periphery_summary'], L['lens_center_summary'], L['hexgridset'])
    x, y = grid('off')
    u = np.linspace(-0.2, 0.2, 40)
    src = source('A', 0)
    sources = [src]

    def nf(c, lens_arg=None):
        a = (lens_arg, None, None) if lens_arg is not None else args
        out = ma.build_nearfield(*src, WL, *a, x_pts=x, y_pts=y, ctx=c)
        return dict({'power': out[6]}, **{k: np.array(v) for k, v in zip(F_KEYS, out[:4])})

    def swept(c, sw):
        sw.queue(sources)
        return _sweep_sums(c, 1, (u.size, u.size))

    def fresh_results():
        c = _lib.Context(0)
        try:
            sw = ma.SourceSweep(WL, *args, x, y, u, u, ctx=c)
            sw.run(sources)
            return nf(c), swept(c, sw)
        finally:
            c.close()

    before = fresh_results()
    p = ma.PreparedLens(*args, WL, ctx=ctx)
    sw = ma.SourceSweep(WL, *args, x, y, u, u, ctx=ctx)
    sw.run(sources)
    assert_same(nf(ctx, p), before[0], 'prepared, before the edit')
    gc = args[0]['gratingcollection_list'][0]
    for key, f in gc.interpolators.items():
        if key[0] == 580:
            f.values[...] = np.asarray(f.values) * 1.25
    after = fresh_results()
    assert not np.array_equal(after[0]['Ex'], before[0]['Ex'])
    # not seen until refresh() / prepare()
    assert_same(nf(ctx, p), before[0], 'prepared, edited, not refreshed')
    assert_same(swept(ctx, sw), before[1], 'queued sweep, edited, not prepared')
    p.refresh()
    assert_same(nf(ctx, p), after[0], 'prepared, refreshed')
    sw.prepare()
    assert_same(swept(ctx, sw), after[1], 'queued sweep, prepared')
    # the plain drop-in hashes the caller's arrays on every call
    assert_same(nf(ctx), after[0], 'build_nearfield')


# ---- the random walk --------------------------------------------------------------------------------------

def _vocabulary():
    ops = []
    for L in ('A', 'B'):
        for g in ('sq', 'off', 'strip'):
            ops += [('nf', L, g, 0, True), ('nf', L, g, 1, False), ('pl', L, g, 0)]
        ops += [('ffres', L, 'off', 0, None)]
    for g in ('sq', 'off'):
        for d in ('lat', 'sym', 'asym', 'pairs'):
            ops.append(('ffd', g, d, 5, None))
    ops += [('ffd', 'strip', 'sym', 5, None)]
    hps = [('hp', 'A', 'sq', 'lat', 'f64', 'auto'), ('hp', 'B', 'off', 'sym', 'f64', 'auto'),
           ('hp', 'A', 'off', 'pairs', 'f64', 'auto'), ('hp', 'B', 'sq', 'asym', 'f32', 'auto'),
           ('hp', 'A', 'sq', 'sym', 'f64', 'gemm', False)]
    ops += hps
    ops += [('sw', 'A', 'off', 'sym', 'mixed'), ('sw', 'B', 'sq', 'asym', 'single')]
    ops += [('junk', 64, 48), ('junk', 256, 256), ('method', 'auto'), ('method', 'gemm'),
            ('precision', 'f32'), ('precision', 'f64')]
    return ops, hps


_ORACLE_DONE = set()


@pytest.mark.parametrize('seed', [1, 2, 3, 4])
def test_random_walk_on_one_context(ma, ctx, seed):
    """seeded random sequences of 40 operations on one long-lived context, every result bit for bit
    the fresh context's; the first occurrence of each operation kind also against the oracle"""
    ops, hps = _vocabulary()
    rng = np.random.default_rng(seed)
    pool = {}
    for desc in hps:                     # pooled HotPaths, built before the walk
        pool[desc] = make_hotpath(ma, ctx, *desc[1:])
    walk = []
    for _ in range(40):
        desc = ops[rng.integers(len(ops))]
        if desc[0] in INHERITS_METHOD:
            desc = desc[:-1] + (ctx.method,)
        walk.append(desc)
        try:
            got = check(ma, ctx, pool, desc)
        except AssertionError as e:
            raise AssertionError('walk %d, step %d: %s\nsequence: %s' % (seed, len(walk), e, walk))
        kind = desc[0] + ('' if desc[0] != 'nf' else str(desc[4])) + (desc[4] if desc[0] == 'hp' else '')
        if got is not None and kind not in _ORACLE_DONE:
            oracle_check(desc, got)
            _ORACLE_DONE.add(kind)
