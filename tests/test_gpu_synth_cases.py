"""Every case of tests/synth_cases.py - inputs the census (test_synth_cases.py) shows to reach the second and third
staging rounds of the ring kernels and the general kernel, every pass count of the wide instantiation, waves with
two collections and partial patches - on the GPU against the CPU oracle: the same zero pattern, fields within
TOL = 1e-12 of the oracle's peak, the incident power to 1e-12, the kernel family the case names.  Each window is
synthesised twice: the first synthesis of a geometry runs over the whole grid, the second from the patch lists.
Needs an MI355X: run with ``-m gpu``."""
import numpy as np
import pytest

import synth_cases
from synth_cases import CASES

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope='module')
def ma():
    import metalens_amd
    return metalens_amd


_WANT = {}


def oracle(name, pol):
    """the oracle's fields and power of a case, computed once per polarisation and left unchanged"""
    if (name, pol) not in _WANT:
        from oracle import nearfield_oracle
        case = CASES[name]
        want = nearfield_oracle.build_nearfield(**synth_cases.call_args(case, synth_cases.make_lens(case.lens), pol))
        for w in want[:4]:
            w.setflags(write=False)
        _WANT[name, pol] = want
    return _WANT[name, pol]


def compare_fields(got, want, what):
    scale = max(np.abs(w).max() for w in want[:4])
    assert scale > 0
    for key, g, w in zip(('Ex', 'Ey', 'Hx', 'Hy'), got[:4], want[:4]):
        flips = int(np.count_nonzero((g == 0) != (w == 0)))
        err = np.abs(g - w).max() / scale
        print(what, key, 'flips', flips, 'error / peak %.2e' % err)
        assert flips == 0, (what, key, flips)
        assert err <= TOL, (what, key, err)


@pytest.mark.parametrize('name', sorted(CASES))
def test_synthesis_cases_vs_oracle(ma, name):
    from metalens_amd import _lib
    case = CASES[name]
    lens = synth_cases.make_lens(case.lens)
    for pol in case.pols:
        args = synth_cases.call_args(case, lens, pol)
        want = oracle(name, pol)
        for attempt in ('full-grid', 'listed'):
            got = ma.build_nearfield(**args)
            assert _lib.default_context().nearfield_kernels()['family'] == case.family
            compare_fields(got, want, (name, pol, attempt))
            assert abs(got[6] - want[6]) <= 1e-12 * abs(want[6]), (name, pol, attempt)


@pytest.mark.parametrize('name', sorted(n for n, c in CASES.items() if c.batch))
def test_synthesis_cases_polarisation_batch_vs_oracle(ma, name):
    """the batch kernels (x, y and z in one pass) on one multi-round case per kernel, member by member"""
    from metalens_amd import _lib
    from metalens_amd.nearfield import nearfield_params
    case = CASES[name]
    lens = synth_cases.make_lens(case.lens)
    pols = 'xyz'
    args = synth_cases.call_args(case, lens, pols[0])
    ctx = _lib.default_context()
    first = ma.build_nearfield(ctx=ctx, **args)   # uploads tables and layout
    params = (_lib.NearfieldParams * len(pols))()
    for m, pol in enumerate(pols):
        params[m] = nearfield_params(args['source_x'], args['source_y'], args['source_z'], pol, args['wavelength'],
                                     first[7], 1e-30, ma.constants.c0, ma.constants.Z0)
    xs, ys = _lib.f64(args['x_pts']), _lib.f64(args['y_pts'])
    _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, len(pols), _lib.dptr(xs), xs.size,
                                                _lib.dptr(ys), ys.size))
    got = {}
    for m, pol in enumerate(pols):
        _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
        F = [np.empty((xs.size, ys.size), dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(f) for f in F]))
        got[pol] = F
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))
    assert ctx.nearfield_kernels()['family'] == case.family
    for pol in pols:
        compare_fields(got[pol], oracle(name, pol), (name, 'batch', pol))
