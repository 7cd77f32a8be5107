"""The fixed-shape synthesis kernels (metalens_amd/csrc/nearfield_simple.hip FIXED3: the narrow ring instantiation and
the centre kernel for tables of exactly three present order slots, one dipole) against the general kernels they replace
in the steady-state launch from the patch lists (csrc/lens_pack.h fixed3_takes), bit for bit, and against the CPU oracle
within the tolerance of test_gpu_synth_cases.py.  Needs an MI355X.

Which form a launch takes is the library's choice per process (METALENS_HIP_FIXED_SYNTH=0: the general kernels for every
call), read once, so each variant runs in a fresh child process: this file as a script, which synthesises every window of
tests/synth_fixed_cases.py twice - the first synthesis of a geometry runs over the whole grid, the second from the lists -
and writes the four field planes and the incident power of the second, with the forms ml_nearfield_synth_info reported
after each.  test_synth_fixed_route.py holds the census to the paths each window claims: a patch of exactly eight blocks,
second and third rounds at capacity eight, two collections in a wave with equal and with different lowest orders,
partial patches on both far sides, patches that the ring and the centre kernel both store into.

The launches outside the conditions - a three-polarisation batch, a plane wave, a lens with one two-slot collection -
run in the same children: they report the general form in both and must not change either."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ('Ex', 'Ey', 'Hx', 'Hy')
VARIANTS = {'default': {}, 'general': {'METALENS_HIP_FIXED_SYNTH': '0'}}


def other_args(name):
    """build_nearfield's arguments for the window's dipole, and whether the launch under test is a plane wave instead"""
    import synth_cases
    import synth_fixed_cases
    spec, window, z = synth_fixed_cases.OTHERS[name]
    case = synth_fixed_cases.CASES[window][0]._replace(lens=spec)
    return synth_cases.call_args(case, synth_cases.make_lens(spec)), z is None


def run_cases(out_path):
    """(child process) every window and the launches outside the conditions, raw planes to out_path"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import metalens_amd as ma
    import synth_cases
    import synth_fixed_cases
    from metalens_amd import _lib
    from metalens_amd.nearfield import nearfield_params
    ctx = _lib.default_context()
    out = {}

    def twice(key, args):
        forms = []
        for attempt in range(2):
            got = ma.build_nearfield(ctx=ctx, **args)
            forms.append(ctx.synth_forms())
        assert ctx.nearfield_kernels()['family'] == 'orders-along-x'
        for plane, a in zip(PLANES, got[:4]):
            out['%s/%s' % (key, plane)] = np.array(a)
        out[key + '/power'] = np.float64(got[6])
        out[key + '/forms'] = np.array(json.dumps(forms))
        return got

    for name, (case, _) in synth_fixed_cases.CASES.items():
        twice(name, synth_cases.call_args(case, synth_cases.make_lens(case.lens)))
    def plane_wave_twice(key, args):
        """normal incidence lies outside these ring tables' range of directions: build_nearfield raises the reference's
        ValueError for it, the kernels evaluate the tables' edge cells - ml_nearfield itself, the reports left unread"""
        n_glass = ma.build_nearfield(ctx=ctx, **args)[7]   # (the dipole: uploads the lens)
        p = nearfield_params(args['source_x'], args['source_y'], -math.inf, 'x', args['wavelength'],
                             n_glass, 1e-30, ma.constants.c0, ma.constants.Z0)
        assert p.plane_wave == 1
        xs, ys = _lib.f64(args['x_pts']), _lib.f64(args['y_pts'])
        power, n_viol, forms = _lib.c_double(0), _lib.c_int(0), []
        for attempt in range(2):
            _lib.check(ctx.lib.ml_nearfield(ctx.handle, _lib.byref(p), _lib.dptr(xs), xs.size, _lib.dptr(ys), ys.size,
                                            _lib.byref(power), None, 0, _lib.byref(n_viol)))
            forms.append(ctx.synth_forms())
        F = [np.empty((xs.size, ys.size), dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(f) for f in F]))
        for plane, a in zip(PLANES, F):
            out['%s/%s' % (key, plane)] = a
        out[key + '/power'] = np.float64(power.value)
        out[key + '/forms'] = np.array(json.dumps(forms))

    for name in synth_fixed_cases.OTHERS:
        args, plane_wave = other_args(name)
        (plane_wave_twice if plane_wave else twice)('other/' + name, args)
    # the three-polarisation batch on a window the fixed kernels take one source at a time
    case = synth_fixed_cases.CASES[synth_fixed_cases.BATCH_CASE][0]
    args = synth_cases.call_args(case, synth_cases.make_lens(case.lens))
    first = twice('batch/single', args)
    params = (_lib.NearfieldParams * 3)()
    for m, pol in enumerate('xyz'):
        params[m] = nearfield_params(args['source_x'], args['source_y'], args['source_z'], pol, args['wavelength'],
                                     first[7], 1e-30, ma.constants.c0, ma.constants.Z0)
    xs, ys = _lib.f64(args['x_pts']), _lib.f64(args['y_pts'])
    forms = []
    for attempt in range(2):
        _lib.check(ctx.lib.ml_nearfield_batch_async(ctx.handle, params, 3, _lib.dptr(xs), xs.size, _lib.dptr(ys), ys.size))
        forms.append(ctx.synth_forms())
    for m, pol in enumerate('xyz'):
        _lib.check(ctx.lib.ml_fields_select(ctx.handle, m))
        F = [np.empty((xs.size, ys.size), dtype=np.complex128) for _ in range(4)]
        _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(f) for f in F]))
        for plane, a in zip(PLANES, F):
            out['batch/%s/%s' % (pol, plane)] = a
    _lib.check(ctx.lib.ml_fields_select(ctx.handle, 0))
    out['batch/forms'] = np.array(json.dumps(forms))
    np.savez(out_path, **out)


if __name__ == '__main__':
    run_cases(sys.argv[1])
    sys.exit(0)

import synth_cases  # noqa: E402
import synth_fixed_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """{variant: the arrays its child process wrote}; one process at a time"""
    base = {k: v for k, v in os.environ.items() if k != 'METALENS_HIP_FIXED_SYNTH'}
    got = {}
    for name, extra in VARIANTS.items():
        path = str(tmp_path_factory.mktemp('synth_fixed') / (name + '.npz'))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(base, **extra),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (name, p.stdout[-1000:], p.stderr[-3000:])
        with np.load(path) as z:
            got[name] = {k: z[k] for k in z.files}
    return got


def forms_of(run, key):
    return json.loads(str(run[key + '/forms']))


def assert_same_bits(runs, key):
    ref, got = runs['general'][key], runs['default'][key]
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert np.array_equal(got.view(np.float64), ref.view(np.float64)), key


_WANT = {}


def oracle(name):
    """the oracle's fields and power of a window, computed once and left unchanged"""
    if name not in _WANT:
        from oracle import nearfield_oracle
        case = synth_fixed_cases.CASES[name][0]
        want = nearfield_oracle.build_nearfield(**synth_cases.call_args(case, synth_cases.make_lens(case.lens)))
        for w in want[:4]:
            w.setflags(write=False)
        _WANT[name] = want
    return _WANT[name]


@pytest.mark.parametrize('name', sorted(synth_fixed_cases.CASES))
def test_fixed_kernels_equal_the_general_kernels_bit_for_bit(runs, name):
    from test_gpu_synth_cases import compare_fields
    claims = synth_fixed_cases.CASES[name][1]
    # the first synthesis of a geometry runs the general kernels over the whole grid, the second the fixed-shape ones
    # from the lists - and the general ones where the switch is off
    first, second = forms_of(runs['default'], name)
    print(name, 'default', first, second, 'switch off', forms_of(runs['general'], name))
    assert first['ring'] == 'general' and second['ring'] == 'fixed3'
    assert first['centre'] in (None, 'general') and second['centre'] in (None, 'fixed3')
    if 'ring-and-centre' in claims:
        assert (first['centre'], second['centre']) == ('general', 'fixed3')
    for forms in forms_of(runs['general'], name):
        assert forms['ring'] == 'general' and forms['centre'] in (None, 'general')
    for plane in PLANES:
        assert_same_bits(runs, '%s/%s' % (name, plane))
    assert_same_bits(runs, name + '/power')
    want = oracle(name)
    compare_fields([runs['default']['%s/%s' % (name, plane)] for plane in PLANES], want, (name, 'fixed3'))
    power = float(runs['default'][name + '/power'])
    assert abs(power - want[6]) <= 1e-12 * abs(want[6]), (name, power, want[6])


@pytest.mark.parametrize('name', sorted(synth_fixed_cases.OTHERS))
def test_launches_outside_the_conditions_keep_the_general_kernels(runs, name):
    key = 'other/' + name
    for variant in VARIANTS:
        for forms in forms_of(runs[variant], key):
            assert forms['ring'] == 'general' and forms['centre'] in (None, 'general'), (variant, forms)
    for plane in PLANES:
        assert_same_bits(runs, '%s/%s' % (key, plane))
        assert np.abs(runs['default']['%s/%s' % (key, plane)]).max() > 0
    assert_same_bits(runs, key + '/power')


def test_a_polarisation_batch_keeps_the_general_kernels(runs):
    # (one source at a time the same window takes the fixed-shape kernels)
    assert forms_of(runs['default'], 'batch/single')[1]['ring'] == 'fixed3'
    for variant in VARIANTS:
        for forms in forms_of(runs[variant], 'batch'):
            assert forms['ring'] == 'general' and forms['centre'] in (None, 'general'), (variant, forms)
    for pol in 'xyz':
        for plane in PLANES:
            assert_same_bits(runs, 'batch/%s/%s' % (pol, plane))
    # member x of the batch against the single-source run of the same window (the fixed-shape kernels): same oracle
    from test_gpu_synth_cases import compare_fields
    case = synth_fixed_cases.CASES[synth_fixed_cases.BATCH_CASE][0]
    assert case.pols == 'x'
    compare_fields([runs['default']['batch/x/' + plane] for plane in PLANES], oracle(synth_fixed_cases.BATCH_CASE), ('batch', 'x'))
