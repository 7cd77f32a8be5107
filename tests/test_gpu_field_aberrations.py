"""examples/field_aberrations.py on a small lens: the table's numbers are those of the yardstick on the downloaded field.
Needs an MI355X."""
import importlib.util
import os

import numpy as np
import pytest

import fields_wavefront_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_field_aberrations_example(capsys):
    from metalens_amd import _lib
    spec = importlib.util.spec_from_file_location('field_aberrations', os.path.join(ROOT, 'examples', 'field_aberrations.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(radius=30e-6, verbose=True)
    said = capsys.readouterr().out
    # one line per term up to order 4 and the rms, for both emitters
    assert said.count('spherical') == 2 and said.count('coma x') == 2 and said.count('defocus') == 2 and said.count('rms wavefront') == 2
    assert len(mod.NAMES) == 15 and len(said.splitlines()) == 2 * (3 + 15)
    for name in ('on_axis', 'off_axis'):
        w = out[name]
        assert w['terms'].shape == (15, 2) and w['moments'].shape == (1, 2, 15) and w['samples'] > 1000 and w['outside'] > 0
        assert 0 < w['P'][0] < w['power_in']                                # a passive lens: no more leaves than arrives
        assert ((w['coherence'] >= 0) & (w['coherence'] <= 1 + 1e-9)).all() and np.isfinite(w['rms']).all()
    assert out['on_axis']['reference'] == (0.0, 0.0) and out['off_axis']['reference'][0] < 0
    # the off-axis field is the one left resident: its table against the yardstick on the download
    w = out['off_axis']
    ctx = _lib.default_context()
    F = [np.empty((w['x'].size, w['y'].size), dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    want = ref.exact(np.stack(F)[None], w['x'], w['y'], 580e-9, w['n_glass'], out['pupil'], 4, reference=('plane',) + w['reference'])
    ref.hold('gpu field_aberrations example', w, want)
