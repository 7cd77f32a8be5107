"""examples/corrected_collimator.py on a small lens: the correction lowers the rms wavefront, the incident power is the
same in both columns, and the corrected record is that of the sweep run by hand with the same pupil.  Needs an MI355X."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_corrected_collimator_example(capsys):
    spec = importlib.util.spec_from_file_location('corrected_collimator', os.path.join(ROOT, 'examples', 'corrected_collimator.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(radius=30e-6, verbose=True)
    said = capsys.readouterr().out
    assert said.count('measured') == 1 and said.count('corrected') == 1 and len(said.splitlines()) == 8
    m, c = out['measured'], out['corrected']
    print(said)
    assert m['power_in'] == c['power_in'] > 0                           # the incident power is not the pupil's business
    assert np.isfinite(m['rms']) and c['rms'] < m['rms'] and c['strehl'] >= m['strehl']
    ap = out['pupil_object']
    assert ap.n_max == 4 and not ap.stop and ap._c[0] == 0 and np.allclose(ap._c[1:], -m['wavefront'][1:], rtol=0, atol=0)
    assert ((c['cone_fraction'] > 0) & (c['cone_fraction'] <= 1)).all()
