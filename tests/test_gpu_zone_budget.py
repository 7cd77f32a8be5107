"""examples/zone_budget.py on a small lens: the table's numbers are those of the twin on the downloaded field.  Needs an
MI355X."""
import importlib.util
import os

import numpy as np
import pytest

import fields_zones_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_zone_budget_example():
    from metalens_amd import _lib
    spec = importlib.util.spec_from_file_location('zone_budget', os.path.join(ROOT, 'examples', 'zone_budget.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(radius=30e-6, verbose=False)
    K = out['edges'].size
    assert K >= 5 and (np.diff(out['edges']) > 0).all()
    for name in ('on_axis', 'off_axis'):
        z = out[name]
        assert z['samples'].shape == (K,) and (z['samples'] > 0).all() and z['P'].shape == (1, K) and z['coherence'].shape == (1, K, 2)
        assert (z['P'] > 0).all() and z['P'].sum() < z['power_in']          # a passive lens: no more leaves than arrives
        assert ((z['coherence'] >= 0) & (z['coherence'] <= 1 + 1e-9)).all()
    assert out['on_axis']['reference'] == (0.0, 0.0) and out['off_axis']['reference'][0] < 0
    # the off-axis field is the one left resident: its table against the yardstick on the download
    z = out['off_axis']
    ctx = _lib.default_context()
    F = [np.empty((z['x'].size, z['y'].size), dtype=np.complex128) for _ in range(4)]
    _lib.check(ctx.lib.ml_fields_download(ctx.handle, *[_lib.dptr(a) for a in F]))
    want = ref.exact(np.stack(F)[None], z['x'], z['y'], 580e-9, z['n_glass'], out['edges'], reference=('plane',) + z['reference'])
    ref.hold('gpu zone_budget example', z, want)
