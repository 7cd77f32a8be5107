"""examples/zone_phasors.py at a small size: its table is that of the host twin on the same field, and re-phasing reaches
``aligned``.  Needs an MI355X."""
import importlib.util
import os

import numpy as np
import pytest

import propagate_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_zone_phasors_example(capsys):
    from metalens_amd import postprocess
    spec = importlib.util.spec_from_file_location('zone_phasors', os.path.join(ROOT, 'examples', 'zone_phasors.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(n=96, zones=6, verbose=True)
    said = capsys.readouterr().out
    assert len(said.splitlines()) == 2 + 6 + 1 and said.count('|p^H E|') == 1 and 'aligned' in said
    before, after = out['before'], out['after']
    assert (before['samples'] > 0).all() and before['outside'] > 0 and before['E'].shape == (1, 6, 3, 1)
    # the corrected aperture reaches the ceiling: the outside is dark (the corners of the grid) and every zone is aligned
    assert out['amplitude_before'] < out['amplitude_after'] <= out['aligned'] * (1 + 1e-12)
    assert abs(out['amplitude_after'] - out['aligned']) <= 1e-9 * out['aligned']
    assert np.abs(after['phase']).max() < 1e-9 and np.abs(before['phase']).max() > 0.1
    # the table against the host twin on the field the example uploaded
    x, f, edges, err = out['x'], out['f'], out['edges'], out['error']
    k, Z = 2 * np.pi * out['n_glass'] / 580e-9, propagate_ref.Z0_SI / out['n_glass']
    r2 = x[:, None] ** 2 + x[None, :] ** 2
    zone = np.searchsorted(edges * edges, r2, side='left')
    Ex = np.where(r2 <= x.max() ** 2, np.exp(-1j * k * np.sqrt(r2 + f * f) + 1j * err[np.minimum(zone, 5)]), 0)
    twin = postprocess.zone_fields(Ex, 0 * Ex, 0 * Ex, Ex / Z, x, x, 580e-9, out['n_glass'], edges, [[0.0, 0.0, f]], Z0=propagate_ref.Z0_SI)
    assert np.array_equal(twin['samples'], before['samples'])
    scale = np.abs(twin['E']).max()
    assert np.abs(twin['E'] - before['E']).max() <= 1e-11 * scale and np.abs(twin['gradient'] - before['gradient']).max() <= 1e-10 * scale ** 2
    assert np.abs(np.angle(np.exp(1j * (twin['phase'] - before['phase'])))).max() <= 1e-10
