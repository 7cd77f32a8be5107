"""examples/focal_plane.py runs as written (GPU) and finds the focus where the wave was aimed"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_focal_plane_example_finds_the_focus():
    spec = importlib.util.spec_from_file_location('focal_plane', os.path.join(ROOT, 'examples', 'focal_plane.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(verbose=False)
    assert out['peak_xy'] == (30, 30) and out['peak_xz'] == (30, 40)
    # energy: what crosses a patch of the focal plane is a part of what left the pupil
    assert 0 < out['power_through_patch'] < out['power_in_pupil']
