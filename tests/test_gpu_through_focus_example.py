"""examples/through_focus.py runs as written (GPU): one 'fft-stack' plan over 33 planes finds the focus where the wave was
aimed - the plane at the focal length, on the axis - and a depth of focus inside the stack"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_through_focus_example_finds_the_focus():
    spec = importlib.util.spec_from_file_location('through_focus', os.path.join(ROOT, 'examples', 'through_focus.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(verbose=False)
    assert out['shape'] == (33, 49, 49) and out['xz_cut'].shape == (49, 33)
    # plane 16 of 33 is z = f, sample 24 of 49 the axis (examples/focal_plane.py finds the same focus with a point list)
    assert out['brightest_plane'] == 16 and out['peak_xyz'] == (16, 24, 24) and out['z_brightest'] == out['f']
    # on-axis |E|^2 stays above half its peak over about lambda / (n (1 - cos theta)) = 3 um; the stack spans 4.8 um
    assert 1.5e-6 < out['depth_of_focus'] < 4.5e-6
