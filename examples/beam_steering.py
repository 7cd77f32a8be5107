"""Beam steering of a collimator: a dipole behind a synthetic lens is stepped off axis, and for every position the far
field is reduced ON THE GPU to where the beam points, how wide it is and how much of the incident power falls inside two
cones about its own peak - one ``SourceSweep.run(beam_cones=...)`` over all positions, one record of 44 doubles per
position; no far-field map of a single position is downloaded and nothing synchronises between the positions (needs an
MI355X and the built library).

    python examples/beam_steering.py

The pointing direction is the centroid of ``P dux duy`` in direction cosines (in the glass), the RMS divergence the root
of the central second moments ``xx + yy``; ``beam_sum`` would be the same record of the incoherent sum ``P_sum``."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(radius=50e-6, numerical_aperture=0.5, wavelength=580e-9, positions=5, step=1.5e-6, verbose=True):
    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design,
                               radius=radius, numerical_aperture=numerical_aperture, wavelength=wavelength,
                               periphery_orders='physical')
    f = lens['source_distance']
    periphery, centre, hgs = lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset']
    # the reference's default sample grid, from the drop-in call (the near field stays on the GPU)
    x, y = ma.build_nearfield(0, 0, -f, 'x', wavelength, periphery, centre, hgs, download=False)[4:6]
    # directions: a window about the axis wide enough for the steered beam, any grid will do (not the FFT lattice)
    u = np.linspace(-0.16, 0.16, 129)
    sweep = ma.SourceSweep(wavelength, periphery, centre, hgs, x, y, u, u)
    cones = (math.sin(math.radians(1.0)), math.sin(math.radians(3.0)))
    offset = step * np.arange(positions)
    res = sweep.run([(dx, 0.0, -f, 'x') for dx in offset], beam_cones=cones)      # one pass over all positions
    b = res['beam']                                                                # leading axis: the positions
    out = {'f': f, 'n_glass': sweep.n_glass, 'du': u[1] - u[0], 'offset': offset, 'pointing': b['centroid_u'], 'peak_u': b['peak_u'],
           'rms_divergence': np.sqrt(b['second_moments_u'][:, 0] + b['second_moments_u'][:, 1]),
           'cone_fraction': res['beam_efficiency']}
    if verbose:
        for k, dx in enumerate(offset):
            print('emitter %4.1f um off axis: beam points to (%+.4f, %+.4f), peak at (%+.4f, %+.4f), rms divergence %.4f; '
                  '%.1f %% of the incident power within 1 degree of the peak, %.1f %% within 3'
                  % (dx * 1e6, *out['pointing'][k], *out['peak_u'][k], out['rms_divergence'][k], *(100 * out['cone_fraction'][k])))
    return out


if __name__ == '__main__':
    main()
