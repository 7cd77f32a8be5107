"""Aberrations of a collimator: what the wavefront behind the lens looks like against the collimated target wave, term by
term.  The near field of an emitter at the focus, and of one 2 um off axis, stays on the GPU and is reduced there to the
Zernike moments of its wavefront over the lens's aperture; one line per term up to radial order 4 - piston, tilts,
defocus, astigmatism, coma, trefoil, spherical - and the rms, nothing but 64 doubles per field crosses PCIe (needs an
MI355X and the built library).

    python examples/field_aberrations.py

The lens is the one of readme_flow.py and zone_budget.py.  The target of the off-axis emitter is the plane wave towards
the direction its chief ray takes in the glass, (ux, uy) = -(dx, dy) / sqrt(dx^2 + dy^2 + f^2) / n_glass.  The column
`wavefront` is the small-aberration reading Im(moment_j / moment_0) in radians: no phase is unwrapped and nothing is fitted,
so it is a faithful coefficient only while the aberration stays well below a radian; `|moment|` is the magnitude of the
complex moment relative to the piston's, which holds at any strength."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = {(0, 0): 'piston', (1, -1): 'tilt y', (1, 1): 'tilt x', (2, -2): 'astigmatism 45', (2, 0): 'defocus', (2, 2): 'astigmatism 0',
         (3, -3): 'trefoil y', (3, -1): 'coma y', (3, 1): 'coma x', (3, 3): 'trefoil x', (4, -4): 'quadrafoil 22', (4, -2): 'astigmatism 45, 2nd',
         (4, 0): 'spherical', (4, 2): 'astigmatism 0, 2nd', (4, 4): 'quadrafoil 0'}


def main(radius=100e-6, numerical_aperture=0.5, wavelength=580e-9, offset=2e-6, verbose=True):
    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design,
                               radius=radius, numerical_aperture=numerical_aperture, wavelength=wavelength,
                               periphery_orders='physical')
    f = lens['source_distance']
    periphery, centre, hgs = lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset']
    pupil = float(periphery['r_max_list'][-1])          # the lens's outer radius
    out = {'f': f, 'pupil': pupil}
    for name, dx in (('on_axis', 0.0), ('off_axis', offset)):
        # the reference's drop-in call; the near field stays on the GPU
        x, y, power_in, n_glass = ma.build_nearfield(dx, 0.0, -f, 'x', wavelength, periphery, centre, hgs, download=False)[4:8]
        ux = -dx / math.sqrt(dx * dx + f * f) / n_glass
        wf = ma.aperture_wavefront(None, None, None, None, x, y, wavelength, n_glass, pupil, n_max=4, reference=('plane', ux, 0.0))
        out[name] = dict(wf, power_in=power_in, reference=(ux, 0.0), x=x, y=y, n_glass=n_glass)
        if not verbose:
            continue
        print('emitter %.1f um off axis: %d samples in the pupil of %.1f um, %.4g of %.4g W leave it; target wave towards ux = %+.5f'
              % (dx * 1e6, wf['samples'], pupil * 1e6, wf['P'][0], power_in, ux))
        print('  Strehl ratio against the target %.4f, rms wavefront %.4f rad   (x component of E)' % (wf['coherence'][0, 0], wf['rms'][0, 0]))
        print('   j   n   m  term                  wavefront rad   |moment| / |piston|')
        rel = np.abs(wf['moments'][0, 0]) / np.abs(wf['moments'][0, 0, 0])
        for j, (n, m) in enumerate(wf['terms']):
            value = wf['piston'][0, 0] if j == 0 else wf['wavefront'][0, 0, j]
            print('  %2d  %2d  %+2d  %-20s  %+12.5f   %12.5f' % (j, n, m, NAMES[(int(n), int(m))], value, rel[j]))
    return out


if __name__ == '__main__':
    main()
