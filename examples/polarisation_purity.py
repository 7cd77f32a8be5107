"""How pure the polarisation behind the lens is: the image of an x-polarised emitter is reduced on the GPU to its Stokes
record - ``PlanePropagator.stokes()``, a few dozen doubles instead of three complex maps -, and the image of an UNPOLARISED
emitter, the incoherent sum of its x, y and z dipoles, to the record of its summed Stokes maps
(``SourceSweep.run(image=..., image_stokes=...)``); needs an MI355X.

    python examples/polarisation_purity.py

Printed: the degree of polarisation of the x-dipole's image (1 for every target alone; below 1 over a disc when the state
varies across it), the share of its transverse light that an analyser along y passes (``postprocess.analyser_power``), the
share of ``|Ez|^2``, and the degree of polarisation of the unpolarised emitter's image inside the same discs.  Sign of S3: +S0
for ``E`` proportional to ``x^ + i y^`` - under ``exp(-i omega t)``, for a wave travelling to +z, the field rotating
counter-clockwise seen looking towards the source (positive helicity)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(radius=20e-6, numerical_aperture=0.3, wavelength=580e-9, z=30e-6, verbose=True, keep_fields=False):
    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design, radius=radius,
                               numerical_aperture=numerical_aperture, wavelength=wavelength, switch_angle=np.deg2rad(8.0),
                               num_gratings=8, num_entries=8)
    f = lens['source_distance']
    periphery, centre, hgs = lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset']
    x, y, _, n_glass = ma.build_nearfield(0.0, 0.0, -f, 'x', wavelength, periphery, centre, hgs, download=False)[4:8]
    u = np.linspace(-0.1, 0.1, 16)
    sweep = ma.SourceSweep(wavelength, periphery, centre, hgs, x, y, u, u)
    # a plane behind the lens, targets above the aperture's samples; the Stokes record needs E alone
    tx, ty = x[0] + np.arange(len(x)) * (x[1] - x[0]), y[0] + np.arange(len(y)) * (y[1] - y[0])
    image = ma.PlanePropagator(x, y, wavelength, n_glass, tx, ty, z, method='fft', want_h=False, ctx=sweep.ctx)
    radii = np.array([0.25, 0.5, 1.0]) * radius
    axis = (float(tx[len(tx) // 2]), float(ty[len(ty) // 2]))
    # the x-dipole alone: its image stays on the GPU as member 0 of the last pass
    sweep.run([(0.0, 0.0, -f, 'x')], image=image)
    one = image.stokes(radii, centre=axis)
    cross = ma.analyser_power(one['S'][0], (0, 1)) / one['S'][0, 0]
    cross_enc = ma.analyser_power(one['encircled_S'][0], (0, 1)) / one['encircled_S'][0, :, 0]
    fields = image._download(0) if keep_fields else None
    # the unpolarised emitter: x, y and z dipoles at one place, their Stokes maps summed on the GPU
    res = sweep.run([(0.0, 0.0, -f, pol) for pol in 'xyz'], image=image, image_stokes=radii, image_centre=axis)
    unpolarised = res['image_stokes']
    out = {'radii': radii, 'dop': float(one['dop'][0]), 'cross_polarised_share': float(cross), 'cross_polarised_share_encircled': cross_enc,
           'longitudinal_share': float(one['longitudinal_share'][0]), 'encircled_dop': one['encircled_dop'][0],
           'dop_unpolarised': float(unpolarised['dop'][0]), 'encircled_dop_unpolarised': unpolarised['encircled_dop'][0],
           'stokes': one, 'fields': fields, 'axes': (tx, ty), 'centre': axis}
    if verbose:
        print('x-dipole: degree of polarisation of the integrated image %.6f, orientation %.3f deg, ellipticity %.3f deg'
              % (out['dop'], np.rad2deg(one['orientation'][0]), np.rad2deg(one['ellipticity'][0])))
        print('cross-polarised share %.17g' % out['cross_polarised_share'])
        print('longitudinal share %.6g' % out['longitudinal_share'])
        for R, d, c, du in zip(radii, out['encircled_dop'], cross_enc, out['encircled_dop_unpolarised']):
            print('  disc of %5.2f um: x-dipole dop %.6f, cross-polarised %.3e; unpolarised emitter dop %.4f' % (R * 1e6, d, c, du))
        print('unpolarised emitter (x + y + z dipoles): degree of polarisation of the summed image %.4f' % out['dop_unpolarised'])
    return out


if __name__ == '__main__':
    main()
