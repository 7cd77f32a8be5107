"""How much of an emitter's light enters a single-mode fibre behind the lens: the lens images the emitter into a beam, a fibre
collimator with a Gaussian mode looks at that beam in a plane behind the lens, and the coupling efficiency is read on the GPU
- ``PlanePropagator.overlap()`` and ``SourceSweep.run(image=..., image_modes=...)`` contract the resident image with the modes
(``ml_propagate_modes_queue``) and only the overlaps cross PCIe (needs an MI355X).

    python examples/fibre_coupling.py

The fibre is ALIGNED first, as on a bench, on the image of the on-axis emitter: a grid of 41 x 41 lateral positions of the
mode in one ``overlap()`` call, then 8 waists x 8 wavefront curvatures taken from the diagonal of a second call, then the
lateral grid once more with the mode found.  The tolerance study follows: the coupling into the aligned mode as a function of
the fibre's lateral offset (a grid of ``centre`` values) and of the emitter's offset (a sweep).  One line per position:
``coupling <emitter um> <fibre um> <share of the power the emitter sends through the lens that enters the x-polarised mode>``.
An emitter off the axis tilts the beam, a fibre off its aligned position misses it: the on-axis pair couples best."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEP = 0.5e-6          # the lateral grid of the alignment; the fibre offsets of the study are multiples of it


def align(image, tx, ty, wavelength, n_glass, w0, verbose=True):
    """the Gaussian mode that couples best to member 0 of the image's last pass -> (centre x, centre y, waist, distance of the
    waist before the plane, coupling_x over the power through the patch)"""
    import metalens_amd as ma
    shifts = (np.arange(41) - 20) * STEP
    axis = lambda t, c, w, z: ma.gaussian_axis(t, w, z, centre=c, wavelength=wavelength, n=n_glass)

    def lateral(cx, cy, w, z):
        got = image.overlap(np.array([axis(tx, cx + s, w, z) for s in shifts]), np.array([axis(ty, cy + s, w, z) for s in shifts]))
        a, b = np.unravel_index(np.argmax(got['coupling_x'][0]), (41, 41))
        return cx + shifts[a], cy + shifts[b], got['coupling_x'][0, a, b]
    cx, cy, best = lateral(0.0, 0.0, w0, 0.0)
    # waists and curvatures: mode k of either axis has the same pair, so the diagonal of the 64 x 64 call holds the beams
    zR = np.pi * n_glass * w0 * w0 / wavelength
    pairs = [(w0 * f, zR * g) for f in (0.5, 0.7, 0.85, 1.0, 1.2, 1.5, 2.0, 3.0) for g in (-2.0, -1.0, -0.5, -0.2, 0.0, 0.2, 0.5, 1.0)]
    got = image.overlap(np.array([axis(tx, cx, w, z) for w, z in pairs]), np.array([axis(ty, cy, w, z) for w, z in pairs]))
    k = int(np.argmax(np.diagonal(got['coupling_x'][0])))
    w, z = pairs[k]
    cx, cy, best = lateral(cx, cy, w, z)
    if verbose:
        print('aligned: centre (%.2f, %.2f) um, waist %.2f um lying %.1f um before the plane, %.4f of the power through the patch'
              % (cx * 1e6, cy * 1e6, w * 1e6, z * 1e6, best))
    return cx, cy, w, z, best


def main(radius=20e-6, numerical_aperture=0.3, wavelength=580e-9, emitter_offsets=(0.0, 1.0e-6, 2.0e-6),
         fibre_offsets=(-8e-6, -4e-6, 0.0, 4e-6, 8e-6), z=30e-6, verbose=True):
    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design, radius=radius,
                               numerical_aperture=numerical_aperture, wavelength=wavelength, switch_angle=np.deg2rad(8.0),
                               num_gratings=8, num_entries=8)
    f = lens['source_distance']
    periphery, centre, hgs = lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset']
    # the reference's drop-in call gives the aperture's grid; the sweep synthesises every emitter position on it
    x, y, _, n_glass = ma.build_nearfield(0.0, 0.0, -f, 'x', wavelength, periphery, centre, hgs, download=False)[4:8]
    u = np.linspace(-0.1, 0.1, 16)
    sweep = ma.SourceSweep(wavelength, periphery, centre, hgs, x, y, u, u)
    # the plane of the fibre collimator: targets above the aperture's samples, on its pitch as method='fft' wants them
    tx, ty = x[0] + np.arange(len(x)) * (x[1] - x[0]), y[0] + np.arange(len(y)) * (y[1] - y[0])
    image = ma.PlanePropagator(x, y, wavelength, n_glass, tx, ty, z, method='fft', ctx=sweep.ctx)
    # the image of the on-axis emitter stays on the GPU; the fibre is aligned on it
    sweep.run([(0.0, 0.0, -f, 'x')], image=image)
    cx, cy, w, zw, patch_share = align(image, tx, ty, wavelength, n_glass, 0.45 * radius, verbose)
    # the tolerance study: fibre offsets about the aligned position (on the alignment's grid), emitter offsets as a sweep
    mode_x = np.array([ma.gaussian_axis(tx, w, zw, centre=cx + c, wavelength=wavelength, n=n_glass) for c in fibre_offsets])
    mode_y = ma.gaussian_axis(ty, w, zw, centre=cy, wavelength=wavelength, n=n_glass)
    sources = [(d, 0.0, -f, 'x') for d in emitter_offsets]
    res = sweep.run(sources, image=image, image_modes=(mode_x, mode_y))
    coupling = res['image_coupling']['coupling_x'][:, 0, :, 0]          # (emitter positions, fibre offsets)
    if verbose:
        for d, row in zip(emitter_offsets, coupling):
            for c, value in zip(fibre_offsets, row):
                print('coupling %.3f %.3f %.6f' % (d * 1e6, c * 1e6, value))
    return {'coupling': coupling, 'emitter_offsets': np.array(emitter_offsets), 'fibre_offsets': np.array(fibre_offsets),
            'power_in': res['power_in'], 'aligned': (cx, cy, w, zw), 'patch_share': patch_share}


if __name__ == '__main__':
    main()
