"""What correcting a collimator's wavefront would buy: measure, correct, look again.  The near field of an emitter 2 um off
axis is synthesised by a ``SourceSweep`` and its beam record - where the beam points, how wide it is, how much of the incident
power falls inside two cones about its peak - is taken on the GPU.  ``ApertureWavefront`` then reads the aberrations of that
field against the plane wave the chief ray takes, ``AperturePupil.from_wavefront`` turns them into the phase plate that
removes them, and the same sweep runs once more with ``pupil=``: the field never leaves the GPU, and the two beam records
stand side by side (needs an MI355X and the built library).

    python examples/corrected_collimator.py

The lens is the one of beam_steering.py.  The correction is the small-aberration reading of field_aberrations.py - first
order, nothing unwrapped or fitted - so one round removes most, not all, of the rms; a second round would take the rest
(tests/test_fields_pupil_host.py runs the loop)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(radius=50e-6, numerical_aperture=0.5, wavelength=580e-9, offset=2e-6, n_max=4, verbose=True):
    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design,
                               radius=radius, numerical_aperture=numerical_aperture, wavelength=wavelength,
                               periphery_orders='physical')
    f = lens['source_distance']
    periphery, centre, hgs = lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset']
    pupil_radius = float(periphery['r_max_list'][-1])          # the lens's outer radius
    # the reference's default sample grid, from the drop-in call (the near field stays on the GPU)
    x, y = ma.build_nearfield(offset, 0.0, -f, 'x', wavelength, periphery, centre, hgs, download=False)[4:6]
    u = np.linspace(-0.16, 0.16, 129)
    sweep = ma.SourceSweep(wavelength, periphery, centre, hgs, x, y, u, u)
    cones = (math.sin(math.radians(1.0)), math.sin(math.radians(3.0)))
    source = [(offset, 0.0, -f, 'x')]
    ux = -offset / math.sqrt(offset * offset + f * f) / sweep.n_glass      # the chief ray's direction in the glass
    aw = ma.ApertureWavefront(x, y, wavelength, sweep.n_glass, pupil_radius, n_max=n_max, reference=('plane', ux, 0.0), ctx=sweep.ctx)
    out = {'f': f, 'pupil': pupil_radius, 'x': x, 'y': y}
    correction = None
    for name in ('measured', 'corrected'):
        res = sweep.run(source, beam_cones=cones, pupil=correction)       # the sweep leaves the (corrected) field resident
        wf = aw.analyse(0, 1)
        b = res['beam']
        out[name] = {'rms': float(wf['rms'][0, 0]), 'strehl': float(wf['coherence'][0, 0]), 'wavefront': wf['wavefront'][0, 0],
                     'pointing': b['centroid_u'][0], 'peak_u': b['peak_u'][0], 'power_in': float(res['power_in'][0]),
                     'rms_divergence': float(np.sqrt(b['second_moments_u'][0, 0] + b['second_moments_u'][0, 1])),
                     'cone_fraction': res['beam_efficiency'][0]}
        if correction is None:
            correction = ma.AperturePupil.from_wavefront(aw, wf, stop=False)
            out['pupil_object'] = correction
    if verbose:
        print('emitter %.1f um off axis, pupil of %.1f um, Zernike terms up to order %d' % (offset * 1e6, pupil_radius * 1e6, n_max))
        print('%-34s %14s %14s' % ('', 'measured', 'corrected'))
        rows = (('rms wavefront / rad', 'rms', '%14.4f'), ('Strehl ratio against the target', 'strehl', '%14.4f'),
                ('rms divergence', 'rms_divergence', '%14.5f'))
        for label, key, fmt in rows:
            print('%-34s' % label + fmt % out['measured'][key] + fmt % out['corrected'][key])
        print('%-34s %+14.5f %+14.5f' % ('beam points to ux', out['measured']['pointing'][0], out['corrected']['pointing'][0]))
        for c, deg in enumerate((1, 3)):
            print('%-34s %13.2f%% %13.2f%%' % ('incident power within %d degree' % deg, 100 * out['measured']['cone_fraction'][c],
                                               100 * out['corrected']['cone_fraction'][c]))
    return out


if __name__ == '__main__':
    main()
