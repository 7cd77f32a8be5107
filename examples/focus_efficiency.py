"""Focus metrics without the volume: the converging wave and the stack of planes of examples/through_focus.py, reduced
on the GPU with ``PlanePropagator.focus()`` - the brightest plane, the depth of focus and the encircled-power curve of the
focal plane from a record of a few dozen doubles per plane; no field crosses PCIe (needs an MI355X).

    python examples/focus_efficiency.py

``focus()`` gives per plane the peak of |E|^2, its moments and the power inside up to 32 radii about a centre.  The on-axis
intensity of a plane is the sum inside a radius of 0 about the axis' target; the focusing efficiency of a plane is the
power ``sum Sz dx dy`` inside a disc over the power through the patch (``SourceSweep.run(image_radii=...)`` divides by the
incident power of its sources instead)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(n=400, planes=33, verbose=True):
    import metalens_amd as ma
    from metalens_amd import _lib
    wl, n_glass, sin_theta = 580e-9, 1.46, 0.5
    k, Z = 2 * np.pi * n_glass / wl, ma.constants.Z0 / n_glass
    x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
    a = x.max()
    f = a / np.tan(np.arcsin(sin_theta))
    r2 = x[:, None] ** 2 + x[None, :] ** 2
    Ex = np.where(r2 <= a * a, np.exp(-1j * k * np.sqrt(r2 + f * f)), 0)      # x-polarised, converging on (0, 0, f)
    zero = np.zeros_like(Ex)
    # the targets of examples/through_focus.py: 49 x 49 at a quarter of the pitch about the axis, planes around f
    s, m = 4, 49
    d = x[1] - x[0]
    t = (np.arange(m) - (m - 1) / 2) * d / s
    z = f + np.linspace(-6, 6, planes) * wl / n_glass
    p = ma.PlanePropagator(x, x, wl, n_glass, t, t, z, method='fft-stack', subsample=(s, s))
    _lib.check(p.ctx.lib.ml_fields_upload(p.ctx.handle, n, n, *[_lib.dptr(_lib.c128(v)) for v in (Ex, zero, zero, Ex / Z)]))
    p.ctx.fields_owner = None
    p.queue_sets(0, 1)                         # the volume stays on the GPU
    # about the axis: a radius of 0 holds the axis' target alone, the others draw the encircled-power curve
    radii = np.concatenate(([0.0], (np.arange(1, 13) + 0.5) * d / s, [2 * m * d / s]))
    on = p.focus(radii, centre=(0.0, 0.0))
    on_axis = on['encircled_I'][:, 0]
    best = int(on_axis.argmax())
    deep = z[on_axis >= on_axis.max() / 2]
    top = int(on['peak_I'].argmax())            # every plane's own peak: where |E|^2 is largest in the volume
    out = {'f': f, 'brightest_plane': best, 'z_brightest': float(z[best]),
           'depth_of_focus': float(deep[-1] - deep[0] + (z[1] - z[0])),
           'peak_xyz': (top,) + tuple(int(i) for i in on['peak_index'][top]),
           'radii': radii[1:], 'encircled_fraction': on['encircled_P'][best, 1:] / on['P'][best],
           'spot_rms': float(np.sqrt(on['second_moments_I'][best, :2].sum()))}
    if verbose:
        print('focal length %.2f um; on-axis |E|^2 is largest in plane %d of %d, z = %.2f um (f %+.0f nm); the largest |E|^2 of the '
              'volume is at sample %s' % (f * 1e6, best, planes, z[best] * 1e6, (z[best] - f) * 1e9, out['peak_xyz']))
        print('depth of focus (on-axis |E|^2 above half its peak) about %.2f um; rms radius of |E|^2 in the brightest plane %.0f nm'
              % (out['depth_of_focus'] * 1e6, out['spot_rms'] * 1e9))
        for R, frac in zip(out['radii'][:8], out['encircled_fraction'][:8]):
            print('  power through a disc of %4.0f nm about the axis: %5.1f %% of the patch' % (R * 1e9, 100 * frac))
    return out


if __name__ == '__main__':
    main()
