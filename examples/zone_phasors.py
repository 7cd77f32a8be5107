"""The phasor diagram of a focus: how much every Fresnel zone of an aperture adds to the field at the focal point, with
which phase, and what re-phasing the zones would buy.  A converging wave of NA 0.9 whose rings carry a phase error each
is uploaded, ``ApertureZoneFields`` reduces it on the GPU to one vector E_z per zone at the focus - the exact Stratton-Chu
sum of ``PlanePropagator`` left un-added across the zones -, ``AperturePupil.from_zone_fields`` turns every zone onto the
polarisation of the focus, and the corrected aperture is analysed again (needs an MI355X and the built library).

    python examples/zone_phasors.py

One line per zone: its samples, |p^H E_z|, its phase against the focus' own polarisation p = E / |E|, and dI / dphi_z, the
derivative of the focal intensity with respect to a phase added to the zone.  Then |p^H E| before and after the
correction, next to ``aligned`` = sum_z |p^H E_z|, the ceiling a phase per ring can reach."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(n=400, zones=12, sin_theta=0.9, error=1.0, verbose=True):
    import metalens_amd as ma
    wl, n_glass = 580e-9, 1.46
    k, Z = 2 * np.pi * n_glass / wl, ma.constants.Z0 / n_glass
    x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
    a = x.max()
    f = a / np.tan(np.arcsin(sin_theta))
    r2 = x[:, None] ** 2 + x[None, :] ** 2
    # zones of equal path difference to the focus; ring z carries a phase error of up to `error` radians
    path = np.sqrt(a * a + f * f) - f
    edges = np.sqrt((f + path * np.arange(1, zones + 1) / zones) ** 2 - f * f)
    edges[-1] = a
    err = np.random.default_rng(12).uniform(-error, error, zones)
    zone = np.searchsorted(edges * edges, r2, side='left')
    Ex = np.where(r2 <= a * a, np.exp(-1j * k * np.sqrt(r2 + f * f) + 1j * err[np.minimum(zone, zones - 1)]), 0)
    zero = np.zeros_like(Ex)
    focus = np.array([[0.0, 0.0, f]])
    azf = ma.ApertureZoneFields(x, x, wl, n_glass, edges, focus)
    before = ma.aperture_zone_fields(Ex, zero, zero, Ex / Z, x, x, wl, n_glass, edges, focus)
    p = before['polarisation'][0, :, 0]                  # the focus' own polarisation: kept for the second look
    pupil = ma.AperturePupil.from_zone_fields(azf, before)
    pupil.apply()
    after = azf.analyse(polarisation=p)
    out = {'f': f, 'edges': edges, 'error': err, 'before': before, 'after': after, 'x': x, 'n_glass': n_glass,
           'amplitude_before': float(np.abs(before['projection'][0, :, 0].sum() + before['outside_projection'][0, 0])),
           'amplitude_after': float(np.abs(after['projection'][0, :, 0].sum() + after['outside_projection'][0, 0])),
           'aligned': float(before['aligned'][0, 0])}
    if verbose:
        print('focus %.2f um behind a %.1f um pupil, NA %.2f: %d zones, phase errors up to %.2f rad' % (f * 1e6, 2 * a * 1e6, sin_theta, zones, error))
        print('  zone   r_out um  samples   |p^H E_z|   phase rad   dI/dphi_z')
        for z in range(zones):
            print('  %4d  %9.3f  %7d  %10.4g   %+9.4f  %+10.4g' % (z, edges[z] * 1e6, before['samples'][z], abs(before['projection'][0, z, 0]),
                                                                 before['phase'][0, z, 0], before['gradient'][0, z, 0]))
        print('|p^H E| at the focus: %.6g before, %.6g after re-phasing; aligned = sum_z |p^H E_z| = %.6g'
              % (out['amplitude_before'], out['amplitude_after'], out['aligned']))
    return out


if __name__ == '__main__':
    main()
