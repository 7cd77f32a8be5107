"""Through focus in one plan: the converging wave of examples/focal_plane.py propagated to a STACK of planes around its
focus with ``method='fft-stack'`` - a volume at a quarter of the aperture's pitch, from which the plane of the largest
intensity, the depth of focus and an xz cut are read off (needs an MI355X).

    python examples/through_focus.py

One ``PlanePropagator`` holds the whole volume: the currents of the aperture are transformed once, every plane is one more
set of kernel spectra, and the result has the shape ``(len(z), len(x), len(y))``."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(n=400, planes=33, verbose=True):
    import metalens_amd as ma
    wl, n_glass, sin_theta = 580e-9, 1.46, 0.5
    k, Z = 2 * np.pi * n_glass / wl, ma.constants.Z0 / n_glass
    x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
    a = x.max()
    f = a / np.tan(np.arcsin(sin_theta))
    r2 = x[:, None] ** 2 + x[None, :] ** 2
    Ex = np.where(r2 <= a * a, np.exp(-1j * k * np.sqrt(r2 + f * f)), 0)      # x-polarised, converging on (0, 0, f)
    zero = np.zeros_like(Ex)
    # 49 x 49 targets at a quarter of the pitch, centred on the axis (an even aperture: the axis lies half a pitch
    # between two samples, which is two fine steps), in planes up to six wavelengths in the glass before and behind f
    s, m = 4, 49
    d = x[1] - x[0]
    t = (np.arange(m) - (m - 1) / 2) * d / s
    z = f + np.linspace(-6, 6, planes) * wl / n_glass
    vol = ma.field_at_plane(Ex, zero, zero, Ex / Z, x, x, wl, n_glass, t, t, z, method='fft-stack', subsample=(s, s))
    I = np.abs(vol['Ex']) ** 2 + np.abs(vol['Ey']) ** 2 + np.abs(vol['Ez']) ** 2      # (planes, 49, 49)
    on_axis = I[:, m // 2, m // 2]
    best = int(on_axis.argmax())
    deep = z[on_axis >= on_axis.max() / 2]
    out = {'f': f, 'shape': I.shape, 'brightest_plane': best, 'z_brightest': float(z[best]),
           'depth_of_focus': float(deep[-1] - deep[0] + (z[1] - z[0])),
           'peak_xyz': tuple(int(i) for i in np.unravel_index(I.argmax(), I.shape)),
           'xz_cut': I[:, :, m // 2].T}
    if verbose:
        print('focal length %.2f um; |E|^2 is largest in plane %d of %d, z = %.2f um (f %+.0f nm), at sample %s of the %d x %d x %d volume'
              % (f * 1e6, best, planes, z[best] * 1e6, (z[best] - f) * 1e9, out['peak_xyz'], *I.shape))
        print('depth of focus (on-axis |E|^2 above half its peak) about %.2f um; the xz cut has %d x %d samples at %.0f nm x %.0f nm'
              % (out['depth_of_focus'] * 1e6, m, planes, d / s * 1e9, (z[1] - z[0]) * 1e9))
    return out


if __name__ == '__main__':
    main()
