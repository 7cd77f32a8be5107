"""The field in and around a focus: an ideal converging wave behind a 106 um pupil, propagated to its focal
plane and to an xz cut through the focus with ``metalens_amd.field_at_plane`` (needs an MI355X).

    python examples/focal_plane.py

The wave is uploaded here; after ``build_nearfield(..., download=False)`` or a ``HotPath`` step the same call
with ``None`` for the four fields propagates the lens' own near field, which is already on the GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(n=400, verbose=True):
    import metalens_amd as ma
    wl, n_glass, sin_theta = 580e-9, 1.46, 0.5
    k, Z = 2 * np.pi * n_glass / wl, ma.constants.Z0 / n_glass
    x = (np.arange(n) - (n - 1) / 2) * (wl / 2.2)
    a = x.max()
    f = a / np.tan(np.arcsin(sin_theta))
    r2 = x[:, None] ** 2 + x[None, :] ** 2
    Ex = np.where(r2 <= a * a, np.exp(-1j * k * np.sqrt(r2 + f * f)), 0)      # x-polarised, converging on (0, 0, f)
    zero = np.zeros_like(Ex)
    w = 0.51 * wl / (n_glass * sin_theta)                                       # scalar Airy width (FWHM)
    t = np.linspace(-3 * w, 3 * w, 61)
    # the focal plane: E, H and the power flow through it
    plane = ma.field_at_plane(Ex, zero, zero, Ex / Z, x, x, wl, n_glass, t, t, f)
    # an xz cut through the focus is a point list; the fields are resident now (Ex = None), E only
    zs = f + np.linspace(-6, 6, 81) * wl / n_glass
    X, Zs = np.meshgrid(t, zs, indexing='ij')
    cut = ma.field_at_plane(None, None, None, None, x, x, wl, n_glass, X.ravel(), np.zeros(X.size), Zs.ravel(),
                            point_list=True, want_h=False)
    I_plane = np.abs(plane['Ex']) ** 2 + np.abs(plane['Ey']) ** 2 + np.abs(plane['Ez']) ** 2
    I_cut = cut['I'].reshape(X.shape)
    above = t[I_plane[:, 30] >= I_plane.max() / 2]
    out = {'f': f, 'airy_fwhm': w, 'fwhm_x': above[-1] - above[0] + (t[1] - t[0]),
           'peak_xy': tuple(int(i) for i in np.unravel_index(I_plane.argmax(), I_plane.shape)),
           'peak_xz': tuple(int(i) for i in np.unravel_index(I_cut.argmax(), I_cut.shape)),
           'power_through_patch': float(plane['Sz'].sum() * (t[1] - t[0]) ** 2),
           'power_in_pupil': float(0.5 * np.real(Ex * np.conj(Ex / Z)).sum() * (x[1] - x[0]) ** 2)}
    if verbose:
        print('focal length %.2f um; |E|^2 peaks at sample %s of the 61 x 61 focal-plane map and %s of the 61 x 81 xz cut'
              % (f * 1e6, out['peak_xy'], out['peak_xz']))
        print('FWHM along x about %.0f nm (scalar Airy %.0f nm); %.1f %% of the pupil\'s power crosses the %.1f um patch'
              % (out['fwhm_x'] * 1e9, w * 1e9, 100 * out['power_through_patch'] / out['power_in_pupil'], 6 * w * 1e6))
    return out


if __name__ == '__main__':
    main()
