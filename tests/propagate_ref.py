"""NumPy restatement of the finite-distance propagator (metalens_amd/propagate.py, csrc/propagate.hip), for the
tests: the Stratton-Chu / Franz fields of the aperture's tangential equivalent currents, once in plain fp64 and
once in ``np.longdouble`` (as tools/oracle_longdouble.py does for the far field).  Test infrastructure: nothing
under metalens_amd/ imports it.

Convention (reference nearfield_farfield.py:94-95, outward normal +z, exp(-i omega t)):

    Jx = -Hy, Jy = Hx, Mx = Ey, My = -Ex;   k = 2 pi n_glass / wavelength,   Z = Z0 / n_glass

For a target r = (x, y, z), z > 0, and every aperture sample r' = (x', y', 0), with R = r - r', R = |R|:

    g = exp(ikR) / (4 pi R),  a = 1 + i/(kR) - 1/(kR)^2,  b = 1 + 3i/(kR) - 3/(kR)^2,  c = ik - 1/R
    E(r) = dx'dy' sum g { i k Z   [a J - b Rhat (Rhat.J)] - c Rhat x M }
    H(r) = dx'dy' sum g { i (k/Z) [a M - b Rhat (Rhat.M)] + c Rhat x J }

Aperture sample [i][j] sits at (x0 + i dx', y0 + j dy') with x0, dx' taken from the axis given (its first
sample and first step) - the definition of the C ABI (ml_propagate_plan), which uploaded fields need because
they carry no axes of their own.  k and Z are the fp64 numbers the library works with in both precisions: the
long-double sum measures the rounding of a sum, not of its inputs.
"""
import numpy as np

Z0_SI = 1.25663706212e-6 * 299792458.0


def direct_sum(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, points, Z0=Z0_SI, *, real=np.float64,
               want_h=True):
    """E [3][T] (and H [3][T]) at ``points`` [T][3]; ``real`` = np.float64 or np.longdouble"""
    cplx = np.complex128 if real is np.float64 else np.clongdouble
    k = real(2 * np.pi * n_glass / wavelength)
    Z = real(Z0 / n_glass)
    pi = 4 * np.arctan(real(1))
    x0, y0 = real(xp_list[0]), real(yp_list[0])
    dxp, dyp = real(xp_list[1] - xp_list[0]), real(yp_list[1] - yp_list[0])
    X, Y = np.meshgrid(x0 + np.arange(len(xp_list)).astype(real) * dxp,
                       y0 + np.arange(len(yp_list)).astype(real) * dyp, indexing='ij')
    Ex, Ey, Hx, Hy = (np.asarray(F).astype(cplx) for F in (Ex, Ey, Hx, Hy))
    Jx, Jy, Mx, My = -Hy, Hx, Ey, -Ex
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    E = np.zeros((3, len(points)), dtype=cplx)
    H = np.zeros((3, len(points)), dtype=cplx)
    i = cplx(1j)

    def dyad(a, b, ux, uy, uz, Vx, Vy):      # a V - b Rhat (Rhat . V), V tangential
        dot = ux * Vx + uy * Vy
        return a * Vx - b * ux * dot, a * Vy - b * uy * dot, -b * uz * dot

    def cross(ux, uy, uz, Vx, Vy):           # Rhat x V
        return -uz * Vy, uz * Vx, ux * Vy - uy * Vx

    for t, (x, y, z) in enumerate(points):
        Rx, Ry, Rz = real(x) - X, real(y) - Y, real(z)
        R = np.sqrt(Rx ** 2 + Ry ** 2 + Rz ** 2)
        ux, uy, uz = Rx / R, Ry / R, Rz / R
        kr = k * R
        g = np.exp(i * kr) / (4 * pi * R)
        a = 1 + i / kr - 1 / kr ** 2
        b = 1 + 3 * i / kr - 3 / kr ** 2
        c = i * k - 1 / R
        dJ, cM = dyad(a, b, ux, uy, uz, Jx, Jy), cross(ux, uy, uz, Mx, My)
        for m in range(3):
            E[m, t] = (g * (i * k * Z * dJ[m] - c * cM[m])).sum() * dxp * dyp
        if want_h:
            dM, cJ = dyad(a, b, ux, uy, uz, Mx, My), cross(ux, uy, uz, Jx, Jy)
            for m in range(3):
                H[m, t] = (g * (i * (k / Z) * dM[m] + c * cJ[m])).sum() * dxp * dyp
    return (E, H) if want_h else E


def poynting(E, H):
    """time-averaged S = Re(E x H*) / 2, [3][T]"""
    return 0.5 * np.real(np.cross(E, np.conj(H), axis=0))


def max_error(got, want):
    """max |got - want| over all components and targets / max |want| (`want` may be long double)"""
    want = np.asarray(want)
    return float(np.abs(np.asarray(got).astype(want.dtype) - want).max() / np.abs(want).max())


# ---- the cases the tests share ---------------------------------------------------------------------------
WL, N_GLASS = 580e-9, 1.46


def tilted_gaussian(n=48):
    """48^2 samples at pitch lambda / 2.2, a Gaussian beam tilted to ux = 0.2 with all four fields non-zero
    -> (Ex, Ey, Hx, Hy), axis, beam direction (ux, uy)"""
    d = WL / 2.2
    x = (np.arange(n) - (n - 1) / 2) * d
    X, Y = np.meshgrid(x, x, indexing='ij')
    k, Z = 2 * np.pi * N_GLASS / WL, Z0_SI / N_GLASS
    env = np.exp(-(X ** 2 + Y ** 2) / (n * d / 5) ** 2) * np.exp(1j * k * 0.2 * X)
    return (env * (1 + 0.3j), 0.4 * env, -0.4 * env / Z * 0.9, env / Z * (1.1 - 0.2j)), x, (0.2, 0.0)


def fan(beam, half=1e-3, n=9):
    """n x n directions around the beam.  Narrow on purpose: at finite distance rho the beam is displaced against
    its far field in FIRST order of 1 / rho (physics, not error: the long-double sum shows the same figures, odd
    in ux - ux_beam, 1.8e-6 / rho[m] of the peak per unit of direction cosine for the 48^2 case), so a fan as wide
    as the beam (0.05) could not meet 1e-8 at 1 m however exact the sum; within 1e-3 that term stays below 2e-9
    and what is left is the second-order Fresnel term, 2.4e-9, and any error in a sign or a constant factor,
    which shows in every direction alike."""
    return beam[0] + np.linspace(-half, half, n), beam[1] + np.linspace(-half, half, n)


def radiant_intensity(P, ux, uy):
    """rho^2 S_r of the far field from the reference's P on the tensor grid ux x uy: P uz / 2 with the reference's own
    two regularisers taken out again - it divides by (uz + 1e-5) where the formula has uz, and by (sin theta + 1e-9)
    in both amplitudes (nearfield_farfield.py:158-189; oracle/farfield_oracle.py project): 1e-5 and 1e-8 of P at
    sin theta = 0.2, both above what this comparison resolves."""
    UX, UY = np.meshgrid(ux, uy, indexing='ij')
    st = np.hypot(UX, UY)
    return P * (np.sqrt(1 - st ** 2) + 1e-5) / 2 * ((st + 1e-9) / st) ** 2


def fan_points(ux, uy, rho):
    """the points rho (ux, uy, uz) of the tensor grid ux x uy, [len(ux) len(uy)][3], and uz"""
    UX, UY = np.meshgrid(ux, uy, indexing='ij')
    UZ = np.sqrt(1 - UX ** 2 - UY ** 2)
    return rho * np.stack([UX.ravel(), UY.ravel(), UZ.ravel()], axis=1), UZ


def converging_wave(n=400, sin_theta=0.5):
    """ideal converging wave on a circular pupil: Ex = exp(-ik sqrt(x'^2 + y'^2 + f^2)), Hy = Ex / Z
    -> (Ex, Ey, Hx, Hy), axis, focal length f, scalar Airy width w = 0.51 lambda / (n_glass sin theta)"""
    d = WL / 2.2
    x = (np.arange(n) - (n - 1) / 2) * d
    X, Y = np.meshgrid(x, x, indexing='ij')
    k, Z = 2 * np.pi * N_GLASS / WL, Z0_SI / N_GLASS
    a = x.max()
    f = a / np.tan(np.arcsin(sin_theta))
    Ex = np.where(X ** 2 + Y ** 2 <= a * a, np.exp(-1j * k * np.sqrt(X ** 2 + Y ** 2 + f * f)), 0)
    zero = np.zeros_like(Ex)
    return (Ex, zero, zero, Ex / Z), x, f, 0.51 * WL / (N_GLASS * sin_theta)


def fwhm(t, I):
    """full width at half maximum of a single-peaked cut I(t), by linear interpolation"""
    h = I.max() / 2
    idx = np.where(I >= h)[0]
    lo, hi = idx[0], idx[-1]
    left = np.interp(h, [I[lo - 1], I[lo]], [t[lo - 1], t[lo]])
    right = np.interp(h, [I[hi + 1], I[hi]], [t[hi + 1], t[hi]])
    return right - left
