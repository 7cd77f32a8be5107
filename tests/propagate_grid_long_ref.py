"""The cases and NumPy restatements for ``PlanePropagator(method='fft-long')`` (csrc/propagate_grid.h grid_axis_route,
propagate_grid.hip, propagate_grid_fft.hip; ml_propagate_plan_grid_long): padded axes of 16384.  Test infrastructure beside
tests/propagate_grid_ref.py, whose kernel planes, axes, fields and error measure it uses; nothing under metalens_amd/
imports it.

``grid_sum`` is propagate_grid_ref.grid_sum without its ``L <= 8192`` assertion.  ``two_level`` restates how an axis of
length L is transformed in two passes: R radix-2 stages on the whole sequence with a thread's 2^R elements at stride
L >> R (the streaming kernels), then independent transforms of blocks of ``len = L >> R`` elements, each a block of the
transform of length L (the LDS kernels) - decimation in frequency forward, natural order in and bit-reversed order out,
and decimation in time back.

The cases are thin: one axis is padded to 16384, the other to 32 (256), so a plane is 8 MB (67 MB) and a pass takes
milliseconds.  A case with both axes at 16384 needs a workspace of 77 GB: that is a measurement (tools/propagate_bench.py
--method fft-long), not a test.
"""
import functools

import numpy as np

import propagate_grid_ref as gref
import propagate_ref as ref

L_LONG_MAX = 16384
WL, N_GLASS = gref.WL, gref.N_GLASS

# name: (nx, ny, mx, my, z, origin x, origin y in pitches)
CASES = {
    'h-long': (8193, 20, 8192, 12, 200e-6, -4000.5, 3.25),        # 16384 x 32: long columns, n + m - 1 = L exactly
    'h-long-y': (20, 8193, 12, 8192, 200e-6, 3.25, -4000.5),      # 32 x 16384: long rows, exact fit
    'i-5000': (5000, 24, 4000, 9, 200e-6, -400.3, 2.5),           # 16384 x 32: 11384 zero rows skipped forward, 4000 rows back
    'i-5000-y': (24, 5000, 9, 4000, 200e-6, 2.5, -400.3),         # 32 x 16384
    'j-both': (8200, 70, 100, 60, 1e-3, 4050.25, -3.5),           # 16384 x 256: long x, several y-rows per workgroup
}
PADDED = {'h-long': (16384, 32), 'h-long-y': (32, 16384), 'i-5000': (16384, 32), 'i-5000-y': (32, 16384),
          'j-both': (16384, 256)}


def grid_sum(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, tx0, ty0, mx, my, z, Z0=ref.Z0_SI, want_h=True):
    """E [3][mx my] (and H) at the targets (tx0 + i dxp, ty0 + j dyp, z), target t = i my + j"""
    nx, ny = np.shape(Ex)
    k, Z = 2 * np.pi * n_glass / wavelength, Z0 / n_glass
    dxp, dyp = xp_list[1] - xp_list[0], yp_list[1] - yp_list[0]
    Lx, Ly = gref.padded_length(nx, mx), gref.padded_length(ny, my)
    assert Lx <= L_LONG_MAX and Ly <= L_LONG_MAX
    K = np.fft.fft2(gref.kernel_planes(Lx, Ly, mx, my, dxp, dyp, tx0 - xp_list[0], ty0 - yp_list[0], z, k))
    Kxx, Kxy, Kyy, Kzx, Kzy, Cx, Cy, Cz = K
    cur = np.zeros((4, Lx, Ly), dtype=np.complex128)
    cur[:, :nx, :ny] = [-np.asarray(Hy), np.asarray(Hx), np.asarray(Ey) / Z, -np.asarray(Ex) / Z]
    Jx, Jy, Mx, My = np.fft.fft2(cur)
    out = [Kxx * Jx + Kxy * Jy + Cz * My, Kxy * Jx + Kyy * Jy - Cz * Mx, Kzx * Jx + Kzy * Jy + Cy * Mx - Cx * My]
    if want_h:
        out += [Kxx * Mx + Kxy * My - Cz * Jy, Kxy * Mx + Kyy * My + Cz * Jx, Kzx * Mx + Kzy * My + Cx * Jy - Cy * Jx]
    out = np.fft.ifft2(np.stack(out))[:, :mx, :my].reshape(len(out), mx * my)
    scale_h = k * k / (4 * np.pi) * dxp * dyp
    E = Z * scale_h * out[:3]
    return (E, scale_h * out[3:]) if want_h else E


def geometry(case):
    nx, ny, mx, my, z, ox, oy = CASES[case]
    x, y = gref.axis(nx), gref.axis(ny)
    return x, y, gref.target_axis(x, ox, mx), gref.target_axis(y, oy, my), z


def subset(mx, my):
    """16 targets: the four corners, the middle and 11 drawn from a fixed seed"""
    fixed = [0, my - 1, (mx - 1) * my, mx * my - 1, (mx // 2) * my + my // 2]
    return np.concatenate([fixed, np.random.default_rng(20241).integers(0, mx * my, 11)])


@functools.lru_cache(maxsize=None)
def reference(case):
    """as propagate_grid_ref.reference: fields F, axes x, y, targets tx, ty, z, the subset ``sub``, the long-double
    sum El, Hl on it, the NumPy FFT form Enp, Hnp on every target, the errors e_ref (E, H) of the plain fp64 direct
    sum and e_np (E, H) of the NumPy FFT form on the subset"""
    x, y, tx, ty, z = geometry(case)
    F = gref.random_fields(x.size, y.size, x.size + y.size)
    T = tx.size * ty.size
    sub = subset(tx.size, ty.size)
    i, j = sub // ty.size, sub % ty.size
    pts = np.stack([tx[i], ty[j], np.full(sub.size, z)], axis=1)
    E64, H64 = ref.direct_sum(*F, x, y, WL, N_GLASS, pts)
    El, Hl = ref.direct_sum(*F, x, y, WL, N_GLASS, pts, real=np.longdouble)
    Enp, Hnp = grid_sum(*F, x, y, WL, N_GLASS, tx[0], ty[0], tx.size, ty.size, z)
    assert Enp.shape == (3, T)
    return dict(F=F, x=x, y=y, tx=tx, ty=ty, z=z, sub=sub, El=El, Hl=Hl, Enp=Enp, Hnp=Hnp,
                e_ref=(ref.max_error(E64, El), ref.max_error(H64, Hl)),
                e_np=(ref.max_error(Enp[:, sub], El), ref.max_error(Hnp[:, sub], Hl)))


# ---- the route of an axis (csrc/propagate_grid.h grid_axis_route) -------------------------------------------
L_MAX, COL_LDS, ROW_BLOCK = 8192, 1024, 4096


def axis_route(L, columns, row_block=ROW_BLOCK):
    """-> dict(top_stages, lds_len, forward, back): rows run whole in the LDS up to 8192 and in blocks of ``row_block``
    above, columns in blocks of 1024; the stages above the block in one streaming pass, first forward and last back"""
    whole = COL_LDS if columns else L_MAX
    lds_len = L if L <= whole else (COL_LDS if columns else row_block)
    top = (L // lds_len).bit_length() - 1
    return dict(top_stages=top, lds_len=lds_len, forward='top,lds' if top else 'lds', back='lds,top' if top else 'lds')


# ---- the two-pass transform -----------------------------------------------------------------------------
def twiddles(L):
    """w[j] = exp(2 pi i j / L), j < L / 2 (csrc/propagate_grid.h grid_twiddles)"""
    return np.exp(2j * np.pi * np.arange(L // 2) / L)


def _bfly(a, b, w, inverse):
    return (a + w * b, a - w * b) if inverse else (a + b, (a - b) * np.conj(w))


def top_stages(v, L, R, tw, inverse):
    """the thread programme of the streaming kernels (stage_group with B = L): thread pos0 < L >> R holds the 2^R
    elements pos0 + e (L >> R); stage t (forward t = 0 ... R - 1, back the reverse) pairs e and e + 2^(R - t - 1) with
    the twiddle of index p_low L / (L >> t), p_low = pos0 + (e mod 2^(R - t - 1)) (L >> R)"""
    estride = L >> R
    pos0 = np.arange(estride)
    e = [v[pos0 + q * estride] for q in range(1 << R)]
    for tt in range(R):
        t = R - 1 - tt if inverse else tt
        he = (1 << R) >> (t + 1)
        step = L // (L >> t)
        for q in range(1 << R):
            if q & he:
                continue
            p_low = pos0 + (q & (he - 1)) * estride
            assert p_low.max() < (L >> t) // 2
            e[q], e[q + he] = _bfly(e[q], e[q + he], tw[p_low * step], inverse)
    out = np.empty_like(v)
    for q in range(1 << R):
        out[pos0 + q * estride] = e[q]
    return out


def block_stages(v, L, length, tw, inverse):
    """the stages of block size ``length`` ... 2 (back: 2 ... ``length``) on every block of ``length`` elements, each a
    block of a transform of length L: the stage of block size B pairs p and p + B / 2 of a block with the twiddle of
    index p L / B"""
    v = v.copy()
    sizes = [length >> s for s in range(length.bit_length() - 1)]
    for B in (reversed(sizes) if inverse else sizes):
        blocks = v.reshape(-1, 2, B // 2)
        w = tw[np.arange(B // 2) * (L // B)]
        a, b = _bfly(blocks[:, 0, :], blocks[:, 1, :], w, inverse)
        v = np.stack([a, b], axis=1).reshape(-1)
    return v


def two_level(v, R, inverse=False):
    """the transform of ``v`` in two passes: forward top stages then blocks, back blocks then top stages"""
    L = v.size
    tw = twiddles(L)
    if inverse:
        return top_stages(block_stages(v, L, L >> R, tw, True), L, R, tw, True) if R else block_stages(v, L, L, tw, True)
    return block_stages(top_stages(v, L, R, tw, False) if R else v, L, L >> R, tw, False)


def bit_reversed(L):
    bits = L.bit_length() - 1
    p = np.arange(L)
    r = np.zeros(L, dtype=np.int64)
    for b in range(bits):
        r |= ((p >> b) & 1) << (bits - 1 - b)
    return r
