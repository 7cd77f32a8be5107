"""NumPy restatement of the tiled FFT form of the finite-distance propagator (csrc/propagate_grid.h GridTilePlan,
propagate_grid_tiled.hip; ``PlanePropagator(method='fft-tiled')``), its plan, and the cases the tests share.  Test
infrastructure beside tests/propagate_grid_ref.py, whose axes, fields and error measure it uses; nothing under
metalens_amd/ imports it.

Overlap-add over tiles of the aperture.  Per axis of n samples and m targets the tile length L is a power of two in
[16, 8192] with L >= m; ``B = L - m + 1`` samples go to each of ``c = ceil(n / B)`` tiles.  Tile a holds the samples
``[a B, min(n, a B + B))`` at the local indices 0 ... B - 1, and index p of its kernel plane holds the true lag

    (p if p < m else p - L) - a B

The eight kernel planes of a lag, the four current planes and the contraction are those of propagate_grid_ref; the
products of all tiles are added in the spectral domain, tile by tile in ascending order, in front of ONE inverse
``numpy.fft.ifft2``, the crop to ``[0, mx) x [0, my)`` and the scales.

The default L of an axis minimises the padded length c L times the measured cost of a padded sample at that length
(``WEIGHT``: flat up to 512); of equals the larger.  The batch - tiles that go through the
transforms together - is ``min(cx cy, 64, max(1, 128 MiB / (4 plane_bytes)))``, the workspace
``(8 cx cy + 4 batch + 6 or 3) Lx Ly 16`` bytes.
"""
import functools

import numpy as np

import propagate_grid_ref as gref
import propagate_ref as ref

L_MIN, L_MAX = 16, 8192
BATCH_MAX, BATCH_BYTES = 64, 128 << 20
WL, N_GLASS = gref.WL, gref.N_GLASS


# ---- the plan ---------------------------------------------------------------------------------------------
def admissible(L, m):
    return L_MIN <= L <= L_MAX and L & (L - 1) == 0 and L >= m


def tiles_of(n, m, L):
    """-> (B, c): samples per tile and tiles of an axis"""
    B = L - m + 1
    return B, -(-n // B)


# the cost of a padded sample of an axis at the tile length L, in 32nds of its cost at L <= 512: the square roots of the
# measured time per padded area of a pass
WEIGHT = {1024: 36, 2048: 42, 4096: 45, 8192: 45}


def tile_default(n, m):
    """the admissible L that minimises c L w(L); ties go to the larger L"""
    best = None
    for e in range(4, 14):
        L = 1 << e
        if admissible(L, m):
            cost = tiles_of(n, m, L)[1] * L * WEIGHT.get(L, 32)
            if best is None or cost <= best[0]:
                best = (cost, L)
    return best[1]


def plan(nx, ny, mx, my, want_h=True, tile=None, batch_bytes=BATCH_BYTES):
    """-> dict(L, tiles, tile_samples, batch, plane_bytes, workspace_bytes), the pairs (x, y)"""
    Lx, Ly = tile if tile else (0, 0)
    Lx, Ly = Lx or tile_default(nx, mx), Ly or tile_default(ny, my)
    assert admissible(Lx, mx) and admissible(Ly, my)
    (bx, cx), (by, cy) = tiles_of(nx, mx, Lx), tiles_of(ny, my, Ly)
    plane = Lx * Ly * 16
    batch = min(cx * cy, BATCH_MAX, max(1, batch_bytes // (4 * plane)))
    return dict(L=(Lx, Ly), tiles=(cx, cy), tile_samples=(bx, by), batch=batch, plane_bytes=plane,
                workspace_bytes=(8 * cx * cy + 4 * batch + (6 if want_h else 3)) * plane)


# ---- the sum ----------------------------------------------------------------------------------------------
def tile_lags(L, m, a, B):
    """the true lag held by every index of the kernel plane of tile a"""
    p = np.arange(L)
    return np.where(p < m, p, p - L) - a * B


def kernel_planes(lag_x, lag_y, dxp, dyp, off_x, off_y, z, k):
    """[8][Lx][Ly]: Kxx, Kxy, Kyy, Kzx, Kzy, Cx, Cy, Cz at the integer lags given (propagate_grid_ref.kernel_planes)"""
    dx = (lag_x * dxp + off_x)[:, None]
    dy = (lag_y * dyp + off_y)[None, :]
    R = np.sqrt(dx ** 2 + dy ** 2 + z ** 2)
    ux, uy, uz = dx / R, dy / R, z / R
    q = 1 / (k * R)
    w = np.exp(1j * k * R) * q
    a = 1 + 1j * q - q ** 2
    b = 1 + 3j * q - 3 * q ** 2
    c = w * (1j - q)
    return np.stack([1j * w * (a - b * ux ** 2), -1j * w * b * ux * uy, 1j * w * (a - b * uy ** 2),
                     -1j * w * b * uz * ux, -1j * w * b * uz * uy, c * ux, c * uy, c * uz])


def tiled_sum(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, tx0, ty0, mx, my, z, tile=None, Z0=ref.Z0_SI,
              want_h=True):
    """E [3][mx my] (and H) at the targets (tx0 + i dxp, ty0 + j dyp, z), target t = i my + j, tile by tile"""
    nx, ny = np.shape(Ex)
    k, Z = 2 * np.pi * n_glass / wavelength, Z0 / n_glass
    dxp, dyp = xp_list[1] - xp_list[0], yp_list[1] - yp_list[0]
    pl = plan(nx, ny, mx, my, want_h, tile)
    (Lx, Ly), (cx, cy), (bx, by) = pl['L'], pl['tiles'], pl['tile_samples']
    currents = np.stack([-np.asarray(Hy), np.asarray(Hx), np.asarray(Ey) / Z, -np.asarray(Ex) / Z])
    total = np.zeros((6 if want_h else 3, Lx, Ly), dtype=np.complex128)
    for a in range(cx):
        for b in range(cy):
            K = np.fft.fft2(kernel_planes(tile_lags(Lx, mx, a, bx), tile_lags(Ly, my, b, by), dxp, dyp,
                                          tx0 - xp_list[0], ty0 - yp_list[0], z, k))
            Kxx, Kxy, Kyy, Kzx, Kzy, Cx, Cy, Cz = K
            part = currents[:, a * bx:a * bx + bx, b * by:b * by + by]
            cur = np.zeros((4, Lx, Ly), dtype=np.complex128)
            cur[:, :part.shape[1], :part.shape[2]] = part
            Jx, Jy, Mx, My = np.fft.fft2(cur)
            out = [Kxx * Jx + Kxy * Jy + Cz * My, Kxy * Jx + Kyy * Jy - Cz * Mx, Kzx * Jx + Kzy * Jy + Cy * Mx - Cx * My]
            if want_h:
                out += [Kxx * Mx + Kxy * My - Cz * Jy, Kxy * Mx + Kyy * My + Cz * Jx, Kzx * Mx + Kzy * My + Cx * Jy - Cy * Jx]
            total += np.stack(out)
    out = np.fft.ifft2(total)[:, :mx, :my].reshape(total.shape[0], mx * my)
    scale_h = k * k / (4 * np.pi) * dxp * dyp
    E = Z * scale_h * out[:3]
    return (E, scale_h * out[3:]) if want_h else E


# ---- the cases the tests share -----------------------------------------------------------------------------
# name: (nx, ny, mx, my, z, origin x, origin y in pitches, tile lengths or None for the default, the targets the
# long-double sum is taken on: a slice of all of them, or 16 for ``subset``)
CASES = {
    'ta-near': (48, 40, 20, 30, 2e-6, 0.3, -0.4, (32, 64), slice(None)),            # 4 x 2 tiles, ragged last tiles
    'tb-one-target': (48, 40, 1, 1, 20e-6, 20.3, 17.6, (16, 16), slice(None)),      # B = L, 3 x 3 tiles
    'tc-far': (61, 35, 24, 17, 1e-3, -100.37, 41.21, None, slice(None)),            # one tile; the geometry of 'c-far'
    'td-many': (97, 80, 30, 25, 20e-6, 40.5, 30.25, (32, 32), 7),   # 33 x 10 tiles: 5 batches of 64, one of 10; every 7th target
    'tg-default': (300, 200, 12, 10, 50e-6, 140.5, -3.25, None, slice(None)),       # the chooser: (128, 256), 3 x 1 tiles
    'te-cols-top': (5000, 20, 100, 12, 200e-6, -2450.5, 3.25, (2048, 32), 16),      # batched planes through the streaming column stages
    'te-rows-long': (20, 5000, 12, 100, 200e-6, 3.25, -2450.5, (32, 2048), 16),     # rows of 2048
    'tf-beyond': (16500, 24, 40, 9, 200e-6, -8230.5, 7.25, None, 16),               # 35 x 1 tiles of (512, 32); 'fft-long' refuses it
}
# what the plan of every case is (the chooser and the tile arithmetic, stated outright)
PLANS = {
    'ta-near': dict(L=(32, 64), tiles=(4, 2), tile_samples=(13, 35), batch=8),
    'tb-one-target': dict(L=(16, 16), tiles=(3, 3), tile_samples=(16, 16), batch=9),
    'tc-far': dict(L=(128, 64), tiles=(1, 1), tile_samples=(105, 48), batch=1),
    'td-many': dict(L=(32, 32), tiles=(33, 10), tile_samples=(3, 8), batch=64),
    'tg-default': dict(L=(128, 256), tiles=(3, 1), tile_samples=(117, 247), batch=3),
    'te-cols-top': dict(L=(2048, 32), tiles=(3, 1), tile_samples=(1949, 21), batch=3),
    'te-rows-long': dict(L=(32, 2048), tiles=(1, 3), tile_samples=(21, 1949), batch=3),
    'tf-beyond': dict(L=(512, 32), tiles=(35, 1), tile_samples=(473, 24), batch=35),     # (by the padded length alone: 17 of 1024)
}
# the defaults the chooser must give: (n, m): (L, tiles)
# (by the padded length alone the first four were (1024, 9), (1024, 5), (2048, 3) and (2048, 9); the half-length tiles
# were measured 12 ... 31 % faster, hence the weights)
DEFAULTS = {(8192, 64): (512, 19), (4096, 64): (512, 10), (4096, 256): (1024, 6), (16384, 64): (512, 37), (2048, 64): (512, 5),
            (48, 20): (128, 1), (61, 24): (128, 1), (35, 17): (64, 1)}


def geometry(case):
    nx, ny, mx, my, z, ox, oy = CASES[case][:7]
    x, y = gref.axis(nx), gref.axis(ny)
    return x, y, gref.target_axis(x, ox, mx), gref.target_axis(y, oy, my), z


def corners(mx, my):
    return [0, my - 1, (mx - 1) * my, mx * my - 1]


def subset(mx, my):
    """16 targets: the four corners, the middle and 11 drawn from a fixed seed"""
    fixed = corners(mx, my) + [(mx // 2) * my + my // 2]
    return np.concatenate([fixed, np.random.default_rng(20243).integers(0, mx * my, 11)])


@functools.lru_cache(maxsize=None)
def reference(case):
    """as propagate_grid_ref.reference: fields F, axes x, y, targets tx, ty, z, the tile lengths asked for ``tile``, the
    ``plan``, the subset ``sub`` of targets, the long-double sum El, Hl on it, the NumPy tiled form Enp, Hnp on every
    target, the errors e_ref (E, H) of the plain fp64 direct sum and e_np (E, H) of the NumPy tiled form on the subset"""
    x, y, tx, ty, z = geometry(case)
    tile, which = CASES[case][7:]
    F = gref.random_fields(x.size, y.size, x.size + y.size)
    T = tx.size * ty.size
    if which == 16:
        sub = subset(tx.size, ty.size)
    elif which == 7:
        sub = np.union1d(np.arange(0, T, 7), corners(tx.size, ty.size))
    else:
        sub = np.arange(T)[which]
    i, j = sub // ty.size, sub % ty.size
    pts = np.stack([tx[i], ty[j], np.full(sub.size, z)], axis=1)
    E64, H64 = ref.direct_sum(*F, x, y, WL, N_GLASS, pts)
    El, Hl = ref.direct_sum(*F, x, y, WL, N_GLASS, pts, real=np.longdouble)
    Enp, Hnp = tiled_sum(*F, x, y, WL, N_GLASS, tx[0], ty[0], tx.size, ty.size, z, tile=tile)
    assert Enp.shape == (3, T)
    return dict(F=F, x=x, y=y, tx=tx, ty=ty, z=z, tile=tile, plan=plan(x.size, y.size, tx.size, ty.size, True, tile),
                sub=sub, El=El, Hl=Hl, Enp=Enp, Hnp=Hnp,
                e_ref=(ref.max_error(E64, El), ref.max_error(H64, Hl)),
                e_np=(ref.max_error(Enp[:, sub], El), ref.max_error(Hnp[:, sub], Hl)))
