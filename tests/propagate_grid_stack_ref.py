"""NumPy restatement of the stack FFT form of the finite-distance propagator (csrc/propagate_grid.h GridStackPlan,
propagate_stack.hip; ``PlanePropagator(method='fft-stack')``), its plan, and the cases the tests share.  Test
infrastructure beside tests/propagate_grid_fine_ref.py, whose fine sum it calls per plane; nothing under metalens_amd/
imports it.

A stack is the fine targets ``tx[:, None] x ty[None, :]`` in ``nz`` planes ``z[0 ... nz - 1]`` (any order, repeats
allowed), target ``t = (p mx + i) my + j``.  The fine plan does not depend on z: one plan of ``(nx, ny, mx, my, sx, sy,
tile)`` serves every plane.  A LAYER is (plane p, lattice (a, b)), numbered ``l = p A + a Ay + b`` with ``A = Ax Ay``
active lattices; the layers are contracted ``PAIR`` at a time in that order - a pair may straddle two planes - and a
single one last if ``nz A`` is odd.

Workspace, in planes of ``Lx Ly 16`` bytes:
    kernel spectra kept (cache_kernels):  8 nz A tiles + 4 tiles + 2 outputs
    filled in every pass:                 16 batch     + 4 tiles + 2 outputs   (no nz: the streamed formula of the fine plan)
"""
import functools

import numpy as np

import propagate_grid_fine_ref as fref
import propagate_grid_ref as gref
import propagate_ref as ref

PLANES_MAX, PAIR = 4096, fref.PAIR
WL, N_GLASS = gref.WL, gref.N_GLASS


# ---- the plan ---------------------------------------------------------------------------------------------
def plan(nx, ny, mx, my, nz, subsample, want_h=True, tile=None, cache_kernels=True):
    """-> the dict of propagate_grid_fine_ref.plan (of one plane) with planes, layers and the workspace of the mode"""
    assert 1 <= nz <= PLANES_MAX and nz * mx * my <= 1 << 26
    p = fref.plan(nx, ny, mx, my, subsample, want_h, tile, cache_kernels)
    tiles, A, outputs = p['tiles'][0] * p['tiles'][1], p['active'][0] * p['active'][1], 6 if want_h else 3
    kernels = 8 * nz * A * tiles if cache_kernels else 8 * PAIR * p['batch']
    p.update(planes=nz, layers=nz * A, workspace_bytes=(kernels + 4 * tiles + PAIR * outputs) * p['plane_bytes'],
             fill_layers=fill_layers(min(PAIR, nz * A), p['batch'], p['plane_bytes']))
    return p


FILL_BYTES = 256 << 20   # the memory-side cache of an MI355X


def fill_layers(layers, tiles, plane_bytes):
    """the layers one fill launch takes: all of a contraction while their 8 planes a tile fit FILL_BYTES, else one"""
    return layers if layers * tiles * 8 * plane_bytes <= FILL_BYTES else 1


def layers(nz, active):
    """-> [(p, a, b)] in contraction order"""
    ax, ay = active
    return [(p, a, b) for p in range(nz) for a in range(ax) for b in range(ay)]


def pairs(n_layers):
    """-> the layers of every contraction: PAIR at a time, a single one last"""
    return [tuple(range(l0, min(l0 + PAIR, n_layers))) for l0 in range(0, n_layers, PAIR)]


# ---- the sum ----------------------------------------------------------------------------------------------
def stack_sum(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, tx, ty, z, subsample, tile=None, Z0=ref.Z0_SI, want_h=True):
    """E [3][nz mx my] (and H), target t = (p mx + i) my + j: ``propagate_grid_fine_ref.fine_sum`` per plane, stacked"""
    per_plane = [fref.fine_sum(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, tx, ty, zp, subsample, tile=tile, Z0=Z0,
                               want_h=want_h) for zp in z]
    if not want_h:
        return np.concatenate(per_plane, axis=1)
    return np.concatenate([e for e, _ in per_plane], axis=1), np.concatenate([h for _, h in per_plane], axis=1)


# ---- the cases the tests share -----------------------------------------------------------------------------
# name: (nx, ny, mx, my, planes z, origin x, origin y in pitches of the aperture, tile lengths or None for the default,
# (sx, sy)); mx, my are the fine targets of one plane.  The smallest shapes at which each path of the stack can go wrong;
# geometry and every z from the cases of propagate_grid_fine_ref.py (2 um ... 1 mm)
CASES = {
    'sa-ragged': (48, 40, 21, 31, (20e-6, 2e-6, 5e-6), 0.3, -0.4, (32, 32), (2, 3)),       # 18 layers, ragged lattices, unsorted z
    'sb-straddle': (48, 40, 3, 1, (20e-6, 2e-6, 50e-6), 20.3, 17.6, (16, 16), (4, 1)),     # 3 active lattices a plane, 9 layers: pairs straddle planes, a single remainder
    'sc-planes': (48, 40, 20, 30, (20e-6, 5e-6, 20e-6, 50e-6, 2e-6), 0.3, -0.4, None, (1, 1)),   # layers are planes only; two equal planes
    'sd-batches': (97, 40, 30, 25, (20e-6, 50e-6), 40.5, 10.25, (16, 16), (2, 2)),         # 490 tiles in eight batches: FIRST = false when streamed; 136 MB cached
    'se-far': (61, 35, 24, 17, (50e-6, 1e-3), -25.37, 11.21, None, (8, 8)),                # 128 layers, near and far
    'sf-one': (48, 40, 21, 31, (5e-6,), 0.3, -0.4, (32, 32), (2, 3)),                      # a single plane of 'sa-ragged'
}
# what the plan of every case is, stated outright
PLANS = {
    'sa-ragged': dict(L=(32, 32), tiles=(3, 2), tile_samples=(22, 22), batch=6, active=(2, 3), lattice_targets=(11, 11), planes=3, layers=18),
    'sb-straddle': dict(L=(16, 16), tiles=(3, 3), tile_samples=(16, 16), batch=9, active=(3, 1), lattice_targets=(1, 1), planes=3, layers=9),
    'sc-planes': dict(L=(128, 128), tiles=(1, 1), tile_samples=(109, 99), batch=1, active=(1, 1), lattice_targets=(20, 30), planes=5, layers=5),
    'sd-batches': dict(L=(16, 16), tiles=(49, 10), tile_samples=(2, 4), batch=64, active=(2, 2), lattice_targets=(15, 13), planes=2, layers=8),
    'se-far': dict(L=(64, 16), tiles=(1, 3), tile_samples=(62, 14), batch=3, active=(8, 8), lattice_targets=(3, 3), planes=2, layers=128),
    'sf-one': dict(L=(32, 32), tiles=(3, 2), tile_samples=(22, 22), batch=6, active=(2, 3), lattice_targets=(11, 11), planes=1, layers=6),
}


def geometry(case):
    nx, ny, mx, my, z, ox, oy, _, (sx, sy) = CASES[case]
    x, y = gref.axis(nx), gref.axis(ny)
    return x, y, fref.fine_axis(x, ox, mx, sx), fref.fine_axis(y, oy, my, sy), np.asarray(z, dtype=float)


def corners(nz, mx, my):
    """the four corners of every plane"""
    return [p * mx * my + c for p in range(nz) for c in (0, my - 1, (mx - 1) * my, mx * my - 1)]


def points(case):
    """-> F, x, y, the subset of targets - all of them up to 700, else every 7th and the corners of every plane - and their
    coordinates [sub][3]"""
    x, y, tx, ty, z = geometry(case)
    F = gref.random_fields(x.size, y.size, x.size + y.size)
    per_plane = tx.size * ty.size
    T = z.size * per_plane
    sub = np.arange(T) if T <= 700 else np.union1d(np.arange(0, T, 7), corners(z.size, tx.size, ty.size))
    p, t = sub // per_plane, sub % per_plane
    return F, x, y, sub, np.stack([tx[t // ty.size], ty[t % ty.size], z[p]], axis=1)


@functools.lru_cache(maxsize=None)
def reference(case):
    """as propagate_grid_fine_ref.reference: fields F, axes x, y, fine targets tx, ty, the planes z, ``tile``, ``subsample``,
    the ``plan`` (cached), the subset ``sub`` of targets, the long-double sum El, Hl on it, the NumPy stack form Enp, Hnp on
    every target, the errors e_ref (E, H) of the plain fp64 direct sum and e_np (E, H) of the NumPy stack form on the
    subset.  Computed once and shared: nobody changes it."""
    x, y, tx, ty, z = geometry(case)
    tile, subsample = CASES[case][7:]
    F, _, _, sub, pts = points(case)
    T = z.size * tx.size * ty.size
    E64, H64 = ref.direct_sum(*F, x, y, WL, N_GLASS, pts)
    El, Hl = ref.direct_sum(*F, x, y, WL, N_GLASS, pts, real=np.longdouble)
    Enp, Hnp = stack_sum(*F, x, y, WL, N_GLASS, tx, ty, z, subsample, tile=tile)
    assert Enp.shape == (3, T)
    return dict(F=F, x=x, y=y, tx=tx, ty=ty, z=z, tile=tile, subsample=subsample, pts=pts,
                plan=plan(x.size, y.size, tx.size, ty.size, z.size, subsample, True, tile), sub=sub, El=El, Hl=Hl, Enp=Enp, Hnp=Hnp,
                e_ref=(ref.max_error(E64, El), ref.max_error(H64, Hl)),
                e_np=(ref.max_error(Enp[:, sub], El), ref.max_error(Hnp[:, sub], Hl)))
