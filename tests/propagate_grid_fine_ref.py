"""NumPy restatement of the fine FFT form of the finite-distance propagator (csrc/propagate_grid.h GridFinePlan,
propagate_grid_fine.hip; ``PlanePropagator(method='fft-fine')``), its plan, and the cases the tests share.  Test
infrastructure beside tests/propagate_grid_tiled_ref.py, whose tiled sum it calls; nothing under metalens_amd/ imports it.

Targets on the aperture's pitch divided by an integer s per axis: m fine targets ``t[i] = t[0] + i dxp / s``.  The targets
``a, a + s, a + 2 s, ...`` are lattice a, ``m_a = ceil((m - a) / s)`` of them on the aperture's pitch with the origin
``t[a]``; ``A = min(s, m)`` lattices hold a target.  Every lattice is planned with the count ``m_c = ceil(m / s)`` of
lattice 0, so all share the tiled plan of ``(nx, ny, m_cx, m_cy)``; the targets of a ragged lattice beyond ``m_a`` are
computed and dropped.  ``fine_sum`` is ``propagate_grid_tiled_ref.tiled_sum`` at the origin ``(tx[a], ty[b])`` for every
active lattice, interleaved.

Workspace, in planes of ``Lx Ly 16`` bytes, with ``A = Ax Ay`` and the tiles and the batch of the tiled plan:
    kernel spectra kept (cache_kernels):  8 A tiles + 4 tiles + 2 outputs
    filled in every pass:                 16 batch  + 4 tiles + 2 outputs
"""
import functools
import hashlib
import os

import numpy as np

import propagate_grid_ref as gref
import propagate_grid_tiled_ref as tref
import propagate_ref as ref

S_MAX, PAIR = 8, 2
WL, N_GLASS = gref.WL, gref.N_GLASS


# ---- the plan ---------------------------------------------------------------------------------------------
def lattices(m, s):
    """-> [(a, m_a)] of the active lattices of an axis"""
    return [(a, -(-(m - a) // s)) for a in range(min(s, m))]


def plan(nx, ny, mx, my, subsample, want_h=True, tile=None, cache_kernels=True):
    """-> the dict of propagate_grid_tiled_ref.plan for ``(nx, ny, m_cx, m_cy)`` with subsample, active (Ax, Ay),
    lattice_targets (m_cx, m_cy), cache_kernels and the workspace of the mode"""
    sx, sy = subsample
    assert 1 <= sx <= S_MAX and 1 <= sy <= S_MAX
    m_cx, m_cy = -(-mx // sx), -(-my // sy)
    p = tref.plan(nx, ny, m_cx, m_cy, want_h, tile)
    tiles, A, outputs = p['tiles'][0] * p['tiles'][1], min(sx, mx) * min(sy, my), 6 if want_h else 3
    kernels = 8 * A * tiles if cache_kernels else 8 * PAIR * p['batch']
    p.update(subsample=(sx, sy), active=(min(sx, mx), min(sy, my)), lattice_targets=(m_cx, m_cy), cache_kernels=bool(cache_kernels),
             workspace_bytes=(kernels + 4 * tiles + PAIR * outputs) * p['plane_bytes'])
    return p


# ---- the sum ----------------------------------------------------------------------------------------------
def fine_sum(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, tx, ty, z, subsample, tile=None, Z0=ref.Z0_SI, want_h=True):
    """E [3][mx my] (and H) at the fine targets ``tx[:, None] x ty[None, :]``, target t = i my + j: every active lattice
    by ``tiled_sum`` at its own origin with the counts (m_cx, m_cy), its first m_a x m_b targets interleaved"""
    sx, sy = subsample
    mx, my = tx.size, ty.size
    m_cx, m_cy = -(-mx // sx), -(-my // sy)
    E = np.zeros((3, mx, my), dtype=np.complex128)
    H = np.zeros((3, mx, my), dtype=np.complex128)
    for a, m_a in lattices(mx, sx):
        for b, m_b in lattices(my, sy):
            got = tref.tiled_sum(Ex, Ey, Hx, Hy, xp_list, yp_list, wavelength, n_glass, tx[a], ty[b], m_cx, m_cy, z, tile=tile,
                                 Z0=Z0, want_h=want_h)
            El, Hl = got if want_h else (got, None)
            E[:, a::sx, b::sy] = El.reshape(3, m_cx, m_cy)[:, :m_a, :m_b]
            if want_h:
                H[:, a::sx, b::sy] = Hl.reshape(3, m_cx, m_cy)[:, :m_a, :m_b]
    E = E.reshape(3, mx * my)
    return (E, H.reshape(3, mx * my)) if want_h else E


# ---- the cases the tests share -----------------------------------------------------------------------------
# name: (nx, ny, mx, my, z, origin x, origin y in pitches of the aperture, tile lengths or None for the default, (sx, sy));
# mx, my are the fine targets
CASES = {
    'fa-ragged': (48, 40, 21, 31, 2e-6, 0.3, -0.4, (32, 32), (2, 3)),        # 3 x 2 tiles; m_c = (11, 11); ragged last lattices; 6 lattices
    'fb-fewer-than-s': (48, 40, 3, 1, 20e-6, 20.3, 17.6, (16, 16), (4, 1)),  # 3 active of 4: a pair and a single; m_c = (1, 1); B = L
    'fc-batches': (97, 40, 30, 25, 20e-6, 40.5, 10.25, (16, 16), (2, 2)),    # 49 x 10 tiles in batches of 64; 61 MiB of kernel spectra
    'fd-eight': (61, 35, 24, 17, 1e-3, -25.37, 11.21, None, (8, 8)),         # 64 lattices of 3 x 3; default tile (64, 16), 1 x 3 tiles
    'fe-default': (300, 200, 35, 19, 50e-6, 140.5, 90.25, None, (3, 2)),     # the chooser on m_c = (12, 10): (128, 256), 3 x 1 tiles
}
# what the plan of every case is, stated outright
PLANS = {
    'fa-ragged': dict(L=(32, 32), tiles=(3, 2), tile_samples=(22, 22), batch=6, active=(2, 3), lattice_targets=(11, 11)),
    'fb-fewer-than-s': dict(L=(16, 16), tiles=(3, 3), tile_samples=(16, 16), batch=9, active=(3, 1), lattice_targets=(1, 1)),
    'fc-batches': dict(L=(16, 16), tiles=(49, 10), tile_samples=(2, 4), batch=64, active=(2, 2), lattice_targets=(15, 13)),
    'fd-eight': dict(L=(64, 16), tiles=(1, 3), tile_samples=(62, 14), batch=3, active=(8, 8), lattice_targets=(3, 3)),
    'fe-default': dict(L=(128, 256), tiles=(3, 1), tile_samples=(117, 247), batch=3, active=(3, 2), lattice_targets=(12, 10)),
}


def fine_axis(ap_axis, origin_pitches, m, s):
    """m targets on the axis' pitch / s, the first ``origin_pitches`` pitches behind the axis' first sample"""
    d = ap_axis[1] - ap_axis[0]
    return (ap_axis[0] + origin_pitches * d) + np.arange(m) * d / s


def geometry(case):
    nx, ny, mx, my, z, ox, oy, _, (sx, sy) = CASES[case]
    x, y = gref.axis(nx), gref.axis(ny)
    return x, y, fine_axis(x, ox, mx, sx), fine_axis(y, oy, my, sy), z


RECORDED = ('fe-default',)   # 665 targets behind 60 000 samples: the long-double sum takes a minute
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'propagate_grid_fine_%s.npz')


def _inputs_key(F, x, y, pts):
    return hashlib.sha256(b''.join(np.ascontiguousarray(a).tobytes() for a in (*F, x, y, pts))).hexdigest()


def long_double_sum(case, F, x, y, pts):
    """-> El, Hl: ``propagate_ref.direct_sum`` in long double at ``pts``.  For the cases of ``RECORDED`` the sum is kept
    under tests/golden/ (``python tests/propagate_grid_fine_ref.py`` writes it), each value as a double and the double of
    what is left - exact for the 64-bit significand - with a hash of the fields, the axes and the points; a record made
    for other inputs is not used.  tests/test_propagate_grid_fine_host.py compares a record with the sum taken afresh on
    some of its targets."""
    path = GOLDEN % case
    if case in RECORDED and os.path.exists(path):
        with np.load(path) as g:
            if str(g['key']) == _inputs_key(F, x, y, pts):
                return tuple(g[n + '_hi'].astype(np.clongdouble) + g[n + '_lo'].astype(np.clongdouble) for n in 'EH')
    return ref.direct_sum(*F, x, y, WL, N_GLASS, pts, real=np.longdouble)


def points(case):
    """-> F, x, y, the subset of targets and their coordinates [sub][3]"""
    x, y, tx, ty, z = geometry(case)
    F = gref.random_fields(x.size, y.size, x.size + y.size)
    T = tx.size * ty.size
    sub = np.arange(T) if T <= 700 else np.union1d(np.arange(0, T, 7), tref.corners(tx.size, ty.size))
    i, j = sub // ty.size, sub % ty.size
    return F, x, y, sub, np.stack([tx[i], ty[j], np.full(sub.size, z)], axis=1)


def record(case):
    F, x, y, _, pts = points(case)
    El, Hl = ref.direct_sum(*F, x, y, WL, N_GLASS, pts, real=np.longdouble)
    parts = {}
    for n, v in (('E', El), ('H', Hl)):
        hi = v.astype(np.complex128)
        parts[n + '_hi'], parts[n + '_lo'] = hi, (v - hi.astype(np.clongdouble)).astype(np.complex128)
    np.savez(GOLDEN % case, key=_inputs_key(F, x, y, pts), **parts)


@functools.lru_cache(maxsize=None)
def reference(case):
    """as propagate_grid_tiled_ref.reference: fields F, axes x, y, fine targets tx, ty, z, ``tile``, ``subsample``, the
    ``plan`` (cached), the subset ``sub`` of targets - all of them up to 700, else every 7th and the corners - the
    long-double sum El, Hl on it, the NumPy fine form Enp, Hnp on every target, the errors e_ref (E, H) of the plain fp64
    direct sum and e_np (E, H) of the NumPy fine form on the subset"""
    x, y, tx, ty, z = geometry(case)
    tile, subsample = CASES[case][7:]
    F, _, _, sub, pts = points(case)
    T = tx.size * ty.size
    E64, H64 = ref.direct_sum(*F, x, y, WL, N_GLASS, pts)
    El, Hl = long_double_sum(case, F, x, y, pts)
    Enp, Hnp = fine_sum(*F, x, y, WL, N_GLASS, tx, ty, z, subsample, tile=tile)
    assert Enp.shape == (3, T)
    return dict(F=F, x=x, y=y, tx=tx, ty=ty, z=z, tile=tile, subsample=subsample,
                plan=plan(x.size, y.size, tx.size, ty.size, subsample, True, tile), sub=sub, El=El, Hl=Hl, Enp=Enp, Hnp=Hnp,
                e_ref=(ref.max_error(E64, El), ref.max_error(H64, Hl)),
                e_np=(ref.max_error(Enp[:, sub], El), ref.max_error(Hnp[:, sub], Hl)))


if __name__ == '__main__':
    for name in RECORDED:
        record(name)
        print('wrote', GOLDEN % name)
