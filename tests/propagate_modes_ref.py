"""The overlap of a propagated image with separable modes (metalens_amd/csrc/propagate_modes.hip, ml_propagate_modes_plan /
_queue / _fetch) restated from downloaded arrays: the yardstick of tests/test_gpu_propagate_modes.py and
tests/test_propagate_modes_host.py.

    O_F[a][b] = sum_i sum_j conj(A[a][i]) conj(B[b][j]) F(i, j)

With a = conj(A[a][i]), b = conj(B[b][j]) and f = F(i, j) a term is the complex product a b f, eight real triple products:
    re:  (a.r b.r) f.r - (a.r b.i) f.i - (a.i b.r) f.i - (a.i b.i) f.r
    im:  (a.r b.r) f.i + (a.r b.i) f.r + (a.i b.r) f.r - (a.i b.i) f.i
Each triple product is formed in doubles and so rounded twice; each of re and im is the ``math.fsum`` - correctly rounded -
of its ``4 mx my`` triple products.  Beside each entry stands
    mag = sum_ij (|a.r| + |a.i|) (|b.r| + |b.i|) (|f.r| + |f.i|),
the sum of the moduli of all eight triple products, which bounds the moduli of whatever the device forms on its way.

Bound of an entry, each of re and im: ``(mx + my + 16) u mag`` with ``u = 2^-53``, made up of relative errors against mag:
    the complex product F Ty                            2 u   (a product and the difference or sum of two)
    the two-level sum over j                            <= (my + 2) u   (at most 32 adds within a segment and ceil(my / 32) adds of
                                                        segments lie on the way of a term: 32 + ceil(my / 32) <= my + 2 where
                                                        my >= 32, and min(my, 32) + 1 <= my + 2 below)
    the product with Tx                                 2 u
    the two-level sum over i                            <= (mx + 2) u
    the yardstick's two roundings per triple product
    and the final rounding of fsum                      3 u
    sum: (mx + my + 11) u, rounded up to                (mx + my + 16) u
(first order in u; at mx + my < 2^12 the second-order terms are below 2^-40 of that).  A derivation, not a measurement."""
import math

import numpy as np

U = 2.0 ** -53
MODES_MAX, SEGMENT = 64, 32          # csrc/propagate_modes.h
TILE_FEW, FEW, ROWS_MANY, TILE_MANY, COLUMN_TILE = 512, 8, 2, 128, 1024
COMPONENTS = ('Ex', 'Ey', 'Hx', 'Hy')


def _last(n, tile):
    """n indices in tiles of ``tile``: -> tiles, segments of the last tile, indices of its last segment"""
    tiles = -(-n // tile)
    last = n - (tiles - 1) * tile
    segments = -(-last // SEGMENT)
    return tiles, segments, last - (segments - 1) * SEGMENT


def plan(mx, my, nv):
    """the launch shapes of the row and the column pass (modes_rows_shape, modes_columns_shape): what ``propagate_modes_plan
    shape`` prints"""
    rows = 1 if nv <= FEW else ROWS_MANY
    tile = TILE_FEW if nv <= FEW else TILE_MANY
    tiles, last_segments, last_segment = _last(my, tile)
    groups = -(-mx // rows)
    col_tiles, col_last_segments, col_last_segment = _last(mx, COLUMN_TILE)
    return dict(rows=rows, tile=tile, tiles=tiles, last_segments=last_segments, last_segment=last_segment, groups=groups,
                last_rows=mx - (groups - 1) * rows, col_tile=COLUMN_TILE, col_tiles=col_tiles, col_last_segments=col_last_segments,
                col_last_segment=col_last_segment)


def bound_factor(mx, my):
    """the bound of an entry over ``u mag`` (module docstring)"""
    return mx + my + 16


def _fsum_rows(a):
    """fsum of every row of a 2-D array"""
    return np.array([math.fsum(row) for row in a.tolist()])


def overlaps(F, A, B):
    """one plane and one component: F complex (mx, my), A complex (nu, mx), B complex (nv, my) -> (O complex (nu, nv), mag
    (nu, nv))"""
    F, A, B = (np.asarray(v, dtype=np.complex128) for v in (F, A, B))
    mx, my = F.shape
    assert A.ndim == B.ndim == 2 and A.shape[1] == mx and B.shape[1] == my
    fr, fi = F.real, F.imag
    br, bi = B.real[:, None, :], -B.imag[:, None, :]          # conj(B), (nv, 1, my)
    O = np.empty((A.shape[0], B.shape[0]), dtype=np.complex128)
    for a in range(A.shape[0]):
        ar, ai = A.real[a][None, :, None], -A.imag[a][None, :, None]          # conj(A[a]), (1, mx, 1)
        rr, ri, ir, ii = ar * br, ar * bi, ai * br, ai * bi          # (nv, mx, my), rounded once
        re = np.stack([rr * fr, -(ri * fi), -(ir * fi), -(ii * fr)], axis=1)          # rounded twice
        im = np.stack([rr * fi, ri * fr, ir * fr, -(ii * fi)], axis=1)
        O[a] = _fsum_rows(re.reshape(len(B), -1)) + 1j * _fsum_rows(im.reshape(len(B), -1))
    wa, wb = np.abs(A.real) + np.abs(A.imag), np.abs(B.real) + np.abs(B.imag)
    mag = wa @ (np.abs(fr) + np.abs(fi)) @ wb.T
    return O, mag


def worst_ratio(got, F, A, B):
    """``got`` complex (nu, nv) against the yardstick -> (the worst ratio of an error to its bound, all within it)"""
    O, mag = overlaps(F, A, B)
    bound = bound_factor(*np.shape(F)) * U * mag
    err = np.maximum(np.abs(got.real - O.real), np.abs(got.imag - O.imag))
    ok = bool((err <= bound).all())
    ratio = float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))
    return ratio, ok
