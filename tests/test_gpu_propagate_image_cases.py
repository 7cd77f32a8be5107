"""The rows of tests/propagate_image_cases.py on the GPU: the focus metrics (csrc/propagate_focus.hip) and the transfer
function (csrc/propagate_otf.hip) of a propagated image at the shapes that reach the second tile of the finish kernel, the
doubled chunk, peaks on chunk and plane edges, the 8-byte reads of the sums over two chunks, the tiled plan's result, and
the row and column passes of the transfer function over more than one tile - each against the yardsticks of
tests/propagate_focus_ref.py and tests/propagate_otf_ref.py on what the same propagator downloads.  Needs an MI355X.

Helpers, wave and bounds are those of tests/test_gpu_propagate_focus.py and tests/test_gpu_propagate_otf.py, imported:
a sum of n terms within (n + 16) u sum |term| from fields and n u sum |term| from the sums (focus), each of re and im within
(n + 96) u sum |term| from fields and (n + 80) from the sums (transfer function), u = 2^-53.  The counts inside the radii
are asserted against a count in integers, 4 (i^2 + j^2) < (2 q + 1)^2, so that discs cut by the plane's edge are held as
whole ones are.  The yardstick of the transfer function takes at most 2^20 terms per call (``_thin``): of the sets here
only 64 x 64 on 1100 x 3 is thinned - it keeps every pairing of corner values -, every other set is compared in full.
The worst ratio of an error to its bound is printed per row as a ``PARITY focus ...`` or ``PARITY otf ...`` line (run with
-s; they belong in profiles/propagate_parity.txt).  Measured: at most 0.076 of the bound from fields and 0.21 from the sums
(focus), 0.0024 (transfer function).

Bit equality across tiles.  An entry of the transfer function is the same sum in the same order whichever of the two row
kernels forms it - one row in tiles of 1024 targets (up to 8 frequencies along y) or four rows in tiles of 256 - and however
many frequencies its call has: the segments of 32 are the same and are added in ascending order.  On rows of 1100 targets
the two kernels cut the row at different places (1024 | 76 and 256 | 256 | 256 | 256 | 76), so a running sum lost, doubled
or reordered at a tile seam in either shows as unequal bits, whatever the bounds allow.

Ties of non-zero values across chunks are held only through zeros: no field of the propagator gives a constant image."""
import numpy as np
import pytest

import propagate_focus_ref as fref
import propagate_image_cases as cases
import test_gpu_propagate_focus as tf
import test_gpu_propagate_otf as to
from test_gpu_propagate_focus import ctx, ma  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

U = fref.U
THIRD = to.THIRD
# the sets of tests/test_gpu_propagate_otf.py and two more: 8 frequencies along y, the most the kernel of one row takes, and
# 33, a batch of 32 and one more in the kernel of four; the corner values among them
FREQS = dict(to.FREQS)
FREQS['2x8'] = (np.array([0.5, -0.1]), np.concatenate([to.CORNERS, to._axis64(8)[:1]]))
FREQS['3x33'] = (np.array([-0.5, 0.0, THIRD]), np.concatenate([to.CORNERS, to._axis64(9)[:26]]))
FOCUS = [(name, h) for name, row in sorted(cases.ROWS.items()) if row.entry == 'focus' for h in row.want_h]
OTF = [name for name, row in sorted(cases.ROWS.items()) if row.entry == 'otf']


def _plan(ma, ctx, name, h, **more):
    row = cases.ROWS[name]
    return tf._make(ma, ctx, name, case=(row.method, row.mx, row.my, h == 'EH'), peak_at=row.peak_at, **more)


def _counts(shape, flat, radii_in_pitches):
    """targets inside half-integer radii about target ``flat``, counted in integers"""
    pi, pj = divmod(flat, shape[1])
    i, j = np.meshgrid(np.arange(shape[0]) - pi, np.arange(shape[1]) - pj, indexing='ij')
    return [int((4 * (i * i + j * j) < int(2 * R) ** 2).sum()) for R in radii_in_pitches]


def _off_the_boundaries(shape, dx, dy, centre, radii):
    for R in radii:
        r2 = fref.inside(shape, dx, dy, *centre, R)[1]
        assert (np.abs(r2 - R * R) > 1e-9 * R * R).all()


# ---- the focus rows: records from the fields and from the sums, about the peak and about a given centre ----------------
@pytest.mark.parametrize('name, h', FOCUS, ids=['%s-%s' % nh for nh in FOCUS])
def test_focus_rows_against_the_yardstick(ma, ctx, name, h):
    row, want_h = cases.ROWS[name], h == 'EH'
    p = _plan(ma, ctx, name, h)
    d = p.propagate()
    dx, dy = tf._pitch(p)
    assert abs(dx - dy) <= 1e-12 * dx          # the argument of _half_radii: half-integer radii lie on no target
    radii, K = np.array(cases.RADII[name]) * dx, len(cases.RADII[name])
    flat, shape = cases.peak_flat(row), (row.mx, row.my)
    counts = _counts(shape, flat, cases.RADII[name])
    if K == 5:          # whole discs hold what the existing tests assert, cut ones less
        assert (counts == [1, 9, 21, 37, 69]) == cases.discs_whole(row, cases.RADII[name])
    assert counts[0] >= 1 and len(set(counts)) == K
    centre = cases.GIVEN_CENTRE.get(name)
    given_radii = np.array(cases.GIVEN_RADII) * dx
    arrays = tf._plane_arrays(p, d, want_h)
    assert len(arrays) == row.planes
    rec = tf._raw(p, radii)
    assert np.array_equal(rec, tf._raw(p, radii))                      # two calls: the same bits
    given = None
    if centre is not None:
        _off_the_boundaries(shape, dx, dy, centre, given_radii)
        given = tf._raw(p, given_radii, centre)
        assert np.array_equal(given, tf._raw(p, given_radii, centre))
        assert np.array_equal(given[:, :fref.CENTRE], rec[:, :fref.CENTRE])      # peak and moments: one pass or two, the same bits
    worst, worst_given, wants = 0.0, 0.0, []
    for q, (I, Sz, scale) in enumerate(arrays):
        # preconditions, on NumPy's values alone: one clear peak, where the table puts it
        assert int(np.argmax(I)) == flat and np.partition(I.ravel(), -2)[-2] < I.max() * (1 - 32 * U)
        want = fref.record(I, Sz, dx, dy, radii, scale=scale)
        wants.append((I, want))
        assert want['n_inside'] == counts and want['peak_index'] == flat
        tf._check_peak(rec[q], I)
        assert int(rec[q][fref.PEAK_INDEX]) == flat
        worst = max(worst, tf._check_record(rec[q], want, K, want_h))
        if centre is not None:
            want = fref.record(I, Sz, dx, dy, given_radii, centre=centre, scale=scale)
            assert want['n_inside'][0] >= 1 and len(set(want['n_inside'])) == len(given_radii)
            worst_given = max(worst_given, tf._check_record(given[q], want, len(given_radii), want_h))
    print('PARITY focus %-10s %-2s fields: worst error / bound %.4f' % (name, h, worst))
    if centre is not None:
        print('PARITY focus %-10s %-2s fields, given centre: worst error / bound %.4f' % (name, h, worst_given))
    # the sums of the same pass with weight 1: the stored doubles are the terms
    p.accumulate([1.0], reset=True)
    I_sum, Sz_sum = p.sums()
    recs = tf._raw(p, radii, source=-1)
    assert np.array_equal(recs, tf._raw(p, radii, source=-1))
    if centre is not None:
        given = tf._raw(p, given_radii, centre, source=-1)
        assert np.array_equal(given, tf._raw(p, given_radii, centre, source=-1))
        assert np.array_equal(given[:, :fref.CENTRE], recs[:, :fref.CENTRE])
    stack = (row.planes,) + shape
    worst = worst_given = 0.0
    for q in range(row.planes):
        I, Sz = I_sum.reshape(stack)[q], (Sz_sum.reshape(stack)[q] if want_h else None)
        tf._check_peak(recs[q], I, from_sums=True)
        assert int(recs[q][fref.PEAK_INDEX]) == flat
        # (without H the stored I is mostly the yardstick's own I: the same terms have the same record)
        want = wants[q][1] if not want_h and np.array_equal(I, wants[q][0]) else fref.record(I, Sz, dx, dy, radii)
        assert want['n_inside'] == counts
        worst = max(worst, tf._check_record(recs[q], want, K, want_h, from_sums=True))
        if centre is not None:          # the whole record: moments and radii of the sums in one pass
            want = fref.record(I, Sz, dx, dy, given_radii, centre=centre)
            worst_given = max(worst_given, tf._check_record(given[q], want, len(given_radii), want_h, from_sums=True))
    print('PARITY focus %-10s %-2s sums:   worst error / bound %.4f' % (name, h, worst))
    if centre is not None:
        print('PARITY focus %-10s %-2s sums,   given centre: worst error / bound %.4f' % (name, h, worst_given))
    if not want_h:   # the stored I of one member with weight 1 is the number the pass forms from its fields
        assert np.array_equal(recs, rec)


# ---- ties: every target of an all-zero field ties ----------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(cases.ZERO_PLANES))
def test_an_all_zero_field_over_several_chunks(ma, ctx, name):
    """five chunks, and 33 chunks in two finish tiles: of equals the lowest index stays - between the waves of a workgroup,
    between chunks and between the tiles of the second launch - so the peak is target 0 and the whole record is zero"""
    mx, my, expect = cases.ZERO_PLANES[name]
    zero = [np.zeros((tf.NX, tf.NY), dtype=np.complex128) for _ in range(4)]
    p = tf._make(ma, ctx, name, F=zero, case=('direct', mx, my, True))
    p.queue_sets(0, 1)
    radii = tf._half_radii(p, 3)
    for centre in (None, (mx - 1.5, my - 2.25)):
        rec = tf._raw(p, radii, centre)
        assert rec.shape == (1, 22) and rec[0, fref.PEAK_INDEX] == 0 and rec[0, fref.PEAK_I] == 0
        assert tuple(rec[0, fref.CENTRE:fref.CENTRE + 2]) == ((0.0, 0.0) if centre is None else centre)
        rec[0, fref.CENTRE:fref.CENTRE + 2] = 0
        assert not rec.any()
    p.accumulate([1.0], reset=True)
    assert not tf._raw(p, radii, source=-1).any() and not tf._raw(p, source=-1).any()
    out = p.focus(radii)
    assert not out['peak_index'].any() and not out['centre_index'].any() and not out['encircled_I'].any()


# ---- stack invariance at two chunks a plane ------------------------------------------------------------------------
@pytest.mark.parametrize('h', ['EH', 'E'])
def test_a_plane_of_the_stack_has_the_record_of_the_plane_alone(ma, ctx, h):
    """'f-stack': 1147 targets a plane, two chunks; plane 1 starts on an odd index and reads its sums 8 bytes at a time, the
    plane alone starts on 0 and reads 16 - the same numbers in the same order"""
    name = 'f-stack'
    centre = cases.GIVEN_CENTRE[name]
    p = _plan(ma, ctx, name, h)
    p.queue_sets(0, 1)
    radii = tf._half_radii(p)
    about_peak, given = tf._raw(p, radii), tf._raw(p, radii, centre)
    p.accumulate([0.75], reset=True)
    of_sums, of_sums_given = tf._raw(p, radii, source=-1), tf._raw(p, radii, centre, source=-1)
    assert not np.array_equal(about_peak[0], about_peak[1]) and not np.array_equal(about_peak[1], about_peak[2])
    for q in range(3):
        one = _plan(ma, ctx, name, h, method='fft-fine', z=q)
        one.queue_sets(0, 1)
        assert np.array_equal(tf._raw(one, radii)[0], about_peak[q]), q
        assert np.array_equal(tf._raw(one, radii, centre)[0], given[q]), q
        one.accumulate([0.75], reset=True)
        assert np.array_equal(tf._raw(one, radii, source=-1)[0], of_sums[q]), q
        assert np.array_equal(tf._raw(one, radii, centre, source=-1)[0], of_sums_given[q]), q


# ---- the transfer-function rows: every frequency set, fields and sums -------------------------------------------
@pytest.mark.parametrize('name', OTF)
def test_otf_rows_against_the_yardstick(ma, ctx, name):
    row = cases.ROWS[name]
    (h,) = row.want_h
    want_h = h == 'EH'
    p = _plan(ma, ctx, name, h)
    d = p.propagate()
    (I, Sz, scale), = tf._plane_arrays(p, d, want_h)
    sets = sorted(set(row.expect) - {'columns'})
    fields = {}
    for key in sets:
        u, v = FREQS[key]
        assert (u.size, v.size) == cases.FREQ_SHAPES[key]
        iu, iv = to._thin(I.size, u, v)
        assert (iu.size == u.size and iv.size == v.size) or key == '64x64'          # compared in full
        got = fields[key] = to._raw(p, u, v)
        assert got.shape == (1, 2, u.size, v.size) and got.tobytes() == to._raw(p, u, v).tobytes()
        print('PARITY otf %-10s fields %-5s: worst error / bound %.4f' % (name, key, to._check_plane(got[0], I, Sz, scale, u, v, want_h)))
    p.accumulate([1.0], reset=True)
    I_sum, Sz_sum = p.sums()
    for key in sets:
        u, v = FREQS[key]
        got = to._raw(p, u, v, source=-1)
        assert got.tobytes() == to._raw(p, u, v, source=-1).tobytes()
        worst = to._check_plane(got[0], I_sum, Sz_sum if want_h else None, None, u, v, want_h, from_sums=True)
        print('PARITY otf %-10s sums   %-5s: worst error / bound %.4f' % (name, key, worst))
        assert np.array_equal(got[:, 0], fields[key][:, 0])          # the stored I of one member with weight 1 is the pass's own


# ---- bit equality across the two row kernels and the column pass over several tiles ------------------------------
def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize('name', ['o-long-y', 'o-long-y-E', 'o-long-x'])
def test_an_entry_has_the_same_bits_however_the_tiles_fall(ma, ctx, name):
    """rows of 1100 targets ('o-long-y', with and without H): an entry asked for alone - the kernel of one row, tiles of 1024 -
    against its place in a call of 64 x 64 - the kernel of four rows, tiles of 256; columns of 1100 rows ('o-long-x'): the same
    entries, one frequency along x against 64.  From the fields and from the sums."""
    row = cases.ROWS[name]
    (h,) = row.want_h
    p = _plan(ma, ctx, name, h)
    p.queue_sets(0, 1)
    u, v = FREQS['64x64']
    rng = np.random.default_rng(43)
    entries = [(0, 0), (63, 63), (0, 63), (63, 0)] + [tuple(int(k) for k in rng.integers(0, 64, 2)) for _ in range(4)]
    for source in (0, -1):
        if source == -1:
            p.accumulate([0.75], reset=True)
        full = to._raw(p, u, v, source=source)
        assert np.isfinite(full).all() and full[0, 0].any() and bool(full[0, 1].any()) == (h == 'EH')
        for a, b in entries:
            assert _same_bits(to._raw(p, u[a:a + 1], v[b:b + 1], source=source)[:, :, 0, 0], full[:, :, a, b]), (source, a, b)
        for nv in (8, 9):          # either side of the two row kernels
            assert _same_bits(to._raw(p, u[:2], v[:nv], source=source), full[:, :, :2, :nv]), (source, nv)
        assert _same_bits(to._raw(p, u[:1], v, source=source), full[:, :, :1]) and _same_bits(to._raw(p, u, v[:1], source=source), full[:, :, :, :1])
