"""Yardstick of the beam metrics of a far-field map (csrc/farfield_beam.hip behind ml_farfield_beam) for
tests/farfield_beam_cases.py: from a float64 map the terms t0 ... t5 of csrc/farfield_beam.h, formed with NumPy's own
single-rounded operations - the device forms the same doubles -, each summed exactly (math.fsum); the peak, the lowest
index of equals, the finite count, the centre, and per cone the directions inside and exactly on its edge.  The plan
arithmetic of farfield_beam.h restated (tools/farfield_beam_plan.cpp prints the header's own), and from it
beam_bound_units.  NumPy and math only; no test is collected from here."""
import math

import numpy as np

U = 2.0 ** -53
THREADS, CHUNK_MIN, CHUNKS_MAX, CONES_MAX, FINISH_TILE, SLOTS = 256, 1024, 1024, 32, 32, 4096
PEAK_P, PEAK_INDEX, FINITE, MOM, CENTRE, K, CONE = 0, 1, 2, 3, 9, 11, 12
RECORD = CONE + CONES_MAX
PARTIAL_CONE, PARTIAL = 9, 9 + CONES_MAX


def chunk_directions(n):
    c = CHUNK_MIN
    while -(-n // c) > CHUNKS_MAX:
        c *= 2
    return c


def plan(n):
    """what `farfield_beam_plan n` prints"""
    chunk = chunk_directions(n)
    chunks = -(-n // chunk)
    tiles = -(-chunks // FINISH_TILE)
    roundings = (chunk // THREADS - 1) + 6 + 3 + (min(chunks, FINISH_TILE) - 1) + (tiles - 1)
    return dict(n=n, chunk=chunk, chunks=chunks, steps=chunk // THREADS, last=n - (chunks - 1) * chunk, finish_tile=FINISH_TILE,
                finish_tiles=tiles, last_tile=chunks - (tiles - 1) * FINISH_TILE, roundings=roundings)


def beam_bound_units(n):
    """the roundings between the exact sum of the terms and the record's sum, in units of 2**-53 of sum |term|, counted
    from the order csrc/farfield_beam.h documents: a lane adds chunk / 256 terms one after the other, the first onto 0
    (chunk / 256 - 1 roundings); the butterfly over the wave (6); the four waves in their order (3); a lane adds the
    partial records of a tile of 32 chunks in index order, the first onto 0 (min(chunks, 32) - 1); a lane adds the tiles
    in index order (tiles - 1).  One unit more for the second order of the product of the (1 + u) factors (the count
    stays below 2**10, so the second order is below 2**-33 of a unit each) and for the final rounding of math.fsum."""
    return plan(n)['roundings'] + 1


def cell_of(ux, uy, pair_list):
    """dux * duy as the library takes it: the axes' first steps, a factor 1 for an axis of one direction, 1 for a pair list"""
    if pair_list:
        return 1.0
    cell = 1.0
    if len(ux) > 1:
        cell *= ux[1] - ux[0]
    if len(uy) > 1:
        cell *= uy[1] - uy[0]
    return float(cell)


def peak_of(P):
    """-> (peak, flat index) over the finite P, the lowest index of equals; (nan, -1) if nothing is finite"""
    flat = np.asarray(P, dtype=float).ravel()
    ok = np.isfinite(flat)
    if not ok.any():
        return float('nan'), -1
    at = int(np.argmax(np.where(ok, flat, -np.inf)))     # (argmax returns the first of equals)
    return float(flat[at]), at


def offsets(ux, uy, pair_list, centre):
    """dx, dy of P's shape: ux[i] - cx, uy[j] - cy, one rounding each"""
    dx = np.asarray(ux, dtype=float) - centre[0]
    dy = np.asarray(uy, dtype=float) - centre[1]
    if pair_list:
        return dx, dy
    shape = (dx.size, dy.size)
    return np.broadcast_to(dx[:, None], shape), np.broadcast_to(dy[None, :], shape)


def cone_masks(ux, uy, pair_list, cone, centre):
    """-> (inside, on_edge) boolean, of P's shape: dx * dx + dy * dy <= cone * cone with every operation rounded on its
    own, and where the two sides are equal"""
    dx, dy = offsets(ux, uy, pair_list, centre)
    rho2 = dx * dx + dy * dy
    lim = float(cone) * float(cone)
    return rho2 <= lim, rho2 == lim


def record(P, ux, uy, pair_list, cones, centre=None):
    """the record of a map.  cones: ascending, as the device takes them; centre: (cx, cy) or None for the map's own peak
    direction.  -> dict: peak, index, finite, centre, k; mom = [sum t0 ... sum t5] and mom_abs = the sums of |t|; cone,
    cone_abs likewise per cone; inside, on_edge = per cone the FINITE directions inside it and those of them exactly on
    its edge"""
    P = np.asarray(P, dtype=float)
    ux, uy = np.asarray(ux, dtype=float), np.asarray(uy, dtype=float)
    assert P.shape == ((ux.size,) if pair_list else (ux.size, uy.size))
    cones = [float(c) for c in cones]
    assert len(cones) <= CONES_MAX and all(b >= a for a, b in zip(cones, cones[1:]))
    peak, at = peak_of(P)
    ok = np.isfinite(P)
    if centre is None:
        if at < 0:
            centre = (float('nan'), float('nan'))
        else:
            centre = (float(ux[at]), float(uy[at])) if pair_list else (float(ux[at // uy.size]), float(uy[at % uy.size]))
    out = dict(peak=peak, index=at, finite=int(ok.sum()), centre=(float(centre[0]), float(centre[1])), k=len(cones))
    if at < 0:
        zero = [0.0] * len(cones)
        out.update(mom=[0.0] * 6, mom_abs=[0.0] * 6, cone=zero, cone_abs=zero, inside=[0] * len(cones), on_edge=[0] * len(cones))
        return out
    dx, dy = offsets(ux, uy, pair_list, centre)
    dx, dy = dx[ok], dy[ok]
    t0 = (P * cell_of(ux, uy, pair_list))[ok]
    xx, yy = dx * dx, dy * dy
    terms = (t0, t0 * dx, t0 * dy, t0 * xx, t0 * yy, t0 * (dx * dy))
    out['mom'] = [math.fsum(t) for t in terms]
    out['mom_abs'] = [math.fsum(np.abs(t)) for t in terms]
    rho2 = xx + yy
    out['cone'], out['cone_abs'], out['inside'], out['on_edge'] = [], [], [], []
    for c in cones:
        inside = rho2 <= c * c
        out['cone'].append(math.fsum(t0[inside]))
        out['cone_abs'].append(math.fsum(np.abs(t0[inside])))
        out['inside'].append(int(inside.sum()))
        out['on_edge'].append(int((rho2 == c * c).sum()))
    return out


def compare(rec, want, n):
    """a device record (RECORD doubles) against `want` = record(...) of the same map of n directions: peak, index, finite
    count, centre and K exactly (NaN equal to NaN), zeros behind K, every sum within beam_bound_units(n) 2**-53 sum |term|.
    -> the worst error over bound (0 where both are 0); AssertionError with the figures otherwise"""
    rec = np.asarray(rec, dtype=float)
    assert rec.shape == (RECORD,)
    same = lambda a, b: a == b or (a != a and b != b)
    assert same(rec[PEAK_P], want['peak']), ('peak', rec[PEAK_P], want['peak'])
    assert rec[PEAK_INDEX] == want['index'], ('index', rec[PEAK_INDEX], want['index'])
    assert rec[FINITE] == want['finite'], ('finite', rec[FINITE], want['finite'])
    assert same(rec[CENTRE], want['centre'][0]) and same(rec[CENTRE + 1], want['centre'][1]), ('centre', rec[CENTRE:CENTRE + 2], want['centre'])
    assert rec[K] == want['k'], ('K', rec[K], want['k'])
    assert not rec[CONE + want['k']:].any(), 'zeros behind K'
    units, worst = beam_bound_units(n), 0.0
    pairs = [(rec[MOM + q], want['mom'][q], want['mom_abs'][q], 'mom[%d]' % q) for q in range(6)]
    pairs += [(rec[CONE + r], want['cone'][r], want['cone_abs'][r], 'cone[%d]' % r) for r in range(want['k'])]
    for got, exact, scale, what in pairs:
        err, bound = abs(got - exact), units * U * scale
        assert err <= bound, (what, got, exact, err / bound if bound else float('inf'))
        if bound:
            worst = max(worst, err / bound)
    return worst
