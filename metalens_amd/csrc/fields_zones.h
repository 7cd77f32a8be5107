// Plan arithmetic and argument checks of the per-zone sums of the resident near field (fields_zones.hip, ml_fields_zones), on
// the host and free of HIP types (as propagate_focus.h and farfield_beam.h): tools/fields_zones_plan.cpp and
// tests/test_fields_zones_host.py run it without a GPU.
//
// Membership.  The host hands over X2[i] = (x[i] - xc)^2, Y2[j] = (y[j] - yc)^2 and E2[z] = e[z]^2, K = n_edges ascending
// squared edges.  Sample (i, j) has r2 = X2[i] + Y2[j] - one rounded addition - and lies in zone
// searchsorted(E2, r2, side = 'left'): zone 0 is the disc r2 <= E2[0], zone z the ring E2[z - 1] < r2 <= E2[z], a sample on
// an edge belongs to the inner zone, and zone K - outside every edge - is not reported.
//
// Terms of a member, per field set, every operation rounded on its own (nothing is contracted into an FMA):
//   S  = 0.5 ((Ex.r Hy.r + Ex.i Hy.i) - (Ey.r Hx.r + Ey.i Hx.i)),  Ix = Ex.r^2 + Ex.i^2,  Iy likewise,
//   Cx = Ex conj(w): re = Ex.r c + Ex.i s, im = Ex.i c - Ex.r s, Cy likewise, (c, s) = (cos phi, sin phi) by sincos_cw
// with the reference phase  phi = ra[i] + rb[j]  (PASS_REF_PLANE)  or  phi = sk sqrt((ra[i] + rb[j]) + ref_c ref_c),
// sk = -sign(ref_c) k, by the correctly rounded square root (PASS_REF_FOCUS).
//
// The record of (field set, zone) has ZONES_RECORD = 8 doubles: [ZONES_N] the members, [ZONES_S] sum S, [ZONES_IX] sum Ix,
// [ZONES_IY] sum Iy, [ZONES_CX] Re, Im of sum Cx, [ZONES_CY] Re, Im of sum Cy.
//
// Order of a sum - a fixed tree over the grid positions, of (nx, ny) and the line vertex alone, in which a sample that is
// no member of the zone adds +0.0 (so the sum of a zone does not depend on the other edges, sets or calls):
//   1. Line i (fixed x, j contiguous) is cut into blocks of PASS_BLOCK = 64 samples, block b = samples 64 b ... 64 b + 63,
//      and at the vertex jv - the first minimum of Y2 - into the side L, j <= jv, and the side R, j > jv; the block that
//      holds jv counts once per side.  Y2 falls to jv and rises again (zones_check holds the caller to that), so along a
//      side the zone index is monotone and the members of a zone on one side of a line are ONE run of samples.
//   2. Per (block, side) the members' terms are added by a butterfly over the 64 lanes (lanes 32, 16, 8, 4, 2, 1 apart),
//      zeros elsewhere.
//   3. The run's sum: the blocks' sums in ascending block order, the first onto +0.0.  A wave walks the line and leaves
//      every finished run as one ZoneRun of 64 bytes in the line's list, the runs of L (zones descending) in front of
//      those of R (zones ascending).  A line has at most zones_run_capacity(ny, K) runs.
//   4. A second launch takes one workgroup of ZONES_SUM_THREADS = 256 lanes per (zone, set): lane l visits the lines
//      l, l + 256, ... in ascending order and adds, per line, the zone's run of L and then of R (found by bisection), the
//      first onto +0.0; then a butterfly over each wave and the four waves in their order, ((w0 + w1) + w2) + w3.
// The members are counted as integers.
#pragma once

#include "fields_pass.h"

namespace ml {

constexpr int ZONES_EDGES_MAX = 4096;     // K at the most: 32 KB of squared edges in the LDS
constexpr int ZONES_SUM_THREADS = 256;    // lanes of a workgroup of the second launch
constexpr int ZONES_RUN_BYTES = 64;       // a ZoneRun: zone, members, 7 sums
constexpr int ZONES_N = 0, ZONES_S = 1, ZONES_IX = 2, ZONES_IY = 3, ZONES_CX = 4, ZONES_CY = 6;
constexpr int ZONES_RECORD = 8;           // doubles of a record
constexpr int ZONES_TERMS = 7;

// runs a line can leave, both sides together: every run holds a sample of its own, and a side meets a zone once
inline long long zones_run_capacity(int ny, int K) { return ny < 2LL * K ? ny : 2LL * K; }

// bytes of scratch of a call: the lines' run lists per set and two run counts per line
inline long long zones_scratch_bytes(int sets, int nx, int ny, int K) {
    return (long long)sets * nx * zones_run_capacity(ny, K) * ZONES_RUN_BYTES + (long long)nx * 8;
}

// ... which stay below the bound the interface states, sets nx min(ny + 2, 2 K + 2) 64
inline long long zones_scratch_bound(int sets, int nx, int ny, int K) {
    return (long long)sets * nx * (zones_run_capacity(ny, K) + 2) * ZONES_RUN_BYTES;
}

// The argument checks of ml_fields_zones.  -> 0; -1: an argument error, -2: the state does not allow the call; `why` is
// filled then.
inline int zones_check(const PassState &s, int first_set, int n_sets, const double *x2, int nx, const double *y2, int ny,
                       const double *e2, int n_edges, int ref_mode, const double *ra, const double *rb, double ref_c, double k,
                       int record_doubles, char *why, size_t why_len) {
    const PassWhy w{"ml_fields_zones", why, why_len};
    if (int rc = pass_check_comm(w, s.n_ranks)) return rc;
    if (int rc = pass_check_set_count(w, n_sets)) return rc;
    if (int rc = pass_check_edge_count(w, n_edges, 1, ZONES_EDGES_MAX)) return rc;
    if (int rc = pass_check_ref_mode(w, ref_mode)) return rc;
    if (record_doubles < ZONES_RECORD)
        return pass_refuse(w, -1, "record_doubles = %d: a record has %d doubles", record_doubles, ZONES_RECORD);
    if (int rc = pass_check_axes(w, nx, ny)) return rc;
    if (!x2 || !y2 || !e2 || !ra || !rb) return pass_refuse(w, -1, "NULL argument");
    if (int rc = pass_check_resident(w, s)) return rc;
    if (int rc = pass_check_shape(w, s, nx, ny)) return rc;
    if (int rc = pass_check_set_range(w, s, first_set, n_sets)) return rc;
    if (int rc = pass_check_squared_axes(w, x2, nx, y2, ny)) return rc;
    if (int rc = pass_check_edges(w, e2, n_edges)) return rc;
    if (int rc = pass_check_vertex(w, y2, ny)) return rc;
    return pass_check_ref_wave(w, ref_mode, ra, nx, rb, ny, ref_c, k);
}

}  // namespace ml
