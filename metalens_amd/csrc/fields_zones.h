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
// with the reference phase  phi = ra[i] + rb[j]  (ZONES_REF_PLANE)  or  phi = sk sqrt((ra[i] + rb[j]) + ref_c ref_c),
// sk = -sign(ref_c) k, by the correctly rounded square root (ZONES_REF_FOCUS).
//
// The record of (field set, zone) has ZONES_RECORD = 8 doubles: [ZONES_N] the members, [ZONES_S] sum S, [ZONES_IX] sum Ix,
// [ZONES_IY] sum Iy, [ZONES_CX] Re, Im of sum Cx, [ZONES_CY] Re, Im of sum Cy.
//
// Order of a sum - a fixed tree over the grid positions, of (nx, ny) and the line vertex alone, in which a sample that is
// no member of the zone adds +0.0 (so the sum of a zone does not depend on the other edges, sets or calls):
//   1. Line i (fixed x, j contiguous) is cut into blocks of ZONES_BLOCK = 64 samples, block b = samples 64 b ... 64 b + 63,
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

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#if defined(__HIPCC__)
#define ML_ZONES_HD __host__ __device__
#else
#define ML_ZONES_HD
#endif

namespace ml {

constexpr int ZONES_EDGES_MAX = 4096;     // K at the most: 32 KB of squared edges in the LDS
constexpr int ZONES_SETS_MAX = 3;         // field sets per call (the members of a synthesis batch)
constexpr int ZONES_BLOCK = 64;           // samples of a block: one per lane of a wave
constexpr int ZONES_LINE_THREADS = 256;   // lanes of a workgroup of the first launch: four lines
constexpr int ZONES_SUM_THREADS = 256;    // lanes of a workgroup of the second launch
constexpr int ZONES_RUN_BYTES = 64;       // a ZoneRun: zone, members, 7 sums
constexpr int ZONES_N = 0, ZONES_S = 1, ZONES_IX = 2, ZONES_IY = 3, ZONES_CX = 4, ZONES_CY = 6;
constexpr int ZONES_RECORD = 8;           // doubles of a record
constexpr int ZONES_TERMS = 7;
constexpr int ZONES_REF_PLANE = 0, ZONES_REF_FOCUS = 1;
constexpr double ZONES_PHASE_LIMIT = 1e9; // common.h PHASE_LIMIT (fields_zones.hip asserts that they agree)

// blocks of a line of ny samples
ML_ZONES_HD inline int zones_blocks(int ny) { return (ny + ZONES_BLOCK - 1) / ZONES_BLOCK; }

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

// the first minimum of y2 (the vertex of every line)
inline int zones_vertex(const double *y2, int ny) {
    int jv = 0;
    for (int j = 1; j < ny; ++j)
        if (y2[j] < y2[jv]) jv = j;
    return jv;
}

// the largest |phi| the reference wave reaches over the grid: |phi| is monotone in ra[i] + rb[j], a rounded sum
inline double zones_phase_max(int ref_mode, const double *ra, int nx, const double *rb, int ny, double ref_c, double k) {
    double a_lo = ra[0], a_hi = ra[0], b_lo = rb[0], b_hi = rb[0];
    for (int i = 1; i < nx; ++i) {
        a_lo = ra[i] < a_lo ? ra[i] : a_lo;
        a_hi = ra[i] > a_hi ? ra[i] : a_hi;
    }
    for (int j = 1; j < ny; ++j) {
        b_lo = rb[j] < b_lo ? rb[j] : b_lo;
        b_hi = rb[j] > b_hi ? rb[j] : b_hi;
    }
    if (ref_mode == ZONES_REF_PLANE) return std::fmax(std::fabs(a_lo + b_lo), std::fabs(a_hi + b_hi));
    return k * std::sqrt((a_hi + b_hi) + ref_c * ref_c);
}

// What the entry knows of the context when it checks a call.
struct ZonesState {
    int n_ranks = 1;
    int nx = 0, ny = 0, n_sets = 0;   // the resident field sets (nx = 0: none)
};

static inline bool zones_bad(const char *name, const double *v, int n, bool nonneg, const char *what, char *why, size_t why_len) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i]) || (nonneg && v[i] < 0)) {
            snprintf(why, why_len, "ml_fields_zones: %s[%d] = %g: %s", name, i, v[i], what);
            return true;
        }
    return false;
}

// The argument checks of ml_fields_zones.  -> 0; -1: an argument error, -2: the state does not allow the call; `why` is
// filled then.
inline int zones_check(const ZonesState &s, int first_set, int n_sets, const double *x2, int nx, const double *y2, int ny,
                       const double *e2, int n_edges, int ref_mode, const double *ra, const double *rb, double ref_c, double k,
                       int record_doubles, char *why, size_t why_len) {
    if (s.n_ranks > 1) {
        snprintf(why, why_len, "ml_fields_zones: this context belongs to a communicator of %d ranks", s.n_ranks);
        return -1;
    }
    if (n_sets < 1 || n_sets > ZONES_SETS_MAX) {
        snprintf(why, why_len, "ml_fields_zones: a pass takes 1 to %d field sets, got %d", ZONES_SETS_MAX, n_sets);
        return -1;
    }
    if (n_edges < 1 || n_edges > ZONES_EDGES_MAX) {
        snprintf(why, why_len, "ml_fields_zones: %d edges: 1 to %d are taken", n_edges, ZONES_EDGES_MAX);
        return -1;
    }
    if (ref_mode != ZONES_REF_PLANE && ref_mode != ZONES_REF_FOCUS) {
        snprintf(why, why_len, "ml_fields_zones: ref_mode %d: %d for a plane wave or %d for a focus", ref_mode, ZONES_REF_PLANE,
                 ZONES_REF_FOCUS);
        return -1;
    }
    if (record_doubles < ZONES_RECORD) {
        snprintf(why, why_len, "ml_fields_zones: record_doubles = %d: a record has %d doubles", record_doubles, ZONES_RECORD);
        return -1;
    }
    if (nx < 1 || ny < 1) {
        snprintf(why, why_len, "ml_fields_zones: the axes have %d x %d samples: at least one each", nx, ny);
        return -1;
    }
    if (!x2 || !y2 || !e2 || !ra || !rb) {
        snprintf(why, why_len, "ml_fields_zones: NULL argument");
        return -1;
    }
    if (s.nx == 0 || s.ny == 0) {
        snprintf(why, why_len, "no resident field set");
        return -2;
    }
    if (nx != s.nx || ny != s.ny) {
        snprintf(why, why_len, "ml_fields_zones: the axes have %d x %d samples, the resident field sets %d x %d", nx, ny, s.nx, s.ny);
        return -1;
    }
    if (first_set < 0 || first_set + n_sets > s.n_sets) {
        snprintf(why, why_len, "ml_fields_zones: field sets %d ... %d asked for, %d resident", first_set, first_set + n_sets - 1, s.n_sets);
        return -1;
    }
    const char *sq = "a squared distance must be finite and >= 0";
    if (zones_bad("x2", x2, nx, true, sq, why, why_len) || zones_bad("y2", y2, ny, true, sq, why, why_len)) return -1;
    if (zones_bad("e2", e2, n_edges, true, "a squared edge must be finite and >= 0", why, why_len)) return -1;
    for (int z = 1; z < n_edges; ++z)
        if (e2[z] < e2[z - 1]) {
            snprintf(why, why_len, "ml_fields_zones: the edges must not decrease: e2[%d] = %g < e2[%d] = %g", z, e2[z], z - 1, e2[z - 1]);
            return -1;
        }
    const int jv = zones_vertex(y2, ny);
    for (int j = 1; j < ny; ++j)
        if (j <= jv ? y2[j] > y2[j - 1] : y2[j] < y2[j - 1]) {
            snprintf(why, why_len, "ml_fields_zones: y2 must fall to its minimum y2[%d] = %g and rise again (a y axis in ascending or "
                     "descending order): y2[%d] = %g follows y2[%d] = %g", jv, y2[jv], j, y2[j], j - 1, y2[j - 1]);
            return -1;
        }
    const bool focus = ref_mode == ZONES_REF_FOCUS;
    const char *rw = focus ? "a squared distance to the focus must be finite and >= 0" : "a reference phase must be finite";
    if (zones_bad("ra", ra, nx, focus, rw, why, why_len) || zones_bad("rb", rb, ny, focus, rw, why, why_len)) return -1;
    if (focus && (!std::isfinite(ref_c) || ref_c == 0)) {
        snprintf(why, why_len, "ml_fields_zones: ref_c = %g: the focus lies at a finite distance zf != 0 from the aperture", ref_c);
        return -1;
    }
    if (focus && !(std::isfinite(k) && k > 0)) {
        snprintf(why, why_len, "ml_fields_zones: k = %g: the wave number must be finite and > 0", k);
        return -1;
    }
    const double phi = zones_phase_max(ref_mode, ra, nx, rb, ny, ref_c, k);
    if (!(phi <= ZONES_PHASE_LIMIT)) {
        snprintf(why, why_len, "ml_fields_zones: the reference phase reaches %.6g rad on this grid: the phase arithmetic covers up to %g",
                 phi, ZONES_PHASE_LIMIT);
        return -1;
    }
    return 0;
}

}  // namespace ml
