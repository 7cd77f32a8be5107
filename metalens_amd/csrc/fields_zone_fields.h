// Plan arithmetic and argument checks of the per-zone contributions to the field at points behind the aperture
// (fields_zone_fields.hip, ml_fields_zone_fields), on the host and free of HIP types (as fields_zones.h):
// tools/fields_zone_fields_plan.cpp and tests/test_zone_fields_host.py run it without a GPU.
//
// Definition.  The direct pair sum of the propagator (propagate.hip, propagate_pair.h), left un-added across the zones of
// ml_fields_zones: for target t and slot z
//   E_z(t) = Z k^2 / (4 pi) dx' dy' sum_{(i, j) in slot z} w { i D(J) - (i - q) Rhat x m }
//   H_z(t) =   k^2 / (4 pi) dx' dy' sum_{(i, j) in slot z} w { i D(m) + (i - q) Rhat x J }
// Membership is that of fields_zones.h to the letter - r2 = X2[i] + Y2[j], one rounded addition, zone
// searchsorted(E2, r2, 'left') - but slot K collects the samples beyond the last edge, so that the K + 1 slots of a target add
// up to the whole field.  A pair's term is formed by the inlined functions of propagate_pair.h in the order of
// propagate_kernel, the currents from the fields as that kernel stages them; the two scales multiply the finished sum once.
//
// A record: ZF_E_DOUBLES = 6 doubles, Re and Im of Ex, Ey, Ez - with H ZF_EH_DOUBLES = 12, those of Hx, Hy, Hz behind them.
// records [set][slot][target][6 or 12], samples [slot].
//
// Order of a sum - the tree of fields_zones.h over the grid positions, of (nx, ny) and the line vertex alone, in which a
// sample that is no member adds +0.0:
//   1. line i is cut into blocks of 64 samples and at the vertex jv into the sides L (j <= jv) and R; along a side the
//      slot index is monotone, so the members of a slot on one side of a line are ONE run of samples;
//   2. per (block, side) the members' terms are added by the butterfly over the 64 lanes, zeros elsewhere;
//   3. the run's sum: its blocks' sums in ascending block order, the first onto +0.0; the wave leaves every finished run
//      once, the runs of L (slots descending) in front of those of R (slots ascending);
//   4. the second launch, one workgroup of ZONES_SUM_THREADS lanes per (slot, target): lane l visits the lines l, l + 256,
//      ... in ascending order and adds per line the slot's run of L, then of R, the first onto +0.0; a butterfly over each
//      wave, the four waves as ((w0 + w1) + w2) + w3, and the scale.
// A target is walked on its own accumulators and stored in its own part of a run: its sums depend neither on the other
// targets of the call nor on where the groups of ZF_TG targets are cut; the field sets are walked one after the other.
//
// Scratch.  A run holds its slot, its members and ZF_TG targets' sums; one set and one group of targets are walked at a
// time, so a call reserves zf_scratch_bytes(nx, ny, K, want_h) whatever n_sets and n_targets are - at most
// nx min(ny + 2, 2 K + 4) (8 + 8 ZF_TG (12 or 6)) bytes (zf_scratch_bound).
#pragma once

#include "fields_zones.h"

namespace ml {

constexpr int ZF_TARGETS_MAX = 64;   // targets of a call
constexpr int ZF_TG = 4;             // targets of a walk: held in registers while a block's fields are loaded once
constexpr int ZF_E_DOUBLES = 6, ZF_EH_DOUBLES = 12;

inline int zf_record_doubles(bool want_h) { return want_h ? ZF_EH_DOUBLES : ZF_E_DOUBLES; }

// doubles of a run: (slot, members) as two ints, then [ZF_TG][6 or 12] sums
inline int zf_run_doubles(bool want_h) { return 1 + ZF_TG * zf_record_doubles(want_h); }

// runs a line can leave, both sides together: every run holds a sample of its own, and a side meets each of the K + 1
// slots once
inline long long zf_run_capacity(int ny, int K) { return ny < 2LL * (K + 1) ? ny : 2LL * (K + 1); }

// walks of a set: groups of ZF_TG targets
inline int zf_groups(int n_targets) { return (n_targets + ZF_TG - 1) / ZF_TG; }

// bytes of scratch of a call: the lines' run lists of one walk and two run counts per line
inline long long zf_scratch_bytes(int nx, int ny, int K, bool want_h) {
    return (long long)nx * zf_run_capacity(ny, K) * zf_run_doubles(want_h) * 8 + (long long)nx * 8;
}

// ... which stay below the bound the interface states
inline long long zf_scratch_bound(int nx, int ny, int K, bool want_h) {
    return (long long)nx * (zf_run_capacity(ny, K) + 2) * zf_run_doubles(want_h) * 8;
}

// The argument checks of ml_fields_zone_fields, those of zones_check in its order, then the targets and the geometry.
// -> 0; -1: an argument error, -2: the state does not allow the call; `why` is filled then.  (The largest k R of the call
// is held against the phase arithmetic by the entry: common.h prop_check_phase.)
inline int zf_check(const PassState &s, int first_set, int n_sets, double dxp, double dyp, double wavelength, double n_glass, double Z0,
                    const double *x2, int nx, const double *y2, int ny, const double *e2, int n_edges, const double *tx,
                    const double *ty, const double *tz, int n_targets, char *why, size_t why_len) {
    const PassWhy w{"ml_fields_zone_fields", why, why_len};
    if (int rc = pass_check_comm(w, s.n_ranks)) return rc;
    if (int rc = pass_check_set_count(w, n_sets)) return rc;
    if (int rc = pass_check_edge_count(w, n_edges, 1, ZONES_EDGES_MAX)) return rc;
    if (n_targets < 1 || n_targets > ZF_TARGETS_MAX)
        return pass_refuse(w, -1, "%d targets: 1 to %d are taken", n_targets, ZF_TARGETS_MAX);
    if (int rc = pass_check_axes(w, nx, ny)) return rc;
    if (!x2 || !y2 || !e2 || !tx || !ty || !tz) return pass_refuse(w, -1, "NULL argument");
    if (int rc = pass_check_resident(w, s)) return rc;
    if (int rc = pass_check_shape(w, s, nx, ny)) return rc;
    if (int rc = pass_check_set_range(w, s, first_set, n_sets)) return rc;
    if (int rc = pass_check_squared_axes(w, x2, nx, y2, ny)) return rc;
    if (int rc = pass_check_edges(w, e2, n_edges)) return rc;
    if (int rc = pass_check_vertex(w, y2, ny)) return rc;
    const char *co = "a target's coordinate must be finite";
    if (int rc = pass_check_range(w, "tx", tx, n_targets, false, co)) return rc;
    if (int rc = pass_check_range(w, "ty", ty, n_targets, false, co)) return rc;
    if (int rc = pass_check_range(w, "tz", tz, n_targets, false, co)) return rc;
    for (int t = 0; t < n_targets; ++t)
        if (!(tz[t] > 0)) return pass_refuse(w, -1, "tz[%d] = %g: a target lies behind the aperture, z > 0", t, tz[t]);
    const double geo[5] = {dxp, dyp, wavelength, n_glass, Z0};
    const char *name[5] = {"dxp", "dyp", "wavelength", "n_glass", "Z0"};
    for (int q = 0; q < 5; ++q)
        if (!(std::isfinite(geo[q]) && geo[q] > 0)) return pass_refuse(w, -1, "%s = %g: must be finite and > 0", name[q], geo[q]);
    return 0;
}

}  // namespace ml
