// Plan arithmetic of the focus metrics of a propagated image (propagate_focus.hip), on the host and free of HIP
// types (as propagate_grid.h and lens_pack.h): tools/propagate_focus_plan.cpp and tests/test_propagate_focus_host.py
// run it without a GPU.
//
// The resident result of a propagation plan is `planes` planes of mx x my targets, target (i, j) of plane p at
// (p mx + i) my + j.  Per plane the metrics are sums over its P = mx my targets and one maximum; they are formed in two
// launches: workgroups reduce CHUNKS of a plane to partial records in a fixed order, a second launch adds the chunks'
// partials in index order.
//
// The cut.  A chunk is focus_chunk_targets(P) consecutive targets of a plane: FOCUS_CHUNK_MIN = 1024, doubled until a
// plane has at most FOCUS_CHUNKS_MAX = 1024 chunks (what the second launch adds one after another).  It depends on P =
// mx my alone - not on the number of planes, the plane, the member or the source - so plane p of a stack is reduced with
// the bits of that plane planned alone.  Within a chunk the workgroup's FOCUS_THREADS = 256 lanes take the targets two
// by two: lane l visits chunk_start + 512 s + 2 l and the target behind it in step s = 0, 1, ...
//
// The record of a plane, in doubles (what ml_propagate_focus returns; K = n_radii):
//   [FOCUS_PEAK_I]          the largest I = |E|^2 of the plane (the sums: the largest stored I_sum)
//   [FOCUS_PEAK_INDEX]      its flat index i my + j within the plane, the lowest one of equals
//   [FOCUS_MOM_I + q]       q = 0 ... 5: sum w, sum w i, sum w j, sum w i^2, sum w j^2, sum w i j  with w = I
//   [FOCUS_MOM_SZ + q]      the same with w = Sz (zeros for a plan without H)
//   [FOCUS_CENTRE]          ci, cj: the centre the radii were taken about, in index units
//   [FOCUS_ENC + r]         r < K: sum of I over the targets inside radius r
//   [FOCUS_ENC + K + r]     r < K: sum of Sz over them (zeros for a plan without H)
// focus_record_doubles(K) = FOCUS_ENC + 2 K.
//
// A partial record of a chunk has FOCUS_PARTIAL doubles: the chunk's peak and its index, the twelve sums, and behind
// them [annulus][I, Sz] for FOCUS_RADII_MAX annuli: annulus a holds the targets inside radius a that are outside every
// radius before it (the radii are sorted: disjoint sets, summed one by one and accumulated by the second launch).
//
// The second launch takes the chunks' partial records through the LDS FOCUS_FINISH_TILE = 32 at a time, in index order:
// focus_finish_tiles(P) tiles, the last of focus_finish_tile_chunks(chunks, tiles - 1) records.  The sums and the peak
// are carried from tile to tile, so the tiles change no order.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#if defined(__HIPCC__)
#define ML_FOCUS_HD __host__ __device__
#else
#define ML_FOCUS_HD
#endif

namespace ml {

constexpr int FOCUS_THREADS = 256;        // lanes of a workgroup
constexpr int FOCUS_STEP = 2 * FOCUS_THREADS;   // targets a workgroup takes per step
constexpr int FOCUS_CHUNK_MIN = 1024;     // targets of the shortest chunk
constexpr int FOCUS_CHUNKS_MAX = 1024;    // chunks of a plane at the most
constexpr int FOCUS_RADII_MAX = 32;
constexpr int FOCUS_FINISH_THREADS = 256; // lanes of the second launch's workgroup, one per plane
constexpr int FOCUS_FINISH_TILE = 32;     // partial records that lie in its LDS at once

constexpr int FOCUS_PEAK_I = 0, FOCUS_PEAK_INDEX = 1, FOCUS_MOM_I = 2, FOCUS_MOM_SZ = 8, FOCUS_CENTRE = 14, FOCUS_ENC = 16;
constexpr int FOCUS_MOMENTS = 6;
constexpr int FOCUS_PARTIAL_ANNULI = 14;                                    // where the annuli of a partial record begin
constexpr int FOCUS_PARTIAL = FOCUS_PARTIAL_ANNULI + 2 * FOCUS_RADII_MAX;   // doubles of a partial record

inline int focus_record_doubles(int n_radii) { return FOCUS_ENC + 2 * n_radii; }

// targets per chunk of a plane of P targets: of P alone
inline long long focus_chunk_targets(long long P) {
    long long c = FOCUS_CHUNK_MIN;
    while ((P + c - 1) / c > FOCUS_CHUNKS_MAX) c *= 2;
    return c;
}

inline int focus_chunks(long long P) {
    const long long c = focus_chunk_targets(P);
    return (int)((P + c - 1) / c);
}

// the tiles the second launch takes `chunks` partial records in, and the records of tile t of them
ML_FOCUS_HD inline int focus_finish_tiles_of(int chunks) { return (chunks + FOCUS_FINISH_TILE - 1) / FOCUS_FINISH_TILE; }

ML_FOCUS_HD inline int focus_finish_tile_chunks(int chunks, int t) {
    const int left = chunks - t * FOCUS_FINISH_TILE;
    return left < FOCUS_FINISH_TILE ? left : FOCUS_FINISH_TILE;
}

inline int focus_finish_tiles(long long P) { return focus_finish_tiles_of(focus_chunks(P)); }

// What the entry knows of the active plan when it checks a call.
struct FocusState {
    bool have_result = false, have_sums = false;
    int T = 0, result_sets = 0;
};

// The argument checks of ml_propagate_focus.  -> 0; -1: an argument error, -2: the state does not allow the call; `why`
// is filled then.  source >= 0: member of the last pass, -1: the sums.  centre: [planes][2] or NULL (every plane's peak).
inline int focus_check(const FocusState &s, int source, int mx, int my, int planes, double dx, double dy, const double *centre,
                       const double *radii, int n_radii, int record_doubles, char *why, size_t why_len) {
    if (!s.have_result) {
        snprintf(why, why_len, "ml_propagate has not run on the active propagation plan");
        return -2;
    }
    if (source < -1) {
        snprintf(why, why_len, "ml_propagate_focus: source %d: a member of the last pass (>= 0) or -1 for the sums", source);
        return -1;
    }
    if (source == -1 && !s.have_sums) {
        snprintf(why, why_len, "ml_propagate_accumulate has not run on the active propagation plan");
        return -2;
    }
    if (source >= s.result_sets) {
        snprintf(why, why_len, "ml_propagate_focus: member %d asked for, the last pass propagated %d field sets", source,
                 s.result_sets);
        return -1;
    }
    if (mx < 1 || my < 1 || planes < 1 || (long long)mx * my * planes != s.T) {
        snprintf(why, why_len, "ml_propagate_focus: %d planes of %d x %d targets are %lld targets, the active propagation plan "
                 "has %d", planes, mx, my, (long long)mx * my * planes, s.T);
        return -1;
    }
    if (!(dx > 0) || !(dy > 0) || !std::isfinite(dx) || !std::isfinite(dy)) {
        snprintf(why, why_len, "ml_propagate_focus: the targets' pitch must be finite and > 0, got dx = %g, dy = %g", dx, dy);
        return -1;
    }
    if (n_radii < 0 || n_radii > FOCUS_RADII_MAX) {
        snprintf(why, why_len, "ml_propagate_focus: %d radii: 0 to %d are taken", n_radii, FOCUS_RADII_MAX);
        return -1;
    }
    if (n_radii > 0 && !radii) {
        snprintf(why, why_len, "ml_propagate_focus: %d radii asked for, radii is NULL", n_radii);
        return -1;
    }
    for (int r = 0; r < n_radii; ++r) {
        if (!std::isfinite(radii[r]) || radii[r] < 0) {
            snprintf(why, why_len, "ml_propagate_focus: radii[%d] = %g: a radius must be finite and >= 0", r, radii[r]);
            return -1;
        }
        if (r > 0 && radii[r] < radii[r - 1]) {
            snprintf(why, why_len, "ml_propagate_focus: the radii must not decrease: radii[%d] = %g < radii[%d] = %g", r,
                     radii[r], r - 1, radii[r - 1]);
            return -1;
        }
    }
    if (centre)
        for (int p = 0; p < planes; ++p)
            if (!std::isfinite(centre[2 * p]) || !std::isfinite(centre[2 * p + 1])) {
                snprintf(why, why_len, "ml_propagate_focus: the centre of plane %d is (%g, %g): it must be finite", p,
                         centre[2 * p], centre[2 * p + 1]);
                return -1;
            }
    if (record_doubles < focus_record_doubles(n_radii)) {
        snprintf(why, why_len, "ml_propagate_focus: a record of %d radii has %d doubles, record_doubles = %d", n_radii,
                 focus_record_doubles(n_radii), record_doubles);
        return -1;
    }
    return 0;
}

}  // namespace ml
