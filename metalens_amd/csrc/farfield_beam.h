// Plan arithmetic of the beam metrics of a far-field map (farfield_beam.hip), on the host and free of HIP types (as
// propagate_focus.h): tools/farfield_beam_plan.cpp and tests/test_farfield_beam_host.py run it without a GPU.
//
// The map P has n directions - mx my of a tensor grid, direction (i, j) at i my + j, or mx of a pair list, direction d
// at (ux[d], uy[d]) - and is NaN outside the unit circle.  Per map the metrics are one maximum, one count and up to
// 6 + BEAM_CONES_MAX sums over the finite P; they are formed in two launches (three when the centre is the map's own
// peak): workgroups reduce CHUNKS of the map to partial records in a fixed order, a last launch of one workgroup adds
// the chunks' partials in index order.
//
// The terms of a finite direction, every operation rounded on its own (nothing is contracted into an FMA):
//   dx = ux[i] - cx, dy = uy[j] - cy;  t0 = P cell;  t1 = t0 dx;  t2 = t0 dy;  t3 = t0 (dx dx);  t4 = t0 (dy dy);
//   t5 = t0 (dx dy);  inside cone r iff dx dx + dy dy <= c_r c_r.
// cell = dux duy (beam_cell below, the one statement of it; ml_farfield_accumulate is its other user): the axes' first
// steps, a factor 1 for an axis of one direction, 1 for a pair list.
//
// The cut.  A chunk is beam_chunk_directions(n) consecutive directions: BEAM_CHUNK_MIN = 1024, doubled until the map
// has at most BEAM_CHUNKS_MAX = 1024 chunks.  It depends on n alone - not on the slot, the source, the centre or the
// cones.  The order of a sum, from the terms to the record:
//   1. lane l of the chunk's BEAM_THREADS = 256 lanes visits chunk_start + 256 s + l in step s = 0, 1, ... and adds
//      its terms in that order: beam_steps(n) = chunk / 256 terms, the first onto 0 (the loads of four steps are
//      issued together, the adds are not reordered);
//   2. a butterfly over each wave of 64 lanes (6 levels: lanes 32, 16, 8, 4, 2, 1 apart);
//   3. the four waves' values added in their order: ((w0 + w1) + w2) + w3      -> the chunk's partial record;
//   4. the last launch cuts the chunks into TILES of BEAM_FINISH_TILE = 32 consecutive partial records; one lane per
//      (tile, sum) adds the tile's records in index order, the first onto 0 (a ragged last tile adds +0.0 for the
//      records it does not have: no rounding);
//   5. one lane per sum adds the tiles' sums in index order, the first onto 0.
// Every cone has a sum of its own through all five levels (a direction outside adds +0.0): the power inside cone r does
// not depend on the other cones of the call.  beam_bound_roundings(n) counts the roundings of 1 ... 5.
// The peak is the largest finite P, of equals the lowest index - a maximum has no order; the count is an integer.
//
// Centre = the map's own peak: a first launch of the same chunks leaves every chunk's peak in a buffer of its own; each
// workgroup of the second launch reduces those (at most 1024 pairs) to the map's peak (ip, jp) and reads the centre
// (ux[ip], uy[jp]) on the device - no host round trip, no launch of one workgroup in between.
//
// A partial record of a chunk has BEAM_PARTIAL doubles: [0] the chunk's peak (-inf if no direction of it is finite), [1]
// its flat index (-1), [2] the finite count, [3 ... 8] the six sums, [9 + r] the sum of t0 inside cone r.
//
// The record of a map, in doubles (what ml_farfield_beams returns; K = n_cones):
//   [BEAM_PEAK_P]        the largest finite P; NaN if no direction is finite
//   [BEAM_PEAK_INDEX]    its flat index i my + j (pair list: i), the lowest of equals; -1 if none
//   [BEAM_FINITE]        the number of finite directions
//   [BEAM_MOM + q]       q = 0 ... 5: sum t0, t1, t2, t3, t4, t5
//   [BEAM_CENTRE]        cx, cy: the centre used; NaN if it is the peak and nothing is finite
//   [BEAM_K]             K
//   [BEAM_CONE + r]      r < K: sum of t0 inside cone r; zeros behind K
// BEAM_RECORD = BEAM_CONE + BEAM_CONES_MAX doubles, whatever K.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#if defined(__HIPCC__)
#define ML_BEAM_HD __host__ __device__
#else
#define ML_BEAM_HD
#endif

namespace ml {

constexpr int BEAM_THREADS = 256;         // lanes of a workgroup, one direction each per step
constexpr int BEAM_CHUNK_MIN = 1024;      // directions of the shortest chunk
constexpr int BEAM_CHUNKS_MAX = 1024;     // chunks of a map at the most
constexpr int BEAM_CONES_MAX = 32;
constexpr int BEAM_FINISH_THREADS = 256;  // lanes of the last launch's one workgroup
constexpr int BEAM_FINISH_TILE = 32;      // partial records one lane adds in sequence
constexpr int BEAM_FINISH_TILES_MAX = BEAM_CHUNKS_MAX / BEAM_FINISH_TILE;
constexpr int BEAM_SLOTS = 4096;          // ML_MAX_SWEEP_SLOTS

constexpr int BEAM_PEAK_P = 0, BEAM_PEAK_INDEX = 1, BEAM_FINITE = 2, BEAM_MOM = 3, BEAM_CENTRE = 9, BEAM_K = 11, BEAM_CONE = 12;
constexpr int BEAM_MOMENTS = 6;
constexpr int BEAM_RECORD = BEAM_CONE + BEAM_CONES_MAX;     // doubles of a record (ML_BEAM_RECORD)
constexpr int BEAM_PARTIAL_CONE = 9;                        // where the cone sums of a partial record begin
constexpr int BEAM_PARTIAL = BEAM_PARTIAL_CONE + BEAM_CONES_MAX;
constexpr long long BEAM_DIRECTIONS_MAX = 0x7fffffffLL;     // the peak's index travels as an int

// directions per chunk of a map of n directions: of n alone
inline long long beam_chunk_directions(long long n) {
    long long c = BEAM_CHUNK_MIN;
    while ((n + c - 1) / c > BEAM_CHUNKS_MAX) c *= 2;
    return c;
}

inline int beam_chunks(long long n) {
    const long long c = beam_chunk_directions(n);
    return (int)((n + c - 1) / c);
}

// terms a lane adds in a full chunk
inline int beam_steps(long long n) { return (int)(beam_chunk_directions(n) / BEAM_THREADS); }

// the tiles the last launch takes `chunks` partial records in, and the records of tile t of them
ML_BEAM_HD inline int beam_finish_tiles_of(int chunks) { return (chunks + BEAM_FINISH_TILE - 1) / BEAM_FINISH_TILE; }

ML_BEAM_HD inline int beam_finish_tile_chunks(int chunks, int t) {
    const int left = chunks - t * BEAM_FINISH_TILE;
    return left < BEAM_FINISH_TILE ? left : BEAM_FINISH_TILE;
}

inline int beam_finish_tiles(long long n) { return beam_finish_tiles_of(beam_chunks(n)); }

// roundings between the exact sum of the terms and the record's sum, level by level of the order above
inline int beam_bound_roundings(long long n) {
    const int chunks = beam_chunks(n), tiles = beam_finish_tiles_of(chunks);
    const int in_tile = chunks < BEAM_FINISH_TILE ? chunks : BEAM_FINISH_TILE;
    return (beam_steps(n) - 1) + 6 + 3 + (in_tile - 1) + (tiles - 1);
}

// dux duy of a map as the reference takes them (nearfield_farfield.py:71-74): the axes' first steps, 1 for an axis of
// one direction, 1 for a pair list (it has no cell).  Taken by ml_farfield_beam and by ml_farfield_accumulate
inline double beam_cell(const double *ux, int mx, const double *uy, int my, bool pair_list) {
    double cell = 1.0;
    if (!pair_list) {
        if (mx > 1) cell *= ux[1] - ux[0];
        if (my > 1) cell *= uy[1] - uy[0];
    }
    return cell;
}

// What an entry that reads the power map knows of the context when it checks a call (farfield_beam.hip beam_state fills
// it, for ml_farfield_beam and for the sweep sums of farfield_sums.hip).
struct BeamState {
    bool projected = false;    // the active plan holds radiation vectors
    bool scattered = false;    // its power map is reduce-scattered over the ranks and not gathered
    long long n = 0;           // directions of the active plan
    bool pair_list = false;
    long long acc_n = 0;       // directions of the plan P_sum was started on, 0: no sums
    bool acc_pair_list = false;
};

// Can the power map be read whole?  The two refusals every such entry shares.  -> 0, or -2 with `why` filled.
inline int beam_check_map(const BeamState &s, char *why, size_t why_len) {
    if (!s.projected) {
        snprintf(why, why_len, "nothing projected: call ml_farfield_transform and ml_farfield_project first");
        return -2;
    }
    if (s.scattered) {
        // after a reduce-scatter a rank holds the power of ITS block of direction rows only: sums over the whole map
        // would mix it with stale rows
        snprintf(why, why_len, "the power map is reduce-scattered over the ranks: call ml_farfield_gather before summing it");
        return -2;
    }
    return 0;
}

// The argument checks of ml_farfield_beam.  -> 0; -1: an argument error, -2: the state does not allow the call; `why`
// is filled then.  source 0: the current projection, -1: P_sum.  centre: {cx, cy} or NULL (the map's peak).
inline int beam_check(const BeamState &s, int source, const double *centre, const double *cones, int n_cones, int slot,
                      char *why, size_t why_len) {
    if (source != 0 && source != -1) {
        snprintf(why, why_len, "ml_farfield_beam: source %d: 0 for the current projection or -1 for P_sum", source);
        return -1;
    }
    if (slot < 0 || slot >= BEAM_SLOTS) {
        snprintf(why, why_len, "ml_farfield_beam: slot %d out of range [0, %d)", slot, BEAM_SLOTS);
        return -1;
    }
    if (n_cones < 0 || n_cones > BEAM_CONES_MAX) {
        snprintf(why, why_len, "ml_farfield_beam: %d cones: 0 to %d are taken", n_cones, BEAM_CONES_MAX);
        return -1;
    }
    if (n_cones > 0 && !cones) {
        snprintf(why, why_len, "ml_farfield_beam: %d cones asked for, cones is NULL", n_cones);
        return -1;
    }
    for (int r = 0; r < n_cones; ++r) {
        if (!std::isfinite(cones[r]) || cones[r] < 0) {
            snprintf(why, why_len, "ml_farfield_beam: cones[%d] = %g: the sine of a half-angle must be finite and >= 0", r, cones[r]);
            return -1;
        }
        if (r > 0 && cones[r] < cones[r - 1]) {
            snprintf(why, why_len, "ml_farfield_beam: the cones must not decrease: cones[%d] = %g < cones[%d] = %g", r, cones[r],
                     r - 1, cones[r - 1]);
            return -1;
        }
    }
    if (centre && (!std::isfinite(centre[0]) || !std::isfinite(centre[1]))) {
        snprintf(why, why_len, "ml_farfield_beam: the centre is (%g, %g): it must be finite", centre[0], centre[1]);
        return -1;
    }
    if (beam_check_map(s, why, why_len) != 0) return -2;
    if (s.n < 1 || s.n > BEAM_DIRECTIONS_MAX) {
        snprintf(why, why_len, "ml_farfield_beam: the active plan has %lld directions: 1 to %lld are taken", s.n, BEAM_DIRECTIONS_MAX);
        return -1;
    }
    if (source == -1) {
        if (!s.acc_n) {
            snprintf(why, why_len, "ml_farfield_beam: this context has no sums yet (ml_farfield_accumulate has not run)");
            return -2;
        }
        if (s.acc_n != s.n || s.acc_pair_list != s.pair_list) {
            snprintf(why, why_len, "ml_farfield_beam: the sums were started on a plan of %lld directions (%s), the active plan has "
                     "%lld (%s)", s.acc_n, s.acc_pair_list ? "pair list" : "tensor grid", s.n, s.pair_list ? "pair list" : "tensor grid");
            return -2;
        }
    }
    return 0;
}

// ... and of ml_farfield_beams
inline int beams_check(int first_slot, int n_slots, char *why, size_t why_len) {
    if (first_slot < 0 || first_slot >= BEAM_SLOTS) {
        snprintf(why, why_len, "ml_farfield_beams: first_slot %d out of range [0, %d)", first_slot, BEAM_SLOTS);
        return -1;
    }
    if (n_slots < 0 || first_slot + (long long)n_slots > BEAM_SLOTS) {
        snprintf(why, why_len, "ml_farfield_beams: %d slots from slot %d on: the slots are [0, %d)", n_slots, first_slot, BEAM_SLOTS);
        return -1;
    }
    return 0;
}

}  // namespace ml
