// The overlap of a propagated image with separable modes (propagate_modes.hip, ml_propagate_modes_plan / _queue / _fetch):
// what host and device share - the order of the sums, the launch shapes, the argument checks and the caps - free of HIP
// types (as propagate_otf.h): tools/propagate_modes_plan.cpp and tests/test_propagate_modes_host.py run it without a GPU.
//
//   O_F[p][a][b] = sum_i sum_j conj(mode_x[a][i]) conj(mode_y[b][j]) F(p, i, j),   F in (Ex, Ey, Hx, Hy), a < nu, b < nv
//
// The tables.  The plan entry conjugates the caller's tables on the host - a sign, exact - and lays them index-major:
// Tx[i][a] = conj(mode_x[a][i]), Ty[j][b] = conj(mode_y[b][j]), so that the lanes of a wave, which differ in the mode, read
// neighbours.
//
// The order.  The contraction is separable: a row pass R_F(i, b) = sum_j F(i, j) Ty(j, b) and a column pass O_F(a, b) =
// sum_i Tx(i, a) R_F(i, b).  A complex product x t is re = x.r t.r - x.i t.i, im = x.r t.i + x.i t.r, every product, the
// difference and the sum rounded on their own.  Both sums run over SEGMENTS of MODES_SEGMENT = 32 consecutive indices (the
// segments of propagate_otf.h): a segment's terms are added one after another from 0, in ascending index, and the
// segments' sums are added one after another from 0, in ascending index.  The order depends on (mx, my) alone - not on
// the planes, the plane, the member, the slot, nu, nv or the other modes -, so an entry is repeatable bit for bit, plane
// p of a stack has the bits of that plane planned alone, and an entry of a call of 64 x 64 modes has the bits of the
// same pair of modes asked for alone.
//
// The caps: mx nu + my nv <= 2^24 table entries (256 MiB), planes mx nv <= 2^25 row sums per component (2 GiB for the
// four), n_slots planes 4 nu nv <= 2^24 output entries (256 MiB), at most 65535 planes (a dimension of the launch grids).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "propagate_otf.h"

namespace ml {

constexpr int MODES_MAX = 64;                       // modes per axis and plan (ML_MODES_MAX)
constexpr int MODES_SEGMENT = OTF_SEGMENT;          // indices whose terms are added one after another
constexpr int MODES_COMPONENTS = 4;                 // Ex, Ey, Hx, Hy: the blocks of an output slot
constexpr int MODES_SLOTS_MAX = 4096;               // output slots of a plan (ML_MAX_SWEEP_SLOTS)
constexpr long long MODES_TABLE_MAX = 1LL << 24;    // mx nu + my nv table entries at the most
constexpr long long MODES_ROWS_MAX = 1LL << 25;     // planes mx nv entries of R per component at the most
constexpr long long MODES_OUT_MAX = 1LL << 24;      // n_slots planes 4 nu nv output entries at the most
constexpr int MODES_PLANES_MAX = OTF_PLANES_MAX;    // planes per plan: a dimension of the launch grids

// The launch shapes of the two passes (the kernels and launchers of propagate_modes.hip call these; tools/
// propagate_modes_plan.cpp prints them).  The row pass takes a row in tiles of MODES_TILE_FEW = 512 targets whose four
// complex components lie in the LDS at once - 64 B per target, four times what a target of the transfer function takes -
// or, above MODES_FEW modes nv, MODES_ROWS_MANY = 2 rows in tiles of 128 targets of each, all nv modes in one batch.  The
// column pass takes the rows in tiles of MODES_COLUMN_TILE.  A tile is whole segments but for the last one of an axis, so
// the tiles cut no segment and change no order.
constexpr int MODES_TILE_FEW = 512;                   // targets of the one row whose fields lie in the LDS at once, nv <= MODES_FEW
constexpr int MODES_FEW = 8, MODES_ROWS_MANY = 2;     // above MODES_FEW modes nv a workgroup takes 2 rows
constexpr int MODES_TILE_MANY = 128;                  // targets of each of the two rows per tile then
constexpr int MODES_COLUMN_TILE = 1024;               // rows per tile of the column pass
static_assert(MODES_TILE_FEW % MODES_SEGMENT == 0 && MODES_TILE_MANY % MODES_SEGMENT == 0 && MODES_COLUMN_TILE % MODES_SEGMENT == 0,
              "whole segments per tile in every kernel");

ML_OTF_HD inline int modes_segments(int n) { return otf_segments(n); }

ML_OTF_HD inline int modes_rows_per_group(int nv) { return nv <= MODES_FEW ? 1 : MODES_ROWS_MANY; }

ML_OTF_HD inline int modes_row_tile(int nv) { return nv <= MODES_FEW ? MODES_TILE_FEW : MODES_TILE_MANY; }

struct ModesRowsShape {
    int rows;            // rows of a plane per workgroup: 1 or MODES_ROWS_MANY
    int tile;            // targets of each row per tile
    int tiles;           // tiles per row
    int last_segments;   // segments of the last tile
    int last_segment;    // indices of its last segment
    int groups;          // workgroups along x
    int last_rows;       // live rows of the last of them
};

inline ModesRowsShape modes_rows_shape(int mx, int my, int nv) {
    ModesRowsShape s;
    s.rows = modes_rows_per_group(nv);
    s.tile = modes_row_tile(nv);
    s.tiles = otf_tiles(my, s.tile);
    const int last = otf_tile_len(my, s.tile, s.tiles - 1);
    s.last_segments = modes_segments(last);
    s.last_segment = last - (s.last_segments - 1) * MODES_SEGMENT;
    s.groups = otf_tiles(mx, s.rows);
    s.last_rows = otf_live_rows(mx, s.rows, s.groups - 1);
    return s;
}

struct ModesColumnsShape {
    int tiles;           // tiles of MODES_COLUMN_TILE rows
    int last_segments;   // segments of the last tile
    int last_segment;    // indices of its last segment
};

inline ModesColumnsShape modes_columns_shape(int mx) {
    ModesColumnsShape s;
    s.tiles = otf_tiles(mx, MODES_COLUMN_TILE);
    const int last = otf_tile_len(mx, MODES_COLUMN_TILE, s.tiles - 1);
    s.last_segments = modes_segments(last);
    s.last_segment = last - (s.last_segments - 1) * MODES_SEGMENT;
    return s;
}

// What the plan entry leaves with the active propagation plan (and what the other two entries check against)
struct ModesState {
    bool planned = false;
    int mx = 0, my = 0, planes = 0, nu = 0, nv = 0, n_slots = 0;
};

// The argument checks of ml_propagate_modes_plan.  -> 0; -1: an argument error; `why` is filled then.  T: the targets of
// the active propagation plan (0: none).  mode_x, mode_y: (re, im) pairs, [nu][mx] and [nv][my].
inline int modes_plan_check(long long T, int mx, int my, int planes, const double *mode_x, int nu, const double *mode_y, int nv,
                            int n_slots, char *why, size_t why_len) {
    if (mx < 1 || my < 1 || planes < 1 || (long long)mx * my * planes != T) {
        snprintf(why, why_len, "ml_propagate_modes_plan: %d planes of %d x %d targets are %lld targets, the active propagation "
                 "plan has %lld", planes, mx, my, (long long)mx * my * planes, T);
        return -1;
    }
    if (planes > MODES_PLANES_MAX) {
        snprintf(why, why_len, "ml_propagate_modes_plan: %d planes, at most %d are taken per plan", planes, MODES_PLANES_MAX);
        return -1;
    }
    if (nu < 1 || nu > MODES_MAX || nv < 1 || nv > MODES_MAX) {
        snprintf(why, why_len, "ml_propagate_modes_plan: %d x %d modes: 1 to %d are taken per axis", nu, nv, MODES_MAX);
        return -1;
    }
    if (!mode_x || !mode_y) {
        snprintf(why, why_len, "ml_propagate_modes_plan: NULL argument (mode_x %s, mode_y %s)", mode_x ? "given" : "NULL",
                 mode_y ? "given" : "NULL");
        return -1;
    }
    if (n_slots < 1 || n_slots > MODES_SLOTS_MAX) {
        snprintf(why, why_len, "ml_propagate_modes_plan: %d output slots: 1 to %d are reserved per plan", n_slots, MODES_SLOTS_MAX);
        return -1;
    }
    const long long table = (long long)mx * nu + (long long)my * nv;
    if (table > MODES_TABLE_MAX) {
        snprintf(why, why_len, "ml_propagate_modes_plan: %d x %d + %d x %d = %lld table entries, at most 2^24 = %lld are held",
                 mx, nu, my, nv, table, MODES_TABLE_MAX);
        return -1;
    }
    const long long rows = (long long)planes * mx * nv;
    if (rows > MODES_ROWS_MAX) {
        snprintf(why, why_len, "ml_propagate_modes_plan: %d planes x %d rows x %d modes = %lld row sums per component, at most "
                 "2^25 = %lld are held", planes, mx, nv, rows, MODES_ROWS_MAX);
        return -1;
    }
    const long long out = (long long)n_slots * planes * MODES_COMPONENTS * nu * nv;
    if (out > MODES_OUT_MAX) {
        snprintf(why, why_len, "ml_propagate_modes_plan: %d slots x %d planes x 4 x %d x %d modes = %lld output entries, at most "
                 "2^24 = %lld are held", n_slots, planes, nu, nv, out, MODES_OUT_MAX);
        return -1;
    }
    for (int axis = 0; axis < 2; ++axis) {
        const double *t = axis ? mode_y : mode_x;
        const int modes = axis ? nv : nu, n = axis ? my : mx;
        for (int a = 0; a < modes; ++a)
            for (int i = 0; i < n; ++i) {
                const double re = t[2 * ((size_t)a * n + i)], im = t[2 * ((size_t)a * n + i) + 1];
                if (!std::isfinite(re) || !std::isfinite(im)) {
                    snprintf(why, why_len, "ml_propagate_modes_plan: mode_%s[%d][%d] = (%.17g, %.17g): a table entry is finite",
                             axis ? "y" : "x", a, i, re, im);
                    return -1;
                }
            }
    }
    return 0;
}

// The argument checks of ml_propagate_modes_queue.  -> 0; -1: an argument error, -2: the state does not allow the call.
inline int modes_queue_check(const FocusState &s, const ModesState &m, int source, int slot, char *why, size_t why_len) {
    if (!s.have_result) {
        snprintf(why, why_len, "ml_propagate has not run on the active propagation plan");
        return -2;
    }
    if (!m.planned) {
        snprintf(why, why_len, "ml_propagate_modes_plan has not run on the active propagation plan");
        return -2;
    }
    if (source < 0) {
        snprintf(why, why_len, "ml_propagate_modes_queue: source %d: a member of the last pass (>= 0); the sums of "
                 "ml_propagate_accumulate carry no phase", source);
        return -1;
    }
    if (source >= s.result_sets) {
        snprintf(why, why_len, "ml_propagate_modes_queue: member %d asked for, the last pass propagated %d field sets", source,
                 s.result_sets);
        return -1;
    }
    if (slot < 0 || slot >= m.n_slots) {
        snprintf(why, why_len, "ml_propagate_modes_queue: slot %d, the plan reserved the slots 0 ... %d", slot, m.n_slots - 1);
        return -1;
    }
    return 0;
}

// The argument checks of ml_propagate_modes_fetch
inline int modes_fetch_check(const ModesState &m, int first_slot, int n_slots, const void *out, char *why, size_t why_len) {
    if (!m.planned) {
        snprintf(why, why_len, "ml_propagate_modes_plan has not run on the active propagation plan");
        return -2;
    }
    if (first_slot < 0 || n_slots < 1 || (long long)first_slot + n_slots > m.n_slots) {
        snprintf(why, why_len, "ml_propagate_modes_fetch: slots %d ... %lld asked for, the plan reserved the slots 0 ... %d",
                 first_slot, (long long)first_slot + n_slots - 1, m.n_slots - 1);
        return -1;
    }
    if (!out) {
        snprintf(why, why_len, "ml_propagate_modes_fetch: NULL argument (out NULL)");
        return -1;
    }
    return 0;
}

}  // namespace ml
