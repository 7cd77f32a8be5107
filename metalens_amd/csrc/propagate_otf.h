// The transfer function of a propagated image (propagate_otf.hip, ml_propagate_otf): what host and device share - the
// phase arithmetic of the Fourier phasors, the order of the sums, the argument checks and the caps - free of HIP types
// (as propagate_focus.h): tools/propagate_otf_plan.cpp and tests/test_propagate_otf_host.py run it without a GPU.
//
//   O_w[p][a][b] = sum_i sum_j w(p, i, j) exp(-2 pi i (u[a] i + v[b] j)),   u, v in cycles per target sample, |u|, |v| <= 1/2
//
// The phase.  u i reaches 2^24 cycles, so its rounding must not reach the phase: otf_phase_fraction(u, i) takes the
// rounding error of the product by an FMA (exact), subtracts the nearest integer (exact) and adds the two, so that the
// fraction of u i in [-1/2, 1/2] is known within 2^-54 whatever i.  The quarter turns come off the fraction before it
// meets pi: otf_phase_quarters(f) = q with f = q / 4 + rest exactly, |rest| <= 1/8, and the phasor is sincos_cw_q(OTF_TWO_PI
// rest, q).  Each component is within 16 u (u = 2^-53) of cos / sin(2 pi frac(u i)) - 1 u for the fraction, 7 u for the
// rounded 2 pi and its product, 4 u for sincos_cw_q (2^-51, nearfield_math.h) -, and at a fraction of 0, +-1/4, +-1/2 it is
// exactly 0 or +-1: the imaginary part of an entry at 0 and Nyquist frequencies, a sum of exact zeros, is 0 and not the
// sin(fl(pi)) = 1.2e-16 per term whose sign a tie of the rounding would decide.
//
// The order.  The contraction is separable: a row pass R_w(i, b) = sum_j w(i, j) Ty(j, b) and a column pass O_w(a, b) =
// sum_i Tx(i, a) R_w(i, b), with Tx(i, a) = exp(-2 pi i u[a] i), Ty(j, b) = exp(-2 pi i v[b] j).  Both sums run over
// SEGMENTS of OTF_SEGMENT = 32 consecutive indices: a segment's terms are added one after another from 0, in ascending
// index, and the segments' sums are added one after another from 0, in ascending index.  Every product and every sum is
// rounded on its own.  The order depends on (mx, my) alone - not on the planes, the plane, the member, the source, nu,
// nv or the other frequencies -, so an entry is repeatable bit for bit, plane p of a stack has the bits of that plane
// planned alone, and an entry of a call of 64 x 64 frequencies has the bits of the same (u, v) asked for alone.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "propagate_focus.h"

#if defined(__HIPCC__)
#define ML_OTF_HD __host__ __device__
#else
#define ML_OTF_HD
#endif

namespace ml {

constexpr int OTF_FREQ_MAX = 64;                  // frequencies per axis and call (ML_OTF_FREQ_MAX)
constexpr int OTF_SEGMENT = 32;                   // indices whose terms are added one after another
constexpr long long OTF_TABLE_MAX = 1LL << 24;    // mx nu + my nv phasors at the most
constexpr long long OTF_ROWS_MAX = 1LL << 26;     // planes mx nv entries of R per weight at the most (2 GiB for both)
constexpr int OTF_PLANES_MAX = 65535;             // planes per call: a dimension of the launch grids
constexpr double OTF_TWO_PI = 6.283185307179586;

// the fraction of u i in [-1/2, 1/2], within 2^-54: i an integer >= 0 held in a double
ML_OTF_HD inline double otf_phase_fraction(double u, double i) {
    const double t = u * i;
    const double e = fma(u, i, -t);   // the product's rounding error, exact
    return (t - rint(t)) + e;         // the difference is exact
}

// the quarter turns of a fraction f in [-1/2, 1/2]: -> q in -2 ... 2 with f = q / 4 + rest exactly, |rest| <= 1/8
ML_OTF_HD inline int otf_phase_quarters(double f, double &rest) {
    const double q = rint(4.0 * f);
    rest = f - 0.25 * q;   // exact: both products are, and the difference of neighbours is
    return (int)q;
}

// what a plain product would give: kept for tests, which show what the FMA buys
ML_OTF_HD inline double otf_phase_fraction_naive(double u, double i) {
    const double t = u * i;
    return t - rint(t);
}

ML_OTF_HD inline int otf_segments(int n) { return (n + OTF_SEGMENT - 1) / OTF_SEGMENT; }

// The launch shapes of the two passes (the kernels and launchers of propagate_otf.hip call these; tools/
// propagate_otf_plan.cpp prints them).  The row pass takes a row in tiles of OTF_TILE targets whose weights lie in the
// LDS at once - or, above OTF_FEW frequencies nv, OTF_ROWS_MANY rows in tiles of OTF_TILE / OTF_ROWS_MANY of each -, the
// column pass takes the rows in tiles of OTF_TILE.  A tile is whole segments but for the last one of an axis, so the
// tiles cut no segment and change no order.
constexpr int OTF_TILE = 1024;                    // targets whose weights lie in the LDS at once
constexpr int OTF_FEW = 8, OTF_ROWS_MANY = 4;     // above OTF_FEW frequencies nv a workgroup takes 4 rows
constexpr int OTF_BATCH = 16;                     // frequencies whose segment sums lie in the LDS at once (four rows: 32)
static_assert(OTF_TILE % (OTF_ROWS_MANY * OTF_SEGMENT) == 0, "whole segments per tile in either row kernel");

ML_OTF_HD inline int otf_rows_per_group(int nv) { return nv <= OTF_FEW ? 1 : OTF_ROWS_MANY; }

// tiles of `tile` indices that hold n, and the indices of tile t of them
ML_OTF_HD inline int otf_tiles(int n, int tile) { return (n + tile - 1) / tile; }

ML_OTF_HD inline int otf_tile_len(int n, int tile, int t) {
    const int left = n - t * tile;
    return left < tile ? left : tile;
}

// the live rows of workgroup g of the row pass (rows behind the plane's last are zeros, never written out)
ML_OTF_HD inline int otf_live_rows(int mx, int rows, int g) { return otf_tile_len(mx, rows, g); }

struct OtfRowsShape {
    int rows;            // rows of a plane per workgroup: 1 or OTF_ROWS_MANY
    int tile;            // targets of each row per tile
    int tiles;           // tiles per row
    int batch;           // frequencies per batch
    int last_segments;   // segments of the last tile
    int last_segment;    // indices of its last segment
    int groups;          // workgroups along x
    int last_rows;       // live rows of the last of them
};

inline OtfRowsShape otf_rows_shape(int mx, int my, int nv) {
    OtfRowsShape s;
    s.rows = otf_rows_per_group(nv);
    s.tile = OTF_TILE / s.rows;
    s.tiles = otf_tiles(my, s.tile);
    s.batch = s.rows == 1 ? OTF_BATCH : 2 * OTF_BATCH;
    const int last = otf_tile_len(my, s.tile, s.tiles - 1);
    s.last_segments = otf_segments(last);
    s.last_segment = last - (s.last_segments - 1) * OTF_SEGMENT;
    s.groups = otf_tiles(mx, s.rows);
    s.last_rows = otf_live_rows(mx, s.rows, s.groups - 1);
    return s;
}

struct OtfColumnsShape {
    int tiles;           // tiles of OTF_TILE rows
    int last_segments;   // segments of the last tile
    int last_segment;    // indices of its last segment
};

inline OtfColumnsShape otf_columns_shape(int mx) {
    OtfColumnsShape s;
    s.tiles = otf_tiles(mx, OTF_TILE);
    const int last = otf_tile_len(mx, OTF_TILE, s.tiles - 1);
    s.last_segments = otf_segments(last);
    s.last_segment = last - (s.last_segments - 1) * OTF_SEGMENT;
    return s;
}

// The argument checks of ml_propagate_otf.  -> 0; -1: an argument error, -2: the state does not allow the call; `why` is
// filled then.  source >= 0: member of the last pass, -1: the sums.
inline int otf_check(const FocusState &s, int source, int mx, int my, int planes, const double *u, int nu, const double *v,
                     int nv, const void *otf, char *why, size_t why_len) {
    if (!s.have_result) {
        snprintf(why, why_len, "ml_propagate has not run on the active propagation plan");
        return -2;
    }
    if (source < -1) {
        snprintf(why, why_len, "ml_propagate_otf: source %d: a member of the last pass (>= 0) or -1 for the sums", source);
        return -1;
    }
    if (source == -1 && !s.have_sums) {
        snprintf(why, why_len, "ml_propagate_accumulate has not run on the active propagation plan");
        return -2;
    }
    if (source >= s.result_sets) {
        snprintf(why, why_len, "ml_propagate_otf: member %d asked for, the last pass propagated %d field sets", source,
                 s.result_sets);
        return -1;
    }
    if (mx < 1 || my < 1 || planes < 1 || (long long)mx * my * planes != s.T) {
        snprintf(why, why_len, "ml_propagate_otf: %d planes of %d x %d targets are %lld targets, the active propagation plan "
                 "has %d", planes, mx, my, (long long)mx * my * planes, s.T);
        return -1;
    }
    if (planes > OTF_PLANES_MAX) {
        snprintf(why, why_len, "ml_propagate_otf: %d planes, at most %d are taken per call", planes, OTF_PLANES_MAX);
        return -1;
    }
    if (nu < 1 || nu > OTF_FREQ_MAX || nv < 1 || nv > OTF_FREQ_MAX) {
        snprintf(why, why_len, "ml_propagate_otf: %d x %d frequencies: 1 to %d are taken per axis", nu, nv, OTF_FREQ_MAX);
        return -1;
    }
    if (!u || !v || !otf) {
        snprintf(why, why_len, "ml_propagate_otf: NULL argument (u %s, v %s, otf %s)", u ? "given" : "NULL", v ? "given" : "NULL",
                 otf ? "given" : "NULL");
        return -1;
    }
    for (int axis = 0; axis < 2; ++axis) {
        const double *f = axis ? v : u;
        for (int a = 0; a < (axis ? nv : nu); ++a)
            if (!std::isfinite(f[a]) || !(std::fabs(f[a]) <= 0.5)) {
                snprintf(why, why_len, "ml_propagate_otf: %s[%d] = %.17g: a frequency is finite and within +-0.5 cycles per "
                         "target sample (Nyquist)", axis ? "v" : "u", a, f[a]);
                return -1;
            }
    }
    const long long table = (long long)mx * nu + (long long)my * nv;
    if (table > OTF_TABLE_MAX) {
        snprintf(why, why_len, "ml_propagate_otf: %d x %d + %d x %d = %lld phasors, at most 2^24 = %lld are tabulated per call",
                 mx, nu, my, nv, table, OTF_TABLE_MAX);
        return -1;
    }
    const long long rows = (long long)planes * mx * nv;
    if (rows > OTF_ROWS_MAX) {
        snprintf(why, why_len, "ml_propagate_otf: %d planes x %d rows x %d frequencies = %lld row sums per weight, at most 2^26 = "
                 "%lld are held", planes, mx, nv, rows, OTF_ROWS_MAX);
        return -1;
    }
    return 0;
}

}  // namespace ml
