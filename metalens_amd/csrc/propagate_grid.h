// Plan arithmetic of the FFT form of the finite-distance propagator (propagate_grid.hip), on the host and free of
// HIP types (as transform_route.h): tools/propagate_grid.cpp and tests/test_propagate_grid_host.py run it without
// a GPU.
//
// For a tensor grid of targets (tx0 + i dxp, ty0 + j dyp, z) on the aperture's own pitch every factor of a
// (sample, target) pair of propagate.hip depends on the lag (i_t - i_s, j_t - j_s) alone: the pair sum is a discrete
// 2-D convolution of the four currents with eight kernels, computed here as a zero-padded circular convolution -
// the same sum in another order.
//
// Per axis, n samples and m targets: the lags l = i_t - i_s range over [-(n - 1), m - 1], n + m - 1 of them.
//   L = the smallest power of two >= max(16, n + m - 1); lag l is stored at index l mod L; index p holds lag
//   p (p < m) or p - L (otherwise) - indices in [m, L - n] are no lag of the problem.
//   L > 8192 is refused: one row of 8192 complex128 is 128 KiB of the 160 KiB LDS of a compute unit.  The long plan
//   (ml_propagate_plan_grid_long) takes L = 16384 too, an axis of that length in two passes (grid_axis_route below);
//   it stops there because the 18 planes of L = 32768 a side are 309 GB.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace ml {

constexpr int GRID_L_MIN = 16, GRID_L_MAX = 8192;
constexpr int GRID_L_LONG_MAX = 16384;   // the cap of the long plan
constexpr int GRID_KERNELS = 8;    // kernel spectra kept for the life of a plan
constexpr int GRID_CURRENTS = 4;   // Jx, Jy, Mx / Z, My / Z

// the smallest power of two >= max(16, n + m - 1); may exceed GRID_L_MAX (the caller refuses)
inline long long grid_padded_length(int n, int m) {
    long long need = (long long)n + m - 1, L = GRID_L_MIN;
    while (L < need) L *= 2;
    return L;
}

inline int grid_lag_index(int lag, int L) { return lag >= 0 ? lag : lag + L; }
inline int grid_index_lag(int p, int m, int L) { return p < m ? p : p - L; }

struct GridPlanFacts {
    int nx = 0, ny = 0, mx = 0, my = 0;   // aperture samples, targets
    int Lx = 0, Ly = 0;
    int outputs = 0;                      // 6 with H, 3 without
    int64_t plane_bytes = 0, workspace_bytes = 0;
};

// -> 0, or -1 with `why` filled: an axis whose padded length exceeds `cap` (GRID_L_MAX, or GRID_L_LONG_MAX for the
// long plan)
inline int grid_plan_facts(int nx, int ny, int mx, int my, int want_h, GridPlanFacts *f, char *why, size_t why_len,
                           int cap = GRID_L_MAX) {
    const long long Lx = grid_padded_length(nx, mx), Ly = grid_padded_length(ny, my);
    if (Lx > cap || Ly > cap) {
        const bool bad_x = Lx > cap;
        snprintf(why, why_len,
                 cap > GRID_L_MAX
                     ? "the FFT form pads the %s axis of n = %d samples and m = %d targets to L = %lld > %d (the planes "
                       "of a longer axis do not fit the card); use the direct method or fewer targets per plan"
                     : "the FFT form pads the %s axis of n = %d samples and m = %d targets to L = %lld > %d (one row of L "
                       "complex128 must fit the LDS); use the direct method or fewer targets per plan",
                 bad_x ? "x" : "y", bad_x ? nx : ny, bad_x ? mx : my, bad_x ? Lx : Ly, cap);
        return -1;
    }
    f->nx = nx;
    f->ny = ny;
    f->mx = mx;
    f->my = my;
    f->Lx = (int)Lx;
    f->Ly = (int)Ly;
    f->outputs = want_h ? 6 : 3;
    f->plane_bytes = (int64_t)Lx * Ly * 16;
    f->workspace_bytes = (int64_t)(GRID_KERNELS + GRID_CURRENTS + f->outputs) * f->plane_bytes;
    return 0;
}

// cos / sin of 2 pi j / L for j < L / 2, evaluated in long double and rounded once: [L / 2][2]
inline std::vector<double> grid_twiddles(int L) {
    std::vector<double> t((size_t)L);
    const long double two_pi = 8.0L * atanl(1.0L);
    for (int j = 0; j < L / 2; ++j) {
        const long double phi = two_pi * (long double)j / (long double)L;
        t[2 * (size_t)j] = (double)cosl(phi);
        t[2 * (size_t)j + 1] = (double)sinl(phi);
    }
    return t;
}

// How an axis of length L is transformed (propagate_grid.hip).  A transform is log2 L radix-2 stages, decimation in
// frequency forward (natural order in, bit-reversed out) and decimation in time back (bit-reversed in, natural out):
// the contraction is bin by bin, so no pass reorders.  The stage of block size B pairs the elements p and p + B / 2
// of every block of B.  Up to three stages run in registers between two exchanges (groups).
//   rows (contiguous):     all stages in the LDS, one row or several short ones per workgroup;
//   columns (stride Ly):   GRID_COLS adjacent columns per workgroup (128 contiguous bytes per access); blocks of up
//                          to GRID_COL_LDS elements in the LDS, and for longer axes the stages above that in one
//                          streaming pass without LDS (L / GRID_COL_LDS <= 8 elements per thread).
// An axis of the long plan with L > GRID_L_MAX:
//   rows:                  the stages above a block of GRID_ROW_BLOCK elements in one streaming pass without LDS
//                          (L / GRID_ROW_BLOCK elements of one row per thread, adjacent lanes adjacent elements), the rest
//                          on blocks of a row in the LDS;
//   columns:               as above, with L / GRID_COL_LDS = 16 elements per thread in the streaming pass.
constexpr int GRID_COLS = 8, GRID_COL_LDS = 1024;
constexpr int GRID_ROW_BLOCK = 4096;   // 68 KiB with its padding: two workgroups per compute unit

inline int grid_log2(int L) {
    int s = 0;
    while ((1 << s) < L) ++s;
    return s;
}
// LDS slot of element p: one slot of padding per 16 (stride-8 and stride-16 accesses of the late stages spread
// over the 16 slots of a bank row)
constexpr int grid_lds_slot(int p) { return p + (p >> 4); }
// slots of one sequence of `len` elements, odd so that adjacent sequences start on different slots
constexpr int grid_lds_seq(int len) { return grid_lds_slot(len) | 1; }


// The launches of one axis: `top_stages` stages (block sizes L ... 2 lds_len) in ONE streaming pass without LDS - none
// if 0 - and the stages of block size lds_len ... 2 in the LDS, sequences of lds_len elements.  Forward (decimation in
// frequency) the streaming pass runs first, back (decimation in time) last.
struct GridAxisRoute {
    int top_stages = 0;
    int lds_len = 0;
};

// `row_block`: the block of a row longer than GRID_L_MAX (GRID_ROW_BLOCK or GRID_L_MAX)
inline GridAxisRoute grid_axis_route(int L, bool columns, int row_block = GRID_ROW_BLOCK) {
    GridAxisRoute r;
    const int whole = columns ? GRID_COL_LDS : GRID_L_MAX;   // the longest axis that runs in the LDS alone
    r.lds_len = L <= whole ? L : columns ? GRID_COL_LDS : row_block;
    r.top_stages = grid_log2(L / r.lds_len);
    return r;
}

// "top,lds" / "lds,top" / "lds": the kernels of an axis in launch order
inline const char *grid_route_order(const GridAxisRoute &r, bool inverse) {
    return r.top_stages == 0 ? "lds" : inverse ? "lds,top" : "top,lds";
}

}  // namespace ml
