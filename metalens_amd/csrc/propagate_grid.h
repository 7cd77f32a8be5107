// Plan arithmetic of the FFT form of the finite-distance propagator (propagate_grid*.hip, propagate_stack.hip), on the host and free of
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

// The tiled plan (ml_propagate_plan_grid_tiled): overlap-add over tiles of the aperture.  The sum is linear in the
// samples, so per axis the n samples are cut into c = ceil(n / B) tiles of B = L - m + 1 samples, each convolved at
// the padded length L (a power of two in [GRID_L_MIN, GRID_L_MAX], >= m); the tiles' products are added in the
// spectral domain in front of ONE inverse transform.  Tile a holds the samples [a B, min(n, a B + B)) at the local
// indices 0 ... B - 1; index p of its kernel plane holds the true lag (p < m ? p : p - L) - a B.  The lags of a tile,
// local target minus local sample in [-(B - 1), m - 1], are exactly L of them: no index is wasted.
//   padded area per axis: c L instead of up to 2 n (8192 -> 64: 9 x 1024 = 9216 instead of 16384)
constexpr int GRID_TILE_BATCH_MAX = 64;                      // tiles per launch: 512 kernel planes
constexpr int64_t GRID_TILE_BATCH_BYTES = (int64_t)128 << 20;   // the four current planes of a batch's tiles stay below this

struct GridTileAxis {
    int L = 0, B = 0, c = 0;   // tile length, samples per tile, tiles
};

inline bool grid_tile_length_ok(long long L, int m) {
    return L >= GRID_L_MIN && L <= GRID_L_MAX && (L & (L - 1)) == 0 && L >= m;
}

inline GridTileAxis grid_tile_axis(int n, int m, int L) {
    GridTileAxis t;
    t.L = L;
    t.B = L - m + 1;
    t.c = (n + t.B - 1) / t.B;
    return t;
}

// What a padded sample of an axis costs at the tile length L, in 32nds of its cost at L <= 512: the square roots of the
// measured time per padded AREA of a cached pass - 1.08 : 1.37 : 1.88 : 2.14 e-7 ms per sample at L = 512 : 1024 : 2048 :
// 4096, the same within 8 % at 4096^2, 8192^2 and 16384^2 -> 64^2 and 4096^2 -> 256^2 (longer tiles
// take more stages, columns above 1024 a streaming pass, and fewer tiles of a batch stay in the memory-side cache).
// Nothing below 512 or at 8192 has been measured: flat below, the weight of 4096 at 8192.
constexpr int grid_tile_weight(int L) { return L <= 512 ? 32 : L == 1024 ? 36 : L == 2048 ? 42 : 45; }

// the admissible L that minimises the weighted padded length c L w(L) of the axis; ties go to the larger L (fewer
// tiles): where one tile of at most 512 holds the axis and shorter tiles would pad it no less, the plan has one tile of
// the L of the untiled plan.  m <= GRID_L_MAX.
inline int grid_tile_default(int n, int m) {
    int best = 0;
    long long best_cost = 0;
    for (int L = GRID_L_MIN; L <= GRID_L_MAX; L *= 2) {
        if (L < m) continue;
        const long long cost = (long long)grid_tile_axis(n, m, L).c * L * grid_tile_weight(L);
        if (!best || cost <= best_cost) {
            best = L;
            best_cost = cost;
        }
    }
    return best;
}

struct GridTilePlan {
    int nx = 0, ny = 0, mx = 0, my = 0;
    GridTileAxis x, y;
    int tiles = 0, batch = 0;             // cx cy; tiles per pass through the transform launchers
    int outputs = 0;                      // 6 with H, 3 without
    int64_t plane_bytes = 0, workspace_bytes = 0;
};

// what is wrong with the tile length L (0: the default) of an axis of n samples (0: not known yet) and m targets;
// -> 0, or -1 with `why` filled
inline int grid_tile_check_axis(const char *axis, int n, int m, int L, char *why, size_t why_len) {
    if (m > GRID_L_MAX) {
        snprintf(why, why_len,
                 "the tiled FFT form takes at most %d targets per axis (a tile is at least as long as the targets, one row "
                 "of L complex128 must fit the LDS): the %s axis of n = %d samples has m = %d targets; use the direct "
                 "method or fewer targets per plan",
                 GRID_L_MAX, axis, n, m);
        return -1;
    }
    if (L != 0 && !grid_tile_length_ok(L, m)) {
        snprintf(why, why_len,
                 "the tile length of the %s axis of n = %d samples and m = %d targets is L = %d: it must be a power of two "
                 "in [%d, %d] and at least m (0: the default)",
                 axis, n, m, L, GRID_L_MIN, GRID_L_MAX);
        return -1;
    }
    return 0;
}

// -> 0, or -1 with `why` filled.  tile_lx, tile_ly: 0 takes grid_tile_default.  batch_bytes: GRID_TILE_BATCH_BYTES.
//   batch G = min(cx cy, GRID_TILE_BATCH_MAX, max(1, batch_bytes / (4 plane_bytes)))
//   workspace: all tiles' kernel spectra (kept for the life of the plan), the currents of one batch, the outputs
inline int grid_tile_plan(int nx, int ny, int mx, int my, int want_h, int tile_lx, int tile_ly, int64_t batch_bytes,
                          GridTilePlan *t, char *why, size_t why_len) {
    if (grid_tile_check_axis("x", nx, mx, tile_lx, why, why_len) != 0) return -1;
    if (grid_tile_check_axis("y", ny, my, tile_ly, why, why_len) != 0) return -1;
    t->nx = nx;
    t->ny = ny;
    t->mx = mx;
    t->my = my;
    t->x = grid_tile_axis(nx, mx, tile_lx ? tile_lx : grid_tile_default(nx, mx));
    t->y = grid_tile_axis(ny, my, tile_ly ? tile_ly : grid_tile_default(ny, my));
    const int64_t tiles = (int64_t)t->x.c * t->y.c;
    if (tiles > (1 << 20)) {
        snprintf(why, why_len,
                 "the tiled FFT form cuts the aperture of %d x %d samples into %d x %d tiles of %d x %d samples (tile lengths "
                 "%d, %d for %d x %d targets): at most 2^20 tiles per plan; use longer tiles",
                 nx, ny, t->x.c, t->y.c, t->x.B, t->y.B, t->x.L, t->y.L, mx, my);
        return -1;
    }
    t->tiles = (int)tiles;
    t->outputs = want_h ? 6 : 3;
    t->plane_bytes = (int64_t)t->x.L * t->y.L * 16;
    const int64_t by_bytes = batch_bytes / (GRID_CURRENTS * t->plane_bytes);
    int64_t G = tiles < GRID_TILE_BATCH_MAX ? tiles : GRID_TILE_BATCH_MAX;
    if (G > (by_bytes > 1 ? by_bytes : 1)) G = by_bytes > 1 ? by_bytes : 1;
    t->batch = (int)G;
    t->workspace_bytes = ((int64_t)GRID_KERNELS * tiles + (int64_t)GRID_CURRENTS * G + t->outputs) * t->plane_bytes;
    return 0;
}

// The fine plan (ml_propagate_plan_grid_fine): a tensor grid of targets on the aperture's pitch divided by an integer s
// per axis.  Per axis, m fine targets t[i] = t[0] + i dxp / s: the targets a, a + s, a + 2 s, ... are lattice a, on the
// aperture's pitch with the origin t[a] - what a tiled plan with tx0 = t[a] would be given.  A = min(s, m) lattices hold a
// target, lattice a holds m_a = ceil((m - a) / s) of them; all are planned with the count m_c = ceil(m / s) = m_0 of
// lattice 0 and share ONE tiled plan of (nx, ny, m_cx, m_cy) - the targets of a ragged lattice beyond m_a are computed and
// dropped.  The currents of a field set are padded and transformed once, tile by tile, and kept; every lattice is a
// contraction of them with its own kernel spectra, an inverse transform and a scatter into the interleaved result.
//   cache_kernels: the kernel spectra of all Ax Ay lattices are kept for the life of the plan,
//                  (8 Ax Ay tiles + 4 tiles + 2 outputs) planes;
//   otherwise:     those of GRID_FINE_PAIR lattices and one batch of tiles are filled and transformed in every pass,
//                  (16 batch + 4 tiles + 2 outputs) planes.
constexpr int GRID_FINE_S_MAX = 8;
constexpr int GRID_FINE_PAIR = 2;   // lattices contracted per read of the currents

inline int grid_fine_count(int m, int s) { return (m + s - 1) / s; }                      // m_c
inline int grid_fine_active(int m, int s) { return s < m ? s : m; }                        // A
inline int grid_fine_lattice_count(int m, int s, int a) { return (m - a + s - 1) / s; }    // m_a, a < A

struct GridFinePlan {
    int sx = 0, sy = 0;       // the pitch ratios
    int ax = 0, ay = 0;       // active lattices per axis
    int mx = 0, my = 0;       // fine targets
    int m_cx = 0, m_cy = 0;   // targets per lattice as planned
    int cache_kernels = 1;
    GridTilePlan tile;        // of (nx, ny, m_cx, m_cy)
    int64_t workspace_bytes = 0;
};

// what is wrong with the ratio s, the m fine targets and the tile length L (0: the default) of an axis of n samples
// (0: not known yet); -> 0, or -1 with `why` filled
inline int grid_fine_check_axis(const char *axis, int n, int m, int s, int L, char *why, size_t why_len) {
    if (s < 1 || s > GRID_FINE_S_MAX) {
        snprintf(why, why_len,
                 "the fine FFT form divides the aperture's pitch by an integer s in [1, %d]: the %s axis of n = %d samples "
                 "and m = %d fine targets has s = %d",
                 GRID_FINE_S_MAX, axis, n, m, s);
        return -1;
    }
    const int m_c = grid_fine_count(m, s);
    if (m_c > GRID_L_MAX) {
        snprintf(why, why_len,
                 "the fine FFT form takes at most %d targets per lattice and axis (a tile is at least as long as a lattice's "
                 "targets, one row of L complex128 must fit the LDS): the %s axis of n = %d samples has m = %d fine targets at "
                 "s = %d, m_c = %d per lattice; use the direct method or fewer targets per plan",
                 GRID_L_MAX, axis, n, m, s, m_c);
        return -1;
    }
    if (L != 0 && !grid_tile_length_ok(L, m_c)) {
        snprintf(why, why_len,
                 "the tile length of the %s axis of n = %d samples and m_c = %d targets per lattice (m = %d fine targets at "
                 "s = %d) is L = %d: it must be a power of two in [%d, %d] and at least m_c (0: the default)",
                 axis, n, m_c, m, s, L, GRID_L_MIN, GRID_L_MAX);
        return -1;
    }
    return 0;
}

// -> 0, or -1 with `why` filled.  mx, my >= 1: the fine targets; the other arguments as grid_tile_plan's.
inline int grid_fine_plan(int nx, int ny, int mx, int my, int sx, int sy, int want_h, int tile_lx, int tile_ly, int cache_kernels,
                          int64_t batch_bytes, GridFinePlan *p, char *why, size_t why_len) {
    if (grid_fine_check_axis("x", nx, mx, sx, tile_lx, why, why_len) != 0) return -1;
    if (grid_fine_check_axis("y", ny, my, sy, tile_ly, why, why_len) != 0) return -1;
    if ((long long)mx * my > (1 << 26)) {
        snprintf(why, why_len, "%lld fine targets (%d x %d): at most 2^26 per plan", (long long)mx * my, mx, my);
        return -1;
    }
    p->sx = sx;
    p->sy = sy;
    p->ax = grid_fine_active(mx, sx);
    p->ay = grid_fine_active(my, sy);
    p->mx = mx;
    p->my = my;
    p->m_cx = grid_fine_count(mx, sx);
    p->m_cy = grid_fine_count(my, sy);
    p->cache_kernels = cache_kernels != 0;
    if (grid_tile_plan(nx, ny, p->m_cx, p->m_cy, want_h, tile_lx, tile_ly, batch_bytes, &p->tile, why, why_len) != 0) return -1;
    const GridTilePlan &t = p->tile;
    const int64_t kernels = p->cache_kernels ? (int64_t)GRID_KERNELS * p->ax * p->ay * t.tiles
                                             : (int64_t)GRID_KERNELS * GRID_FINE_PAIR * t.batch;
    p->workspace_bytes = (kernels + (int64_t)GRID_CURRENTS * t.tiles + GRID_FINE_PAIR * t.outputs) * t.plane_bytes;
    return 0;
}

// The stack plan (ml_propagate_plan_grid_stack): the fine targets in nz planes z[0 ... nz - 1], any order, equal values
// allowed.  The fine plan of (nx, ny, mx, my, sx, sy, tile_lx, tile_ly) does not depend on z: a stack has ONE, and the
// currents of a field set are padded and transformed once for all planes.  A LAYER is (plane p, lattice (a, b)), numbered
//   l = p A + a Ay + b,  A = Ax Ay,
// with its own eight kernel spectra - those of the fine plan's lattice (a, b) planned at z[p].  The layers are contracted
// GRID_FINE_PAIR at a time in that order (a pair may straddle two planes), a single one last if nz A is odd.  The result
// is plane-major: target t = (p mx + i) my + j, T = nz mx my <= 2^26.
//   cache_kernels: the kernel spectra of all nz A layers are kept for the life of the plan,
//                  (8 nz A tiles + 4 tiles + 2 outputs) planes;
//   otherwise:     the streamed workspace of the fine plan, (16 batch + 4 tiles + 2 outputs) planes, whatever nz is.
constexpr int GRID_STACK_PLANES_MAX = 4096;
// The fill kernel takes the kernels of up to GRID_FINE_PAIR layers x GRID_TILE_BATCH_MAX tiles per launch.  What a launch
// writes is read next by the row pass: all layers of a contraction go into one launch while their planes fit the 256 MiB
// memory-side cache, else one launch and its transforms per layer.  Measured on an MI355X, 8 planes of 64^2 fine targets at
// half the pitch behind 4096^2, streamed (a batch of 8 tiles of 512^2: 256 MiB per layer): a launch per layer 111.6 ms,
// the pair's 512 MiB in one launch 129.3 ms, the loop of eight 'fft-fine' plans 124.2 ms.
constexpr int64_t GRID_STACK_FILL_BYTES = (int64_t)256 << 20;
inline int grid_stack_fill_layers(int layers, int tiles, int64_t plane_bytes) {
    return (int64_t)layers * tiles * GRID_KERNELS * plane_bytes <= GRID_STACK_FILL_BYTES ? layers : 1;
}

struct GridStackPlan {
    int nz = 0;
    int layers = 0;           // nz Ax Ay
    GridFinePlan fine;        // of one plane
    int64_t workspace_bytes = 0;
};

struct GridStackLayer {
    int p = 0, a = 0, b = 0;   // plane, lattice
};

inline GridStackLayer grid_stack_layer(int l, int ax, int ay) {
    GridStackLayer s;
    const int A = ax * ay, r = l % A;
    s.p = l / A;
    s.a = r / ay;
    s.b = r % ay;
    return s;
}

// what is wrong with the planes of a stack of mx x my fine targets, whatever the aperture; -> 0, or -1 with `why` filled
inline int grid_stack_check_planes(const double *z, int nz, int mx, int my, char *why, size_t why_len) {
    if (nz < 1 || nz > GRID_STACK_PLANES_MAX) {
        snprintf(why, why_len, "a stack has 1 to %d planes, got nz = %d", GRID_STACK_PLANES_MAX, nz);
        return -1;
    }
    for (int p = 0; p < nz; ++p)
        if (!(std::isfinite(z[p]) && z[p] > 0)) {
            snprintf(why, why_len, "plane %d of the stack lies at z[%d] = %g: the propagator needs a finite z > 0", p, p, z[p]);
            return -1;
        }
    if ((long long)nz * mx * my > (1 << 26)) {
        snprintf(why, why_len, "%lld targets (%d planes of %d x %d fine targets): at most 2^26 per plan", (long long)nz * mx * my, nz,
                 mx, my);
        return -1;
    }
    return 0;
}

// -> 0, or -1 with `why` filled.  z[0 ... nz - 1]: the planes; the other arguments as grid_fine_plan's, whose refusals
// apply unchanged.
inline int grid_stack_plan(int nx, int ny, int mx, int my, int sx, int sy, int want_h, int tile_lx, int tile_ly, int cache_kernels,
                           int64_t batch_bytes, const double *z, int nz, GridStackPlan *s, char *why, size_t why_len) {
    if (nz < 1 || nz > GRID_STACK_PLANES_MAX) return grid_stack_check_planes(z, nz, mx, my, why, why_len);
    if (grid_fine_plan(nx, ny, mx, my, sx, sy, want_h, tile_lx, tile_ly, cache_kernels, batch_bytes, &s->fine, why, why_len) != 0)
        return -1;
    if (grid_stack_check_planes(z, nz, mx, my, why, why_len) != 0) return -1;
    const GridFinePlan &f = s->fine;
    const GridTilePlan &t = f.tile;
    s->nz = nz;
    s->layers = nz * f.ax * f.ay;
    const int64_t kernels = f.cache_kernels ? (int64_t)GRID_KERNELS * s->layers * t.tiles
                                            : (int64_t)GRID_KERNELS * GRID_FINE_PAIR * t.batch;
    s->workspace_bytes = (kernels + (int64_t)GRID_CURRENTS * t.tiles + GRID_FINE_PAIR * t.outputs) * t.plane_bytes;
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

// How an axis of length L is transformed (propagate_grid_fft.hip).  A transform is log2 L radix-2 stages, decimation in
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
