// Which way a far-field transform call goes (farfield.hip transform_impl): the kind of each stage, the layout of
// stage 1's result G, the allocator that backs it and the rows both stages work on - decided here, as a value, from
// plain facts; farfield.hip's stage functions consume it.
//
// Host code without HIP types: compiled by hipcc into the library (common.h) and by the host compiler into
// tools/transform_route.cpp, which prints the route of given plan facts (tests/test_transform_route.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <float.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "metalens_hip.h"
#include "zfft_core.h"

#ifndef ML_STAGE1_TRANSPOSED
#define ML_STAGE1_TRANSPOSED 1   // 0: stage 1's result stays row-major whatever the aperture
#endif

namespace ml {

// The facts of one FFT axis of a plan (common.h ZfftAxis adds the axis' device tables).
struct ZfftAxisGeo {
    bool ok = false;
    int N_eff = 0, j0 = 0, pad1 = 0, pad2 = 0;
    int jstep = 1;   // output j is bin (j + j0) jstep of the N_eff-sample lattice (zfft_core.h Geo::jstep)
    // split > 1 (lattices beyond 8192 samples): `split` launches over interleaved sub-sequences of
    // N_eff / split samples; wk / kbin then belong to the SHORT lattice and pj holds [split][M]
    int split = 1;
    // passes > 1: ONE launch per row set, the residues of a row in that many groups through half
    // (a quarter) of the LDS (zfft_pass_kernel); lattices of 8192 < N_eff <= 16384 samples with at
    // most 1024 wanted bins run this way instead of split in two
    int passes = 0;
    // method 'fft-mixed' on a lattice that is not a multiple of 256 long: N_eff = A B R samples (the lattice itself
    // or the twice finer one: jstep = 1 or 2) through zfft_mixed_kernel<A, B>; pad1 is its one padding and tw its
    // [B][A] twiddle table (zfft_core.h mixed_choose).  A = 0: the 256 R3 scheme
    int A = 0, B = 0, R = 0;
};

// the facts of a FarfieldPlan (common.h adds its tables and buffers).  Set in farfield_plan.hip: method and the sizes by
// ml_farfield_plan, fold / fold_S and fold2 / fold2_S by plan_fold_axis from fold_split (ZfftAxisGeo: plan_fft_axis)
struct PlanFacts {
    int method = 0;    // ml_farfield_set_method value the plan was made under
    int nx_total = 0, ny = 0, mx = 0, my = 0, pair_list = 0;
    // the directions of the plan: mx x my of a tensor grid, direction (i, j) at i my + j; mx of a pair list (one column)
    int out_my() const { return pair_list ? 1 : my; }
    size_t directions() const { return (size_t)mx * out_my(); }
    // centre-symmetric uy / ux: the folded (even/odd) GEMM exists for stage 1 / stage 2, over S half-directions
    bool fold = false, fold2 = false;
    int fold_S = 0, fold2_S = 0;
};

enum class ShardKind { block, mirrored, interleaved };

// the resident rows of a call: rows [row0, row0 + nx), mirrored pairs from row0, or interleaved blocks
struct Shard {
    ShardKind kind = ShardKind::block;
    int row0 = 0;
    int block = 0, n_ranks = 1, rank = 0;   // interleaved
};

// The tuning and ablation knobs of the route, by the names diag_int() reads them under in a diagnostic build
// (common.h); the product library runs on these defaults.
struct RouteKnobs {
    int stage1_split = 0;       // ML_STAGE1_SPLIT > 0: the folded stage 1's split, whatever the tile count
    int g_skew = 8;             // ML_G_SKEW: the transposed G's pitch is the resident rows + this many elements
    int g_tiled = 1;            // ML_G_TILED=0: the plain transposed G where the tiled one would be taken
    long fold2_min_tiles = 32;  // ML_FOLD2_MIN_TILES: the folded stage 2 from this many tiles on
    int no_row_trim = 0;        // ML_NO_ROW_TRIM=1: both FFT stages on every resident row
    int no_gt_direct = 0;       // ML_NO_GT_DIRECT=1: folded + folded through the transposer
};

// layout of stage 1's result G for stage 2: row-major G[f][n1][b], transposed G[f][b][n1], or tiled G[f][b / 8][n1][b % 8]
enum class GLayout { row_major, transposed, tiled };

// Where "row (f, n1), bin b" of G lies, for stage 1's writer and stage 2's reader alike: element
// off + f s_f + (n1 - trim_lo) s_row + b s_bin for the row-major and the transposed G; in the tiled one bin b is
// element b % 8 of tile b / 8, s_bin the stride of the tiles.  off is where row trim_lo begins: stage 1 writes rows
// [trim_lo, trim_hi) only and stage 2 reads those.  Stage 1 takes (s_f, s_row, s_bin) as its output strides, stage 2
// walks the same array by columns: its rows are G's bins (tiles), its elements G's rows.
struct GView {
    int64_t off, s_f, s_row, s_bin;
    int cols;   // columns (tiles) per field plane: the rows of stage 2
};

inline GView g_view(GLayout layout, int nxl, int my, int64_t g_ld, int trim_lo) {
    GView v;
    v.s_f = layout == GLayout::row_major ? (int64_t)nxl * my : (int64_t)my * g_ld;
    v.s_row = layout == GLayout::row_major ? my : layout == GLayout::transposed ? 1 : 8;
    v.s_bin = layout == GLayout::row_major ? 1 : layout == GLayout::transposed ? g_ld : 8 * g_ld;
    v.cols = layout == GLayout::tiled ? my / 8 : my;
    v.off = (int64_t)trim_lo * v.s_row;
    return v;
}

enum class Stage1Kind { fft, folded, generic };
enum class Stage2Kind { interleaved, fft, fft_tiles, folded, generic_mirrored, generic, coldot };

struct TransformRoute {
    Stage1Kind stage1;
    // the folded stage 1's wanted split (the slabs it writes: zfold_splits of it, applied by the caller)
    int want_split1;
    GLayout g_layout;
    bool g_transposed() const { return g_layout != GLayout::row_major; }
    int64_t g_ld;          // pitch of the transposed / tiled G in elements
    size_t g_bytes;        // of G; per split-K slab of a folded stage 1
    bool pieces_wanted;    // G in 4 MB physical pieces (common.h PieceBuf) if they can be had, else hipMalloc
    int trim_lo, trim_hi;  // resident rows both FFT stages work on
    bool gt_direct;        // folded + folded: stage 1 writes its result transposed and modulated for stage 2
    Stage2Kind stage2;
};

// nxl: resident rows.  trim_rows: the resident rows that meet the lens circle, [trim_rows[0], trim_rows[1]), where
// the fields carry a row_first (have_row_first: synthesised fields on the grid the rows were found for).
inline TransformRoute transform_route(const PlanFacts &pl, const ZfftAxisGeo &fft_y, const ZfftAxisGeo &fft_x,
                                      const Shard &sh, int nxl, bool have_row_first, const int trim_rows[2],
                                      const RouteKnobs &knobs = RouteKnobs()) {
    TransformRoute rt;
    const int ny = pl.ny, mx = pl.mx, my = pl.my;
    const bool mirrored = sh.kind == ShardKind::mirrored, interleaved = sh.kind == ShardKind::interleaved;
    const bool fft1 = fft_y.ok, fft2 = fft_x.ok && !pl.pair_list;
    rt.stage1 = fft1 ? Stage1Kind::fft : pl.fold ? Stage1Kind::folded : Stage1Kind::generic;
    // few resident rows (multi-GPU shards) and a long reduction: split the pairs of stage 1 over
    // several workgroups per tile; the slabs are summed by the next kernel
    rt.want_split1 = 1;
    if (pl.fold) {
        // Measured (tools/zfold_shape_sweep.py): tiles of 128 half-directions read the aperture
        // fewer times and win when at most a 2-way split fills the chip; otherwise 64-wide
        // tiles with as many splits as it takes to reach ~2.5 workgroups per CU.
        const long t128 = (long)((4 * nxl + 31) / 32) * ((pl.fold_S + 127) / 128);
        const long t64 = (long)((4 * nxl + 31) / 32) * ((pl.fold_S + 63) / 64);
        if (t128 >= 480)
            rt.want_split1 = 1;
        else if (2 * t128 >= 480)
            rt.want_split1 = 2;
        else
            rt.want_split1 = (int)std::min<long>(8, std::max<long>(1, (640 + t64 - 1) / std::max<long>(t64, 1)));
        if (knobs.stage1_split > 0) rt.want_split1 = knobs.stage1_split;
    }
    // Both axes one-level FFTs on a large aperture: stage 1 writes its result TRANSPOSED, G[f][b][n1]
    // with rows of nxl + 8 (a 128-byte skew: consecutive bins of a row transform land in different
    // L2 channels), and stage 2 streams contiguous rows with non-temporal loads like stage 1 does,
    // instead of gathering 16-byte pieces 8 KB apart with loads that keep G in the caches.  What this
    // buys is mostly NOT in the transform (4096^2 -> 512^2: stage 1 0.179 -> 0.207 ms for its 16-byte
    // scattered stores - neighbouring rows meet in the XCD's L2 -, stage 2 0.057 -> 0.037) but in the
    // NEXT synthesis, 0.265 -> 0.229 ms: a G that is read once and dropped no longer pushes the
    // geometry records (134 MB at 4096^2, + 134 MB of G > the 256 MB memory-side cache) out between
    // steps.  Small apertures, where everything fits anyway, keep the row-major G (2048^2 -> 256^2,
    // 67 MB of records + G: 0.167 against 0.178 ms per step; from 2560^2 -> 320^2, 105 MB, on the
    // transposed one is 1-1.5 % ahead: 0.282 against 0.287 ms, 3072^2 0.368 / 0.372, 3584^2 0.458 / 0.463).
    const bool transposed = ML_STAGE1_TRANSPOSED && fft_y.ok && fft_x.ok && !pl.pair_list &&
                            fft_y.split == 1 && fft_x.split == 1 && !interleaved &&
                            (pl.method == ML_METHOD_FFT_STREAMED || pl.method == ML_METHOD_FFT_MIXED ||
                             (size_t)nxl * ny * 8 + (size_t)4 * nxl * my * 16 > (size_t)96 << 20);
    // (skew sweep at 4096^2 -> 512^2, stage 1: 0 elements 0.220 ms, 16 0.222, 1 0.204, 2 0.212, 24 0.208,
    // 72 0.206, 4 0.190, 8 0.194-0.196, 40 0.196, 136 0.192: anything but a multiple of 256 bytes)
    rt.g_ld = nxl + knobs.g_skew;
    // Where both transforms take the one-level kernels, the transposed G is stored TILED instead: G[f][b / 8][n1][b % 8],
    // the 8 bins of a 128-byte line side by side, tiles 8 g_ld elements long (zfft_core.h tile_off) - the same bytes.
    // Stage 1 then stores whole lines (8 lanes = one line, a 64-lane store 8 lines in 8 tiles, 8 x 65 KB apart, instead
    // of 64 16-byte pieces one pitch apart), and stage 2 (zfft.hip zfft_tiles_kernel) reads whole lines once, the 8
    // columns of a tile together.  (Measured at 4096^2 -> 512^2: DESIGN.md 4.2.)
    const int r3y = fft_y.N_eff / 256;
    rt.g_layout = !transposed ? GLayout::row_major
                  : (knobs.g_tiled != 0 && my % 8 == 0 && mx <= zf::TL_NT && r3y >= 3 && r3y <= 16 &&
                     fft_y.passes <= 1 && fft_x.passes <= 1 && !fft_y.A && !fft_x.A)
                      ? GLayout::tiled
                      : GLayout::transposed;
    // The TRANSPOSED result of rows up to 8192 samples lies in physical pieces of 4 MB, each an allocation of its own,
    // mapped side by side (common.h PieceBuf).  Stage 1 stores it in 16-byte pieces one pitch (65 KB at 4096 samples)
    // apart, and how fast those go is decided by the physical layout behind the buffer: 0.33 ms over one physically
    // contiguous allocation (whatever the pitch), 0.5-1.3 ms in pieces below the 2 MB translation fragment, 0.178-0.190
    // in pieces of 2 to 8 MB in three processes of four (8192 samples, pitch 131 KB: 0.75 in 2 MB pieces, 0.70 in 4 MB,
    // 0.72 in 8 MB) - and 0.183 or 0.200, one of two each, from hipMalloc, whose layout is whatever the driver's free
    // lists hold: the two 'modes' of rounds 4-6 (profiles/r06_ab_runs.txt).  The two-pass kernel of
    // longer rows (one 152 KB workgroup per CU, whole lines stored) is the other way round: 16384^2 -> 1024^2 stage 1
    // 4.01-4.16 ms over hipMalloc, 4.95 in 4 MB pieces, 4.32 in 8, 4.45 in 16, 4.13 in 32, 4.03 in 64 - it keeps
    // hipMalloc, as does every other layout.  A context that runs both kinds holds both buffers.
    // (METALENS_HIP_PIECES=0 in the environment: plain hipMalloc - the way out should a driver's virtual-memory API
    // misbehave; so is a PieceBuf that has failed once: it is not tried again.  Both are the allocation's business:
    // farfield.hip reserve_g)
    rt.g_bytes = transposed ? (size_t)4 * my * rt.g_ld * 2 * sizeof(double)
                            : (size_t)4 * nxl * my * 2 * sizeof(double);
    rt.pieces_wanted = transposed && nxl <= 8192;
    // Rows of a synthesised field that lie wholly outside the lens circle are zeros, and so are their row transforms:
    // both FFT stages run on the resident rows [trim_lo, trim_hi) only (7 % fewer of each in a window of the size
    // good_fft_number hands out, nearfield.py:30-36, 95-97).  Stage 1 neither reads those rows nor writes their part
    // of G; stage 2 takes them as rows the rank does not hold (FftArgs::a0 / h0: read as zero without a load; the short
    // transforms of an interleaved shard likewise, by LOCAL row).
    // Which rows: the kernels' own inside-the-lens test at the sample nearest y = 0 (row_extent_kernel), on the host's
    // copies of the axes (farfield.hip trim_rows_of).
    rt.trim_lo = 0;
    rt.trim_hi = nxl;
    if (fft1 && fft2 && !mirrored && have_row_first && !knobs.no_row_trim) {
        rt.trim_lo = trim_rows[0];
        rt.trim_hi = trim_rows[1];
    }
    // the folded stage 2 pays once its grid (32-row x 64-half-direction tiles over the 4*my
    // transposed rows) fills the chip; below that the generic GEMM with 32 x 32 tiles is faster
    const bool whole = (sh.row0 == 0 && nxl == pl.nx_total);
    const bool fold2_pays = (long)((4 * my + 31) / 32) * ((pl.fold2_S + 63) / 64) >= knobs.fold2_min_tiles;
    const bool use_fold2 = !fft2 && !pl.pair_list && pl.fold2 && fold2_pays && (mirrored || whole) && !interleaved;
    // both stages folded: stage 1 writes its result already transposed for stage 2
    rt.gt_direct = pl.fold && use_fold2 && !knobs.no_gt_direct;
    rt.stage2 = interleaved                            ? Stage2Kind::interleaved
                : fft2 && rt.g_layout == GLayout::tiled ? Stage2Kind::fft_tiles
                : fft2                                 ? Stage2Kind::fft
                : use_fold2                            ? Stage2Kind::folded
                : pl.pair_list                         ? Stage2Kind::coldot
                : mirrored                             ? Stage2Kind::generic_mirrored
                                                       : Stage2Kind::generic;
    return rt;
}

// ---- The launch shapes of the GEMM-path stage kernels: which tile and how many split-K slabs a stage takes for its
// sizes, as the launchers apply them (zfold.hip zfold_stage1, farfield_plan.hip stage2_tables, zgemm.hip pick_tile; the
// reasons and measurements stand there).  Pure arithmetic, so that tools/transform_route.cpp can name the kernel of
// each stage (tests/gemm_cases.py).  The forcing knobs of a diagnostic build (ML_ZFOLD_TILE, ML_STAGE2_SPLIT,
// ML_ZGEMM_TILE) stay with the launchers.

// pairs per split-K slab of zfold_kernel: a multiple of 64, so that every K tile and re-seed point stays aligned
inline int zfold_t_chunk(int T, int ksplit) {
    ksplit = ksplit < 1 ? 1 : ksplit;
    return ((T + ksplit - 1) / ksplit + 63) / 64 * 64;
}

// the slabs zfold_kernel writes for a wanted split of ksplit over T pairs
inline int zfold_eff_splits(int T, int ksplit) {
    const int chunk = zfold_t_chunk(T, ksplit);
    return (T + chunk - 1) / chunk;
}

// 32 x 128 tiles of 8 waves once tiles x slabs give ~2 workgroups per CU, else 32 x 64 tiles
inline bool zfold_take_wide(int M, int S, int splits) {
    return (long)((M + 31) / 32) * ((S + 127) / 128) * splits >= 480;
}

// the folded stage 2's wanted split: few rows (4 my) and a long reduction
inline int fold2_want_split(int my, int fold2_S) {
    const long tiles = (long)((4 * my + 31) / 32) * ((fold2_S + 63) / 64);
    return (int)std::min<long>(8, std::max<long>(1, 1024 / std::max<long>(tiles, 1)));
}

// zgemm_kernel's tile id: 15 = 128 x 64 with 8 waves as soon as that gives one workgroup per CU, 10 = 64 x 64
// likewise, else 11 = 32 x 32
inline int zgemm_tile(int M, int N, int batch) {
    const long t128 = (long)((M + 127) / 128) * ((N + 63) / 64) * batch;
    const long t64 = (long)((M + 63) / 64) * ((N + 63) / 64) * batch;
    if (t128 >= 256) return 15;
    if (t64 >= 256) return 10;
    return 11;
}

// ---- The launch rules of the pruned FFT on lattices of 256 R3 samples (zfft.hip): how an axis is cut
// into launches (farfield_plan.hip plan_fft_axis), the block of an interleaved shard (farfield.hip interleave_block) and
// which kernel instantiation a call launches (zfft.hip zfft_run, zfft_run_tiles, zfft_run_interleaved) - pure
// arithmetic over the call's facts, applied by those launchers and printed by tools/transform_route.cpp
// (tests/fft_cases.py).  The reasons and measurements stand with the kernels.

#ifndef ML_ZFFT_IP
// exchange 2 of the one-level kernel in place for lattices up to this many residues (A/B builds: 0 =
// never).  Measured on one box, stage 1: R3 = 16 (4096^2) 0.183 -> 0.179 ms, R3 = 8 (2048^2) 0.0585 ->
// 0.0579, R3 = 32 (8192^2, NA 0.94, one workgroup per CU) 0.678 -> 0.713: the longer bank-conflict
// tail of the in-place pattern costs more than the barrier where nothing else is resident to hide it
#define ML_ZFFT_IP 16
#endif
#ifndef ML_FFT_PASSES_R32
// default: two passes for 8192-sample lattices (one 131 KB workgroup per CU otherwise:
// stage 1 0.77 -> 0.71 ms at 8192^2); one pass below - at 4096 samples four two-wave
// workgroups per CU measured 12 % SLOWER than two four-wave ones with the register prefetch
// (R3 = 16 as 2 x 8: stage 1 0.201 against 0.178 ms; R3 = 8 as 2 x 4: 0.108 against 0.060)
#define ML_FFT_PASSES_R32 2
#endif

// Two-level transforms: an axis of N_eff = 256 R3 samples with R3 > 32 is transformed as s
// interleaved sub-sequences of N_eff / s samples (decimation in time: X[k] = sum_i W_N^(i k) X_i[k
// mod N / s]), each by one launch of the one-level kernel that adds its bins - carried to the full
// lattice by a per-bin phasor - to the result.  Smallest s that brings R3 / s to <= 32; 0 if none
// up to 16 does (R3 with no such divisor).
inline int zfft_split(int N_eff) {
    if (N_eff % 256) return 0;
    const int R3 = N_eff / 256;
    for (int s = 1; s <= 16; ++s)
        if (R3 % s == 0 && R3 / s <= 32) return s;
    return 0;
}

// Is the uniform grid u[0..M) a run of consecutive bins of the FFT lattice of an axis of n samples
// `step` apart?  kappa = n_glass / wavelength (turns per unit length per unit direction cosine).
// `tol`: allowed phase deviation [rad] at the aperture edge.  On success fills N_eff and j0.
// (N_plain, if given: the lattice the grid sits on, 0 if none, and *j0 its first bin - also where the function
// returns false because the 256 R3 scheme has no place for that lattice)
inline bool zfft_commensurate(int n, double step, long double kappa, const double *u, int M,
                       long double tol, int *N_eff, int *j0, int *jstep, int *N_plain = nullptr) {
    if (N_plain) *N_plain = 0;
    if (M < 2 || n < 2) return false;
    const long double du = ((long double)u[M - 1] - (long double)u[0]) / (M - 1);
    const long double turns = kappa * fabsl((long double)step) * du;   // per (sample, bin)
    if (!(turns > 0)) return false;                    // descending or degenerate grids: GEMM
    if (step < 0) return false;
    const long double inv = 1.0L / turns;
    if (!(inv < 1e7L)) return false;
    const long N = lrintl(inv);                        // the lattice the directions sit on
    if (N < n || N < M) return false;
    const long double du_exact = 1.0L / (kappa * fabsl((long double)step) * N);
    const long jj = lrintl((long double)u[0] / du_exact);
    // worst phase error over the grid at the outermost sample
    const long double p_max = 0.5L * n * fabsl((long double)step) + fabsl((long double)step);
    long double worst = 0;
    for (int j = 0; j < M; ++j)
        worst = fmaxl(worst, fabsl((long double)u[j] - (jj + j) * du_exact));
    const bool on_lattice = !(2 * M_PIl * kappa * p_max * worst > tol);
    // (N_plain: the lattice itself and its first bin, for the mixed-radix kernels - whether or not the 256 R3
    // scheme below has a place for it)
    if (on_lattice && N_plain && labs(jj) <= (1L << 29)) {
        *N_plain = (int)N;
        *j0 = (int)jj;
    }
    // The kernels transform 256 R3 samples.  A lattice that is not a multiple of 256 long - the
    // reference's default grids are the smallest 2^a 3^b 5^c above a goal (nearfield.py:30-36: 400, 1920,
    // 2000 ...) - runs on the s-times finer lattice of N s samples, s = 256 / gcd(N, 256), the aperture
    // zero-padded: its every s-th bin is a bin of the lattice asked for (Geo::jstep)
    long g = 256, r = N % 256;
    while (r) {
        const long t = g % r;
        g = r;
        r = t;
    }
    const long s = 256 / g, Ne = N * s;
    if (Ne > (1L << 20)) return false;
    const int R3 = (int)(Ne / 256);
    // one workgroup holds 8192 samples in LDS (257 * R3 * 16 bytes, R3 <= 32); longer lattices are
    // split into up to 16 interleaved sub-sequences, one launch each (zfft_split)
    if (R3 < 1 || zfft_split((int)Ne) == 0) return false;
    if (labs(jj) > (1L << 30) / s) return false;
    if (!on_lattice) return false;
    *N_eff = (int)Ne;
    *j0 = (int)jj;
    *jstep = (int)s;
    return true;
}

// How far (in radians of phase at the aperture edge) a direction grid may deviate from exact
// centre symmetry and still take the folded path: 1e-13 rad, or - for large apertures, where
// that is less than the grid's own representation error - four times the phase uncertainty that
// half an ulp of the largest direction cosine already carries (2 pi kappa p_max eps/2 max|u|).
// A grid computed as centre +/- k*step in floating point is symmetric to about one ulp; without
// the second term a 16384-sample aperture (4.3 mm at lambda/2.2) falls back to the generic
// complex GEMM, 5x slower, for an asymmetry of 3e-13 rad that the inputs cannot resolve anyway.
inline long double symmetry_tolerance(long double kappa, long double p_max, const double *u, int n) {
    long double umax = 0;
    for (int k = 0; k < n; ++k) umax = fmaxl(umax, fabsl((long double)u[k]));
    const long double inherent = 2 * M_PIl * kappa * p_max * umax * (long double)DBL_EPSILON * 0.5L;
    return fmaxl(1e-13L, 4 * inherent);
}

// Does the axis of m direction cosines u fold - is it centre-symmetric to symmetry_tolerance at the edge of an aperture
// axis of n samples `step` apart?  If so the folded (even/odd) GEMM (zfold.hip) runs over S = ceil(m / 2) half-
// directions v_s = (u[m-1-s] - u[s]) / 2 about the centre u_c = (u[0] + u[m-1]) / 2, both computed in long double and
// split into (hi, lo) doubles for the phase tables (farfield_plan.hip fold_tables).  m < 2 or n < 2: does not fold.
struct FoldSplit {
    bool ok = false;
    int S = 0;
    bool has_E = false;      // u_c != 0: the input carries the modulation E_k = exp(-i kappa p_k u_c)
    std::vector<double> v;   // hi[S], lo[S], then u_c as (hi, lo)
};

inline FoldSplit fold_split(const double *u, int m, int n, double step, double wavelength, double n_glass) {
    FoldSplit f;
    if (m < 2 || n < 2) return f;
    const int S = (m + 1) / 2;
    const long double kappa = (long double)n_glass / (long double)wavelength;
    const long double p_max = 0.5L * (n - 1) * fabsl((long double)step);
    const long double uc = 0.5L * ((long double)u[0] + (long double)u[m - 1]);
    std::vector<double> v(2 * (size_t)S + 2);
    long double worst = 0;
    for (int s = 0; s < S; ++s) {
        const long double up = u[m - 1 - s], um = u[s];
        worst = fmaxl(worst, fabsl(0.5L * (up + um) - uc));
        const long double vs = 0.5L * (up - um);
        v[s] = (double)vs;
        v[S + s] = (double)(vs - (long double)v[s]);
    }
    if (2 * M_PIl * kappa * p_max * worst > symmetry_tolerance(kappa, p_max, u, m)) return f;
    v[2 * (size_t)S] = (double)uc;
    v[2 * (size_t)S + 1] = (double)(uc - (long double)v[2 * (size_t)S]);
    f.ok = true;
    f.S = S;
    f.has_E = (uc != 0);
    f.v.swap(v);
    return f;
}

// the lattice of one axis of a plan, as plan_fft_axis asks for it: n samples `step` apart, sample j at
// (j - ceil(n / 2)) step, the m directions u
inline bool zfft_axis_lattice(int n, double step, double wavelength, double n_glass, const double *u, int m,
                              int *N_eff, int *j0, int *jstep, int *N_plain = nullptr) {
    const long double kappa = (long double)n_glass / (long double)wavelength;
    const long double p_max = 0.5L * (n + 1) * fabsl((long double)step);
    return zfft_commensurate(n, step, kappa, u, m, symmetry_tolerance(kappa, p_max, u, m), N_eff, j0, jstep, N_plain);
}

// How plan_fft_axis runs an axis whose M wanted bins sit on the lattice of N_eff = 256 R3 samples, every jstep-th bin
// a bin of the lattice asked for (zfft_commensurate): `split` launches over sub-sequences, or one launch in `passes`
// residue passes; taken = false: the method leaves this axis to the GEMMs
struct ZfftAxisRule {
    bool taken;
    int split, passes;
};

inline ZfftAxisRule zfft_axis_rule(int method, int N_eff, int jstep, int M) {
    ZfftAxisRule r{true, 0, 0};
    // A lattice that is not a multiple of 256 long runs jstep-fold padded, at jstep times the arithmetic and (beyond
    // 8192 padded samples) as many passes over the rows.  Measured against the folded GEMMs on square apertures
    // (tools/padded_fft_sweep.py, profiles/r06_padded_fft_sweep.txt; M = 64, 256, N directions): jstep 2 (1920, 3200
    // samples) 1.7-5.3 x faster, 4 (320, 960, 1600) 1.1-2.5 x, 8 (800, 1440, 2400) 0.5-1.1 x, 16 (400, 2000, 3600)
    // 0.1-0.7 x, 32 (1000, 3000) 0.1-0.2 x, 128 (250) 0.1 x.  `auto` leaves the lattices padded more than 4-fold to
    // the GEMMs; `fft-streamed` takes the FFT wherever there is one
    if (method == ML_METHOD_AUTO && jstep > 4) r.taken = false;
    r.split = zfft_split(N_eff);
    // 8192 < N_eff <= 16384 with at most 1024 wanted bins: one launch in two residue passes (every
    // row read once, whole 128-byte lines, no accumulating store) instead of two sub-sequences
    if (N_eff / 256 == 64 && M <= 1024) {   // (the two-pass kernel exists for groups of 16 and 32 residues)
        r.split = 1;
        r.passes = 2;
    }
    return r;
}

// A short transform of n_sub samples of an interleaved shard runs on the lattice of n_sub * stuff = 256 R3 samples,
// zero-stuffed when n_sub is below 256 (zfft_interleaved_kernel); 0: n_sub does not fit
inline int interleave_stuff(int n_sub) {
    for (int z = 1; z <= 8; z <<= 1)
        if ((n_sub * z) % 256 == 0) return z;
    return 0;
}

// Block size s of an interleaved shard over n_ranks ranks of an x axis on the lattice of N samples, nx_total of which
// exist (farfield.hip interleave_block: what the plan must be like); s as large as fits, up to 8; 0: none
inline int interleave_block_of(int N, int nx_total, int n_ranks) {
    if (n_ranks < 2) return 0;
    for (int s = 8; s >= 1; s >>= 1) {
        if (N % (s * n_ranks) != 0 || nx_total % (s * n_ranks) != 0) continue;
        const int stuff = interleave_stuff(N / (s * n_ranks));
        if (!stuff) continue;
        const int r3 = N / (s * n_ranks) * stuff / 256;
        // (the s transforms of a column share one workgroup: 16 r3 s threads, s buffers of 4 r3 KB)
        if (r3 >= 1 && r3 <= 32 && r3 * s <= 32) return s;
    }
    return 0;
}

// the facts of one launch: the lattice of the (sub-sequence of the) axis, the wanted bins, the axis' passes, how the
// rows lie (ZfftCall in_es == 1, second, tiled_out), the entry point (tiles: zfft_run_tiles; s > 0:
// zfft_run_interleaved with s transforms of n_valid samples, zero-stuffed `stuff`-fold, per column)
struct ZfftLaunchFacts {
    int N_eff = 0, M = 0, passes = 0;
    bool contiguous = false, second = false, tiled_out = false;
    bool tiles = false;
    int s = 0, stuff = 1, n_valid = 0;
};

enum class ZfftFamily { none, one, pass, multi, tiles, interleaved, cols128 };

// family = none: no kernel takes the facts (more than 32 residues in one launch)
struct ZfftLaunch {
    ZfftFamily family = ZfftFamily::none;
    int R3T = 0, PASS = 0;        // zfft_kernel<R3T, ., ., PASS, ip>: R3T = 0 the generic residue count; multi: PASS
    bool ip = false;              // exchange 2 in place
    int R3P = 0, P = 0, NB = 0;   // zfft_pass_kernel<R3P, P, NB, ., PASS>
    int threads = 0;              // of a workgroup
    int cpw = 0;                  // multi: rows per workgroup
    bool repad = false;           // the launcher chooses the paddings again (in place, pass geometry)
};

inline ZfftLaunch zfft_launch_rule(const ZfftLaunchFacts &f) {
    ZfftLaunch L;
    const int R3 = f.N_eff / 256;
    if (f.tiles) {
        L.family = ZfftFamily::tiles;
        L.threads = zf::TL_NT;
        return L;
    }
    if (f.s > 0) {
#ifndef ML_NO_COLS128
        if (f.stuff == 2 && f.N_eff == 256 && f.s == 8 && f.n_valid <= 128) {
            // eight 128-sample transforms per column: one wave each (zfft_cols128_kernel)
            L.family = ZfftFamily::cols128;
            L.threads = 64;
            return L;
        }
#endif
        L.family = ZfftFamily::interleaved;
        L.threads = 16 * R3 * f.s;
        return L;
    }
    // PASS (a template argument so that profiles can tell the launches apart): 1 rows of the aperture,
    // 2 strided columns of a row-major stage-1 result, 3 contiguous rows of a transposed one, 4 rows of the
    // aperture into a tiled one
    if (R3 <= 2) {
        // short transforms: 64 threads = 4 or 2 rows per workgroup (zfft_multi_kernel)
        L.family = ZfftFamily::multi;
        L.cpw = 4 / std::max(R3, 1);
        L.PASS = f.contiguous ? 1 : 2;
        L.threads = 16 * R3 * L.cpw;
        return L;
    }
    // pass-split form (zfft_pass_kernel): passes = 2 groups of residues, where an instantiation covers the shape
    const int P = f.passes > 0 ? f.passes : (R3 == 32 ? ML_FFT_PASSES_R32 : 1);
    if (P > 1 && R3 % P == 0) {
        const int R3P = R3 / P;
        if (P == 2 && (R3P == 16 || R3P == 32) && f.M <= 2 * 16 * R3P) {   // (NB = 2 wanted bins per thread)
            L.family = ZfftFamily::pass;
            L.R3P = R3P, L.P = P, L.NB = 2;
            L.PASS = f.contiguous ? (f.second ? 3 : 1) : 2;
            L.threads = 16 * R3P;
            L.repad = true;
            return L;
        }
    }
    if (R3 > 32) return L;
    const bool pow2 = R3 == 4 || R3 == 8 || R3 == 16 || R3 == 32;
    L.family = ZfftFamily::one;
    L.threads = 16 * R3;
    // the in-place layout answers to one padding, chosen for its four access patterns
    L.ip = L.repad = R3 <= ML_ZFFT_IP && pow2;
    if (f.contiguous && f.second && (R3 == 8 || R3 == 16 || R3 == 32))
        L.PASS = 3, L.R3T = R3;
    else if (f.tiled_out)   // pass 1 into a tiled G
        L.PASS = 4, L.R3T = pow2 && R3 != 32 ? R3 : 0;
    else
        L.PASS = f.contiguous ? 1 : 2, L.R3T = pow2 ? R3 : 0;
    return L;
}

}  // namespace ml
