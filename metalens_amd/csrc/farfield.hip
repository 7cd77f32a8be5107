// The near-to-far-field transform on MI355X: the resident aperture fields -> the four radiation vectors of every
// direction of the active plan (farfield_plan.hip), V_f[a][b] = alpha_f sum_n1 sum_n2 exp(-i k x'_n1 ux_a)
// F_f[n1][n2] exp(-i k y'_n2 uy_b), in two stages: stage 1 along y leaves G[(f, n1)][b], stage 2 along x the vectors.
// One call is validate -> route (transform_route.h decides the kind of each stage and G's layout, as a value) ->
// reserve G -> stage 1 -> stage 2; the stage launchers below consume the route.  A stage runs as
//   * a complex GEMM (zgemm.hip), or the column dot of a pair list;
//   * a folded GEMM on centre-symmetric directions (zfold.hip: real cos / sin tables over half the directions, split-K);
//     the folded stage 2 leaves its slabs in pl.fold2_ot and only RECORDS the unfold in pl.unfold: the projection
//     (farfield_project.hip) or flush_unfold consumes it;
//   * an output-pruned FFT on directions that sit on the aperture's FFT lattice (zfft.hip, zfft_rows.hip), over the rows
//     that meet the lens circle (trim_rows_of);
// and over the resident rows of a shard: a block, a mirrored pair of blocks, or interleaved blocks dealt round robin
// over the ranks, whose column pass is `block` short transforms (interleave_block).
// Layouts: G in transform_route.h (GLayout, g_view), the vectors and the plan's tables in common.h (FarfieldPlan).
// Entries: ml_farfield_transform, ml_farfield_transform_mirrored, their _async forms,
// ml_farfield_transform_interleaved_async and ml_farfield_interleave_block.
#include "common.h"
#include "zfft_core.h"

namespace ml {

// out[b][c][r] = sum_s in[s][b][r][c] (complex), 32 x 32 tiles through LDS; `splits` split-K
// slabs of `slab` elements each are summed on the way
__global__ __launch_bounds__(256) void ztranspose_kernel(const double2 *in, double2 *out, int rows,
                                                         int cols, int splits, size_t slab) {
    __shared__ double2 tile[32][33];
    const size_t plane = (size_t)rows * cols;
    in += blockIdx.z * plane;
    out += blockIdx.z * plane;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < rows && c0 + tx < cols) {
            double2 v = in[(size_t)(r0 + k) * cols + c0 + tx];
            for (int sp = 1; sp < splits; ++sp) {
                const double2 w = in[sp * slab + (size_t)(r0 + k) * cols + c0 + tx];
                v.x += w.x;
                v.y += w.y;
            }
            tile[k][tx] = v;
        }
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (c0 + k < cols && r0 + tx < rows) out[(size_t)(c0 + k) * rows + r0 + tx] = tile[tx][k];
}

// in[0] += in[1] + ... + in[splits-1]  (split-K slabs of stage 1 when the consumer is not the
// transposing kernel)
__global__ __launch_bounds__(256) void zsum_slabs_kernel(double2 *in, size_t n, int splits) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n) return;
    double2 v = in[at];
    for (int sp = 1; sp < splits; ++sp) {
        const double2 w = in[sp * n + at];
        v.x += w.x;
        v.y += w.y;
    }
    in[at] = v;
}

// Folded stage 2 for a mirror-symmetric set of resident rows: local row k pairs with local
// row nxl-1-k, pair t sits at +/-(half_x - row0 - t) dx.  G is transposed so that the
// reduction index is contiguous, run through the same folded kernel as stage 1 (rows = 4*my
// stage-1 columns, "directions" = ux), and transposed back with the signs applied.
// `gt_direct`: stage 1 already wrote its result transposed (GT layout, pl.stage1_splits slabs)
// AND multiplied by this stage's input modulation; the slabs are summed while the folded kernel
// loads its tiles and no transposer runs.  `tables_ready`: stage2_tables has been queued.
static int stage2_folded(ml_ctx *ctx, int row0, int mirrored, int accumulate, const double *alpha,
                         bool gt_direct, bool tables_ready, int want_split) {
    FarfieldPlan &pl = ctx->plan;
    const int nxl = ctx->fields.nx, mx = pl.mx, my = pl.my, S = pl.fold2_S, T = (nxl + 1) / 2;
    const size_t g_elems = (size_t)4 * nxl * my;
    if (!gt_direct) ML_TRY(pl.fold2_gt.reserve(g_elems * 2 * sizeof(double)));
    if (!tables_ready) ML_TRY(stage2_tables(ctx, row0, mirrored, &want_split));
    const int splits = zfold_splits(T, want_split);
    FoldIO io;
    const double *gt = pl.fold2_gt.as<double>();
    if (gt_direct) {
        gt = pl.stage1.as<double>();
        io.in_slabs = pl.stage1_splits;
        io.in_slab_stride = (int64_t)4 * nxl * my;
    } else {
        // G[(f, n1)][j] -> GT[(f, j)][n1]
        hipLaunchKernelGGL(ztranspose_kernel, dim3((my + 31) / 32, (nxl + 31) / 32, 4), dim3(256),
                           0, ctx->stream, pl.stage1.as<double2>(), pl.fold2_gt.as<double2>(), nxl,
                           my, pl.stage1_splits, (size_t)4 * nxl * my);
        ML_HIP(hipGetLastError());
    }
    pl.stage1_splits = 1;   // consumed
    ML_TRY(zfold_stage1(ctx->stream, 4 * my, nxl, gt, nxl,
                        pl.fold_x.cm.as<double>(), pl.fold_x.sm.as<double>(), pl.fold_x.r4.as<double>(),
                        T, S, pl.fold_x.has_E && !gt_direct ? pl.fold_x.E.as<double>() : nullptr,
                        pl.fold_x.D.as<double>(), pl.fold2_ot.as<double>(), mx, mx, nullptr, 1,
                        want_split, (int64_t)4 * my * mx, ctx->gemm_f32 != 0, io));
    // the slabs are summed / transposed / signed into `vectors` by the next consumer: the
    // projection kernel if it comes first (one launch for both), flush_unfold otherwise
    for (int k = 0; k < 4; ++k) pl.unfold.alpha[k] = alpha[k];
    pl.unfold.splits = splits;
    pl.unfold.accumulate = accumulate;
    pl.unfold.pending = true;
    static const bool eager = diag_int("ML_EAGER_UNFOLD", 0) != 0;
    if (eager) ML_TRY(flush_unfold(ctx));
    return ML_OK;
}

// Block size of an interleaved shard over n_ranks ranks: rank r holds the rows n = s (G m + r) + i,
// i < s - blocks of s rows, dealt round robin.  The column pass of such a shard is s transforms of
// Nsub = N / (s G) points per column (decimation in time: the partial sum over rows sG apart IS a
// short DFT on the same bins), i.e. 1 / G of the whole aperture's column pass, where a contiguous
// or mirrored block of rows costs every rank the full-length pass.  Needs the x axis on the pruned
// FFT with a lattice of exactly the aperture's rows; Nsub = 256 R3 with R3 <= 32.  s is taken as
// large as that allows (up to 8: the synthesis works on 8-row patches and wants neighbouring rows).
// (transform_route.h interleave_stuff, interleave_block_of)
static int interleave_block(const FarfieldPlan &pl, int n_ranks) {
    if (!pl.ready || pl.pair_list || !pl.fft_x.ok || pl.fft_x.A || n_ranks < 2) return 0;
    // N = the x axis' lattice (longer than the aperture when the direction grid is finer than the
    // aperture's own: the rows beyond nx_total are zeros nobody holds); the rows that exist must
    // deal out evenly
    return interleave_block_of(pl.fft_x.N_eff, pl.nx_total, n_ranks);
}

static int validate_shard(ml_ctx *ctx, const Shard &sh, int accumulate) {
    ML_REQUIRE(ctx, "ctx is NULL");
    const int row0 = sh.row0;
    FarfieldPlan &pl = ctx->plan;
    if (!pl.ready) {
        set_error("ml_farfield_plan has not been called");
        return ML_ESTATE;
    }
    if (ctx->fields.nx == 0) {
        set_error("no resident field set");
        return ML_ESTATE;
    }
    ML_REQUIRE(ctx->fields.ny == pl.ny, "resident fields have ny=%d but the plan has ny=%d", ctx->fields.ny,
               pl.ny);
    if (sh.kind == ShardKind::interleaved) {
        ML_REQUIRE(sh.block >= 1 && sh.block == interleave_block(pl, sh.n_ranks),
                   "interleaved shard: block %d is not what ml_farfield_interleave_block gives for %d ranks "
                   "on this plan (%d)", sh.block, sh.n_ranks, interleave_block(pl, sh.n_ranks));
        ML_REQUIRE(sh.rank >= 0 && sh.rank < sh.n_ranks && ctx->fields.nx == pl.nx_total / sh.n_ranks,
                   "interleaved shard: rank %d of %d with %d resident rows of %d", sh.rank, sh.n_ranks,
                   ctx->fields.nx, pl.nx_total);
    } else if (sh.kind == ShardKind::mirrored) {
        ML_REQUIRE(ctx->fields.nx % 2 == 0 && row0 >= 0 && 2 * row0 + ctx->fields.nx <= pl.nx_total,
                   "mirrored shard: %d resident rows starting at %d do not form row pairs of a "
                   "%d-row aperture", ctx->fields.nx, row0, pl.nx_total);
        ML_REQUIRE(!pl.pair_list, "mirrored shards are for tensor grids");
    } else {
        ML_REQUIRE(row0 >= 0 && row0 + ctx->fields.nx <= pl.nx_total,
                   "rows [%d, %d) fall outside the planned aperture of %d rows", row0,
                   row0 + ctx->fields.nx, pl.nx_total);
    }
    ML_REQUIRE(!accumulate || pl.have_vectors, "accumulate requested but nothing to add to");
    return ML_OK;
}

// (diagnostic builds: the route's knobs from the environment, read once)
static const RouteKnobs &route_knobs() {
    static const RouteKnobs knobs = [] {
        RouteKnobs k;
        k.stage1_split = diag_int("ML_STAGE1_SPLIT", k.stage1_split);
        k.g_skew = diag_int("ML_G_SKEW", k.g_skew);
        k.g_tiled = diag_int("ML_G_TILED", k.g_tiled);
        k.fold2_min_tiles = diag_int("ML_FOLD2_MIN_TILES", (int)k.fold2_min_tiles);
        k.no_row_trim = diag_int("ML_NO_ROW_TRIM", k.no_row_trim);
        k.no_gt_direct = diag_int("ML_NO_GT_DIRECT", k.no_gt_direct);
        return k;
    }();
    return knobs;
}

// The resident rows that meet the lens circle (transform_route.h), into ctx->grid.trim_rows, found once per (grid, layout).
// false: the resident fields carry no row_first for their grid (uploaded fields) - nothing is known about their rows.
static bool trim_rows_of(ml_ctx *ctx) {
    const SynthGrid &grid = ctx->grid;
    const int nxl = ctx->fields.nx;
    const double r_outer = ctx->lens.search.r_outer;
    if (!ctx->caches.rows_describe_fields || (int)grid.h_x_pts.size() != nxl || (int)grid.h_y_pts.size() != ctx->fields.ny ||
        !(r_outer > 0))
        return false;
    const Key<2> key = ctx->caches.grid_layout_key();
    if (!ctx->caches.trim.matches(key.v)) {
        double ymin = INFINITY;
        for (double y : grid.h_y_pts) ymin = std::min(ymin, std::fabs(y));
        int lo = nxl, hi = 0;
        for (int i = 0; i < nxl; ++i) {
            const double x = grid.h_x_pts[i];
            if (!(std::sqrt(x * x + ymin * ymin) > r_outer)) {
                lo = std::min(lo, i);
                hi = i + 1;
            }
        }
        if (lo >= hi) lo = 0, hi = std::min(nxl, 1);   // (an empty window keeps one row: nothing to gain)
        ctx->grid.trim_rows[0] = lo;
        ctx->grid.trim_rows[1] = hi;
        ctx->caches.trim.set(key.v);
    }
    return true;
}

// G of this call: in physical pieces where the route wants them and they can be had (transform_route.h), else hipMalloc
static int reserve_g(FarfieldPlan &pl, const TransformRoute &rt, double **g) {
    static const bool pieces_off = [] { const char *e = getenv("METALENS_HIP_PIECES"); return e && e[0] == '0'; }();
    const size_t bytes = (size_t)pl.stage1_splits * rt.g_bytes;
    const bool pieced = rt.pieces_wanted && !pieces_off && pl.stage1_pieces.reserve(bytes) == ML_OK;
    if (!pieced) ML_TRY(pl.stage1.reserve(bytes));
    *g = pieced ? pl.stage1_pieces.as<double>() : pl.stage1.as<double>();
    return ML_OK;
}

// the axis part of a call: the lattice of (a sub-sequence of) the axis, its M wanted bins and its tables
static void call_axis(ZfftCall &c, const FarfieldPlan &pl, const ZfftAxis &ax, int M) {
    c.passes = ax.passes;
    c.N_eff = ax.N_eff / ax.split;
    c.M = M;
    c.j0 = ax.j0;
    c.jstep = ax.jstep;
    c.pad1 = ax.pad1;
    c.pad2 = ax.pad2;
    c.tw1 = ax.A ? ax.tw.as<double>() : pl.fft_tw1.as<double>();
    c.mixA = ax.A;
    c.mixB = ax.B;
    c.wk = ax.wk.as<double>();
    c.pj = ax.pj.as<double>();
    c.kbin = ax.kbin.as<int>();
}

// the output part of a column pass: row (f, b) of the call, bin a -> V[3 - f][a][b] * alpha_f
static void call_into_vectors(ZfftCall &c, const FarfieldPlan &pl, const double *alpha) {
    c.out = pl.vectors.as<double>() + (size_t)3 * pl.mx * pl.my * 2;
    c.out_rb = pl.my;
    c.out_s1 = -(int64_t)pl.mx * pl.my;
    c.out_s2 = 1;
    c.out_es = pl.my;
    for (int k = 0; k < 4; ++k) c.alpha[k] = alpha[k];
    c.alpha_rb = pl.my;
}

// one launch per sub-sequence of the axis (two-level: sub-sequence i of every row adds its bins, zfft.hip zfft_split)
static int run_subsequences(hipStream_t stream, ZfftCall &c, const ZfftAxis &ax, int accumulate) {
    for (int i = 0; i < ax.split; ++i) {
        c.sub_s = ax.split;
        c.sub_i = i;
        c.pj = ax.pj.as<double>() + (size_t)i * c.M * 2;
        c.accumulate = i > 0 ? 1 : accumulate;
        ML_TRY(zfft_run(stream, c));
    }
    return ML_OK;
}

// stage 1 as a pruned FFT along y
static int stage1_fft(ml_ctx *ctx, const TransformRoute &rt, double *g) {
    FarfieldPlan &pl = ctx->plan;
    const int nxl = ctx->fields.nx, ny = pl.ny, my = pl.my, trim_lo = rt.trim_lo, nxt = rt.trim_hi - rt.trim_lo;
    const GView v = g_view(rt.g_layout, nxl, my, rt.g_ld, trim_lo);
    ZfftCall c;
    call_axis(c, pl, pl.fft_y, my);
    c.n_valid = ny;
    // row (f, n1') of the launch = row n1 = trim_lo + n1' of field plane f
    c.in = ctx->fields.set_ptr() + (size_t)trim_lo * ny * 2;
    c.rows = 4 * nxt;
    c.in_rb = nxt;
    c.in_s1 = (int64_t)nxl * ny;
    c.in_s2 = ny;
    c.in_es = 1;
    c.a0 = 0;
    c.h0 = ny;
    c.a1 = c.h1 = 0;
    c.row_first = ctx->caches.rows_describe_fields ? ctx->grid.row_first.as<int>() + trim_lo : nullptr;
    c.rf_mod = nxt;
    c.out = g + (size_t)v.off * 2;
    c.out_rb = nxt;
    c.out_s1 = v.s_f;
    c.out_s2 = v.s_row;
    c.out_es = v.s_bin;
    c.tiled_out = rt.g_layout == GLayout::tiled;
    for (int k = 0; k < 4; ++k) c.alpha[k] = 1.0;
    c.alpha_rb = c.rows;   // (every row: alpha[0])
    return run_subsequences(ctx->stream, c, pl.fft_y, 0);
}

// stage 1: G[(f, n1)][b] = sum_n2 F_f[n1][n2] * exp(-i k y'_n2 uy_b)
static int stage1(ml_ctx *ctx, const TransformRoute &rt, double *g) {
    FarfieldPlan &pl = ctx->plan;
    const int nxl = ctx->fields.nx, ny = pl.ny, my = pl.my;
    // resident fields that the synthesis already multiplied by this plan's input modulation
    // (ml_nearfield_premodulate): stage 1 then runs without it
    bool fields_premodulated = false;
    if (ctx->fields.premod_serial >= 0) {
        if (ctx->fields.premod_serial != pl.serial || !pl.fold) {
            set_error("the resident fields carry the input modulation of an earlier far-field plan "
                      "(ml_nearfield_premodulate): synthesise them again after ml_farfield_plan");
            return ML_ESTATE;
        }
        fields_premodulated = true;
    }
    ProfScope scope(ctx, ML_K_ZGEMM_STAGE1);
    if (rt.stage1 == Stage1Kind::fft) return stage1_fft(ctx, rt, g);
    if (rt.stage1 == Stage1Kind::folded) {
        FoldIO io;
        const FoldAxis &fy = pl.fold_y;
        if (rt.gt_direct) {   // (stage2_tables has run: fold_x.E is stage 2's input modulation)
            io.out_t_rows = nxl;
            io.out_E = pl.fold_x.has_E ? pl.fold_x.E.as<double>() : nullptr;
        }
        return zfold_stage1(ctx->stream, 4 * nxl, ny, ctx->fields.set_ptr(), ny, fy.cm.as<double>(), fy.sm.as<double>(),
                            fy.r4.as<double>(), (ny + 1) / 2, pl.fold_S,
                            fy.has_E && !fields_premodulated ? fy.E.as<double>() : nullptr, fy.D.as<double>(), g, my, my,
                            ctx->caches.rows_describe_fields ? ctx->grid.row_first.as<int>() : nullptr, nxl, rt.want_split1,
                            (int64_t)4 * nxl * my, ctx->gemm_f32 != 0, io);
    }
    const double one[4] = {1.0, 1.0, 1.0, 1.0};
    return zgemm(ctx->stream, 4 * nxl, my, ny, one, ctx->fields.set_ptr(), ny, 0, pl.tw_y.as<double>(), my, 0, g, my, 0, 1,
                 0);
}

// the split-K slabs of a folded stage 1 summed into the first, for a stage 2 that reads one array
static int collapse_stage1(ml_ctx *ctx, double *g) {
    FarfieldPlan &pl = ctx->plan;
    if (pl.stage1_splits > 1) {
        const size_t n = (size_t)4 * ctx->fields.nx * pl.my;
        hipLaunchKernelGGL(zsum_slabs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                           ctx->stream, reinterpret_cast<double2 *>(g), n, pl.stage1_splits);
        ML_HIP(hipGetLastError());
        pl.stage1_splits = 1;
    }
    return ML_OK;
}

// stage 2 of an interleaved shard: `block` short transforms per column (see interleave_block).
// Transform i reads the local rows i, i + s, i + 2 s, ... of column (f, b) and adds its M
// bins, carried to the full lattice by pj[i][.], into V[3 - f][.][b]
static int stage2_interleaved(ml_ctx *ctx, const TransformRoute &rt, const Shard &sh, const double *g,
                              const double *alpha, int accumulate) {
    FarfieldPlan &pl = ctx->plan;
    const int nxl = ctx->fields.nx, mx = pl.mx, my = pl.my;
    const int s = sh.block, G = sh.n_ranks, N = pl.fft_x.N_eff;
    const int stuff = interleave_stuff(N / (s * G)), Nsub = N / (s * G) * stuff;   // the lattice it runs on
    const int n_have = pl.nx_total / (s * G);   // samples of each short transform that exist
    const long key[4] = {pl.serial, s, G, sh.rank};
    if (!pl.il_for.matches(key)) {
        ML_TRY(pl.il_wk.reserve((size_t)mx * 2 * sizeof(double)));
        ML_TRY(pl.il_kbin.reserve((size_t)mx * sizeof(int)));
        ML_TRY(pl.il_pj.reserve((size_t)s * mx * 2 * sizeof(double)));
        ML_TRY(zfft_build_interleave_tables(ctx->stream, pl.il_wk.as<double>(), pl.il_pj.as<double>(),
                                            pl.il_kbin.as<int>(), mx, pl.fft_x.j0, Nsub, N,
                                            pl.nx_total - pl.nx_total / 2, s * sh.rank, s, pl.fft_x.jstep));
        zfft_choose_pads(Nsub, mx, pl.fft_x.j0, &pl.il_pad1, &pl.il_pad2, pl.fft_x.jstep);
        pl.il_for.set(key);
    }
    // (the row-major G from its first local row: the rows stage 1 left out are told by a0 / h0)
    const GView v = g_view(rt.g_layout, nxl, my, rt.g_ld, 0);
    ZfftCall c;
    c.N_eff = Nsub;
    c.n_valid = n_have;
    c.M = mx;
    c.j0 = pl.fft_x.j0;
    c.jstep = pl.fft_x.jstep;
    c.pad1 = pl.il_pad1;
    c.pad2 = pl.il_pad2;
    c.in = g;
    c.rows = 4 * my;
    c.in_rb = v.cols;
    c.in_s1 = v.s_f;
    c.in_s2 = v.s_bin;
    c.in_es = (int64_t)s * v.s_row;
    // (local rows [a0, a0 + h0) exist in G: stage 1 left out the rows outside the lens circle)
    c.a0 = rt.trim_lo;
    c.h0 = rt.trim_hi - rt.trim_lo;
    c.a1 = c.h1 = 0;
    c.row_first = nullptr;
    c.rf_mod = 1;
    call_into_vectors(c, pl, alpha);
    c.tw1 = pl.fft_tw1.as<double>();
    c.wk = pl.il_wk.as<double>();
    c.pj = pl.il_pj.as<double>();
    c.kbin = pl.il_kbin.as<int>();
    c.accumulate = accumulate;
    return zfft_run_interleaved(ctx->stream, c, s, my, stuff);
}

// stage 2 along x as a pruned FFT over the columns of stage 1's result: row (f, b) reads
// G[f][n1][b] for the resident n1 (zero elsewhere) and writes V[3 - f][a][b] * alpha_f
static int stage2_fft(ml_ctx *ctx, const TransformRoute &rt, const Shard &sh, const double *g, const double *alpha,
                      int accumulate) {
    FarfieldPlan &pl = ctx->plan;
    const int nxl = ctx->fields.nx, mx = pl.mx, my = pl.my;
    const GView v = g_view(rt.g_layout, nxl, my, rt.g_ld, rt.trim_lo);
    ZfftCall c;
    call_axis(c, pl, pl.fft_x, mx);
    c.n_valid = pl.nx_total;
    c.in = g + (size_t)v.off * 2;
    c.rows = 4 * my;
    c.in_rb = v.cols;   // (tiled: tile (f, t) at f in_s1 + t in_s2, my / 8 tiles per plane)
    c.in_s1 = v.s_f;
    c.in_s2 = v.s_bin;
    c.in_es = v.s_row;
    c.second = rt.g_layout == GLayout::transposed;
    if (sh.kind == ShardKind::mirrored) {
        c.a0 = sh.row0;
        c.h0 = nxl / 2;
        c.a1 = pl.nx_total - sh.row0 - nxl / 2;
        c.h1 = nxl / 2;
    } else {
        // (resident rows = the rows stage 1 transformed: those outside the lens circle were never written)
        c.a0 = sh.row0 + rt.trim_lo;
        c.h0 = rt.trim_hi - rt.trim_lo;
        c.a1 = c.h1 = 0;
    }
    c.row_first = nullptr;
    c.rf_mod = 1;
    call_into_vectors(c, pl, alpha);
    if (rt.stage2 == Stage2Kind::fft_tiles) {
        c.accumulate = accumulate;
        return zfft_run_tiles(ctx->stream, c);
    }
    return run_subsequences(ctx->stream, c, pl.fft_x, accumulate);
}

// stage 2: V_f[a][b] = alpha_f * sum_n1 exp(-i k x'_n1 ux_a) * G[(f, n1)][b];
// batch entry f writes radiation-vector slot 3 - f.  One GEMM per run of resident rows: two on a mirrored shard
static int stage2_generic(ml_ctx *ctx, const Shard &sh, const double *g, const double *alpha, int accumulate) {
    FarfieldPlan &pl = ctx->plan;
    const int nxl = ctx->fields.nx, mx = pl.mx, my = pl.my, row0 = sh.row0;
    const int runs = sh.kind == ShardKind::mirrored ? 2 : 1, h = nxl / runs;
    double *slot3 = pl.vectors.as<double>() + (size_t)3 * mx * my * 2;
    for (int run = 0; run < runs; ++run) {
        const int first = run == 0 ? row0 : pl.nx_total - row0 - h;
        ML_TRY(zgemm(ctx->stream, mx, my, h, alpha, pl.tw_x.as<double>() + (size_t)first * 2, pl.nx_total, 0,
                     g + (size_t)run * h * my * 2, my, (int64_t)nxl * my, slot3, my, -(int64_t)mx * my, 4,
                     run == 0 ? accumulate : 1));
    }
    return ML_OK;
}

static int stage2(ml_ctx *ctx, const TransformRoute &rt, const Shard &sh, double *g, int want_split2,
                  int accumulate) {
    FarfieldPlan &pl = ctx->plan;
    const int mirrored = sh.kind == ShardKind::mirrored;
    const double dA = pl.dxp * pl.dyp;
    // fields are stored Ex,Ey,Hx,Hy; radiation vectors Nx,Ny,Lx,Ly = -Hy, Hx, Ey, -Ex (x dA)
    const double alpha[4] = {-dA, dA, dA, -dA};
    const bool needs_tw_x = rt.stage2 == Stage2Kind::generic || rt.stage2 == Stage2Kind::generic_mirrored ||
                            rt.stage2 == Stage2Kind::coldot;
    if (needs_tw_x) ML_TRY(need_tw_x(ctx));
    ProfScope scope(ctx, rt.stage2 == Stage2Kind::coldot ? ML_K_COLDOT : ML_K_ZGEMM_STAGE2);
    if (rt.stage2 == Stage2Kind::folded)   // (sums stage 1's slabs itself)
        return stage2_folded(ctx, sh.row0, mirrored, accumulate, alpha, rt.gt_direct, rt.gt_direct, want_split2);
    ML_TRY(collapse_stage1(ctx, g));
    switch (rt.stage2) {
    case Stage2Kind::interleaved: return stage2_interleaved(ctx, rt, sh, g, alpha, accumulate);
    case Stage2Kind::fft:
    case Stage2Kind::fft_tiles: return stage2_fft(ctx, rt, sh, g, alpha, accumulate);
    case Stage2Kind::coldot:
        return zcoldot(ctx->stream, 4, ctx->fields.nx, pl.mx, alpha, pl.tw_x.as<double>(), pl.mx, sh.row0, g,
                       pl.vectors.as<double>(), accumulate);
    default: return stage2_generic(ctx, sh, g, alpha, accumulate);
    }
}

// One far-field step: validate -> route (transform_route.h) -> reserve G -> stage 1 -> stage 2
static int transform_impl(ml_ctx *ctx, const Shard &sh, int accumulate) {
    ML_TRY(validate_shard(ctx, sh, accumulate));
    FarfieldPlan &pl = ctx->plan;
    ML_HIP(hipSetDevice(ctx->device));
    // a deferred unfold of the previous transform: needed if this one adds to it, moot otherwise
    if (accumulate)
        ML_TRY(flush_unfold(ctx));
    else
        pl.unfold.pending = false;
    const TransformRoute rt =
        transform_route(pl, pl.fft_y, pl.fft_x, sh, ctx->fields.nx, trim_rows_of(ctx), ctx->grid.trim_rows, route_knobs());
    pl.stage1_splits = pl.fold ? zfold_splits((pl.ny + 1) / 2, rt.want_split1) : 1;
    double *g = nullptr;
    ML_TRY(reserve_g(pl, rt, &g));
    int want_split2 = 1;
    // both stages folded: stage 2's tables first, stage 1's epilogue applies stage 2's input modulation
    if (rt.gt_direct) ML_TRY(stage2_tables(ctx, sh.row0, sh.kind == ShardKind::mirrored, &want_split2));
    ML_TRY(stage1(ctx, rt, g));
    ML_TRY(stage2(ctx, rt, sh, g, want_split2, accumulate));
    pl.have_vectors = true;
    pl.amplitudes_reduced = false;
    return ML_OK;
}

static Shard block_shard(int row0, int mirrored) {
    Shard sh;
    sh.kind = mirrored ? ShardKind::mirrored : ShardKind::block;
    sh.row0 = row0;
    return sh;
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_farfield_transform_async(ml_ctx *ctx, int row0, int accumulate) {
    return transform_impl(ctx, block_shard(row0, 0), accumulate);
}

int ml_farfield_transform_mirrored_async(ml_ctx *ctx, int row0, int accumulate) {
    return transform_impl(ctx, block_shard(row0, 1), accumulate);
}

int ml_farfield_transform(ml_ctx *ctx, int row0, int accumulate) {
    ML_TRY(transform_impl(ctx, block_shard(row0, 0), accumulate));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return prof_harvest(ctx);
}

int ml_farfield_transform_mirrored(ml_ctx *ctx, int row0, int accumulate) {
    ML_TRY(transform_impl(ctx, block_shard(row0, 1), accumulate));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return prof_harvest(ctx);
}

int ml_farfield_interleave_block(ml_ctx *ctx, int n_ranks, int *block) {
    ML_REQUIRE(ctx && block, "NULL argument");
    if (!ctx->plan.ready) {
        set_error("ml_farfield_plan has not been called");
        return ML_ESTATE;
    }
    *block = interleave_block(ctx->plan, n_ranks);
    return ML_OK;
}

int ml_farfield_transform_interleaved_async(ml_ctx *ctx, int block, int n_ranks, int rank, int accumulate) {
    Shard sh;
    sh.kind = ShardKind::interleaved;
    sh.block = block;
    sh.n_ranks = n_ranks;
    sh.rank = rank;
    return transform_impl(ctx, sh, accumulate);
}

}  // extern "C"
