// The 2-D transform of the padded planes of the FFT form of the finite-distance propagator: what every pass of
// propagate_grid.hip, propagate_grid_tiled.hip, propagate_grid_fine.hip and propagate_stack.hip sends its kernel, current
// and output planes through (grid_fft_rows, grid_fft_cols), and the upload of the twiddle tables (grid_upload_twiddles).
// fp64, in place, no atomics.  It serves no entry of its own.
//
// The transform (propagate_grid.h grid_axis_route): radix-2 stages, decimation in frequency forward and in time back, no
// reordering; up to three stages in registers per exchange.  Twiddles from the host's table (long double, rounded once).
//   rows:    contiguous along y, a whole row (or several short ones) per workgroup in the LDS;
//   columns: GRID_COLS = 8 adjacent columns per workgroup - every global access is 128 contiguous bytes - with blocks
//            of up to 1024 elements in the LDS; the stages above 1024 in a streaming pass (8 elements per thread, a
//            wave reads 1 KiB contiguous per element).
// Rows that are zero are not transformed: a row pass takes the rows [0, rows) (the column passes take every column).
// An axis of L = 16384 (the long plan) as well:
//   rows:    the stages above a block of GRID_ROW_BLOCK elements in a streaming pass (grid_rows_top_kernel: the
//            L / GRID_ROW_BLOCK elements of one row at that stride per thread, adjacent lanes adjacent elements), the
//            rest on blocks of a row in the LDS (grid_rows_block_kernel);
//   columns: the streaming pass with 16 elements per thread, then the blocks of 1024.
// Layouts: planes [planes][Lx][Ly] back to back (GridFftArgs); the LDS slots in propagate_grid.h (grid_lds_slot); the
// tables in PropagatePlan::grid_tw_x, grid_tw_y (common.h).
// The launchers read the lengths of the ACTIVE plan (ctx->prop.grid.Lx, Ly) and its tables: a prepare sets pp.grid and
// uploads the tables before its first transform.
// Known limit: the `attr_done` flags below (the LDS size a kernel may ask for, set once) are per process, not per device.
#include "propagate_grid_launch.h"

namespace ml {

typedef double2 d2;

// forward: (a, b) -> (a + b, (a - b) conj(w));  back: (a, b) -> (a + w b, a - w b);  w = (cos, sin)
template <bool INV>
__device__ __forceinline__ void bfly(d2 &a, d2 &b, d2 w) {
    if (!INV) {
        const d2 s = make_double2(a.x + b.x, a.y + b.y), d = make_double2(a.x - b.x, a.y - b.y);
        a = s;
        b = make_double2(fma(d.x, w.x, d.y * w.y), fma(d.y, w.x, -(d.x * w.y)));
    } else {
        const d2 t = make_double2(fma(b.x, w.x, -(b.y * w.y)), fma(b.x, w.y, b.y * w.x));
        b = make_double2(a.x - t.x, a.y - t.y);
        a = make_double2(a.x + t.x, a.y + t.y);
    }
}

// R stages in registers: v[e] is the element at pos0 + e estride of a block of B = estride 2^R (pos0 < estride) of a
// transform of length L; stage t has blocks of B >> t (forward: t = 0 ... R - 1, back: the reverse)
template <int R, bool INV>
__device__ __forceinline__ void stage_group(d2 (&v)[1 << R], const d2 *__restrict__ tw, int L, int B, int pos0, int estride) {
#pragma unroll
    for (int tt = 0; tt < R; ++tt) {
        const int t = INV ? R - 1 - tt : tt;
        const int he = (1 << R) >> (t + 1);       // partner distance in elements of v
        const int tw_step = L / (B >> t);          // table entries per position of the stage's block
#pragma unroll
        for (int e = 0; e < (1 << R); ++e) {
            if (e & he) continue;
            const int p_low = pos0 + (e & (he - 1)) * estride;   // < (B >> t) / 2
            bfly<INV>(v[e], v[e + he], tw[p_low * tw_step]);
        }
    }
}

template <int R, bool INV>
__device__ __forceinline__ void lds_group(d2 *s, int nseq, int len, int seq_slots, const d2 *__restrict__ tw, int L, int B) {
    const int per_seq = len >> R, estride = B >> R;
    for (int wi = threadIdx.x; wi < nseq * per_seq; wi += blockDim.x) {
        const int seq = wi / per_seq, rem = wi - seq * per_seq;
        const int blk = rem / estride, pos0 = rem - blk * estride;
        d2 *base = s + (size_t)seq * seq_slots;
        const int p0 = blk * B + pos0;
        d2 v[1 << R];
#pragma unroll
        for (int e = 0; e < (1 << R); ++e) v[e] = base[grid_lds_slot(p0 + e * estride)];
        stage_group<R, INV>(v, tw, L, B, pos0, estride);
#pragma unroll
        for (int e = 0; e < (1 << R); ++e) base[grid_lds_slot(p0 + e * estride)] = v[e];
    }
    __syncthreads();
}

// the stages of block size len ... 2 (back: 2 ... len) of nseq sequences of len elements in the LDS, each a block of a
// transform of length L.  Groups of three stages; the one or two left over run at the large end.
template <bool INV>
__device__ __forceinline__ void lds_stages(d2 *s, int nseq, int len, int seq_slots, const d2 *__restrict__ tw, int L) {
    const int S = 31 - __clz(len), rest = S % 3;
    if (!INV) {
        int B = len;
        if (rest == 1) lds_group<1, false>(s, nseq, len, seq_slots, tw, L, B);
        if (rest == 2) lds_group<2, false>(s, nseq, len, seq_slots, tw, L, B);
        for (B >>= rest; B > 1; B >>= 3) lds_group<3, false>(s, nseq, len, seq_slots, tw, L, B);
    } else {
        for (int B = 8; B <= (len >> rest); B <<= 3) lds_group<3, true>(s, nseq, len, seq_slots, tw, L, B);
        if (rest == 1) lds_group<1, true>(s, nseq, len, seq_slots, tw, L, len);
        if (rest == 2) lds_group<2, true>(s, nseq, len, seq_slots, tw, L, len);
    }
}

struct GridFftArgs {
    d2 *planes;             // [planes][Lx][Ly]
    size_t plane_stride;    // elements
    const d2 *tw;           // the axis' table
    int Lx, Ly;
    int rows;               // row pass: the rows [0, rows) are transformed
    int per_wg;             // row pass: rows per workgroup;  column pass: elements of a column in the LDS
};

// rows [blockIdx.x per_wg, ...) of plane blockIdx.y along y
template <bool INV>
__global__ __launch_bounds__(1024) void grid_rows_kernel(const GridFftArgs a) {
    extern __shared__ __align__(16) unsigned char grid_lds_raw[];
    d2 *s = reinterpret_cast<d2 *>(grid_lds_raw);
    const int L = a.Ly, row0 = blockIdx.x * a.per_wg, nseq = min(a.per_wg, a.rows - row0);
    const int seq_slots = grid_lds_seq(L);
    d2 *g = a.planes + blockIdx.y * a.plane_stride + (size_t)row0 * L;
    for (int idx = threadIdx.x; idx < nseq * L; idx += blockDim.x) {
        const int r = idx / L, p = idx - r * L;
        s[(size_t)r * seq_slots + grid_lds_slot(p)] = g[idx];
    }
    __syncthreads();
    lds_stages<INV>(s, nseq, L, seq_slots, a.tw, L);
    for (int idx = threadIdx.x; idx < nseq * L; idx += blockDim.x) {
        const int r = idx / L, p = idx - r * L;
        g[idx] = s[(size_t)r * seq_slots + grid_lds_slot(p)];
    }
}

// the rows [blockIdx.y per_wg, + per_wg) of the columns [8 blockIdx.x, + 8) of plane blockIdx.z along x: the stages of
// block size per_wg and below
template <bool INV>
__global__ __launch_bounds__(1024) void grid_cols_kernel(const GridFftArgs a) {
    extern __shared__ __align__(16) unsigned char grid_lds_raw[];
    d2 *s = reinterpret_cast<d2 *>(grid_lds_raw);
    const int len = a.per_wg, seq_slots = grid_lds_seq(len);
    d2 *g = a.planes + blockIdx.z * a.plane_stride + (size_t)blockIdx.y * len * a.Ly + blockIdx.x * GRID_COLS;
    for (int idx = threadIdx.x; idx < len * GRID_COLS; idx += blockDim.x) {
        const int i = idx / GRID_COLS, c = idx % GRID_COLS;
        s[(size_t)c * seq_slots + grid_lds_slot(i)] = g[(size_t)i * a.Ly + c];
    }
    __syncthreads();
    lds_stages<INV>(s, GRID_COLS, len, seq_slots, a.tw, a.Lx);
    for (int idx = threadIdx.x; idx < len * GRID_COLS; idx += blockDim.x) {
        const int i = idx / GRID_COLS, c = idx % GRID_COLS;
        g[(size_t)i * a.Ly + c] = s[(size_t)c * seq_slots + grid_lds_slot(i)];
    }
}

// the R stages of block size Lx ... Lx >> (R - 1) along x, without LDS: a thread holds the 2^R elements
// pos0 + e (Lx >> R) of one column; adjacent lanes take adjacent columns
template <int R, bool INV>
__global__ __launch_bounds__(256) void grid_cols_top_kernel(const GridFftArgs a) {
    const int estride = a.Lx >> R;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < estride Ly (a multiple of 256)
    const int pos0 = (int)(id / a.Ly), j = (int)(id - (size_t)pos0 * a.Ly);
    d2 *g = a.planes + blockIdx.y * a.plane_stride + (size_t)pos0 * a.Ly + j;
    const size_t step = (size_t)estride * a.Ly;
    d2 v[1 << R];
#pragma unroll
    for (int e = 0; e < (1 << R); ++e) v[e] = g[e * step];
    stage_group<R, INV>(v, a.tw, a.Lx, a.Lx, pos0, estride);
#pragma unroll
    for (int e = 0; e < (1 << R); ++e) g[e * step] = v[e];
}

// the R stages of block size Ly ... Ly >> (R - 1) along y of the rows [0, rows), without LDS: a thread holds the 2^R
// elements pos0 + e (Ly >> R) of one row; adjacent lanes take adjacent pos0 (a wave reads 1 KiB contiguous per element)
template <int R, bool INV>
__global__ __launch_bounds__(256) void grid_rows_top_kernel(const GridFftArgs a) {
    const int estride = a.Ly >> R;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < rows estride (estride: a multiple of 256)
    const int row = (int)(id / estride), pos0 = (int)(id - (size_t)row * estride);
    d2 *g = a.planes + blockIdx.y * a.plane_stride + (size_t)row * a.Ly + pos0;
    d2 v[1 << R];
#pragma unroll
    for (int e = 0; e < (1 << R); ++e) v[e] = g[(size_t)e * estride];
    stage_group<R, INV>(v, a.tw, a.Ly, a.Ly, pos0, estride);
#pragma unroll
    for (int e = 0; e < (1 << R); ++e) g[(size_t)e * estride] = v[e];
}

// block blockIdx.x of per_wg elements of the rows [0, rows) of plane blockIdx.y along y (the blocks of a plane's leading
// rows are contiguous: block b of row r starts at (r Ly / per_wg + b) per_wg): the stages of block size per_wg and below
template <bool INV>
__global__ __launch_bounds__(1024) void grid_rows_block_kernel(const GridFftArgs a) {
    extern __shared__ __align__(16) unsigned char grid_lds_raw[];
    d2 *s = reinterpret_cast<d2 *>(grid_lds_raw);
    const int len = a.per_wg;
    d2 *g = a.planes + blockIdx.y * a.plane_stride + (size_t)blockIdx.x * len;
    for (int p = threadIdx.x; p < len; p += blockDim.x) s[grid_lds_slot(p)] = g[p];
    __syncthreads();
    lds_stages<INV>(s, 1, len, grid_lds_seq(len), a.tw, a.Ly);
    for (int p = threadIdx.x; p < len; p += blockDim.x) g[p] = s[grid_lds_slot(p)];
}

template <typename Kern>
static int big_lds(Kern kern, bool &done) {
    if (!done) {
        ML_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        done = true;
    }
    return ML_OK;
}

template <bool INV>
static int fft_rows_top(ml_ctx *ctx, const GridFftArgs &a, int n_planes, int R) {   // R = 1, 2
    const dim3 grid((unsigned)(((size_t)a.rows * (a.Ly >> R)) / 256), n_planes);
    if (R == 1)
        hipLaunchKernelGGL((grid_rows_top_kernel<1, INV>), grid, dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((grid_rows_top_kernel<2, INV>), grid, dim3(256), 0, ctx->stream, a);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

// a row longer than GRID_L_MAX: the top stages streaming, blocks of the row in the LDS (grid_axis_route)
template <bool INV>
static int fft_rows_long(ml_ctx *ctx, GridFftArgs a, int n_planes) {
    static bool attr_done = false;   // per instantiation
    ML_TRY(big_lds(grid_rows_block_kernel<INV>, attr_done));
    // (diagnostic build: ML_GRID_ROW_BLOCK=8192 takes whole blocks of GRID_L_MAX, one stage streaming, for timing)
    const bool whole = diag_int("ML_GRID_ROW_BLOCK", GRID_ROW_BLOCK) == GRID_L_MAX;
    const GridAxisRoute r = grid_axis_route(a.Ly, false, whole ? GRID_L_MAX : GRID_ROW_BLOCK);
    a.per_wg = r.lds_len;
    if (!INV) ML_TRY(fft_rows_top<INV>(ctx, a, n_planes, r.top_stages));
    const size_t lds = (size_t)grid_lds_seq(a.per_wg) * sizeof(d2);
    hipLaunchKernelGGL(grid_rows_block_kernel<INV>, dim3((unsigned)((size_t)a.rows * (a.Ly / a.per_wg)), n_planes),
                       dim3(std::min(1024, a.per_wg / 8)), lds, ctx->stream, a);
    ML_HIP(hipGetLastError());
    if (INV) ML_TRY(fft_rows_top<INV>(ctx, a, n_planes, r.top_stages));
    return ML_OK;
}

// `planes` planes along y, rows [0, rows)
template <bool INV>
static int fft_rows(ml_ctx *ctx, d2 *planes, int n_planes, int rows) {
    const PropagatePlan &pp = ctx->prop;
    static bool attr_done = false;   // per instantiation
    ML_TRY(big_lds(grid_rows_kernel<INV>, attr_done));
    GridFftArgs a;
    a.planes = planes;
    a.plane_stride = (size_t)pp.grid.Lx * pp.grid.Ly;
    a.tw = pp.grid_tw_y.as<d2>();
    a.Lx = pp.grid.Lx;
    a.Ly = pp.grid.Ly;
    a.rows = rows;
    if (a.Ly > GRID_L_MAX) return fft_rows_long<INV>(ctx, a, n_planes);
    a.per_wg = std::max(1, 2048 / a.Ly);
    const int elems = a.per_wg * a.Ly, threads = std::min(1024, std::max(256, elems / 8));
    const size_t lds = (size_t)a.per_wg * grid_lds_seq(a.Ly) * sizeof(d2);
    hipLaunchKernelGGL(grid_rows_kernel<INV>, dim3((rows + a.per_wg - 1) / a.per_wg, n_planes), dim3(threads), lds,
                       ctx->stream, a);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

template <bool INV>
static int fft_cols_lds(ml_ctx *ctx, GridFftArgs a, int n_planes) {
    static bool attr_done = false;   // per instantiation
    ML_TRY(big_lds(grid_cols_kernel<INV>, attr_done));
    const int threads = std::min(1024, std::max(64, a.per_wg));
    const size_t lds = (size_t)GRID_COLS * grid_lds_seq(a.per_wg) * sizeof(d2);
    hipLaunchKernelGGL(grid_cols_kernel<INV>, dim3(a.Ly / GRID_COLS, a.Lx / a.per_wg, n_planes), dim3(threads), lds,
                       ctx->stream, a);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

template <bool INV>
static int fft_cols_top(ml_ctx *ctx, const GridFftArgs &a, int n_planes) {
    const int R = grid_log2(a.Lx / a.per_wg);   // 1 ... 3; 4: Lx = 16384 of the long plan
    const dim3 grid((unsigned)(((size_t)(a.Lx >> R) * a.Ly) / 256), n_planes);
    if (R == 1)
        hipLaunchKernelGGL((grid_cols_top_kernel<1, INV>), grid, dim3(256), 0, ctx->stream, a);
    else if (R == 2)
        hipLaunchKernelGGL((grid_cols_top_kernel<2, INV>), grid, dim3(256), 0, ctx->stream, a);
    else if (R == 3)
        hipLaunchKernelGGL((grid_cols_top_kernel<3, INV>), grid, dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((grid_cols_top_kernel<4, INV>), grid, dim3(256), 0, ctx->stream, a);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

// `planes` planes along x, every column
template <bool INV>
static int fft_cols(ml_ctx *ctx, d2 *planes, int n_planes) {
    const PropagatePlan &pp = ctx->prop;
    GridFftArgs a;
    a.planes = planes;
    a.plane_stride = (size_t)pp.grid.Lx * pp.grid.Ly;
    a.tw = pp.grid_tw_x.as<d2>();
    a.Lx = pp.grid.Lx;
    a.Ly = pp.grid.Ly;
    a.rows = a.Lx;
    const GridAxisRoute r = grid_axis_route(a.Lx, true);
    a.per_wg = r.lds_len;
    const bool top = r.top_stages > 0;
    if (top && !INV) ML_TRY(fft_cols_top<INV>(ctx, a, n_planes));
    ML_TRY(fft_cols_lds<INV>(ctx, a, n_planes));
    if (top && INV) ML_TRY(fft_cols_top<INV>(ctx, a, n_planes));
    return ML_OK;
}

int grid_fft_rows(ml_ctx *ctx, double2 *planes, int n_planes, int rows, bool inverse) {
    return inverse ? fft_rows<true>(ctx, planes, n_planes, rows) : fft_rows<false>(ctx, planes, n_planes, rows);
}

int grid_fft_cols(ml_ctx *ctx, double2 *planes, int n_planes, bool inverse) {
    return inverse ? fft_cols<true>(ctx, planes, n_planes) : fft_cols<false>(ctx, planes, n_planes);
}

static int upload_twiddles(ml_ctx *ctx, DevBuf &buf, int L) {
    const std::vector<double> t = grid_twiddles(L);
    ML_TRY(buf.reserve(t.size() * sizeof(double)));
    ML_HIP(hipMemcpyAsync(buf.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));   // (`t` goes away)
    return ML_OK;
}

int grid_upload_twiddles(ml_ctx *ctx) {
    PropagatePlan &pp = ctx->prop;
    ML_TRY(upload_twiddles(ctx, pp.grid_tw_x, pp.grid.Lx));
    return upload_twiddles(ctx, pp.grid_tw_y, pp.grid.Ly);
}

}  // namespace ml
