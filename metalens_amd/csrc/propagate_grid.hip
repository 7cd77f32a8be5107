// The finite-distance propagator for a tensor grid of targets on the aperture's own pitch, as an FFT convolution
// (ml_propagate_plan_grid; plan arithmetic: propagate_grid.h).  fp64 throughout, no atomics.
//
// With the notation of propagate.hip - R = r - r', q = 1 / (k R), w = e^{i k R} / (k R), a = 1 + i q - q^2,
// b = 1 + 3 i q - 3 q^2, u = Rhat, m = M / Z - the braces of its pair sum are linear in the four currents with
// coefficients that depend on the lag (i_t - i_s, j_t - j_s) alone.  Eight kernels:
//   Kxx = i w (a - b ux^2)   Kxy = -i w b ux uy   Kyy = i w (a - b uy^2)   Kzx = -i w b uz ux   Kzy = -i w b uz uy
//   Cx = w (i - q) ux        Cy = w (i - q) uy    Cz = w (i - q) uz
//   E / scale_e:  Ex = Kxx Jx + Kxy Jy + Cz my     Ey = Kxy Jx + Kyy Jy - Cz mx     Ez = Kzx Jx + Kzy Jy + Cy mx - Cx my
//   H / scale_h:  Hx = Kxx mx + Kxy my - Cz Jy     Hy = Kxy mx + Kyy my + Cz Jx     Hz = Kzx mx + Kzy my + Cx Jy - Cy Jx
// each product a convolution over the aperture.  The kernels of a lag (grid_green), a field sample as a current
// (grid_current), this term table (grid_products) and the scaled store of a target (grid_store_scaled) are stated once,
// in propagate_grid_dev.h; the kernels below find the lag, the sample and the pointer and call them.
//
// A pass: pad the four currents of a set into Lx x Ly planes (zeros outside the aperture and outside the row extents
// of a synthesised field), transform them, contract bin by bin with the eight kernel spectra into 6 (3) output
// spectra, transform back, crop [0, mx) x [0, my) into the result with the direct path's scales times 1 / (Lx Ly) (a
// power of two).  The sets of a pass run one after another through the same launches: a set has the bits of that set
// propagated alone, and every operation is linear in the fields, so a field times two gives the output times two.
//
// The transform (propagate_grid.h): radix-2 stages, decimation in frequency forward and in time back, no reordering;
// up to three stages in registers per exchange.  Twiddles from the host's table (long double, rounded once).
//   rows:    contiguous along y, a whole row (or several short ones) per workgroup in the LDS;
//   columns: GRID_COLS = 8 adjacent columns per workgroup - every global access is 128 contiguous bytes - with blocks
//            of up to 1024 elements in the LDS; the stages above 1024 in a streaming pass (8 elements per thread, a
//            wave reads 1 KiB contiguous per element).
// Rows that are zero are not transformed: the forward row pass takes the nx aperture rows, the inverse row pass the mx
// target rows (launch arguments; the column passes take every column).
// The long plan (ml_propagate_plan_grid_long) takes an axis of L = 16384 as well (grid_axis_route):
//   rows:    the stages above a block of GRID_ROW_BLOCK elements in a streaming pass (grid_rows_top_kernel: the
//            L / GRID_ROW_BLOCK elements of one row at that stride per thread, adjacent lanes adjacent elements), the
//            rest on blocks of a row in the LDS (grid_rows_block_kernel);
//   columns: the streaming pass with 16 elements per thread, then the blocks of 1024.
// An axis of L <= 8192 of a long plan goes through the launches above.
// The tiled plan (ml_propagate_plan_grid_tiled) cuts the aperture into tiles, convolves each at a short padded length
// and adds the tiles' products in the spectral domain (overlap-add; the grid_tile_* kernels below, through the same
// transform launches with more planes per launch).
// The fine plan (ml_propagate_plan_grid_fine) puts targets on the pitch divided by (sx, sy): sx sy lattices on the pitch,
// each a tiled convolution of the SAME current spectra with its own kernel spectra (the grid_fine_* kernels).
// The stack plan (ml_propagate_plan_grid_stack) is a fine plan in several planes z; it is planned here, and its pass and
// its fill and scatter kernels are in propagate_stack.hip, which reaches the transform and contraction launchers of this
// file, the currents of a batch of tiles (grid_tile_currents) and the host helpers through propagate_grid_launch.h.
#include "propagate_grid_dev.h"
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

// the eight kernels at every index of the padded grid: index p holds lag p (p < m) or p - L (GridGeoArgs:
// propagate_grid_launch.h)
__global__ __launch_bounds__(256) void grid_fill_kernel(const GridGeoArgs a) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < Lx Ly (a multiple of 256)
    const int p = (int)(id / a.Ly), r = (int)(id - (size_t)p * a.Ly);
    const int lx = p < a.mx ? p : p - a.Lx, ly = r < a.my ? r : r - a.Ly;
    grid_green(lx, ly, a.dxp, a.dyp, a.tx_off, a.ty_off, a.z, a.k, a.inv_k, a.out + id, a.plane_stride);
}

// current c = blockIdx.y of one field set into its padded plane (grid_current)
__global__ __launch_bounds__(256) void grid_pad_kernel(const d2 *fields, const int *row_first, d2 *cur, size_t plane_stride,
                                                       int nx, int ny, int Lx, int Ly, double Z) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < Lx Ly
    const int i = (int)(id / Ly), j = (int)(id - (size_t)i * Ly);
    const int c = blockIdx.y;
    cur[c * plane_stride + id] = grid_current(fields, row_first, nx, ny, i, j, c, Z);
}

// per bin: the 6 (3) output spectra from the 4 current spectra and the 8 kernel spectra (grid_products); the kernel
// spectra by plain loads, here and not through a function (propagate_grid_dev.h grid_load_kernels)
template <bool WANT_H>
__global__ __launch_bounds__(256) void grid_contract_kernel(const d2 *K, const d2 *cur, d2 *out, size_t ps) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < Lx Ly
    d2 e[6];
    const GridKernels8 k8 = {K[id],          K[ps + id],     K[2 * ps + id], K[3 * ps + id],
                             K[4 * ps + id], K[5 * ps + id], K[6 * ps + id], K[7 * ps + id]};
    grid_products<WANT_H, true>(e, k8, cur[id], cur[ps + id], cur[2 * ps + id], cur[3 * ps + id]);
    out[id] = e[0];
    out[ps + id] = e[1];
    out[2 * ps + id] = e[2];
    if (WANT_H) {
        out[3 * ps + id] = e[3];
        out[4 * ps + id] = e[4];
        out[5 * ps + id] = e[5];
    }
}

// result[component blockIdx.y][i my + j] = scale out[component][i][j], i < mx, j < my
__global__ __launch_bounds__(256) void grid_crop_kernel(const d2 *out, size_t ps, d2 *result, int mx, int my, int Ly,
                                                        double scale_e, double scale_h) {
    const int t = blockIdx.x * 256 + threadIdx.x, T = mx * my;
    if (t >= T) return;
    const int i = t / my, j = t - i * my, m = blockIdx.y;
    grid_store_scaled(&result[(size_t)m * T + t], out[m * ps + (size_t)i * Ly + j], m, scale_e, scale_h);
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

static int upload_twiddles(ml_ctx *ctx, DevBuf &buf, int L) {
    const std::vector<double> t = grid_twiddles(L);
    ML_TRY(buf.reserve(t.size() * sizeof(double)));
    ML_HIP(hipMemcpyAsync(buf.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));   // (`t` goes away)
    return ML_OK;
}

static int grid_cap(int method) { return method == ML_PROPAGATE_FFT_LONG ? GRID_L_LONG_MAX : GRID_L_MAX; }

GridGeoArgs grid_geo(const PropagatePlan &pp, double tx_off, double ty_off, double z) {
    const GridPlanFacts &f = pp.grid;
    const double k = 2.0 * M_PI * pp.n_glass / pp.wavelength;
    return {nullptr, (size_t)f.Lx * f.Ly, f.Lx, f.Ly, f.mx, f.my, tx_off, ty_off, pp.dxp, pp.dyp, z, k, 1.0 / k};
}

GridScales grid_scales(const PropagatePlan &pp, const GridPlanFacts &f, double Z0) {
    const double k = 2.0 * M_PI * pp.n_glass / pp.wavelength, Z = Z0 / pp.n_glass;
    const double scale_h = k * k / (4.0 * M_PI) * pp.dxp * pp.dyp;
    const double inv_n = 1.0 / ((double)f.Lx * (double)f.Ly);   // a power of two
    return {Z, Z * scale_h * inv_n, scale_h * inv_n};
}

void grid_facts_of_tile(GridPlanFacts &f, const GridTilePlan &t, int m_x, int m_y, int64_t workspace_bytes) {
    f = {t.nx, t.ny, m_x, m_y, t.x.L, t.y.L, t.outputs, t.plane_bytes, workspace_bytes};
}

// the workspace and the kernel spectra for the resident field's shape (kept while the shape stays)
static int grid_prepare(ml_ctx *ctx) {
    PropagatePlan &pp = ctx->prop;
    if (pp.spectra_ready && pp.grid.nx == ctx->fields.nx && pp.grid.ny == ctx->fields.ny) return ML_OK;
    pp.spectra_ready = false;
    const int mx = pp.grid.mx, my = pp.grid.my;
    char why[320];
    GridPlanFacts f;
    if (grid_plan_facts(ctx->fields.nx, ctx->fields.ny, mx, my, pp.want_h, &f, why, sizeof why, grid_cap(pp.method)) != 0) {
        set_error("%s", why);
        return ML_EINVAL;
    }
    pp.grid = f;
    ML_TRY(pp.grid_work.reserve((size_t)f.workspace_bytes));
    ML_TRY(upload_twiddles(ctx, pp.grid_tw_x, f.Lx));
    ML_TRY(upload_twiddles(ctx, pp.grid_tw_y, f.Ly));
    GridGeoArgs g = grid_geo(pp, pp.tx_off, pp.ty_off, pp.z);
    g.out = pp.grid_work.as<d2>();
    hipLaunchKernelGGL(grid_fill_kernel, dim3((unsigned)(g.plane_stride / 256)), dim3(256), 0, ctx->stream, g);
    ML_HIP(hipGetLastError());
    ML_TRY(fft_rows<false>(ctx, g.out, GRID_KERNELS, f.Lx));
    ML_TRY(fft_cols<false>(ctx, g.out, GRID_KERNELS));
    pp.spectra_ready = true;
    return ML_OK;
}

// ---- the tiled plan (ml_propagate_plan_grid_tiled; propagate_grid.h GridTilePlan) --------------------------------
// Tile t = a cy + b holds the samples [a Bx, a Bx + Bx) x [b By, b By + By) of the aperture.  Kernel spectra
// [tiles][8][Lx][Ly], kept for the life of the plan; currents [batch][4][Lx][Ly]; outputs [6 or 3][Lx][Ly].  A pass
// takes the tiles in batches through pad - row pass - column pass - contraction; the contraction adds the batch's
// tiles, in ascending order, to the output spectra, which go back through ONE inverse transform after the last batch.

struct GridTileGeoArgs {
    GridGeoArgs g;       // out: the first plane of the launch's first tile
    int tile0, cy;       // the launch's first tile; tiles along y
    int Bx, By;          // samples per tile
};

// the eight kernels of tile tile0 + blockIdx.y at every index of the tile's padded grid: index p holds the lag
// (p < m ? p : p - L) - a B, which goes into grid_green as grid_fill_kernel's lag does
__global__ __launch_bounds__(256) void grid_tile_fill_kernel(const GridTileGeoArgs t) {
    const GridGeoArgs &a = t.g;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < Lx Ly (a multiple of 256)
    const int tile = t.tile0 + blockIdx.y, ta = tile / t.cy, tb = tile - ta * t.cy;
    const int p = (int)(id / a.Ly), r = (int)(id - (size_t)p * a.Ly);
    const int lx = (p < a.mx ? p : p - a.Lx) - ta * t.Bx, ly = (r < a.my ? r : r - a.Ly) - tb * t.By;
    grid_green(lx, ly, a.dxp, a.dyp, a.tx_off, a.ty_off, a.z, a.k, a.inv_k,
               a.out + (size_t)blockIdx.y * GRID_KERNELS * a.plane_stride + id, a.plane_stride);
}

struct GridTilePadArgs {
    const d2 *fields;       // one field set [4][nx][ny]
    const int *row_first;   // of a synthesised field, or NULL
    d2 *cur;                // [tiles of the launch][4][Lx][Ly]
    size_t plane_stride;
    int nx, ny, Lx, Ly, Bx, By, tile0, cy;
    double Z;
};

// current c = blockIdx.y of tile tile0 + blockIdx.z into its padded plane (grid_current): zeros beyond the tile's samples,
// beyond the aperture and outside the row extents of a synthesised field
__global__ __launch_bounds__(256) void grid_tile_pad_kernel(const GridTilePadArgs a) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < Lx Ly
    const int il = (int)(id / a.Ly), jl = (int)(id - (size_t)il * a.Ly);
    const int tile = a.tile0 + blockIdx.z, ta = tile / a.cy, tb = tile - ta * a.cy;
    const int i = ta * a.Bx + il, j = tb * a.By + jl;
    const int c = blockIdx.y;
    d2 v = make_double2(0.0, 0.0);
    if (il < a.Bx && jl < a.By) v = grid_current(a.fields, a.row_first, a.nx, a.ny, i, j, c, a.Z);
    a.cur[((size_t)blockIdx.z * GRID_CURRENTS + c) * a.plane_stride + id] = v;
}

// the products of one tile: its four currents, its kernel spectra by streaming loads, the term table
template <bool WANT_H, bool START>
__device__ __forceinline__ void tile_products(d2 (&e)[6], const d2 *K, const d2 *cur, size_t ps, size_t id) {
    const GridKernels8 k8 = grid_load_kernels(K, ps, id);
    const d2 Jx = cur[id], Jy = cur[ps + id], mx = cur[2 * ps + id], my = cur[3 * ps + id];
    grid_products<WANT_H, START>(e, k8, Jx, Jy, mx, my);
}

// per bin: the n tiles of a batch (K: the batch's first tile's spectra, cur: its currents) added in ascending order to
// the 6 (3) output spectra, held in registers and written once.  FIRST (the pass' first batch): the sums start from the
// first tile's first product, as grid_contract_kernel's do; otherwise from the stored value.  No atomics.
template <bool WANT_H, bool FIRST>
__global__ __launch_bounds__(256) void grid_tile_contract_kernel(const d2 *K, const d2 *cur, d2 *out, size_t ps, int n) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < Lx Ly
    constexpr int NC = WANT_H ? 6 : 3;
    d2 e[6];
    int g = 0;
    if (FIRST) {
        tile_products<WANT_H, true>(e, K, cur, ps, id);
        g = 1;
    } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) e[c] = out[c * ps + id];
    }
    for (; g < n; ++g)
        tile_products<WANT_H, false>(e, K + (size_t)g * GRID_KERNELS * ps, cur + (size_t)g * GRID_CURRENTS * ps, ps, id);
#pragma unroll
    for (int c = 0; c < NC; ++c) out[c * ps + id] = e[c];
}

// (diagnostic build: ML_GRID_TILE_BATCH_MIB sets the bytes a batch's currents may take, for timing)
static int64_t tile_batch_bytes() { return (int64_t)diag_int("ML_GRID_TILE_BATCH_MIB", (int)(GRID_TILE_BATCH_BYTES >> 20)) << 20; }

// the workspace and every tile's kernel spectra for the resident field's shape (kept while the shape stays)
static int tile_prepare(ml_ctx *ctx) {
    PropagatePlan &pp = ctx->prop;
    if (pp.spectra_ready && pp.grid.nx == ctx->fields.nx && pp.grid.ny == ctx->fields.ny) return ML_OK;
    pp.spectra_ready = false;
    char why[400];
    GridTilePlan t;
    if (grid_tile_plan(ctx->fields.nx, ctx->fields.ny, pp.grid.mx, pp.grid.my, pp.want_h, pp.tile_lx, pp.tile_ly,
                       tile_batch_bytes(), &t, why, sizeof why) != 0) {
        set_error("%s", why);
        return ML_EINVAL;
    }
    pp.tile = t;
    GridPlanFacts &f = pp.grid;
    grid_facts_of_tile(f, t, f.mx, f.my, t.workspace_bytes);
    ML_TRY(pp.grid_work.reserve((size_t)t.workspace_bytes));
    ML_TRY(upload_twiddles(ctx, pp.grid_tw_x, f.Lx));
    ML_TRY(upload_twiddles(ctx, pp.grid_tw_y, f.Ly));
    GridTileGeoArgs a;
    GridGeoArgs &g = a.g = grid_geo(pp, pp.tx_off, pp.ty_off, pp.z);
    a.cy = t.y.c;
    a.Bx = t.x.B;
    a.By = t.y.B;
    for (int tile0 = 0; tile0 < t.tiles; tile0 += GRID_TILE_BATCH_MAX) {   // 512 planes per launch at the most
        const int nt = std::min(GRID_TILE_BATCH_MAX, t.tiles - tile0);
        a.tile0 = tile0;
        g.out = pp.grid_work.as<d2>() + (size_t)tile0 * GRID_KERNELS * g.plane_stride;
        hipLaunchKernelGGL(grid_tile_fill_kernel, dim3((unsigned)(g.plane_stride / 256), nt), dim3(256), 0, ctx->stream, a);
        ML_HIP(hipGetLastError());
        ML_TRY(fft_rows<false>(ctx, g.out, nt * GRID_KERNELS, f.Lx));
        ML_TRY(fft_cols<false>(ctx, g.out, nt * GRID_KERNELS));
    }
    pp.spectra_ready = true;
    return ML_OK;
}

template <bool WANT_H>
static void launch_tile_contract(ml_ctx *ctx, unsigned blocks, bool first, const d2 *K, const d2 *cur, d2 *out, size_t ps, int n) {
    if (first)
        hipLaunchKernelGGL((grid_tile_contract_kernel<WANT_H, true>), dim3(blocks), dim3(256), 0, ctx->stream, K, cur, out, ps, n);
    else
        hipLaunchKernelGGL((grid_tile_contract_kernel<WANT_H, false>), dim3(blocks), dim3(256), 0, ctx->stream, K, cur, out, ps, n);
}

// the currents of the tiles [tile0, tile0 + nt) of the active plan (pp.tile, pp.grid) and their forward transforms: what the
// tiled, the fine and the stack pass do with a batch of tiles of a field set
int grid_tile_currents(ml_ctx *ctx, const double2 *fields, double Z, double2 *cur, int tile0, int nt, int rows_fwd) {
    const PropagatePlan &pp = ctx->prop;
    const GridPlanFacts &f = pp.grid;
    const GridTilePlan &t = pp.tile;
    const int *row_first = ctx->caches.rows_describe_fields ? ctx->grid.row_first.as<int>() : (const int *)nullptr;
    const GridTilePadArgs p = {fields, row_first, cur, (size_t)f.Lx * f.Ly, t.nx, t.ny, f.Lx, f.Ly, t.x.B, t.y.B, tile0, t.y.c, Z};
    hipLaunchKernelGGL(grid_tile_pad_kernel, dim3((unsigned)(p.plane_stride / 256), GRID_CURRENTS, nt), dim3(256), 0, ctx->stream, p);
    ML_HIP(hipGetLastError());
    ML_TRY(fft_rows<false>(ctx, cur, nt * GRID_CURRENTS, rows_fwd));
    return fft_cols<false>(ctx, cur, nt * GRID_CURRENTS);
}

static int propagate_tile_sets(ml_ctx *ctx, double Z0, int first, int n) {
    PropagatePlan &pp = ctx->prop;
    pp.have_result = false;
    ML_TRY(tile_prepare(ctx));
    const GridPlanFacts &f = pp.grid;
    const GridTilePlan &t = pp.tile;
    const int T = pp.T, nc = f.outputs;
    ML_TRY(pp.result.reserve((size_t)n * nc * T * sizeof(d2)));
    const size_t ps = (size_t)f.Lx * f.Ly;
    d2 *K = pp.grid_work.as<d2>(), *cur = K + (size_t)t.tiles * GRID_KERNELS * ps, *out = cur + (size_t)t.batch * GRID_CURRENTS * ps;
    const GridScales sc = grid_scales(pp, f, Z0);
    const unsigned blocks = (unsigned)(ps / 256);
    const int rows_fwd = std::min(t.x.B, t.nx);   // the rows below hold no sample of any tile
    for (int m = 0; m < n; ++m) {
        const d2 *fields = ctx->fields.buf.as<d2>() + (size_t)(first + m) * 4 * t.nx * t.ny;
        for (int tile0 = 0; tile0 < t.tiles; tile0 += t.batch) {
            const int nt = std::min(t.batch, t.tiles - tile0);
            ML_TRY(grid_tile_currents(ctx, fields, sc.Z, cur, tile0, nt, rows_fwd));
            const d2 *Kt = K + (size_t)tile0 * GRID_KERNELS * ps;
            if (pp.want_h)
                launch_tile_contract<true>(ctx, blocks, tile0 == 0, Kt, cur, out, ps, nt);
            else
                launch_tile_contract<false>(ctx, blocks, tile0 == 0, Kt, cur, out, ps, nt);
            ML_HIP(hipGetLastError());
        }
        ML_TRY(fft_cols<true>(ctx, out, nc));
        ML_TRY(fft_rows<true>(ctx, out, nc, f.mx));
        hipLaunchKernelGGL(grid_crop_kernel, dim3((T + 255) / 256, nc), dim3(256), 0, ctx->stream, out, ps,
                           pp.result.as<d2>() + (size_t)m * nc * T, f.mx, f.my, f.Ly, sc.scale_e, sc.scale_h);
        ML_HIP(hipGetLastError());
    }
    pp.have_result = true;
    pp.result_sets = n;
    return ML_OK;
}

// ---- the fine plan (ml_propagate_plan_grid_fine; propagate_grid.h GridFinePlan) ----------------------------------
// Targets on the aperture's pitch divided by (sx, sy): Ax Ay lattices on the pitch, lattice l = a Ay + b with the origin
// (fine_tx[a], fine_ty[b]), all on the tiled plan of (nx, ny, m_cx, m_cy).  Current spectra [tiles][4][Lx][Ly], padded
// and transformed once per field set in the batches of the tiled plan and kept for the pass; kernel spectra
// [lattices][tiles][8] kept for the life of the plan (cache_kernels), or [2][batch][8] filled and transformed in every
// pass; outputs [2][6 or 3].  Then lattice by lattice, in pairs (a single one last if Ax Ay is odd): contraction over
// all tiles in ascending order, ONE inverse transform of the pair's planes, scatter into the interleaved result.

// the products of one tile and one lattice from currents already loaded
template <bool WANT_H, bool START>
__device__ __forceinline__ void fine_products(d2 (&e)[6], const d2 *K, size_t ps, size_t id, d2 Jx, d2 Jy, d2 mx, d2 my) {
    grid_products<WANT_H, START>(e, grid_load_kernels(K, ps, id), Jx, Jy, mx, my);
}

// per bin: the n tiles of a launch (cur: the first one's currents) added in ascending order to the 6 (3) output spectra
// of G lattices - K: the first tile's spectra of the first lattice, those of the second k_lattice elements behind; out:
// [G][6 or 3] planes.  The four currents of a tile are loaded once for the G lattices; per lattice the sums are those of
// grid_tile_contract_kernel, bit for bit (FIRST as there).  Sums in registers, no atomics.
template <bool WANT_H, bool FIRST, int G>
__global__ __launch_bounds__(256) void grid_fine_contract_kernel(const d2 *K, size_t k_lattice, const d2 *cur, d2 *out, size_t ps,
                                                                 int n) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < Lx Ly
    constexpr int NC = WANT_H ? 6 : 3;
    d2 e[G][6];
    int g = 0;
    if (FIRST) {
        const d2 Jx = cur[id], Jy = cur[ps + id], mx = cur[2 * ps + id], my = cur[3 * ps + id];
#pragma unroll
        for (int l = 0; l < G; ++l) fine_products<WANT_H, true>(e[l], K + l * k_lattice, ps, id, Jx, Jy, mx, my);
        g = 1;
    } else {
#pragma unroll
        for (int l = 0; l < G; ++l)
#pragma unroll
            for (int c = 0; c < NC; ++c) e[l][c] = out[(l * NC + c) * ps + id];
    }
    for (; g < n; ++g) {
        const d2 *ct = cur + (size_t)g * GRID_CURRENTS * ps;
        const d2 Jx = ct[id], Jy = ct[ps + id], mx = ct[2 * ps + id], my = ct[3 * ps + id];
#pragma unroll
        for (int l = 0; l < G; ++l)
            fine_products<WANT_H, false>(e[l], K + l * k_lattice + (size_t)g * GRID_KERNELS * ps, ps, id, Jx, Jy, mx, my);
    }
#pragma unroll
    for (int l = 0; l < G; ++l)
#pragma unroll
        for (int c = 0; c < NC; ++c) out[(l * NC + c) * ps + id] = e[l][c];
}

struct GridFineScatterArgs {
    const d2 *out;          // [lattices of the launch][nc][Lx][Ly]
    d2 *result;             // [nc][mx my] of one field set
    size_t plane_stride;
    int nc, Ly;
    int m_cx, m_cy;         // targets per lattice as planned
    int mx, my, sx, sy;     // fine targets, pitch ratios
    int a[GRID_FINE_PAIR], b[GRID_FINE_PAIR];   // the lattices of the launch
    double scale_e, scale_h;
};

// lattice (a, b) = blockIdx.z of the launch, component blockIdx.y: result[component][(a + sx i) my + b + sy j] = scale
// out[component][i][j] (the scales of grid_crop_kernel) for the targets the lattice has - (a + sx i, b + sy j) inside
// mx x my; those of a ragged lattice beyond are dropped
__global__ __launch_bounds__(256) void grid_fine_scatter_kernel(const GridFineScatterArgs s) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= s.m_cx * s.m_cy) return;
    const int i = t / s.m_cy, j = t - i * s.m_cy, m = blockIdx.y, l = blockIdx.z;
    const int fi = s.a[l] + s.sx * i, fj = s.b[l] + s.sy * j;
    if (fi >= s.mx || fj >= s.my) return;
    grid_store_scaled(&s.result[(size_t)m * s.mx * s.my + (size_t)fi * s.my + fj],
                      s.out[((size_t)l * s.nc + m) * s.plane_stride + (size_t)i * s.Ly + j], m, s.scale_e, s.scale_h);
}

// (diagnostic build: ML_GRID_FINE_PAIR=1 contracts one lattice per read of the currents, for timing)
static int fine_pair() { return diag_int("ML_GRID_FINE_PAIR", GRID_FINE_PAIR) == 1 ? 1 : GRID_FINE_PAIR; }

// the eight kernel spectra of the tiles [tile0, tile0 + nt) of lattice (a, b) into K: the fill of a tiled plan whose
// origin is the lattice's, and the forward transform
static int fine_kernels(ml_ctx *ctx, int a, int b, int tile0, int nt, d2 *K) {
    const PropagatePlan &pp = ctx->prop;
    const GridPlanFacts &f = pp.grid;
    const GridTilePlan &t = pp.fine.tile;
    GridTileGeoArgs ta;
    GridGeoArgs &g = ta.g = grid_geo(pp, pp.fine_tx[a], pp.fine_ty[b], pp.z);
    ta.cy = t.y.c;
    ta.Bx = t.x.B;
    ta.By = t.y.B;
    for (int done = 0; done < nt; done += GRID_TILE_BATCH_MAX) {   // 512 planes per launch at the most
        const int now = std::min(GRID_TILE_BATCH_MAX, nt - done);
        ta.tile0 = tile0 + done;
        g.out = K + (size_t)done * GRID_KERNELS * g.plane_stride;
        hipLaunchKernelGGL(grid_tile_fill_kernel, dim3((unsigned)(g.plane_stride / 256), now), dim3(256), 0, ctx->stream, ta);
        ML_HIP(hipGetLastError());
        ML_TRY(fft_rows<false>(ctx, g.out, now * GRID_KERNELS, f.Lx));
        ML_TRY(fft_cols<false>(ctx, g.out, now * GRID_KERNELS));
    }
    return ML_OK;
}

// the plan and the workspace for the resident field's shape and, with cache_kernels, every lattice's kernel spectra
// (kept while the shape stays)
static int fine_prepare(ml_ctx *ctx) {
    PropagatePlan &pp = ctx->prop;
    if (pp.spectra_ready && pp.grid.nx == ctx->fields.nx && pp.grid.ny == ctx->fields.ny) return ML_OK;
    pp.spectra_ready = false;
    char why[480];
    GridFinePlan p;
    if (grid_fine_plan(ctx->fields.nx, ctx->fields.ny, pp.fine.mx, pp.fine.my, pp.fine.sx, pp.fine.sy, pp.want_h, pp.tile_lx,
                       pp.tile_ly, pp.fine.cache_kernels, tile_batch_bytes(), &p, why, sizeof why) != 0) {
        set_error("%s", why);
        return ML_EINVAL;
    }
    pp.fine = p;
    const GridTilePlan &t = pp.tile = p.tile;
    GridPlanFacts &f = pp.grid;
    grid_facts_of_tile(f, t, p.m_cx, p.m_cy, p.workspace_bytes);
    if (pp.grid_work.reserve((size_t)p.workspace_bytes) != ML_OK) {
        if (p.cache_kernels) {
            GridFinePlan streamed;
            grid_fine_plan(t.nx, t.ny, p.mx, p.my, p.sx, p.sy, pp.want_h, pp.tile_lx, pp.tile_ly, 0, tile_batch_bytes(), &streamed,
                           why, sizeof why);
            set_error("the fine FFT form keeps the kernel spectra of %d x %d lattices and %d tiles: the device did not give the "
                      "%lld bytes of its workspace; cache_kernels=0 fills them in every pass and takes %lld bytes",
                      p.ax, p.ay, t.tiles, (long long)p.workspace_bytes, (long long)streamed.workspace_bytes);
        } else {
            set_error("the fine FFT form: the device did not give the %lld bytes of its workspace (%d tiles; the current spectra "
                      "of all tiles are kept for a pass)", (long long)p.workspace_bytes, t.tiles);
        }
        return ML_ENOMEM;
    }
    ML_TRY(upload_twiddles(ctx, pp.grid_tw_x, f.Lx));
    ML_TRY(upload_twiddles(ctx, pp.grid_tw_y, f.Ly));
    if (p.cache_kernels) {
        const size_t per_lattice = (size_t)t.tiles * GRID_KERNELS * f.Lx * f.Ly;
        for (int l = 0; l < p.ax * p.ay; ++l)
            ML_TRY(fine_kernels(ctx, l / p.ay, l % p.ay, 0, t.tiles, pp.grid_work.as<d2>() + l * per_lattice));
    }
    pp.spectra_ready = true;
    return ML_OK;
}

template <bool WANT_H, int G>
static void launch_fine_contract(ml_ctx *ctx, unsigned blocks, bool first, const d2 *K, size_t k_lattice, const d2 *cur, d2 *out,
                                 size_t ps, int n) {
    if (first)
        hipLaunchKernelGGL((grid_fine_contract_kernel<WANT_H, true, G>), dim3(blocks), dim3(256), 0, ctx->stream, K, k_lattice, cur,
                           out, ps, n);
    else
        hipLaunchKernelGGL((grid_fine_contract_kernel<WANT_H, false, G>), dim3(blocks), dim3(256), 0, ctx->stream, K, k_lattice, cur,
                           out, ps, n);
}

// the tiles [tile0, tile0 + n) into the output spectra of `lattices` (1 or 2) lattices
static int fine_contract(ml_ctx *ctx, int lattices, unsigned blocks, bool first, const d2 *K, size_t k_lattice, const d2 *cur,
                         d2 *out, size_t ps, int n) {
    const bool h = ctx->prop.want_h;
    if (lattices == 2)
        h ? launch_fine_contract<true, 2>(ctx, blocks, first, K, k_lattice, cur, out, ps, n)
          : launch_fine_contract<false, 2>(ctx, blocks, first, K, k_lattice, cur, out, ps, n);
    else
        h ? launch_fine_contract<true, 1>(ctx, blocks, first, K, k_lattice, cur, out, ps, n)
          : launch_fine_contract<false, 1>(ctx, blocks, first, K, k_lattice, cur, out, ps, n);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

static int propagate_fine_sets(ml_ctx *ctx, double Z0, int first, int n) {
    PropagatePlan &pp = ctx->prop;
    pp.have_result = false;
    ML_TRY(fine_prepare(ctx));
    const GridPlanFacts &f = pp.grid;
    const GridFinePlan &fp = pp.fine;
    const GridTilePlan &t = fp.tile;
    const int T = pp.T, nc = f.outputs, lattices = fp.ax * fp.ay, pair = fine_pair();
    ML_TRY(pp.result.reserve((size_t)n * nc * T * sizeof(d2)));
    const size_t ps = (size_t)f.Lx * f.Ly;
    // cached: [lattices][tiles][8]; streamed: [2][batch][8]
    const size_t k_lattice = (size_t)(fp.cache_kernels ? t.tiles : t.batch) * GRID_KERNELS * ps;
    d2 *K = pp.grid_work.as<d2>(), *cur = K + (size_t)(fp.cache_kernels ? lattices : GRID_FINE_PAIR) * k_lattice;
    d2 *out = cur + (size_t)t.tiles * GRID_CURRENTS * ps;
    const GridScales sc = grid_scales(pp, f, Z0);
    const unsigned blocks = (unsigned)(ps / 256);
    const int rows_fwd = std::min(t.x.B, t.nx);   // the rows below hold no sample of any tile
    GridFineScatterArgs s;
    s.out = out;
    s.plane_stride = ps;
    s.nc = nc;
    s.Ly = f.Ly;
    s.m_cx = fp.m_cx;
    s.m_cy = fp.m_cy;
    s.mx = fp.mx;
    s.my = fp.my;
    s.sx = fp.sx;
    s.sy = fp.sy;
    s.scale_e = sc.scale_e;
    s.scale_h = sc.scale_h;
    for (int m = 0; m < n; ++m) {
        const d2 *fields = ctx->fields.buf.as<d2>() + (size_t)(first + m) * 4 * t.nx * t.ny;
        for (int tile0 = 0; tile0 < t.tiles; tile0 += t.batch)   // the current spectra of every tile, once per set
            ML_TRY(grid_tile_currents(ctx, fields, sc.Z, cur + (size_t)tile0 * GRID_CURRENTS * ps, tile0,
                                      std::min(t.batch, t.tiles - tile0), rows_fwd));
        s.result = pp.result.as<d2>() + (size_t)m * nc * T;
        for (int l0 = 0; l0 < lattices; l0 += pair) {
            const int nl = std::min(pair, lattices - l0);
            for (int l = 0; l < nl; ++l) {
                s.a[l] = (l0 + l) / fp.ay;
                s.b[l] = (l0 + l) % fp.ay;
            }
            if (fp.cache_kernels) {
                ML_TRY(fine_contract(ctx, nl, blocks, true, K + (size_t)l0 * k_lattice, k_lattice, cur, out, ps, t.tiles));
            } else {
                for (int tile0 = 0; tile0 < t.tiles; tile0 += t.batch) {
                    const int nt = std::min(t.batch, t.tiles - tile0);
                    for (int l = 0; l < nl; ++l) ML_TRY(fine_kernels(ctx, s.a[l], s.b[l], tile0, nt, K + l * k_lattice));
                    ML_TRY(fine_contract(ctx, nl, blocks, tile0 == 0, K, k_lattice, cur + (size_t)tile0 * GRID_CURRENTS * ps, out, ps,
                                         nt));
                }
            }
            ML_TRY(fft_cols<true>(ctx, out, nl * nc));
            ML_TRY(fft_rows<true>(ctx, out, nl * nc, fp.m_cx));
            hipLaunchKernelGGL(grid_fine_scatter_kernel, dim3((fp.m_cx * fp.m_cy + 255) / 256, nc, nl), dim3(256), 0, ctx->stream, s);
            ML_HIP(hipGetLastError());
        }
    }
    pp.have_result = true;
    pp.result_sets = n;
    return ML_OK;
}

int propagate_grid_sets(ml_ctx *ctx, double Z0, int first, int n) {
    PropagatePlan &pp = ctx->prop;
    if (pp.method == ML_PROPAGATE_FFT_TILED) return propagate_tile_sets(ctx, Z0, first, n);
    if (pp.method == ML_PROPAGATE_FFT_FINE) return propagate_fine_sets(ctx, Z0, first, n);
    if (pp.method == ML_PROPAGATE_FFT_STACK) return propagate_stack_sets(ctx, Z0, first, n);
    pp.have_result = false;
    ML_TRY(grid_prepare(ctx));
    const GridPlanFacts &f = pp.grid;
    const int T = pp.T, nc = f.outputs;
    ML_TRY(pp.result.reserve((size_t)n * nc * T * sizeof(d2)));
    const size_t ps = (size_t)f.Lx * f.Ly;
    d2 *K = pp.grid_work.as<d2>(), *cur = K + GRID_KERNELS * ps, *out = cur + GRID_CURRENTS * ps;
    const GridScales sc = grid_scales(pp, f, Z0);
    const unsigned blocks = (unsigned)(ps / 256);
    // rows that are zero need no transform (diagnostic build: ML_GRID_ALL_ROWS=1 transforms them all, for timing)
    const bool all_rows = diag_int("ML_GRID_ALL_ROWS", 0) != 0;
    const int rows_fwd = all_rows ? f.Lx : ctx->fields.nx, rows_inv = all_rows ? f.Lx : f.mx;
    for (int m = 0; m < n; ++m) {
        const d2 *fields = ctx->fields.buf.as<d2>() + (size_t)(first + m) * 4 * ctx->fields.nx * ctx->fields.ny;
        hipLaunchKernelGGL(grid_pad_kernel, dim3(blocks, GRID_CURRENTS), dim3(256), 0, ctx->stream, fields,
                           ctx->caches.rows_describe_fields ? ctx->grid.row_first.as<int>() : (const int *)nullptr, cur, ps,
                           ctx->fields.nx, ctx->fields.ny,
                           f.Lx, f.Ly, sc.Z);
        ML_HIP(hipGetLastError());
        ML_TRY(fft_rows<false>(ctx, cur, GRID_CURRENTS, rows_fwd));
        ML_TRY(fft_cols<false>(ctx, cur, GRID_CURRENTS));
        if (pp.want_h)
            hipLaunchKernelGGL(grid_contract_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream, K, cur, out, ps);
        else
            hipLaunchKernelGGL(grid_contract_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, K, cur, out, ps);
        ML_HIP(hipGetLastError());
        ML_TRY(fft_cols<true>(ctx, out, nc));
        ML_TRY(fft_rows<true>(ctx, out, nc, rows_inv));
        hipLaunchKernelGGL(grid_crop_kernel, dim3((T + 255) / 256, nc), dim3(256), 0, ctx->stream, out, ps,
                           pp.result.as<d2>() + (size_t)m * nc * T, f.mx, f.my, f.Ly, sc.scale_e, sc.scale_h);
        ML_HIP(hipGetLastError());
    }
    pp.have_result = true;
    pp.result_sets = n;
    return ML_OK;
}

// what propagate_stack.hip goes through (propagate_grid_launch.h) beside grid_tile_currents and the helpers above
int grid_fft_rows(ml_ctx *ctx, double2 *planes, int n_planes, int rows, bool inverse) {
    return inverse ? fft_rows<true>(ctx, planes, n_planes, rows) : fft_rows<false>(ctx, planes, n_planes, rows);
}
int grid_fft_cols(ml_ctx *ctx, double2 *planes, int n_planes, bool inverse) {
    return inverse ? fft_cols<true>(ctx, planes, n_planes) : fft_cols<false>(ctx, planes, n_planes);
}
int grid_fine_contract(ml_ctx *ctx, int lattices, unsigned blocks, bool first, const double2 *K, size_t k_lattice, const double2 *cur,
                       double2 *out, size_t ps, int n) {
    return fine_contract(ctx, lattices, blocks, first, K, k_lattice, cur, out, ps, n);
}
int grid_upload_twiddles(ml_ctx *ctx, DevBuf &buf, int L) { return upload_twiddles(ctx, buf, L); }
int64_t grid_tile_batch_bytes() { return tile_batch_bytes(); }

}  // namespace ml

using namespace ml;

// what ml_propagate_plan_grid_fine asks for beyond a tiled plan; ml_propagate_plan_grid_stack: and the planes (the `z` of
// plan_grid is then the largest of them, checked by the entry)
struct FineAsk {
    const double *tx_first, *ty_first;   // the first min(s, m) coordinates of each fine axis
    int sx, sy, cache_kernels;
    const double *z = nullptr;           // the planes of a stack, or NULL
    int nz = 0;
};

// the origins of an axis' lattices: strictly ascending within one pitch
static int fine_origins_ok(const char *entry, const char *axis, const double *first, int active, double pitch) {
    for (int a = 1; a < active; ++a)
        ML_REQUIRE(first[a] > first[a - 1], "%s: the %s origins of the lattices must ascend strictly: %s_first[%d] = %.17g is not "
                   "above %s_first[%d] = %.17g", entry, axis, axis, a, first[a], axis, a - 1, first[a - 1]);
    ML_REQUIRE(first[active - 1] - first[0] < pitch, "%s: the %s origins of the lattices must span less than the aperture's pitch "
               "%.17g: %s_first[%d] - %s_first[0] = %.17g", entry, axis, pitch, axis, active - 1, axis, first[active - 1] - first[0]);
    return ML_OK;
}

// every refusal of an entry names it: the name in front of a message that lacks it; -> rc
static int named_refusal(const char *entry, int rc) {
    if (rc != ML_OK && strncmp(ml_last_error(), entry, strlen(entry)) != 0) {
        const std::string said = ml_last_error();
        set_error("%s: %s", entry, said.c_str());
    }
    return rc;
}

// ml_propagate_plan_grid, ml_propagate_plan_grid_long, ml_propagate_plan_grid_tiled, ml_propagate_plan_grid_fine and
// ml_propagate_plan_grid_stack (a fine plan with planes in `fine`; T is then planes x fine targets): `entry`
// is the caller's name, `method` its ML_PROPAGATE_*; tile_lx, tile_ly: the tile lengths of the tiled and the fine plan (0:
// the default); `fine`: of the fine plan, whose mx, my are the FINE targets and tx0, ty0 its first lattice's origin
static int plan_grid(ml_ctx *ctx, const char *entry, int method, double x0, double y0, double dxp, double dyp, double wavelength,
                     double n_glass, double tx0, double ty0, int mx, int my, double z, int want_h, int tile_lx = 0,
                     int tile_ly = 0, const FineAsk *fine = nullptr) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(ctx->n_ranks <= 1, "%s: this context belongs to a communicator of %d ranks; the "
               "finite-distance propagator sums a whole aperture on one GPU (sharded propagation is not implemented)",
               entry, ctx->n_ranks);
    ML_REQUIRE(mx >= 1 && my >= 1, "no targets");
    ML_REQUIRE(wavelength > 0 && n_glass > 0 && dxp > 0 && dyp > 0, "bad geometry");
    ML_REQUIRE(z > 0, "the target plane lies at z = %g: the propagator needs z > 0", z);
    ML_REQUIRE((long long)mx * my <= (1 << 26), "%lld targets: at most 2^26 per plan", (long long)mx * my);
    const bool stack = fine && fine->z;
    std::vector<GridStackLayerRow> layers;   // of a stack: what the device reads per layer
    GridPlanFacts f;
    f.mx = mx;
    f.my = my;
    GridTilePlan tile;
    GridFinePlan fp;
    if (fine) {   // as for the tiled plan below
        char why[480];
        const bool resident = ctx->fields.nx && ctx->fields.ny;
        const int bad = resident ? grid_fine_plan(ctx->fields.nx, ctx->fields.ny, mx, my, fine->sx, fine->sy, want_h, tile_lx, tile_ly,
                                                  fine->cache_kernels, tile_batch_bytes(), &fp, why, sizeof why)
                                 : (grid_fine_check_axis("x", 0, mx, fine->sx, tile_lx, why, sizeof why) ||
                                    grid_fine_check_axis("y", 0, my, fine->sy, tile_ly, why, sizeof why));
        if (bad) {
            set_error("%s: %s", entry, why);
            return ML_EINVAL;
        }
        fp.sx = fine->sx;   // (what was asked for is known without a shape)
        fp.sy = fine->sy;
        fp.mx = mx;
        fp.my = my;
        fp.ax = grid_fine_active(mx, fp.sx);
        fp.ay = grid_fine_active(my, fp.sy);
        fp.m_cx = grid_fine_count(mx, fp.sx);
        fp.m_cy = grid_fine_count(my, fp.sy);
        fp.cache_kernels = fine->cache_kernels != 0;
        ML_TRY(fine_origins_ok(entry, "tx", fine->tx_first, fp.ax, dxp));
        ML_TRY(fine_origins_ok(entry, "ty", fine->ty_first, fp.ay, dyp));
        tile = fp.tile;
        f.mx = fp.m_cx;   // per lattice: what the launches read
        f.my = fp.m_cy;
        f.Lx = resident ? tile.x.L : tile_lx;
        f.Ly = resident ? tile.y.L : tile_ly;
    } else if (method == ML_PROPAGATE_FFT_TILED) {   // what is wrong with the targets or the lengths whatever the shape, and
        char why[400];                        // the plan for the shape a pass would meet now
        const bool resident = ctx->fields.nx && ctx->fields.ny;
        const int bad = resident ? grid_tile_plan(ctx->fields.nx, ctx->fields.ny, mx, my, want_h, tile_lx, tile_ly,
                                                  tile_batch_bytes(), &tile, why, sizeof why)
                                 : (grid_tile_check_axis("x", 0, mx, tile_lx, why, sizeof why) ||
                                    grid_tile_check_axis("y", 0, my, tile_ly, why, sizeof why));
        if (bad) {
            set_error("%s: %s", entry, why);
            return ML_EINVAL;
        }
        f.Lx = resident ? tile.x.L : tile_lx;   // (the lengths asked for are known without a shape)
        f.Ly = resident ? tile.y.L : tile_ly;
    } else if (ctx->fields.nx && ctx->fields.ny) {   // the shape a pass would meet now: refuse here, with the previous plan as it was
        char why[320];
        if (grid_plan_facts(ctx->fields.nx, ctx->fields.ny, mx, my, want_h, &f, why, sizeof why, grid_cap(method)) != 0) {
            set_error("%s: %s", entry, why);
            return ML_EINVAL;
        }
    }
    // the largest lag of the plan bounds k R as the direct plan's bounding box does (propagate.hip): checked against the
    // resident shape here, and by every pass against the shape it meets
    PropExtent ext;
    ext.tx_lo = tx0 - x0;
    ext.tx_hi = ext.tx_lo + (mx - 1) * (dxp / (fine ? fine->sx : 1));
    ext.ty_lo = ty0 - y0;
    ext.ty_hi = ext.ty_lo + (my - 1) * (dyp / (fine ? fine->sy : 1));
    ext.z_hi = z;
    if (ctx->fields.nx && ctx->fields.ny)
        ML_TRY(prop_check_phase(entry, ext, ctx->fields.nx, ctx->fields.ny, dxp, dyp, wavelength, n_glass));
    ML_HIP(hipSetDevice(ctx->device));
    PropagatePlan &pp = ctx->prop;
    if (stack) {   // the layer table, once per plan: layer l = p A + a Ay + b (propagate_grid.h grid_stack_layer)
        layers.resize((size_t)fine->nz * fp.ax * fp.ay);
        for (size_t l = 0; l < layers.size(); ++l) {
            const GridStackLayer s = grid_stack_layer((int)l, fp.ax, fp.ay);
            layers[l] = {fine->tx_first[s.a] - x0, fine->ty_first[s.b] - y0, fine->z[s.p], s.p, s.a, s.b, 0};
        }
        ML_TRY(pp.stack_layers.reserve(layers.size() * sizeof(GridStackLayerRow)));
        ML_HIP(hipMemcpyAsync(pp.stack_layers.p, layers.data(), layers.size() * sizeof(GridStackLayerRow), hipMemcpyHostToDevice,
                              ctx->stream));
        ML_HIP(hipStreamSynchronize(ctx->stream));   // (`layers` goes away)
    }
    pp.ready = pp.have_result = pp.have_sums = false;   // results and sums of the previous plan are gone
    pp.spectra_ready = false;
    pp.method = method;
    pp.extent = ext;
    pp.grid = f;
    pp.tile = tile;
    pp.fine = fp;
    for (int a = 0; a < fp.ax; ++a) pp.fine_tx[a] = fine->tx_first[a] - x0;
    for (int b = 0; b < fp.ay; ++b) pp.fine_ty[b] = fine->ty_first[b] - y0;
    pp.tile_lx = tile_lx;
    pp.tile_ly = tile_ly;
    pp.T = (stack ? fine->nz : 1) * mx * my;
    pp.stack_z.clear();
    if (stack) pp.stack_z.assign(fine->z, fine->z + fine->nz);
    pp.want_h = want_h != 0;
    pp.x0 = x0;
    pp.y0 = y0;
    pp.dxp = dxp;
    pp.dyp = dyp;
    pp.wavelength = wavelength;
    pp.n_glass = n_glass;
    pp.tx_off = tx0 - x0;
    pp.ty_off = ty0 - y0;
    pp.z = z;
    pp.ready = true;
    return ML_OK;
}

extern "C" {

int ml_propagate_plan_grid(ml_ctx *ctx, double x0, double y0, double dxp, double dyp, double wavelength, double n_glass,
                           double tx0, double ty0, int mx, int my, double z, int want_h) {
    return plan_grid(ctx, "ml_propagate_plan_grid", ML_PROPAGATE_FFT, x0, y0, dxp, dyp, wavelength, n_glass, tx0, ty0, mx, my, z,
                     want_h);
}

int ml_propagate_plan_grid_long(ml_ctx *ctx, double x0, double y0, double dxp, double dyp, double wavelength, double n_glass,
                                double tx0, double ty0, int mx, int my, double z, int want_h) {
    return plan_grid(ctx, "ml_propagate_plan_grid_long", ML_PROPAGATE_FFT_LONG, x0, y0, dxp, dyp, wavelength, n_glass, tx0, ty0,
                     mx, my, z, want_h);
}

int ml_propagate_plan_grid_tiled(ml_ctx *ctx, double x0, double y0, double dxp, double dyp, double wavelength, double n_glass,
                                 double tx0, double ty0, int mx, int my, double z, int want_h, int tile_lx, int tile_ly) {
    return plan_grid(ctx, "ml_propagate_plan_grid_tiled", ML_PROPAGATE_FFT_TILED, x0, y0, dxp, dyp, wavelength, n_glass, tx0, ty0,
                     mx, my, z, want_h, tile_lx, tile_ly);
}

int ml_propagate_plan_grid_fine(ml_ctx *ctx, double x0, double y0, double dxp, double dyp, double wavelength, double n_glass,
                                const double *tx_first, int sx, const double *ty_first, int sy, int mx, int my, double z, int want_h,
                                int tile_lx, int tile_ly, int cache_kernels) {
    ML_REQUIRE(tx_first && ty_first, "ml_propagate_plan_grid_fine: NULL argument");
    const FineAsk fine = {tx_first, ty_first, sx, sy, cache_kernels};
    const char *entry = "ml_propagate_plan_grid_fine";
    return named_refusal(entry, plan_grid(ctx, entry, ML_PROPAGATE_FFT_FINE, x0, y0, dxp, dyp, wavelength, n_glass, tx_first[0],
                                          ty_first[0], mx, my, z, want_h, tile_lx, tile_ly, &fine));
}

int ml_propagate_plan_grid_stack(ml_ctx *ctx, double x0, double y0, double dxp, double dyp, double wavelength, double n_glass,
                                 const double *tx_first, int sx, const double *ty_first, int sy, int mx, int my, const double *z,
                                 int nz, int want_h, int tile_lx, int tile_ly, int cache_kernels) {
    const char *entry = "ml_propagate_plan_grid_stack";
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(tx_first && ty_first && z, "%s: NULL argument", entry);
    ML_REQUIRE(mx >= 1 && my >= 1, "%s: no targets", entry);
    char why[480];
    if (grid_stack_check_planes(z, nz, mx, my, why, sizeof why) != 0) {
        set_error("%s: %s", entry, why);
        return ML_EINVAL;
    }
    FineAsk fine = {tx_first, ty_first, sx, sy, cache_kernels};
    fine.z = z;
    fine.nz = nz;
    return named_refusal(entry, plan_grid(ctx, entry, ML_PROPAGATE_FFT_STACK, x0, y0, dxp, dyp, wavelength, n_glass, tx_first[0],
                                          ty_first[0], mx, my, *std::max_element(z, z + nz), want_h, tile_lx, tile_ly, &fine));
}

int ml_propagate_plan_planes(ml_ctx *ctx, int *nz) {
    ML_REQUIRE(ctx, "ctx is NULL");
    const PropagatePlan &pp = ctx->prop;
    if (!pp.ready || pp.method != ML_PROPAGATE_FFT_STACK) {
        set_error("ml_propagate_plan_planes: no stack propagation plan is active");
        return ML_ESTATE;
    }
    if (nz) *nz = (int)pp.stack_z.size();
    return ML_OK;
}

int ml_propagate_plan_lattices(ml_ctx *ctx, int *sx, int *sy, int *mcx, int *mcy, int *cached) {
    ML_REQUIRE(ctx, "ctx is NULL");
    const PropagatePlan &pp = ctx->prop;
    if (!pp.ready || (pp.method != ML_PROPAGATE_FFT_FINE && pp.method != ML_PROPAGATE_FFT_STACK)) {
        set_error("ml_propagate_plan_lattices: no fine propagation plan is active");
        return ML_ESTATE;
    }
    if (sx) *sx = pp.fine.sx;
    if (sy) *sy = pp.fine.sy;
    if (mcx) *mcx = pp.fine.m_cx;
    if (mcy) *mcy = pp.fine.m_cy;
    if (cached) *cached = pp.fine.cache_kernels;
    return ML_OK;
}

int ml_propagate_plan_tiles(ml_ctx *ctx, int *cx, int *cy, int *bx, int *by, int *batch) {
    ML_REQUIRE(ctx, "ctx is NULL");
    const PropagatePlan &pp = ctx->prop;
    if (!pp.ready || (pp.method != ML_PROPAGATE_FFT_TILED && pp.method != ML_PROPAGATE_FFT_FINE && pp.method != ML_PROPAGATE_FFT_STACK)) {
        set_error("ml_propagate_plan_tiles: no tiled propagation plan is active");
        return ML_ESTATE;
    }
    if (cx) *cx = pp.tile.x.c;
    if (cy) *cy = pp.tile.y.c;
    if (bx) *bx = pp.tile.x.B;
    if (by) *by = pp.tile.y.B;
    if (batch) *batch = pp.tile.batch;
    return ML_OK;
}

int ml_propagate_plan_info(ml_ctx *ctx, int *method, int *lx, int *ly, int64_t *workspace_bytes) {
    ML_REQUIRE(ctx, "ctx is NULL");
    const PropagatePlan &pp = ctx->prop;
    if (!pp.ready) {
        set_error("no propagation plan is active");
        return ML_ESTATE;
    }
    const bool fft = pp.method != ML_PROPAGATE_DIRECT;
    if (method) *method = pp.method;
    if (lx) *lx = fft ? pp.grid.Lx : 0;
    if (ly) *ly = fft ? pp.grid.Ly : 0;
    if (workspace_bytes) *workspace_bytes = (int64_t)(fft ? pp.grid_work.bytes : pp.partial.bytes);
    return ML_OK;
}

}  // extern "C"
