// The tiled plan of the FFT form of the finite-distance propagator (ml_propagate_plan_grid_tiled, method 'fft-tiled';
// propagate_grid.h GridTilePlan): its pass, propagate_tile_sets, and what the fine and the stack pass take from it - the
// kernel spectra of a range of tiles for one origin (grid_tile_kernels), the current spectra of a batch of tiles
// (grid_tile_currents) and the bytes of a batch (grid_tile_batch_bytes).  fp64 throughout, no atomics.
//
// The aperture is cut into tiles, each convolved at a short padded length; the tiles' products are added in the spectral
// domain (overlap-add).  Tile t = a cy + b holds the samples [a Bx, a Bx + Bx) x [b By, b By + By) of the aperture.
// Kernel spectra [tiles][8][Lx][Ly], kept for the life of the plan; currents [batch][4][Lx][Ly]; outputs [6 or 3][Lx][Ly]
// (PropagatePlan::grid_work, common.h grid_work_tiled).  A pass takes the tiles in batches through pad - row pass -
// column pass - contraction; the contraction adds the batch's tiles, in ascending order, to the output spectra, which go
// back through ONE inverse transform after the last batch (grid_finish_set, as the plain pass ends).
// The transform: propagate_grid_fft.hip, with the tile lengths in pp.grid and more planes per launch.
#include "propagate_grid_dev.h"
#include "propagate_grid_launch.h"

namespace ml {

typedef double2 d2;

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
int64_t grid_tile_batch_bytes() { return (int64_t)diag_int("ML_GRID_TILE_BATCH_MIB", (int)(GRID_TILE_BATCH_BYTES >> 20)) << 20; }

void grid_facts_of_tile(GridPlanFacts &f, const GridTilePlan &t, int m_x, int m_y, int64_t workspace_bytes) {
    f = {t.nx, t.ny, m_x, m_y, t.x.L, t.y.L, t.outputs, t.plane_bytes, workspace_bytes};
}

int grid_tile_kernels(ml_ctx *ctx, double tx_off, double ty_off, int tile0, int nt, d2 *K) {
    const PropagatePlan &pp = ctx->prop;
    const GridPlanFacts &f = pp.grid;
    const GridTilePlan &t = pp.tile;
    GridTileGeoArgs a;
    GridGeoArgs &g = a.g = grid_geo(pp, tx_off, ty_off, pp.z);
    a.cy = t.y.c;
    a.Bx = t.x.B;
    a.By = t.y.B;
    for (int done = 0; done < nt; done += GRID_TILE_BATCH_MAX) {   // 512 planes per launch at the most
        const int now = std::min(GRID_TILE_BATCH_MAX, nt - done);
        a.tile0 = tile0 + done;
        g.out = K + (size_t)done * GRID_KERNELS * g.plane_stride;
        hipLaunchKernelGGL(grid_tile_fill_kernel, dim3((unsigned)(g.plane_stride / 256), now), dim3(256), 0, ctx->stream, a);
        ML_HIP(hipGetLastError());
        ML_TRY(grid_fft_rows(ctx, g.out, now * GRID_KERNELS, f.Lx, false));
        ML_TRY(grid_fft_cols(ctx, g.out, now * GRID_KERNELS, false));
    }
    return ML_OK;
}

// the workspace and every tile's kernel spectra for the resident field's shape (kept while the shape stays)
static int tile_prepare(ml_ctx *ctx) {
    PropagatePlan &pp = ctx->prop;
    if (grid_spectra_kept(ctx)) return ML_OK;
    char why[400];
    GridTilePlan t;
    if (grid_tile_plan(ctx->fields.nx, ctx->fields.ny, pp.grid.mx, pp.grid.my, pp.want_h, pp.tile_lx, pp.tile_ly,
                       grid_tile_batch_bytes(), &t, why, sizeof why) != 0) {
        set_error("%s", why);
        return ML_EINVAL;
    }
    pp.tile = t;
    grid_facts_of_tile(pp.grid, t, pp.grid.mx, pp.grid.my, t.workspace_bytes);
    ML_TRY(pp.grid_work.reserve((size_t)t.workspace_bytes));
    ML_TRY(grid_upload_twiddles(ctx));
    ML_TRY(grid_tile_kernels(ctx, pp.tx_off, pp.ty_off, 0, t.tiles, grid_work_tiled(pp).K));
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

// (of the active plan: pp.tile, pp.grid - what the tiled, the fine and the stack pass do with a batch of tiles of a set)
int grid_tile_currents(ml_ctx *ctx, const double2 *fields, double Z, double2 *cur, int tile0, int nt, int rows_fwd) {
    const PropagatePlan &pp = ctx->prop;
    const GridPlanFacts &f = pp.grid;
    const GridTilePlan &t = pp.tile;
    const int *row_first = ctx->caches.rows_describe_fields ? ctx->grid.row_first.as<int>() : (const int *)nullptr;
    const GridTilePadArgs p = {fields, row_first, cur, (size_t)f.Lx * f.Ly, t.nx, t.ny, f.Lx, f.Ly, t.x.B, t.y.B, tile0, t.y.c, Z};
    hipLaunchKernelGGL(grid_tile_pad_kernel, dim3((unsigned)(p.plane_stride / 256), GRID_CURRENTS, nt), dim3(256), 0, ctx->stream, p);
    ML_HIP(hipGetLastError());
    ML_TRY(grid_fft_rows(ctx, cur, nt * GRID_CURRENTS, rows_fwd, false));
    return grid_fft_cols(ctx, cur, nt * GRID_CURRENTS, false);
}

int propagate_tile_sets(ml_ctx *ctx, double Z0, int first, int n) {
    PropagatePlan &pp = ctx->prop;
    return grid_pass(ctx, Z0, n, tile_prepare, [&](const GridPass &p) -> int {
        const GridTilePlan &t = pp.tile;
        const GridWork w = grid_work_tiled(pp);
        const int rows_fwd = std::min(t.x.B, t.nx);   // the rows below hold no sample of any tile
        for (int m = 0; m < n; ++m) {
            const d2 *fields = ctx->fields.buf.as<d2>() + (size_t)(first + m) * 4 * t.nx * t.ny;
            for (int tile0 = 0; tile0 < t.tiles; tile0 += t.batch) {
                const int nt = std::min(t.batch, t.tiles - tile0);
                ML_TRY(grid_tile_currents(ctx, fields, p.sc.Z, w.cur, tile0, nt, rows_fwd));
                const d2 *Kt = w.K + (size_t)tile0 * GRID_KERNELS * p.ps;
                if (pp.want_h)
                    launch_tile_contract<true>(ctx, p.blocks, tile0 == 0, Kt, w.cur, w.out, p.ps, nt);
                else
                    launch_tile_contract<false>(ctx, p.blocks, tile0 == 0, Kt, w.cur, w.out, p.ps, nt);
                ML_HIP(hipGetLastError());
            }
            ML_TRY(grid_finish_set(ctx, p, w.out, m, pp.grid.mx));
        }
        return ML_OK;
    });
}

}  // namespace ml
