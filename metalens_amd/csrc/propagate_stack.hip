// The finite-distance propagator for a STACK of planes of fine targets (ml_propagate_plan_grid_stack; plan arithmetic:
// propagate_grid.h GridStackPlan).  fp64 throughout, no atomics.
//
// The fine plan of propagate_grid_fine.hip contracts ONE set of current spectra with the kernel spectra of every lattice
// (a, b), an origin (tx_off, ty_off) on the pitch.  A plane at another z is one more such set of kernels: here a LAYER is
// (plane p, lattice (a, b)), l = p Ax Ay + a Ay + b, and its (tx_off, ty_off, z) come from a table in device memory that
// the plan entry uploads once (GridStackLayerRow).  The pass is the layered driver of propagate_grid_fine.hip
// (grid_layered_sets) with this file's fill and scatter (stack_ops).  Per field set:
//   1. the currents of every tile are padded and transformed once, in the batches of the tiled plan, and kept
//      (grid_tile_currents: the tiled plan's own pad kernel and launch);
//   2. the layers go GRID_FINE_PAIR at a time, a single one last if their number is odd - a pair may straddle two planes:
//        cached:    one contraction over all tiles (the kernel spectra [layers][tiles][8] are filled by the first pass on a
//                   shape and kept while the plan and the shape stay);
//        streamed:  per batch of tiles the fill of the pair ([2][batch][8]) - ONE launch where the pair's planes fit the
//                   memory-side cache, else a launch per layer (grid_stack_fill_layers) - the forward transforms, the
//                   contraction - FIRST on the first batch only;
//   3. one inverse transform of the pair's 2 x (6 or 3) planes, rows [0, m_cx);
//   4. the scatter into result[component][(p mx + a + sx i) my + b + sy j].
// The transforms, the pad and the contraction are the kernels of propagate_grid_fft.hip, propagate_grid_tiled.hip and
// propagate_grid_fine.hip through their launchers (propagate_grid_launch.h); the fill calls the grid_green of
// grid_tile_fill_kernel and the scatter the grid_store_scaled of grid_fine_scatter_kernel (propagate_grid_dev.h), so plane
// p of a stack has the bits of the fine plan planned at z[p].
// Layouts: the workspace in PropagatePlan::grid_work (common.h grid_work_layered), the layer table in GridStackLayerRow.
// The result is [set][6 or 3][T], T = nz mx my, plane-major: ml_propagate, ml_propagate_sets, the downloads,
// ml_propagate_accumulate and ml_propagate_sums read T alone and serve it unchanged.
#include "propagate_grid_dev.h"
#include "propagate_grid_launch.h"

namespace ml {

typedef double2 d2;

struct GridStackFillArgs {
    d2 *out;                            // the first plane of the launch's first tile of its first layer
    size_t plane_stride, layer_stride;  // elements from plane to plane, from layer to layer
    const GridStackLayerRow *layers;    // the launch's first layer
    int Lx, Ly, mx, my;                 // tile lengths, targets per lattice as planned
    int tile0, cy;                      // the launch's first tile; tiles along y
    int Bx, By;                         // samples per tile
    double dxp, dyp, k, inv_k;
};

// the eight kernels of tile tile0 + blockIdx.y and layer blockIdx.z of the launch at every index of the tile's padded
// grid: index p holds the lag (p < m ? p : p - L) - a B, as in grid_tile_fill_kernel; the layer's origin and plane are
// uniform loads from the table
__global__ __launch_bounds__(256) void grid_stack_fill_kernel(const GridStackFillArgs t) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < Lx Ly (a multiple of 256)
    const GridStackLayerRow &layer = t.layers[blockIdx.z];
    const double tx_off = layer.tx_off, ty_off = layer.ty_off, z = layer.z;
    const int tile = t.tile0 + blockIdx.y, ta = tile / t.cy, tb = tile - ta * t.cy;
    const int p = (int)(id / t.Ly), r = (int)(id - (size_t)p * t.Ly);
    const int lx = (p < t.mx ? p : p - t.Lx) - ta * t.Bx, ly = (r < t.my ? r : r - t.Ly) - tb * t.By;
    grid_green(lx, ly, t.dxp, t.dyp, tx_off, ty_off, z, t.k, t.inv_k,
               t.out + (size_t)blockIdx.z * t.layer_stride + (size_t)blockIdx.y * GRID_KERNELS * t.plane_stride + id, t.plane_stride);
}

struct GridStackScatterArgs {
    const d2 *out;                     // [layers of the launch][nc][Lx][Ly]
    d2 *result;                        // [nc][T] of one field set
    size_t plane_stride, T;            // T = nz mx my
    const GridStackLayerRow *layers;   // the launch's first layer
    int nc, Ly;
    int m_cx, m_cy;                    // targets per lattice as planned
    int mx, my, sx, sy;                // fine targets of a plane, pitch ratios
    double scale_e, scale_h;
};

// layer (p, a, b) = blockIdx.z of the launch, component blockIdx.y: result[component][(p mx + a + sx i) my + b + sy j] =
// scale out[component][i][j] - grid_fine_scatter_kernel with the layer's plane; the targets of a ragged lattice beyond
// mx x my are dropped
__global__ __launch_bounds__(256) void grid_stack_scatter_kernel(const GridStackScatterArgs s) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= s.m_cx * s.m_cy) return;
    const int i = t / s.m_cy, j = t - i * s.m_cy, m = blockIdx.y, l = blockIdx.z;
    const GridStackLayerRow &layer = s.layers[l];
    const int fi = layer.a + s.sx * i, fj = layer.b + s.sy * j;
    if (fi >= s.mx || fj >= s.my) return;
    grid_store_scaled(&s.result[(size_t)m * s.T + ((size_t)layer.p * s.mx + fi) * s.my + fj],
                      s.out[((size_t)l * s.nc + m) * s.plane_stride + (size_t)i * s.Ly + j], m, s.scale_e, s.scale_h);
}

// the eight kernels of the tiles [tile0, tile0 + nt), nt <= GRID_TILE_BATCH_MAX, of the nl layers from l0 on into K
// (layer_stride elements from layer to layer) and their forward transforms
static int stack_kernels(ml_ctx *ctx, int l0, int nl, int tile0, int nt, d2 *K, size_t layer_stride) {
    const PropagatePlan &pp = ctx->prop;
    const GridPlanFacts &f = pp.grid;
    const GridTilePlan &t = pp.fine.tile;
    const GridGeoArgs g = grid_geo(pp, 0.0, 0.0, 0.0);   // (the origin and the plane: per layer, from the table)
    GridStackFillArgs a = {nullptr, g.plane_stride, layer_stride, nullptr, g.Lx, g.Ly, g.mx, g.my, tile0, t.y.c, t.x.B, t.y.B,
                           g.dxp, g.dyp, g.k, g.inv_k};   // (out, layers: per launch)
    // what a launch fills goes through the row pass next: all nl layers in one launch where that fits the memory-side
    // cache, else layer by layer (propagate_grid.h grid_stack_fill_layers)
    const int per_launch = grid_stack_fill_layers(nl, nt, f.plane_bytes);
    for (int l = 0; l < nl; l += per_launch) {
        a.out = K + l * layer_stride;
        a.layers = pp.stack_layers.as<GridStackLayerRow>() + l0 + l;
        hipLaunchKernelGGL(grid_stack_fill_kernel, dim3((unsigned)(a.plane_stride / 256), nt, per_launch), dim3(256), 0, ctx->stream, a);
        ML_HIP(hipGetLastError());
        const bool joined = per_launch > 1 && layer_stride == (size_t)nt * GRID_KERNELS * a.plane_stride;   // planes back to back
        const int passes = joined ? 1 : per_launch, planes = (joined ? per_launch : 1) * nt * GRID_KERNELS;
        for (int m = 0; m < passes; ++m) {
            ML_TRY(grid_fft_rows(ctx, a.out + m * layer_stride, planes, f.Lx, false));
            ML_TRY(grid_fft_cols(ctx, a.out + m * layer_stride, planes, false));
        }
    }
    return ML_OK;
}

// GridLayeredOps::fill: a launch takes GRID_TILE_BATCH_MAX tiles per layer (512 planes) at the most
static int stack_fill(ml_ctx *ctx, int l0, int nl, int tile0, int nt, d2 *K, size_t k_layer) {
    const size_t tile_stride = (size_t)GRID_KERNELS * ctx->prop.grid.Lx * ctx->prop.grid.Ly;
    for (int done = 0; done < nt; done += GRID_TILE_BATCH_MAX)
        ML_TRY(stack_kernels(ctx, l0, nl, tile0 + done, std::min(GRID_TILE_BATCH_MAX, nt - done), K + done * tile_stride, k_layer));
    return ML_OK;
}

static int stack_scatter(ml_ctx *ctx, const GridPass &p, const d2 *out, d2 *result, int l0, int nl) {
    const PropagatePlan &pp = ctx->prop;
    const GridFinePlan &fp = pp.fine;
    const GridStackScatterArgs s = {out, result, p.ps, (size_t)p.T, pp.stack_layers.as<GridStackLayerRow>() + l0, p.nc, pp.grid.Ly,
                                    fp.m_cx, fp.m_cy, fp.mx, fp.my, fp.sx, fp.sy, p.sc.scale_e, p.sc.scale_h};
    hipLaunchKernelGGL(grid_stack_scatter_kernel, dim3((fp.m_cx * fp.m_cy + 255) / 256, p.nc, nl), dim3(256), 0, ctx->stream, s);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

static void stack_no_memory(ml_ctx *ctx, int64_t workspace_bytes) {
    const PropagatePlan &pp = ctx->prop;
    const GridFinePlan &p = pp.fine;
    const GridTilePlan &t = p.tile;
    const int nz = (int)pp.stack_z.size();
    if (p.cache_kernels) {
        char why[480];
        GridStackPlan streamed;
        grid_stack_plan(t.nx, t.ny, p.mx, p.my, p.sx, p.sy, pp.want_h, pp.tile_lx, pp.tile_ly, 0, grid_tile_batch_bytes(),
                        pp.stack_z.data(), nz, &streamed, why, sizeof why);
        set_error("the stack FFT form keeps the kernel spectra of %d planes x %d x %d lattices and %d tiles: the device did not "
                  "give the %lld bytes of its workspace; cache_kernels=0 fills them in every pass and takes %lld bytes",
                  nz, p.ax, p.ay, t.tiles, (long long)workspace_bytes, (long long)streamed.workspace_bytes);
    } else {
        set_error("the stack FFT form: the device did not give the %lld bytes of its workspace (%d tiles; the current spectra "
                  "of all tiles are kept for a pass)", (long long)workspace_bytes, t.tiles);
    }
}

static int stack_prepare(ml_ctx *ctx);
static GridLayeredOps stack_ops(const PropagatePlan &pp) {
    return {(int)pp.stack_z.size() * pp.fine.ax * pp.fine.ay, GRID_FINE_PAIR, stack_prepare, stack_fill, stack_scatter, stack_no_memory};
}

// the plan and the workspace for the resident field's shape and, with cache_kernels, every layer's kernel spectra (kept
// while the shape stays)
static int stack_prepare(ml_ctx *ctx) {
    const PropagatePlan &pp = ctx->prop;
    if (grid_spectra_kept(ctx)) return ML_OK;
    char why[480];
    GridStackPlan s;
    if (grid_stack_plan(ctx->fields.nx, ctx->fields.ny, pp.fine.mx, pp.fine.my, pp.fine.sx, pp.fine.sy, pp.want_h, pp.tile_lx,
                        pp.tile_ly, pp.fine.cache_kernels, grid_tile_batch_bytes(), pp.stack_z.data(), (int)pp.stack_z.size(), &s, why,
                        sizeof why) != 0) {
        set_error("%s", why);
        return ML_EINVAL;
    }
    return grid_layered_prepare(ctx, stack_ops(pp), s.fine, s.workspace_bytes);
}

int propagate_stack_sets(ml_ctx *ctx, double Z0, int first, int n) { return grid_layered_sets(ctx, Z0, first, n, stack_ops(ctx->prop)); }

}  // namespace ml
