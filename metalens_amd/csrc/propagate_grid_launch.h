// What crosses the files of the FFT form of the finite-distance propagator on the host - propagate_grid_fft.hip (the
// transform), propagate_grid.hip (the plain pass and the dispatch), propagate_grid_tiled.hip, propagate_grid_fine.hip (with
// the driver of the layered passes), propagate_stack.hip and propagate_grid_plan.hip (the entries) - each function defined
// in the file named with it, and what all of them state once: the stamp test of a prepare and the frame of a pass.  The
// transform launchers read the active plan's lengths and twiddle tables from ctx->prop.  (The device functions the files
// share: propagate_grid_dev.h; the parts of the workspace: common.h grid_work_*.)
#pragma once

#include "common.h"

namespace ml {

// A layer of a stack plan as the device reads it (PropagatePlan::stack_layers): the lattice's origin minus the aperture's,
// the plane's z, and where the layer's targets go in the result
struct GridStackLayerRow {
    double tx_off, ty_off, z;
    int p, a, b, unused;
};

// what a fill kernel reads of the plan
struct GridGeoArgs {
    double2 *out;          // kernel planes [8][Lx][Ly]
    size_t plane_stride;
    int Lx, Ly, mx, my;
    double tx_off, ty_off, dxp, dyp, z, k, inv_k;
};

// the medium's impedance and what a target's E and H are multiplied by: the direct path's scales times 1 / (Lx Ly)
struct GridScales {
    double Z, scale_e, scale_h;
};

// the padded length an axis of `method` may have
inline int grid_cap(int method) { return method == ML_PROPAGATE_FFT_LONG ? GRID_L_LONG_MAX : GRID_L_MAX; }

// how every prepare opens: the workspace and the kernel spectra of the resident field's shape are there (kept while the
// shape stays); if not, none are until the prepare has run through
inline bool grid_spectra_kept(ml_ctx *ctx) {
    PropagatePlan &pp = ctx->prop;
    const bool kept = pp.spectra_ready && pp.grid.nx == ctx->fields.nx && pp.grid.ny == ctx->fields.ny;
    if (!kept) pp.spectra_ready = false;
    return kept;
}

// what a pass reads once its prepare has run: elements of a plane, the workgroups of a launch over one, the outputs and
// targets of a set, the scales, and the result [n][nc][T]
struct GridPass {
    size_t ps;
    unsigned blocks;
    int nc, T;
    GridScales sc;
    double2 *result;
};

// ---- propagate_grid_fft.hip
// `n_planes` planes of the plan's Lx x Ly along y, rows [0, rows); along x, every column
int grid_fft_rows(ml_ctx *ctx, double2 *planes, int n_planes, int rows, bool inverse);
int grid_fft_cols(ml_ctx *ctx, double2 *planes, int n_planes, bool inverse);
// the tables of both axes of pp.grid.Lx, pp.grid.Ly into pp.grid_tw_x, pp.grid_tw_y
int grid_upload_twiddles(ml_ctx *ctx);

// ---- propagate_grid.hip
// ... of the active plan (pp.grid's lengths and targets) for the origin (tx_off, ty_off) and the plane z; `out` is NULL
GridGeoArgs grid_geo(const PropagatePlan &pp, double tx_off, double ty_off, double z);
GridScales grid_scales(const PropagatePlan &pp, const GridPlanFacts &f, double Z0);
// how the plain and the tiled pass end a set: the nc output spectra back along x and along y, rows [0, rows_inv), and
// the targets of pp.grid cropped and scaled into set m of the result
int grid_finish_set(ml_ctx *ctx, const GridPass &p, double2 *out, int m, int rows_inv);

// ---- propagate_grid_tiled.hip
int propagate_tile_sets(ml_ctx *ctx, double Z0, int first, int n);
// what the transform launchers read of a tile plan: its lengths; m_x, m_y: the targets the launches read
void grid_facts_of_tile(GridPlanFacts &f, const GridTilePlan &t, int m_x, int m_y, int64_t workspace_bytes);
// the bytes the four current planes of a batch's tiles may take (GRID_TILE_BATCH_BYTES)
int64_t grid_tile_batch_bytes();
// the eight kernel spectra of the tiles [tile0, tile0 + nt) of the active tile plan (pp.tile) for the origin
// (tx_off, ty_off) into K [nt][8][Lx][Ly]: grid_tile_fill_kernel, then the forward passes
int grid_tile_kernels(ml_ctx *ctx, double tx_off, double ty_off, int tile0, int nt, double2 *K);
// the four current spectra of the tiles [tile0, tile0 + nt) of one field set [4][nx][ny] into cur [nt][4][Lx][Ly]:
// grid_tile_pad_kernel, then the forward passes over the rows [0, rows_fwd) and every column
int grid_tile_currents(ml_ctx *ctx, const double2 *fields, double Z, double2 *cur, int tile0, int nt, int rows_fwd);

// ---- propagate_grid_fine.hip: the fine pass, and the driver of the layered passes (fine: a layer is a lattice; stack: a
// plane and a lattice).  What differs between the two:
struct GridLayeredOps {
    int layers;   // all of them
    int pair;     // layers contracted per read of the currents
    int (*prepare)(ml_ctx *ctx);
    // the kernel spectra of the layers [l0, l0 + nl) and the tiles [tile0, tile0 + nt) into K, k_layer elements from a
    // layer's first tile to the next layer's, and their forward transforms
    int (*fill)(ml_ctx *ctx, int l0, int nl, int tile0, int nt, double2 *K, size_t k_layer);
    // the planes out [nl][nc][Lx][Ly] of the layers [l0, l0 + nl), transformed back, into one set's result
    int (*scatter)(ml_ctx *ctx, const GridPass &p, const double2 *out, double2 *result, int l0, int nl);
    // set_error for a workspace the device did not give
    void (*no_memory)(ml_ctx *ctx, int64_t workspace_bytes);
};
int propagate_fine_sets(ml_ctx *ctx, double Z0, int first, int n);
// the rest of a layered prepare once the plan `p` of the resident shape stands: pp.fine, pp.tile and pp.grid from it,
// the workspace, the twiddles and, with cache_kernels, every layer's kernel spectra
int grid_layered_prepare(ml_ctx *ctx, const GridLayeredOps &ops, const GridFinePlan &p, int64_t workspace_bytes);
// the pass: per set the current spectra of every tile once, then the layers `pair` at a time, a single one last
int grid_layered_sets(ml_ctx *ctx, double Z0, int first, int n, const GridLayeredOps &ops);

// ---- propagate_stack.hip
int propagate_stack_sets(ml_ctx *ctx, double Z0, int first, int n);

// The frame of a pass of n sets: no result while it runs; `prepare`; the result's memory; what `body` reads (GridPass);
// then the result stands
template <typename Body>
int grid_pass(ml_ctx *ctx, double Z0, int n, int (*prepare)(ml_ctx *), Body body) {
    PropagatePlan &pp = ctx->prop;
    pp.have_result = false;
    ML_TRY(prepare(ctx));
    const GridPlanFacts &f = pp.grid;
    GridPass p;
    p.ps = (size_t)f.Lx * f.Ly;
    p.blocks = (unsigned)(p.ps / 256);
    p.nc = f.outputs;
    p.T = pp.T;
    ML_TRY(pp.result.reserve((size_t)n * p.nc * p.T * sizeof(double2)));
    p.sc = grid_scales(pp, f, Z0);
    p.result = pp.result.as<double2>();
    ML_TRY(body(p));
    pp.have_result = true;
    pp.result_sets = n;
    return ML_OK;
}

}  // namespace ml
