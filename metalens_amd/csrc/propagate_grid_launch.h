// What propagate_stack.hip shares with propagate_grid.hip on the host: plain functions around that file's own (templated,
// static) launchers, so that a stack pass runs the same transform, pad and contraction kernels with the same launch shapes
// as the fine plan, and the helpers that state the geometry arguments, the scales and the plan facts once.  They read the
// active plan's lengths and twiddle tables from ctx->prop.  (The device functions both files share: propagate_grid_dev.h.)
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
// ... of the active plan (pp.grid's lengths and targets) for the origin (tx_off, ty_off) and the plane z; `out` is NULL
GridGeoArgs grid_geo(const PropagatePlan &pp, double tx_off, double ty_off, double z);

// the medium's impedance and what a target's E and H are multiplied by: the direct path's scales times 1 / (Lx Ly)
struct GridScales {
    double Z, scale_e, scale_h;
};
GridScales grid_scales(const PropagatePlan &pp, const GridPlanFacts &f, double Z0);

// what the transform launchers read of a tile plan: its lengths; m_x, m_y: the targets the launches read
void grid_facts_of_tile(GridPlanFacts &f, const GridTilePlan &t, int m_x, int m_y, int64_t workspace_bytes);

// `n_planes` planes of the plan's Lx x Ly along y, rows [0, rows); along x, every column
int grid_fft_rows(ml_ctx *ctx, double2 *planes, int n_planes, int rows, bool inverse);
int grid_fft_cols(ml_ctx *ctx, double2 *planes, int n_planes, bool inverse);
// the four current spectra of the tiles [tile0, tile0 + nt) of one field set [4][nx][ny] into cur [nt][4][Lx][Ly]:
// grid_tile_pad_kernel, then the forward passes over the rows [0, rows_fwd) and every column
int grid_tile_currents(ml_ctx *ctx, const double2 *fields, double Z, double2 *cur, int tile0, int nt, int rows_fwd);
// grid_fine_contract_kernel<want_h of the plan, first, lattices>: the tiles [.., + n) into the output spectra of 1 or 2
// lattices, the second one's kernel spectra k_lattice elements behind the first one's
int grid_fine_contract(ml_ctx *ctx, int lattices, unsigned blocks, bool first, const double2 *K, size_t k_lattice, const double2 *cur,
                       double2 *out, size_t ps, int n);
int grid_upload_twiddles(ml_ctx *ctx, DevBuf &buf, int L);
// the bytes the four current planes of a batch's tiles may take (GRID_TILE_BATCH_BYTES)
int64_t grid_tile_batch_bytes();

}  // namespace ml
