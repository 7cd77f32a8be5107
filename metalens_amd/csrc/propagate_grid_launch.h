// The host launchers of propagate_grid.hip that propagate_stack.hip goes through: plain functions around that file's
// own (templated, static) ones, so that a stack pass runs the same transform and contraction kernels with the same launch
// shapes as the fine plan.  They read the active plan's lengths and twiddle tables from ctx->prop, as those do.
#pragma once

#include "common.h"

namespace ml {

// A layer of a stack plan as the device reads it (PropagatePlan::stack_layers): the lattice's origin minus the aperture's,
// the plane's z, and where the layer's targets go in the result
struct GridStackLayerRow {
    double tx_off, ty_off, z;
    int p, a, b, unused;
};

// `n_planes` planes of the plan's Lx x Ly along y, rows [0, rows); along x, every column
int grid_fft_rows(ml_ctx *ctx, double2 *planes, int n_planes, int rows, bool inverse);
int grid_fft_cols(ml_ctx *ctx, double2 *planes, int n_planes, bool inverse);
// grid_fine_contract_kernel<want_h of the plan, first, lattices>: the tiles [.., + n) into the output spectra of 1 or 2
// lattices, the second one's kernel spectra k_lattice elements behind the first one's
int grid_fine_contract(ml_ctx *ctx, int lattices, unsigned blocks, bool first, const double2 *K, size_t k_lattice, const double2 *cur,
                       double2 *out, size_t ps, int n);
int grid_upload_twiddles(ml_ctx *ctx, DevBuf &buf, int L);
// the bytes the four current planes of a batch's tiles may take (GRID_TILE_BATCH_BYTES)
int64_t grid_tile_batch_bytes();

}  // namespace ml
