// The fine plan of the FFT form of the finite-distance propagator (ml_propagate_plan_grid_fine, method 'fft-fine';
// propagate_grid.h GridFinePlan): its pass, propagate_fine_sets, and the driver of the LAYERED passes, which the stack
// plan's pass (propagate_stack.hip) goes through as well (grid_layered_prepare, grid_layered_sets; GridLayeredOps in
// propagate_grid_launch.h says what differs).  fp64 throughout, no atomics.
//
// Targets on the aperture's pitch divided by (sx, sy): Ax Ay lattices on the pitch, lattice l = a Ay + b with the origin
// (fine_tx[a], fine_ty[b]), all on the tiled plan of (nx, ny, m_cx, m_cy): each a tiled convolution of the SAME current
// spectra with its own kernel spectra.  A layer is what has kernel spectra of its own: a lattice here, a (plane, lattice)
// of a stack.  Current spectra [tiles][4][Lx][Ly], padded and transformed once per field set in the batches of the tiled
// plan and kept for the pass; kernel spectra [layers][tiles][8] kept for the life of the plan (cache_kernels), or
// [2][batch][8] filled and transformed in every pass; outputs [2][6 or 3] (PropagatePlan::grid_work, common.h
// grid_work_layered).  Then layer by layer, in pairs (a single one last if their number is odd): contraction over all
// tiles in ascending order, ONE inverse transform of the pair's planes, scatter into the interleaved result.
// The kernel spectra of a lattice and the currents of a batch of tiles: propagate_grid_tiled.hip; the transform:
// propagate_grid_fft.hip.
#include "propagate_grid_dev.h"
#include "propagate_grid_launch.h"

namespace ml {

typedef double2 d2;

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

// ---- the layered driver ----------------------------------------------------------------------------------------------

int grid_layered_prepare(ml_ctx *ctx, const GridLayeredOps &ops, const GridFinePlan &p, int64_t workspace_bytes) {
    PropagatePlan &pp = ctx->prop;
    pp.fine = p;
    const GridTilePlan &t = pp.tile = p.tile;
    grid_facts_of_tile(pp.grid, t, p.m_cx, p.m_cy, workspace_bytes);
    if (pp.grid_work.reserve((size_t)workspace_bytes) != ML_OK) {
        ops.no_memory(ctx, workspace_bytes);
        return ML_ENOMEM;
    }
    ML_TRY(grid_upload_twiddles(ctx));
    if (p.cache_kernels) {
        const GridWork w = grid_work_layered(pp, ops.layers);
        for (int l0 = 0; l0 < ops.layers; l0 += ops.pair)
            ML_TRY(ops.fill(ctx, l0, std::min(ops.pair, ops.layers - l0), 0, t.tiles, w.K + l0 * w.k_layer, w.k_layer));
    }
    pp.spectra_ready = true;
    return ML_OK;
}

int grid_layered_sets(ml_ctx *ctx, double Z0, int first, int n, const GridLayeredOps &ops) {
    const PropagatePlan &pp = ctx->prop;
    return grid_pass(ctx, Z0, n, ops.prepare, [&](const GridPass &p) -> int {
        const GridFinePlan &fp = pp.fine;
        const GridTilePlan &t = fp.tile;
        const GridWork w = grid_work_layered(pp, ops.layers);
        const int rows_fwd = std::min(t.x.B, t.nx);   // the rows below hold no sample of any tile
        for (int m = 0; m < n; ++m) {
            const d2 *fields = ctx->fields.buf.as<d2>() + (size_t)(first + m) * 4 * t.nx * t.ny;
            for (int tile0 = 0; tile0 < t.tiles; tile0 += t.batch)   // the current spectra of every tile, once per set
                ML_TRY(grid_tile_currents(ctx, fields, p.sc.Z, w.cur + (size_t)tile0 * GRID_CURRENTS * p.ps, tile0,
                                          std::min(t.batch, t.tiles - tile0), rows_fwd));
            for (int l0 = 0; l0 < ops.layers; l0 += ops.pair) {
                const int nl = std::min(ops.pair, ops.layers - l0);
                if (fp.cache_kernels) {
                    ML_TRY(fine_contract(ctx, nl, p.blocks, true, w.K + l0 * w.k_layer, w.k_layer, w.cur, w.out, p.ps, t.tiles));
                } else {
                    for (int tile0 = 0; tile0 < t.tiles; tile0 += t.batch) {
                        const int nt = std::min(t.batch, t.tiles - tile0);
                        ML_TRY(ops.fill(ctx, l0, nl, tile0, nt, w.K, w.k_layer));
                        ML_TRY(fine_contract(ctx, nl, p.blocks, tile0 == 0, w.K, w.k_layer,
                                             w.cur + (size_t)tile0 * GRID_CURRENTS * p.ps, w.out, p.ps, nt));
                    }
                }
                ML_TRY(grid_fft_cols(ctx, w.out, nl * p.nc, true));
                ML_TRY(grid_fft_rows(ctx, w.out, nl * p.nc, fp.m_cx, true));
                ML_TRY(ops.scatter(ctx, p, w.out, p.result + (size_t)m * p.nc * p.T, l0, nl));
            }
        }
        return ML_OK;
    });
}

// ---- the fine pass -----------------------------------------------------------------------------------------------------

// (diagnostic build: ML_GRID_FINE_PAIR=1 contracts one lattice per read of the currents, for timing)
static int fine_pair() { return diag_int("ML_GRID_FINE_PAIR", GRID_FINE_PAIR) == 1 ? 1 : GRID_FINE_PAIR; }

// the eight kernel spectra of the tiles [tile0, tile0 + nt) of lattice (a, b) into K: the fill of a tiled plan whose
// origin is the lattice's, and the forward transform
static int fine_kernels(ml_ctx *ctx, int a, int b, int tile0, int nt, d2 *K) {
    return grid_tile_kernels(ctx, ctx->prop.fine_tx[a], ctx->prop.fine_ty[b], tile0, nt, K);
}

static int fine_fill(ml_ctx *ctx, int l0, int nl, int tile0, int nt, d2 *K, size_t k_layer) {
    const int ay = ctx->prop.fine.ay;
    for (int l = l0; l < l0 + nl; ++l) ML_TRY(fine_kernels(ctx, l / ay, l % ay, tile0, nt, K + (l - l0) * k_layer));
    return ML_OK;
}

static int fine_scatter(ml_ctx *ctx, const GridPass &p, const d2 *out, d2 *result, int l0, int nl) {
    const GridFinePlan &fp = ctx->prop.fine;
    GridFineScatterArgs s = {out, result, p.ps, p.nc, ctx->prop.grid.Ly, fp.m_cx, fp.m_cy, fp.mx, fp.my, fp.sx, fp.sy, {}, {},
                             p.sc.scale_e, p.sc.scale_h};
    for (int l = 0; l < nl; ++l) {
        s.a[l] = (l0 + l) / fp.ay;
        s.b[l] = (l0 + l) % fp.ay;
    }
    hipLaunchKernelGGL(grid_fine_scatter_kernel, dim3((fp.m_cx * fp.m_cy + 255) / 256, p.nc, nl), dim3(256), 0, ctx->stream, s);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

static void fine_no_memory(ml_ctx *ctx, int64_t workspace_bytes) {
    const PropagatePlan &pp = ctx->prop;
    const GridFinePlan &p = pp.fine;
    const GridTilePlan &t = p.tile;
    if (p.cache_kernels) {
        char why[480];
        GridFinePlan streamed;
        grid_fine_plan(t.nx, t.ny, p.mx, p.my, p.sx, p.sy, pp.want_h, pp.tile_lx, pp.tile_ly, 0, grid_tile_batch_bytes(), &streamed,
                       why, sizeof why);
        set_error("the fine FFT form keeps the kernel spectra of %d x %d lattices and %d tiles: the device did not give the "
                  "%lld bytes of its workspace; cache_kernels=0 fills them in every pass and takes %lld bytes",
                  p.ax, p.ay, t.tiles, (long long)workspace_bytes, (long long)streamed.workspace_bytes);
    } else {
        set_error("the fine FFT form: the device did not give the %lld bytes of its workspace (%d tiles; the current spectra "
                  "of all tiles are kept for a pass)", (long long)workspace_bytes, t.tiles);
    }
}

static int fine_prepare(ml_ctx *ctx);
static GridLayeredOps fine_ops(const PropagatePlan &pp) {
    return {pp.fine.ax * pp.fine.ay, fine_pair(), fine_prepare, fine_fill, fine_scatter, fine_no_memory};
}

// the plan and the workspace for the resident field's shape and, with cache_kernels, every lattice's kernel spectra
// (kept while the shape stays)
static int fine_prepare(ml_ctx *ctx) {
    const PropagatePlan &pp = ctx->prop;
    if (grid_spectra_kept(ctx)) return ML_OK;
    char why[480];
    GridFinePlan p;
    if (grid_fine_plan(ctx->fields.nx, ctx->fields.ny, pp.fine.mx, pp.fine.my, pp.fine.sx, pp.fine.sy, pp.want_h, pp.tile_lx,
                       pp.tile_ly, pp.fine.cache_kernels, grid_tile_batch_bytes(), &p, why, sizeof why) != 0) {
        set_error("%s", why);
        return ML_EINVAL;
    }
    return grid_layered_prepare(ctx, fine_ops(pp), p, p.workspace_bytes);
}

int propagate_fine_sets(ml_ctx *ctx, double Z0, int first, int n) { return grid_layered_sets(ctx, Z0, first, n, fine_ops(ctx->prop)); }

}  // namespace ml
