// The finite-distance propagator for a STACK of planes of fine targets (ml_propagate_plan_grid_stack; plan arithmetic:
// propagate_grid.h GridStackPlan).  fp64 throughout, no atomics.
//
// The fine plan of propagate_grid.hip contracts ONE set of current spectra with the kernel spectra of every lattice
// (a, b), an origin (tx_off, ty_off) on the pitch.  A plane at another z is one more such set of kernels: here a LAYER is
// (plane p, lattice (a, b)), l = p Ax Ay + a Ay + b, and its (tx_off, ty_off, z) come from a table in device memory that
// the plan entry uploads once (GridStackLayerRow).  Per field set:
//   1. the currents of every tile are padded and transformed once, in the batches of the tiled plan, and kept;
//   2. the layers go GRID_FINE_PAIR at a time, a single one last if their number is odd - a pair may straddle two planes:
//        cached:    one contraction over all tiles (the kernel spectra [layers][tiles][8] are filled by the first pass on a
//                   shape and kept while the plan and the shape stay);
//        streamed:  per batch of tiles the fill of the pair ([2][batch][8]) - ONE launch where the pair's planes fit the
//                   memory-side cache, else a launch per layer (grid_stack_fill_layers) - the forward transforms, the
//                   contraction - FIRST on the first batch only;
//   3. one inverse transform of the pair's 2 x (6 or 3) planes, rows [0, m_cx);
//   4. the scatter into result[component][(p mx + a + sx i) my + b + sy j].
// The transforms and the contraction are propagate_grid.hip's own kernels through its launchers
// (propagate_grid_launch.h); the fill has the arithmetic of grid_tile_fill_kernel operation for operation, the pad that
// of grid_tile_pad_kernel and the scatter the scales of grid_fine_scatter_kernel, so plane p of a stack has the bits of
// the fine plan planned at z[p].  The result is [set][6 or 3][T], T = nz mx my, plane-major: ml_propagate,
// ml_propagate_sets, the downloads, ml_propagate_accumulate and ml_propagate_sums read T alone and serve it unchanged.
#include "nearfield_math.h"
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
// grid: index p holds the lag (p < m ? p : p - L) - a B; the layer's origin and plane are uniform loads from the table.
// From the lag on, grid_tile_fill_kernel operation for operation.
__global__ __launch_bounds__(256) void grid_stack_fill_kernel(const GridStackFillArgs t) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < Lx Ly (a multiple of 256)
    const GridStackLayerRow &layer = t.layers[blockIdx.z];
    const double tx_off = layer.tx_off, ty_off = layer.ty_off, z = layer.z;
    const int tile = t.tile0 + blockIdx.y, ta = tile / t.cy, tb = tile - ta * t.cy;
    const int p = (int)(id / t.Ly), r = (int)(id - (size_t)p * t.Ly);
    const int lx = (p < t.mx ? p : p - t.Lx) - ta * t.Bx, ly = (r < t.my ? r : r - t.Ly) - tb * t.By;
    const double dx = fma((double)lx, t.dxp, tx_off), dy = fma((double)ly, t.dyp, ty_off);
    const double s_row = fma(dx, dx, z * z);
    const double R = sqrt_exact(fma(dy, dy, s_row));
    const double iR = recip(R);
    const double ux = dx * iR, uy = dy * iR, uz = z * iR;
    const double q = iR * t.inv_k, q2 = q * q;
    double sn, cs;
    sincos_cw(t.k * R, sn, cs);
    const c2 w = {cs * q, sn * q};
    const c2 ca = {1.0 - q2, q}, cb = {fma(-3.0, q2, 1.0), 3.0 * q};
    const c2 wb = cmulf(w, cb);
    const c2 txx = {fma(-(ux * ux), cb.r, ca.r), fma(-(ux * ux), cb.i, ca.i)};
    const c2 tyy = {fma(-(uy * uy), cb.r, ca.r), fma(-(uy * uy), cb.i, ca.i)};
    const c2 wxx = cmulf(w, txx), wyy = cmulf(w, tyy);
    const c2 ci = {fma(-q, w.r, -w.i), fma(-q, w.i, w.r)};   // w (i - q)
    const double gxy = ux * uy, gzx = uz * ux, gzy = uz * uy;
    d2 *o = t.out + (size_t)blockIdx.z * t.layer_stride + (size_t)blockIdx.y * GRID_KERNELS * t.plane_stride + id;
    o[0] = make_double2(-wxx.i, wxx.r);
    o[t.plane_stride] = make_double2(wb.i * gxy, -(wb.r * gxy));
    o[2 * t.plane_stride] = make_double2(-wyy.i, wyy.r);
    o[3 * t.plane_stride] = make_double2(wb.i * gzx, -(wb.r * gzx));
    o[4 * t.plane_stride] = make_double2(wb.i * gzy, -(wb.r * gzy));
    o[5 * t.plane_stride] = make_double2(ci.r * ux, ci.i * ux);
    o[6 * t.plane_stride] = make_double2(ci.r * uy, ci.i * uy);
    o[7 * t.plane_stride] = make_double2(ci.r * uz, ci.i * uz);
}

struct GridStackPadArgs {
    const d2 *fields;       // one field set [4][nx][ny]
    const int *row_first;   // of a synthesised field, or NULL
    d2 *cur;                // [tiles of the launch][4][Lx][Ly]
    size_t plane_stride;
    int nx, ny, Lx, Ly, Bx, By, tile0, cy;
    double Z;
};

// current c = blockIdx.y of tile tile0 + blockIdx.z into its padded plane: grid_tile_pad_kernel, the same conversion, the
// same zeros (that kernel and its launch stay in propagate_grid.hip, whose launches its tests pin)
__global__ __launch_bounds__(256) void grid_stack_pad_kernel(const GridStackPadArgs a) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;   // < Lx Ly
    const int il = (int)(id / a.Ly), jl = (int)(id - (size_t)il * a.Ly);
    const int tile = a.tile0 + blockIdx.z, ta = tile / a.cy, tb = tile - ta * a.cy;
    const int i = ta * a.Bx + il, j = tb * a.By + jl;
    const int c = blockIdx.y, f = 3 - c;
    d2 v = make_double2(0.0, 0.0);
    if (il < a.Bx && jl < a.By && i < a.nx && j < a.ny) {
        const int first = a.row_first ? a.row_first[i] : 0;   // (0x7f7f7f7f: no sample of the row is inside)
        if (j >= first && j < a.ny - first) {
            const double sg = (f == 0 || f == 3) ? -1.0 : 1.0, den = f < 2 ? a.Z : 1.0;
            const d2 s = a.fields[((size_t)f * a.nx + i) * a.ny + j];
            v = make_double2(sg * s.x / den, sg * s.y / den);
        }
    }
    a.cur[((size_t)blockIdx.z * GRID_CURRENTS + c) * a.plane_stride + id] = v;
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
    const double scale = m < 3 ? s.scale_e : s.scale_h;
    const d2 v = s.out[((size_t)l * s.nc + m) * s.plane_stride + (size_t)i * s.Ly + j];
    s.result[(size_t)m * s.T + ((size_t)layer.p * s.mx + fi) * s.my + fj] = make_double2(scale * v.x, scale * v.y);
}

// the eight kernels of the tiles [tile0, tile0 + nt), nt <= GRID_TILE_BATCH_MAX, of the nl layers from l0 on into K
// (layer_stride elements from layer to layer) and their forward transforms
static int stack_kernels(ml_ctx *ctx, int l0, int nl, int tile0, int nt, d2 *K, size_t layer_stride) {
    const PropagatePlan &pp = ctx->prop;
    const GridPlanFacts &f = pp.grid;
    const GridTilePlan &t = pp.fine.tile;
    GridStackFillArgs a;
    a.out = K;
    a.plane_stride = (size_t)f.Lx * f.Ly;
    a.layer_stride = layer_stride;
    a.layers = pp.stack_layers.as<GridStackLayerRow>() + l0;
    a.Lx = f.Lx;
    a.Ly = f.Ly;
    a.mx = f.mx;
    a.my = f.my;
    a.tile0 = tile0;
    a.cy = t.y.c;
    a.Bx = t.x.B;
    a.By = t.y.B;
    a.dxp = pp.dxp;
    a.dyp = pp.dyp;
    a.k = 2.0 * M_PI * pp.n_glass / pp.wavelength;
    a.inv_k = 1.0 / a.k;
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

// the plan and the workspace for the resident field's shape and, with cache_kernels, every layer's kernel spectra (kept
// while the shape stays)
static int stack_prepare(ml_ctx *ctx) {
    PropagatePlan &pp = ctx->prop;
    if (pp.spectra_ready && pp.grid.nx == ctx->fields.nx && pp.grid.ny == ctx->fields.ny) return ML_OK;
    pp.spectra_ready = false;
    char why[480];
    GridStackPlan s;
    const int nz = (int)pp.stack_z.size();
    if (grid_stack_plan(ctx->fields.nx, ctx->fields.ny, pp.fine.mx, pp.fine.my, pp.fine.sx, pp.fine.sy, pp.want_h, pp.tile_lx,
                        pp.tile_ly, pp.fine.cache_kernels, grid_tile_batch_bytes(), pp.stack_z.data(), nz, &s, why, sizeof why) != 0) {
        set_error("%s", why);
        return ML_EINVAL;
    }
    const GridFinePlan &p = pp.fine = s.fine;
    const GridTilePlan &t = pp.tile = p.tile;
    GridPlanFacts &f = pp.grid;   // what the transform launchers read: the tile's lengths
    f.nx = t.nx;
    f.ny = t.ny;
    f.mx = p.m_cx;
    f.my = p.m_cy;
    f.Lx = t.x.L;
    f.Ly = t.y.L;
    f.outputs = t.outputs;
    f.plane_bytes = t.plane_bytes;
    f.workspace_bytes = s.workspace_bytes;
    if (pp.grid_work.reserve((size_t)s.workspace_bytes) != ML_OK) {
        if (p.cache_kernels) {
            GridStackPlan streamed;
            grid_stack_plan(t.nx, t.ny, p.mx, p.my, p.sx, p.sy, pp.want_h, pp.tile_lx, pp.tile_ly, 0, grid_tile_batch_bytes(),
                            pp.stack_z.data(), nz, &streamed, why, sizeof why);
            set_error("the stack FFT form keeps the kernel spectra of %d planes x %d x %d lattices and %d tiles: the device did not "
                      "give the %lld bytes of its workspace; cache_kernels=0 fills them in every pass and takes %lld bytes",
                      nz, p.ax, p.ay, t.tiles, (long long)s.workspace_bytes, (long long)streamed.workspace_bytes);
        } else {
            set_error("the stack FFT form: the device did not give the %lld bytes of its workspace (%d tiles; the current spectra "
                      "of all tiles are kept for a pass)", (long long)s.workspace_bytes, t.tiles);
        }
        return ML_ENOMEM;
    }
    ML_TRY(grid_upload_twiddles(ctx, pp.grid_tw_x, f.Lx));
    ML_TRY(grid_upload_twiddles(ctx, pp.grid_tw_y, f.Ly));
    if (p.cache_kernels) {   // [layers][tiles][8]
        const size_t ps = (size_t)f.Lx * f.Ly, per_layer = (size_t)t.tiles * GRID_KERNELS * ps;
        for (int l0 = 0; l0 < s.layers; l0 += GRID_FINE_PAIR) {
            const int nl = std::min(GRID_FINE_PAIR, s.layers - l0);
            for (int tile0 = 0; tile0 < t.tiles; tile0 += GRID_TILE_BATCH_MAX) {   // 512 planes per layer and launch at the most
                const int nt = std::min(GRID_TILE_BATCH_MAX, t.tiles - tile0);
                ML_TRY(stack_kernels(ctx, l0, nl, tile0, nt,
                                     pp.grid_work.as<d2>() + l0 * per_layer + (size_t)tile0 * GRID_KERNELS * ps, per_layer));
            }
        }
    }
    pp.spectra_ready = true;
    return ML_OK;
}

int propagate_stack_sets(ml_ctx *ctx, double Z0, int first, int n) {
    PropagatePlan &pp = ctx->prop;
    pp.have_result = false;
    ML_TRY(stack_prepare(ctx));
    const GridPlanFacts &f = pp.grid;
    const GridFinePlan &fp = pp.fine;
    const GridTilePlan &t = fp.tile;
    const int T = pp.T, nc = f.outputs, layers = (int)pp.stack_z.size() * fp.ax * fp.ay;
    ML_TRY(pp.result.reserve((size_t)n * nc * T * sizeof(d2)));
    const size_t ps = (size_t)f.Lx * f.Ly;
    // cached: [layers][tiles][8]; streamed: [2][batch][8]
    const size_t k_layer = (size_t)(fp.cache_kernels ? t.tiles : t.batch) * GRID_KERNELS * ps;
    d2 *K = pp.grid_work.as<d2>(), *cur = K + (size_t)(fp.cache_kernels ? layers : GRID_FINE_PAIR) * k_layer;
    d2 *out = cur + (size_t)t.tiles * GRID_CURRENTS * ps;
    const double k = 2.0 * M_PI * pp.n_glass / pp.wavelength, Z = Z0 / pp.n_glass;
    const double scale_h = k * k / (4.0 * M_PI) * pp.dxp * pp.dyp;
    const double inv_n = 1.0 / ((double)f.Lx * (double)f.Ly);   // a power of two
    const unsigned blocks = (unsigned)(ps / 256);
    const int rows_fwd = std::min(t.x.B, t.nx);   // the rows below hold no sample of any tile
    GridStackPadArgs p;
    p.row_first = ctx->caches.rows_describe_fields ? ctx->grid.row_first.as<int>() : (const int *)nullptr;
    p.plane_stride = ps;
    p.nx = t.nx;
    p.ny = t.ny;
    p.Lx = f.Lx;
    p.Ly = f.Ly;
    p.Bx = t.x.B;
    p.By = t.y.B;
    p.cy = t.y.c;
    p.Z = Z;
    GridStackScatterArgs s;
    s.out = out;
    s.plane_stride = ps;
    s.T = (size_t)T;
    s.nc = nc;
    s.Ly = f.Ly;
    s.m_cx = fp.m_cx;
    s.m_cy = fp.m_cy;
    s.mx = fp.mx;
    s.my = fp.my;
    s.sx = fp.sx;
    s.sy = fp.sy;
    s.scale_e = Z * scale_h * inv_n;
    s.scale_h = scale_h * inv_n;
    for (int m = 0; m < n; ++m) {
        p.fields = ctx->fields.buf.as<d2>() + (size_t)(first + m) * 4 * t.nx * t.ny;
        for (int tile0 = 0; tile0 < t.tiles; tile0 += t.batch) {   // the current spectra of every tile, once per set
            const int nt = std::min(t.batch, t.tiles - tile0);
            p.tile0 = tile0;
            p.cur = cur + (size_t)tile0 * GRID_CURRENTS * ps;
            hipLaunchKernelGGL(grid_stack_pad_kernel, dim3(blocks, GRID_CURRENTS, nt), dim3(256), 0, ctx->stream, p);
            ML_HIP(hipGetLastError());
            ML_TRY(grid_fft_rows(ctx, p.cur, nt * GRID_CURRENTS, rows_fwd, false));
            ML_TRY(grid_fft_cols(ctx, p.cur, nt * GRID_CURRENTS, false));
        }
        s.result = pp.result.as<d2>() + (size_t)m * nc * T;
        for (int l0 = 0; l0 < layers; l0 += GRID_FINE_PAIR) {
            const int nl = std::min(GRID_FINE_PAIR, layers - l0);
            if (fp.cache_kernels) {
                ML_TRY(grid_fine_contract(ctx, nl, blocks, true, K + (size_t)l0 * k_layer, k_layer, cur, out, ps, t.tiles));
            } else {
                for (int tile0 = 0; tile0 < t.tiles; tile0 += t.batch) {
                    const int nt = std::min(t.batch, t.tiles - tile0);
                    ML_TRY(stack_kernels(ctx, l0, nl, tile0, nt, K, k_layer));
                    ML_TRY(grid_fine_contract(ctx, nl, blocks, tile0 == 0, K, k_layer, cur + (size_t)tile0 * GRID_CURRENTS * ps, out,
                                              ps, nt));
                }
            }
            ML_TRY(grid_fft_cols(ctx, out, nl * nc, true));
            ML_TRY(grid_fft_rows(ctx, out, nl * nc, fp.m_cx, true));
            s.layers = pp.stack_layers.as<GridStackLayerRow>() + l0;
            hipLaunchKernelGGL(grid_stack_scatter_kernel, dim3((fp.m_cx * fp.m_cy + 255) / 256, nc, nl), dim3(256), 0, ctx->stream, s);
            ML_HIP(hipGetLastError());
        }
    }
    pp.have_result = true;
    pp.result_sets = n;
    return ML_OK;
}

}  // namespace ml
