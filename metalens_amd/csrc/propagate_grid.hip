// The finite-distance propagator for a tensor grid of targets on the aperture's own pitch, as an FFT convolution: the
// plain plan (ml_propagate_plan_grid, ml_propagate_plan_grid_long; methods 'fft', 'fft-long'), and propagate_grid_sets,
// which hands a pass of any other plan of the FFT form over to its file (propagate_grid_tiled.hip, propagate_grid_fine.hip,
// propagate_stack.hip).  The plans are made in propagate_grid_plan.hip, their arithmetic is in propagate_grid.h, the
// transform in propagate_grid_fft.hip.  fp64 throughout, no atomics.
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
// in propagate_grid_dev.h; the kernels of every file of the FFT form find the lag, the sample and the pointer and call them.
//
// A pass: pad the four currents of a set into Lx x Ly planes (zeros outside the aperture and outside the row extents
// of a synthesised field), transform them, contract bin by bin with the eight kernel spectra into 6 (3) output
// spectra, transform back, crop [0, mx) x [0, my) into the result with the direct path's scales times 1 / (Lx Ly) (a
// power of two).  The sets of a pass run one after another through the same launches: a set has the bits of that set
// propagated alone, and every operation is linear in the fields, so a field times two gives the output times two.
// Rows that are zero are not transformed: the forward row pass takes the nx aperture rows, the inverse row pass the mx
// target rows.  The long plan differs in the cap of a padded axis alone (grid_cap; the transform takes L = 16384 as well).
// Layouts: the workspace in PropagatePlan::grid_work (common.h, grid_work_plain), the result in PropagatePlan::result.
#include "propagate_grid_dev.h"
#include "propagate_grid_launch.h"

namespace ml {

typedef double2 d2;

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

int grid_finish_set(ml_ctx *ctx, const GridPass &p, d2 *out, int m, int rows_inv) {
    const GridPlanFacts &f = ctx->prop.grid;
    ML_TRY(grid_fft_cols(ctx, out, p.nc, true));
    ML_TRY(grid_fft_rows(ctx, out, p.nc, rows_inv, true));
    hipLaunchKernelGGL(grid_crop_kernel, dim3((p.T + 255) / 256, p.nc), dim3(256), 0, ctx->stream, out, p.ps,
                       p.result + (size_t)m * p.nc * p.T, f.mx, f.my, f.Ly, p.sc.scale_e, p.sc.scale_h);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

// the workspace and the kernel spectra for the resident field's shape (kept while the shape stays)
static int grid_prepare(ml_ctx *ctx) {
    PropagatePlan &pp = ctx->prop;
    if (grid_spectra_kept(ctx)) return ML_OK;
    const int mx = pp.grid.mx, my = pp.grid.my;
    char why[320];
    GridPlanFacts f;
    if (grid_plan_facts(ctx->fields.nx, ctx->fields.ny, mx, my, pp.want_h, &f, why, sizeof why, grid_cap(pp.method)) != 0) {
        set_error("%s", why);
        return ML_EINVAL;
    }
    pp.grid = f;
    ML_TRY(pp.grid_work.reserve((size_t)f.workspace_bytes));
    ML_TRY(grid_upload_twiddles(ctx));
    GridGeoArgs g = grid_geo(pp, pp.tx_off, pp.ty_off, pp.z);
    g.out = grid_work_plain(pp).K;
    hipLaunchKernelGGL(grid_fill_kernel, dim3((unsigned)(g.plane_stride / 256)), dim3(256), 0, ctx->stream, g);
    ML_HIP(hipGetLastError());
    ML_TRY(grid_fft_rows(ctx, g.out, GRID_KERNELS, f.Lx, false));
    ML_TRY(grid_fft_cols(ctx, g.out, GRID_KERNELS, false));
    pp.spectra_ready = true;
    return ML_OK;
}

int propagate_grid_sets(ml_ctx *ctx, double Z0, int first, int n) {
    PropagatePlan &pp = ctx->prop;
    if (pp.method == ML_PROPAGATE_FFT_TILED) return propagate_tile_sets(ctx, Z0, first, n);
    if (pp.method == ML_PROPAGATE_FFT_FINE) return propagate_fine_sets(ctx, Z0, first, n);
    if (pp.method == ML_PROPAGATE_FFT_STACK) return propagate_stack_sets(ctx, Z0, first, n);
    return grid_pass(ctx, Z0, n, grid_prepare, [&](const GridPass &p) -> int {
        const GridPlanFacts &f = pp.grid;
        const int nx = ctx->fields.nx, ny = ctx->fields.ny;
        const GridWork w = grid_work_plain(pp);
        // rows that are zero need no transform (diagnostic build: ML_GRID_ALL_ROWS=1 transforms them all, for timing)
        const bool all_rows = diag_int("ML_GRID_ALL_ROWS", 0) != 0;
        const int rows_fwd = all_rows ? f.Lx : nx, rows_inv = all_rows ? f.Lx : f.mx;
        const int *row_first = ctx->caches.rows_describe_fields ? ctx->grid.row_first.as<int>() : (const int *)nullptr;
        for (int m = 0; m < n; ++m) {
            const d2 *fields = ctx->fields.buf.as<d2>() + (size_t)(first + m) * 4 * nx * ny;
            hipLaunchKernelGGL(grid_pad_kernel, dim3(p.blocks, GRID_CURRENTS), dim3(256), 0, ctx->stream, fields, row_first, w.cur,
                               p.ps, nx, ny, f.Lx, f.Ly, p.sc.Z);
            ML_HIP(hipGetLastError());
            ML_TRY(grid_fft_rows(ctx, w.cur, GRID_CURRENTS, rows_fwd, false));
            ML_TRY(grid_fft_cols(ctx, w.cur, GRID_CURRENTS, false));
            if (pp.want_h)
                hipLaunchKernelGGL(grid_contract_kernel<true>, dim3(p.blocks), dim3(256), 0, ctx->stream, w.K, w.cur, w.out, p.ps);
            else
                hipLaunchKernelGGL(grid_contract_kernel<false>, dim3(p.blocks), dim3(256), 0, ctx->stream, w.K, w.cur, w.out, p.ps);
            ML_HIP(hipGetLastError());
            ML_TRY(grid_finish_set(ctx, p, w.out, m, rows_inv));
        }
        return ML_OK;
    });
}

}  // namespace ml
