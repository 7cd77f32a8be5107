// The plans of the FFT form of the finite-distance propagator: the entries ml_propagate_plan_grid, _grid_long,
// _grid_tiled, _grid_fine and _grid_stack - one function, plan_grid, checks what is asked for against the resident shape
// and sets ctx->prop; a refusal leaves the previous plan as it was - and the queries of the active plan,
// ml_propagate_plan_planes, _lattices, _tiles and _info.  No kernel and no launch: the passes that run a plan are in
// propagate_grid.hip, propagate_grid_tiled.hip, propagate_grid_fine.hip and propagate_stack.hip, each of which plans
// again for the shape it meets.  The plan arithmetic and its refusals are in propagate_grid.h, what a plan holds in
// PropagatePlan (common.h), the layer table of a stack in GridStackLayerRow (propagate_grid_launch.h).
#include "propagate_grid_launch.h"

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
    const bool stack = fine && fine->z, tiled = fine || method == ML_PROPAGATE_FFT_TILED;
    // the shape a pass would meet now, if there is one: refuse here, with the previous plan as it was
    const int nx = ctx->fields.nx, ny = ctx->fields.ny;
    const bool resident = nx && ny;
    GridPlanFacts f;
    f.mx = mx;
    f.my = my;
    GridTilePlan tile;
    GridFinePlan fp;
    // what is wrong with the targets, the ratios or the tile lengths whatever the shape, and the plan for a resident one
    char why[480];
    int bad = 0;
    if (fine)
        bad = resident ? grid_fine_plan(nx, ny, mx, my, fine->sx, fine->sy, want_h, tile_lx, tile_ly, fine->cache_kernels,
                                        grid_tile_batch_bytes(), &fp, why, sizeof why)
                       : (grid_fine_check_axis("x", 0, mx, fine->sx, tile_lx, why, sizeof why) ||
                          grid_fine_check_axis("y", 0, my, fine->sy, tile_ly, why, sizeof why));
    else if (tiled)
        bad = resident ? grid_tile_plan(nx, ny, mx, my, want_h, tile_lx, tile_ly, grid_tile_batch_bytes(), &tile, why, sizeof why)
                       : (grid_tile_check_axis("x", 0, mx, tile_lx, why, sizeof why) ||
                          grid_tile_check_axis("y", 0, my, tile_ly, why, sizeof why));
    else if (resident)
        bad = grid_plan_facts(nx, ny, mx, my, want_h, &f, why, sizeof why, grid_cap(method));
    if (bad) {
        set_error("%s: %s", entry, why);
        return ML_EINVAL;
    }
    if (fine) {
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
    }
    if (tiled) {   // (the lengths asked for are known without a shape)
        f.Lx = resident ? tile.x.L : tile_lx;
        f.Ly = resident ? tile.y.L : tile_ly;
    }
    // the largest lag of the plan bounds k R as the direct plan's bounding box does (propagate.hip): checked against the
    // resident shape here, and by every pass against the shape it meets
    PropExtent ext;
    ext.tx_lo = tx0 - x0;
    ext.tx_hi = ext.tx_lo + (mx - 1) * (dxp / (fine ? fine->sx : 1));
    ext.ty_lo = ty0 - y0;
    ext.ty_hi = ext.ty_lo + (my - 1) * (dyp / (fine ? fine->sy : 1));
    ext.z_hi = z;
    if (resident) ML_TRY(prop_check_phase(entry, ext, nx, ny, dxp, dyp, wavelength, n_glass));
    ML_HIP(hipSetDevice(ctx->device));
    PropagatePlan &pp = ctx->prop;
    if (stack) {   // the layer table, once per plan: layer l = p A + a Ay + b (propagate_grid.h grid_stack_layer)
        std::vector<GridStackLayerRow> layers((size_t)fine->nz * fp.ax * fp.ay);   // what the device reads per layer
        for (size_t l = 0; l < layers.size(); ++l) {
            const GridStackLayer s = grid_stack_layer((int)l, fp.ax, fp.ay);
            layers[l] = {fine->tx_first[s.a] - x0, fine->ty_first[s.b] - y0, fine->z[s.p], s.p, s.a, s.b, 0};
        }
        ML_TRY(pp.stack_layers.reserve(layers.size() * sizeof(GridStackLayerRow)));
        ML_HIP(hipMemcpyAsync(pp.stack_layers.p, layers.data(), layers.size() * sizeof(GridStackLayerRow), hipMemcpyHostToDevice,
                              ctx->stream));
        ML_HIP(hipStreamSynchronize(ctx->stream));   // (`layers` goes away)
    }
    // nothing below refuses: the new state, in one place
    pp.ready = pp.have_result = pp.have_sums = pp.have_stokes = false;   // results and sums of the previous plan are gone
    pp.modes.planned = false;                           // and its mode tables (propagate_modes.hip)
    pp.spectra_ready = false;
    pp.method = method;
    pp.extent = ext;
    pp.grid = f;
    pp.tile = tile;
    pp.fine = fp;
    if (fine) {
        for (int a = 0; a < fp.ax; ++a) pp.fine_tx[a] = fine->tx_first[a] - x0;
        for (int b = 0; b < fp.ay; ++b) pp.fine_ty[b] = fine->ty_first[b] - y0;
    }
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
