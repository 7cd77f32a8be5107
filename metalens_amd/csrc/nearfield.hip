// Near-field synthesis on MI355X: the steps of a synthesis, the choice of its kernels and the small helper
// kernels.  The kernels themselves (one thread per aperture sample, reference nearfield.py:117-477;
// oracle/nearfield_oracle.py is the NumPy statement of the same thing): nearfield_geometry.hip the per-sample
// records and patch lists, nearfield_simple.hip the fields of a round lens' order sets, nearfield_general.hip of any other.
// Compiled with -ffp-contract=off: the arguments of the large phases (k*distance ~ 1e4 rad) must
// be rounded exactly like the reference's NumPy expressions, so no multiply-add may be fused.
//
// Data in HBM
//   fields          complex128 [4][nx][ny]   Ex, Ey, Hx, Hy planes, y fastest (64 B / sample,
//                                            the only compulsory HBM traffic of this kernel)
//   tables          complex128 [order][n0][n1][n2][4]  per collection, <= ~1 MB in total,
//                                            L2-resident; one 64-byte line = the four
//                                            amplitudes of one grid node
//   ring arrays     float64 [n_rings]        + a uniform-in-r lookup table for the ring search
//   centre cells    sorted by spatial bin    (uniform grid, exact nearest neighbour)
#include <algorithm>
#include <cstdlib>

#include "nearfield_dev.h"
#include "synth_staging.h"

namespace ml {

// Per aperture row: how far from the row's two ends the first sample inside the lens is,
// min(j, ny-1-j).  Samples outside the lens are exactly zero, so the far-field GEMM skips that
// outer part of each row (zfold.hip).  Inside-the-lens is the kernels' own test
// sqrt(x^2 + y^2) <= outer boundary, which is monotone in |y|.
// Depends on the grid and the lens radius only, so it runs when one of them has changed.
__global__ __launch_bounds__(256) void row_extent_kernel(const NfArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nx) return;
    const double x = a.x_pts[i], rmax = a.B[a.n_rings];
    auto inside = [&](int j) { return !(sqrt(x * x + a.y_pts[j] * a.y_pts[j]) > rmax); };
    // The grid is uniform (the host checks the pitch), so the chord ends are known to +/- 1
    // sample in closed form; the kernels' own test then settles the last sample (a few loads
    // instead of three dependent binary searches).  A non-uniform y_pts only costs more steps.
    const int ny = a.ny;
    const double y0 = a.y_pts[0], dy = ny > 1 ? (a.y_pts[ny - 1] - y0) / (ny - 1) : 1.0;
    const double half_chord = sqrt(fmax(rmax * rmax - x * x, 0.0));
    auto clampi = [&](double v) { return (int)fmin(fmax(v, 0.0), (double)(ny - 1)); };
    // sample closest to y = 0: if it is outside, the whole row is
    int jc = clampi(rint(-y0 / dy));
    while (jc > 0 && fabs(a.y_pts[jc - 1]) < fabs(a.y_pts[jc])) --jc;
    while (jc < ny - 1 && fabs(a.y_pts[jc + 1]) < fabs(a.y_pts[jc])) ++jc;
    int first = 0x7f7f7f7f;
    if (inside(jc)) {
        int lo = min(clampi(ceil((-half_chord - y0) / dy)), jc);
        int hi = max(clampi(floor((half_chord - y0) / dy)), jc);
        while (lo > 0 && inside(lo - 1)) --lo;
        while (!inside(lo)) ++lo;                  // smallest inside index (<= jc)
        while (hi < ny - 1 && inside(hi + 1)) ++hi;
        while (!inside(hi)) --hi;                  // largest inside index (>= jc)
        first = min(lo, ny - 1 - hi);
    }
    a.row_first[i] = first;
}

// deterministic tree sum of the per-block partials (the same routine runs as a spare block of
// the projection kernel when a transform follows, farfield_project.hip)
__global__ __launch_bounds__(256) void sum_partials_kernel(const double *partial, int n,
                                                           double *groups) {
    // blockIdx.y = field set (member of a polarisation batch)
    sum_partials_group(partial + (size_t)blockIdx.y * n, n, groups + blockIdx.y * POWER_GROUPS,
                       blockIdx.x, threadIdx.x);
}

bool plan_cache_disabled() {
    static const bool v = diag_int("ML_NO_PLAN_CACHE", 0) != 0;
    return v;
}

int power_flush(ml_ctx *ctx) {
    SynthOut &out = ctx->out;
    if (!out.power_pending) return ML_OK;
    hipLaunchKernelGGL(sum_partials_kernel, dim3(POWER_GROUPS, ctx->fields.n_sets), dim3(256), 0,
                       ctx->stream, out.partial_power.as<double>(), out.n_partials,
                       out.power.as<double>());
    ML_HIP(hipGetLastError());
    out.power_pending = false;
    return ML_OK;
}

// upper bound on the centre list's length before the host has seen the lists: the patches with a sample inside
// the square around the centre disc (the axes' host copies are the grid's)
static int centre_patch_bound(const ml_ctx *ctx, int nx, int ny) {
    auto span = [&](const std::vector<double> &axis, int n) {
        int lo = n, hi = -1;
        for (int i = 0; i < n && i < (int)axis.size(); ++i)
            if (std::fabs(axis[i]) <= ctx->lens.search.r_centre) {
                lo = std::min(lo, i);
                hi = std::max(hi, i);
            }
        return hi < lo ? 0 : hi / 8 - lo / 8 + 1;
    };
    return span(ctx->grid.h_x_pts, nx) * span(ctx->grid.h_y_pts, ny);
}

void fill_layout_args(const ml_ctx *ctx, NfArgs &a) {
    const Lens &lens = ctx->lens;
    a.n_rings = lens.n_rings;
    a.B = lens.ring_boundaries.as<double>();
    a.rc = lens.ring_r_center.as<double>();
    a.period = lens.ring_period.as<double>();
    a.dphi = lens.ring_dphi.as<double>();
    a.lateral = lens.ring_lateral.as<double>();
    a.gc = lens.ring_gc.as<int>();
    a.rot_center = lens.ring_rot_center.as<int>();
    a.rot_half = lens.ring_rot_half.as<int>();
    a.rot_table = lens.rot_table.as<double2>();
    a.tie_table = lens.tie_table.as<double>();
    a.lut = lens.ring_lut.as<int>();
    a.lutrec = lens.ring_lutrec.as<RingBucket>();
    const RingSearchFacts &S = lens.search;
    a.lut_buckets = S.lut_buckets;
    a.lut_inv_h = S.lut_inv_h;
    a.lutrec_buckets = S.lutrec_buckets;
    a.lutrec_inv_h = S.lutrec_inv_h;
    a.r_outer = S.r_outer;
    a.n_cells = lens.n_cells;
    a.cx = lens.cell_x.as<double>();
    a.cy = lens.cell_y.as<double>();
    a.cwhich = lens.cell_which.as<int>();
    a.cindex = lens.cell_index.as<int>();
    a.cxy = lens.cell_xy.as<double2>();
    a.bin_start = lens.bin_start.as<int>();
    const BinFacts &C = lens.bins;
    a.bins_x = C.bins_x;
    a.bins_y = C.bins_y;
    a.bx0 = C.x0;
    a.by0 = C.y0;
    a.bh = C.h;
    a.inv_bh = 1.0 / C.h;
    const LatticeFacts &L = lens.lattice;
    a.lat_map = L.ok ? lens.cell_lattice_map.as<int>() : nullptr;
    a.lat_rec = L.ok ? lens.cell_lattice_rec.as<CellRec>() : nullptr;
    a.lat_c0x = L.c0x;
    a.lat_c0y = L.c0y;
    for (int k = 0; k < 4; ++k) a.lat_inv[k] = L.inv[k];
    a.lat_accept_r2 = L.accept_r2;
    for (int k = 0; k < 3; ++k) a.lat_g[k] = L.g[k];
    a.lat_guard = L.guard;
    a.lat_amin = L.amin;
    a.lat_bmin = L.bmin;
    a.lat_na = L.na;
    a.lat_nb = L.nb;
}

void fill_nf_args(ml_ctx *ctx, const ml_nearfield_params *p, int n, int nx, int ny, NfArgs &a) {
    a.p = p[0];
    a.n_pol = n;
    a.e_from_h = p[0].Z0 * (1.0 / p[0].n_glass) * (1.0 / p[0].k_glass);
    a.n_partials = 4 * ((ny + 7) / 8) * ((nx + 7) / 8);   // four per 8 x 8 patch (wave_power)
    for (int m = 0; m < MAX_POL; ++m) {
        const ml_nearfield_params &q = p[m < n ? m : 0];
        for (int k = 0; k < 3; ++k) a.pol[m][k] = q.pol[k];
        a.hcoef[m] = q.H_coef;
        a.dmom[m] = q.dipole_moment;
        // nearfield.py:225-228, the reference's own expressions (this file is compiled without contraction)
        const double Ex_i = q.pol[0] * q.dipole_moment, Ey_i = q.pol[1] * q.dipole_moment;
        a.pw_Hx[m] = -q.pol[1] * q.dipole_moment / q.Z0;
        a.pw_Hy[m] = q.pol[0] * q.dipole_moment / q.Z0;
        a.pw_power[m] = Ex_i * a.pw_Hy[m] - Ey_i * a.pw_Hx[m];
        a.pcoef[m] = q.Z0 * q.H_coef * q.H_coef;
    }
    a.nx = nx;
    a.ny = ny;
    a.patches_x = (ny + 7) / 8;

    const SynthGrid &grid = ctx->grid;
    a.x_pts = grid.x_pts.as<double>();
    a.y_pts = grid.y_pts.as<double>();
    a.row_first = grid.row_first.as<int>();
    a.geo_ix = grid.geo_ix.as<int2>();
    a.active_list = grid.active_list.as<int2>();
    a.active_count = grid.active_count.as<int>();
    a.active_flag = grid.active_flag.as<int>();
    a.list_stride = a.n_partials / 4;
    a.count_stride = a.n_partials / 4 / 1024 + 4;
    a.use_active = 0;
    a.list_count = nullptr;
    a.first_pass = 0;
    a.centre_patch_bound = 0;   // (launch_members: first pass only)
    for (int k = 0; k < 4; ++k) a.n_active[k] = 0;

    fill_layout_args(ctx, a);
    const Lens &lens = ctx->lens;

    a.tables = lens.table_desc.as<TableDesc>();
    a.center_desc = lens.h_center_desc;
    a.ring_rec = lens.ring_rec.as<double2>();
    a.ring_coll = lens.ring_coll.as<int>();
    for (int c = 0; c < MAX_RING_COLLS; ++c) a.coll[c] = lens.h_coll[c];
    a.ring_tab = lens.ring_tab.as<double2>();
    a.ring_ok = lens.ring_ok.as<double>();
    a.ring_ok_off = lens.ring_ok_off.as<int>();
    for (int k = 0; k < 4; ++k) a.ring_bounds_all[k] = lens.ring_bounds_all[k];
    const LensClass &K = lens.cls;
    a.simple_orders = K.simple ? 1 : 0;
    a.wide_mask = K.wide_mask;
    a.narrow_exists = K.narrow_exists;
    a.general_mask = K.general_mask;
    a.narrow_mask = K.narrow_mask;
    a.centre_general = K.centre_general;
    // (eight blocks of up to three orders or six of four: synth_staging.h)
    a.narrow_pitch = narrow_pitch(K.narrow_slots_max);
    a.narrow_cap = narrow_cap(a.narrow_pitch);
    a.center_tab = lens.center_qmajor.as<double2>();
    a.center_n_slots = lens.centre.n_slots;
    a.center_lo = lens.centre.lo;
    a.center_present = lens.centre.present;

    const Ties &ties = ctx->ties;
    a.tie_count = ties.count.as<int>();
    a.tie_list = ties.list.as<long long>();
    a.tie_cap = ML_TIE_CAPACITY;
    a.ovr_key = ties.ovr_key.as<long long>();
    a.ovr_slot = ties.ovr_slot.as<int>();
    a.n_ovr = ties.n_ovr;

    const SynthOut &out = ctx->out;
    a.fields = ctx->fields.buf.as<double>();
    a.partial_power = out.partial_power.as<double>();
    a.n_viol_keys = (MAX_SLOTS + 1) * MAX_ORDERS * 6;
    a.viol = out.violations.as<unsigned long long>() + (size_t)out.viol_half * a.n_viol_keys;
    a.viol_next = out.violations.as<unsigned long long>() + (size_t)(1 - out.viol_half) * a.n_viol_keys;
    // opt-in fusion: write the fields already multiplied by the plan's column phasors
    const FarfieldPlan &pl = ctx->plan;
    const bool premod = ctx->premod_enabled && pl.ready && pl.fold &&
                        pl.fold_y.has_E && pl.ny == ny;
    a.premod = premod ? pl.fold_y.E.as<double2>() : nullptr;
    ctx->fields.premod_serial = premod ? pl.serial : -1;
    // Three-order tables on uniform axes lit by one dipole have kernels of their own with the same arithmetic
    // (nearfield_simple.hip FIXED3; lens_pack.h fixed3_takes): what a listed steady-state launch of these arguments
    // may take - bit 0 the ring launch, bit 1 the centre launch; the launch code knows whether it is one.
    // METALENS_HIP_FIXED_SYNTH=0 in the environment, read once: the general kernels for every call
    static const bool fixed_off = [] { const char *e = getenv("METALENS_HIP_FIXED_SYNTH"); return e && e[0] == '0'; }();
    const Fixed3Facts facts = {a.coll, a.narrow_mask, a.center_n_slots, a.center_present, a.center_desc.uniform,
                               n, 1, 0, a.p.plane_wave, a.premod != nullptr};
    const Fixed3 fixed = fixed3_takes(facts);
    a.fixed3 = fixed_off ? 0 : (fixed.ring ? 1 : 0) | (fixed.centre ? 2 : 0);
}

// ---- the steps of a synthesis (nearfield_launch), each named for what it ensures; synth_caches.h says what each
// cache is keyed on and which event drops it ----

// row extents for the far-field GEMM: a function of the grid and the lens radius
static int ensure_row_extents(ml_ctx *ctx, const NfArgs &a) {
    const Key<2> key = ctx->caches.grid_layout_key();
    if (!plan_cache_disabled() && ctx->caches.row_extents.matches(key.v)) return ML_OK;
    hipLaunchKernelGGL(row_extent_kernel, dim3((a.nx + 255) / 256), dim3(256), 0, ctx->stream, a);
    ctx->caches.row_extents.set(key.v);
    return ML_OK;
}

// the per-sample records depend on the grid, the layout and the tie answers: rebuilt when one
// of them changes (the samples the kernel cannot settle are counted from zero each time)
// (... and, for the lists, on which collections are the wide ring instantiation's)
static int ensure_geometry(ml_ctx *ctx, const NfArgs &a) {
    SynthCaches &caches = ctx->caches;
    const Key<5> key = caches.geometry_key((long)a.nx * a.ny, ctx->lens.cls.list_word());
    if (!plan_cache_disabled() && caches.geometry.matches(key.v)) return ML_OK;
    ProfScope scope(ctx, ML_K_TWIDDLE);
    ML_HIP(hipMemsetAsync(ctx->ties.count.p, 0, sizeof(int), ctx->stream));
    ML_TRY(nearfield_geometry_launch(ctx, a));
    caches.geometry.set(key.v);
    caches.geometry_rebuilt();
    // the lists' lengths start their way back now, behind the scans and in front of the synthesis
    if (!ctx->counts_pinned) {
        ML_HIP(hipHostMalloc((void **)&ctx->counts_pinned, 4 * sizeof(int), hipHostMallocDefault));
        ML_HIP(hipEventCreateWithFlags(&ctx->counts_ready, hipEventDisableTiming));
    }
    // (one strided copy: the four totals lie count_stride integers apart)
    ML_HIP(hipMemcpy2DAsync(ctx->counts_pinned, sizeof(int), ctx->grid.active_count.p, (size_t)a.count_stride * sizeof(int),
                            sizeof(int), 4, hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipEventRecord(ctx->counts_ready, ctx->stream));
    caches.lengths = SynthCaches::QUEUED;
    return ML_OK;
}

// The lengths of the patch lists come back from the GPU once per geometry; the power partials of the patches that are
// not launched stay at the zeros written here.
static int ensure_list_lengths(ml_ctx *ctx, const NfArgs &a) {
    SynthCaches &caches = ctx->caches;
    if (caches.lengths == SynthCaches::KNOWN) return ML_OK;
    const LensClass &K = ctx->lens.cls;
    int *n_active = ctx->grid.n_active;
    // (list 0: the general kernel's - every lens patch of a lens without simple tables, the patches with samples of
    // general tables of a mixed one)
    const bool mixed = K.simple && (K.general_mask || K.centre_general);
    const int lo = K.simple && !mixed ? 1 : 0, hi = K.simple ? 3 : 0;
    for (int k = 0; k < 4; ++k) n_active[k] = 0;
    if (caches.lengths == SynthCaches::QUEUED) {
        // (queued with the geometry, an earlier call: normally long there - no draining of the stream)
        ML_HIP(hipEventSynchronize(ctx->counts_ready));
        for (int k = lo; k <= hi; ++k) n_active[k] = ctx->counts_pinned[k];
        caches.lengths = SynthCaches::KNOWN;
        ML_HIP(hipMemsetAsync(ctx->out.partial_power.p, 0, ctx->out.partial_power.bytes, ctx->stream));
    } else {
        caches.lengths = SynthCaches::KNOWN;
        for (int k = lo; k <= hi; ++k)
            ML_HIP(hipMemcpyAsync(&n_active[k], ctx->grid.active_count.as<int>() + (size_t)k * a.count_stride,
                                  sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        ML_HIP(hipMemsetAsync(ctx->out.partial_power.p, 0, ctx->out.partial_power.bytes, ctx->stream));
        ML_HIP(hipStreamSynchronize(ctx->stream));
    }
    return ML_OK;
}

// members at ONE source position share everything but two real weights per sample and go through
// the batch kernels (NP = n); members at DIFFERENT positions (a field-of-view sweep) are
// synthesised one after the other into their field sets - the same kernels and arguments as n
// single calls, so bit-identical to them - before any of them is transformed: geometry, lists and
// tables are set up once, and the geometry records are still cached when the next member reads
// them (no stage-1 result in between)
static int launch_members(ml_ctx *ctx, const ml_nearfield_params *p, int n, bool members_alone, NfArgs &a,
                          int *n_partials) {
    const int nx = a.nx, ny = a.ny;
    // one wave (= one workgroup) per 8 x 8 patch.  A wave that walks several patches so that its stores drain under the
    // next patch's arithmetic costs registers the kernel does not have (spills): 25-40 % slower.
    const dim3 full((ny + 7) / 8, (nx + 7) / 8);
    *n_partials = (int)(full.x * full.y) * 4;   // four power partials per patch (wave_power)
    // the kernels of a round lens' order sets, else the general one - over list 0 once the zeros are in place
    auto launch = [&](const NfArgs &q) {
        return q.simple_orders ? nearfield_simple_launch(ctx, q) : nearfield_general_launch(ctx, q, q.use_active ? dim3(q.n_active[0]) : full);
    };
    if (!a.use_active) a.centre_patch_bound = centre_patch_bound(ctx, nx, ny);
    bool one_position = true;
    for (int m = 1; m < n; ++m)
        one_position = one_position && p[m].source_x == p[0].source_x && p[m].source_y == p[0].source_y &&
                       p[m].source_z == p[0].source_z;
    ProfScope scope(ctx, ML_K_NEARFIELD);
    if (one_position && !members_alone) return launch(a);
    for (int m = 0; m < n; ++m) {
        NfArgs am;
        fill_nf_args(ctx, p + m, 1, nx, ny, am);
        am.outside_is_zero = a.outside_is_zero;
        am.use_active = a.use_active;
        am.centre_patch_bound = a.centre_patch_bound;
        for (int k = 0; k < 4; ++k) am.n_active[k] = a.n_active[k];
        am.fields += (size_t)m * 4 * nx * ny * 2;
        am.partial_power += (size_t)m * a.n_partials;
        ML_TRY(launch(am));
    }
    return ML_OK;
}

// the partials are summed by the projection kernel if one follows, else on demand
static int note_powers(ml_ctx *ctx, int n, int n_partials, bool keep_powers) {
    ctx->out.n_partials = n_partials;
    if (keep_powers) return ML_OK;   // (the partials just written are not summed: `power` stays as it is)
    ctx->out.power_pending = true;
    // a batch sums the partials of all its members now (the projection kernel's spare block,
    // which does it for free in the single-source pipeline, knows one set only)
    if (n > 1) ML_TRY(power_flush(ctx));
    return ML_OK;
}

int nearfield_launch(ml_ctx *ctx, const ml_nearfield_params *p, int n, int nx, int ny, bool members_alone,
                     bool keep_powers) {
    if (keep_powers) ML_TRY(power_flush(ctx));   // partials of the synthesis before, about to be overwritten
    NfArgs a;
    // this launch reports into the half the previous launch cleared
    ctx->out.viol_half = 1 - ctx->out.viol_half;
    fill_nf_args(ctx, p, n, nx, ny, a);
    ML_TRY(ensure_row_extents(ctx, a));
    ML_TRY(ensure_geometry(ctx, a));
    // samples outside the lens are zero whatever the source: stored by the first synthesis into
    // this buffer for this geometry, skipped afterwards (27 % of the stores of a 4096^2 window
    // around the 1 mm lens); anything else that writes the buffer drops the stamp (ml_fields_upload)
    const Key<6> zeros = ctx->caches.zeros_key((long)(intptr_t)ctx->fields.buf.p, (long)ctx->fields.buf.bytes, n, (long)nx * ny);
    a.outside_is_zero = !plan_cache_disabled() && ctx->caches.zeros.matches(zeros.v);
    if (a.outside_is_zero) {
        // ... and then only the patches that hold lens samples are launched at all
        ML_TRY(ensure_list_lengths(ctx, a));
        const int *n_active = ctx->grid.n_active;
        if (n_active[0] + n_active[1] + n_active[2] + n_active[3] > 0) {
            a.use_active = 1;
            for (int k = 0; k < 4; ++k) a.n_active[k] = n_active[k];
        }
    }
    int n_partials = 0;
    ctx->out.ring_form = ctx->out.centre_form = 0;   // (set by the launch code of the kernels that have two forms)
    ML_TRY(launch_members(ctx, p, n, members_alone, a, &n_partials));
    ctx->caches.zeros.set(zeros.v);
    ML_HIP(hipGetLastError());
    return note_powers(ctx, n, n_partials, keep_powers);
}

}  // namespace ml
