// Context, uploads (tables / layout / fields), near-field entry points, profiling.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "common.h"

namespace ml {

static thread_local std::string g_error;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}

static int h2d(ml_ctx *ctx, DevBuf &dst, const void *src, size_t bytes) {
    ML_TRY(dst.reserve(std::max<size_t>(bytes, 16)));
    if (bytes) ML_HIP(hipMemcpyAsync(dst.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return ML_OK;
}

// ---- profiling ---------------------------------------------------------------------------
static hipEvent_t take_event(ml_ctx *ctx) {
    if (!ctx->prof.pool.empty()) {
        hipEvent_t e = ctx->prof.pool.back();
        ctx->prof.pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void prof_begin(ml_ctx *ctx, int kernel, hipEvent_t *a, hipEvent_t *b, hipStream_t stream) {
    if (kernel < 0 || kernel >= ML_K_COUNT) return;   // launches that are not timed
    if (!ctx->prof.on || !((ctx->prof.mask >> kernel) & 1u)) return;
    if (ctx->prof.seen[kernel]++ % ctx->prof.period != 0) return;
    *a = take_event(ctx);
    *b = take_event(ctx);
    (void)hipEventRecord(*a, stream ? stream : ctx->stream);
}

void prof_end(ml_ctx *ctx, int kernel, hipEvent_t a, hipEvent_t b, hipStream_t stream) {
    if (!ctx->prof.on || !a || !b) return;
    (void)hipEventRecord(b, stream ? stream : ctx->stream);
    ctx->prof.pending.push_back({kernel, a, b});
}

int prof_harvest(ml_ctx *ctx) {
    for (auto &pd : ctx->prof.pending) {
        ML_HIP(hipEventSynchronize(pd.b));
        float ms = 0.f;
        ML_HIP(hipEventElapsedTime(&ms, pd.a, pd.b));
        ctx->prof.launches[pd.kernel] += 1;
        ctx->prof.total_ms[pd.kernel] += ms;
        ctx->prof.pool.push_back(pd.a);
        ctx->prof.pool.push_back(pd.b);
    }
    ctx->prof.pending.clear();
    return ML_OK;
}

// ---- what the kernels read about the lens: laid out by lens_pack.h, uploaded here ----------
static int fail(const PackError &e) {
    set_error("%s", e.msg.c_str());
    return e.code;
}
// ... once copies queued out of vectors that the return destroys have finished
static int fail_synced(ml_ctx *ctx, const PackError &e) {
    (void)hipStreamSynchronize(ctx->stream);
    return fail(e);
}

static int refresh_table_desc(ml_ctx *ctx) {
    Lens &lens = ctx->lens;
    if (!lens.tables_dirty) return ML_OK;
    std::vector<TableDesc> h(MAX_SLOTS + 1);
    memset(h.data(), 0, h.size() * sizeof(TableDesc));
    for (int s = 0; s <= MAX_SLOTS; ++s) {
        const TableSlot &t = (s == MAX_SLOTS) ? lens.center : lens.slots[s];
        if (!t.present) continue;
        TableDesc &d = h[s];
        d = describe_table(t, s == MAX_SLOTS);
        d.axis0 = t.axis0.as<double>();
        d.axis1 = t.axis1.as<double>();
        d.values = t.values.as<double>();
        d.order_k = t.order_k.as<double>();
    }
    ML_TRY(h2d(ctx, lens.table_desc, h.data(), h.size() * sizeof(TableDesc)));
    lens.h_center_desc = h[MAX_SLOTS];
    lens.h_table_desc = h;
    ML_HIP(hipStreamSynchronize(ctx->stream));   // h goes out of scope
    lens.tables_dirty = false;
    return ML_OK;
}

// The per-ring tables, records and collection descriptors and the centre table in the fast kernels' form
// (lens_pack.h locate_rings, classify_lens, pack_ring_tables, pack_centre_table).
static int refresh_ring_locations(ml_ctx *ctx) {
    Lens &lens = ctx->lens;
    const HostTable *slots[MAX_SLOTS], *colls[MAX_RING_COLLS];
    const TableDesc *desc[MAX_RING_COLLS];
    for (int s = 0; s < MAX_SLOTS; ++s) slots[s] = &lens.slots[s];
    const RingLocations at = locate_rings(slots, lens.h_ring_gc.data(), lens.h_ring_period.data(), lens.n_rings);
    if (at.err.code != ML_OK) return fail(at.err);
    for (int c = 0; c < lens.n_colls; ++c) {
        colls[c] = slots[lens.coll_slot[c]];
        desc[c] = &lens.h_table_desc[lens.coll_slot[c]];
    }
    // (diagnostic build only: ML_FORCE_GENERAL=1 sends a lens that qualifies through the general kernels - what
    // the order-list kernels are measured against; ML_FORCE_GENERAL_COLL = mask of dense collection
    // numbers, bit 16 = the centre table: those only)
    static const bool force_general = diag_int("ML_FORCE_GENERAL", 0) != 0;
    static const int force_general_coll = diag_int("ML_FORCE_GENERAL_COLL", 0);
    const LensClass K = classify_lens(colls, lens.n_colls, &lens.center, force_general, force_general_coll);
    if (K.lists_differ(lens.cls)) ctx->caches.lens_class_changed();
    lens.cls = K;
    const RingInputs rings = {lens.n_rings, lens.h_ring_coll.data(), lens.h_ring_period.data(), lens.h_ring_lateral.data(),
                              lens.h_ring_rc.data()};
    const RingTables T = pack_ring_tables(colls, desc, lens.coll_slot, lens.n_colls, K, rings, at);
    if (T.err.code != ML_OK) return fail(T.err);
    for (int c = 0; c < lens.n_colls; ++c) lens.h_coll[c] = T.coll[c];
    for (int k = 0; k < 4; ++k) lens.ring_bounds_all[k] = T.ring_bounds_all[k];
    ML_TRY(h2d(ctx, lens.ring_rec, T.rec.data(), T.rec.size() * sizeof(double)));
    ML_TRY(h2d(ctx, lens.ring_tab, T.tab.data(), T.tab.size() * sizeof(double)));
    ML_TRY(h2d(ctx, lens.ring_ok, T.ok.data(), T.ok.size() * sizeof(double)));
    ML_TRY(h2d(ctx, lens.ring_ok_off, T.ok_off.data(), T.ok_off.size() * sizeof(int32_t)));
    CentreTable C;
    if (lens.center.present) {
        C = pack_centre_table(lens.center, K.centre_simple, K.canon_center);
        ML_TRY(h2d(ctx, lens.center_qmajor, C.cq.data(), C.cq.size() * sizeof(double)));
    }
    lens.centre = C.slots;
    ML_HIP(hipStreamSynchronize(ctx->stream));   // T and C go out of scope
    return ML_OK;
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_abi_version(void) { return ML_ABI_VERSION; }

const char *ml_last_error(void) { return g_error.c_str(); }

int ml_device_count(int *count) {
    ML_REQUIRE(count, "count is NULL");
    ML_HIP(hipGetDeviceCount(count));
    return ML_OK;
}

int ml_ctx_create(int device, ml_ctx **out) {
    ML_REQUIRE(out, "out is NULL");
    *out = nullptr;
    int n = 0;
    ML_HIP(hipGetDeviceCount(&n));
    ML_REQUIRE(device >= 0 && device < n, "device %d out of range (%d visible)", device, n);
    ML_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    ML_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("libmetalens_hip is built for gfx950 (MI355X) only; device %d is %s", device,
                  prop.gcnArchName);
        return ML_EINVAL;
    }
    ml_ctx *ctx = new ml_ctx();
    ctx->device = device;
    snprintf(ctx->arch, sizeof ctx->arch, "%s", prop.gcnArchName);
    ctx->cu_count = prop.multiProcessorCount;
    ctx->hbm_bytes = (int64_t)prop.totalGlobalMem;
    hipError_t e = hipSuccess;
#ifdef ML_DIAG
    // (tools/cu_split_probe.py: this context's stream on the compute units [lo, hi) only - ML_STREAM_CUS="lo:hi", or
    // "lo:hi:k" = every k-th of them - read when the context is made)
    if (const char *m = getenv("ML_STREAM_CUS")) {
        int lo = 0, hi = 0, k = 1;
        if (sscanf(m, "%d:%d:%d", &lo, &hi, &k) >= 2 && hi > lo && k >= 1) {
            uint32_t mask[8] = {0};
            for (int c = lo; c < hi && c < 256; c += k) mask[c >> 5] |= 1u << (c & 31);
            e = hipExtStreamCreateWithCUMask(&ctx->stream, 8, mask);
            fprintf(stderr, "ML_STREAM_CUS %d:%d:%d -> %s\n", lo, hi, k, hipGetErrorString(e));
        }
    }
    if (!ctx->stream)
#endif
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
        delete ctx;
        return ML_EHIP;
    }
    *out = ctx;
    return ML_OK;
}

void ml_ctx_destroy(ml_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    comm_release(ctx);
    if (ctx->counts_pinned) (void)hipHostFree(ctx->counts_pinned);
    if (ctx->counts_ready) (void)hipEventDestroy(ctx->counts_ready);
    if (ctx->comm_stream) {
        for (int k = 0; k < 2; ++k) {
            (void)hipEventDestroy(ctx->amp_ready[k]);
            (void)hipEventDestroy(ctx->reduce_done[k]);
        }
        (void)hipStreamDestroy(ctx->comm_stream);
    }
    for (auto &pd : ctx->prof.pending) {
        (void)hipEventDestroy(pd.a);
        (void)hipEventDestroy(pd.b);
    }
    for (auto e : ctx->prof.pool) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;   // (the device buffers free themselves, on the device set above)
}

int ml_device_info(ml_ctx *ctx, char *name, int name_len, int *cu_count, int64_t *hbm_bytes) {
    ML_REQUIRE(ctx, "ctx is NULL");
    if (name && name_len > 0) snprintf(name, name_len, "%s", ctx->arch);
    if (cu_count) *cu_count = ctx->cu_count;
    if (hbm_bytes) *hbm_bytes = ctx->hbm_bytes;
    return ML_OK;
}

int ml_host_alloc(uint64_t bytes, void **ptr) {
    ML_REQUIRE(ptr && bytes > 0, "bad argument");
    ML_HIP(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
    return ML_OK;
}

int ml_host_free(void *ptr) {
    if (ptr) ML_HIP(hipHostFree(ptr));
    return ML_OK;
}

int ml_sync(ml_ctx *ctx) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_HIP(hipSetDevice(ctx->device));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    ML_TRY(comm_join(ctx, true));
    return ML_OK;
}

int ml_upload_table(ml_ctx *ctx, int slot, const double *axis0, int n0, const double *axis1,
                    int n1, const double *axis2, int n2, const int32_t *orders,
                    const double *order_k, int n_orders, const double *values,
                    const double *bounds, const double *center_periods) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(slot >= -1 && slot < MAX_SLOTS, "slot %d out of range [-1, %d)", slot, MAX_SLOTS);
    ML_REQUIRE(axis0 && axis1 && axis2 && orders && order_k && values && bounds, "NULL argument");
    ML_REQUIRE(n0 >= 2 && n1 >= 2 && n2 >= 2, "each table axis needs >= 2 nodes (%d,%d,%d)", n0,
               n1, n2);
    ML_REQUIRE(n_orders >= 1 && n_orders <= MAX_ORDERS, "n_orders %d out of range [1, %d]",
               n_orders, MAX_ORDERS);
    ML_REQUIRE(slot >= 0 || center_periods, "the centre table needs center_periods");
    ML_HIP(hipSetDevice(ctx->device));
    TableSlot &t = (slot < 0) ? ctx->lens.center : ctx->lens.slots[slot];
    ML_TRY(h2d(ctx, t.axis0, axis0, n0 * sizeof(double)));
    ML_TRY(h2d(ctx, t.axis1, axis1, n1 * sizeof(double)));
    ML_TRY(h2d(ctx, t.order_k, order_k, 2 * n_orders * sizeof(double)));
    ML_TRY(h2d(ctx, t.values, values, (size_t)n_orders * n0 * n1 * n2 * 4 * 2 * sizeof(double)));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    t.n0 = n0;
    t.n1 = n1;
    t.n2 = n2;
    t.n_orders = n_orders;
    t.h_axis0.assign(axis0, axis0 + n0);
    t.h_axis1.assign(axis1, axis1 + n1);
    t.h_axis2.assign(axis2, axis2 + n2);
    t.h_order_k.assign(order_k, order_k + 2 * n_orders);
    t.h_values.assign(values, values + (size_t)n_orders * n0 * n1 * n2 * 4 * 2);
    for (int k = 0; k < 6; ++k) t.bounds[k] = bounds[k];
    if (center_periods) {
        t.center_periods[0] = center_periods[0];
        t.center_periods[1] = center_periods[1];
    }
    t.present = true;
    ctx->lens.tables_dirty = true;
    return ML_OK;
}

int ml_upload_layout(ml_ctx *ctx, int n_rings, const double *B, const double *r_center,
                     const double *period, const double *dphi, const double *lateral,
                     const int32_t *ring_gc, const double *rot_table, const double *tie_table,
                     int rot_len,
                     const int32_t *ring_rot_center, const int32_t *ring_rot_half, int n_cells,
                     const double *cells) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(n_rings >= 1 && B && r_center && period && dphi && lateral && ring_gc,
               "ring arrays missing (n_rings=%d)", n_rings);
    ML_REQUIRE(rot_table && tie_table && rot_len >= 1 && ring_rot_center && ring_rot_half,
               "rotation table missing");
    // the field kernel's block-sharing key packs (ring, i0, i1) into 31 bits (nearfield_general.hip)
    ML_REQUIRE(n_rings < (1 << 19), "%d rings: at most %d are supported", n_rings, (1 << 19) - 1);
    for (int r = 0; r < n_rings; ++r)
        ML_REQUIRE(ring_rot_half[r] >= 0 && ring_rot_center[r] - ring_rot_half[r] - 1 >= 0 &&
                       ring_rot_center[r] + ring_rot_half[r] < rot_len,
                   "rotation table range of ring %d falls outside the table", r);
    ML_REQUIRE(n_cells >= 0 && (n_cells == 0 || cells), "cell array missing");
    for (int r = 0; r < n_rings; ++r)
        ML_REQUIRE(B[r] <= B[r + 1], "ring boundaries must be ascending (ring %d)", r);
    ML_HIP(hipSetDevice(ctx->device));
    Lens &lens = ctx->lens;
    lens.have_layout = false;
    lens.n_rings = n_rings;
    ML_TRY(h2d(ctx, lens.ring_boundaries, B, (n_rings + 1) * sizeof(double)));
    ML_TRY(h2d(ctx, lens.ring_r_center, r_center, n_rings * sizeof(double)));
    ML_TRY(h2d(ctx, lens.ring_period, period, n_rings * sizeof(double)));
    ML_TRY(h2d(ctx, lens.ring_dphi, dphi, n_rings * sizeof(double)));
    ML_TRY(h2d(ctx, lens.ring_lateral, lateral, n_rings * sizeof(double)));
    ML_TRY(h2d(ctx, lens.ring_gc, ring_gc, n_rings * sizeof(int32_t)));
    ML_TRY(h2d(ctx, lens.rot_table, rot_table, (size_t)rot_len * 2 * sizeof(double)));
    ML_TRY(h2d(ctx, lens.tie_table, tie_table, (size_t)rot_len * 6 * sizeof(double)));
    ML_TRY(h2d(ctx, lens.ring_rot_center, ring_rot_center, n_rings * sizeof(int32_t)));
    ML_TRY(h2d(ctx, lens.ring_rot_half, ring_rot_half, n_rings * sizeof(int32_t)));
    lens.h_ring_period.assign(period, period + n_rings);
    lens.h_ring_rc.assign(r_center, r_center + n_rings);
    lens.h_ring_lateral.assign(lateral, lateral + n_rings);
    lens.h_ring_gc.assign(ring_gc, ring_gc + n_rings);
    const DenseColls D = dense_collections(ring_gc, n_rings);
    if (D.err.code != ML_OK) return fail_synced(ctx, D.err);
    lens.n_colls = D.n_colls;
    for (int c = 0; c < D.n_colls; ++c) lens.coll_slot[c] = D.coll_slot[c];
    lens.h_ring_coll = D.ring_coll;
    ML_TRY(h2d(ctx, lens.ring_coll, D.ring_coll.data(), n_rings * sizeof(int32_t)));

    const RingSearch S = pack_ring_search(B, n_rings);
    if (S.err.code != ML_OK) return fail_synced(ctx, S.err);
    ML_TRY(h2d(ctx, lens.ring_lut, S.lut.data(), S.lut.size() * sizeof(int32_t)));
    ML_TRY(h2d(ctx, lens.ring_lutrec, S.rec.data(), S.rec.size() * sizeof(RingBucket)));
    lens.search = S.facts;

    lens.n_cells = n_cells;
    lens.lattice = LatticeFacts();
    if (n_cells > 0) {
        const CellBins C = bin_cells(cells, n_cells);
        if (C.err.code != ML_OK) return fail_synced(ctx, C.err);
        ML_TRY(h2d(ctx, lens.cell_x, C.sx.data(), n_cells * sizeof(double)));
        ML_TRY(h2d(ctx, lens.cell_y, C.sy.data(), n_cells * sizeof(double)));
        ML_TRY(h2d(ctx, lens.cell_xy, C.sxy.data(), C.sxy.size() * sizeof(double)));
        ML_TRY(h2d(ctx, lens.cell_which, C.sw.data(), n_cells * sizeof(int32_t)));
        ML_TRY(h2d(ctx, lens.cell_index, C.si.data(), n_cells * sizeof(int32_t)));
        lens.h_slot_of_cell = C.slot_of_cell;
        ML_TRY(h2d(ctx, lens.bin_start, C.start.data(), C.start.size() * sizeof(int32_t)));
        // lattice shortcut for the nearest-cell search (sorted slots index the arrays above)
        static const bool no_lattice = diag_int("ML_NO_CELL_LATTICE", 0) != 0;
        const LatticeFit L = no_lattice ? LatticeFit() : fit_lattice(C.sx, C.sy);
        std::vector<CellRec> rec;
        if (L.facts.ok) {
            ML_TRY(h2d(ctx, lens.cell_lattice_map, L.map.data(), L.map.size() * sizeof(int32_t)));
            rec = lattice_records(L, C);
            ML_TRY(h2d(ctx, lens.cell_lattice_rec, rec.data(), rec.size() * sizeof(CellRec)));
            lens.lattice = L.facts;
        }
        ML_HIP(hipStreamSynchronize(ctx->stream));   // C, L and rec go out of scope
        lens.bins = C.facts;
    }
    ML_HIP(hipStreamSynchronize(ctx->stream));
    lens.have_layout = true;
    ctx->caches.layout_changed();
    lens.tables_dirty = true;   // per-ring table locations depend on the ring periods
    return ML_OK;
}

static int nearfield_prepare(ml_ctx *ctx, const ml_nearfield_params *p, int n, const double *x_pts,
                             int nx, const double *y_pts, int ny, bool members_alone = false, bool keep_powers = false) {
    ML_REQUIRE(ctx && p && x_pts && y_pts, "NULL argument");
    ML_REQUIRE(nx >= 1 && ny >= 1, "empty grid (%d x %d)", nx, ny);
    ML_REQUIRE(n >= 1 && n <= 3, "a batch has 1 to 3 members, got %d", n);
    for (int m = 1; m < n; ++m)
        ML_REQUIRE(p[m].kvac == p[0].kvac && p[m].k_glass == p[0].k_glass && p[m].n_glass == p[0].n_glass &&
                       p[m].Z0 == p[0].Z0 && p[m].plane_wave == p[0].plane_wave,
                   "members of a batch share wavelength, substrate and source kind (member %d): they may differ "
                   "in position, polarisation and dipole moment", m);
    if (!ctx->lens.have_layout) {
        set_error("ml_upload_layout has not been called");
        return ML_ESTATE;
    }
    // a finite source: the phase k_vac |r - r_source| of a sample inside the lens goes through reduce_pio2 / sincos_cw
    // (nearfield_math.h), which cover arguments up to PHASE_LIMIT; the plane wave has no such phase
    for (int m = 0; m < n; ++m) {
        if (p[m].plane_wave) continue;
        const double rho = std::hypot(p[m].source_x, p[m].source_y) + ctx->lens.search.r_outer;
        const double R = std::sqrt(rho * rho + p[m].source_z2), kR = p[m].kvac * R;
        ML_REQUIRE(kR <= PHASE_LIMIT, "source %d lies up to %.6g m from a sample of the lens, k R = %.6g: the phase arithmetic "
                   "covers k R up to %g (a plane wave, source_z = -inf, has no such limit)", m, R, kR, PHASE_LIMIT);
    }
    ML_HIP(hipSetDevice(ctx->device));
    if (ctx->lens.n_cells > 0 && !ctx->lens.center.present) {
        set_error("centre cells present but no HexGridSet table uploaded (slot -1)");
        return ML_ESTATE;
    }
    if (ctx->lens.tables_dirty) {
        ML_TRY(refresh_table_desc(ctx));
        ML_TRY(refresh_ring_locations(ctx));
    }
    // the grid usually repeats from call to call (sweeps over sources): upload only on change
    auto grid_axis = [&](DevBuf &dev, std::vector<double> &host, const double *src, int n) -> int {
        if ((int)host.size() == n && dev.p && memcmp(host.data(), src, n * sizeof(double)) == 0)
            return ML_OK;
        ML_HIP(hipStreamSynchronize(ctx->stream));   // an earlier async copy may still read `host`
        host.assign(src, src + n);
        ctx->caches.grid_changed();
        return h2d(ctx, dev, host.data(), n * sizeof(double));
    };
    ML_TRY(grid_axis(ctx->grid.x_pts, ctx->grid.h_x_pts, x_pts, nx));
    ML_TRY(grid_axis(ctx->grid.y_pts, ctx->grid.h_y_pts, y_pts, ny));
    const size_t plane = (size_t)nx * ny;
    ML_TRY(ctx->fields.buf.reserve((size_t)n * 4 * plane * 2 * sizeof(double)));
    ctx->fields.nx = nx;
    ctx->fields.ny = ny;
    ctx->fields.n_sets = n;
    ctx->fields.field_set = 0;
    // four power partials per wave (8 x 8 samples: one per row of sixteen lanes, nearfield_dev.h wave_power)
    const int blocks = ((ny + 7) / 8) * ((nx + 7) / 8);
    ML_TRY(ctx->out.partial_power.reserve((size_t)n * blocks * 4 * sizeof(double)));
    ML_TRY(ctx->out.power.reserve((size_t)n * POWER_GROUPS * sizeof(double)));
    // two halves: each synthesis launch clears the one the next launch reports into
    const size_t viol_bytes = (size_t)2 * (MAX_SLOTS + 1) * MAX_ORDERS * 6 * sizeof(unsigned long long);
    ML_TRY(ctx->out.violations.reserve(viol_bytes));
    if (!ctx->out.viol_zeroed) {
        ML_HIP(hipMemsetAsync(ctx->out.violations.p, 0, viol_bytes, ctx->stream));
        ctx->out.viol_zeroed = true;
    }
    ML_TRY(ctx->grid.row_first.reserve((size_t)nx * sizeof(int)));
    ctx->caches.rows_describe_fields = true;
    // nearest-cell ties: answers for another geometry are dropped
    if (!ctx->ties.count.p) {
        ML_TRY(ctx->ties.count.reserve(2 * sizeof(int)));
        ML_HIP(hipMemsetAsync(ctx->ties.count.p, 0, 2 * sizeof(int), ctx->stream));
    }
    ML_TRY(ctx->ties.list.reserve((size_t)ML_TIE_CAPACITY * sizeof(long long)));
    if (ctx->caches.drop_foreign_answers()) ctx->ties.n_ovr = 0;
    ML_TRY(ctx->grid.geo_ix.reserve((size_t)blocks * 64 * 2 * sizeof(int)));   // patch-major, 64 per patch
    ML_TRY(ctx->grid.active_list.reserve((size_t)4 * blocks * 2 * sizeof(int)));           // four lists (NfArgs::active_list)
    ML_TRY(ctx->grid.active_count.reserve((size_t)4 * (blocks / 1024 + 4) * sizeof(int)));   // each: total + one per chunk of 1024 patches
    ML_TRY(ctx->grid.active_flag.reserve((size_t)blocks * sizeof(int)));
    return nearfield_launch(ctx, p, n, nx, ny, members_alone, keep_powers);
}

int ml_nearfield_async(ml_ctx *ctx, const ml_nearfield_params *p, const double *x_pts, int nx,
                       const double *y_pts, int ny) {
    return nearfield_prepare(ctx, p, 1, x_pts, nx, y_pts, ny);
}

int ml_nearfield_batch_async(ml_ctx *ctx, const ml_nearfield_params *p, int n, const double *x_pts,
                             int nx, const double *y_pts, int ny) {
    return nearfield_prepare(ctx, p, n, x_pts, nx, y_pts, ny);
}

int ml_nearfield_members_async(ml_ctx *ctx, const ml_nearfield_params *p, int n, const double *x_pts, int nx,
                               const double *y_pts, int ny, int keep_powers) {
    ML_REQUIRE(ctx, "ctx is NULL");
    if (keep_powers && !(ctx->out.power.p && ctx->fields.nx == nx && ctx->fields.ny == ny && ctx->fields.n_sets == n)) {
        set_error("ml_nearfield_members_async: keep_powers needs a synthesis of %d members on %d x %d samples before it", n,
                  nx, ny);
        return ML_ESTATE;
    }
    return nearfield_prepare(ctx, p, n, x_pts, nx, y_pts, ny, true, keep_powers != 0);
}

int ml_fields_select(ml_ctx *ctx, int set) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(set >= 0 && set < ctx->fields.n_sets, "field set %d out of range (%d resident)", set,
               ctx->fields.n_sets);
    ctx->fields.field_set = set;
    return ML_OK;
}

int ml_nearfield_powers(ml_ctx *ctx, double *power, int n) {
    ML_REQUIRE(ctx && power, "NULL argument");
    ML_REQUIRE(n >= 1 && n <= ctx->fields.n_sets, "%d powers asked for, %d field sets resident", n, ctx->fields.n_sets);
    ML_REQUIRE(ctx->out.power.p, "no near field has been synthesised");
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(power_flush(ctx));
    std::vector<double> groups((size_t)n * POWER_GROUPS);
    ML_HIP(hipMemcpyAsync(groups.data(), ctx->out.power.p, groups.size() * sizeof(double),
                          hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    for (int m = 0; m < n; ++m) {
        double pw = 0;
        for (int g = 0; g < POWER_GROUPS; ++g) pw += groups[(size_t)m * POWER_GROUPS + g];
        power[m] = pw;
    }
    return ML_OK;
}

static double decode_key(unsigned long long k, int check) {
    if ((check & 1) == 0) k = ~k;
    unsigned long long b = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}

int ml_nearfield_ties(ml_ctx *ctx, int64_t *sample_ids, int max_ids, int *n_ties) {
    ML_REQUIRE(ctx && n_ties, "NULL argument");
    if (!ctx->ties.count.p) {   // nothing synthesised yet: nothing pending
        *n_ties = 0;
        return ML_OK;
    }
    ML_HIP(hipSetDevice(ctx->device));
    int count = 0;
    ML_HIP(hipMemcpyAsync(&count, ctx->ties.count.as<int>(), sizeof count,
                          hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    *n_ties = count;
    const int n = std::min(std::min(count, ML_TIE_CAPACITY), max_ids);
    if (sample_ids && n > 0) {
        static_assert(sizeof(long long) == sizeof(int64_t), "sample ids are 64-bit");
        ML_HIP(hipMemcpy(sample_ids, ctx->ties.list.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    return ML_OK;
}

int ml_nearfield_tie_answers(ml_ctx *ctx, const int64_t *sample_ids, const int32_t *cell_index, int n) {
    ML_REQUIRE(ctx && (n == 0 || (sample_ids && cell_index)), "NULL argument");
    ML_REQUIRE(n >= 0, "negative count");
    ML_HIP(hipSetDevice(ctx->device));
    ML_HIP(hipStreamSynchronize(ctx->stream));   // a running synthesis may be reading the old list
    std::vector<std::pair<long long, int>> kv((size_t)n);
    for (int k = 0; k < n; ++k) {
        ML_REQUIRE(cell_index[k] >= 0 && (size_t)cell_index[k] < ctx->lens.h_slot_of_cell.size(),
                   "cell index %d out of range", cell_index[k]);
        kv[k] = {(long long)sample_ids[k], ctx->lens.h_slot_of_cell[cell_index[k]]};
    }
    std::sort(kv.begin(), kv.end());
    std::vector<long long> keys((size_t)n);
    std::vector<int32_t> slots((size_t)n);
    for (int k = 0; k < n; ++k) {
        keys[k] = kv[k].first;
        slots[k] = kv[k].second;
    }
    if (n > 0) {
        ML_TRY(h2d(ctx, ctx->ties.ovr_key, keys.data(), keys.size() * sizeof(long long)));
        ML_TRY(h2d(ctx, ctx->ties.ovr_slot, slots.data(), slots.size() * sizeof(int32_t)));
        ML_HIP(hipStreamSynchronize(ctx->stream));   // the staging vectors go out of scope
    }
    ctx->ties.n_ovr = n;
    ctx->caches.answers_given(n);
    return ML_OK;
}

int ml_nearfield_result(ml_ctx *ctx, double *power, ml_bound_violation *violations,
                        int max_violations, int *n_violations) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_HIP(hipSetDevice(ctx->device));
    const size_t n_keys = (size_t)(MAX_SLOTS + 1) * MAX_ORDERS * 6;
    std::vector<unsigned long long> keys(n_keys);
    double pw = 0, group_sums[POWER_GROUPS];
    ML_REQUIRE(ctx->out.power.p && ctx->out.violations.p, "no near field has been synthesised");
    ML_TRY(power_flush(ctx));
    ML_HIP(hipMemcpyAsync(group_sums, ctx->out.power.p, sizeof group_sums, hipMemcpyDeviceToHost,
                          ctx->stream));
    ML_HIP(hipMemcpyAsync(keys.data(),
                          ctx->out.violations.as<unsigned long long>() + (size_t)ctx->out.viol_half * n_keys,
                          n_keys * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    ML_TRY(prof_harvest(ctx));
    for (int g = 0; g < POWER_GROUPS; ++g) pw += group_sums[g];   // last level of the reduction
    if (power) *power = pw;
    int count = 0;
    // reference check order: collections in list order, then the centre; per order; ux<, ux>,
    // uy<, uy>, period<, period>
    for (int s = 0; s <= MAX_SLOTS; ++s) {
        const TableSlot &t = (s == MAX_SLOTS) ? ctx->lens.center : ctx->lens.slots[s];
        if (!t.present) continue;
        for (int o = 0; o < t.n_orders; ++o)
            for (int c = 0; c < 6; ++c) {
                const unsigned long long k = keys[((size_t)s * MAX_ORDERS + o) * 6 + c];
                if (k == 0) continue;
                if (violations && count < max_violations) {
                    ml_bound_violation &v = violations[count];
                    v.slot = (s == MAX_SLOTS) ? -1 : s;
                    v.order = o;
                    v.check = c;
                    v.reserved = 0;
                    v.value = decode_key(k, c);
                    v.bound = t.bounds[c];
                }
                ++count;
            }
    }
    if (n_violations) *n_violations = count;
    return ML_OK;
}

int ml_nearfield_kernel_info(ml_ctx *ctx, int *family, int *ring_orders_max, int *centre_orders) {
    ML_REQUIRE(ctx, "ctx is NULL");
    if (ctx->lens.tables_dirty || !ctx->lens.have_layout) {
        set_error("no near field has been synthesised from the current tables and layout");
        return ML_ESTATE;
    }
    int widest = 0;
    for (int c = 0; c < ctx->lens.n_colls; ++c) widest = std::max(widest, ctx->lens.h_coll[c].n_slots);
    if (family) *family = ctx->lens.cls.simple ? ((ctx->lens.cls.general_mask || ctx->lens.cls.centre_general) ? 2 : 1) : 0;
    if (ring_orders_max) *ring_orders_max = ctx->lens.cls.simple ? widest : 0;
    if (centre_orders) *centre_orders = ctx->lens.cls.simple ? ctx->lens.centre.n_slots : 0;
    return ML_OK;
}

int ml_nearfield_synth_info(ml_ctx *ctx, int *ring_form, int *centre_form) {
    ML_REQUIRE(ctx, "ctx is NULL");
    if (ring_form) *ring_form = ctx->out.ring_form;
    if (centre_form) *centre_form = ctx->out.centre_form;
    return ML_OK;
}

int ml_nearfield(ml_ctx *ctx, const ml_nearfield_params *p, const double *x_pts, int nx,
                 const double *y_pts, int ny, double *power, ml_bound_violation *violations,
                 int max_violations, int *n_violations) {
    ML_TRY(nearfield_prepare(ctx, p, 1, x_pts, nx, y_pts, ny));
    return ml_nearfield_result(ctx, power, violations, max_violations, n_violations);
}

int ml_fields_shape(ml_ctx *ctx, int *nx, int *ny) {
    ML_REQUIRE(ctx, "ctx is NULL");
    if (nx) *nx = ctx->fields.nx;
    if (ny) *ny = ctx->fields.ny;
    return ML_OK;
}

int ml_fields_download(ml_ctx *ctx, double *Ex, double *Ey, double *Hx, double *Hy) {
    ML_REQUIRE(ctx, "ctx is NULL");
    if (ctx->fields.nx == 0 || ctx->fields.ny == 0) {
        set_error("no resident field set");
        return ML_ESTATE;
    }
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(comm_join(ctx, false));
    ML_TRY(fields_unmodulate(ctx));   // the host always sees the plain near field
    const size_t plane_bytes = (size_t)ctx->fields.nx * ctx->fields.ny * 2 * sizeof(double);
    double *dst[4] = {Ex, Ey, Hx, Hy};
    for (int f = 0; f < 4; ++f)
        if (dst[f])
            ML_HIP(hipMemcpyAsync(dst[f], (char *)ctx->fields.set_ptr() + f * plane_bytes, plane_bytes,
                                  hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

int ml_fields_upload(ml_ctx *ctx, int nx, int ny, const double *Ex, const double *Ey,
                     const double *Hx, const double *Hy) {
    ML_REQUIRE(ctx && Ex && Ey && Hx && Hy, "NULL argument");
    ML_REQUIRE(nx >= 1 && ny >= 1, "empty grid (%d x %d)", nx, ny);
    ML_HIP(hipSetDevice(ctx->device));
    const size_t plane_bytes = (size_t)nx * ny * 2 * sizeof(double);
    ML_TRY(ctx->fields.buf.reserve(4 * plane_bytes));
    const double *src[4] = {Ex, Ey, Hx, Hy};
    ctx->fields.premod_serial = -1;
    for (int f = 0; f < 4; ++f)
        ML_HIP(hipMemcpyAsync((char *)ctx->fields.buf.p + f * plane_bytes, src[f], plane_bytes,
                              hipMemcpyHostToDevice, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    ctx->fields.nx = nx;
    ctx->fields.ny = ny;
    ctx->fields.n_sets = 1;
    ctx->fields.field_set = 0;
    ctx->caches.fields_overwritten();
    return ML_OK;
}

int ml_profile_enable(ml_ctx *ctx, int on) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ctx->prof.on = on != 0;
    return ML_OK;
}

int ml_profile_select(ml_ctx *ctx, unsigned mask) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ctx->prof.mask = mask;
    return ML_OK;
}

int ml_profile_sample(ml_ctx *ctx, int period) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(period >= 1, "period must be >= 1");
    ctx->prof.period = period;
    for (int k = 0; k < ML_K_COUNT; ++k) ctx->prof.seen[k] = 0;
    return ML_OK;
}

int ml_profile_reset(ml_ctx *ctx) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_HIP(hipSetDevice(ctx->device));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    ML_TRY(prof_harvest(ctx));
    for (int k = 0; k < ML_K_COUNT; ++k) {
        ctx->prof.launches[k] = 0;
        ctx->prof.total_ms[k] = 0;
        ctx->prof.seen[k] = 0;
    }
    return ML_OK;
}

int ml_profile_get(ml_ctx *ctx, int kernel, int64_t *launches, double *total_ms) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(kernel >= 0 && kernel < ML_K_COUNT, "kernel id %d out of range", kernel);
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(prof_harvest(ctx));
    if (launches) *launches = ctx->prof.launches[kernel];
    if (total_ms) *total_ms = ctx->prof.total_ms[kernel];
    return ML_OK;
}

}  // extern "C"
