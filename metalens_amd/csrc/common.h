// Internal declarations shared by the translation units of libmetalens_hip.so.
// gfx950 (MI355X) only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "metalens_hip.h"
#include "lens_pack.h"
#include "synth_caches.h"
#include "transform_route.h"
#include "propagate_grid.h"
#include "fields_pupil.h"
#include "propagate_modes.h"

namespace ml {

void set_error(const char *fmt, ...);

#define ML_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            ml::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                          __LINE__);                                                      \
            return (e_ == hipErrorOutOfMemory) ? ML_ENOMEM : ML_EHIP;                     \
        }                                                                                 \
    } while (0)

#define ML_REQUIRE(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            ml::set_error(__VA_ARGS__);  \
            return ML_EINVAL;            \
        }                                \
    } while (0)

#define ML_TRY(expr)          \
    do {                      \
        int rc_ = (expr);     \
        if (rc_ != ML_OK) return rc_; \
    } while (0)

// Tuning and ablation knobs exist only in the diagnostic build (make EXTRA=-DML_DIAG BUILD=build_diag
// TARGET=...): there diag_int() reads an environment variable, in the product library it is the
// default, a constant.  The product reads no environment except the test communicator switch
// (comm.hip, ML_COMM_BACKEND).
#ifdef ML_DIAG
inline int diag_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
#else
constexpr int diag_int(const char *, int dflt) { return dflt; }
#endif

// A device allocation (hipMalloc) that only grows and is freed with its owner.  Not copyable: a copy would free the
// same memory twice.  None may have static storage duration: its destructor would run after the HIP runtime's.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t want) {
        if (want <= bytes) return ML_OK;
        release();
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            set_error("hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
            p = nullptr;
            return ML_ENOMEM;
        }
        bytes = want;
        return ML_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

// A device allocation that only grows, made of PHYSICAL pieces of `piece` bytes, each an allocation of its own
// (hipMemCreate), mapped side by side into one reserved address range (hipMemMap).  What that is for: how fast 16-byte
// stores a fixed large stride apart go (the row transform's transposed result, farfield.hip stage1_fft) depends on the physical
// layout behind the buffer, which hipMalloc leaves to the driver's free lists - measured at 4096^2 -> 512^2, stage 1
// (profiles/r06_ab_runs.txt): one physically contiguous allocation 0.33 ms, pieces of 16 KB 1.28, 512 KB 0.8-1.0, 1 MB
// 0.51 (address translation: the 2 MB fragment is lost), 2 / 4 / 8 MB 0.178-0.190 in three processes of four (else
// 0.195-0.20), 32 MB 0.186; plain hipMalloc 0.183 or 0.200, one of two each, depending on what the process was handed.
// reserve() either succeeds or leaves the buffer empty and returns an error; after the first failure (out of memory,
// or a driver without the virtual-memory API) the buffer stays unavailable and reserve() fails at once - the caller
// falls back to a DevBuf.
// ADDRESS RANGES ARE NEVER GIVEN BACK.  On this runtime (ROCm 7.2) an address range that has been unmapped, freed
// (hipMemAddressFree) and handed out again by a later hipMemAddressReserve reads back wrong data: a stand-alone program
// that fills and checks a freshly mapped buffer fails from the first round whose range overlaps an earlier one (19 008
// ... 644 992 mismatching words; none when the old ranges stay reserved, tools/vmm_reuse.hip) - translations of the old
// mapping survive.  So a buffer reserves four times what it needs (at least 256 MB) and GROWS by mapping more pieces
// behind the ones it has; a buffer that outgrows its range, fails or is destroyed unmaps and releases its physical
// pieces and leaves the range reserved for the life of the process.  That holds memory too, not only address space:
// this runtime returns unmapped, released pieces only with their range (free device memory stays down by the pieces
// until hipMemAddressFree), so each abandoned range keeps the pieces that were last mapped into it.
struct PieceBuf {
    void *p = nullptr;
    size_t bytes = 0;
    const size_t piece;
    explicit PieceBuf(size_t piece_bytes) : piece(piece_bytes) {}
    PieceBuf(const PieceBuf &) = delete;
    PieceBuf &operator=(const PieceBuf &) = delete;
    ~PieceBuf() { drop(); }
    int reserve(size_t want) {
        if (want <= bytes) return ML_OK;
        if (failed != ML_OK) return failed;
        const int rc = grow(want);
        if (rc != ML_OK) {
            (void)hipGetLastError();
            drop();
            failed = rc;
        }
        return rc;
    }
    template <typename T>
    T *as() const { return reinterpret_cast<T *>(p); }

  private:
    std::vector<hipMemGenericAllocationHandle_t> handles;   // the pieces behind p
    void *base = nullptr;    // the reserved range (p, once a piece is mapped) ...
    size_t va_bytes = 0;     // ... of this many bytes
    int failed = ML_OK;      // the error of the first failed reserve(): never tried again

    int grow(size_t want) {
        int dev = 0;
        ML_HIP(hipGetDevice(&dev));
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = dev;
        size_t gran = 0;
        ML_HIP(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
        ML_REQUIRE(gran && piece % gran == 0, "pieces of %zu bytes are not a multiple of the granularity %zu", piece,
                   gran);
        const size_t total = (want + piece - 1) / piece * piece;
        if (total > va_bytes) {   // a new range; the old one (if any) stays reserved
            drop();
            const size_t va = std::max(4 * total, (size_t)256 << 20);
            ML_HIP(hipMemAddressReserve(&base, va, piece, nullptr, 0));
            va_bytes = va;
        }
        hipMemAccessDesc acc = {};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        while (bytes < total) {
            hipMemGenericAllocationHandle_t h;
            ML_HIP(hipMemCreate(&h, piece, &prop, 0));
            void *at = static_cast<char *>(base) + bytes;
            const hipError_t e = hipMemMap(at, piece, 0, h, 0);
            if (e != hipSuccess) {
                (void)hipMemRelease(h);
                set_error("hipMemMap failed: %s", hipGetErrorString(e));
                return ML_EHIP;
            }
            handles.push_back(h);
            p = base;
            bytes += piece;
            ML_HIP(hipMemSetAccess(at, piece, &acc, 1));
        }
        return ML_OK;
    }
    // unmap and release the physical pieces; the address range stays reserved (see above)
    void drop() {
        if (!handles.empty()) {
            (void)hipDeviceSynchronize();   // (as hipFree would: launches still in flight may use the range)
            for (size_t k = 0; k < handles.size(); ++k) {
                (void)hipMemUnmap(static_cast<char *>(base) + k * piece, piece);
                (void)hipMemRelease(handles[k]);
            }
            (void)hipGetLastError();
            handles.clear();
        }
        p = nullptr;
        bytes = 0;
    }
};

// (lens_pack.h: the limits and the records the near-field kernels read - MAX_SLOTS, TableDesc, CollDesc, RingBucket,
// CellRec, the cell-block constants - and HostTable, the host's copy of a table)
struct TableSlot : HostTable {   // (lens_pack.h: what the packing reads) and the table as uploaded
    DevBuf axis0, axis1, values, order_k;
};

struct KernelTimer {
    hipEvent_t start = nullptr, stop = nullptr;
};

struct Profile {
    bool on = false;
    unsigned mask = 0xffffffffu;   // bit k: kernel id k is timed while `on`
    int period = 1;                // every period-th launch of a selected kernel is timed
    int64_t seen[ML_K_COUNT] = {0};
    int64_t launches[ML_K_COUNT] = {0};
    double total_ms[ML_K_COUNT] = {0};
    // events are recorded around each launch and harvested lazily
    struct Pending {
        int kernel;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
};

// One axis of a plan whose direction grid sits on the aperture's FFT lattice (zfft.hip): the
// transform along that axis runs as an output-pruned FFT instead of a GEMM.
struct ZfftAxis : ZfftAxisGeo {   // (transform_route.h: the axis' facts)
    DevBuf tw;
    DevBuf wk, pj, kbin;   // per-bin Horner ratio, origin phasor, reduced bin (zfft.hip FftArgs)
};

// The tables of the folded (even/odd) GEMM along one centre-symmetric direction axis (zfold.hip), over the S half-
// directions of the plan's facts: farfield_plan.hip plan_fold_axis uploads v, fold_tables fills the rest.
struct FoldAxis {
    bool has_E = false;        // u_c != 0: the input modulation E exists
    DevBuf v;                  // the split directions (transform_route.h FoldSplit::v) ...
    std::vector<double> h_v;   // ... and the host's copy of them
    DevBuf cm, sm;             // real [T][S]: cos / sin of kappa p_t v_s over the T pairs of resident samples
    DevBuf r4;                 // real [2][S]: the rotation that advances cm / sm by four samples
    DevBuf E, D;               // complex [samples] input modulation, complex [directions] output diagonal
};

// the folded stage 2 leaves its split-K slabs in fold2_ot; they are summed, transposed and signed into `vectors` by
// whoever needs the vectors next - the projection does it in the same kernel (farfield_project.hip flush_unfold /
// unfold_project_kernel); the transform only records it here.  What that consumer needs to know:
struct DeferredUnfold {
    bool pending = false;
    int splits = 1, accumulate = 0;
    double alpha[4] = {0, 0, 0, 0};
};

struct FarfieldPlan : PlanFacts {   // (transform_route.h: the facts a call's route is decided from)
    bool ready = false;
    ZfftAxis fft_y, fft_x;
    DevBuf fft_tw1;
    // column pass of an interleaved row shard (farfield.hip stage2_interleaved): tables of its `block` short
    // transforms and what they were built for (plan serial, block, ranks, rank)
    DevBuf il_wk, il_pj, il_kbin;
    Stamp<4> il_for;
    int il_pad1 = 0, il_pad2 = 0;
    long serial = 0;   // incremented by every ml_farfield_plan call
    bool amplitudes_reduced = false;   // ml_farfield_project_reduce ran on the current vectors
    // ... and left the amplitudes RANK-BLOCKED when amp_rows > 0: blocks of amp_rows direction rows, both
    // planes of a block contiguous (what a reduce-scatter deals to the ranks; farfield_project.hip ProjArgs);
    // amp_gathered: every rank holds every block's sum (and the whole power map), not only its own
    int amp_rows = 0;
    bool amp_gathered = true;
    double dxp = 0, dyp = 0, wavelength = 0, n_glass = 0;
    DevBuf ux, uy;       // direction cosines
    DevBuf tw_x;         // complex [mx][nx_total]   exp(-i k x' ux)   (A operand of stage 2)
    DevBuf tw_y;         // complex [ny][my]         exp(-i k y' uy)   (B operand of stage 1)
    DevBuf stage1;       // complex [4][nx_local][my], or transposed (transform_route.h GLayout) ...
    PieceBuf stage1_pieces{(size_t)4 << 20};   // ... the transposed one of rows up to 8192 samples
    DevBuf vectors;      // complex [4][mx][my]  (Nx, Ny, Lx, Ly)  or [4][mx] for a pair list
    DevBuf power;        // double  [mx][my]
    // complex [2 slots][2][mx][my]  (a_theta, a_phi).  Two slots: with a communicator the
    // all-reduce of step k's amplitudes runs on its own stream while step k + 1 is synthesised
    // and projects into the other slot (ml_farfield_project_reduce)
    DevBuf amplitudes;
    int amp_slot = 0;
    double *amp_ptr() const { return reinterpret_cast<double *>(amplitudes.p) + (size_t)amp_slot * 4 * directions(); }
    bool have_vectors = false;
    bool tw_x_ready = false;  // complex x twiddles built for the current plan
    int stage1_splits = 1;   // split-K slabs currently held in `stage1`
    std::vector<double> h_ux, h_uy;   // host copies of the plan's inputs
    // folded stage 1 along y (uy centre-symmetric) and folded stage 2 along x (centre-symmetric ux and a mirror-
    // symmetric set of resident rows): the facts are PlanFacts::fold / fold_S and fold2 / fold2_S
    FoldAxis fold_y, fold_x;
    // stage 2's own: the transposed stage-1 result and its split-K output slabs
    DevBuf fold2_gt, fold2_ot;
    // the stage-2 tables depend on the plan and on which rows are resident: rebuilt only when
    // that changes (serial, row0, resident rows, mirrored)
    Stamp<4> fold2_for;
    DeferredUnfold unfold;
};

// The range the phase arithmetic is tested over and the entries enforce (nearfield_math.h sincos_cw, reduce_pio2): an
// argument k R of magnitude up to 1e9.  Beyond 2^31 pi/2 = 3.4e9 the quadrant count leaves the int range and the phase
// is wrong without a sign of it, so a geometry that can reach past the limit is refused where it is set up.
constexpr double PHASE_LIMIT = 1e9;

// Where the targets of a propagation plan lie: their bounding box minus the aperture's origin (x0, y0), and the
// largest z
struct PropExtent {
    double tx_lo = 0, tx_hi = 0, ty_lo = 0, ty_hi = 0, z_hi = 0;
};

// the largest distance a pass can meet between a sample (i dxp, j dyp) of an nx x ny aperture and a point of the box
inline double prop_largest_R(const PropExtent &e, int nx, int ny, double dxp, double dyp) {
    const double ax = (nx - 1) * dxp, ay = (ny - 1) * dyp;
    const double dx = std::max(std::max(std::fabs(e.tx_lo), std::fabs(e.tx_hi)),
                               std::max(std::fabs(e.tx_lo - ax), std::fabs(e.tx_hi - ax)));
    const double dy = std::max(std::max(std::fabs(e.ty_lo), std::fabs(e.ty_hi)),
                               std::max(std::fabs(e.ty_lo - ay), std::fabs(e.ty_hi - ay)));
    return std::sqrt(dx * dx + dy * dy + e.z_hi * e.z_hi);
}

// ML_EINVAL, with the distance, k R and the limit in the message, unless k R <= PHASE_LIMIT for every pair of such a
// pass (k = 2 pi n_glass / wavelength); a NaN is refused too
inline int prop_check_phase(const char *who, const PropExtent &e, int nx, int ny, double dxp, double dyp, double wavelength,
                            double n_glass) {
    const double R = prop_largest_R(e, nx, ny, dxp, dyp), kR = 2.0 * M_PI * n_glass / wavelength * R;
    ML_REQUIRE(kR <= PHASE_LIMIT, "%s: a target can lie %.6g m from a sample of the %d x %d aperture, k R = %.6g: the phase "
               "arithmetic covers k R up to %g", who, R, nx, ny, kR, PHASE_LIMIT);
    return ML_OK;
}

// Targets and buffers of the finite-distance propagator (propagate.hip).  Its own: nothing here is shared with the
// far-field plan, the radiation vectors or the sweep sums.
struct PropagatePlan {
    bool ready = false, have_result = false, have_sums = false;
    bool have_stokes = false;   // stokes_sums hold a pass (ml_propagate_accumulate_stokes); cleared with have_sums by every plan
    int T = 0, want_h = 1;
    int result_sets = 0;   // field sets in `result`: 1 after ml_propagate, n after ml_propagate_sets
    double x0 = 0, y0 = 0, dxp = 0, dyp = 0, wavelength = 0, n_glass = 0;
    PropExtent extent;   // of the targets: every pass checks it against the shape it meets (prop_check_phase)
    DevBuf targets;   // double [5][T]: x - x0, y - y0, z of every target, then the low parts of x - x0 and y - y0 (propagate_direct.h)
    DevBuf partial;   // double [splits][sets][12 or 6][T]: the aperture's row sets, summed by the second pass in their order
    DevBuf result;    // complex [sets][6 or 3][T]: Ex, Ey, Ez (, Hx, Hy, Hz) of every set of the last pass
    DevBuf sums;      // double [2][T]: weighted sums of |E|^2 and of Sz over the passes since the last reset (ml_propagate_accumulate)
    // the FFT form (propagate_grid_plan.hip ml_propagate_plan_grid*; passes: propagate_grid.hip and the files it hands
    // over to): targets (x0 + tx_off + i dxp, y0 + ty_off + j dyp, z)
    int method = 0;   // ML_PROPAGATE_DIRECT / ML_PROPAGATE_FFT / ML_PROPAGATE_FFT_LONG / ML_PROPAGATE_FFT_TILED / ML_PROPAGATE_FFT_FINE / ML_PROPAGATE_FFT_STACK
    GridPlanFacts grid;   // (propagate_grid.h) for the aperture shape last met; spectra_ready: its kernel spectra are in grid_work
    bool spectra_ready = false;
    double tx_off = 0, ty_off = 0, z = 0;
    // the tiled plan (ml_propagate_plan_grid_tiled): the tile lengths asked for (0: the default) and the plan for the
    // aperture shape last met; grid.Lx, grid.Ly are then the TILE lengths (what the transform launchers read)
    int tile_lx = 0, tile_ly = 0;
    GridTilePlan tile;
    // the fine plan (ml_propagate_plan_grid_fine): what was asked for - the ratios, the fine counts and the mode in
    // `fine`, the lattices' origins minus (x0, y0) - and the plan for the aperture shape last met (fine.tile; `tile` is a
    // copy of it, for ml_propagate_plan_tiles).  grid.mx, grid.my are then the counts PER LATTICE, T the fine targets
    GridFinePlan fine;
    double fine_tx[GRID_FINE_S_MAX] = {}, fine_ty[GRID_FINE_S_MAX] = {};
    // the stack plan (ml_propagate_plan_grid_stack; propagate_stack.hip): a fine plan - `fine`, `tile`, the origins above -
    // in the planes stack_z; T is then planes x fine targets, `z` the largest plane.  stack_layers: the device's table of
    // the layers (plane, lattice) in contraction order, uploaded by the plan entry
    std::vector<double> stack_z;
    DevBuf stack_layers;
    // complex [8 kernel spectra + 4 currents + 6 or 3 outputs][Lx][Ly]; the tiled plan: [tiles][8] kernel spectra,
    // [batch][4] currents, [6 or 3] outputs; the fine plan: [lattices][tiles][8] (or [2][batch][8]) kernel spectra,
    // [tiles][4] currents, [2][6 or 3] outputs, and the stack plan the same with its layers for the lattices; released by
    // a direct plan.  Where the parts begin: grid_work_plain, grid_work_tiled, grid_work_layered below
    DevBuf grid_work;
    DevBuf grid_tw_x, grid_tw_y;   // (cos, sin) of 2 pi j / L, j < L / 2, per axis
    // the focus metrics (propagate_focus.hip, ml_propagate_focus): the chunks' partial records [planes][chunks][FOCUS_PARTIAL],
    // the planes' records and the centres [planes][2] the radii are taken about; they read result and sums and change neither
    DevBuf focus_partial, focus_records, focus_centre;
    // the Stokes records (propagate_stokes.hip, ml_propagate_stokes): the weighted sums [5][T] of S0, S1, S2, S3 and |Ez|^2 over
    // the passes since the last reset (ml_propagate_accumulate_stokes), the chunks' partial records [planes][chunks][STOKES_PARTIAL],
    // the planes' records and the centres [planes][2]; they read the result and change nothing but their own sums
    DevBuf stokes_sums, stokes_partial, stokes_records, stokes_centre;
    // the transfer function (propagate_otf.hip, ml_propagate_otf): the phasor tables Tx[mx][nu], Ty[my][nv], the row sums
    // R[2][planes][mx][nv] and the device copy of the output [planes][2][nu][nv]; it reads result and sums and changes neither
    DevBuf otf_tables, otf_rows, otf_out;
    // the mode overlaps (propagate_modes.hip, ml_propagate_modes_plan / _queue / _fetch): what is planned, the conjugated
    // tables Tx[mx][nu], Ty[my][nv], the row sums R[4 or 2][planes][mx][nv] and the output slots [n_slots][planes][4][nu][nv].
    // The tables belong to the plan: every ml_propagate_plan* entry drops them (modes.planned).  They read the result and
    // change nothing but their own slots
    ModesState modes;
    DevBuf modes_tables, modes_rows, modes_out;
};

// The parts of PropagatePlan::grid_work in planes of ps = grid.Lx grid.Ly elements, one function per layout: what a
// prepare fills and what its pass reads.  k_layer: the elements from a lattice's (a layer's) kernel spectra to the next.
struct GridWork {
    double2 *K, *cur, *out;
    size_t k_layer;
};
inline GridWork grid_work_at(const PropagatePlan &pp, size_t k_layer, size_t k_layers, size_t cur_tiles) {
    const size_t ps = (size_t)pp.grid.Lx * pp.grid.Ly;
    double2 *K = pp.grid_work.as<double2>(), *cur = K + k_layers * k_layer;
    return {K, cur, cur + cur_tiles * GRID_CURRENTS * ps, k_layer};
}
inline GridWork grid_work_plain(const PropagatePlan &pp) {   // [8][4][6 or 3]
    return grid_work_at(pp, (size_t)GRID_KERNELS * pp.grid.Lx * pp.grid.Ly, 1, 1);
}
inline GridWork grid_work_tiled(const PropagatePlan &pp) {   // [tiles][8], [batch][4], [6 or 3]
    return grid_work_at(pp, (size_t)pp.tile.tiles * GRID_KERNELS * pp.grid.Lx * pp.grid.Ly, 1, pp.tile.batch);
}
// `layers`: the lattices of a fine plan, planes x lattices of a stack plan.  cached: [layers][tiles][8]; streamed:
// [2][batch][8]; then [tiles][4], [2][6 or 3]
inline GridWork grid_work_layered(const PropagatePlan &pp, int layers) {
    const GridTilePlan &t = pp.fine.tile;
    const bool cached = pp.fine.cache_kernels;
    return grid_work_at(pp, (size_t)(cached ? t.tiles : t.batch) * GRID_KERNELS * pp.grid.Lx * pp.grid.Ly,
                        cached ? layers : GRID_FINE_PAIR, t.tiles);
}

// What the kernels read about the lens (lens_pack.h lays it out, ctx.hip uploads it): the tables, the layout and what is
// packed from both.  The scalars are held as the packers return them.
struct Lens {
    // tables
    TableSlot slots[MAX_SLOTS];
    TableSlot center;
    DevBuf table_desc;                       // TableDesc[MAX_SLOTS + 1], last = centre
    std::vector<TableDesc> h_table_desc;     // host copy of table_desc
    TableDesc h_center_desc;                 // the centre entry again: it travels in the kernel arguments
    bool tables_dirty = true;
    // which kernel takes which table's samples (classify_lens): cls.simple - SOME table in use holds orders (ox, 0),
    // |ox| <= 5 only, its samples take nearfield_simple.hip - and the others the general kernel
    LensClass cls;
    // packed from tables and layout (refresh_ring_locations)
    DevBuf ring_rec, ring_coll;              // 4 doubles per ring; dense collection number per ring
    DevBuf ring_tab, ring_ok, ring_ok_off;   // fast-kernel per-ring tables (offsets into ring_tab: ring_rec)
    DevBuf center_qmajor;                    // fast-kernel centre table [order][n0][n1][4][K]
    CentreSlots centre;                      // (pack_centre_table)
    CollDesc h_coll[MAX_RING_COLLS] = {};
    double ring_bounds_all[4] = {0, 0, 0, 0};   // intersection of the ring tables' (ux', uy') bounds (NfArgs)

    // layout
    bool have_layout = false;
    int n_rings = 0, n_cells = 0;
    std::vector<double> h_ring_period, h_ring_lateral, h_ring_rc;
    std::vector<int32_t> h_ring_gc, h_ring_coll;   // slot and dense collection number per ring (dense_collections)
    int n_colls = 0;
    int32_t coll_slot[MAX_RING_COLLS] = {0};       // dense collection number -> slot
    DevBuf ring_boundaries, ring_r_center, ring_period, ring_dphi, ring_lateral, ring_gc;
    DevBuf rot_table, tie_table, ring_rot_center, ring_rot_half;
    DevBuf ring_lut;       // uniform-in-r bucket -> first candidate boundary
    DevBuf ring_lutrec;    // fast kernel: coarser buckets that carry the boundaries
    RingSearchFacts search;
    DevBuf cell_x, cell_y, cell_xy, cell_which, cell_index, bin_start;
    BinFacts bins;
    std::vector<int32_t> h_slot_of_cell;   // original cell index -> bin-sorted slot
    // nearest-cell lattice shortcut (fit_lattice): cells = nodes c0 + a b1 + b b2
    LatticeFacts lattice;
    DevBuf cell_lattice_map, cell_lattice_rec;
};

// The grid a synthesis runs on and what is derived from grid and lens alone; synth_caches.h says when each is rebuilt.
struct SynthGrid {
    DevBuf x_pts, y_pts;
    std::vector<double> h_x_pts, h_y_pts;   // what x_pts / y_pts hold (re-uploaded only on change)
    DevBuf row_first;                       // see row_extent_kernel
    int trim_rows[2] = {0, 0};              // rows of the local aperture that meet the lens circle, [lo, hi) - farfield.hip trim_rows_of
    // per-sample geometry records and the four patch lists (nearfield_geometry.hip; NfArgs::active_list)
    DevBuf geo_ix, active_list, active_count, active_flag;
    int n_active[4] = {0, 0, 0, 0};         // the lists' lengths, once SynthCaches::lengths == KNOWN
};

// exact nearest-cell ties (nearfield_geometry.hip settle_tie): samples the last synthesis could not settle, and the host's
// answers for the current (grid, layout)
struct Ties {
    DevBuf count, list, ovr_key, ovr_slot;
    int n_ovr = 0;
};

// resident field sets: complex [n_sets][4][nx][ny] (one set per member of a polarisation batch); the far-field and
// download entry points work on set `field_set`
struct FieldSets {
    DevBuf buf;
    int nx = 0, ny = 0, n_sets = 1, field_set = 0;
    double *set_ptr() const { return reinterpret_cast<double *>(buf.p) + (size_t)field_set * 4 * nx * ny * 2; }
    // ml_nearfield_premodulate: serial of the plan whose stage-1 input modulation the sets carry (-1: none)
    long premod_serial = -1;
};

// what a synthesis leaves besides the fields
struct SynthOut {
    DevBuf partial_power, power, violations;
    // bound-violation keys are double-buffered: the synthesis kernel that fills one half clears
    // the other for the next launch (no separate memset per call)
    int viol_half = 0;
    bool viol_zeroed = false;
    // the per-block power partials of the last synthesis have not been summed into `power` yet:
    // the projection kernel does it in a spare block, ml_nearfield_result otherwise
    bool power_pending = false;
    int n_partials = 0;
    // which instantiation the last synthesis launched for the ring samples of narrow collections and for the centre
    // samples (ml_nearfield_synth_info): 0 none, 1 general, 2 fixed-shape (nearfield_simple.hip FIXED3)
    int ring_form = 0, centre_form = 0;
};

}  // namespace ml

struct ml_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    char arch[64] = {0};
    int cu_count = 0;
    int64_t hbm_bytes = 0;

    ml::Lens lens;
    ml::SynthGrid grid;
    ml::Ties ties;
    ml::FieldSets fields;
    ml::SynthOut out;
    ml::SynthCaches caches;
    // the patch lists' lengths on their way back (page-locked; queued right behind the scans that make them, so that
    // the second synthesis on a geometry finds them there instead of draining the stream for four integers)
    int *counts_pinned = nullptr;
    hipEvent_t counts_ready = nullptr;

    // far-field sums kept on the GPU across the sources of a sweep (farfield_sums.hip, ml_farfield_accumulate)
    ml::DevBuf acc_P, acc_partials, acc_sums;
    // the plan P_sum was accumulated on: its direction count and kind (0 directions: nothing accumulated yet).  acc_P is
    // sized by it, so adding onto it or reading it under a plan of another size or kind is refused
    size_t acc_n = 0;
    int acc_pair_list = 0;
    // beam metrics of the far field (farfield_beam.hip, ml_farfield_beam): the chunks' partial records of the call in flight,
    // and the slots' records - a buffer of its own, not acc_sums
    ml::DevBuf beam_partials, beam_records;
    // per-zone sums of the resident near field (fields_zones.hip, ml_fields_zones): the call's axis arrays and edges, the
    // lines' run lists with their counts, and the device copy of the records
    ml::DevBuf zones_in, zones_runs, zones_records;
    // per-zone contributions to the field at points behind the aperture (fields_zone_fields.hip, ml_fields_zone_fields): the
    // call's axis arrays, edges and targets, the run lists of one walk with their counts, and a set's records and members
    ml::DevBuf zf_in, zf_runs, zf_records;
    // Zernike moments of the resident near field's wavefront (fields_wavefront.hip, ml_fields_zernike): the call's axis
    // arrays, the line records, and the sets' monomial moments
    ml::DevBuf wavefront_in, wavefront_lines, wavefront_records;
    // the pupil function applied to the resident near field (fields_pupil.hip, ml_fields_pupil_plan / _apply): the plan's
    // axis arrays, line table, edges and factors, and what the plan was made for; it stays until the next plan
    ml::DevBuf pupil_in;
    ml::PupilPlan pupil;
    ml::DevBuf lattice_in;  // staging for ml_farfield_lattice_power
    int gemm_f32 = 0;   // ml_farfield_set_precision: folded GEMMs on the fp32 matrix cores
    int ff_method = 0;  // ml_farfield_set_method: 0 auto (FFT on lattice grids), 1 GEMMs only
    bool premod_enabled = false;   // ml_nearfield_premodulate: the synthesis applies the active plan's stage-1 input modulation

    ml::FarfieldPlan plan;
    ml::PropagatePlan prop;
    ml::Profile prof;

    // RCCL.  comm_stream carries the all-reduce of the projected amplitudes and the power kernel
    // behind it; amp_ready[s] / reduce_done[s] order it against the main stream per amplitude slot
    hipStream_t comm_stream = nullptr;
    hipEvent_t amp_ready[2] = {nullptr, nullptr}, reduce_done[2] = {nullptr, nullptr};
    bool reduce_in_flight = false;
    bool reduce_by_allreduce = false;   // ml_comm_set_reduce: all-reduce instead of reduce-scatter (comparison runs)
    void *comm = nullptr;
    int comm_max_channels = 4;   // ncclConfig_t::maxCTAs of the communicator ml_comm_init makes (0: RCCL's own choice)
    int n_ranks = 1, rank = 0;
    // ML_COMM_BACKEND=file: TEST backend, all-reduce through files in /tmp (several ranks may
    // then share one GPU, which RCCL refuses); never used unless asked for
    bool comm_file = false;
    std::string comm_file_key;
    long comm_file_seq = 0;
    ml::DevBuf comm_scratch;
};

namespace ml {

// profile helpers (ctx.hip)
void prof_begin(ml_ctx *ctx, int kernel, hipEvent_t *a, hipEvent_t *b, hipStream_t stream = nullptr);
void prof_end(ml_ctx *ctx, int kernel, hipEvent_t a, hipEvent_t b, hipStream_t stream = nullptr);
int prof_harvest(ml_ctx *ctx);

struct ProfScope {
    ml_ctx *ctx;
    int kernel;
    hipStream_t stream;   // the stream the timed work is queued on (default: the context's)
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(ml_ctx *c, int k, hipStream_t s = nullptr) : ctx(c), kernel(k), stream(s) {
        prof_begin(ctx, kernel, &a, &b, stream);
    }
    ~ProfScope() { prof_end(ctx, kernel, a, b, stream); }
};

// zgemm.hip: C[M][N] (+)= alpha * A[M][K] * B[K][N], complex128 interleaved, row-major.
// batch > 1 strides A, B, C by the given element (complex) strides.
// alpha[batch] are real scale factors, one per batch entry (batch <= 4).
int zgemm(hipStream_t stream, int M, int N, int K, const double *alpha, const double *A,
          int64_t lda, int64_t strideA, const double *B, int64_t ldb, int64_t strideB, double *C,
          int64_t ldc, int64_t strideC, int batch, int accumulate);
// out[f][d] (+)= alpha[f] * sum_j TX[d][j0 + j] * G[f][j][d]   (pair-list stage 2)
int zcoldot(hipStream_t stream, int n_fields, int rows, int cols, const double *alpha4,
            const double *TX, int64_t ldtx, int j0, const double *G, double *out, int accumulate);
// how zfold_stage1 reads and writes (defaults: one input array, row-major output)
struct FoldIO {
    int in_slabs = 1;            // A is the sum of this many arrays ...
    int64_t in_slab_stride = 0;  // ... this many complex elements apart
    int out_t_rows = 0;          // > 0: write C transposed per field, see zfold.hip FoldArgs
    const double *out_E = nullptr;  // with out_t_rows: complex [out_t_rows], multiplied into row n1
};
// zfold.hip: stage 1 with both mirror symmetries folded (real cos/sin kernel)
int zfold_stage1(hipStream_t stream, int M, int ny, const double *A, int64_t lda, const double *Cm,
                 const double *Sm, const double *R4, int T, int S, const double *E,
                 const double *D, double *C, int64_t ldc, int my, const int *row_first = nullptr,
                 int nxl = 1, int ksplit = 1, int64_t split_stride = 0, bool f32 = false,
                 FoldIO io = FoldIO());
// number of split-K slabs zfold_stage1 will actually write for (T, ksplit)
int zfold_splits(int T, int ksplit);
// zfft.hip: output-pruned FFT along one axis for lattice-commensurate direction grids
struct ZfftCall {
    int N_eff = 0, n_valid = 0, M = 0, j0 = 0, pad1 = 0, pad2 = 0;
    int jstep = 1;
    const double *in = nullptr;   // complex
    int64_t in_s1 = 0, in_s2 = 0, in_es = 0;
    int in_rb = 0, a0 = 0, h0 = 0, a1 = 0, h1 = 0;
    const int *row_first = nullptr;
    int rf_mod = 0;
    int sub_s = 1, sub_i = 0;   // this launch: samples sub_i, sub_i + sub_s, ... of the axis (two-level)
    double *out = nullptr;      // complex
    int64_t out_s1 = 0, out_s2 = 0, out_es = 0;
    int out_rb = 0;
    const double *tw1 = nullptr, *wk = nullptr, *pj = nullptr;
    const int *kbin = nullptr;
    double alpha[4] = {0, 0, 0, 0};
    int alpha_rb = 0, rows = 0, accumulate = 0;
    int passes = 0;                  // > 1: the pass-split kernel (0: the library's default)
    int second = 0;                  // contiguous rows that are the SECOND stage (of a transposed stage-1 result)
    int tiled_out = 0;               // bins stored in tiles of 8 (zfft_core.h tile_off; out_es = the tile's stride)
    int mixA = 0, mixB = 0;          // > 0: N_eff = mixA mixB R through zfft_mixed_kernel, tw1 = the axis' [B][A] table
};
// the column pass over a tiled stage-1 result (zfft.hip zfft_tiles_kernel)
int zfft_run_tiles(hipStream_t stream, const ZfftCall &c);
// tw1: [B][A] W_AB^(n1 k2) - 16 x 16 for the 256 R3 scheme, the legs of a mixed-radix axis otherwise
int zfft_build_tables(hipStream_t stream, double *tw1, double *wk, double *pj, int *kbin, int M,
                      int j0, int N_eff, int c, int jstep = 1, int A = 16, int B = 16);
// the padding of a mixed-radix axis' exchange layout with the fewest LDS conflict cycles
int zfft_choose_pad_mixed(int A, int B, int R, int M, int j0, int jstep);
void zfft_choose_pads(int N_eff, int M, int j0, int *pad1, int *pad2, int jstep = 1);
// the column pass of an interleaved shard: s short transforms per column in one workgroup; c.pj holds
// [s][M] phasors, sub-sequence i starts sub_off elements behind sub-sequence i - 1
// (stuff > 1: the transforms have c.N_eff / stuff samples and run zero-stuffed at c.N_eff)
int zfft_run_interleaved(hipStream_t stream, const ZfftCall &c, int s, int64_t sub_off, int stuff);
int zfft_build_interleave_tables(hipStream_t stream, double *wk, double *pj, int *kbin, int M, int j0, int Nsub,
                                 int N, int c, int first, int block, int jstep = 1);
int zfft_run(hipStream_t stream, const ZfftCall &c);
// comm.hip
void comm_release(ml_ctx *ctx);
// farfield_plan.hip: undo ml_nearfield_premodulate on the resident fields (no-op if plain)
int fields_unmodulate(ml_ctx *ctx);
// farfield_plan.hip, plan tables the transform builds on first use: the folded stage 2's phase tables for the resident
// rows (the split-K factor through *want_split), and the complex x twiddles of the generic stage 2 / the column dot
int stage2_tables(ml_ctx *ctx, int row0, int mirrored, int *want_split);
int need_tw_x(ml_ctx *ctx);
// farfield_project.hip: write the radiation vectors a folded stage 2 left in split-K slabs (no-op if none)
int flush_unfold(ml_ctx *ctx);
// farfield_beam.hip: what the checks of farfield_beam.h read of a context (ml_farfield_beam, the sweep sums)
struct BeamState;
BeamState beam_state(const ml_ctx *ctx);
// propagate_grid.hip: the pass of propagate.hip's propagate_sets for a plan of ml_propagate_plan_grid* (checks done); it
// hands the tiled, the fine and the stack plan over to their files (propagate_grid_launch.h)
int propagate_grid_sets(ml_ctx *ctx, double Z0, int first, int n);
// in-place sum of `count` doubles over the communicator, queued on `stream` (no-op without one)
int comm_allreduce_sum(ml_ctx *ctx, double *buf, size_t count, hipStream_t stream);
// buf = n_ranks chunks of `chunk` doubles: afterwards chunk `rank` holds the sum over the ranks of
// their chunk `rank` (the other chunks are scratch) / every chunk r holds rank r's chunk r
int comm_reduce_scatter_sum(ml_ctx *ctx, double *buf, size_t chunk, hipStream_t stream);
int comm_allgather(ml_ctx *ctx, double *buf, size_t chunk, hipStream_t stream);
// the main stream (and the host, if `host`) waits for a reduction still running on comm_stream
int comm_join(ml_ctx *ctx, bool host);

// nearfield.hip: synthesis of a batch of n sources that differ in polarisation only
// members_alone: every member through the single-source kernels, also when all share one position; keep_powers: the
// incident powers of the synthesis before stay what ml_nearfield_powers returns (ml_nearfield_members_async)
int nearfield_launch(ml_ctx *ctx, const ml_nearfield_params *p, int n, int nx, int ny, bool members_alone = false,
                     bool keep_powers = false);
// sum the pending power partials now (no-op if none are pending)
int power_flush(ml_ctx *ctx);
// ML_NO_PLAN_CACHE=1: rebuild every geometry-only table on every call (for timing them)
bool plan_cache_disabled();
// Incident-power reduction, second level: the per-block partials of the synthesis kernel are
// summed in POWER_GROUPS contiguous groups (group g = partial[g*n/G .. (g+1)*n/G), one
// 256-thread block per group at a time, fixed order inside the group); the host adds the
// POWER_GROUPS group sums in order.  Deterministic, and no single block walks all partials.
constexpr int POWER_GROUPS = 32;
__device__ __forceinline__ void sum_partials_group(const double *partial, int n, double *groups,
                                                   int g, int tid) {
    __shared__ double s_part[256];
    const int lo = (int)((long long)n * g / POWER_GROUPS), hi = (int)((long long)n * (g + 1) / POWER_GROUPS);
    double acc = 0.0;
    for (int k = lo + tid; k < hi; k += 256) acc += partial[k];
    __syncthreads();   // s_part may still be read by the previous group's tree
    s_part[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) s_part[tid] += s_part[tid + w];
        __syncthreads();
    }
    if (tid == 0) groups[g] = s_part[0];
}

}  // namespace ml
