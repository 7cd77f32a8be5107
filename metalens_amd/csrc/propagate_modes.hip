// The overlap of a propagated image with separable modes, contracted where the image lies: per plane of the active
// propagation plan's resident result and per component F in (Ex, Ey, Hx, Hy) of one member of the last pass
//   O_F[p][a][b] = sum_i sum_j conj(mode_x[a][i]) conj(mode_y[b][j]) F(p, i, j)
// (ml_propagate_modes_plan / _queue / _fetch) - how much of the light enters a fibre mode, a Gaussian beam, a Hermite-Gauss
// order -, without the image crossing PCIe.  The order of the sums, the launch shapes, the checks and the caps:
// propagate_modes.h.  The reference has no counterpart.
//
// The plan entry uploads the conjugated tables Tx[mx][nu], Ty[my][nv] and reserves the row sums and the output slots; a
// queue call is two launches into its slot, no atomics, no synchronisation.
//   Rows.    A workgroup of 256 lanes takes one row i of one plane (grid: mx x planes) in tiles of 512 targets - two rows
//            in tiles of 128 where nv > 8, which shares every table entry a lane loads between them and changes no sum.
//            The lanes load the tile's fields once in coalesced 16-byte loads - 64 bytes per target with H, 32 without;
//            Ez and Hz are never read - and leave them in the LDS, where they serve all nv modes.  Then a lane takes a
//            (segment, mode) pair: the 32 terms of the segment one after another, the four components beside each other.
//            The segments' sums wait in the LDS for the one lane per (row, component, re / im, mode) that adds them in
//            their order to its running sum.  R[F][p][i][b], mx nv complex per plane and component, goes to memory.
//   Columns. A workgroup per (a, component, plane): the same two levels over the rows.
// The segments of a row lie 33 complex numbers apart in the LDS: lanes that walk different segments in step (few modes)
// read different banks with their 16-byte reads, lanes that share a segment (many modes) read one address.
// LDS per workgroup: 41.5 KB in the one-row kernel (three workgroups per CU), 56.5 KB in the two-row kernel (two).
#include <vector>

#include "common.h"
#include "propagate_modes.h"

#pragma clang fp contract(off)

namespace ml {

constexpr int MODES_THREADS = 256;
constexpr int MODES_SEG_PITCH = MODES_SEGMENT + 1;   // complex numbers between two segments' fields in the LDS
static_assert(MODES_MAX * 2 <= MODES_THREADS, "a lane per (mode, re / im) keeps a running sum in the column pass");
static_assert(ML_MODES_MAX == MODES_MAX && ML_MAX_SWEEP_SLOTS == MODES_SLOTS_MAX, "the header's constants are the kernels'");

struct ModesRowArgs {
    const double2 *result;   // [6 or 3][T] of the member
    const double2 *ty;       // [my][nv]
    double2 *rows;           // [4 or 2][planes][mx][nv]: 4 with H, 2 without
    int T, mx, my, nv, planes;
};

// ROWS rows of a plane per workgroup: 1 in tiles of 512 targets where few modes leave the pass to the stream of the image, 2
// in tiles of 128 where many make it the stream of Ty and the arithmetic.  How the work is dealt out does not touch the
// order of a sum: the segments are the same 32 indices, added from 0, and the segments' sums are added in ascending order.
template <bool WANT_H, int ROWS>
__global__ __launch_bounds__(MODES_THREADS) void modes_rows_kernel(const ModesRowArgs a) {
    constexpr int NC = WANT_H ? 4 : 2, NQ = 2 * NC;
    constexpr int TILE = ROWS == 1 ? MODES_TILE_FEW : MODES_TILE_MANY, TILE_SEGS = TILE / MODES_SEGMENT;
    constexpr int BATCH = ROWS == 1 ? MODES_FEW : MODES_MAX;   // every mode of a call in one batch
    constexpr int LOADS = NC * ROWS * TILE / MODES_THREADS;
    static_assert(NC * ROWS * TILE % MODES_THREADS == 0 && TILE % MODES_SEGMENT == 0, "whole steps and whole segments per tile");
    __shared__ double2 s_f[NC][ROWS][TILE_SEGS * MODES_SEG_PITCH];
    __shared__ double s_part[TILE_SEGS][ROWS][NQ][BATCH];   // (re, im) of Ex, Ey (, Hx, Hy): the mode runs fastest
    __shared__ double s_run[ROWS][NQ][BATCH];
    const int tid = threadIdx.x, i0 = blockIdx.x * ROWS, plane = blockIdx.y;
    const int rows = otf_live_rows(a.mx, ROWS, blockIdx.x);
    const size_t row0 = ((size_t)plane * a.mx + i0) * a.my;   // the first row's first target
    const size_t T = (size_t)a.T;
    for (int e = tid; e < ROWS * NQ * BATCH; e += MODES_THREADS) (&s_run[0][0][0])[e] = 0.0;
    const int tiles = otf_tiles(a.my, TILE);
    for (int tile = 0; tile < tiles; ++tile) {
        const int t0 = tile * TILE, n = otf_tile_len(a.my, TILE, tile), segs = modes_segments(n);
        // the fields of the tile, once per target (a row behind the plane's last: zeros, never written out)
#pragma unroll
        for (int k = 0; k < LOADS; ++k) {
            const int e = tid + k * MODES_THREADS, c = e / (ROWS * TILE), rem = e - c * (ROWS * TILE), r = rem / TILE, l = rem - r * TILE;
            if (l >= n) continue;
            double2 f = make_double2(0.0, 0.0);
            if (r < rows) f = a.result[(size_t)(c < 2 ? c : c + 1) * T + row0 + (size_t)r * a.my + t0 + l];   // Ex, Ey, Hx, Hy of [6][T]
            s_f[c][r][(l / MODES_SEGMENT) * MODES_SEG_PITCH + (l % MODES_SEGMENT)] = f;
        }
        __syncthreads();
        for (int item = tid; item < segs * a.nv; item += MODES_THREADS) {
            const int s = item / a.nv, b = item - s * a.nv;
            const int cnt = min(MODES_SEGMENT, n - s * MODES_SEGMENT);
            const double2 *ty = a.ty + (size_t)(t0 + s * MODES_SEGMENT) * a.nv + b;
            double acc[ROWS][NQ];
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[r][q] = 0.0;
#pragma unroll 4
            for (int k = 0; k < cnt; ++k) {   // (unrolled: the loads of four terms fly together; the adds keep their order)
                const double2 t = ty[(size_t)k * a.nv];
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const double2 x = s_f[c][r][s * MODES_SEG_PITCH + k];
                        acc[r][2 * c] += x.x * t.x - x.y * t.y;
                        acc[r][2 * c + 1] += x.x * t.y + x.y * t.x;
                    }
            }
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
#pragma unroll
                for (int q = 0; q < NQ; ++q) s_part[s][r][q][b] = acc[r][q];
        }
        __syncthreads();
        for (int o = tid; o < ROWS * NQ * a.nv; o += MODES_THREADS) {   // the segments' sums in their order
            const int rq = o / a.nv, b = o - rq * a.nv, r = rq / NQ, q = rq - r * NQ;
            double run = s_run[r][q][b];
            for (int s = 0; s < segs; ++s) run += s_part[s][r][q][b];
            s_run[r][q][b] = run;
        }
        __syncthreads();   // s_part and s_f are free again
    }
    __syncthreads();   // (a plane without targets along y cannot be planned; the zeros of s_run for good measure)
    for (int o = tid; o < rows * NC * a.nv; o += MODES_THREADS) {
        const int rc = o / a.nv, b = o - rc * a.nv, r = rc / NC, c = rc - r * NC;
        a.rows[(((size_t)c * a.planes + plane) * a.mx + i0 + r) * a.nv + b] = make_double2(s_run[r][2 * c][b], s_run[r][2 * c + 1][b]);
    }
}

template <bool WANT_H>
static void modes_rows_launch(hipStream_t stream, const ModesRowArgs &a) {
    const int rows = modes_rows_per_group(a.nv);
    const dim3 grid(otf_tiles(a.mx, rows), a.planes);
    if (rows == 1)
        hipLaunchKernelGGL((modes_rows_kernel<WANT_H, 1>), grid, dim3(MODES_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL((modes_rows_kernel<WANT_H, MODES_ROWS_MANY>), grid, dim3(MODES_THREADS), 0, stream, a);
}

// O_F[p][a][b] = sum_i Tx(i, a) R_F(p, i, b): a workgroup per (a, F, p), tiles of 1024 rows, a lane per (segment, b), then a
// lane per (b, re / im) that adds the segments' sums in their order to its running sum (a register: every tile has the
// same lane).  out: the slot, [planes][4][nu][nv]
__global__ __launch_bounds__(MODES_THREADS) void modes_columns_kernel(const double2 *tx, const double2 *rows, double2 *out, int mx, int nu,
                                                                      int nv, int planes) {
    constexpr int TILE_SEGS = MODES_COLUMN_TILE / MODES_SEGMENT;
    __shared__ double s_part[TILE_SEGS][2][MODES_MAX];
    const int tid = threadIdx.x, a = blockIdx.x, c = blockIdx.y, plane = blockIdx.z;
    const double2 *R = rows + ((size_t)c * planes + plane) * mx * nv;
    double run = 0.0;
    const int tiles = otf_tiles(mx, MODES_COLUMN_TILE);
    for (int tile = 0; tile < tiles; ++tile) {
        const int t0 = tile * MODES_COLUMN_TILE, n = otf_tile_len(mx, MODES_COLUMN_TILE, tile), segs = modes_segments(n);
        for (int item = tid; item < segs * nv; item += MODES_THREADS) {
            const int s = item / nv, b = item - s * nv;
            const int i0 = t0 + s * MODES_SEGMENT, cnt = min(MODES_SEGMENT, n - s * MODES_SEGMENT);
            double re = 0.0, im = 0.0;
            for (int k = 0; k < cnt; ++k) {
                const double2 t = tx[(size_t)(i0 + k) * nu + a];
                const double2 x = R[(size_t)(i0 + k) * nv + b];
                re += x.x * t.x - x.y * t.y;
                im += x.x * t.y + x.y * t.x;
            }
            s_part[s][0][b] = re;
            s_part[s][1][b] = im;
        }
        __syncthreads();
        if (tid < nv * 2)
            for (int s = 0; s < segs; ++s) run += s_part[s][tid & 1][tid >> 1];
        __syncthreads();
    }
    if (tid < nv * 2)
        reinterpret_cast<double *>(out + (((size_t)plane * MODES_COMPONENTS + c) * nu + a) * nv + (tid >> 1))[tid & 1] = run;
}

static size_t modes_slot_entries(const ModesState &m) { return (size_t)m.planes * MODES_COMPONENTS * m.nu * m.nv; }

}  // namespace ml

using namespace ml;

extern "C" {

int ml_propagate_modes_plan(ml_ctx *ctx, int mx, int my, int planes, const double *mode_x, int nu, const double *mode_y, int nv,
                            int n_slots) {
    ML_REQUIRE(ctx, "NULL argument");
    ML_REQUIRE(ctx->n_ranks <= 1, "ml_propagate_modes_plan: this context belongs to a communicator of %d ranks", ctx->n_ranks);
    PropagatePlan &pp = ctx->prop;
    char why[320];
    if (modes_plan_check(pp.ready ? pp.T : 0, mx, my, planes, mode_x, nu, mode_y, nv, n_slots, why, sizeof why) != 0) {
        set_error("%s", why);
        return ML_EINVAL;
    }
    ML_HIP(hipSetDevice(ctx->device));
    const size_t n_tx = (size_t)mx * nu, n_ty = (size_t)my * nv;
    const size_t n_rows = (size_t)(pp.want_h ? MODES_COMPONENTS : 2) * planes * mx * nv;   // the components the row pass writes
    const size_t n_out = (size_t)n_slots * planes * MODES_COMPONENTS * nu * nv;
    // the conjugates, index-major: Tx[i][a] = conj(mode_x[a][i]), Ty[j][b] = conj(mode_y[b][j])
    std::vector<double> h(2 * (n_tx + n_ty));
    for (int a = 0; a < nu; ++a)
        for (int i = 0; i < mx; ++i) {
            h[2 * ((size_t)i * nu + a)] = mode_x[2 * ((size_t)a * mx + i)];
            h[2 * ((size_t)i * nu + a) + 1] = -mode_x[2 * ((size_t)a * mx + i) + 1];
        }
    for (int b = 0; b < nv; ++b)
        for (int j = 0; j < my; ++j) {
            h[2 * (n_tx + (size_t)j * nv + b)] = mode_y[2 * ((size_t)b * my + j)];
            h[2 * (n_tx + (size_t)j * nv + b) + 1] = -mode_y[2 * ((size_t)b * my + j) + 1];
        }
    // (calls queued on the tables of an earlier plan are ahead on the stream; a buffer that grows waits for them.)  The
    // earlier tables and slots are given up where the first step that can destroy them begins: a buffer that has to grow -
    // the only reserve that can fail - or, with every buffer large enough, the upload.  Up to there a refusal leaves them
    const size_t want[3] = {(n_tx + n_ty) * sizeof(double2), n_rows * sizeof(double2), n_out * sizeof(double2)};
    DevBuf *const bufs[3] = {&pp.modes_tables, &pp.modes_rows, &pp.modes_out};
    for (int b = 0; b < 3; ++b) {
        if (want[b] > bufs[b]->bytes) pp.modes.planned = false;
        ML_TRY(bufs[b]->reserve(want[b]));
    }
    pp.modes.planned = false;
    ML_HIP(hipMemcpyAsync(pp.modes_tables.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ML_HIP(hipMemsetAsync(pp.modes_out.p, 0, n_out * sizeof(double2), ctx->stream));   // a slot never written reads zeros
    ML_HIP(hipStreamSynchronize(ctx->stream));   // (`h` goes away)
    pp.modes.mx = mx;
    pp.modes.my = my;
    pp.modes.planes = planes;
    pp.modes.nu = nu;
    pp.modes.nv = nv;
    pp.modes.n_slots = n_slots;
    pp.modes.planned = true;
    return ML_OK;
}

int ml_propagate_modes_queue(ml_ctx *ctx, int source, int slot) {
    ML_REQUIRE(ctx, "NULL argument");
    ML_REQUIRE(ctx->n_ranks <= 1, "ml_propagate_modes_queue: this context belongs to a communicator of %d ranks", ctx->n_ranks);
    PropagatePlan &pp = ctx->prop;
    FocusState st;
    st.have_result = pp.ready && pp.have_result;
    st.have_sums = pp.have_sums;
    st.T = pp.T;
    st.result_sets = pp.result_sets;
    const ModesState &m = pp.modes;
    char why[320];
    const int rc = modes_queue_check(st, m, source, slot, why, sizeof why);
    if (rc != 0) {
        set_error("%s", why);
        return rc == -2 ? ML_ESTATE : ML_EINVAL;
    }
    ML_HIP(hipSetDevice(ctx->device));
    double2 *tx = pp.modes_tables.as<double2>(), *ty = tx + (size_t)m.mx * m.nu;
    double2 *out = pp.modes_out.as<double2>() + (size_t)slot * modes_slot_entries(m);
    ModesRowArgs a;
    a.result = pp.result.as<double2>() + (size_t)source * (pp.want_h ? 6 : 3) * pp.T;
    a.ty = ty;
    a.rows = pp.modes_rows.as<double2>();
    a.T = pp.T;
    a.mx = m.mx;
    a.my = m.my;
    a.nv = m.nv;
    a.planes = m.planes;
    if (pp.want_h)
        modes_rows_launch<true>(ctx->stream, a);
    else
        modes_rows_launch<false>(ctx->stream, a);
    ML_HIP(hipGetLastError());
    const int nc = pp.want_h ? MODES_COMPONENTS : 2;
    if (nc < MODES_COMPONENTS) ML_HIP(hipMemsetAsync(out, 0, modes_slot_entries(m) * sizeof(double2), ctx->stream));   // the H blocks: zeros
    hipLaunchKernelGGL(modes_columns_kernel, dim3(m.nu, nc, m.planes), dim3(MODES_THREADS), 0, ctx->stream, tx, a.rows, out, m.mx, m.nu,
                       m.nv, m.planes);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

int ml_propagate_modes_fetch(ml_ctx *ctx, int first_slot, int n_slots, double *out) {
    ML_REQUIRE(ctx, "NULL argument");
    ML_REQUIRE(ctx->n_ranks <= 1, "ml_propagate_modes_fetch: this context belongs to a communicator of %d ranks", ctx->n_ranks);
    PropagatePlan &pp = ctx->prop;
    const ModesState &m = pp.modes;
    char why[320];
    const int rc = modes_fetch_check(m, first_slot, n_slots, out, why, sizeof why);
    if (rc != 0) {
        set_error("%s", why);
        return rc == -2 ? ML_ESTATE : ML_EINVAL;
    }
    ML_HIP(hipSetDevice(ctx->device));
    const size_t slot = modes_slot_entries(m);
    ML_HIP(hipMemcpyAsync(out, pp.modes_out.as<double2>() + (size_t)first_slot * slot, (size_t)n_slots * slot * sizeof(double2),
                          hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

}  // extern "C"
