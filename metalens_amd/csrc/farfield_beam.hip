// Beam metrics of a far-field map, reduced where the map lies: of the active plan's current projection or of the P_sum
// of a sweep the peak and its direction, the number of finite directions, the zeroth to second moments of P dux duy
// about a centre and the power inside up to 32 cones about it (ml_farfield_beam), one record per call, queued into a
// slot of the context; ml_farfield_beams downloads slots.  The far-field counterpart of ml_propagate_focus.  Layouts,
// the cut into chunks, the order of every sum and the record: farfield_beam.h.  The reference has no counterpart: its
// callers form these numbers from the downloaded P in NumPy.
//
// Per direction the terms are those of farfield_beam.h operation by operation (nothing is contracted: -ffp-contract=off
// and the pragma below), so NumPy forms the same terms from the same doubles and a direction on a cone's edge is inside
// for both.  Sums and peak run over the finite P only - the isfinite rule of accumulate_kernel.
//
// Shape.  A workgroup of 256 lanes reduces one chunk; a lane takes one direction per step - consecutive lanes read
// consecutive doubles of P - and keeps the peak, the count, the six moment sums and one sum per cone in registers, in
// ascending order of its directions.  The chunk ends in a butterfly over the wave and the four waves' values added in
// their order.  No atomics: a record is repeatable bit for bit and depends on the map alone, not on the slot.
// Cones.  Every cone has a register of its own in every lane (the loop over the cones is unrolled, the cones behind the
// K-th skipped by a uniform branch each); a cone's sum does not depend on the other cones.
// Centre = the map's own peak: beam_chunk_kernel<false> leaves the chunks' peaks in a buffer of their own, and every
// workgroup of beam_chunk_kernel<true> reduces those to the map's peak and reads (ux[ip], uy[jp]) itself.
// The last launch, one workgroup, adds the chunks' partial records in two fixed-order levels: a lane per (tile of 32
// records, sum), then a lane per sum over the tiles - 32 + 32 additions in sequence at the most, not 1024.
#include "common.h"
#include "farfield_beam.h"

#pragma clang fp contract(off)

namespace ml {

static_assert(BEAM_RECORD == ML_BEAM_RECORD && BEAM_CONES_MAX == ML_BEAM_CONES_MAX && BEAM_SLOTS == ML_MAX_SWEEP_SLOTS,
              "farfield_beam.h and metalens_hip.h disagree");

struct BeamArgs {
    const double *P, *ux, *uy;
    const double *peaks;     // [chunks][2] of the first launch (centre = the peak), else unused
    double *partial;         // [chunks][BEAM_PARTIAL]
    int n, my, pair_list, chunk, chunks, K, centre_is_peak;
    double cell, cx, cy;
    double c2[BEAM_CONES_MAX];   // c c per cone
};

__device__ __forceinline__ double beam_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the larger of two peaks, of equals the lower index (an index of 0x7fffffff: none)
__device__ __forceinline__ void beam_peak_take(double &bv, int &bi, double ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
    }
}

__device__ __forceinline__ void beam_wave_peak(double &bv, int &bi) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(bv, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        beam_peak_take(bv, bi, ov, oi);
    }
}

constexpr int BEAM_NONE = 0x7fffffff;
constexpr int BEAM_UNROLL = 4;   // steps whose loads are in flight together; BEAM_CHUNK_MIN = BEAM_UNROLL * BEAM_THREADS
static_assert(BEAM_CHUNK_MIN % (BEAM_UNROLL * BEAM_THREADS) == 0, "a chunk is whole rounds of BEAM_UNROLL steps");

// FULL = false: the chunk's peak alone -> peaks[chunk][2];  FULL = true: the chunk's partial record
template <bool FULL>
__global__ __launch_bounds__(BEAM_THREADS) void beam_chunk_kernel(const BeamArgs a) {
    __shared__ double s_red[BEAM_THREADS / 64][BEAM_PARTIAL];
    __shared__ double s_pv[BEAM_THREADS / 64];
    __shared__ int s_pi[BEAM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x;
    const long long c0 = (long long)chunk * a.chunk, c1 = min((long long)a.n, c0 + a.chunk);   // the chunk's directions
    double cx = a.cx, cy = a.cy;
    if (FULL && a.centre_is_peak) {
        // the map's peak from the chunks' peaks (a maximum: any order gives the same pair)
        double bv = -INFINITY;
        int bi = BEAM_NONE;
        for (int c = tid; c < a.chunks; c += BEAM_THREADS) {
            const int oi = (int)a.peaks[2 * c + 1];
            if (oi >= 0) beam_peak_take(bv, bi, a.peaks[2 * c], oi);
        }
        beam_wave_peak(bv, bi);
        if (lane == 0) {
            s_pv[wave] = bv;
            s_pi[wave] = bi;
        }
        __syncthreads();
        bv = s_pv[0];
        bi = s_pi[0];
        for (int w = 1; w < BEAM_THREADS / 64; ++w) beam_peak_take(bv, bi, s_pv[w], s_pi[w]);
        if (bi == BEAM_NONE) {
            cx = cy = NAN;
        } else {
            const int ip = a.pair_list ? bi : bi / a.my, jp = a.pair_list ? bi : bi - ip * a.my;
            cx = a.ux[ip];
            cy = a.uy[jp];
        }
        __syncthreads();   // (s_pv, s_pi are written again below)
    }
    double bv = -INFINITY;
    int bi = BEAM_NONE, count = 0;
    double mom[BEAM_MOMENTS], cone[BEAM_CONES_MAX];
#pragma unroll
    for (int q = 0; q < BEAM_MOMENTS; ++q) mom[q] = 0.0;
#pragma unroll
    for (int r = 0; r < BEAM_CONES_MAX; ++r) cone[r] = 0.0;
    // four steps at a time (a chunk is a multiple of 1024 directions): the loads of all four are issued before the first
    // is added, the adds stay in ascending order of the lane's directions
    for (long long s0 = c0; s0 < c1; s0 += BEAM_UNROLL * BEAM_THREADS) {
        double Pv[BEAM_UNROLL], uxv[BEAM_UNROLL], uyv[BEAM_UNROLL];
        int atv[BEAM_UNROLL];
#pragma unroll
        for (int u = 0; u < BEAM_UNROLL; ++u) {
            const long long at64 = s0 + u * BEAM_THREADS + tid;
            const bool valid = at64 < c1;
            const int at = valid ? (int)at64 : (int)c0;   // (a lane past the end reads the chunk's first direction and drops it)
            atv[u] = at;
            Pv[u] = a.P[at];
            if (!valid) Pv[u] = NAN;
            if (FULL) {
                const int i = a.pair_list ? at : at / a.my, j = a.pair_list ? at : at - i * a.my;
                uxv[u] = a.ux[i];
                uyv[u] = a.uy[j];
            }
        }
#pragma unroll
        for (int u = 0; u < BEAM_UNROLL; ++u) {
            const double P = Pv[u];
            if (!isfinite(P)) continue;
            if (P > bv) {   // (ascending directions: of equals the first stays)
                bv = P;
                bi = atv[u];
            }
            if (!FULL) continue;
            ++count;
            const double dx = uxv[u] - cx, dy = uyv[u] - cy;
            const double t0 = P * a.cell;
            const double xx = dx * dx, yy = dy * dy;
            mom[0] += t0;
            mom[1] += t0 * dx;
            mom[2] += t0 * dy;
            mom[3] += t0 * xx;
            mom[4] += t0 * yy;
            mom[5] += t0 * (dx * dy);
            const double rho2 = xx + yy;
#pragma unroll
            for (int r = 0; r < BEAM_CONES_MAX; ++r) {
                if (r < a.K) cone[r] += rho2 <= a.c2[r] ? t0 : 0.0;
            }
        }
    }
    beam_wave_peak(bv, bi);
    if (!FULL) {
        if (lane == 0) {
            s_pv[wave] = bv;
            s_pi[wave] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < BEAM_THREADS / 64; ++w) beam_peak_take(bv, bi, s_pv[w], s_pi[w]);
            double *out = const_cast<double *>(a.peaks) + 2 * (size_t)chunk;
            out[0] = bv;
            out[1] = bi == BEAM_NONE ? -1.0 : (double)bi;
        }
        return;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) count += __shfl_xor(count, m, 64);
#pragma unroll
    for (int q = 0; q < BEAM_MOMENTS; ++q) mom[q] = beam_wave_sum(mom[q]);
#pragma unroll
    for (int r = 0; r < BEAM_CONES_MAX; ++r) {
        if (r < a.K) cone[r] = beam_wave_sum(cone[r]);
    }
    if (lane == 0) {
        s_pv[wave] = bv;
        s_pi[wave] = bi;
        s_red[wave][2] = (double)count;
#pragma unroll
        for (int q = 0; q < BEAM_MOMENTS; ++q) s_red[wave][3 + q] = mom[q];
#pragma unroll
        for (int r = 0; r < BEAM_CONES_MAX; ++r) {
            if (r < a.K) s_red[wave][BEAM_PARTIAL_CONE + r] = cone[r];
        }
    }
    __syncthreads();
    double *out = a.partial + (size_t)chunk * BEAM_PARTIAL;
    if (tid == 0) {
        for (int w = 1; w < BEAM_THREADS / 64; ++w) beam_peak_take(bv, bi, s_pv[w], s_pi[w]);
        out[0] = bv;
        out[1] = bi == BEAM_NONE ? -1.0 : (double)bi;
    } else if (tid >= 2 && tid < BEAM_PARTIAL_CONE + a.K) {
        out[tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    }
}

// last launch, one workgroup: the chunks' partial records -> the record of the map (BEAM_RECORD doubles at rec).
// Level 1: lane (t, q) adds column q of the records of tile t in index order (column 0: the tile's peak, of equals the
// lowest chunk, which holds the lowest index); level 2: lane q takes the tiles in index order.
__global__ __launch_bounds__(BEAM_FINISH_THREADS) void beam_finish_kernel(const double *partial, double *rec, const double *ux,
                                                                          const double *uy, int chunks, int my, int pair_list,
                                                                          int K, int centre_is_peak, double cx, double cy) {
    __shared__ double s_l1[BEAM_FINISH_TILES_MAX][BEAM_PARTIAL];
    const int tid = threadIdx.x;
    const int cols = BEAM_PARTIAL_CONE + K, tiles = beam_finish_tiles_of(chunks);
    for (int f = tid; f < tiles * cols; f += BEAM_FINISH_THREADS) {
        const int t = f / cols, q = f - t * cols;
        if (q == 1) continue;   // (the peak's index goes with the peak)
        const int n = beam_finish_tile_chunks(chunks, t);
        const double *p = partial + (size_t)t * BEAM_FINISH_TILE * BEAM_PARTIAL;
        if (q == 0) {
            double pv[BEAM_FINISH_TILE], pi[BEAM_FINISH_TILE];
#pragma unroll
            for (int c = 0; c < BEAM_FINISH_TILE; ++c) {
                pv[c] = c < n ? p[c * BEAM_PARTIAL] : -INFINITY;
                pi[c] = c < n ? p[c * BEAM_PARTIAL + 1] : -1.0;
            }
            double bv = -INFINITY, bi = -1.0;
#pragma unroll
            for (int c = 0; c < BEAM_FINISH_TILE; ++c)
                if (pv[c] > bv) {
                    bv = pv[c];
                    bi = pi[c];
                }
            s_l1[t][0] = bv;
            s_l1[t][1] = bi;
        } else {
            // all loads of the tile first, then the chain of adds (a record the tile does not have adds +0.0)
            double v[BEAM_FINISH_TILE];
#pragma unroll
            for (int c = 0; c < BEAM_FINISH_TILE; ++c) v[c] = c < n ? p[c * BEAM_PARTIAL + q] : 0.0;
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < BEAM_FINISH_TILE; ++c) s += v[c];
            s_l1[t][q] = s;
        }
    }
    __syncthreads();
    if (tid == 0) {
        double bv = -INFINITY, bi = -1.0;
        for (int t = 0; t < tiles; ++t)
            if (s_l1[t][0] > bv) {
                bv = s_l1[t][0];
                bi = s_l1[t][1];
            }
        rec[BEAM_PEAK_P] = bi < 0 ? NAN : bv;
        rec[BEAM_PEAK_INDEX] = bi;
        if (centre_is_peak) {
            if (bi < 0) {
                cx = cy = NAN;
            } else {
                const int idx = (int)bi, ip = pair_list ? idx : idx / my, jp = pair_list ? idx : idx - ip * my;
                cx = ux[ip];
                cy = uy[jp];
            }
        }
        rec[BEAM_CENTRE] = cx;
        rec[BEAM_CENTRE + 1] = cy;
        rec[BEAM_K] = (double)K;
    } else if (tid >= 2 && tid < cols) {
        double s = 0.0;
        for (int t = 0; t < tiles; ++t) s += s_l1[t][tid];
        // columns 2 ... 8 are the record's own; the cones lie behind the centre and K
        rec[tid < BEAM_PARTIAL_CONE ? tid : BEAM_CONE + (tid - BEAM_PARTIAL_CONE)] = s;
    } else if (tid >= cols && tid < BEAM_PARTIAL) {
        rec[BEAM_CONE + (tid - BEAM_PARTIAL_CONE)] = 0.0;   // behind K
    }
}

// what the checks of farfield_beam.h read of a context
BeamState beam_state(const ml_ctx *ctx) {
    const FarfieldPlan &pl = ctx->plan;
    BeamState st;
    st.projected = pl.ready && pl.have_vectors;
    st.scattered = pl.amp_rows && !pl.amp_gathered;
    st.n = pl.ready ? (long long)pl.directions() : 0;
    st.pair_list = pl.pair_list != 0;
    st.acc_n = (long long)ctx->acc_n;
    st.acc_pair_list = ctx->acc_pair_list != 0;
    return st;
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_farfield_beam(ml_ctx *ctx, int source, const double *centre, const double *cones, int n_cones, int slot) {
    ML_REQUIRE(ctx, "ctx is NULL");
    FarfieldPlan &pl = ctx->plan;
    const BeamState st = beam_state(ctx);
    char why[320];
    const int rc = beam_check(st, source, centre, cones, n_cones, slot, why, sizeof why);
    if (rc != 0) {
        set_error("%s", why);
        return rc == -2 ? ML_ESTATE : ML_EINVAL;
    }
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(comm_join(ctx, false));
    const int n = (int)st.n, chunk = (int)beam_chunk_directions(st.n), chunks = beam_chunks(st.n);
    ML_TRY(ctx->beam_partials.reserve(((size_t)chunks * BEAM_PARTIAL + (size_t)chunks * 2) * sizeof(double)));
    if (!ctx->beam_records.p) {
        const size_t bytes = (size_t)BEAM_SLOTS * BEAM_RECORD * sizeof(double);
        ML_TRY(ctx->beam_records.reserve(bytes));
        ML_HIP(hipMemsetAsync(ctx->beam_records.p, 0, bytes, ctx->stream));
    }
    BeamArgs a;
    a.P = source == 0 ? pl.power.as<double>() : ctx->acc_P.as<double>();
    a.ux = pl.ux.as<double>();
    a.uy = pl.uy.as<double>();
    a.partial = ctx->beam_partials.as<double>();
    a.peaks = a.partial + (size_t)chunks * BEAM_PARTIAL;
    a.n = n;
    a.my = pl.out_my();
    a.pair_list = pl.pair_list != 0;
    a.chunk = chunk;
    a.chunks = chunks;
    a.K = n_cones;
    a.centre_is_peak = centre ? 0 : 1;
    a.cell = beam_cell(pl.h_ux.data(), pl.mx, pl.h_uy.data(), pl.my, pl.pair_list != 0);
    a.cx = centre ? centre[0] : 0.0;
    a.cy = centre ? centre[1] : 0.0;
    for (int r = 0; r < BEAM_CONES_MAX; ++r) a.c2[r] = r < n_cones ? cones[r] * cones[r] : 0.0;
    if (!centre) {
        hipLaunchKernelGGL((beam_chunk_kernel<false>), dim3(chunks), dim3(BEAM_THREADS), 0, ctx->stream, a);
        ML_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((beam_chunk_kernel<true>), dim3(chunks), dim3(BEAM_THREADS), 0, ctx->stream, a);
    ML_HIP(hipGetLastError());
    hipLaunchKernelGGL(beam_finish_kernel, dim3(1), dim3(BEAM_FINISH_THREADS), 0, ctx->stream, a.partial,
                       ctx->beam_records.as<double>() + (size_t)slot * BEAM_RECORD, a.ux, a.uy, chunks, a.my, a.pair_list, n_cones,
                       a.centre_is_peak, a.cx, a.cy);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

int ml_farfield_beams(ml_ctx *ctx, int first_slot, int n_slots, double *records) {
    ML_REQUIRE(ctx, "ctx is NULL");
    char why[320];
    if (beams_check(first_slot, n_slots, why, sizeof why) != 0) {
        set_error("%s", why);
        return ML_EINVAL;
    }
    ML_REQUIRE(records || n_slots == 0, "ml_farfield_beams: %d slots asked for, records is NULL", n_slots);
    if (n_slots == 0) return ML_OK;
    const size_t count = (size_t)n_slots * BEAM_RECORD;
    if (!ctx->beam_records.p) {   // no record was ever queued: every slot reads zeros
        std::fill(records, records + count, 0.0);
        return ML_OK;
    }
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(comm_join(ctx, false));
    ML_HIP(hipMemcpyAsync(records, ctx->beam_records.as<double>() + (size_t)first_slot * BEAM_RECORD, count * sizeof(double),
                          hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

}  // extern "C"
