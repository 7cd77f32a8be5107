// Focus metrics of a propagated image, reduced where the image lies: per plane of the active propagation plan's resident
// result (or of its sums) the peak of |E|^2 and its place, the zeroth to second moments of |E|^2 and of Sz, and the sums
// of both inside up to 32 radii about a centre (ml_propagate_focus).  Layouts, the cut into chunks and the record:
// propagate_focus.h.  The reference has no counterpart; the far-field side's is ml_farfield_accumulate.
//
// Per target the weights are those of propagate_accumulate_kernel, operation by operation:
//   I = ((Ex.r^2 + Ex.i^2) + (Ey.r^2 + Ey.i^2)) + (Ez.r^2 + Ez.i^2),   Sz = 0.5 ((Ex.r Hy.r + Ex.i Hy.i) - (Ey.r Hx.r + Ey.i Hx.i))
// (nothing is contracted: -ffp-contract=off), so the sums of one member with weight 1 hold the numbers this pass forms
// from that member's fields.  From the sums the stored doubles are taken as they are.
//
// Shape.  A workgroup of 256 lanes reduces one chunk of one plane (grid: chunks x planes); a lane takes two neighbouring
// targets per step - 32 bytes per component of a field set, one 16-byte load of each sum where the plane starts on an even
// index (an odd plane size puts every other plane of a stack on an odd one: those read 8 bytes at a time, the same
// numbers in the same order) - and keeps the peak and the twelve moment sums in registers, in ascending order of its
// targets.  The chunk ends in a butterfly over the wave and the four waves' values added in their order.  No atomics:
// a record is repeatable bit for bit, and the order depends on (mx, my) alone.
// Radii.  The sorted radii cut the plane into disjoint annuli; a target's annulus is found by bisection of the squared
// radii (LDS, 6 reads).  A wave adds its targets annulus by annulus: for every annulus met among its 64 targets, the
// members' weights are summed by the butterfly (zeros elsewhere) and added to the wave's own bin in the LDS.  A row of
// 64 neighbouring targets meets few annuli - one, mostly.  A wave none of whose 128 targets of a step lies inside the
// largest radius has computed their squared distances and nothing more; in a pass over the radii alone it does not
// read them either, so a disc in a large plane costs the index arithmetic of the plane and the reads of the disc's rows.
// The second launch adds the chunks' annuli in index order and accumulates them into the radii's sums.
// A target is inside radius R iff fx fx + fy fy <= R R with fx = dx (i - ci), fy = dy (j - cj), every operation rounded on
// its own - what NumPy computes from the same doubles.
// Centre = the plane's own peak: the moments run first, their second launch leaves (i, j) of the peak in the centre
// buffer on the device, and the radii run as a second pair of launches that reads it there.
#include "common.h"
#include "propagate_focus.h"

#pragma clang fp contract(off)

namespace ml {

struct FocusArgs {
    const double2 *result;   // [6 or 3][T] of the member (fields), or
    const double *sums;      // [2][T]
    const double *centre;    // [planes][2], index units
    double *partial;         // [planes][chunks][FOCUS_PARTIAL]
    int T, P, my, chunk, chunks, want_h, K;
    double dx, dy;
    double r2[FOCUS_RADII_MAX];   // R R per radius, +inf behind the last
};

__device__ __forceinline__ double focus_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct FocusAcc {
    double bv;
    int bi;
    double mi[FOCUS_MOMENTS], ms[FOCUS_MOMENTS];
};

__device__ __forceinline__ void focus_moments(double m[FOCUS_MOMENTS], double w, double fi, double fj) {
    m[0] += w;
    m[1] += w * fi;
    m[2] += w * fj;
    m[3] += w * (fi * fi);   // (the products of the indices are exact)
    m[4] += w * (fj * fj);
    m[5] += w * (fi * fj);
}

// the squared distance the membership rule compares: three lines, every operation rounded on its own
__device__ __forceinline__ double focus_r2(double dx, double dy, double ci, double cj, int i, int j) {
    const double fx = dx * ((double)i - ci);
    const double fy = dy * ((double)j - cj);
    return fx * fx + fy * fy;
}

// the first radius a target at r2 lies inside, 32 if none (s_r2: 32 squared radii, ascending, +inf behind the K-th)
__device__ __forceinline__ int focus_annulus(const double *s_r2, double r2) {
    int k = 0;
#pragma unroll
    for (int step = FOCUS_RADII_MAX / 2; step >= 1; step >>= 1)
        if (!(r2 <= s_r2[k + step - 1])) k += step;
    if (!(r2 <= s_r2[k])) ++k;
    return k;
}

// every annulus met in the wave: the sum of its members' weights into the wave's bin (ann >= K: no member of any)
__device__ __forceinline__ void focus_annuli_add(int ann, int K, double I, double S, bool want_h, double (*bins)[2], int lane) {
    unsigned long long todo = __ballot(ann < K);
    while (todo) {
        const int k = __shfl(ann, __ffsll((long long)todo) - 1, 64);
        const bool mine = ann == k;
        const double sI = focus_wave_sum(mine ? I : 0.0);
        const double sS = want_h ? focus_wave_sum(mine ? S : 0.0) : 0.0;
        if (lane == 0) {
            bins[k][0] += sI;
            bins[k][1] += sS;
        }
        todo &= ~__ballot(mine);
    }
}

template <bool FIELDS, bool MOMENTS, bool RADII>
__global__ __launch_bounds__(FOCUS_THREADS) void focus_chunk_kernel(const FocusArgs a) {
    __shared__ double s_r2[FOCUS_RADII_MAX];
    __shared__ double s_bins[FOCUS_THREADS / 64][FOCUS_RADII_MAX][2];
    __shared__ double s_red[FOCUS_THREADS / 64][FOCUS_PARTIAL_ANNULI];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int plane = blockIdx.y, chunk = blockIdx.x;
    const size_t plane0 = (size_t)plane * a.P;
    const int c0 = chunk * a.chunk, c1 = min(a.P, c0 + a.chunk);   // the chunk's targets within the plane
    double ci = 0.0, cj = 0.0, r2_max = 0.0;
    if (RADII) {
        if (tid < FOCUS_RADII_MAX) s_r2[tid] = a.r2[tid];
        for (int f = tid; f < (FOCUS_THREADS / 64) * FOCUS_RADII_MAX * 2; f += FOCUS_THREADS) (&s_bins[0][0][0])[f] = 0.0;
        ci = a.centre[2 * plane];
        cj = a.centre[2 * plane + 1];
        r2_max = a.r2[a.K - 1];   // (a pass over radii has K >= 1)
        __syncthreads();
    }
    // 16-byte loads of the sums need an even index: c0 and 2 tid are even
    const bool even_i = (plane0 & 1) == 0, even_s = ((plane0 + (size_t)a.T) & 1) == 0;
    FocusAcc acc;
    acc.bv = -INFINITY;
    acc.bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < FOCUS_MOMENTS; ++q) acc.mi[q] = acc.ms[q] = 0.0;
    for (int s0 = c0; s0 < c1; s0 += FOCUS_STEP) {   // (uniform: every lane of a wave takes every step)
        const int t = s0 + 2 * tid;
        const bool v0 = t < c1, v1 = t + 1 < c1;
        const int i0 = t / a.my, j0 = t - i0 * a.my;
        const bool wraps = j0 + 1 == a.my;                      // the second target begins the next row
        const int i1 = wraps ? i0 + 1 : i0, j1 = wraps ? 0 : j0 + 1;
        int ann[2] = {a.K, a.K};
        bool near = false;   // (of the wave) a target inside the largest radius
        if (RADII) {
            const double ra = v0 ? focus_r2(a.dx, a.dy, ci, cj, i0, j0) : INFINITY;
            const double rb = v1 ? focus_r2(a.dx, a.dy, ci, cj, i1, j1) : INFINITY;
            near = __ballot(ra <= r2_max || rb <= r2_max) != 0;
            if (!MOMENTS && !near) continue;                    // nothing of this step is summed: nothing is read
            if (ra <= r2_max) ann[0] = focus_annulus(s_r2, ra);
            if (rb <= r2_max) ann[1] = focus_annulus(s_r2, rb);
        }
        double I[2] = {0.0, 0.0}, S[2] = {0.0, 0.0};
        if (FIELDS) {
            const size_t T = (size_t)a.T;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (!(u ? v1 : v0)) continue;
                const double2 *r = a.result + plane0 + t + u;
                const double2 Ex = r[0], Ey = r[T], Ez = r[2 * T];
                I[u] = ((Ex.x * Ex.x + Ex.y * Ex.y) + (Ey.x * Ey.x + Ey.y * Ey.y)) + (Ez.x * Ez.x + Ez.y * Ez.y);
                if (a.want_h) {
                    const double2 Hx = r[3 * T], Hy = r[4 * T];
                    S[u] = 0.5 * ((Ex.x * Hy.x + Ex.y * Hy.y) - (Ey.x * Hx.x + Ey.y * Hx.y));
                }
            }
        } else {
            const double *pi = a.sums + plane0 + t;
            if (even_i && v1) {
                const double2 v = *reinterpret_cast<const double2 *>(pi);
                I[0] = v.x;
                I[1] = v.y;
            } else {
                if (v0) I[0] = pi[0];
                if (v1) I[1] = pi[1];
            }
            if (a.want_h) {
                const double *ps = pi + a.T;
                if (even_s && v1) {
                    const double2 v = *reinterpret_cast<const double2 *>(ps);
                    S[0] = v.x;
                    S[1] = v.y;
                } else {
                    if (v0) S[0] = ps[0];
                    if (v1) S[1] = ps[1];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool valid = u ? v1 : v0;
            const int i = u ? i1 : i0, j = u ? j1 : j0;
            if (MOMENTS && valid) {
                if (I[u] > acc.bv) {   // (ascending targets: of equals the first stays)
                    acc.bv = I[u];
                    acc.bi = t + u;
                }
                focus_moments(acc.mi, I[u], (double)i, (double)j);
                if (a.want_h) focus_moments(acc.ms, S[u], (double)i, (double)j);
            }
            if (RADII && near) focus_annuli_add(ann[u], a.K, I[u], S[u], a.want_h != 0, s_bins[wave], lane);
        }
    }
    if (MOMENTS) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(acc.bv, m, 64);
            const int oi = __shfl_xor(acc.bi, m, 64);
            if (ov > acc.bv || (ov == acc.bv && oi < acc.bi)) {
                acc.bv = ov;
                acc.bi = oi;
            }
        }
#pragma unroll
        for (int q = 0; q < FOCUS_MOMENTS; ++q) {
            acc.mi[q] = focus_wave_sum(acc.mi[q]);
            acc.ms[q] = focus_wave_sum(acc.ms[q]);
        }
        if (lane == 0) {
            s_red[wave][0] = acc.bv;
            s_red[wave][1] = (double)acc.bi;
#pragma unroll
            for (int q = 0; q < FOCUS_MOMENTS; ++q) {
                s_red[wave][FOCUS_MOM_I + q] = acc.mi[q];
                s_red[wave][FOCUS_MOM_SZ + q] = acc.ms[q];
            }
        }
    }
    __syncthreads();
    double *out = a.partial + ((size_t)plane * a.chunks + chunk) * FOCUS_PARTIAL;
    if (MOMENTS) {
        if (tid == 0) {
            double bv = s_red[0][0], bi = s_red[0][1];
            for (int w = 1; w < FOCUS_THREADS / 64; ++w)
                if (s_red[w][0] > bv || (s_red[w][0] == bv && s_red[w][1] < bi)) {
                    bv = s_red[w][0];
                    bi = s_red[w][1];
                }
            out[0] = bv;
            out[1] = bi;
        } else if (tid >= FOCUS_MOM_I && tid < FOCUS_PARTIAL_ANNULI) {
            out[tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
        }
    }
    if (RADII && tid >= 64 && tid < 64 + 2 * a.K) {
        const int f = tid - 64, k = f >> 1, c = f & 1;
        out[FOCUS_PARTIAL_ANNULI + f] = ((s_bins[0][k][c] + s_bins[1][k][c]) + s_bins[2][k][c]) + s_bins[3][k][c];
    }
}

// second launch, a workgroup per plane: the chunks' partial records in index order -> the plane's record (rd doubles).
// The records pass through the LDS FOCUS_FINISH_TILE chunks at a time - loaded by all lanes at once, so that the one lane
// per sum that adds them in their order waits for the LDS and not for a load from memory per chunk.
// moments: the peak (of equals the lowest chunk, which holds the lowest index), the twelve sums and the centre - the
// peak's (i, j), written to the centre buffer too, or the one the buffer holds; radii: the annuli, then accumulated
// (FOCUS_FINISH_THREADS, FOCUS_FINISH_TILE and the tiles of a plane: propagate_focus.h)
__global__ __launch_bounds__(FOCUS_FINISH_THREADS) void focus_finish_kernel(const double *partial, double *records, double *centre,
                                                                            int chunks, int my, int K, int rd, int moments,
                                                                            int radii, int centre_is_peak) {
    __shared__ double s_tile[FOCUS_FINISH_TILE][FOCUS_PARTIAL];
    __shared__ double s_ann[2 * FOCUS_RADII_MAX];
    const int tid = threadIdx.x, plane = blockIdx.x;
    const double *p = partial + (size_t)plane * chunks * FOCUS_PARTIAL;
    double *rec = records + (size_t)plane * rd;
    const bool peak = moments && tid == 0;
    const bool sum = (moments && tid >= FOCUS_MOM_I && tid < FOCUS_PARTIAL_ANNULI) ||
                     (radii && tid >= FOCUS_PARTIAL_ANNULI && tid < FOCUS_PARTIAL_ANNULI + 2 * K);
    double s = 0.0, bv = -INFINITY, bi = 0.0;
    const int tiles = focus_finish_tiles_of(chunks);
    for (int t = 0; t < tiles; ++t) {
        const int c0 = t * FOCUS_FINISH_TILE, n = focus_finish_tile_chunks(chunks, t);
        __syncthreads();   // the previous tile has been added
        for (int f = tid; f < n * FOCUS_PARTIAL; f += FOCUS_FINISH_THREADS) (&s_tile[0][0])[f] = p[(size_t)c0 * FOCUS_PARTIAL + f];
        __syncthreads();
        if (sum)
            for (int c = 0; c < n; ++c) s += s_tile[c][tid];
        if (peak)
            for (int c = 0; c < n; ++c)
                if (s_tile[c][0] > bv) {
                    bv = s_tile[c][0];
                    bi = s_tile[c][1];
                }
    }
    if (peak) {
        rec[FOCUS_PEAK_I] = bv;
        rec[FOCUS_PEAK_INDEX] = bi;
        if (centre_is_peak) {
            const int idx = (int)bi;
            centre[2 * plane] = rec[FOCUS_CENTRE] = (double)(idx / my);
            centre[2 * plane + 1] = rec[FOCUS_CENTRE + 1] = (double)(idx % my);
        }
    }
    if (sum && tid < FOCUS_PARTIAL_ANNULI) rec[tid] = s;
    if (moments && !centre_is_peak && tid >= FOCUS_CENTRE && tid < FOCUS_CENTRE + 2) rec[tid] = centre[2 * plane + tid - FOCUS_CENTRE];
    if (radii) {
        if (sum && tid >= FOCUS_PARTIAL_ANNULI) s_ann[tid - FOCUS_PARTIAL_ANNULI] = s;
        __syncthreads();
        if (tid < 2) {   // 0: I, 1: Sz
            double run = 0.0;
            for (int k = 0; k < K; ++k) {
                run += s_ann[2 * k + tid];
                rec[FOCUS_ENC + tid * K + k] = run;
            }
        }
    }
}

template <bool FIELDS>
static void focus_launch(hipStream_t stream, dim3 grid, const FocusArgs &a, bool moments, bool radii) {
    if (moments && radii)
        hipLaunchKernelGGL((focus_chunk_kernel<FIELDS, true, true>), grid, dim3(FOCUS_THREADS), 0, stream, a);
    else if (moments)
        hipLaunchKernelGGL((focus_chunk_kernel<FIELDS, true, false>), grid, dim3(FOCUS_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL((focus_chunk_kernel<FIELDS, false, true>), grid, dim3(FOCUS_THREADS), 0, stream, a);
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_propagate_focus(ml_ctx *ctx, int source, int mx, int my, int planes, double dx, double dy, const double *centre,
                       const double *radii, int n_radii, double *records, int record_doubles) {
    ML_REQUIRE(ctx && records, "NULL argument");
    ML_REQUIRE(ctx->n_ranks <= 1, "ml_propagate_focus: this context belongs to a communicator of %d ranks", ctx->n_ranks);
    PropagatePlan &pp = ctx->prop;
    FocusState st;
    st.have_result = pp.ready && pp.have_result;
    st.have_sums = pp.have_sums;
    st.T = pp.T;
    st.result_sets = pp.result_sets;
    char why[320];
    const int rc = focus_check(st, source, mx, my, planes, dx, dy, centre, radii, n_radii, record_doubles, why, sizeof why);
    if (rc != 0) {
        set_error("%s", why);
        return rc == -2 ? ML_ESTATE : ML_EINVAL;
    }
    ML_HIP(hipSetDevice(ctx->device));
    const int K = n_radii, rd = focus_record_doubles(K), P = mx * my;
    const int chunk = (int)focus_chunk_targets(P), chunks = focus_chunks(P);
    ML_TRY(pp.focus_partial.reserve((size_t)planes * chunks * FOCUS_PARTIAL * sizeof(double)));
    ML_TRY(pp.focus_records.reserve((size_t)planes * rd * sizeof(double)));
    ML_TRY(pp.focus_centre.reserve((size_t)planes * 2 * sizeof(double)));
    if (centre)
        ML_HIP(hipMemcpyAsync(pp.focus_centre.p, centre, (size_t)planes * 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    FocusArgs a;
    const bool fields = source >= 0;
    a.result = fields ? pp.result.as<double2>() + (size_t)source * (pp.want_h ? 6 : 3) * pp.T : nullptr;
    a.sums = fields ? nullptr : pp.sums.as<double>();
    a.centre = pp.focus_centre.as<double>();
    a.partial = pp.focus_partial.as<double>();
    a.T = pp.T;
    a.P = P;
    a.my = my;
    a.chunk = chunk;
    a.chunks = chunks;
    a.want_h = pp.want_h ? 1 : 0;
    a.K = K;
    a.dx = dx;
    a.dy = dy;
    for (int r = 0; r < FOCUS_RADII_MAX; ++r) a.r2[r] = r < K ? radii[r] * radii[r] : INFINITY;
    const dim3 grid(chunks, planes);
    double *rec = pp.focus_records.as<double>(), *cen = pp.focus_centre.as<double>();
    // the centre is known (given, or no radius asks for one): one pass; else the moments, then the radii about the peak
    const bool one_pass = centre != nullptr || K == 0;
    if (fields)
        focus_launch<true>(ctx->stream, grid, a, true, one_pass && K > 0);
    else
        focus_launch<false>(ctx->stream, grid, a, true, one_pass && K > 0);
    ML_HIP(hipGetLastError());
    hipLaunchKernelGGL(focus_finish_kernel, dim3(planes), dim3(FOCUS_FINISH_THREADS), 0, ctx->stream, a.partial, rec, cen, chunks, my, K, rd, 1,
                       (int)(one_pass && K > 0), (int)(centre == nullptr));
    ML_HIP(hipGetLastError());
    if (!one_pass) {
        if (fields)
            focus_launch<true>(ctx->stream, grid, a, false, true);
        else
            focus_launch<false>(ctx->stream, grid, a, false, true);
        ML_HIP(hipGetLastError());
        hipLaunchKernelGGL(focus_finish_kernel, dim3(planes), dim3(FOCUS_FINISH_THREADS), 0, ctx->stream, a.partial, rec, cen, chunks, my, K, rd, 0,
                           1, 1);
        ML_HIP(hipGetLastError());
    }
    if (record_doubles == rd) {
        ML_HIP(hipMemcpyAsync(records, rec, (size_t)planes * rd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        ML_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        std::vector<double> h((size_t)planes * rd);
        ML_HIP(hipMemcpyAsync(h.data(), rec, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        ML_HIP(hipStreamSynchronize(ctx->stream));
        for (int p = 0; p < planes; ++p) std::copy(h.begin() + (size_t)p * rd, h.begin() + (size_t)(p + 1) * rd, records + (size_t)p * record_doubles);
    }
    return ML_OK;
}

}  // extern "C"
