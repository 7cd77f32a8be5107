// Stokes records of a propagated image, reduced where the image lies: per plane of the active propagation plan's resident
// result (or of its Stokes sums) the peak of I = |E|^2 and its place, the sums of S0, S1, S2, S3 and Iz = |Ez|^2 over the
// plane and inside up to 32 radii about a centre (ml_propagate_stokes); the weighted Stokes maps of the sets of a pass
// kept on the GPU (ml_propagate_accumulate_stokes, ml_propagate_stokes_sums).  Layouts, the record and the formulas,
// operation by operation: propagate_stokes.h.  The fourth sibling of focus_chunk_kernel (propagate_focus.hip); the
// reference has no counterpart.
//
// Sign.  S3 = 2 Im(conj(Ex) Ey) = +S0 for E proportional to x^ + i y^.  Under the project's exp(-i omega t), for a wave
// travelling to +z, that is the field rotating counter-clockwise seen looking towards the source (positive helicity).
//
// Shape: that of focus_chunk_kernel.  A workgroup of 256 lanes reduces one chunk of one plane (grid: chunks x planes); a
// lane takes two neighbouring targets per step - 32 bytes of each of Ex, Ey, Ez, 48 of the 96 bytes of a target with H,
// which is never read; one 16-byte load of each of the five sums where the map's plane starts on an even index (an odd T
// puts the odd components on odd offsets, an odd plane size every other plane: those read 8 bytes at a time, the same
// numbers in the same order) - and keeps the peak and the five sums in registers, in ascending order of its targets.  The
// chunk ends in a butterfly over the wave and the four waves' values added in their order.  No atomics: a record is
// repeatable bit for bit, and the order depends on (mx, my) alone.
// Radii.  The sorted radii cut the plane into disjoint annuli; a target's annulus is found by bisection of the squared
// radii, as in focus_chunk_kernel.  What is summed is the inside of every radius itself: for every annulus a met among
// the wave's 64 targets, in ascending order, the butterfly adds the five components of the targets of the annuli up to a
// (zeros elsewhere), and lane r adds that sum to the wave's bin of radius r for a <= r < the next annulus met - no target
// of the wave lies between them, so it is the sum of the wave's targets inside radius r, formed by operations that do
// not know the other radii.  The second launch adds the chunks' bins in index order and nothing across radii: a radius
// alone has the bits it has among 32.  A wave none of whose 128 targets of a step lies inside the largest radius has
// computed their squared distances and no more for the radii.
#include "common.h"
#include "propagate_direct.h"   // PROP_MAX_SETS
#include "propagate_stokes.h"

#pragma clang fp contract(off)

namespace ml {

struct StokesArgs {
    const double2 *result;   // [6 or 3][T] of the member (fields), or
    const double *sums;      // [5][T]
    const double *centre;    // [planes][2], index units (radii only)
    double *partial;         // [planes][chunks][STOKES_PARTIAL]
    int T, P, my, chunk, chunks, K;
    double dx, dy;
    double r2[STOKES_RADII_MAX];   // R R per radius, +inf behind the last
};

__device__ __forceinline__ double stokes_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// S0, S1, S2, S3, Iz of a target: propagate_stokes.h, line by line
__device__ __forceinline__ void stokes_of(const double2 Ex, const double2 Ey, const double2 Ez, double v[STOKES_COMPONENTS]) {
    const double a = Ex.x * Ex.x + Ex.y * Ex.y;
    const double b = Ey.x * Ey.x + Ey.y * Ey.y;
    v[4] = Ez.x * Ez.x + Ez.y * Ez.y;
    v[0] = a + b;
    v[1] = a - b;
    v[2] = 2.0 * (Ex.x * Ey.x + Ex.y * Ey.y);
    v[3] = 2.0 * (Ex.x * Ey.y - Ex.y * Ey.x);
}

// the squared distance the membership rule compares and the first radius a target lies inside: those of propagate_focus.hip
__device__ __forceinline__ double stokes_r2(double dx, double dy, double ci, double cj, int i, int j) {
    const double fx = dx * ((double)i - ci);
    const double fy = dy * ((double)j - cj);
    return fx * fx + fy * fy;
}

__device__ __forceinline__ int stokes_annulus(const double *s_r2, double r2) {
    int k = 0;
#pragma unroll
    for (int step = STOKES_RADII_MAX / 2; step >= 1; step >>= 1)
        if (!(r2 <= s_r2[k + step - 1])) k += step;
    if (!(r2 <= s_r2[k])) ++k;
    return k;
}

// one target per lane (ann >= K: inside no radius): the wave's sums inside every radius into its bins [radius][component]
__device__ __forceinline__ void stokes_radii_add(int ann, int K, const double v[STOKES_COMPONENTS], double (*bins)[STOKES_COMPONENTS],
                                                 int lane) {
    unsigned long long todo = __ballot(ann < K);
    unsigned met = 0;   // the annuli met in the wave, a bit each
    while (todo) {
        const int k = __shfl(ann, __ffsll((long long)todo) - 1, 64);
        met |= 1u << k;
        todo &= ~__ballot(ann == k);
    }
    while (met) {
        const int k = __ffs((int)met) - 1;
        met &= met - 1;
        const int next = met ? __ffs((int)met) - 1 : K;
        const bool in = ann <= k;
        double c[STOKES_COMPONENTS];
#pragma unroll
        for (int q = 0; q < STOKES_COMPONENTS; ++q) c[q] = stokes_wave_sum(in ? v[q] : 0.0);
        if (lane >= k && lane < next) {
#pragma unroll
            for (int q = 0; q < STOKES_COMPONENTS; ++q) bins[lane][q] += c[q];
        }
    }
}

template <bool FIELDS, bool RADII>
__global__ __launch_bounds__(STOKES_THREADS) void stokes_chunk_kernel(const StokesArgs a) {
    __shared__ double s_r2[STOKES_RADII_MAX];
    __shared__ double s_bins[STOKES_THREADS / 64][STOKES_RADII_MAX][STOKES_COMPONENTS];
    __shared__ double s_red[STOKES_THREADS / 64][STOKES_PARTIAL_RADII];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int plane = blockIdx.y, chunk = blockIdx.x;
    const size_t plane0 = (size_t)plane * a.P;
    const int c0 = chunk * a.chunk, c1 = min(a.P, c0 + a.chunk);   // the chunk's targets within the plane
    double ci = 0.0, cj = 0.0, r2_max = 0.0;
    if (RADII) {
        if (tid < STOKES_RADII_MAX) s_r2[tid] = a.r2[tid];
        for (int f = tid; f < (STOKES_THREADS / 64) * STOKES_RADII_MAX * STOKES_COMPONENTS; f += STOKES_THREADS) (&s_bins[0][0][0])[f] = 0.0;
        ci = a.centre[2 * plane];
        cj = a.centre[2 * plane + 1];
        r2_max = a.r2[a.K - 1];   // (a pass over radii has K >= 1)
        __syncthreads();
    }
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    double acc[STOKES_COMPONENTS];
#pragma unroll
    for (int q = 0; q < STOKES_COMPONENTS; ++q) acc[q] = 0.0;
    for (int s0 = c0; s0 < c1; s0 += STOKES_STEP) {   // (uniform: every lane of a wave takes every step)
        const int t = s0 + 2 * tid;
        const bool v0 = t < c1, v1 = t + 1 < c1;
        int ann[2] = {a.K, a.K};
        bool near = false;   // (of the wave) a target inside the largest radius
        if (RADII) {
            const int i0 = t / a.my, j0 = t - i0 * a.my;
            const bool wraps = j0 + 1 == a.my;                      // the second target begins the next row
            const int i1 = wraps ? i0 + 1 : i0, j1 = wraps ? 0 : j0 + 1;
            const double ra = v0 ? stokes_r2(a.dx, a.dy, ci, cj, i0, j0) : INFINITY;
            const double rb = v1 ? stokes_r2(a.dx, a.dy, ci, cj, i1, j1) : INFINITY;
            near = __ballot(ra <= r2_max || rb <= r2_max) != 0;
            if (ra <= r2_max) ann[0] = stokes_annulus(s_r2, ra);
            if (rb <= r2_max) ann[1] = stokes_annulus(s_r2, rb);
        }
        double v[2][STOKES_COMPONENTS];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < STOKES_COMPONENTS; ++q) v[u][q] = 0.0;
        if (FIELDS) {
            const size_t T = (size_t)a.T;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (!(u ? v1 : v0)) continue;
                const double2 *r = a.result + plane0 + t + u;
                stokes_of(r[0], r[T], r[2 * T], v[u]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < STOKES_COMPONENTS; ++q) {
                const size_t at = (size_t)q * a.T + plane0;   // 16-byte loads need an even index: c0 and 2 tid are even
                const double *pq = a.sums + at + t;
                if ((at & 1) == 0 && v1) {
                    const double2 w = *reinterpret_cast<const double2 *>(pq);
                    v[0][q] = w.x;
                    v[1][q] = w.y;
                } else {
                    if (v0) v[0][q] = pq[0];
                    if (v1) v[1][q] = pq[1];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u ? v1 : v0) {
                const double I = v[u][0] + v[u][4];
                if (I > bv) {   // (ascending targets: of equals the first stays)
                    bv = I;
                    bi = t + u;
                }
#pragma unroll
                for (int q = 0; q < STOKES_COMPONENTS; ++q) acc[q] += v[u][q];
            }
            if (RADII && near) stokes_radii_add(ann[u], a.K, v[u], s_bins[wave], lane);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(bv, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
    }
#pragma unroll
    for (int q = 0; q < STOKES_COMPONENTS; ++q) acc[q] = stokes_wave_sum(acc[q]);
    if (lane == 0) {
        s_red[wave][0] = bv;
        s_red[wave][1] = (double)bi;
#pragma unroll
        for (int q = 0; q < STOKES_COMPONENTS; ++q) s_red[wave][STOKES_SUMS + q] = acc[q];
    }
    __syncthreads();
    double *out = a.partial + ((size_t)plane * a.chunks + chunk) * STOKES_PARTIAL;
    if (tid == 0) {
        double pv = s_red[0][0], pi = s_red[0][1];
        for (int w = 1; w < STOKES_THREADS / 64; ++w)
            if (s_red[w][0] > pv || (s_red[w][0] == pv && s_red[w][1] < pi)) {
                pv = s_red[w][0];
                pi = s_red[w][1];
            }
        out[0] = pv;
        out[1] = pi;
    } else if (tid >= STOKES_SUMS && tid < STOKES_PARTIAL_RADII) {
        out[tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    }
    if (RADII && tid >= 64 && tid < 64 + STOKES_COMPONENTS * a.K) {
        const int f = tid - 64, k = f / STOKES_COMPONENTS, q = f - k * STOKES_COMPONENTS;
        out[STOKES_PARTIAL_RADII + f] = ((s_bins[0][k][q] + s_bins[1][k][q]) + s_bins[2][k][q]) + s_bins[3][k][q];
    }
}

// second launch, a workgroup per plane: the chunks' partial records in index order -> the plane's record (rd doubles),
// through the LDS STOKES_FINISH_TILE chunks at a time as focus_finish_kernel takes them - of every record the 7 + 5 K
// doubles the chunks wrote, not the STOKES_PARTIAL it has room for (one workgroup loads them: with whole records this
// launch took longer than the chunks' on a plane of 1024 chunks).  Lane 0: the peak (of equals the
// lowest chunk, which holds the lowest index) and the centre - the one given, or the peak's (i, j); lanes 2 ... 6: the
// plane's sums; lanes 7 ... 7 + 5 K - 1: the sums inside the radii, each on its own
__global__ __launch_bounds__(STOKES_FINISH_THREADS) void stokes_finish_kernel(const double *partial, double *records, const double *centre,
                                                                              int chunks, int my, int K, int rd, int have_centre) {
    __shared__ double s_tile[STOKES_FINISH_TILE][STOKES_PARTIAL];
    const int tid = threadIdx.x, plane = blockIdx.x;
    const double *p = partial + (size_t)plane * chunks * STOKES_PARTIAL;
    double *rec = records + (size_t)plane * rd;
    const bool peak = tid == 0;
    const bool sum = tid >= STOKES_SUMS && tid < STOKES_PARTIAL_RADII + STOKES_COMPONENTS * K;
    double s = 0.0, bv = -INFINITY, bi = 0.0;
    const int tiles = focus_finish_tiles_of(chunks);
    const int used = STOKES_PARTIAL_RADII + STOKES_COMPONENTS * K;   // what the chunks wrote of a partial record, and all that is read
    for (int t = 0; t < tiles; ++t) {
        const int c0 = t * STOKES_FINISH_TILE, n = focus_finish_tile_chunks(chunks, t);
        __syncthreads();   // the previous tile has been added
        for (int f = tid; f < n * used; f += STOKES_FINISH_THREADS) {
            const int c = f / used, e = f - c * used;
            s_tile[c][e] = p[(size_t)(c0 + c) * STOKES_PARTIAL + e];
        }
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
        rec[STOKES_PEAK_I] = bv;
        rec[STOKES_PEAK_INDEX] = bi;
        const int idx = (int)bi;
        rec[STOKES_CENTRE] = have_centre ? centre[2 * plane] : (double)(idx / my);
        rec[STOKES_CENTRE + 1] = have_centre ? centre[2 * plane + 1] : (double)(idx % my);
    }
    if (sum) rec[tid < STOKES_PARTIAL_RADII ? tid : tid + (STOKES_ENC - STOKES_PARTIAL_RADII)] = s;
}

struct StokesWeights {
    double w[PROP_MAX_SETS];
};

// sums[q][t] (+)= sum_m w_m S_q of set m, q = S0, S1, S2, S3, Iz, over the n sets of `result`: as
// propagate_accumulate_kernel, the pass's own sum is formed first, in set order, and then added once to what the sums hold
// (`reset`: to zero) - one lane per target, plain stores
__global__ __launch_bounds__(256) void stokes_accumulate_kernel(const double2 *result, double *sums, int T, int n, int nc, int reset,
                                                                const StokesWeights wt) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    double acc[STOKES_COMPONENTS];
    for (int m = 0; m < n; ++m) {
        const double2 *r = result + (size_t)m * nc * T + t;
        double v[STOKES_COMPONENTS];
        stokes_of(r[0], r[T], r[2 * (size_t)T], v);
#pragma unroll
        for (int q = 0; q < STOKES_COMPONENTS; ++q) {
            const double wv = wt.w[m] * v[q];
            acc[q] = m == 0 ? wv : acc[q] + wv;
        }
    }
#pragma unroll
    for (int q = 0; q < STOKES_COMPONENTS; ++q) {
        double *s = sums + (size_t)q * T + t;
        *s = reset ? acc[q] : *s + acc[q];
    }
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_propagate_stokes(ml_ctx *ctx, int source, int mx, int my, int planes, double dx, double dy, const double *centre,
                        const double *radii, int n_radii, double *record, int record_doubles) {
    ML_REQUIRE(ctx && record, "NULL argument");
    ML_REQUIRE(ctx->n_ranks <= 1, "ml_propagate_stokes: this context belongs to a communicator of %d ranks", ctx->n_ranks);
    PropagatePlan &pp = ctx->prop;
    StokesState st;
    st.have_result = pp.ready && pp.have_result;
    st.have_stokes = pp.have_stokes;
    st.T = pp.T;
    st.result_sets = pp.result_sets;
    char why[320];
    const int rc = stokes_check(st, source, mx, my, planes, dx, dy, centre, radii, n_radii, record_doubles, why, sizeof why);
    if (rc != 0) {
        set_error("%s", why);
        return rc == -2 ? ML_ESTATE : ML_EINVAL;
    }
    ML_HIP(hipSetDevice(ctx->device));
    const int K = n_radii, rd = stokes_record_doubles(K), P = mx * my;
    const int chunk = (int)focus_chunk_targets(P), chunks = focus_chunks(P);
    ML_TRY(pp.stokes_partial.reserve((size_t)planes * chunks * STOKES_PARTIAL * sizeof(double)));
    ML_TRY(pp.stokes_records.reserve((size_t)planes * rd * sizeof(double)));
    ML_TRY(pp.stokes_centre.reserve((size_t)planes * 2 * sizeof(double)));
    if (centre)
        ML_HIP(hipMemcpyAsync(pp.stokes_centre.p, centre, (size_t)planes * 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    StokesArgs a;
    const bool fields = source >= 0;
    a.result = fields ? pp.result.as<double2>() + (size_t)source * (pp.want_h ? 6 : 3) * pp.T : nullptr;
    a.sums = fields ? nullptr : pp.stokes_sums.as<double>();
    a.centre = pp.stokes_centre.as<double>();
    a.partial = pp.stokes_partial.as<double>();
    a.T = pp.T;
    a.P = P;
    a.my = my;
    a.chunk = chunk;
    a.chunks = chunks;
    a.K = K;
    a.dx = dx;
    a.dy = dy;
    for (int r = 0; r < STOKES_RADII_MAX; ++r) a.r2[r] = r < K ? radii[r] * radii[r] : INFINITY;
    const dim3 grid(chunks, planes), block(STOKES_THREADS);
    if (fields && K > 0)
        hipLaunchKernelGGL((stokes_chunk_kernel<true, true>), grid, block, 0, ctx->stream, a);
    else if (fields)
        hipLaunchKernelGGL((stokes_chunk_kernel<true, false>), grid, block, 0, ctx->stream, a);
    else if (K > 0)
        hipLaunchKernelGGL((stokes_chunk_kernel<false, true>), grid, block, 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((stokes_chunk_kernel<false, false>), grid, block, 0, ctx->stream, a);
    ML_HIP(hipGetLastError());
    double *rec = pp.stokes_records.as<double>();
    hipLaunchKernelGGL(stokes_finish_kernel, dim3(planes), dim3(STOKES_FINISH_THREADS), 0, ctx->stream, a.partial, rec, a.centre, chunks, my,
                       K, rd, (int)(centre != nullptr));
    ML_HIP(hipGetLastError());
    if (record_doubles == rd) {
        ML_HIP(hipMemcpyAsync(record, rec, (size_t)planes * rd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        ML_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        std::vector<double> h((size_t)planes * rd);
        ML_HIP(hipMemcpyAsync(h.data(), rec, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        ML_HIP(hipStreamSynchronize(ctx->stream));
        for (int p = 0; p < planes; ++p) std::copy(h.begin() + (size_t)p * rd, h.begin() + (size_t)(p + 1) * rd, record + (size_t)p * record_doubles);
    }
    return ML_OK;
}

int ml_propagate_accumulate_stokes(ml_ctx *ctx, const double *weights, int n, int reset) {
    ML_REQUIRE(ctx && weights, "NULL argument");
    ML_REQUIRE(ctx->n_ranks <= 1, "ml_propagate_accumulate_stokes: this context belongs to a communicator of %d ranks", ctx->n_ranks);
    PropagatePlan &pp = ctx->prop;
    if (!pp.ready || !pp.have_result) {
        set_error("ml_propagate has not run on the active propagation plan");
        return ML_ESTATE;
    }
    ML_REQUIRE(n >= 1 && n <= pp.result_sets, "ml_propagate_accumulate_stokes: %d field sets to add, the last pass propagated %d", n,
               pp.result_sets);
    if (!reset && !pp.have_stokes) {
        set_error("ml_propagate_accumulate_stokes: the active propagation plan has no Stokes sums yet (the first call needs reset = 1)");
        return ML_ESTATE;
    }
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(pp.stokes_sums.reserve((size_t)STOKES_COMPONENTS * pp.T * sizeof(double)));
    StokesWeights wt = {};
    for (int m = 0; m < n; ++m) wt.w[m] = weights[m];
    hipLaunchKernelGGL(stokes_accumulate_kernel, dim3((pp.T + 255) / 256), dim3(256), 0, ctx->stream, pp.result.as<double2>(),
                       pp.stokes_sums.as<double>(), pp.T, n, pp.want_h ? 6 : 3, reset, wt);
    ML_HIP(hipGetLastError());
    pp.have_stokes = true;
    return ML_OK;
}

int ml_propagate_stokes_sums(ml_ctx *ctx, double *out) {
    ML_REQUIRE(ctx && out, "NULL argument");
    ML_REQUIRE(ctx->n_ranks <= 1, "ml_propagate_stokes_sums: this context belongs to a communicator of %d ranks", ctx->n_ranks);
    PropagatePlan &pp = ctx->prop;
    if (!pp.ready || !pp.have_stokes) {
        set_error("ml_propagate_accumulate_stokes has not run on the active propagation plan");
        return ML_ESTATE;
    }
    ML_HIP(hipSetDevice(ctx->device));
    ML_HIP(hipMemcpyAsync(out, pp.stokes_sums.p, (size_t)STOKES_COMPONENTS * pp.T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

}  // extern "C"
