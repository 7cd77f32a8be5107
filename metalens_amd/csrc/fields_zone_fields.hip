// Per-zone contributions to the field at points behind the aperture (ml_fields_zone_fields): the direct pair sum of the
// propagator (propagate.hip) left un-added across the Fresnel zones of the resident near field - for every zone of a list
// of ring edges, every target and every field set of a call E_z(t) (and H_z(t)), with E(t) = sum_z E_z(t).  How much a ring
// adds at the focus and with which phase, in one pass over the aperture per group of targets instead of one pupil and one
// propagation per zone.  Definitions, the order of every sum and the scratch: fields_zone_fields.h.
//
// Neither existing shape fits: propagate_kernel puts a target on a lane (63 idle lanes at one focus point, nowhere to keep
// K bins), zones_line_kernel has the run-per-zone machinery with scalar terms.  This is the line walk of fields_zones.hip
// carrying the pair arithmetic of propagate_pair.h.
//
// First launch, zf_line_kernel<WANT_H>.  One wave per line, four lines per workgroup, the squared edges in the LDS, one
// field set.  The wave takes the line in blocks of 64 samples, lane = sample; the four fields of a sample are four 16-byte
// loads issued one block ahead and serve the ZF_TG targets of the walk.  Per target the lane forms its pair's term - 6
// doubles, 12 with H - on zeroed accumulators; for every slot met in a (block, side) the butterfly adds the members' terms,
// zeros elsewhere, onto the target's current run, which every lane holds.  Every target walks on a state of its own (slot,
// members, run index, 6 or 12 sums) and stores its own part of a finished run, so that only one target's terms are live at
// a time; the states' integers are the same for all targets.  Lanes beyond the last edge take part (slot K); lanes behind
// the line's end add nothing.  Every run is written at most once and never read by this launch.
// Second launch, zf_sum_kernel.  One workgroup per (slot, target): a lane takes every 256th line, skips the lines the slot
// cannot meet, finds the slot's run in the line's two sorted lists by bisection and adds them; butterfly, four waves, the
// scale, one record.
//
// Nothing is contracted and every accumulator starts at +0.0: two calls agree to the bit, and a record depends neither on
// the other sets, the other edges, the other targets nor on H being asked for.
#include "nearfield_math.h"

#pragma clang fp contract(off)

#include "fields_dev.h"
#include "fields_zone_fields.h"
#include "propagate_direct.h"   // prop_two_diff
#include "propagate_pair.h"

namespace ml {

struct ZfArgs {
    const double2 *fields;   // [4][nx][ny]: Ex, Ey, Hx, Hy of the set of the walk
    const double *x2, *y2;   // [nx], [ny]
    const double *e2;        // [K]
    const double *tx, *ty, *tz, *tx_lo, *ty_lo;   // of the walk's first target: x - x0, y - y0 (two doubles each) and z
    double *runs;            // [nx][cap][1 + ZF_TG NQ]
    int2 *line_runs;         // [nx]: runs of side L, runs of side R
    int nx, ny, K, cap, jv, nt;   // nt: targets of the walk, 1 ... ZF_TG
    double dxp, dyp, k, inv_k, Z;
};

// what a lane holds of a block: its sample's squared distance (behind the line's end: none) and its four fields
struct ZfBlock {
    double r2;
    bool live;
    double2 f[4];
};

__device__ __forceinline__ void zf_fetch(const ZfArgs &a, const double2 *row, size_t plane, double x2, int j, ZfBlock &b) {
    b.live = j < a.ny;
    b.r2 = b.live ? x2 + a.y2[j] : INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c) b.f[c] = make_double2(0.0, 0.0);
    if (b.live) {
#pragma unroll
        for (int c = 0; c < 4; ++c) b.f[c] = row[(size_t)c * plane + j];
    }
}

// the run a target's walk is adding to (every lane holds the same values), and where its next finished run goes
template <int NQ>
struct ZfWalk {
    int zone, n, slot;
    double v[NQ];
};

template <int NQ>
__device__ __forceinline__ void zf_flush(const ZfArgs &a, double *list, ZfWalk<NQ> &w, int g, int lane) {
    if (w.zone < 0) return;
    if (lane == 0 && w.slot < a.cap) {   // (the capacity holds every run of a line: fields_zone_fields.h zf_run_capacity)
        double *r = list + (size_t)w.slot * (1 + ZF_TG * NQ);
        if (g == 0) *reinterpret_cast<int2 *>(r) = make_int2(w.zone, w.n);
#pragma unroll
        for (int q = 0; q < NQ; ++q) r[1 + g * NQ + q] = w.v[q];
    }
    ++w.slot;
    w.zone = -1;
}

// every slot met among the lanes of `in_side`: the members' terms by the butterfly onto the current run
template <int NQ>
__device__ __forceinline__ void zf_add(const ZfArgs &a, double *list, ZfWalk<NQ> &w, int g, int zone, bool in_side,
                                       const double (&t)[NQ], int lane) {
    unsigned long long todo = __ballot(in_side);
    while (todo) {
        const int k = __shfl(zone, __ffsll((long long)todo) - 1, 64);
        const bool mine = in_side && zone == k;
        const unsigned long long members = __ballot(mine);
        if (k != w.zone) {
            zf_flush<NQ>(a, list, w, g, lane);
            w.zone = k;
            w.n = 0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) w.v[q] = 0.0;
        }
        w.n += __popcll(members);
#pragma unroll
        for (int q = 0; q < NQ; ++q) w.v[q] += pass_wave_sum(mine ? t[q] : 0.0);
        todo &= ~members;
    }
}

template <bool WANT_H>
__global__ __launch_bounds__(PASS_LINE_THREADS) void zf_line_kernel(const ZfArgs a) {
    constexpr int NQ = WANT_H ? ZF_EH_DOUBLES : ZF_E_DOUBLES;
    extern __shared__ double s_e2[];
    for (int k = threadIdx.x; k < a.K; k += PASS_LINE_THREADS) s_e2[k] = a.e2[k];
    __syncthreads();
    const int lane = threadIdx.x & 63, line = blockIdx.x * (PASS_LINE_THREADS / 64) + (threadIdx.x >> 6);
    if (line >= a.nx) return;
    const double x2 = a.x2[line];
    const size_t plane = (size_t)a.nx * a.ny;
    const double2 *row = a.fields + (size_t)line * a.ny;
    double *list = a.runs + (size_t)line * a.cap * (1 + ZF_TG * NQ);
    ZfWalk<NQ> w[ZF_TG];
    int runs_l[ZF_TG];
#pragma unroll
    for (int g = 0; g < ZF_TG; ++g) {
        w[g].zone = -1;
        w[g].n = w[g].slot = 0;
        runs_l[g] = 0;
    }
    const int blocks = pass_blocks(a.ny);
    ZfBlock cur, nxt;
    zf_fetch(a, row, plane, x2, lane, cur);
    for (int b = 0; b < blocks; ++b) {
        const int j0 = b * PASS_BLOCK, j = j0 + lane;
        if (b + 1 < blocks) zf_fetch(a, row, plane, x2, j + PASS_BLOCK, nxt);   // (in flight over this block's arithmetic)
        const int zone = cur.live ? pass_find(s_e2, a.K, cur.r2) : a.K;
        // the currents, as propagate_kernel stages them
        const double2 v0 = pair_current(-1.0, 1.0, cur.f[3]), v1 = pair_current(1.0, 1.0, cur.f[2]);
        const double2 v2 = pair_current(1.0, a.Z, cur.f[1]), v3 = pair_current(-1.0, a.Z, cur.f[0]);
        const c2 Jx = {v0.x, v0.y}, Jy = {v1.x, v1.y}, Mx = {v2.x, v2.y}, My = {v3.x, v3.y};
        const bool vertex_here = j0 <= a.jv && a.jv < j0 + PASS_BLOCK;
#pragma unroll
        for (int g = 0; g < ZF_TG; ++g) {
            if (g >= a.nt) break;
            const double z = a.tz[g];
            const double dx = pair_offset(line, a.dxp, a.tx[g], a.tx_lo[g]);
            const double s_row = fma(dx, dx, z * z);
            const double dy = pair_offset(j, a.dyp, a.ty[g], a.ty_lo[g]);
            const PairGeom p = pair_geom(dx, dy, z, s_row, a.k, a.inv_k);
            c2 E[3] = {c2{0, 0}, c2{0, 0}, c2{0, 0}};
            pair_term<-1>(E, p.w, p.q, p.a, p.b, p.ux, p.uy, p.uz, Jx, Jy, Mx, My);
            double t[NQ];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                t[2 * d] = E[d].r;
                t[2 * d + 1] = E[d].i;
            }
            if (WANT_H) {
                c2 H[3] = {c2{0, 0}, c2{0, 0}, c2{0, 0}};
                pair_term<1>(H, p.w, p.q, p.a, p.b, p.ux, p.uy, p.uz, Mx, My, Jx, Jy);
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    t[(NQ - 6) + 2 * d] = H[d].r;
                    t[(NQ - 6) + 2 * d + 1] = H[d].i;
                }
            }
            zf_add<NQ>(a, list, w[g], g, zone, cur.live && j <= a.jv, t, lane);
            if (vertex_here) {   // the vertex's block: side L ends here
                zf_flush<NQ>(a, list, w[g], g, lane);
                runs_l[g] = w[g].slot;
            }
            zf_add<NQ>(a, list, w[g], g, zone, cur.live && j > a.jv, t, lane);
        }
        if (b + 1 < blocks) cur = nxt;
    }
#pragma unroll
    for (int g = 0; g < ZF_TG; ++g)
        if (g < a.nt) zf_flush<NQ>(a, list, w[g], g, lane);
    if (lane == 0) a.line_runs[line] = make_int2(runs_l[0], w[0].slot - runs_l[0]);
}

// the run of `zone` among n runs of `rs` doubles whose slots descend (dir = -1) or ascend (dir = 1) strictly, or nullptr
__device__ __forceinline__ const double *zf_run_of(const double *list, int rs, int n, int zone, int dir) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (dir * (reinterpret_cast<const int *>(list + (size_t)mid * rs)[0] - zone) < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && reinterpret_cast<const int *>(list + (size_t)lo * rs)[0] == zone ? list + (size_t)lo * rs : nullptr;
}

// records [K + 1][T][NQ], samples [K + 1]: target t0 + blockIdx.y of slot blockIdx.x
template <int NQ>
__global__ __launch_bounds__(ZONES_SUM_THREADS) void zf_sum_kernel(const double *runs, const int2 *line_runs, const double *x2,
                                                                   const double *e2, double *records, long long *samples, int nx,
                                                                   int cap, int K, int t0, int T, double y2_min, double y2_max,
                                                                   double scale_e, double scale_h) {
    constexpr int RS = 1 + ZF_TG * NQ;
    __shared__ double s_red[ZONES_SUM_THREADS / 64][NQ + 1];
    const int tid = threadIdx.x, z = blockIdx.x, g = blockIdx.y;
    const double e_hi = z < K ? e2[z] : INFINITY, e_lo = z > 0 ? e2[z - 1] : -1.0;   // (r2 >= 0 > -1: zone 0 has no inner edge)
    double acc[NQ + 1];   // the sums, then the members
#pragma unroll
    for (int q = 0; q < NQ + 1; ++q) acc[q] = 0.0;
    long long n = 0;
    for (int i = tid; i < nx; i += ZONES_SUM_THREADS) {
        const double x = x2[i];
        if (!(x + y2_min <= e_hi) || x + y2_max <= e_lo) continue;   // every sample of the line lies outside / inside the ring
        int2 lr = line_runs[i];
        lr.x = min(lr.x, cap);   // (never more than the capacity: the lists are read inside their line)
        lr.y = min(lr.y, cap - lr.x);
        const double *list = runs + (size_t)i * cap * RS;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const double *r = side == 0 ? zf_run_of(list, RS, lr.x, z, -1) : zf_run_of(list + (size_t)lr.x * RS, RS, lr.y, z, 1);
            if (!r) continue;
            n += reinterpret_cast<const int *>(r)[1];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] += r[1 + g * NQ + q];
        }
    }
    acc[NQ] = (double)n;   // (integers below 2^53: exact in any order)
#pragma unroll
    for (int q = 0; q < NQ + 1; ++q) acc[q] = pass_wave_sum(acc[q]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int q = 0; q < NQ + 1; ++q) s_red[tid >> 6][q] = acc[q];
    __syncthreads();
    if (tid <= NQ) {
        const double sum = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
        if (tid < NQ)
            records[((size_t)z * T + t0 + g) * NQ + tid] = (tid < 6 ? scale_e : scale_h) * sum;
        else if (t0 + g == 0)
            samples[z] = (long long)sum;
    }
}

template <bool WANT_H>
static void zf_walk(hipStream_t stream, const ZfArgs &a, double *records, long long *samples, int t0, int T, double y2_min,
                    double y2_max, double scale_e, double scale_h) {
    constexpr int NQ = WANT_H ? ZF_EH_DOUBLES : ZF_E_DOUBLES;
    const int lines = PASS_LINE_THREADS / 64;
    hipLaunchKernelGGL((zf_line_kernel<WANT_H>), dim3((a.nx + lines - 1) / lines), dim3(PASS_LINE_THREADS), (size_t)a.K * sizeof(double),
                       stream, a);
    hipLaunchKernelGGL((zf_sum_kernel<NQ>), dim3(a.K + 1, a.nt), dim3(ZONES_SUM_THREADS), 0, stream, a.runs, a.line_runs, a.x2, a.e2,
                       records, samples, a.nx, a.cap, a.K, t0, T, y2_min, y2_max, scale_e, scale_h);
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_fields_zone_fields(ml_ctx *ctx, int first_set, int n_sets, double x0, double y0, double dxp, double dyp, double wavelength,
                          double n_glass, double Z0, const double *x2, int nx, const double *y2, int ny, const double *e2, int n_edges,
                          const double *tx, const double *ty, const double *tz, int n_targets, int want_h, double *records,
                          long long *samples) {
    ML_REQUIRE(ctx && records && samples, "NULL argument");
    char why[400];
    ML_TRY(pass_checked(zf_check(pass_state(ctx), first_set, n_sets, dxp, dyp, wavelength, n_glass, Z0, x2, nx, y2, ny, e2, n_edges, tx,
                                 ty, tz, n_targets, why, sizeof why), why));
    ML_REQUIRE(std::isfinite(x0) && std::isfinite(y0), "ml_fields_zone_fields: the aperture's origin (%g, %g) must be finite", x0, y0);
    // no pair of the call may leave the range of the phase arithmetic: the targets' bounding box, as a propagation plan's
    PropExtent ext;
    ext.tx_lo = *std::min_element(tx, tx + n_targets) - x0;
    ext.tx_hi = *std::max_element(tx, tx + n_targets) - x0;
    ext.ty_lo = *std::min_element(ty, ty + n_targets) - y0;
    ext.ty_hi = *std::max_element(ty, ty + n_targets) - y0;
    ext.z_hi = *std::max_element(tz, tz + n_targets);
    ML_TRY(prop_check_phase("ml_fields_zone_fields", ext, nx, ny, dxp, dyp, wavelength, n_glass));
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(fields_unmodulate(ctx));   // as ml_fields_download: the plain near field
    const int K = n_edges, T = n_targets, cap = (int)zf_run_capacity(ny, K);
    const bool h = want_h != 0;
    const int nq = zf_record_doubles(h);
    PassPack in;   // the inputs in one upload: x2 [nx]; y2 [ny]; e2 [K]; the targets [5][T] as a propagation plan keeps them
    const size_t at_x2 = in.add(x2, nx), at_y2 = in.add(y2, ny), at_e2 = in.add(e2, K), at_t = in.add(nullptr, (size_t)PROP_TARGET_ROWS * T);
    for (int t = 0; t < T; ++t) {
        double *p = in.h.data() + at_t + t;
        p[0] = prop_two_diff(tx[t], x0, &p[3 * (size_t)T]);
        p[T] = prop_two_diff(ty[t], y0, &p[4 * (size_t)T]);
        p[2 * (size_t)T] = tz[t];
    }
    const size_t rec_doubles = (size_t)(K + 1) * T * nq;
    ML_TRY(ctx->zf_in.reserve(in.bytes()));
    ML_TRY(ctx->zf_runs.reserve((size_t)zf_scratch_bytes(nx, ny, K, h)));
    ML_TRY(ctx->zf_records.reserve((rec_doubles + (size_t)(K + 1)) * 8));
    ML_HIP(hipMemcpyAsync(ctx->zf_in.p, in.h.data(), in.bytes(), hipMemcpyHostToDevice, ctx->stream));
    const double *d_in = ctx->zf_in.as<double>();
    ZfArgs a;
    a.x2 = d_in + at_x2;
    a.y2 = d_in + at_y2;
    a.e2 = d_in + at_e2;
    a.runs = ctx->zf_runs.as<double>();
    a.line_runs = reinterpret_cast<int2 *>(a.runs + (size_t)nx * cap * zf_run_doubles(h));   // behind the lists: 8-byte aligned
    a.nx = nx;
    a.ny = ny;
    a.K = K;
    a.cap = cap;
    a.jv = pass_vertex(y2, ny);
    a.dxp = dxp;
    a.dyp = dyp;
    a.k = 2.0 * M_PI * n_glass / wavelength;
    a.inv_k = 1.0 / a.k;
    a.Z = Z0 / n_glass;
    const double scale_h = a.k * a.k / (4.0 * M_PI) * dxp * dyp, scale_e = a.Z * scale_h;
    const double y2_min = y2[a.jv], y2_max = std::max(y2[0], y2[ny - 1]);
    double *rec = ctx->zf_records.as<double>();
    long long *cnt = reinterpret_cast<long long *>(rec + rec_doubles);
    for (int m = 0; m < n_sets; ++m) {
        a.fields = ctx->fields.buf.as<double2>() + (size_t)(first_set + m) * 4 * nx * ny;
        for (int t0 = 0; t0 < T; t0 += ZF_TG) {
            const double *dt = d_in + at_t + t0;
            a.tx = dt;
            a.ty = dt + T;
            a.tz = dt + 2 * (size_t)T;
            a.tx_lo = dt + 3 * (size_t)T;
            a.ty_lo = dt + 4 * (size_t)T;
            a.nt = std::min(ZF_TG, T - t0);
            if (h)
                zf_walk<true>(ctx->stream, a, rec, cnt, t0, T, y2_min, y2_max, scale_e, scale_h);
            else
                zf_walk<false>(ctx->stream, a, rec, cnt, t0, T, y2_min, y2_max, scale_e, scale_h);
            ML_HIP(hipGetLastError());
        }
        // (the copy is ordered behind the set's walks and in front of the next set's on the stream)
        ML_HIP(hipMemcpyAsync(records + (size_t)m * rec_doubles, rec, rec_doubles * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    ML_HIP(hipMemcpyAsync(samples, cnt, (size_t)(K + 1) * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

}  // extern "C"
