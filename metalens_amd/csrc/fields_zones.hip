// Per-zone sums of the resident near field (ml_fields_zones): for every zone of a list of ring edges about a centre - the
// Fresnel zones of a lens - and every field set of a call the members, the sums of Sz, |Ex|^2, |Ey|^2 and the complex
// overlaps sum Ex conj(w), sum Ey conj(w) with a reference wave w, reduced where the fields lie.  Definitions, the order of
// every sum and the scratch: fields_zones.h.  The reference has no counterpart ("checked by eye").
//
// A lens has hundreds to thousands of zones: no bin per zone fits the LDS (propagate_focus.hip keeps 32), and a dense
// record per workgroup and zone would be larger than the fields.  But along a line of contiguous samples the zone index is
// monotone on each side of the line's vertex, so the members of a zone on one side of a line are one run of samples:
// the first launch walks the lines and stores one record per RUN, the second adds every zone's runs in a fixed order -
// the store pass and the per-destination sum pass that take the place of float atomics, whose sums are not repeatable.
//
// First launch, zones_line_kernel<NS>.  One wave per line, four lines per workgroup; the squared edges lie in the LDS
// (8 K bytes).  The wave takes the line in blocks of 64 samples in ascending order.  Zone, phase and sincos of a sample
// are computed once and serve all NS sets of the call; per set the four fields of a sample are four 16-byte loads,
// coalesced over the wave, and the loads of block b + 1 are issued before the arithmetic of block b.  A lane whose
// sample lies outside the largest edge (or behind the line's end) loads nothing: a block wholly outside costs its index
// arithmetic, a line wholly outside (its vertex is) nothing.  For every zone met in a (block, side) the members' terms
// are summed by the butterfly, zeros elsewhere (the idiom of propagate_focus.hip focus_annuli_add), and added to the
// running record of the current run, which every lane holds; when the zone changes lane 0 stores the finished run.  Every
// slot is written at most once and never read by this launch.
// Second launch, zones_sum_kernel.  One workgroup per (zone, set): a lane takes every 256th line, skips the lines the zone
// cannot meet (X2[i] + min Y2 > E2[z], or X2[i] + max Y2 <= E2[z - 1]), finds the zone's run in the line's two sorted lists
// by bisection and adds them; butterfly, four waves, one record.
//
// Nothing is contracted (-ffp-contract=off) and every accumulator starts at +0.0, so none is ever -0.0 and the blocks,
// lines and lanes that add nothing leave no trace: the record of zone (e_a, e_b] has the same bits whatever the other
// edges are, the record of a set the same bits whatever the other sets of the call are, and two calls agree to the bit.
#include "nearfield_math.h"

#pragma clang fp contract(off)

#include "fields_dev.h"

namespace ml {

// a finished run: the members of one zone on one side of one line, 64 bytes
struct alignas(ZONES_RUN_BYTES) ZoneRun {
    int zone, n;
    double v[ZONES_TERMS];
};
static_assert(sizeof(ZoneRun) == ZONES_RUN_BYTES, "a run is one 64-byte slot");

struct ZonesArgs {
    const double2 *fields;   // [NS][4][nx][ny]: Ex, Ey, Hx, Hy of the first set of the call, the others behind it
    const double *x2, *y2;   // [nx], [ny]
    const double *ra, *rb;   // [nx], [ny]: the reference wave's per-axis arrays
    const double *e2;        // [K]
    ZoneRun *runs;           // [NS][nx][cap]
    int2 *line_runs;         // [nx]: runs of side L, runs of side R
    int nx, ny, K, cap, jv, focus;
    double zz, sk;           // focus: ref_c ref_c and -sign(ref_c) k
};

// what a lane holds of a block: its sample's squared distance, whether it lies inside the largest edge, and then its
// share of the reference phase and the four fields of every set
template <int NS>
struct ZoneBlock {
    double r2, rb;
    bool member;
    double2 f[NS][4];
};

template <int NS>
__device__ __forceinline__ void zones_fetch(const ZonesArgs &a, const double2 *row, size_t plane, double x2, double e2_max, int j,
                                            ZoneBlock<NS> &b) {
    b.r2 = j < a.ny ? x2 + a.y2[j] : INFINITY;
    b.member = b.r2 <= e2_max;
    b.rb = 0.0;
    pass_zero<NS>(b.f);
    if (b.member) {
        b.rb = a.rb[j];
        pass_load<NS>(b.f, row, plane, j);
    }
}

// the run a wave is adding to (every lane holds the same values), and where the next finished run goes
template <int NS>
struct ZoneWalk {
    int zone, n, slot;
    double v[NS][ZONES_TERMS];
};

template <int NS>
__device__ __forceinline__ void zones_flush(const ZonesArgs &a, ZoneRun *list, ZoneWalk<NS> &w, int lane) {
    if (w.zone < 0) return;
    if (lane == 0 && w.slot < a.cap) {   // (the capacity holds every run of a line: fields_zones.h zones_run_capacity)
#pragma unroll
        for (int m = 0; m < NS; ++m) {
            ZoneRun r;
            r.zone = w.zone;
            r.n = w.n;
#pragma unroll
            for (int q = 0; q < ZONES_TERMS; ++q) r.v[q] = w.v[m][q];
            list[(size_t)m * a.nx * a.cap + w.slot] = r;
        }
    }
    ++w.slot;
    w.zone = -1;
}

// every zone met among the lanes of `in_side`: the members' terms by the butterfly onto the current run
template <int NS>
__device__ __forceinline__ void zones_add(const ZonesArgs &a, ZoneRun *list, ZoneWalk<NS> &w, int zone, bool in_side,
                                          const double (&t)[NS][ZONES_TERMS], int lane) {
    unsigned long long todo = __ballot(in_side && zone < a.K);
    while (todo) {
        const int k = __shfl(zone, __ffsll((long long)todo) - 1, 64);
        const bool mine = in_side && zone == k;
        const unsigned long long members = __ballot(mine);
        if (k != w.zone) {
            zones_flush<NS>(a, list, w, lane);
            w.zone = k;
            w.n = 0;
#pragma unroll
            for (int m = 0; m < NS; ++m)
#pragma unroll
                for (int q = 0; q < ZONES_TERMS; ++q) w.v[m][q] = 0.0;
        }
        w.n += __popcll(members);
#pragma unroll
        for (int m = 0; m < NS; ++m)
#pragma unroll
            for (int q = 0; q < ZONES_TERMS; ++q) w.v[m][q] += pass_wave_sum(mine ? t[m][q] : 0.0);
        todo &= ~members;
    }
}

template <int NS>
__global__ __launch_bounds__(PASS_LINE_THREADS) void zones_line_kernel(const ZonesArgs a) {
    extern __shared__ double s_e2[];
    for (int k = threadIdx.x; k < a.K; k += PASS_LINE_THREADS) s_e2[k] = a.e2[k];
    __syncthreads();
    const int lane = threadIdx.x & 63, line = blockIdx.x * (PASS_LINE_THREADS / 64) + (threadIdx.x >> 6);
    if (line >= a.nx) return;
    const double x2 = a.x2[line], ra = a.ra[line], e2_max = s_e2[a.K - 1];
    if (!(x2 + a.y2[a.jv] <= e2_max)) {   // the vertex lies outside: so does the line
        if (lane == 0) a.line_runs[line] = make_int2(0, 0);
        return;
    }
    const size_t plane = (size_t)a.nx * a.ny;
    const double2 *row = a.fields + (size_t)line * a.ny;
    ZoneRun *list = a.runs + (size_t)line * a.cap;
    ZoneWalk<NS> w;
    w.zone = -1;
    w.n = w.slot = 0;
    int runs_l = 0;
    const int blocks = pass_blocks(a.ny);
    ZoneBlock<NS> cur, nxt;
    zones_fetch<NS>(a, row, plane, x2, e2_max, lane, cur);
    for (int b = 0; b < blocks; ++b) {
        const int j0 = b * PASS_BLOCK, j = j0 + lane;
        if (b + 1 < blocks) zones_fetch<NS>(a, row, plane, x2, e2_max, j + PASS_BLOCK, nxt);   // (in flight over this block's arithmetic)
        if (__ballot(cur.member)) {
            int zone = a.K;
            double t[NS][ZONES_TERMS];
            double sn = 0.0, cs = 1.0;
            if (cur.member) {
                zone = pass_find(s_e2, a.K, cur.r2);
                pass_ref_sincos(a.focus, a.sk, a.zz, ra + cur.rb, sn, cs);
            }
#pragma unroll
            for (int m = 0; m < NS; ++m) pass_terms(cur.f[m], sn, cs, t[m]);
            zones_add<NS>(a, list, w, zone, j <= a.jv, t, lane);
            if (j0 <= a.jv && a.jv < j0 + PASS_BLOCK) {   // the vertex's block: side L ends here
                zones_flush<NS>(a, list, w, lane);
                runs_l = w.slot;
            }
            zones_add<NS>(a, list, w, zone, j > a.jv, t, lane);
        }
        if (b + 1 < blocks) cur = nxt;
    }
    zones_flush<NS>(a, list, w, lane);
    if (lane == 0) a.line_runs[line] = make_int2(runs_l, w.slot - runs_l);
}

// the run of `zone` among n runs whose zones descend (dir = -1) or ascend (dir = 1) strictly, or nullptr
__device__ __forceinline__ const ZoneRun *zones_run_of(const ZoneRun *list, int n, int zone, int dir) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (dir * (list[mid].zone - zone) < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && list[lo].zone == zone ? list + lo : nullptr;
}

__global__ __launch_bounds__(ZONES_SUM_THREADS) void zones_sum_kernel(const ZoneRun *runs, const int2 *line_runs, const double *x2,
                                                                      const double *e2, double *records, int nx, int cap, int K,
                                                                      double y2_min, double y2_max) {
    __shared__ double s_red[ZONES_SUM_THREADS / 64][ZONES_RECORD];
    const int tid = threadIdx.x, z = blockIdx.x, set = blockIdx.y;
    const double e_hi = e2[z], e_lo = z > 0 ? e2[z - 1] : -1.0;   // (r2 >= 0 > -1: zone 0 has no inner edge)
    double acc[ZONES_RECORD];
#pragma unroll
    for (int q = 0; q < ZONES_RECORD; ++q) acc[q] = 0.0;
    int n = 0;
    for (int i = tid; i < nx; i += ZONES_SUM_THREADS) {
        const double x = x2[i];
        if (!(x + y2_min <= e_hi) || x + y2_max <= e_lo) continue;   // every sample of the line lies outside / inside the ring
        int2 lr = line_runs[i];
        lr.x = min(lr.x, cap);   // (never more than the capacity: the lists are read inside their line)
        lr.y = min(lr.y, cap - lr.x);
        const ZoneRun *list = runs + ((size_t)set * nx + i) * cap;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const ZoneRun *r = side == 0 ? zones_run_of(list, lr.x, z, -1) : zones_run_of(list + lr.x, lr.y, z, 1);
            if (!r) continue;
            n += r->n;
#pragma unroll
            for (int q = 0; q < ZONES_TERMS; ++q) acc[1 + q] += r->v[q];
        }
    }
    acc[ZONES_N] = (double)n;   // (integers: exact in any order)
#pragma unroll
    for (int q = 0; q < ZONES_RECORD; ++q) acc[q] = pass_wave_sum(acc[q]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int q = 0; q < ZONES_RECORD; ++q) s_red[tid >> 6][q] = acc[q];
    __syncthreads();
    if (tid < ZONES_RECORD)
        records[((size_t)set * K + z) * ZONES_RECORD + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_fields_zones(ml_ctx *ctx, int first_set, int n_sets, const double *x2, int nx, const double *y2, int ny, const double *e2,
                    int n_edges, int ref_mode, const double *ra, const double *rb, double ref_c, double k, double *records,
                    int record_doubles) {
    ML_REQUIRE(ctx && records, "NULL argument");
    char why[400];
    ML_TRY(pass_checked(zones_check(pass_state(ctx), first_set, n_sets, x2, nx, y2, ny, e2, n_edges, ref_mode, ra, rb, ref_c, k,
                                    record_doubles, why, sizeof why), why));
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(fields_unmodulate(ctx));   // as ml_fields_download: the plain near field
    const int K = n_edges, cap = (int)zones_run_capacity(ny, K);
    PassPack in;   // the inputs in one upload: x2, ra [nx]; y2, rb [ny]; e2 [K]
    const size_t at_x2 = in.add(x2, nx), at_ra = in.add(ra, nx), at_y2 = in.add(y2, ny), at_rb = in.add(rb, ny), at_e2 = in.add(e2, K);
    ML_TRY(ctx->zones_in.reserve(in.bytes()));
    ML_TRY(ctx->zones_runs.reserve((size_t)zones_scratch_bytes(n_sets, nx, ny, K)));
    ML_TRY(ctx->zones_records.reserve((size_t)n_sets * K * ZONES_RECORD * sizeof(double)));
    ML_HIP(hipMemcpyAsync(ctx->zones_in.p, in.h.data(), in.bytes(), hipMemcpyHostToDevice, ctx->stream));
    ZonesArgs a;
    a.fields = ctx->fields.buf.as<double2>() + (size_t)first_set * 4 * nx * ny;
    const double *d_in = ctx->zones_in.as<double>();
    a.x2 = d_in + at_x2;
    a.ra = d_in + at_ra;
    a.y2 = d_in + at_y2;
    a.rb = d_in + at_rb;
    a.e2 = d_in + at_e2;
    a.runs = ctx->zones_runs.as<ZoneRun>();
    a.line_runs = reinterpret_cast<int2 *>(a.runs + (size_t)n_sets * nx * cap);   // behind the lists: 8-byte aligned
    a.nx = nx;
    a.ny = ny;
    a.K = K;
    a.cap = cap;
    a.jv = pass_vertex(y2, ny);
    a.focus = ref_mode == PASS_REF_FOCUS;
    a.zz = ref_c * ref_c;
    a.sk = ref_c > 0 ? -k : k;
    const int lines = PASS_LINE_THREADS / 64;
    pass_for_sets(n_sets, [&](auto ns) {
        hipLaunchKernelGGL((zones_line_kernel<decltype(ns)::value>), dim3((nx + lines - 1) / lines), dim3(PASS_LINE_THREADS),
                           (size_t)K * sizeof(double), ctx->stream, a);
    });
    ML_HIP(hipGetLastError());
    double *rec = ctx->zones_records.as<double>();
    hipLaunchKernelGGL(zones_sum_kernel, dim3(K, n_sets), dim3(ZONES_SUM_THREADS), 0, ctx->stream, a.runs, a.line_runs, a.x2, a.e2, rec,
                       nx, cap, K, y2[a.jv], std::max(y2[0], y2[ny - 1]));
    ML_HIP(hipGetLastError());
    if (record_doubles == ZONES_RECORD) {
        ML_HIP(hipMemcpyAsync(records, rec, (size_t)n_sets * K * ZONES_RECORD * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        ML_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        std::vector<double> out((size_t)n_sets * K * ZONES_RECORD);
        ML_HIP(hipMemcpyAsync(out.data(), rec, out.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        ML_HIP(hipStreamSynchronize(ctx->stream));
        for (size_t r = 0; r < (size_t)n_sets * K; ++r)
            std::copy(out.begin() + r * ZONES_RECORD, out.begin() + (r + 1) * ZONES_RECORD, records + r * record_doubles);
    }
    return ML_OK;
}

}  // extern "C"
