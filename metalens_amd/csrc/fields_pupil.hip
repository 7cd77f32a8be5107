// A pupil function applied to the resident near field where it lies (ml_fields_pupil_plan, ml_fields_pupil_apply): an
// aperture stop, one complex factor per zone and a Zernike phase plate, multiplied into the field sets in place, so that
// the transform, the propagator, the zone and wavefront analyses and a sweep see the modified aperture without a change of
// their own.  Definitions, which samples change and how every value is formed: fields_pupil.h.  The reference has no
// counterpart (SURVEY.md section 4 ends at "checked by eye").
//
// The plan does the host's share once: it checks the call, forms the monomial coefficients B_pq of the phase plate and the
// per-line table b_q(i) = sum_p B_pq xi^p, and uploads axes, table, edges and factors into one buffer of the context.
//
// The pass, pupil_line_kernel<NS, NQ, EDGES>, is ONE launch: one wave per line, four lines per workgroup, as
// wavefront_line_kernel; the squared edges lie in the LDS (8 K bytes) and a lane finds its zone there by bisection, the
// zone's factor is a gather from global memory (K <= 4096 factors: they stay in the caches).  The wave takes the line in
// blocks of 64 samples in ascending order.  Membership, zone, psi and its sincos are computed once per sample and serve all
// NS sets of the call; per set the four fields of a sample are four 16-byte loads and four 16-byte stores past the
// caches, coalesced over the wave, and the loads of block b + 1 are issued before the arithmetic of block b.  What a lane
// does NOT do: a stopped non-member is stored as zeros and never loaded; a line whose vertex lies outside a stopped pupil
// is stores only; a sample whose factor is exactly 1 - without stop and edges every non-member, and with them whatever
// lies outside the last edge - is neither loaded nor stored.  No atomics, no reduction, nothing read back: the launch is
// queued and the entry returns.
#include "nearfield_math.h"

#pragma clang fp contract(off)

#include "fields_dev.h"

namespace ml {

struct PupilArgs {
    double2 *fields;         // [NS][4][nx][ny]: Ex, Ey, Hx, Hy of the first set of the call, the others behind it
    const double *x2, *y2;   // [nx], [ny]
    const double *eta;       // [ny]
    const double *table;     // [nx][PUPIL_NQ]: b_q(i)
    const double *e2;        // [K]
    const double *g;         // [K][2]
    int nx, ny, K, jv, stop;
    double r2;
};

// one 16-byte store past the caches, as the synthesis stores its fields: at 4096^2 a set is 1 GB, nothing of it is still
// cached when the transform reads it, and with the transform right behind the pass this was the faster of the two
// (0.585 ms against 0.594 with plain stores)
__device__ __forceinline__ void pupil_store(double2 *p, double re, double im) {
    typedef double double2v __attribute__((ext_vector_type(2)));
    __builtin_nontemporal_store((double2v){re, im}, reinterpret_cast<double2v *>(p));
}

// what a lane holds of a block: what becomes of its sample, then its pupil coordinate, its zone factor and the four
// fields of every set
template <int NS>
struct PupilBlock {
    bool member, touch, zero;   // touch: multiplied by a factor; zero: a stopped non-member
    double eta;
    double2 g;
    double2 f[NS][4];
};

template <int NS, int NQ, bool EDGES>
__device__ __forceinline__ void pupil_fetch(const PupilArgs &a, const double *s_e2, const double2 *row, size_t plane, double x2, int j,
                                            PupilBlock<NS> &b) {
    const bool in_line = j < a.ny;
    const double r2 = in_line ? x2 + a.y2[j] : INFINITY;
    b.member = r2 <= a.r2;
    b.zero = in_line && !b.member && a.stop;
    b.eta = 0.0;
    b.g = make_double2(1.0, 0.0);
    bool factor = false;   // a zone factor of its own
    if (EDGES && in_line && !b.zero) {
        const int z = pass_find(s_e2, a.K, r2);
        if (z < a.K) {   // (z < K: inside g)
            factor = true;
            b.g = make_double2(a.g[2 * z], a.g[2 * z + 1]);
        }
    }
    b.touch = in_line && !b.zero && (factor || (NQ > 0 && b.member));
    pass_zero<NS>(b.f);
    if (b.touch) {   // (j < ny: inside the line)
        if (NQ > 0 && b.member) b.eta = a.eta[j];
        pass_load<NS>(b.f, row, plane, j);
    }
}

template <int NS, int NQ, bool EDGES>
__global__ __launch_bounds__(PASS_LINE_THREADS) void pupil_line_kernel(const PupilArgs a) {
    extern __shared__ double s_e2[];
    if (EDGES) {
        for (int k = threadIdx.x; k < a.K; k += PASS_LINE_THREADS) s_e2[k] = a.e2[k];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int line = __builtin_amdgcn_readfirstlane(blockIdx.x * (PASS_LINE_THREADS / 64) + (threadIdx.x >> 6));
    if (line >= a.nx) return;
    const double x2 = a.x2[line];
    const size_t plane = (size_t)a.nx * a.ny;
    double2 *row = a.fields + (size_t)line * a.ny;
    if (!(x2 + a.y2[a.jv] <= a.r2)) {   // the vertex lies outside: so does the line
        if (a.stop) {                   // stores only
            for (int j = lane; j < a.ny; j += PASS_BLOCK)
#pragma unroll
                for (int q = 0; q < 4 * NS; ++q) pupil_store(row + (size_t)q * plane + j, 0.0, 0.0);
            return;
        }
        if (!EDGES) return;             // every factor is exactly 1
    }
    double bq[NQ > 0 ? NQ : 1];
#pragma unroll
    for (int q = 0; q < NQ; ++q) bq[q] = a.table[(size_t)line * PUPIL_NQ + q];
    const int blocks = pass_blocks(a.ny);
    PupilBlock<NS> cur, nxt;
    pupil_fetch<NS, NQ, EDGES>(a, s_e2, row, plane, x2, lane, cur);
    for (int b = 0; b < blocks; ++b) {
        const int j = b * PASS_BLOCK + lane;
        if (b + 1 < blocks) pupil_fetch<NS, NQ, EDGES>(a, s_e2, row, plane, x2, j + PASS_BLOCK, nxt);   // (in flight over this block's arithmetic)
        if (cur.zero) {   // (zero: j < ny)
#pragma unroll
            for (int q = 0; q < 4 * NS; ++q) pupil_store(row + (size_t)q * plane + j, 0.0, 0.0);
        } else if (cur.touch) {   // (touch: j < ny)
            double fr = cur.g.x, fi = cur.g.y;
            if (NQ > 0 && cur.member) {
                double psi = bq[NQ > 0 ? NQ - 1 : 0];   // Horner in eta, q descending
#pragma unroll
                for (int q = NQ - 2; q >= 0; --q) psi = psi * cur.eta + bq[q];
                double sn, cs;
                sincos_cw(psi, sn, cs);
                fr = cur.g.x * cs - cur.g.y * sn;
                fi = cur.g.x * sn + cur.g.y * cs;
            }
#pragma unroll
            for (int m = 0; m < NS; ++m)
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    const double2 E = cur.f[m][f];
                    pupil_store(row + (size_t)(4 * m + f) * plane + j, E.x * fr - E.y * fi, E.x * fi + E.y * fr);
                }
        }
        if (b + 1 < blocks) cur = nxt;
    }
}

template <int NS, int NQ>
static void pupil_launch_edges(hipStream_t stream, dim3 grid, const PupilArgs &a) {
    if (a.K > 0)
        hipLaunchKernelGGL((pupil_line_kernel<NS, NQ, true>), grid, dim3(PASS_LINE_THREADS), (size_t)a.K * sizeof(double), stream, a);
    else
        hipLaunchKernelGGL((pupil_line_kernel<NS, NQ, false>), grid, dim3(PASS_LINE_THREADS), 0, stream, a);
}

template <int NS>
static void pupil_launch_phase(hipStream_t stream, dim3 grid, const PupilArgs &a, int nq) {
    if (nq == 0)
        pupil_launch_edges<NS, 0>(stream, grid, a);
    else if (nq == 5)
        pupil_launch_edges<NS, 5>(stream, grid, a);
    else
        pupil_launch_edges<NS, PUPIL_NQ>(stream, grid, a);
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_fields_pupil_plan(ml_ctx *ctx, const double *x2, const double *xi, int nx, const double *y2, const double *eta, int ny, double r2,
                         int stop, int n_max, const double *c, const double *e2, int n_edges, const double *g) {
    ML_REQUIRE(ctx, "NULL argument");
    char why[400];
    double B[PUPIL_NQ * PUPIL_NQ];
    ML_TRY(pass_checked(pupil_check(ctx->n_ranks, x2, xi, nx, y2, eta, ny, r2, stop, n_max, c, e2, n_edges, g, B, why, sizeof why), why));
    ML_HIP(hipSetDevice(ctx->device));
    const int K = n_edges;
    // the plan's arrays in one upload of pupil_plan_doubles(nx, ny, K) doubles; the plan keeps where each begins
    PassPack in;
    PupilPlan next;
    next.x2 = in.add(x2, nx);
    next.y2 = in.add(y2, ny);
    next.eta = in.add(eta, ny);
    next.table = in.add(nullptr, (size_t)nx * PUPIL_NQ);
    pupil_line_table(n_max, B, xi, nx, in.h.data() + next.table);
    next.e2 = in.add(e2, K);
    next.g = in.add(g, 2 * (size_t)K);
    // a pass of the plan before may still read the buffer: the copy is queued behind it, and a larger buffer is
    // allocated only once the stream has drained
    if (in.bytes() > ctx->pupil_in.bytes) ML_HIP(hipStreamSynchronize(ctx->stream));
    ML_TRY(ctx->pupil_in.reserve(in.bytes()));
    ML_HIP(hipMemcpyAsync(ctx->pupil_in.p, in.h.data(), in.bytes(), hipMemcpyHostToDevice, ctx->stream));
    PupilPlan &p = ctx->pupil;
    p.valid = false;
    ML_HIP(hipStreamSynchronize(ctx->stream));   // the host arrays leave with this call
    p = next;
    p.nx = nx;
    p.ny = ny;
    p.K = K;
    p.jv = pass_vertex(y2, ny);
    p.nq = !c ? 0 : n_max <= 4 ? 5 : PUPIL_NQ;
    p.stop = stop;
    p.r2 = r2;
    p.valid = true;
    return ML_OK;
}

int ml_fields_pupil_apply(ml_ctx *ctx, int first_set, int n_sets) {
    ML_REQUIRE(ctx, "NULL argument");
    char why[400];
    ML_TRY(pass_checked(pupil_apply_check(pass_state(ctx), ctx->pupil, first_set, n_sets, why, sizeof why), why));
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(fields_unmodulate(ctx));   // as ml_fields_download: the plain near field
    const PupilPlan &p = ctx->pupil;
    PupilArgs a;
    a.fields = ctx->fields.buf.as<double2>() + (size_t)first_set * 4 * p.nx * p.ny;
    const double *d_in = ctx->pupil_in.as<double>();
    a.x2 = d_in + p.x2;
    a.y2 = d_in + p.y2;
    a.eta = d_in + p.eta;
    a.table = d_in + p.table;
    a.e2 = d_in + p.e2;
    a.g = d_in + p.g;
    a.nx = p.nx;
    a.ny = p.ny;
    a.K = p.K;
    a.jv = p.jv;
    a.stop = p.stop;
    a.r2 = p.r2;
    const int lines = PASS_LINE_THREADS / 64;
    const dim3 grid((p.nx + lines - 1) / lines);
    pass_for_sets(n_sets, [&](auto ns) { pupil_launch_phase<decltype(ns)::value>(ctx->stream, grid, a, p.nq); });
    ML_HIP(hipGetLastError());
    // the fields are no longer the synthesis's: nothing is assumed about the zeros outside the lens, and row_first is
    // not theirs - the next synthesis writes every sample again
    ctx->caches.fields_overwritten();
    return ML_OK;
}

}  // extern "C"
