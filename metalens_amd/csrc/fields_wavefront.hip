// Zernike moments of the resident near field's wavefront (ml_fields_zernike): for every field set of a call the members of
// a circular pupil, the sums of Sz, |Ex|^2, |Ey|^2 and the complex moments sum Ex conj(w) Z_j, sum Ey conj(w) Z_j of the
// aperture field against a reference wave w, for the Zernike terms up to radial order n_max <= 8 - tilt, defocus,
// astigmatism, coma, spherical ... - reduced where the fields lie.  Definitions, the order of every sum, the coefficient
// table and the scratch: fields_wavefront.h.  The reference has no counterpart ("checked by eye").
//
// Z_j is a polynomial in the pupil coordinates (xi, eta), so the moments of all J <= 45 terms follow from the monomial
// moments M_pq = sum_i xi[i]^p sum_j C(i, j) eta[j]^q, p + q <= n_max, which are separable: a sample costs n_max + 1
// multiply-adds per real component, no atan2 and no trigonometry beyond the reference wave's sincos.
//
// First launch, wavefront_line_kernel<NS, NQ>.  One wave per line, four lines per workgroup, as zones_line_kernel.  The wave
// takes the line in blocks of 64 samples in ascending order.  Membership, phase and sincos of a sample are computed once
// and serve all NS sets of the call; per set the four fields of a sample are four 16-byte loads, coalesced over the wave,
// and the loads of block b + 1 are issued before the arithmetic of block b.  A non-member loads nothing, a block without
// members is skipped by ballot, a line whose vertex lies outside stores zeros and costs nothing else.  A lane holds 4
// header sums and 4 NQ moment sums per set (NQ = 5 serves n_max <= 4, NQ = 9 the orders up to 8); at the line's end one
// butterfly per accumulator, and lane 0 stores the line record.
// Second launch, wavefront_sum_kernel.  One workgroup per (set, q) and one per set for the header sums: a lane takes every
// 256th line that holds members, forms the powers of xi[i] and adds xi^p T_q(i) for every p <= n_max - q; butterfly, four
// waves, the monomial moments of the set.  The host turns them into the Zernike record (fields_wavefront.h wf_convert).
//
// Nothing is contracted (-ffp-contract=off), every accumulator starts at +0.0 and there are no atomics: two calls agree
// to the bit, the record of a set does not depend on the other sets of the call, and the terms up to order n' have the
// same bits whatever n_max >= n' the call asks for.
#include "nearfield_math.h"

#pragma clang fp contract(off)

#include "fields_dev.h"

namespace ml {

struct WavefrontArgs {
    const double2 *fields;   // [NS][4][nx][ny]: Ex, Ey, Hx, Hy of the first set of the call, the others behind it
    const double *x2, *y2;   // [nx], [ny]
    const double *eta;       // [ny]
    const double *ra, *rb;   // [nx], [ny]: the reference wave's per-axis arrays
    double *lines;           // [NS][nx][lr]: the line records
    int nx, ny, nq, lr, jv, focus;   // nq = n_max + 1, lr = wf_line_record(n_max)
    double r2;               // the squared radius of the pupil
    double zz, sk;           // focus: ref_c ref_c and -sign(ref_c) k
};

// what a lane holds of a block: whether its sample is a member, and then its pupil coordinate, its share of the
// reference phase and the four fields of every set
template <int NS>
struct WavefrontBlock {
    double rb, eta;
    bool member;
    double2 f[NS][4];
};

template <int NS>
__device__ __forceinline__ void wavefront_fetch(const WavefrontArgs &a, const double2 *row, size_t plane, double x2, int j,
                                                WavefrontBlock<NS> &b) {
    b.member = j < a.ny && x2 + a.y2[j] <= a.r2;
    b.rb = b.eta = 0.0;
    pass_zero<NS>(b.f);
    if (b.member) {
        b.rb = a.rb[j];
        b.eta = a.eta[j];
        pass_load<NS>(b.f, row, plane, j);
    }
}

template <int NS, int NQ>
__global__ __launch_bounds__(PASS_LINE_THREADS) void wavefront_line_kernel(const WavefrontArgs a) {
    const int lane = threadIdx.x & 63, line = blockIdx.x * (PASS_LINE_THREADS / 64) + (threadIdx.x >> 6);
    if (line >= a.nx) return;
    const double x2 = a.x2[line], ra = a.ra[line];
    double *out = a.lines + (size_t)line * a.lr;
    const size_t set_stride = (size_t)a.nx * a.lr;
    if (!(x2 + a.y2[a.jv] <= a.r2)) {   // the vertex lies outside: so does the line
        for (int m = 0; m < NS; ++m)
            for (int q = lane; q < a.lr; q += 64) out[m * set_stride + q] = 0.0;
        return;
    }
    const size_t plane = (size_t)a.nx * a.ny;
    const double2 *row = a.fields + (size_t)line * a.ny;
    int n = 0;
    double h[NS][3], t[NS][NQ][4];
#pragma unroll
    for (int m = 0; m < NS; ++m) {
#pragma unroll
        for (int c = 0; c < 3; ++c) h[m][c] = 0.0;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) t[m][q][c] = 0.0;
    }
    const int blocks = pass_blocks(a.ny);
    WavefrontBlock<NS> cur, nxt;
    wavefront_fetch<NS>(a, row, plane, x2, lane, cur);
    for (int b = 0; b < blocks; ++b) {
        if (b + 1 < blocks) wavefront_fetch<NS>(a, row, plane, x2, (b + 1) * PASS_BLOCK + lane, nxt);   // (in flight over this block's arithmetic)
        if (__ballot(cur.member)) {
            if (cur.member) {
                double sn, cs;
                pass_ref_sincos(a.focus, a.sk, a.zz, ra + cur.rb, sn, cs);
                ++n;
                double C[NS][4];
#pragma unroll
                for (int m = 0; m < NS; ++m) {
                    h[m][0] += pass_sz(cur.f[m]);
                    h[m][1] += pass_abs2(cur.f[m][0]);
                    h[m][2] += pass_abs2(cur.f[m][1]);
                    pass_overlap(cur.f[m][0], sn, cs, C[m][0], C[m][1]);
                    pass_overlap(cur.f[m][1], sn, cs, C[m][2], C[m][3]);
                }
                double e = 1.0;   // eta^q by repeated multiplication
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
#pragma unroll
                    for (int m = 0; m < NS; ++m)
#pragma unroll
                        for (int c = 0; c < 4; ++c) t[m][q][c] += C[m][c] * e;
                    e *= cur.eta;
                }
            }
        }
        if (b + 1 < blocks) cur = nxt;
    }
    const double members = pass_wave_sum((double)n);   // (integers: exact in any order)
#pragma unroll
    for (int m = 0; m < NS; ++m) {
        double *rec = out + m * set_stride;
#pragma unroll
        for (int c = 0; c < 3; ++c) h[m][c] = pass_wave_sum(h[m][c]);
        if (lane == 0) {
            rec[WF_N] = members;
            rec[WF_S] = h[m][0];
            rec[WF_IX] = h[m][1];
            rec[WF_IY] = h[m][2];
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
#pragma unroll
            for (int c = 0; c < 4; ++c) t[m][q][c] = pass_wave_sum(t[m][q][c]);
            if (lane == 0 && q < a.nq) {   // (q < nq: inside the line record)
#pragma unroll
                for (int c = 0; c < 4; ++c) rec[WF_HEAD + 4 * q + c] = t[m][q][c];
            }
        }
    }
}

// mono: [sets][WF_HEAD + 4 wf_terms(n_max)], the header sums and the monomial moments in the order of wf_monomial
__global__ __launch_bounds__(WF_SUM_THREADS) void wavefront_sum_kernel(const double *lines, const double *xi, double *mono, int nx,
                                                                       int nq, int lr) {
    constexpr int NP = WF_ORDER_MAX + 1;
    __shared__ double s_red[WF_SUM_THREADS / 64][NP * 4];
    const int tid = threadIdx.x, set = blockIdx.y;
    const int q = (int)blockIdx.x - 1;                    // -1: the header sums
    const int p_max = q < 0 ? 0 : nq - 1 - q;
    const int at = q < 0 ? 0 : WF_HEAD + 4 * q;           // the four doubles of a line record this group adds
    const double *base = lines + (size_t)set * nx * lr;
    double acc[NP][4];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[p][c] = 0.0;
    for (int i = tid; i < nx; i += WF_SUM_THREADS) {
        const double *r = base + (size_t)i * lr;
        if (r[WF_N] == 0.0) continue;   // a line without members adds nothing
        double T[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) T[c] = r[at + c];
        const double x = xi[i];
        double pw = 1.0;   // xi^p by repeated multiplication
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (p <= p_max) {
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[p][c] += pw * T[c];
                pw *= x;
            }
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double v = pass_wave_sum(acc[p][c]);
            if ((tid & 63) == 0) s_red[tid >> 6][4 * p + c] = v;
        }
    __syncthreads();
    const int p = tid >> 2, c = tid & 3;
    if (p <= p_max) {   // (p_max <= 8: inside s_red and inside the set's moments)
        const int n_max = nq - 1;
        const int slot = q < 0 ? c : WF_HEAD + 4 * wf_monomial(n_max, p, q) + c;
        mono[(size_t)set * (WF_HEAD + 4 * wf_terms(n_max)) + slot] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    }
}

template <int NQ>
static void wavefront_launch(hipStream_t stream, dim3 grid, const WavefrontArgs &a, int n_sets) {
    pass_for_sets(n_sets, [&](auto ns) {
        hipLaunchKernelGGL((wavefront_line_kernel<decltype(ns)::value, NQ>), grid, dim3(PASS_LINE_THREADS), 0, stream, a);
    });
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_fields_zernike(ml_ctx *ctx, int first_set, int n_sets, const double *x2, const double *xi, int nx, const double *y2,
                      const double *eta, int ny, double r2, int n_max, int ref_mode, const double *ra, const double *rb, double ref_c,
                      double k, double *records, int record_doubles) {
    ML_REQUIRE(ctx && records, "NULL argument");
    char why[400];
    ML_TRY(pass_checked(wf_check(pass_state(ctx), first_set, n_sets, x2, xi, nx, y2, eta, ny, r2, n_max, ref_mode, ra, rb, ref_c, k,
                                 record_doubles, why, sizeof why), why));
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(fields_unmodulate(ctx));   // as ml_fields_download: the plain near field
    const int nq = n_max + 1, lr = wf_line_record(n_max), mono_doubles = WF_HEAD + 4 * wf_terms(n_max);
    PassPack in;   // the inputs in one upload: x2, xi, ra [nx]; y2, eta, rb [ny]
    const size_t at_x2 = in.add(x2, nx), at_xi = in.add(xi, nx), at_ra = in.add(ra, nx);
    const size_t at_y2 = in.add(y2, ny), at_eta = in.add(eta, ny), at_rb = in.add(rb, ny);
    ML_TRY(ctx->wavefront_in.reserve(in.bytes()));
    ML_TRY(ctx->wavefront_lines.reserve((size_t)wf_scratch_bytes(n_sets, nx, n_max)));
    ML_TRY(ctx->wavefront_records.reserve((size_t)n_sets * mono_doubles * sizeof(double)));
    ML_HIP(hipMemcpyAsync(ctx->wavefront_in.p, in.h.data(), in.bytes(), hipMemcpyHostToDevice, ctx->stream));
    WavefrontArgs a;
    a.fields = ctx->fields.buf.as<double2>() + (size_t)first_set * 4 * nx * ny;
    const double *d_in = ctx->wavefront_in.as<double>();
    a.x2 = d_in + at_x2;
    a.ra = d_in + at_ra;
    a.y2 = d_in + at_y2;
    a.eta = d_in + at_eta;
    a.rb = d_in + at_rb;
    a.lines = ctx->wavefront_lines.as<double>();
    a.nx = nx;
    a.ny = ny;
    a.nq = nq;
    a.lr = lr;
    a.jv = pass_vertex(y2, ny);
    a.focus = ref_mode == PASS_REF_FOCUS;
    a.r2 = r2;
    a.zz = ref_c * ref_c;
    a.sk = ref_c > 0 ? -k : k;
    const int lines = PASS_LINE_THREADS / 64;
    const dim3 grid((nx + lines - 1) / lines);
    if (n_max <= 4)
        wavefront_launch<5>(ctx->stream, grid, a, n_sets);
    else
        wavefront_launch<WF_ORDER_MAX + 1>(ctx->stream, grid, a, n_sets);
    ML_HIP(hipGetLastError());
    double *mono = ctx->wavefront_records.as<double>();
    hipLaunchKernelGGL(wavefront_sum_kernel, dim3(nq + 1, n_sets), dim3(WF_SUM_THREADS), 0, ctx->stream, a.lines, d_in + at_xi, mono, nx, nq, lr);
    ML_HIP(hipGetLastError());
    std::vector<double> got((size_t)n_sets * mono_doubles);
    ML_HIP(hipMemcpyAsync(got.data(), mono, got.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    for (int m = 0; m < n_sets; ++m) wf_convert(got.data() + (size_t)m * mono_doubles, n_max, records + (size_t)m * record_doubles);
    return ML_OK;
}

}  // extern "C"
