// The transfer function of a propagated image, contracted where the image lies: per plane of the active propagation
// plan's resident result (or of its sums) and per weight w (I = |E|^2, Sz)
//   O_w[p][a][b] = sum_i sum_j w(p, i, j) exp(-2 pi i (u[a] i + v[b] j))      (ml_propagate_otf)
// - the Fourier transform of the point-spread function at nu x nv chosen frequencies, of which the modulation transfer
// function is the modulus.  The phase arithmetic, the order of the sums, the checks and the caps: propagate_otf.h.
// The reference has no counterpart.
//
// Per target the weights are those of propagate_accumulate_kernel and focus_chunk_kernel, operation by operation:
//   I = ((Ex.r^2 + Ex.i^2) + (Ey.r^2 + Ey.i^2)) + (Ez.r^2 + Ez.i^2),   Sz = 0.5 ((Ex.r Hy.r + Ex.i Hy.i) - (Ey.r Hx.r + Ey.i Hx.i))
// (nothing is contracted: -ffp-contract=off).  From the sums the stored doubles are taken as they are.
//
// Three launches, no atomics.
//   Tables.  Tx[mx][nu], Ty[my][nv] = (cos, -sin) of 2 pi frac(u i): a lane per entry, otf_phase_fraction, the quarter
//            turns taken off exactly, sincos_cw_q of the rest.
//   Rows.    A workgroup of 256 lanes takes one row i of one plane (grid: mx x planes) in tiles of 1024 targets - four
//            rows in tiles of 256 where nv > 8, which shares every phasor it loads among them and changes no sum.  The
//            lanes form the tile's weights once - 96 bytes read per target with H, 48 without, 8 or 16 from the sums, in
//            8-byte loads of the sums, so a plane on an odd index reads as any other - and leave them in the LDS, where
//            they serve all nv frequencies; a weight map never reaches memory.  Then a lane takes a (segment, frequency)
//            pair: the 32 terms of the segment one after another, both weights beside each other.  The segments' sums of
//            16 (four rows: 32) frequencies at a time wait in the LDS for the one lane per (frequency, weight, component) that adds them
//            in their order to its running sum.  R[w][p][i][b], mx nv complex per plane and weight, goes to memory: under
//            1 % of the image's own bytes.
//   Columns. A workgroup per (a, weight, plane): the same two levels over the rows, complex times complex, every product
//            and sum rounded on its own.
// The segments of a row lie 33 doubles apart in the LDS: lanes that walk different segments in step (few frequencies)
// read different banks, lanes that share a segment (many frequencies) read one address.
#include "common.h"
#include "nearfield_math.h"
#include "propagate_otf.h"

#pragma clang fp contract(off)

namespace ml {

constexpr int OTF_THREADS = 256;
// (OTF_TILE, OTF_BATCH, OTF_FEW, OTF_ROWS_MANY and the tiles they give: propagate_otf.h)
constexpr int OTF_TILE_SEGS = OTF_TILE / OTF_SEGMENT;       // 32
constexpr int OTF_SEG_PITCH = OTF_SEGMENT + 1;              // doubles between two segments' weights in the LDS
static_assert(OTF_FREQ_MAX * 4 <= OTF_THREADS, "a lane per (frequency, weight, component) keeps a running sum");
static_assert(OTF_TILE % OTF_THREADS == 0 && OTF_TILE % OTF_SEGMENT == 0, "whole steps and whole segments per tile");

struct OtfFreqs {
    double u[OTF_FREQ_MAX], v[OTF_FREQ_MAX];
};

// sin and cos of 2 pi frac(f index), index >= 0 (propagate_otf.h; math_probe.hip restates these three lines)
__device__ __forceinline__ void otf_phasor_sincos(double f, int index, double &s, double &c) {
    double rest;
    const int q = otf_phase_quarters(otf_phase_fraction(f, (double)index), rest);
    sincos_cw_q(OTF_TWO_PI * rest, q, s, c);
}

__global__ __launch_bounds__(OTF_THREADS) void otf_table_kernel(const OtfFreqs f, int mx, int nu, int my, int nv, double2 *tx,
                                                                double2 *ty) {
    const int e = blockIdx.x * OTF_THREADS + threadIdx.x;   // (mx nu + my nv <= 2^24)
    const int nx = mx * nu;
    if (e >= nx + my * nv) return;
    double s, c;
    if (e < nx) {
        const int i = e / nu, a = e - i * nu;
        otf_phasor_sincos(f.u[a], i, s, c);
        tx[e] = make_double2(c, -s);
    } else {
        const int g = e - nx, j = g / nv, b = g - j * nv;
        otf_phasor_sincos(f.v[b], j, s, c);
        ty[g] = make_double2(c, -s);
    }
}

struct OtfRowArgs {
    const double2 *result;   // [6 or 3][T] of the member (fields), or
    const double *sums;      // [2][T]
    const double2 *ty;       // [my][nv]
    double2 *rows;           // [2][planes][mx][nv]
    int T, mx, my, nv, planes;
};

// ROWS rows of a plane per workgroup, in tiles of 1024 / ROWS targets of each: 1 where few frequencies leave the pass to
// the stream of the image, 4 where many make it the stream of Ty - every row read Ty[my][nv] from the L2 on its own, 16 GB
// for 4096^2 targets at nv = 64; four rows share each phasor a lane loads.  How the work is dealt out does not touch the
// order of a sum: the segments are the same 32 indices, added from 0, and the segments' sums are added in ascending order.
template <bool FIELDS, bool WANT_H, int ROWS>
__global__ __launch_bounds__(OTF_THREADS) void otf_rows_kernel(const OtfRowArgs a) {
    constexpr int TILE = OTF_TILE / ROWS, TILE_SEGS = TILE / OTF_SEGMENT, BATCH = ROWS == 1 ? OTF_BATCH : 2 * OTF_BATCH;
    static_assert(TILE % OTF_SEGMENT == 0 && OTF_FREQ_MAX % BATCH == 0, "whole segments per tile, whole batches per call");
    __shared__ double s_w[2][ROWS][TILE_SEGS * OTF_SEG_PITCH];
    __shared__ double s_part[TILE_SEGS][BATCH][ROWS][4];   // (re, im) with I, (re, im) with Sz
    __shared__ double s_run[ROWS][OTF_FREQ_MAX][4];
    const int tid = threadIdx.x, i0 = blockIdx.x * ROWS, plane = blockIdx.y;
    const int rows = otf_live_rows(a.mx, ROWS, blockIdx.x);
    const size_t row0 = ((size_t)plane * a.mx + i0) * a.my;   // the first row's first target
    const size_t T = (size_t)a.T;
    for (int e = tid; e < ROWS * OTF_FREQ_MAX * 4; e += OTF_THREADS) (&s_run[0][0][0])[e] = 0.0;
    const int tiles = otf_tiles(a.my, TILE);
    for (int tile = 0; tile < tiles; ++tile) {
        const int t0 = tile * TILE, n = otf_tile_len(a.my, TILE, tile), segs = otf_segments(n);
        // the weights of the tile, once per target (a row behind the plane's last: zeros, never written out)
#pragma unroll
        for (int k = 0; k < OTF_TILE / OTF_THREADS; ++k) {
            const int e = tid + k * OTF_THREADS, r = e / TILE, l = e - r * TILE;
            if (l >= n) continue;
            double I = 0.0, S = 0.0;
            if (r < rows) {
                const size_t t = row0 + (size_t)r * a.my + t0 + l;
                if (FIELDS) {
                    const double2 *f = a.result + t;
                    const double2 Ex = f[0], Ey = f[T], Ez = f[2 * T];
                    I = ((Ex.x * Ex.x + Ex.y * Ex.y) + (Ey.x * Ey.x + Ey.y * Ey.y)) + (Ez.x * Ez.x + Ez.y * Ez.y);
                    if (WANT_H) {
                        const double2 Hx = f[3 * T], Hy = f[4 * T];
                        S = 0.5 * ((Ex.x * Hy.x + Ex.y * Hy.y) - (Ey.x * Hx.x + Ey.y * Hx.y));
                    }
                } else {
                    I = a.sums[t];
                    if (WANT_H) S = a.sums[T + t];
                }
            }
            const int at = (l / OTF_SEGMENT) * OTF_SEG_PITCH + (l % OTF_SEGMENT);
            s_w[0][r][at] = I;
            if (WANT_H) s_w[1][r][at] = S;
        }
        __syncthreads();
        for (int b0 = 0; b0 < a.nv; b0 += BATCH) {
            const int nb = min(BATCH, a.nv - b0);
            for (int item = tid; item < segs * nb; item += OTF_THREADS) {
                const int s = item / nb, bb = item - s * nb;
                const int cnt = min(OTF_SEGMENT, n - s * OTF_SEGMENT);
                const double2 *ty = a.ty + (size_t)(t0 + s * OTF_SEGMENT) * a.nv + b0 + bb;
                double acc[ROWS][4];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.0;
#pragma unroll 4
                for (int k = 0; k < cnt; ++k) {   // (unrolled: the loads of four terms fly together; the adds keep their order)
                    const double2 t = ty[(size_t)k * a.nv];
#pragma unroll
                    for (int r = 0; r < ROWS; ++r) {
                        const double w = s_w[0][r][s * OTF_SEG_PITCH + k];
                        acc[r][0] += w * t.x;
                        acc[r][1] += w * t.y;
                        if (WANT_H) {
                            const double h = s_w[1][r][s * OTF_SEG_PITCH + k];
                            acc[r][2] += h * t.x;
                            acc[r][3] += h * t.y;
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
#pragma unroll
                    for (int q = 0; q < 4; ++q) s_part[s][bb][r][q] = acc[r][q];
            }
            __syncthreads();
            for (int o = tid; o < ROWS * nb * 4; o += OTF_THREADS) {   // the segments' sums in their order
                const int r = o / (nb * 4), rem = o - r * nb * 4, bb = rem >> 2, q = rem & 3;
                if (!WANT_H && (q & 2)) continue;
                double run = s_run[r][b0 + bb][q];
                for (int s = 0; s < segs; ++s) run += s_part[s][bb][r][q];
                s_run[r][b0 + bb][q] = run;
            }
            __syncthreads();   // s_part is free again, and behind the last batch s_w too
        }
    }
    __syncthreads();   // (a plane without targets along y cannot be planned; the zeros of s_run for good measure)
    for (int o = tid; o < rows * a.nv * 4; o += OTF_THREADS) {
        const int r = o / (a.nv * 4), rem = o - r * a.nv * 4, b = rem >> 2, q = rem & 3, w = q >> 1;
        if (WANT_H || w == 0) {
            double *out = reinterpret_cast<double *>(a.rows + (((size_t)w * a.planes + plane) * a.mx + i0 + r) * a.nv + b);
            out[q & 1] = s_run[r][b][q];
        }
    }
}

template <bool FIELDS, bool WANT_H>
static void otf_rows_launch(hipStream_t stream, const OtfRowArgs &a) {
    const int rows = otf_rows_per_group(a.nv);
    const dim3 grid(otf_tiles(a.mx, rows), a.planes);
    if (rows == 1)
        hipLaunchKernelGGL((otf_rows_kernel<FIELDS, WANT_H, 1>), grid, dim3(OTF_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL((otf_rows_kernel<FIELDS, WANT_H, OTF_ROWS_MANY>), grid, dim3(OTF_THREADS), 0, stream, a);
}

// O_w[p][a][b] = sum_i Tx(i, a) R_w(p, i, b): a workgroup per (a, w, p), tiles of 1024 rows, a lane per (segment, b), then a
// lane per (b, component) that adds the segments' sums in their order to its running sum (a register: every tile has the
// same lane)
__global__ __launch_bounds__(OTF_THREADS) void otf_columns_kernel(const double2 *tx, const double2 *rows, double2 *otf, int mx, int nu,
                                                                  int nv, int planes) {
    __shared__ double s_part[OTF_TILE_SEGS][OTF_FREQ_MAX][2];
    const int tid = threadIdx.x, a = blockIdx.x, w = blockIdx.y, plane = blockIdx.z;
    const double2 *R = rows + ((size_t)w * planes + plane) * mx * nv;
    double run = 0.0;
    const int tiles = otf_tiles(mx, OTF_TILE);
    for (int tile = 0; tile < tiles; ++tile) {
        const int t0 = tile * OTF_TILE, n = otf_tile_len(mx, OTF_TILE, tile), segs = otf_segments(n);
        for (int item = tid; item < segs * nv; item += OTF_THREADS) {
            const int s = item / nv, b = item - s * nv;
            const int i0 = t0 + s * OTF_SEGMENT, cnt = min(OTF_SEGMENT, n - s * OTF_SEGMENT);
            double re = 0.0, im = 0.0;
            for (int k = 0; k < cnt; ++k) {
                const double2 t = tx[(size_t)(i0 + k) * nu + a];
                const double2 r = R[(size_t)(i0 + k) * nv + b];
                re += t.x * r.x - t.y * r.y;
                im += t.x * r.y + t.y * r.x;
            }
            s_part[s][b][0] = re;
            s_part[s][b][1] = im;
        }
        __syncthreads();
        if (tid < nv * 2)
            for (int s = 0; s < segs; ++s) run += s_part[s][tid >> 1][tid & 1];
        __syncthreads();
    }
    if (tid < nv * 2)
        reinterpret_cast<double *>(otf + (((size_t)plane * 2 + w) * nu + a) * nv + (tid >> 1))[tid & 1] = run;
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_propagate_otf(ml_ctx *ctx, int source, int mx, int my, int planes, const double *u, int nu, const double *v, int nv,
                     double *otf) {
    ML_REQUIRE(ctx, "NULL argument");
    ML_REQUIRE(ctx->n_ranks <= 1, "ml_propagate_otf: this context belongs to a communicator of %d ranks", ctx->n_ranks);
    PropagatePlan &pp = ctx->prop;
    FocusState st;
    st.have_result = pp.ready && pp.have_result;
    st.have_sums = pp.have_sums;
    st.T = pp.T;
    st.result_sets = pp.result_sets;
    char why[320];
    const int rc = otf_check(st, source, mx, my, planes, u, nu, v, nv, otf, why, sizeof why);
    if (rc != 0) {
        set_error("%s", why);
        return rc == -2 ? ML_ESTATE : ML_EINVAL;
    }
    ML_HIP(hipSetDevice(ctx->device));
    const size_t n_table = (size_t)mx * nu + (size_t)my * nv, n_rows = (size_t)planes * mx * nv;
    const size_t n_out = (size_t)planes * 2 * nu * nv;
    const int nw = pp.want_h ? 2 : 1;
    ML_TRY(pp.otf_tables.reserve(n_table * sizeof(double2)));
    ML_TRY(pp.otf_rows.reserve(2 * n_rows * sizeof(double2)));
    ML_TRY(pp.otf_out.reserve(n_out * sizeof(double2)));
    double2 *tx = pp.otf_tables.as<double2>(), *ty = tx + (size_t)mx * nu;
    OtfFreqs f;
    for (int a = 0; a < OTF_FREQ_MAX; ++a) {
        f.u[a] = a < nu ? u[a] : 0.0;
        f.v[a] = a < nv ? v[a] : 0.0;
    }
    hipLaunchKernelGGL(otf_table_kernel, dim3((unsigned)((n_table + OTF_THREADS - 1) / OTF_THREADS)), dim3(OTF_THREADS), 0, ctx->stream, f,
                       mx, nu, my, nv, tx, ty);
    ML_HIP(hipGetLastError());
    OtfRowArgs a;
    const bool fields = source >= 0;
    a.result = fields ? pp.result.as<double2>() + (size_t)source * (pp.want_h ? 6 : 3) * pp.T : nullptr;
    a.sums = fields ? nullptr : pp.sums.as<double>();
    a.ty = ty;
    a.rows = pp.otf_rows.as<double2>();
    a.T = pp.T;
    a.mx = mx;
    a.my = my;
    a.nv = nv;
    a.planes = planes;
    const dim3 block(OTF_THREADS);
    if (fields && pp.want_h)
        otf_rows_launch<true, true>(ctx->stream, a);
    else if (fields)
        otf_rows_launch<true, false>(ctx->stream, a);
    else if (pp.want_h)
        otf_rows_launch<false, true>(ctx->stream, a);
    else
        otf_rows_launch<false, false>(ctx->stream, a);
    ML_HIP(hipGetLastError());
    double2 *out = pp.otf_out.as<double2>();
    if (nw == 1) ML_HIP(hipMemsetAsync(out, 0, n_out * sizeof(double2), ctx->stream));   // the Sz blocks: zeros
    hipLaunchKernelGGL(otf_columns_kernel, dim3(nu, nw, planes), block, 0, ctx->stream, tx, a.rows, out, mx, nu, nv, planes);
    ML_HIP(hipGetLastError());
    ML_HIP(hipMemcpyAsync(otf, out, n_out * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

}  // extern "C"
