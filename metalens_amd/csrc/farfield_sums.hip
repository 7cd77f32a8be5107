// Sums over the sources of a sweep, kept on the GPU: of the active plan's power map
// (farfield_project.hip) P_sum (+)= weight * P (NaN outside the unit circle stays NaN), and per source slot the
// reference's total_P = sum of the finite P * dux * duy (nearfield_farfield.py:74) plus the same restricted to the cone
// sqrt(ux^2 + uy^2) <= cone_u.  Two-level fixed-order sums (accumulate_kernel: 256 directions per block to a pair of
// partials; accumulate_finish_kernel: the partials to the slot): deterministic.  The sums live in the context (common.h
// ml_ctx acc_P, acc_partials, acc_sums), not in the plan; what the power map must be like to be summed, and its cell
// dux duy, are stated in farfield_beam.h, which the beam metrics (farfield_beam.hip) share.
// Entries: ml_farfield_accumulate, ml_farfield_total_power, ml_farfield_sums.
#include "common.h"
#include "farfield_beam.h"

using namespace ml;

extern "C" {

struct AccArgs {
    const double *P, *ux, *uy;
    double *P_sum, *partials;   // partials[block][2]
    int mx, my, pair_list, reset;
    double weight, cell, cone_u2, cone_ux0, cone_uy0;
};

__global__ __launch_bounds__(256) void accumulate_kernel(const AccArgs a) {
    __shared__ double s_tot[256], s_cone[256];
    const size_t n = (size_t)a.mx * (a.pair_list ? 1 : a.my);
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    double tot = 0.0, cone = 0.0;
    if (at < n) {
        const double P = a.P[at];
        if (a.P_sum) a.P_sum[at] = a.reset ? a.weight * P : a.P_sum[at] + a.weight * P;
        if (isfinite(P)) {
            const int i = a.pair_list ? (int)at : (int)(at / a.my), j = a.pair_list ? (int)at : (int)(at % a.my);
            const double ux = a.ux[i] - a.cone_ux0, uy = a.uy[j] - a.cone_uy0;
            tot = P * a.cell;
            if (ux * ux + uy * uy <= a.cone_u2) cone = tot;
        }
    }
    s_tot[threadIdx.x] = tot;
    s_cone[threadIdx.x] = cone;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_tot[threadIdx.x] += s_tot[threadIdx.x + w];
            s_cone[threadIdx.x] += s_cone[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.partials[2 * blockIdx.x] = s_tot[0];
        a.partials[2 * blockIdx.x + 1] = s_cone[0];
    }
}

// sums[2 * slot + {0, 1}] = fixed-order sum of the block partials
__global__ __launch_bounds__(256) void accumulate_finish_kernel(const double *partials, int n_blocks,
                                                                double *sums) {
    __shared__ double s[256];
    for (int k = 0; k < 2; ++k) {
        double v = 0.0;
        for (int b = threadIdx.x; b < n_blocks; b += 256) v += partials[2 * b + k];
        __syncthreads();
        s[threadIdx.x] = v;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[k] = s[0];
    }
}

// slot ML_MAX_SWEEP_SLOTS is private to ml_farfield_total_power: a one-off total never lands in a
// slot (or the P_sum) that a sweep on the same context is filling
static int accumulate_impl(ml_ctx *ctx, double weight, double cone_u, double cone_ux0, double cone_uy0,
                           int slot, int reset, bool into_sum) {
    FarfieldPlan &pl = ctx->plan;
    char why[320];
    if (beam_check_map(beam_state(ctx), why, sizeof why) != 0) {
        set_error("%s", why);
        return ML_ESTATE;
    }
    const size_t n = pl.directions();
    if (into_sum && !reset) {
        // P_sum is sized by the plan it was started on: adding onto it needs that plan's directions
        if (!ctx->acc_n) {
            set_error("ml_farfield_accumulate: this context has no sums yet (the first call needs reset = 1)");
            return ML_ESTATE;
        }
        if (ctx->acc_n != n || ctx->acc_pair_list != pl.pair_list) {
            set_error("ml_farfield_accumulate: the sums were started on a plan of %zu directions (%s), the active plan "
                      "has %zu (%s): start a new sum with reset = 1", ctx->acc_n,
                      ctx->acc_pair_list ? "pair list" : "tensor grid", n, pl.pair_list ? "pair list" : "tensor grid");
            return ML_ESTATE;
        }
    }
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(comm_join(ctx, false));
    const int blocks = (int)((n + 255) / 256);
    if (into_sum) {
        ctx->acc_n = 0;   // (a reserve that fails has let go of the old sum)
        ML_TRY(ctx->acc_P.reserve(n * sizeof(double)));
        ctx->acc_n = n;
        ctx->acc_pair_list = pl.pair_list;
    }
    ML_TRY(ctx->acc_partials.reserve((size_t)blocks * 2 * sizeof(double)));
    if (!ctx->acc_sums.p) {
        const size_t bytes = (size_t)(ML_MAX_SWEEP_SLOTS + 1) * 2 * sizeof(double);
        ML_TRY(ctx->acc_sums.reserve(bytes));
        ML_HIP(hipMemsetAsync(ctx->acc_sums.p, 0, bytes, ctx->stream));
    }
    AccArgs a;
    a.P = pl.power.as<double>();
    a.ux = pl.ux.as<double>();
    a.uy = pl.uy.as<double>();
    a.P_sum = into_sum ? ctx->acc_P.as<double>() : nullptr;
    a.partials = ctx->acc_partials.as<double>();
    a.mx = pl.mx;
    a.my = pl.my;
    a.pair_list = pl.pair_list;
    a.reset = reset;
    a.weight = weight;
    // dux * duy as the reference takes them (nearfield_farfield.py:71-74): farfield_beam.h beam_cell
    a.cell = beam_cell(pl.h_ux.data(), pl.mx, pl.h_uy.data(), pl.my, pl.pair_list != 0);
    a.cone_u2 = cone_u * cone_u;
    a.cone_ux0 = cone_ux0;
    a.cone_uy0 = cone_uy0;
    hipLaunchKernelGGL(accumulate_kernel, dim3(blocks), dim3(256), 0, ctx->stream, a);
    ML_HIP(hipGetLastError());
    hipLaunchKernelGGL(accumulate_finish_kernel, dim3(1), dim3(256), 0, ctx->stream,
                       ctx->acc_partials.as<double>(), blocks, ctx->acc_sums.as<double>() + 2 * slot);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

int ml_farfield_accumulate(ml_ctx *ctx, double weight, double cone_u, double cone_ux0, double cone_uy0,
                           int slot, int reset) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(slot >= 0 && slot < ML_MAX_SWEEP_SLOTS, "slot %d out of range [0, %d)", slot,
               ML_MAX_SWEEP_SLOTS);
    return accumulate_impl(ctx, weight, cone_u, cone_ux0, cone_uy0, slot, reset, true);
}

int ml_farfield_total_power(ml_ctx *ctx, double *total_P) {
    ML_REQUIRE(ctx && total_P, "NULL argument");
    ML_TRY(accumulate_impl(ctx, 1.0, 0.0, 0.0, 0.0, ML_MAX_SWEEP_SLOTS, 0, false));
    ML_HIP(hipMemcpyAsync(total_P, ctx->acc_sums.as<double>() + 2 * ML_MAX_SWEEP_SLOTS, sizeof(double),
                          hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

int ml_farfield_sums(ml_ctx *ctx, double *P_sum, double *total_P, double *cone_P, int n_slots) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(n_slots >= 0 && n_slots <= ML_MAX_SWEEP_SLOTS, "n_slots %d out of range", n_slots);
    ML_REQUIRE(ctx->acc_P.p && ctx->acc_sums.p, "ml_farfield_accumulate has not run");
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(comm_join(ctx, false));
    FarfieldPlan &pl = ctx->plan;
    const size_t n = pl.directions();
    if (P_sum && (!pl.ready || ctx->acc_n != n || ctx->acc_pair_list != pl.pair_list)) {
        // P_sum has the size of the plan it was accumulated on; the slot scalars do not depend on it (P_sum = NULL)
        set_error("ml_farfield_sums: P_sum was accumulated on a plan of %zu directions (%s), the active plan has %zu "
                  "(%s)", ctx->acc_n, ctx->acc_pair_list ? "pair list" : "tensor grid", pl.ready ? n : (size_t)0,
                  pl.pair_list ? "pair list" : "tensor grid");
        return ML_ESTATE;
    }
    std::vector<double> sums((size_t)2 * std::max(n_slots, 1));
    if (P_sum)
        ML_HIP(hipMemcpyAsync(P_sum, ctx->acc_P.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (n_slots)
        ML_HIP(hipMemcpyAsync(sums.data(), ctx->acc_sums.p, (size_t)2 * n_slots * sizeof(double),
                              hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n_slots; ++k) {
        if (total_P) total_P[k] = sums[2 * k];
        if (cone_P) cone_P[k] = sums[2 * k + 1];
    }
    return ML_OK;
}

}  // extern "C"
