// Test surface only: one function of nearfield_math.h per lane, on arguments the caller chooses (ml_math_probe;
// tests/test_gpu_device_math.py).  The functions are inlined into every hot kernel and reached there only at the
// arguments a lens happens to produce; here they meet their documented ranges and the neighbours of their worst cases.
// Built with the library's own flags (-ffp-contract=off), so a lane computes what a lane of a hot kernel computes.
// No product code calls this entry.
#include "common.h"
#include "nearfield_math.h"
#include "propagate_otf.h"

namespace ml {

constexpr int PROBE_MAX_N = 1 << 24;

__global__ __launch_bounds__(256) void math_probe_kernel(int op, const double *x, const int *kq, int n, double *out0,
                                                         double *out1, int *outk) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double a = 0.0, b = 0.0;
    int k = 0;
    switch (op) {
    case ML_PROBE_SINCOS: sincos_cw(v, a, b); break;
    case ML_PROBE_SINCOS_Q: sincos_cw_q(v, kq[i], a, b); break;
    case ML_PROBE_REDUCE: reduce_pio2(v, a, k); break;
    case ML_PROBE_SQRT: a = sqrt_exact(v); break;
    case ML_PROBE_RECIP: a = recip(v); break;
    case ML_PROBE_RSQRT: a = rsqrt_fast(v); break;
    case ML_PROBE_RAW_RCP: a = __builtin_amdgcn_rcp(v); break;
    case ML_PROBE_RAW_RSQ: a = __builtin_amdgcn_rsq(v); break;
    case ML_PROBE_OTF_PHASOR: {   // propagate_otf.hip otf_phasor_sincos
        double rest;
        const int q = otf_phase_quarters(otf_phase_fraction(v, (double)kq[i]), rest);
        sincos_cw_q(OTF_TWO_PI * rest, q, a, b);
        break;
    }
    }
    out0[i] = a;
    if (out1) out1[i] = b;
    if (outk) outk[i] = k;
}

}  // namespace ml

using namespace ml;

extern "C" int ml_math_probe(ml_ctx *ctx, int op, const double *x, const int *kq, int n, double *out0, double *out1,
                             int *outk) {
    ML_REQUIRE(ctx && x && out0, "ml_math_probe: NULL argument");
    ML_REQUIRE((op >= ML_PROBE_SINCOS && op <= ML_PROBE_RAW_RSQ) || op == ML_PROBE_OTF_PHASOR,
               "ml_math_probe: unknown op %d (0 ... %d, %d)", op, ML_PROBE_RAW_RSQ, ML_PROBE_OTF_PHASOR);
    ML_REQUIRE(n >= 1 && n <= PROBE_MAX_N, "ml_math_probe: n = %d values, 1 ... 2^24 are taken", n);
    ML_REQUIRE(op != ML_PROBE_SINCOS_Q || kq, "ml_math_probe: op %d (sincos_cw_q) needs the quadrants kq", op);
    ML_REQUIRE(op != ML_PROBE_OTF_PHASOR || kq, "ml_math_probe: op %d (the phasor of ml_propagate_otf) needs the indices kq", op);
    const bool two = op == ML_PROBE_SINCOS || op == ML_PROBE_SINCOS_Q || op == ML_PROBE_OTF_PHASOR;
    ML_REQUIRE(!two || out1, "ml_math_probe: op %d returns sin and cos: out1 is NULL", op);
    ML_REQUIRE(op != ML_PROBE_REDUCE || outk, "ml_math_probe: op %d (reduce_pio2) returns the quadrants: outk is NULL", op);
    ML_HIP(hipSetDevice(ctx->device));
    const size_t nd = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int);
    // [x][out0][out1] doubles, then [kq][outk] ints
    DevBuf buf;
    ML_TRY(buf.reserve(3 * nd + 2 * ni));
    double *dx = buf.as<double>(), *d0 = dx + n, *d1 = dx + 2 * (size_t)n;
    int *dkq = reinterpret_cast<int *>(dx + 3 * (size_t)n), *dk = dkq + n;
    ML_HIP(hipMemcpyAsync(dx, x, nd, hipMemcpyHostToDevice, ctx->stream));
    if (op == ML_PROBE_SINCOS_Q || op == ML_PROBE_OTF_PHASOR) ML_HIP(hipMemcpyAsync(dkq, kq, ni, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, op, dx, dkq, n, d0,
                       two ? d1 : nullptr, op == ML_PROBE_REDUCE ? dk : nullptr);
    ML_HIP(hipGetLastError());
    ML_HIP(hipMemcpyAsync(out0, d0, nd, hipMemcpyDeviceToHost, ctx->stream));
    if (two) ML_HIP(hipMemcpyAsync(out1, d1, nd, hipMemcpyDeviceToHost, ctx->stream));
    if (op == ML_PROBE_REDUCE) ML_HIP(hipMemcpyAsync(outk, dk, ni, hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}
