// What the kernels and entries of the passes over the resident near field share (fields_zones.hip, fields_wavefront.hip,
// fields_pupil.hip; the host's share: fields_pass.h): the butterfly over a wave, the bisection over the squared edges, the
// four fields of every set of a sample, the reference wave's sincos, the terms of a member, the choice of the kernel for
// 1, 2 or 3 sets, and the entries' first steps.
//
// The device functions hold no guard of their own: the kernel zeroes f in front of its `if (member)` and loads inside it,
// next to its other loads, so that the loads of block b + 1 stay in flight over the arithmetic of block b.  Each kernel keeps
// its own line loop.  Include after nearfield_math.h, under `#pragma clang fp contract(off)`.
#pragma once

#include <type_traits>

#include "fields_pupil.h"

namespace ml {

static_assert(PASS_PHASE_LIMIT == PHASE_LIMIT, "fields_pass.h restates common.h PHASE_LIMIT");

// the sum over the 64 lanes, lanes 32, 16, 8, 4, 2, 1 apart; every lane gets it
__device__ __forceinline__ double pass_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// searchsorted(e2, r2, side = 'left'): the number of edges below r2
__device__ __forceinline__ int pass_find(const double *e2, int K, double r2) {
    int lo = 0, hi = K;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e2[mid] < r2)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Ex, Ey, Hx, Hy of the NS sets of a sample: +0.0, and sample j of the line `row` ([NS][4] planes of `plane` samples)
template <int NS>
__device__ __forceinline__ void pass_zero(double2 (&f)[NS][4]) {
#pragma unroll
    for (int m = 0; m < NS; ++m)
#pragma unroll
        for (int c = 0; c < 4; ++c) f[m][c] = make_double2(0.0, 0.0);
}

template <int NS>
__device__ __forceinline__ void pass_load(double2 (&f)[NS][4], const double2 *row, size_t plane, int j) {
#pragma unroll
    for (int m = 0; m < NS; ++m)
#pragma unroll
        for (int c = 0; c < 4; ++c) f[m][c] = row[(size_t)(4 * m + c) * plane + j];
}

// (sin, cos) of the reference phase of a sample with u = ra[i] + rb[j]; zz = ref_c ref_c, sk = -sign(ref_c) k
__device__ __forceinline__ void pass_ref_sincos(int focus, double sk, double zz, double u, double &sn, double &cs) {
    sincos_cw(focus ? sk * sqrt_exact(u + zz) : u, sn, cs);
}

// The terms of a member (fields_zones.h): S of a set's four fields, |E|^2, and E conj(w)
__device__ __forceinline__ double pass_sz(const double2 (&f)[4]) {
    return 0.5 * ((f[0].x * f[3].x + f[0].y * f[3].y) - (f[1].x * f[2].x + f[1].y * f[2].y));
}

__device__ __forceinline__ double pass_abs2(double2 E) { return E.x * E.x + E.y * E.y; }

__device__ __forceinline__ void pass_overlap(double2 E, double sn, double cs, double &re, double &im) {
    re = E.x * cs + E.y * sn;
    im = E.y * cs - E.x * sn;
}

// ... in the order of a ZoneRun: S, Ix, Iy, Re Cx, Im Cx, Re Cy, Im Cy
__device__ __forceinline__ void pass_terms(const double2 (&f)[4], double sn, double cs, double (&t)[7]) {
    t[0] = pass_sz(f);
    t[1] = pass_abs2(f[0]);
    t[2] = pass_abs2(f[1]);
    pass_overlap(f[0], sn, cs, t[3], t[4]);
    pass_overlap(f[1], sn, cs, t[5], t[6]);
}

// launch(std::integral_constant<int, NS>) for the NS = 1, 2 or 3 sets of a checked call
template <class Launch>
static void pass_for_sets(int ns, Launch &&launch) {
    if (ns == 1)
        launch(std::integral_constant<int, 1>{});
    else if (ns == 2)
        launch(std::integral_constant<int, 2>{});
    else
        launch(std::integral_constant<int, 3>{});
}

// what an entry's check function sees of the context
static inline PassState pass_state(const ml_ctx *ctx) {
    PassState st;
    st.n_ranks = ctx->n_ranks;
    st.nx = ctx->fields.nx;
    st.ny = ctx->fields.ny;
    st.n_sets = ctx->fields.n_sets;
    return st;
}

// the outcome of a check function as the entry's: ML_OK, or the message set and ML_ESTATE (-2) / ML_EINVAL
static inline int pass_checked(int rc, const char *why) {
    if (rc == 0) return ML_OK;
    set_error("%s", why);
    return rc == -2 ? ML_ESTATE : ML_EINVAL;
}

}  // namespace ml
