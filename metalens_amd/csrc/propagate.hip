// Propagation of the resident near field to points at finite distance behind the aperture: the
// Stratton-Chu / Franz fields of the tangential equivalent currents, as a direct pair sum over
// (aperture samples inside the lens) x (targets), fp64.  The reference has no such propagator (SURVEY.md
// D2); the currents, the medium and the time convention are those of its far field
// (nearfield_farfield.py:94-101, 183-185): J = (-Hy, Hx), M = (Ey, -Ex), k = 2 pi n_glass / wavelength,
// Z = Z0 / n_glass, e^{-i omega t}.
//
// With R = r - r', q = 1 / (k R), w = e^{i k R} / (k R), a = 1 + i q - q^2, b = 1 + 3 i q - 3 q^2, m = M / Z and
// D(V) = a V - b Rhat (Rhat . V):
//   E(r) = Z k^2 / (4 pi) dx' dy' sum w { i D(J) - (i - q) Rhat x m }
//   H(r) =   k^2 / (4 pi) dx' dy' sum w { i D(m) + (i - q) Rhat x J }
// (g = e^{ikR} / (4 pi R) = k w / (4 pi) and c = i k - 1 / R = k (i - q) taken out of the braces.)
//
// Shape.  A lane is a target, a workgroup 256 of them.  The samples of an aperture row are uniform across
// the workgroup: tiles of PROP_TILE samples are staged through the LDS as the four current components
// (64 bytes per sample) and read back by broadcast.  The aperture's rows are dealt round robin to `splits`
// workgroups per target tile - few targets still fill the chip, and every workgroup crosses the lens
// alike - each of which leaves a partial sum; a second pass adds the partials in their order.  No atomics:
// the result is bit-for-bit repeatable, and `splits` depends on the sizes alone.
// A synthesised field carries row extents (nearfield.hip row_extent_kernel): samples outside them are
// exact zeros and are not visited.  The extents are read from the device's own array.  A skipped sample
// would have added +-0 to every accumulator, so the result has the bits of the whole sum.
// The phase k R (1.6e4 rad at 1 mm, 1e7 at 1 m) is the accuracy: R by a correctly rounded square root,
// sin / cos by the three-constant Cody-Waite reduction (nearfield_math.h, |k R| < 1e9).
#include "nearfield_math.h"

namespace ml {

constexpr int PROP_THREADS = 256;   // targets per workgroup
constexpr int PROP_TILE = 128;      // aperture samples per LDS tile (8 KiB)
constexpr int PROP_BLOCKS = 2048;   // workgroups aimed at: eight per compute unit

struct PropArgs {
    const double2 *fields;   // [4][nx][ny]: Ex, Ey, Hx, Hy of the selected field set
    const int *row_first;    // [nx] (row_extent_kernel) or nullptr: every sample is read
    const double *tx, *ty, *tz;   // [T]: x - x0, y - y0, z
    double *partial;         // [splits][12 or 6][T]
    int nx, ny, T, splits;
    double dxp, dyp, k, inv_k, Z;
};

// acc += w t
__device__ __forceinline__ void cfma(c2 &acc, c2 w, double tr, double ti) {
    acc.r = fma(-w.i, ti, fma(w.r, tr, acc.r));
    acc.i = fma(w.i, tr, fma(w.r, ti, acc.i));
}

// acc[0..3) += w { i D(V) + sgn (i - q) Rhat x U },  D(V) = a V - b Rhat (Rhat . V);  V, U tangential
template <int SGN>
__device__ __forceinline__ void pair_term(c2 acc[3], c2 w, double q, c2 a, c2 b, double ux, double uy, double uz, c2 Vx,
                                          c2 Vy, c2 Ux, c2 Uy) {
    const c2 dot = {fma(ux, Vx.r, uy * Vy.r), fma(ux, Vx.i, uy * Vy.i)};
    const c2 bd = cmulf(b, dot);
    const c2 Dx = {fma(-ux, bd.r, fma(a.r, Vx.r, -(a.i * Vx.i))), fma(-ux, bd.i, fma(a.r, Vx.i, a.i * Vx.r))};
    const c2 Dy = {fma(-uy, bd.r, fma(a.r, Vy.r, -(a.i * Vy.i))), fma(-uy, bd.i, fma(a.r, Vy.i, a.i * Vy.r))};
    const c2 Dz = {-uz * bd.r, -uz * bd.i};
    const c2 Xx = {-uz * Uy.r, -uz * Uy.i};
    const c2 Xy = {uz * Ux.r, uz * Ux.i};
    const c2 Xz = {fma(ux, Uy.r, -(uy * Ux.r)), fma(ux, Uy.i, -(uy * Ux.i))};
    // i D = (-D.i, D.r);  (i - q) X = (-q X.r - X.i, X.r - q X.i)
    const double s = (double)SGN;
    cfma(acc[0], w, fma(s, fma(-q, Xx.r, -Xx.i), -Dx.i), fma(s, fma(-q, Xx.i, Xx.r), Dx.r));
    cfma(acc[1], w, fma(s, fma(-q, Xy.r, -Xy.i), -Dy.i), fma(s, fma(-q, Xy.i, Xy.r), Dy.r));
    cfma(acc[2], w, fma(s, fma(-q, Xz.r, -Xz.i), -Dz.i), fma(s, fma(-q, Xz.i, Xz.r), Dz.r));
}

template <bool WANT_H>
__global__ __launch_bounds__(PROP_THREADS) void propagate_kernel(const PropArgs a) {
    __shared__ double2 s_cur[PROP_TILE][4];   // Jx, Jy, Mx / Z, My / Z
    const int tid = threadIdx.x;
    const int t = blockIdx.x * PROP_THREADS + tid;
    const int tc = min(t, a.T - 1);   // (lanes past the last target work on a copy of it and store nothing)
    const double tx = a.tx[tc], ty = a.ty[tc], z = a.tz[tc];
    const double zz = z * z;
    const bool wave_live = blockIdx.x * PROP_THREADS + (tid & ~63) < a.T;
    // staging: this thread converts field f of the columns c and c + 64 of a tile into current 3 - f:
    // Ex -> My / Z = -Ex / Z, Ey -> Mx / Z, Hx -> Jy, Hy -> Jx = -Hy  (a division: exact for Z = 1, and x 2 commutes)
    const int f = tid >> 6, c = tid & 63;
    const double sg = (f == 0 || f == 3) ? -1.0 : 1.0, den = f < 2 ? a.Z : 1.0;
    c2 E[3] = {{0, 0}, {0, 0}, {0, 0}}, H[3] = {{0, 0}, {0, 0}, {0, 0}};
    for (int i = blockIdx.y; i < a.nx; i += a.splits) {
        const int first = a.row_first ? a.row_first[i] : 0;   // (0x7f7f7f7f: no sample of the row is inside)
        const int j_hi = a.ny - first;
        if (first >= j_hi) continue;
        const double dx = fma(-(double)i, a.dxp, tx);
        const double s_row = fma(dx, dx, zz);
        const double2 *row = a.fields + ((size_t)f * a.nx + i) * a.ny;
        for (int j0 = first; j0 < j_hi; j0 += PROP_TILE) {
            const int n = min(PROP_TILE, j_hi - j0);
            __syncthreads();   // the previous tile has been read
            for (int cc = c; cc < n; cc += 64) {
                const double2 v = row[j0 + cc];
                s_cur[cc][3 - f] = make_double2(sg * v.x / den, sg * v.y / den);
            }
            __syncthreads();
            if (!wave_live) continue;
            for (int s = 0; s < n; ++s) {
                const double2 v0 = s_cur[s][0], v1 = s_cur[s][1], v2 = s_cur[s][2], v3 = s_cur[s][3];
                const c2 Jx = {v0.x, v0.y}, Jy = {v1.x, v1.y}, Mx = {v2.x, v2.y}, My = {v3.x, v3.y};
                const double dy = fma(-(double)(j0 + s), a.dyp, ty);
                const double R = sqrt_exact(fma(dy, dy, s_row));
                const double iR = recip(R);
                const double ux = dx * iR, uy = dy * iR, uz = z * iR;
                const double q = iR * a.inv_k, q2 = q * q;
                double sn, cs;
                sincos_cw(a.k * R, sn, cs);
                const c2 w = {cs * q, sn * q};
                const c2 ca = {1.0 - q2, q}, cb = {fma(-3.0, q2, 1.0), 3.0 * q};
                pair_term<-1>(E, w, q, ca, cb, ux, uy, uz, Jx, Jy, Mx, My);
                if (WANT_H) pair_term<1>(H, w, q, ca, cb, ux, uy, uz, Mx, My, Jx, Jy);
            }
        }
    }
    if (t >= a.T) return;
    constexpr int NQ = WANT_H ? 12 : 6;
    double *out = a.partial + (size_t)blockIdx.y * NQ * a.T + t;
    for (int m = 0; m < 3; ++m) {
        out[(size_t)(2 * m) * a.T] = E[m].r;
        out[(size_t)(2 * m + 1) * a.T] = E[m].i;
        if (WANT_H) {
            out[(size_t)(6 + 2 * m) * a.T] = H[m].r;
            out[(size_t)(7 + 2 * m) * a.T] = H[m].i;
        }
    }
}

// second pass: result[component][target] = scale * (partial 0 + partial 1 + ...), in that order
__global__ __launch_bounds__(256) void propagate_reduce_kernel(const double *partial, double2 *result, int T, int splits,
                                                               int nq, double scale_e, double scale_h) {
    const int t = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;   // m: complex component, 0-2 E, 3-5 H
    if (t >= T) return;
    double re = 0.0, im = 0.0;
    for (int s = 0; s < splits; ++s) {
        const double *p = partial + ((size_t)s * nq + 2 * m) * T + t;
        re += p[0];
        im += p[T];
    }
    const double scale = m < 3 ? scale_e : scale_h;
    result[(size_t)m * T + t] = make_double2(scale * re, scale * im);
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_propagate_plan(ml_ctx *ctx, double x0, double y0, double dxp, double dyp, double wavelength, double n_glass,
                      const double *x, int nx_t, const double *y, int ny_t, const double *z, int nz, int point_list,
                      int want_h) {
    ML_REQUIRE(ctx && x && y && z, "NULL argument");
    ML_REQUIRE(ctx->n_ranks <= 1, "ml_propagate_plan: this context belongs to a communicator of %d ranks; the "
               "finite-distance propagator sums a whole aperture on one GPU (sharded propagation is not implemented)",
               ctx->n_ranks);
    ML_REQUIRE(nx_t >= 1 && ny_t >= 1 && nz >= 1, "no targets");
    if (point_list)
        ML_REQUIRE(ny_t == nx_t && nz == nx_t, "a point list needs len(x) == len(y) == len(z) (%d, %d, %d)", nx_t, ny_t, nz);
    else
        ML_REQUIRE(nz == 1, "a tensor grid of targets lies in one plane: one z, got %d", nz);
    ML_REQUIRE(wavelength > 0 && n_glass > 0 && dxp > 0 && dyp > 0, "bad geometry");
    const long long T = point_list ? nx_t : (long long)nx_t * ny_t;
    ML_REQUIRE(T <= (1 << 26), "%lld targets: at most 2^26 per plan", T);
    for (int d = 0; d < nz; ++d) ML_REQUIRE(z[d] > 0, "target %d lies at z = %g: the propagator needs z > 0", d, z[d]);
    ML_HIP(hipSetDevice(ctx->device));
    PropagatePlan &pp = ctx->prop;
    pp.ready = pp.have_result = false;
    std::vector<double> h((size_t)3 * T);
    for (long long t = 0; t < T; ++t) {
        const int ix = point_list ? (int)t : (int)(t / ny_t), iy = point_list ? (int)t : (int)(t % ny_t);
        h[t] = x[ix] - x0;
        h[T + t] = y[iy] - y0;
        h[2 * T + t] = z[point_list ? (int)t : 0];
    }
    ML_TRY(pp.targets.reserve(h.size() * sizeof(double)));
    ML_HIP(hipMemcpyAsync(pp.targets.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));   // (`h` goes away)
    pp.T = (int)T;
    pp.want_h = want_h != 0;
    pp.x0 = x0;
    pp.y0 = y0;
    pp.dxp = dxp;
    pp.dyp = dyp;
    pp.wavelength = wavelength;
    pp.n_glass = n_glass;
    pp.ready = true;
    return ML_OK;
}

int ml_propagate(ml_ctx *ctx, double Z0) {
    ML_REQUIRE(ctx, "ctx is NULL");
    PropagatePlan &pp = ctx->prop;
    if (!pp.ready) {
        set_error("ml_propagate_plan has not been called");
        return ML_ESTATE;
    }
    if (ctx->nx == 0 || ctx->ny == 0) {
        set_error("no resident field set");
        return ML_ESTATE;
    }
    ML_REQUIRE(ctx->n_ranks <= 1, "ml_propagate: this context belongs to a communicator of %d ranks", ctx->n_ranks);
    ML_REQUIRE(Z0 > 0, "Z0 must be positive");
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(fields_unmodulate(ctx));   // as ml_fields_download: the plain near field
    const int T = pp.T, nq = pp.want_h ? 12 : 6, tiles = (T + PROP_THREADS - 1) / PROP_THREADS;
    const int splits = std::max(1, std::min(ctx->nx, (PROP_BLOCKS + tiles - 1) / tiles));
    ML_TRY(pp.partial.reserve((size_t)splits * nq * T * sizeof(double)));
    ML_TRY(pp.result.reserve((size_t)(nq / 2) * T * 2 * sizeof(double)));
    PropArgs a;
    a.fields = reinterpret_cast<const double2 *>(ctx->set_ptr());
    a.row_first = ctx->row_first_valid ? ctx->row_first.as<int>() : nullptr;
    a.tx = pp.targets.as<double>();
    a.ty = a.tx + T;
    a.tz = a.tx + 2 * (size_t)T;
    a.partial = pp.partial.as<double>();
    a.nx = ctx->nx;
    a.ny = ctx->ny;
    a.T = T;
    a.splits = splits;
    a.dxp = pp.dxp;
    a.dyp = pp.dyp;
    a.k = 2.0 * M_PI * pp.n_glass / pp.wavelength;
    a.inv_k = 1.0 / a.k;
    a.Z = Z0 / pp.n_glass;
    const dim3 grid(tiles, splits);
    if (pp.want_h)
        hipLaunchKernelGGL(propagate_kernel<true>, grid, dim3(PROP_THREADS), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(propagate_kernel<false>, grid, dim3(PROP_THREADS), 0, ctx->stream, a);
    ML_HIP(hipGetLastError());
    const double scale_h = a.k * a.k / (4.0 * M_PI) * pp.dxp * pp.dyp;
    hipLaunchKernelGGL(propagate_reduce_kernel, dim3((T + 255) / 256, nq / 2), dim3(256), 0, ctx->stream,
                       pp.partial.as<double>(), pp.result.as<double2>(), T, splits, nq, a.Z * scale_h, scale_h);
    ML_HIP(hipGetLastError());
    pp.have_result = true;
    return ML_OK;
}

int ml_propagate_download(ml_ctx *ctx, double *E, double *H) {
    ML_REQUIRE(ctx && E, "NULL argument");
    PropagatePlan &pp = ctx->prop;
    if (!pp.ready || !pp.have_result) {
        set_error("ml_propagate has not run on the active propagation plan");
        return ML_ESTATE;
    }
    ML_REQUIRE(!H || pp.want_h, "the active propagation plan computes E only");
    ML_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)3 * pp.T * 2 * sizeof(double);
    ML_HIP(hipMemcpyAsync(E, pp.result.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (H) ML_HIP(hipMemcpyAsync(H, (const char *)pp.result.p + bytes, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

}  // extern "C"
