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
// Several field sets in one pass (NS = 2, 3: the members of a synthesis batch, ml_propagate_sets).  Everything above
// that depends on the pair alone - dy, R, 1 / R, Rhat, q, the sincos of k R, w, a, b: about 69 of the 177 vector
// instructions of a pair - is computed once per pair and serves every set; a tile is staged as
// [sample][set][current] (64 NS bytes per sample, 24 KiB at NS = 3) and pair_term runs once per set into that set's own
// accumulators.  The per-pair expressions are the same inlined functions in the same order whatever NS is, nothing is
// contracted (-ffp-contract=off, explicit fma() only) and `splits` does not depend on NS: the result of a set has
// the bits of that set propagated alone.
// A synthesised field carries row extents (nearfield.hip row_extent_kernel): samples outside them are
// exact zeros and are not visited.  The extents are read from the device's own array.  A skipped sample
// would have added +-0 to every accumulator, so the result has the bits of the whole sum.
// The phase k R (1.6e4 rad at 1 mm, 1e7 at 1 m) is the accuracy: R by a correctly rounded square root (nearfield_math.h
// sqrt_exact: bit for bit np.sqrt over 1e-200 ... 1e200), sin / cos by the two-constant Cody-Waite reduction with FMA
// (sincos_cw: within 2^-51 absolute for |k R| <= 1e9) - both held to that on the GPU by tests/test_gpu_device_math.py.
// A target's coordinates against the aperture's origin, x - x0 and y - y0, are kept as two doubles each (propagate_direct.h
// prop_two_diff) and the low part is added behind the fma that forms dx and dy: with the rounded difference alone the
// distance to the sample under a target is off by up to u |x - x0| - a 1e-14 of the field 30 nm behind a sample, 28 x the
// error of the plain NumPy sum (tests/propagate_direct_cases.py, row d-near).  One addition per pair, 0.5 % of a pass.
// k R <= 1e9 is enforced: the plan keeps the targets' bounding box and the largest z, and a plan or a pass whose largest
// possible k R over the aperture exceeds the limit is refused (common.h prop_check_phase; 1e9 is 92 m at 580 nm in glass).
#include "nearfield_math.h"
#include "propagate_direct.h"   // PROP_THREADS, PROP_TILE, PROP_MAX_SETS, PROP_BLOCKS; tiles, splits and buffer sizes of a pass
#include "propagate_pair.h"     // cfma, pair_term and the per-pair prologue: shared with fields_zone_fields.hip

namespace ml {

struct PropArgs {
    const double2 *fields;   // [NS][4][nx][ny]: Ex, Ey, Hx, Hy of the first field set of the pass, the others behind it
    const int *row_first;    // [nx] (row_extent_kernel) or nullptr: every sample is read
    const double *tx, *ty, *tz;   // [T]: x - x0, y - y0, z
    const double *tx_lo, *ty_lo;  // [T]: what the rounding of x - x0 and y - y0 left behind (propagate_direct.h prop_two_diff)
    double *partial;         // [splits][NS][12 or 6][T]
    int nx, ny, T, splits;
    double dxp, dyp, k, inv_k, Z;
};

template <bool WANT_H, int NS>
__global__ __launch_bounds__(PROP_THREADS) void propagate_kernel(const PropArgs a) {
    __shared__ double2 s_cur[PROP_TILE][NS][4];   // per field set: Jx, Jy, Mx / Z, My / Z
    const int tid = threadIdx.x;
    const int t = blockIdx.x * PROP_THREADS + tid;
    const int tc = min(t, a.T - 1);   // (lanes past the last target work on a copy of it and store nothing)
    const double tx = a.tx[tc], ty = a.ty[tc], z = a.tz[tc], ty_lo = a.ty_lo[tc];
    const double zz = z * z;
    const bool wave_live = blockIdx.x * PROP_THREADS + (tid & ~63) < a.T;
    // staging: this thread converts field f of the columns c and c + 64 of a tile into current 3 - f, set by set
    // (propagate_pair.h pair_current)
    const int f = tid >> 6, c = tid & 63;
    const double sg = (f == 0 || f == 3) ? -1.0 : 1.0, den = f < 2 ? a.Z : 1.0;
    const size_t set_stride = (size_t)4 * a.nx * a.ny;
    c2 E[NS][3], H[NS][3];
#pragma unroll
    for (int m = 0; m < NS; ++m)
#pragma unroll
        for (int d = 0; d < 3; ++d) E[m][d] = H[m][d] = c2{0, 0};
    for (int i = blockIdx.y; i < a.nx; i += a.splits) {
        const int first = a.row_first ? a.row_first[i] : 0;   // (0x7f7f7f7f: no sample of the row is inside)
        const int j_hi = a.ny - first;
        if (first >= j_hi) continue;
        // (dx and dy: propagate_pair.h pair_offset, written out)
        const double dx = fma(-(double)i, a.dxp, tx) + a.tx_lo[tc];   // (the low part: once per row, not kept in registers)
        const double s_row = fma(dx, dx, zz);
        const double2 *row = a.fields + ((size_t)f * a.nx + i) * a.ny;
        for (int j0 = first; j0 < j_hi; j0 += PROP_TILE) {
            const int n = min(PROP_TILE, j_hi - j0);
            __syncthreads();   // the previous tile has been read
            for (int cc = c; cc < n; cc += 64) {
#pragma unroll
                for (int m = 0; m < NS; ++m) {
                    const double2 v = (row + m * set_stride)[j0 + cc];
                    s_cur[cc][m][3 - f] = pair_current(sg, den, v);
                }
            }
            __syncthreads();
            if (!wave_live) continue;
            for (int s = 0; s < n; ++s) {
                const double dy = fma(-(double)(j0 + s), a.dyp, ty) + ty_lo;
                const PairGeom g = pair_geom(dx, dy, z, s_row, a.k, a.inv_k);
#pragma unroll
                for (int m = 0; m < NS; ++m) {
                    const double2 v0 = s_cur[s][m][0], v1 = s_cur[s][m][1], v2 = s_cur[s][m][2], v3 = s_cur[s][m][3];
                    const c2 Jx = {v0.x, v0.y}, Jy = {v1.x, v1.y}, Mx = {v2.x, v2.y}, My = {v3.x, v3.y};
                    pair_term<-1>(E[m], g.w, g.q, g.a, g.b, g.ux, g.uy, g.uz, Jx, Jy, Mx, My);
                    if (WANT_H) pair_term<1>(H[m], g.w, g.q, g.a, g.b, g.ux, g.uy, g.uz, Mx, My, Jx, Jy);
                }
            }
        }
    }
    if (t >= a.T) return;
    constexpr int NQ = WANT_H ? 12 : 6;
    double *out = a.partial + (size_t)blockIdx.y * NS * NQ * a.T + t;
#pragma unroll
    for (int m = 0; m < NS; ++m)
        for (int d = 0; d < 3; ++d) {
            out[(size_t)(m * NQ + 2 * d) * a.T] = E[m][d].r;
            out[(size_t)(m * NQ + 2 * d + 1) * a.T] = E[m][d].i;
            if (WANT_H) {
                out[(size_t)(m * NQ + 6 + 2 * d) * a.T] = H[m][d].r;
                out[(size_t)(m * NQ + 7 + 2 * d) * a.T] = H[m][d].i;
            }
        }
}

// second pass: result[set][component][target] = scale * (partial 0 + partial 1 + ...), in that order
__global__ __launch_bounds__(256) void propagate_reduce_kernel(const double *partial, double2 *result, int T, int splits,
                                                               int nq, double scale_e, double scale_h) {
    const int t = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;   // m: complex component, 0-2 E, 3-5 H
    const int set = blockIdx.z, ns = gridDim.z;
    if (t >= T) return;
    double re = 0.0, im = 0.0;
    for (int s = 0; s < splits; ++s) {
        const double *p = partial + (((size_t)s * ns + set) * nq + 2 * m) * T + t;
        re += p[0];
        im += p[T];
    }
    const double scale = m < 3 ? scale_e : scale_h;
    result[((size_t)set * (nq / 2) + m) * T + t] = make_double2(scale * re, scale * im);
}

struct PropWeights {
    double w[PROP_MAX_SETS];
};

// sums[0][t] (+)= sum_m w_m |E_m|^2, sums[1][t] (+)= sum_m w_m Re(E_m x H_m*)_z / 2 over the n sets of `result`: the pass's
// own sum is formed first, in set order, and then added once to what the sums hold (`reset`: to zero) - one lane per
// target, plain stores
__global__ __launch_bounds__(256) void propagate_accumulate_kernel(const double2 *result, double *sums, int T, int n,
                                                                   int want_h, int reset, const PropWeights wt) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int nc = want_h ? 6 : 3;
    double I = 0.0, Sz = 0.0;
    for (int m = 0; m < n; ++m) {
        const double2 *r = result + (size_t)m * nc * T + t;
        const double2 Ex = r[0], Ey = r[T], Ez = r[2 * (size_t)T];
        const double i_m = ((Ex.x * Ex.x + Ex.y * Ex.y) + (Ey.x * Ey.x + Ey.y * Ey.y)) + (Ez.x * Ez.x + Ez.y * Ez.y);
        const double wi = wt.w[m] * i_m;
        I = m == 0 ? wi : I + wi;
        if (want_h) {
            const double2 Hx = r[3 * (size_t)T], Hy = r[4 * (size_t)T];
            const double s_m = 0.5 * ((Ex.x * Hy.x + Ex.y * Hy.y) - (Ey.x * Hx.x + Ey.y * Hx.y));
            const double ws = wt.w[m] * s_m;
            Sz = m == 0 ? ws : Sz + ws;
        }
    }
    sums[t] = reset ? I : sums[t] + I;
    if (want_h) sums[(size_t)T + t] = reset ? Sz : sums[(size_t)T + t] + Sz;
}

template <bool WANT_H>
static void launch_pairs(hipStream_t stream, dim3 grid, const PropArgs &a, int ns) {
    if (ns == 1)
        hipLaunchKernelGGL((propagate_kernel<WANT_H, 1>), grid, dim3(PROP_THREADS), 0, stream, a);
    else if (ns == 2)
        hipLaunchKernelGGL((propagate_kernel<WANT_H, 2>), grid, dim3(PROP_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL((propagate_kernel<WANT_H, 3>), grid, dim3(PROP_THREADS), 0, stream, a);
}

// the sets first ... first + n - 1 of the resident field in one pass -> pp.result [n][6 or 3][T]
static int propagate_sets(ml_ctx *ctx, const char *who, double Z0, int first, int n) {
    PropagatePlan &pp = ctx->prop;
    if (!pp.ready) {
        set_error("ml_propagate_plan has not been called");
        return ML_ESTATE;
    }
    if (ctx->fields.nx == 0 || ctx->fields.ny == 0) {
        set_error("no resident field set");
        return ML_ESTATE;
    }
    ML_REQUIRE(ctx->n_ranks <= 1, "%s: this context belongs to a communicator of %d ranks", who, ctx->n_ranks);
    ML_REQUIRE(Z0 > 0, "Z0 must be positive");
    ML_REQUIRE(n >= 1 && n <= PROP_MAX_SETS, "%s: a pass takes 1 to %d field sets, got %d", who, PROP_MAX_SETS, n);
    ML_REQUIRE(first >= 0 && first + n <= ctx->fields.n_sets, "%s: field sets %d ... %d asked for, %d resident", who, first,
               first + n - 1, ctx->fields.n_sets);
    // the shape is known here at the latest: no pair of this pass may leave the range of the phase arithmetic
    ML_TRY(prop_check_phase(who, pp.extent, ctx->fields.nx, ctx->fields.ny, pp.dxp, pp.dyp, pp.wavelength, pp.n_glass));
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(fields_unmodulate(ctx));   // as ml_fields_download: the plain near field
    if (pp.method != ML_PROPAGATE_DIRECT) return propagate_grid_sets(ctx, Z0, first, n);
    const int T = pp.T, nq = prop_partial_doubles(pp.want_h), tiles = prop_tiles(T);
    const int splits = prop_splits(T, ctx->fields.nx);   // (of T and nx alone)
    pp.have_result = false;
    ML_TRY(pp.partial.reserve(prop_partial_bytes(T, ctx->fields.nx, n, pp.want_h)));
    ML_TRY(pp.result.reserve(prop_result_bytes(T, n, pp.want_h)));
    PropArgs a;
    a.fields = ctx->fields.buf.as<double2>() + (size_t)first * 4 * ctx->fields.nx * ctx->fields.ny;
    a.row_first = ctx->caches.rows_describe_fields ? ctx->grid.row_first.as<int>() : nullptr;
    a.tx = pp.targets.as<double>();
    a.ty = a.tx + T;
    a.tz = a.tx + 2 * (size_t)T;
    a.tx_lo = a.tx + 3 * (size_t)T;
    a.ty_lo = a.tx + 4 * (size_t)T;
    a.partial = pp.partial.as<double>();
    a.nx = ctx->fields.nx;
    a.ny = ctx->fields.ny;
    a.T = T;
    a.splits = splits;
    a.dxp = pp.dxp;
    a.dyp = pp.dyp;
    a.k = 2.0 * M_PI * pp.n_glass / pp.wavelength;
    a.inv_k = 1.0 / a.k;
    a.Z = Z0 / pp.n_glass;
    const dim3 grid(tiles, splits);
    if (pp.want_h)
        launch_pairs<true>(ctx->stream, grid, a, n);
    else
        launch_pairs<false>(ctx->stream, grid, a, n);
    ML_HIP(hipGetLastError());
    const double scale_h = a.k * a.k / (4.0 * M_PI) * pp.dxp * pp.dyp;
    hipLaunchKernelGGL(propagate_reduce_kernel, dim3((T + 255) / 256, nq / 2, n), dim3(256), 0, ctx->stream,
                       pp.partial.as<double>(), pp.result.as<double2>(), T, splits, nq, a.Z * scale_h, scale_h);
    ML_HIP(hipGetLastError());
    pp.have_result = true;
    pp.result_sets = n;
    return ML_OK;
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
    // the targets' bounding box and the largest z stay with the plan: with them every pass bounds k R for the shape it
    // meets (propagate_sets).  A field set resident now is that shape: refuse here, with the previous plan as it was
    PropExtent ext;
    ext.tx_lo = *std::min_element(x, x + nx_t) - x0;
    ext.tx_hi = *std::max_element(x, x + nx_t) - x0;
    ext.ty_lo = *std::min_element(y, y + ny_t) - y0;
    ext.ty_hi = *std::max_element(y, y + ny_t) - y0;
    ext.z_hi = *std::max_element(z, z + nz);
    if (ctx->fields.nx && ctx->fields.ny)
        ML_TRY(prop_check_phase("ml_propagate_plan", ext, ctx->fields.nx, ctx->fields.ny, dxp, dyp, wavelength, n_glass));
    ML_HIP(hipSetDevice(ctx->device));
    PropagatePlan &pp = ctx->prop;
    pp.ready = pp.have_result = pp.have_sums = pp.have_stokes = false;   // results and sums of the previous plan are gone
    pp.modes.planned = false;                           // and its mode tables (propagate_modes.hip)
    pp.method = ML_PROPAGATE_DIRECT;
    pp.spectra_ready = false;
    pp.grid_work.release();   // (the spectra of an FFT plan live as long as that plan)
    std::vector<double> h((size_t)PROP_TARGET_ROWS * T);   // x - x0 and y - y0 as two doubles each: nothing of a target is lost
    for (long long t = 0; t < T; ++t) {
        const int ix = point_list ? (int)t : (int)(t / ny_t), iy = point_list ? (int)t : (int)(t % ny_t);
        h[t] = prop_two_diff(x[ix], x0, &h[3 * T + t]);
        h[T + t] = prop_two_diff(y[iy], y0, &h[4 * T + t]);
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
    pp.extent = ext;
    pp.ready = true;
    return ML_OK;
}

int ml_propagate(ml_ctx *ctx, double Z0) {
    ML_REQUIRE(ctx, "ctx is NULL");
    return propagate_sets(ctx, "ml_propagate", Z0, ctx->fields.field_set, 1);
}

int ml_propagate_sets(ml_ctx *ctx, double Z0, int first_set, int n_sets) {
    ML_REQUIRE(ctx, "ctx is NULL");
    return propagate_sets(ctx, "ml_propagate_sets", Z0, first_set, n_sets);
}

int ml_fields_sets(ml_ctx *ctx, int *n_sets) {
    ML_REQUIRE(ctx && n_sets, "NULL argument");
    *n_sets = (ctx->fields.nx && ctx->fields.ny) ? ctx->fields.n_sets : 0;
    return ML_OK;
}

static int download_set(ml_ctx *ctx, int set, double *E, double *H) {
    PropagatePlan &pp = ctx->prop;
    if (!pp.ready || !pp.have_result) {
        set_error("ml_propagate has not run on the active propagation plan");
        return ML_ESTATE;
    }
    ML_REQUIRE(set >= 0 && set < pp.result_sets, "member %d asked for, the last pass propagated %d field sets", set,
               pp.result_sets);
    ML_REQUIRE(!H || pp.want_h, "the active propagation plan computes E only");
    ML_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)3 * pp.T * 2 * sizeof(double);
    const char *src = (const char *)pp.result.p + (size_t)set * (pp.want_h ? 2 : 1) * bytes;
    ML_HIP(hipMemcpyAsync(E, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (H) ML_HIP(hipMemcpyAsync(H, src + bytes, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

int ml_propagate_download(ml_ctx *ctx, double *E, double *H) {
    ML_REQUIRE(ctx && E, "NULL argument");
    return download_set(ctx, 0, E, H);
}

int ml_propagate_download_set(ml_ctx *ctx, int set, double *E, double *H) {
    ML_REQUIRE(ctx && E, "NULL argument");
    return download_set(ctx, set, E, H);
}

int ml_propagate_accumulate(ml_ctx *ctx, const double *weights, int n, int reset) {
    ML_REQUIRE(ctx && weights, "NULL argument");
    PropagatePlan &pp = ctx->prop;
    if (!pp.ready || !pp.have_result) {
        set_error("ml_propagate has not run on the active propagation plan");
        return ML_ESTATE;
    }
    ML_REQUIRE(n >= 1 && n <= pp.result_sets, "%d field sets to add, the last pass propagated %d", n, pp.result_sets);
    if (!reset && !pp.have_sums) {
        set_error("ml_propagate_accumulate: the active propagation plan has no sums yet (the first call needs reset = 1)");
        return ML_ESTATE;
    }
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(pp.sums.reserve((size_t)2 * pp.T * sizeof(double)));
    PropWeights wt = {};
    for (int m = 0; m < n; ++m) wt.w[m] = weights[m];
    hipLaunchKernelGGL(propagate_accumulate_kernel, dim3((pp.T + 255) / 256), dim3(256), 0, ctx->stream,
                       pp.result.as<double2>(), pp.sums.as<double>(), pp.T, n, (int)pp.want_h, reset, wt);
    ML_HIP(hipGetLastError());
    pp.have_sums = true;
    return ML_OK;
}

int ml_propagate_sums(ml_ctx *ctx, double *I, double *Sz) {
    ML_REQUIRE(ctx && I, "NULL argument");
    PropagatePlan &pp = ctx->prop;
    if (!pp.ready || !pp.have_sums) {
        set_error("ml_propagate_accumulate has not run on the active propagation plan");
        return ML_ESTATE;
    }
    ML_REQUIRE(!Sz || pp.want_h, "the active propagation plan computes E only");
    ML_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)pp.T * sizeof(double);
    ML_HIP(hipMemcpyAsync(I, pp.sums.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (Sz) ML_HIP(hipMemcpyAsync(Sz, (const char *)pp.sums.p + bytes, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

}  // extern "C"
