// The far-field projection: the four radiation vectors of every direction of the active plan -> spherical components
// -> the two far-field amplitudes -> radiated power, elementwise, restating nearfield_farfield.py:153-189 operation by
// operation (project_point; -ffp-contract=off, so NumPy rounds alike).
//   * project_kernel          one direction per lane: all of it (stage 0), the linear part up to the amplitudes (stage 1:
//                             a rank's partial sums, reduced over the ranks) or the power of reduced amplitudes (stage 2)
//   * unfold_project_kernel   the same behind a folded stage 2 whose unfold the transform (farfield.hip) deferred in
//                             pl.unfold: sums the split-K slabs, transposes and signs them into the vectors and projects
//                             them while they are on chip; a spare row of blocks sums the synthesis' power partials
//   * zunfold_out_kernel      the unfold alone (flush_unfold), for whoever wants the vectors before a projection
// Layouts: the vectors, amplitudes and power in FarfieldPlan (common.h), the rank-blocked amplitudes in ProjArgs below.
// Entries: ml_farfield_project_async, ml_farfield_project_reduce, ml_farfield_gather, ml_farfield_project,
// ml_farfield_download, and ml_farfield_lattice_power - the same projection on the caller's FFT'd fields (drop-in for
// farfield_from_nearfield_helper).
#include "common.h"

namespace ml {

struct Alpha4f {
    double v[4];
};

// V[3 - f][a][j] (+)= alpha_f * in[f][j][a]: transposes the folded stage-2 result back into
// the radiation-vector layout, applies the reference's signs x dA and the field -> vector map
// (in may hold `splits` split-K slabs of 4*my*mx elements each; they are summed here)
__global__ __launch_bounds__(256) void zunfold_out_kernel(const double2 *in, double2 *out, int my,
                                                          int mx, Alpha4f alpha, int accumulate,
                                                          int splits) {
    __shared__ double2 tile[32][33];
    const int f = blockIdx.z;
    const size_t plane = (size_t)mx * my;
    in += (size_t)f * plane;
    out += (size_t)(3 - f) * plane;
    const double al = alpha.v[f];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int a0 = blockIdx.x * 32, j0 = blockIdx.y * 32;   // in is [j][a]
    for (int k = ty; k < 32; k += 8)
        if (j0 + k < my && a0 + tx < mx) {
            double2 v = in[(size_t)(j0 + k) * mx + a0 + tx];
            for (int sp = 1; sp < splits; ++sp) {
                const double2 w = in[(size_t)sp * 4 * plane + (size_t)(j0 + k) * mx + a0 + tx];
                v.x += w.x;
                v.y += w.y;
            }
            tile[k][tx] = v;
        }
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (a0 + k < mx && j0 + tx < my) {
            double2 v = tile[tx][k];
            v.x *= al;
            v.y *= al;
            double2 *dst = out + (size_t)(a0 + k) * my + j0 + tx;
            if (accumulate) {
                v.x += dst->x;
                v.y += dst->y;
            }
            *dst = v;
        }
}

struct ProjArgs {
    const double2 *Nx, *Ny, *Lx, *Ly;   // each [mx][my]
    const double *ux, *uy;
    int mx, my, pair_list;
    // N, L = sign * (fft * dxp) * dyp when from_fft (nearfield_farfield.py:135-138)
    int from_fft;
    double dxp, dyp;
    double Z, coef;                      // Z0/n_glass and (2 pi n/lambda)^2 / (32 pi^2 Z)
    double *P;
    double2 *a_theta, *a_phi;            // may be null (stage 0)
    // 0: vectors -> amplitudes -> power in one go; 1: vectors -> amplitudes only (the linear
    // part: a rank's partial sums, to be reduced over the ranks); 2: amplitudes -> power
    int stage;
    // blk_rows > 0: the amplitudes in RANK-BLOCKED order (common.h FarfieldPlan::amp_rows) - element
    // (plane p, direction row i, column j) at ((i / R) 2 R + p R + i mod R) my + j with R = blk_rows,
    // so that block b = rows [b R, (b + 1) R) of BOTH planes is one contiguous chunk: what a
    // reduce-scatter hands rank b.  a_theta = a_phi = the slot's base then.
    int blk_rows;
    int row_lo, row_hi;                  // stage 2: only the direction rows [row_lo, row_hi)
};

__device__ __forceinline__ double2 cscale(double2 a, double s) {
    return make_double2(a.x * s, a.y * s);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) {
    return make_double2(a.x + b.x, a.y + b.y);
}
__device__ __forceinline__ double2 cneg(double2 a) { return make_double2(-a.x, -a.y); }

// One direction: radiation vectors -> spherical components -> the two far-field amplitudes ->
// power (nearfield_farfield.py:153-189).  Shared by the stand-alone kernel and the fused
// unfold + projection kernel so that both produce the same bits.
__device__ __forceinline__ void project_point(const ProjArgs &a, size_t at, int i, int j,
                                              double2 Nx, double2 Ny, double2 Lx, double2 Ly) {
    const double ux = a.ux[i];
    const double uy = a.pair_list ? a.uy[i] : a.uy[j];
    double uz = 1 - ux * ux - uy * uy;
    uz = (uz < 0) ? NAN : sqrt(uz);
    size_t ta = at, pa = at;   // where this direction's two amplitudes live
    if (a.blk_rows) {
        ta = ((size_t)(i / a.blk_rows) * a.blk_rows + i) * a.my + j;
        pa = ta + (size_t)a.blk_rows * a.my;
    }
    if (a.stage == 2) {
        if (i < a.row_lo || i >= a.row_hi) return;
        const double2 at_ = a.a_theta[ta], ap_ = a.a_phi[pa];
        const double m1 = hypot(at_.x, at_.y), m2 = hypot(ap_.x, ap_.y);
        double P = (a.coef * (m1 * m1 + m2 * m2)) / (uz + 1e-5);
        P *= 2;
        a.P[at] = P;
        return;
    }
    if (a.from_fft) {
        // Nx = -fftHy*dxp*dyp, Ny = fftHx*dxp*dyp, Lx = fftEy*dxp*dyp, Ly = -fftEx*dxp*dyp
        Nx = cscale(cscale(cneg(Nx), a.dxp), a.dyp);
        Ny = cscale(cscale(Ny, a.dxp), a.dyp);
        Lx = cscale(cscale(Lx, a.dxp), a.dyp);
        Ly = cscale(cscale(cneg(Ly), a.dxp), a.dyp);
    }
    const double sintheta = sqrt(ux * ux + uy * uy);
    const double scl = 1.0 / (sintheta + 1e-9);   // numpy: complex / real = multiply by 1/x
    double2 Nth, Nph, Lth, Lph;
    if (ux == 0 && uy == 0) {
        Nth = Nx;
        Nph = Ny;
        Lth = Lx;
        Lph = Ly;
    } else {
        Nth = cadd(cscale(cscale(cscale(Nx, ux), uz), scl), cscale(cscale(cscale(Ny, uy), uz), scl));
        Nph = cadd(cscale(cscale(cneg(Nx), uy), scl), cscale(cscale(Ny, ux), scl));
        Lth = cadd(cscale(cscale(cscale(Lx, ux), uz), scl), cscale(cscale(cscale(Ly, uy), uz), scl));
        Lph = cadd(cscale(cscale(cneg(Lx), uy), scl), cscale(cscale(Ly, ux), scl));
    }
    const double2 at_ = cadd(Lph, cscale(Nth, a.Z));            // Lphi + Z*Ntheta
    const double2 ap_ = cadd(Lth, cneg(cscale(Nph, a.Z)));      // Ltheta - Z*Nphi
    if (a.stage == 1) {
        a.a_theta[ta] = at_;
        a.a_phi[pa] = ap_;
        return;
    }
    const double m1 = hypot(at_.x, at_.y), m2 = hypot(ap_.x, ap_.y);
    double P = (a.coef * (m1 * m1 + m2 * m2)) / (uz + 1e-5);
    P *= 2;
    a.P[at] = P;
    if (a.a_theta) a.a_theta[ta] = at_;
    if (a.a_phi) a.a_phi[pa] = ap_;
}

__global__ __launch_bounds__(256) void project_kernel(const ProjArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= a.my) return;
    const size_t at = (size_t)i * a.my + j;
    const double2 zero = make_double2(0.0, 0.0);
    if (a.stage == 2)
        project_point(a, at, i, j, zero, zero, zero, zero);
    else
        project_point(a, at, i, j, a.Nx[at], a.Ny[at], a.Lx[at], a.Ly[at]);
}

// The folded stage 2 leaves `splits` split-K slabs in[sp][f][j][a]; this kernel sums them,
// transposes to the radiation-vector layout V[3 - f][a][j] (+)= alpha_f * in (exactly what
// zunfold_out_kernel does, same order of additions) AND projects the four vectors of each
// direction while they are on chip.  One block = 8 x 8 directions x 4 fields; block index
// row gridDim.y - 1 is a spare row of blocks, launched when power partials are pending, which sums
// the synthesis kernel's incident-power partials into their POWER_GROUPS group sums instead.
struct UnfoldArgs {
    const double2 *in;
    double2 *out;
    Alpha4f alpha;
    int accumulate, splits;
    const double *partial;   // null: no power sum
    int n_partials;
    double *power_out;
};

__global__ __launch_bounds__(256) void unfold_project_kernel(const ProjArgs a, const UnfoldArgs u) {
    if (u.partial && blockIdx.y == gridDim.y - 1) {   // the spare row of blocks
        for (int g = blockIdx.x; g < POWER_GROUPS; g += gridDim.x)
            sum_partials_group(u.partial, u.n_partials, u.power_out, g, threadIdx.x);
        return;
    }
    // one block = 8 x 8 directions x 4 fields: thread (f, ty, tx) sums the slabs of one element
    // (four times as many blocks as one thread per direction with all four fields: 12 vs 15 us at
    // 256 x 256 directions, the same at 512 x 512)
    __shared__ double2 tile[4][8][9];
    const int mx = a.mx, my = a.my;
    const size_t plane = (size_t)mx * my;
    const int f = threadIdx.x >> 6, ty = (threadIdx.x >> 3) & 7, tx = threadIdx.x & 7;
    const int a0 = blockIdx.x * 8, j0 = blockIdx.y * 8;   // in is [j][a]
    if (j0 + ty < my && a0 + tx < mx) {
        const double2 *src = u.in + (size_t)f * plane + (size_t)(j0 + ty) * mx + a0 + tx;
        double2 v = src[0];
        for (int sp = 1; sp < u.splits; ++sp) {
            const double2 w = src[(size_t)sp * 4 * plane];
            v.x += w.x;
            v.y += w.y;
        }
        tile[f][ty][tx] = v;
    }
    __syncthreads();
    // transposed: now ty walks the directions' first axis; every thread writes its field's plane
    const int i = a0 + ty, j = j0 + tx;
    const bool in_range = i < mx && j < my;
    const size_t at = (size_t)i * my + j;
    if (in_range) {
        double2 v = tile[f][tx][ty];
        v.x *= u.alpha.v[f];
        v.y *= u.alpha.v[f];
        double2 *dst = u.out + (size_t)(3 - f) * plane + at;
        if (u.accumulate) {
            v.x += dst->x;
            v.y += dst->y;
        }
        *dst = v;
        tile[f][tx][ty] = v;   // own element: no other thread reads it before the barrier
    }
    __syncthreads();
    if (f == 0 && in_range)   // one wave projects the 64 directions; plane p = field 3 - p
        project_point(a, at, i, j, tile[3][tx][ty], tile[2][tx][ty], tile[1][tx][ty], tile[0][tx][ty]);
}

// Materialise the radiation vectors of a folded stage 2 whose unfold was deferred.
int flush_unfold(ml_ctx *ctx) {
    FarfieldPlan &pl = ctx->plan;
    if (!pl.unfold.pending) return ML_OK;
    Alpha4f al;
    for (int k = 0; k < 4; ++k) al.v[k] = pl.unfold.alpha[k];
    hipLaunchKernelGGL(zunfold_out_kernel, dim3((pl.mx + 31) / 32, (pl.my + 31) / 32, 4), dim3(256),
                       0, ctx->stream, pl.fold2_ot.as<double2>(), pl.vectors.as<double2>(), pl.my,
                       pl.mx, al, pl.unfold.accumulate, pl.unfold.splits);
    ML_HIP(hipGetLastError());
    pl.unfold.pending = false;
    return ML_OK;
}

// The arguments of a plain projection (stage 0) of mx x my directions whose four vector planes, n elements each, lie
// one behind the other from `base` on: vectors as they are, every row, no amplitudes kept, no power plane yet.  The
// callers set what differs.
static ProjArgs proj_args(const double2 *base, size_t n, const double *ux, const double *uy, int mx, int my,
                          double n_glass, double wavelength, double Z0) {
    ProjArgs a;
    a.Nx = base;
    a.Ny = base + n;
    a.Lx = base + 2 * n;
    a.Ly = base + 3 * n;
    a.ux = ux;
    a.uy = uy;
    a.mx = mx;
    a.my = my;
    a.pair_list = 0;
    a.from_fft = 0;
    a.dxp = a.dyp = 1.0;
    a.Z = Z0 / n_glass;
    a.coef = pow(2 * M_PI * n_glass / wavelength, 2) / (32 * pow(M_PI, 2) * a.Z);
    a.P = nullptr;
    a.a_theta = a.a_phi = nullptr;
    a.stage = 0;
    a.blk_rows = 0;
    a.row_lo = 0;
    a.row_hi = mx;
    return a;
}

static int project_launch(ml_ctx *ctx, const ProjArgs &a, int kernel_id, hipStream_t stream = nullptr) {
    // (the power kernel behind a reduction on the second stream is not timed as a projection)
    ProfScope scope(ctx, stream ? ML_K_COUNT : kernel_id);
    hipLaunchKernelGGL(project_kernel, dim3((a.my + 255) / 256, a.mx), dim3(256), 0,
                       stream ? stream : ctx->stream, a);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

static int project_stage(ml_ctx *ctx, double Z0, int stage, hipStream_t stream = nullptr) {
    ML_REQUIRE(ctx, "ctx is NULL");
    FarfieldPlan &pl = ctx->plan;
    if (!pl.ready || !pl.have_vectors) {
        set_error("no radiation vectors: call ml_farfield_plan and ml_farfield_transform first");
        return ML_ESTATE;
    }
    ML_HIP(hipSetDevice(ctx->device));
    const int mx = pl.mx, my = pl.out_my();
    const size_t n = pl.directions();
    ProjArgs a = proj_args(pl.vectors.as<double2>(), n, pl.ux.as<double>(), pl.uy.as<double>(), mx, my, pl.n_glass,
                           pl.wavelength, Z0);
    a.pair_list = pl.pair_list;
    a.P = pl.power.as<double>();
    a.a_theta = reinterpret_cast<double2 *>(pl.amp_ptr());
    a.a_phi = a.a_theta + n;
    a.stage = stage;
    a.blk_rows = stage == 0 ? 0 : pl.amp_rows;
    if (a.blk_rows) {
        a.a_phi = a.a_theta;
        if (stage == 2 && !pl.amp_gathered) {   // this rank holds the sum of its own block only
            a.row_lo = ctx->rank * pl.amp_rows;
            a.row_hi = a.row_lo + pl.amp_rows;
        }
    }
    if (pl.unfold.pending && stage != 2) {
        // vectors still in split-K slabs: unfold and project in one kernel, and let a spare
        // block sum the synthesis kernel's power partials if they are waiting too
        UnfoldArgs u;
        u.in = pl.fold2_ot.as<double2>();
        u.out = pl.vectors.as<double2>();
        for (int k = 0; k < 4; ++k) u.alpha.v[k] = pl.unfold.alpha[k];
        u.accumulate = pl.unfold.accumulate;
        u.splits = pl.unfold.splits;
        u.partial = ctx->out.power_pending ? ctx->out.partial_power.as<double>() : nullptr;
        u.n_partials = ctx->out.n_partials;
        u.power_out = ctx->out.power.as<double>();
        ProfScope scope(ctx, ML_K_PROJECT);
        hipLaunchKernelGGL(unfold_project_kernel,
                           dim3((mx + 7) / 8, (my + 7) / 8 + (u.partial ? 1 : 0)), dim3(256), 0,
                           ctx->stream, a, u);
        ML_HIP(hipGetLastError());
        pl.unfold.pending = false;
        ctx->out.power_pending = false;
        return ML_OK;
    }
    ML_TRY(flush_unfold(ctx));
    return project_launch(ctx, a, ML_K_PROJECT, stream);
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_farfield_project_async(ml_ctx *ctx, double Z0) {
    if (ctx && ctx->plan.amplitudes_reduced) return ML_OK;   // ml_farfield_project_reduce did it
    if (ctx) {
        ctx->plan.amp_rows = 0;
        ctx->plan.amp_gathered = true;
    }
    return project_stage(ctx, Z0, 0);
}

// Multi-GPU: the projection is linear up to the two complex amplitudes, so the ranks' partial
// radiation vectors need not be summed themselves: project locally, all-reduce 2 complex
// planes instead of 4, then take the power (nearfield_farfield.py:184-189).  The radiation
// vectors stay local partial sums (ml_farfield_allreduce sums those, if they are wanted).
// With a communicator the all-reduce (latency-bound: 2 planes of a few MB over xGMI) and the power
// kernel behind it run on the context's second stream: the main stream only projects the partial
// sums into the free amplitude slot and moves on to the next step's synthesis.
int ml_farfield_project_reduce(ml_ctx *ctx, double Z0) {
    ML_REQUIRE(ctx, "ctx is NULL");
    FarfieldPlan &pl = ctx->plan;
    const bool overlap = ctx->comm || ctx->comm_file;
    if (!overlap) {
        pl.amp_rows = 0;
        pl.amp_gathered = true;
        ML_TRY(project_stage(ctx, Z0, 1));
        ML_TRY(project_stage(ctx, Z0, 2));
        pl.amplitudes_reduced = true;
        return ML_OK;
    }
    ML_HIP(hipSetDevice(ctx->device));
    if (!ctx->comm_stream) {
        ML_HIP(hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            ML_HIP(hipEventCreateWithFlags(&ctx->amp_ready[k], hipEventDisableTiming));
            ML_HIP(hipEventCreateWithFlags(&ctx->reduce_done[k], hipEventDisableTiming));
        }
    }
    const int slot = pl.amp_slot ^ 1;
    // the reduction that last used this slot (two calls ago) has to be through with it
    // (timed as ML_K_COMM_WAIT: what the main stream loses to a collective that has not caught up)
    if (ctx->reduce_in_flight) {
        ProfScope wait_scope(ctx, ML_K_COMM_WAIT);
        ML_HIP(hipStreamWaitEvent(ctx->stream, ctx->reduce_done[slot], 0));
    }
    pl.amp_slot = slot;
    // REDUCE-SCATTER where the direction rows divide by the rank count: every rank ends up with the
    // sum of ONE block of rows (both amplitudes) and takes the power of that block - (G - 1) / G of the
    // payload per rank where the all-reduce moves 2 (G - 1) / G.  ml_farfield_gather completes the
    // picture on every rank when somebody asks for it.
    const int G = ctx->n_ranks;
    const int mx = pl.mx;
    const bool scatter = G > 1 && mx % G == 0 && !ctx->reduce_by_allreduce;
    pl.amp_rows = scatter ? mx / G : 0;
    pl.amp_gathered = !scatter;
    ML_TRY(project_stage(ctx, Z0, 1));
    ML_HIP(hipEventRecord(ctx->amp_ready[slot], ctx->stream));
    ML_HIP(hipStreamWaitEvent(ctx->comm_stream, ctx->amp_ready[slot], 0));
    const size_t n = pl.directions();
    {
        ProfScope coll_scope(ctx, ML_K_COLLECTIVE, ctx->comm_stream);
        if (scatter)
            ML_TRY(comm_reduce_scatter_sum(ctx, pl.amp_ptr(), 2 * n * 2 / G, ctx->comm_stream));
        else
            ML_TRY(comm_allreduce_sum(ctx, pl.amp_ptr(), 2 * n * 2, ctx->comm_stream));
    }
    ML_TRY(project_stage(ctx, Z0, 2, ctx->comm_stream));
    ML_HIP(hipEventRecord(ctx->reduce_done[slot], ctx->comm_stream));
    ctx->reduce_in_flight = true;
    pl.amplitudes_reduced = true;
    return ML_OK;
}

int ml_farfield_gather(ml_ctx *ctx) {
    ML_REQUIRE(ctx, "ctx is NULL");
    FarfieldPlan &pl = ctx->plan;
    if (!pl.amp_rows || pl.amp_gathered) return ML_OK;
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(comm_join(ctx, false));   // the reduce-scatter and the block's power are on the second stream
    const int G = ctx->n_ranks;
    const size_t n = pl.directions();
    ML_TRY(comm_allgather(ctx, pl.amp_ptr(), 2 * n * 2 / G, ctx->stream));
    ML_TRY(comm_allgather(ctx, pl.power.as<double>(), n / G, ctx->stream));
    pl.amp_gathered = true;
    return ML_OK;
}

int ml_farfield_project(ml_ctx *ctx, double Z0, double *P, double *a_theta, double *a_phi) {
    ML_TRY(ml_farfield_project_async(ctx, Z0));
    ML_TRY(comm_join(ctx, false));   // a reduction on the second stream writes what is copied here
    FarfieldPlan &pl = ctx->plan;
    if (pl.amp_rows && !pl.amp_gathered) {
        set_error("the amplitudes are scattered over the ranks: every rank calls ml_farfield_gather first");
        return ML_ESTATE;
    }
    const int my = pl.out_my();
    const size_t n = pl.directions();
    if (P)
        ML_HIP(hipMemcpyAsync(P, pl.power.p, n * sizeof(double), hipMemcpyDeviceToHost,
                              ctx->stream));
    // rank-blocked amplitudes (blocks of amp_rows direction rows, both planes per block) are put
    // back in order by the copies
    const size_t rows = pl.amp_rows ? pl.amp_rows : pl.mx, blocks = pl.mx / rows, chunk = rows * my * 2;
    for (size_t b = 0; b < blocks; ++b) {
        const double *src = pl.amp_ptr() + b * 2 * chunk;
        if (a_theta)
            ML_HIP(hipMemcpyAsync(a_theta + b * chunk, src, chunk * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (a_phi)
            ML_HIP(hipMemcpyAsync(a_phi + b * chunk, src + (pl.amp_rows ? chunk : 2 * n), chunk * sizeof(double),
                                  hipMemcpyDeviceToHost, ctx->stream));
    }
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return prof_harvest(ctx);
}

int ml_farfield_download(ml_ctx *ctx, double *Nx, double *Ny, double *Lx, double *Ly) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_TRY(comm_join(ctx, false));
    FarfieldPlan &pl = ctx->plan;
    if (!pl.ready || !pl.have_vectors) {
        set_error("no radiation vectors to download");
        return ML_ESTATE;
    }
    ML_HIP(hipSetDevice(ctx->device));
    ML_TRY(flush_unfold(ctx));
    const size_t n = pl.directions();
    double *dst[4] = {Nx, Ny, Lx, Ly};
    for (int k = 0; k < 4; ++k)
        if (dst[k])
            ML_HIP(hipMemcpyAsync(dst[k], pl.vectors.as<double>() + k * n * 2,
                                  n * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}

int ml_farfield_lattice_power(ml_ctx *ctx, int nx, int ny, const double *fftEx,
                              const double *fftEy, const double *fftHx, const double *fftHy,
                              const double *ux_list, const double *uy_list, double dxp, double dyp,
                              double wavelength, double n_glass, double Z0, double *P) {
    ML_REQUIRE(ctx && fftEx && fftEy && fftHx && fftHy && ux_list && uy_list && P, "NULL argument");
    ML_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    ML_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)nx * ny;
    DevBuf &in = ctx->lattice_in;
    ML_TRY(in.reserve(4 * n * 2 * sizeof(double) + (nx + ny) * sizeof(double) + n * sizeof(double)));
    double *base = in.as<double>();
    // order in the staging buffer: Nx<-fftHy, Ny<-fftHx, Lx<-fftEy, Ly<-fftEx
    const double *src[4] = {fftHy, fftHx, fftEy, fftEx};
    for (int k = 0; k < 4; ++k)
        ML_HIP(hipMemcpyAsync(base + k * n * 2, src[k], n * 2 * sizeof(double),
                              hipMemcpyHostToDevice, ctx->stream));
    double *d_ux = base + 4 * n * 2, *d_uy = d_ux + nx, *d_P = d_uy + ny;
    ML_HIP(hipMemcpyAsync(d_ux, ux_list, nx * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ML_HIP(hipMemcpyAsync(d_uy, uy_list, ny * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ProjArgs a = proj_args(reinterpret_cast<const double2 *>(base), n, d_ux, d_uy, nx, ny, n_glass, wavelength, Z0);
    a.from_fft = 1;
    a.dxp = dxp;
    a.dyp = dyp;
    a.P = d_P;
    ML_TRY(project_launch(ctx, a, ML_K_LATTICE_POWER));
    ML_HIP(hipMemcpyAsync(P, d_P, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return prof_harvest(ctx);
}

}  // extern "C"
