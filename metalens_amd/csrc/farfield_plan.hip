// The far-field plan: what ml_farfield_plan sets up for the transform (farfield.hip) and the projection
// (farfield_project.hip), which meet only through FarfieldPlan (common.h).  A plan holds the direction cosines, the
// buffers of the radiation vectors, amplitudes and power, and per axis the phase tables of the way that axis will run:
//   * twiddle_kernel       the complex tables exp(-i k x' u) of the generic GEMM and the pair-list column dot
//   * phase_batch_kernel   the cos / sin tables, input modulation and output diagonal of the folded GEMM (zfold.hip), the
//                          three to five tables of an axis in one launch
//   * plan_fft_axis        the per-bin tables of an axis whose directions sit on the aperture's FFT lattice (zfft.hip)
// Every phase is reduced mod one turn in double-double before the sin/cos (phases reach ~1e4 rad).  Which way an axis
// runs is decided from plain facts in transform_route.h (fold_split, zfft_axis_rule); the layouts of the tables are
// documented with FoldAxis and ZfftAxis in common.h.
// Two tables depend on the call, not on the plan alone, and are built by the transform on first use: stage2_tables
// (which rows are resident) and need_tw_x (only the generic stage 2 reads it).
// Entries: ml_farfield_plan, ml_farfield_plan_info, ml_farfield_plan_kernels, and the options a plan is made under -
// ml_farfield_set_method, ml_farfield_set_precision, ml_nearfield_premodulate (undone by fields_unmodulate).
#include "common.h"
#include "zfft_core.h"

namespace ml {

// 2*pi split into two doubles
#define ML_TWO_PI_HI 6.283185307179586232e+00
#define ML_TWO_PI_LO 2.449293598294706414e-16

// out[r][c] = exp(-2 pi i * frac(s * (sample - center) * u[dir])),
// (sample, dir) = (r, c) if sample_major else (c, r).
__global__ __launch_bounds__(256) void twiddle_kernel(double2 *out, int rows, int cols,
                                                      int sample_major, int center, double s_hi,
                                                      double s_lo, const double *u) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (c >= cols) return;
    const int sample = sample_major ? r : c;
    const int dir = sample_major ? c : r;
    const double kk = (double)(sample - center);
    const double uu = u[dir];
    // p = kk * s  (double-double), q = p * u (double-double)
    const double p_hi = kk * s_hi;
    const double p_lo = fma(kk, s_hi, -p_hi) + kk * s_lo;
    const double q_hi = p_hi * uu;
    const double q_lo = fma(p_hi, uu, -q_hi) + p_lo * uu;
    const double f = (q_hi - rint(q_hi)) + q_lo;   // turns, |f| <= 0.5 (+ tiny)
    const double a_hi = f * ML_TWO_PI_HI;
    const double ang = a_hi + (fma(f, ML_TWO_PI_HI, -a_hi) + f * ML_TWO_PI_LO);
    double sn, cs;
    sincos(ang, &sn, &cs);
    out[(size_t)r * cols + c] = make_double2(cs, -sn);
}

// General phase table: out[r][c] = exp(-2 pi i frac(s * coord * u)) with
// coord = coord0 + coord_step * (sample index), u = u_hi[dir] + u_lo[dir] (u_lo may be null),
// (sample, dir) = (r, c) if sample_major else (c, r).  outc != null writes cos and +sin
// into two REAL planes (outc, outs) instead of one complex array.
// Several phase tables in ONE launch (a plan needs 3-5 small ones; launched separately they
// cost more in launch latency than in arithmetic).  Job j owns blocks [block0[j], block0[j+1]).
constexpr int MAX_PHASE_JOBS = 6;
struct PhaseJob {
    double2 *out;
    double *outc, *outs;
    int rows, cols, sample_major, block0;
    double coord0, coord_step, s_hi, s_lo;
    const double *u_hi, *u_lo;
};
struct PhaseBatch {
    PhaseJob job[MAX_PHASE_JOBS];
    int n, blocks;
};

__global__ __launch_bounds__(256) void phase_batch_kernel(const PhaseBatch b) {
    int j = 0;
    for (int k = 1; k < b.n; ++k)
        if ((int)blockIdx.x >= b.job[k].block0) j = k;
    const PhaseJob &q = b.job[j];
    const int per_row = (q.cols + 255) / 256;
    const int local = blockIdx.x - q.block0;
    const int r = local / per_row, c = (local % per_row) * 256 + threadIdx.x;
    if (c >= q.cols) return;
    const int sample = q.sample_major ? r : c;
    const int dir = q.sample_major ? c : r;
    const double kk = q.coord0 + q.coord_step * (double)sample;   // exact: (half-)integers
    const double uh = q.u_hi[dir], ul = q.u_lo ? q.u_lo[dir] : 0.0;
    const double p_hi = kk * q.s_hi;
    const double p_lo = fma(kk, q.s_hi, -p_hi) + kk * q.s_lo;
    const double q_hi = p_hi * uh;
    const double q_lo = fma(p_hi, uh, -q_hi) + (p_lo * uh + p_hi * ul);
    const double fr = (q_hi - rint(q_hi)) + q_lo;
    const double a_hi = fr * ML_TWO_PI_HI;
    const double ang = a_hi + (fma(fr, ML_TWO_PI_HI, -a_hi) + fr * ML_TWO_PI_LO);
    double sn, cs;
    sincos(ang, &sn, &cs);
    const size_t at = (size_t)r * q.cols + c;
    if (q.outc) {
        q.outc[at] = cs;
        q.outs[at] = sn;
    } else {
        q.out[at] = make_double2(cs, -sn);
    }
}

static void batch_add(PhaseBatch &b, double2 *out, double *outc, double *outs, int rows, int cols,
                      int sample_major, double coord0, double coord_step, double s_hi, double s_lo,
                      const double *u_hi, const double *u_lo) {
    PhaseJob &q = b.job[b.n++];
    q.out = out;
    q.outc = outc;
    q.outs = outs;
    q.rows = rows;
    q.cols = cols;
    q.sample_major = sample_major;
    q.block0 = b.blocks;
    q.coord0 = coord0;
    q.coord_step = coord_step;
    q.s_hi = s_hi;
    q.s_lo = s_lo;
    q.u_hi = u_hi;
    q.u_lo = u_lo;
    b.blocks += ((cols + 255) / 256) * rows;
}

static int batch_launch(ml_ctx *ctx, const PhaseBatch &b) {
    if (b.n == 0) return ML_OK;
    hipLaunchKernelGGL(phase_batch_kernel, dim3(b.blocks), dim3(256), 0, ctx->stream, b);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

// fields[f][i][j] *= conj(E[j]) (undo ml_nearfield_premodulate before the fields leave the GPU)
__global__ __launch_bounds__(256) void zunmodulate_kernel(double2 *fields, const double2 *E, int ny,
                                                          size_t n) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n) return;
    const double2 e = E[at % ny], v = fields[at];
    fields[at] = make_double2(v.x * e.x + v.y * e.y, v.y * e.x - v.x * e.y);
}

static int launch_twiddle(ml_ctx *ctx, double *out, int rows, int cols, int sample_major, int n,
                          double step, double wavelength, double n_glass, const double *u_dev) {
    // turns per (sample index x direction cosine): n_glass * step / wavelength, in extended
    // precision on the host, split into two doubles
    const long double s = (long double)n_glass * (long double)step / (long double)wavelength;
    const double s_hi = (double)s;
    const double s_lo = (double)(s - (long double)s_hi);
    const int center = n - n / 2;   // ceil(n/2): fftshift moves sample j to (j + n//2) mod n
    ProfScope scope(ctx, ML_K_TWIDDLE);
    hipLaunchKernelGGL(twiddle_kernel, dim3((cols + 255) / 256, rows), dim3(256), 0, ctx->stream,
                       reinterpret_cast<double2 *>(out), rows, cols, sample_major, center, s_hi,
                       s_lo, u_dev);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

// Host arrays that parametrise a plan are kept in the plan and re-uploaded only when they
// change, so that re-planning the same geometry every step queues kernels only (no host
// synchronisation): the phase tables themselves are recomputed on every call.
static int upload_if_changed(ml_ctx *ctx, DevBuf &dev, std::vector<double> &host,
                             const double *src, size_t n) {
    if (host.size() == n && dev.p && memcmp(host.data(), src, n * sizeof(double)) == 0)
        return ML_OK;
    // an earlier asynchronous copy may still be reading `host`
    ML_HIP(hipStreamSynchronize(ctx->stream));
    host.assign(src, src + n);
    ML_TRY(dev.reserve(std::max<size_t>(n, 2) * sizeof(double)));
    ML_HIP(hipMemcpyAsync(dev.p, host.data(), n * sizeof(double), hipMemcpyHostToDevice,
                          ctx->stream));
    return ML_OK;
}

// Phase tables of the folded GEMM (zfold.hip) along one axis: m directions (`directions` on the device, split into
// S half-directions in ax.v), n_total samples `step` apart of which `rows` from row0 on are resident - or, mirrored,
// rows / 2 from row0 and their mirror images.  Pair t of resident samples sits at +/- (half - row0 - t) step.
static int fold_tables(ml_ctx *ctx, FoldAxis &ax, int S, const DevBuf &directions, int m, int n_total, double step,
                       int row0, int rows, int mirrored) {
    const FarfieldPlan &pl = ctx->plan;
    const int T = (rows + 1) / 2;
    ML_TRY(ax.cm.reserve((size_t)T * S * sizeof(double)));
    ML_TRY(ax.sm.reserve((size_t)T * S * sizeof(double)));
    ML_TRY(ax.r4.reserve((size_t)S * 2 * sizeof(double)));
    ML_TRY(ax.E.reserve((size_t)rows * 2 * sizeof(double)));
    ML_TRY(ax.D.reserve((size_t)m * 2 * sizeof(double)));
    // turns per (sample index x u)
    const long double sl = (long double)pl.n_glass / (long double)pl.wavelength * (long double)step;
    const double s_hi = (double)sl, s_lo = (double)(sl - (long double)s_hi);
    const double half = 0.5 * (n_total - 1);
    // (the single direction u_c travels behind v)
    const double *v_hi = ax.v.as<double>(), *v_lo = v_hi + S, *uc = v_hi + 2 * (size_t)S;
    ProfScope scope(ctx, ML_K_TWIDDLE);
    PhaseBatch pb;
    pb.n = pb.blocks = 0;
    // cos / sin of kappa p_t v_s, p_t = (half - row0 - t) step
    batch_add(pb, nullptr, ax.cm.as<double>(), ax.sm.as<double>(), T, S, 1, half - row0, -1.0, s_hi, s_lo, v_hi, v_lo);
    // rotation that advances the table by four samples: cos / sin of kappa (4 step) v_s
    batch_add(pb, nullptr, ax.r4.as<double>(), ax.r4.as<double>() + S, 1, S, 1, 4.0, 0.0, s_hi, s_lo, v_hi, v_lo);
    if (ax.has_E) {
        // input modulation E_k = exp(-i kappa p_k u_c), p_k = (k - half) step, at the resident samples: one run, or
        // two for a mirrored shard; skipped when u_c == 0
        const int h = mirrored ? rows / 2 : rows;
        batch_add(pb, ax.E.as<double2>(), nullptr, nullptr, 1, h, 0, row0 - half, 1.0, s_hi, s_lo, uc, uc + 1);
        if (mirrored)
            batch_add(pb, ax.E.as<double2>() + h, nullptr, nullptr, 1, h, 0, (double)(n_total - row0 - h) - half, 1.0,
                      s_hi, s_lo, uc, uc + 1);
    }
    // output diagonal D_j = exp(-i kappa delta u_j), delta = (half - ceil(n_total / 2)) step
    const double delta = half - (double)(n_total - n_total / 2);
    batch_add(pb, ax.D.as<double2>(), nullptr, nullptr, 1, m, 1, delta, 0.0, s_hi, s_lo, directions.as<double>(), nullptr);
    return batch_launch(ctx, pb);
}

// Can the GEMM along one axis run folded (zfold.hip)?  Needs directions that are centre-symmetric to within
// symmetry_tolerance of phase at the aperture edge (transform_route.h fold_split); uploads the split directions.
static int plan_fold_axis(ml_ctx *ctx, FoldAxis &ax, const double *u, int m, int n, double step, bool &fold, int &S) {
    const FoldSplit f = fold_split(u, m, n, step, ctx->plan.wavelength, ctx->plan.n_glass);
    if (!f.ok) return ML_OK;
    ML_TRY(upload_if_changed(ctx, ax.v, ax.h_v, f.v.data(), f.v.size()));
    ax.has_E = f.has_E;
    fold = true;
    S = f.S;
    return ML_OK;
}

// stage 1 (needs a tensor grid): every sample of a row is resident, so its tables are built with the plan
static int plan_fold(ml_ctx *ctx, const double *uy) {
    FarfieldPlan &pl = ctx->plan;
    pl.fold = false;
    static const bool disabled = diag_int("ML_NO_FOLD", 0) != 0;
    if (disabled || pl.pair_list) return ML_OK;
    ML_TRY(plan_fold_axis(ctx, pl.fold_y, uy, pl.my, pl.ny, pl.dyp, pl.fold, pl.fold_S));
    return pl.fold ? fold_tables(ctx, pl.fold_y, pl.fold_S, pl.uy, pl.my, pl.ny, pl.dyp, 0, pl.ny, 0) : ML_OK;
}

// stage 2: its tables depend on which aperture rows are resident and are built in the transform call (stage2_tables)
static int plan_fold2(ml_ctx *ctx, const double *ux) {
    FarfieldPlan &pl = ctx->plan;
    pl.fold2 = false;
    static const bool disabled = diag_int("ML_NO_FOLD2", 0) != 0;
    if (disabled || pl.pair_list) return ML_OK;
    return plan_fold_axis(ctx, pl.fold_x, ux, pl.mx, pl.nx_total, pl.dxp, pl.fold2, pl.fold2_S);
}

// Does the direction grid along one axis sit on the FFT lattice of that aperture axis (zfft.hip)?
// If so build its per-bin tables.  n samples `step` apart, sample j at (j - ceil(n/2)) step.
static int plan_fft_axis(ml_ctx *ctx, ZfftAxis &ax, int n, double step, const double *u, int m) {
    FarfieldPlan &pl = ctx->plan;
    ax.ok = false;
    int N_eff = 0, j0 = 0, jstep = 1;
    int N_plain = 0;
    const bool fits256 = zfft_axis_lattice(n, step, pl.wavelength, pl.n_glass, u, m, &N_eff, &j0, &jstep, &N_plain);
    ax.A = ax.B = ax.R = 0;
    // 'fft-mixed': a lattice that is not a multiple of 256 long runs unpadded or padded 2-fold as A x B x R samples
    // where the factor chooser finds legs for it (zfft_core.h mixed_choose; up to 8192 samples, one rank) - 729 =
    // 9 x 9 x 9 too, which the 256 R3 scheme has no place for; where it finds none, what follows is what
    // 'fft-streamed' does
    if (pl.method == ML_METHOD_FFT_MIXED && N_plain > 0 && N_plain % 256 != 0 && ctx->n_ranks == 1) {
        const int N = N_plain;
        const zf::MixChoice ch = zf::mixed_choose(N, m);
        if (ch.s) {
            ML_TRY(ax.tw.reserve((size_t)ch.A * ch.B * 2 * sizeof(double)));
            ML_TRY(ax.wk.reserve((size_t)m * 2 * sizeof(double)));
            ML_TRY(ax.pj.reserve((size_t)m * 2 * sizeof(double)));
            ML_TRY(ax.kbin.reserve((size_t)m * sizeof(int)));
            ProfScope scope(ctx, ML_K_TWIDDLE);
            ML_TRY(zfft_build_tables(ctx->stream, ax.tw.as<double>(), ax.wk.as<double>(), ax.pj.as<double>(),
                                     ax.kbin.as<int>(), m, j0, N * ch.s, n - n / 2, ch.s, ch.A, ch.B));
            ax.pad1 = zfft_choose_pad_mixed(ch.A, ch.B, ch.R, m, j0, ch.s);
            ax.pad2 = 0;
            ax.A = ch.A;
            ax.B = ch.B;
            ax.R = ch.R;
            ax.split = 1;
            ax.passes = 0;
            ax.N_eff = N * ch.s;
            ax.j0 = j0;
            ax.jstep = ch.s;
            ax.ok = true;
            return ML_OK;
        }
    }
    if (!fits256) return ML_OK;
    // whether this method takes the axis, and in how many sub-sequences or passes: transform_route.h zfft_axis_rule
    const ZfftAxisRule rule = zfft_axis_rule(pl.method, N_eff, jstep, m);
    if (!rule.taken) return ML_OK;
    const int split = rule.split;
    ax.passes = rule.passes;
    ML_TRY(pl.fft_tw1.reserve(256 * 2 * sizeof(double)));
    ML_TRY(ax.wk.reserve((size_t)m * 2 * sizeof(double)));
    ML_TRY(ax.pj.reserve((size_t)split * m * 2 * sizeof(double)));
    ML_TRY(ax.kbin.reserve((size_t)m * sizeof(int)));
    ProfScope scope(ctx, ML_K_TWIDDLE);
    // (tw1 is shared by every axis and every lattice; with split > 1 the per-bin tables belong to the
    // sub-sequences' lattice and pj[i][.] carries sub-sequence i's bins to the full one)
    ML_TRY(zfft_build_tables(ctx->stream, pl.fft_tw1.as<double>(), ax.wk.as<double>(),
                             ax.pj.as<double>(), ax.kbin.as<int>(), m, j0, N_eff, n - n / 2, jstep));
    if (split > 1)
        ML_TRY(zfft_build_interleave_tables(ctx->stream, ax.wk.as<double>(), ax.pj.as<double>(),
                                            ax.kbin.as<int>(), m, j0, N_eff / split, N_eff, n - n / 2, 0, split, jstep));
    zfft_choose_pads(N_eff / split, m, j0, &ax.pad1, &ax.pad2, jstep);
    ax.split = split;
    ax.N_eff = N_eff;
    ax.j0 = j0;
    ax.jstep = jstep;
    ax.ok = true;
    return ML_OK;
}

// Phase tables of the folded stage 2 for the resident rows: local row k pairs with local row nxl-1-k, pair t sits at
// +/-(half_x - row0 - t) dx (farfield.hip stage2_folded).  They do not depend on stage 1's result, so the transform can
// queue them ahead of it.  Returns the split-K factor through *want_split.
int stage2_tables(ml_ctx *ctx, int row0, int mirrored, int *want_split_out) {
    FarfieldPlan &pl = ctx->plan;
    const int nxl = ctx->fields.nx, mx = pl.mx, my = pl.my, S = pl.fold2_S, T = (nxl + 1) / 2;
    // few rows (4*my) and a long reduction: split the pairs over several workgroups per tile
    static const int forced_split2 = diag_int("ML_STAGE2_SPLIT", 0);
    const int want_split = forced_split2 > 0 ? forced_split2 : fold2_want_split(my, S);
    *want_split_out = want_split;
    const long key[4] = {pl.serial, row0, nxl, mirrored};
    if (!plan_cache_disabled() && pl.fold2_for.matches(key)) return ML_OK;
    const int splits = zfold_splits(T, want_split);
    ML_TRY(pl.fold2_ot.reserve((size_t)splits * 4 * my * mx * 2 * sizeof(double)));
    ML_TRY(fold_tables(ctx, pl.fold_x, S, pl.ux, mx, pl.nx_total, pl.dxp, row0, nxl, mirrored));
    pl.fold2_for.set(key);
    return ML_OK;
}

// tw_x: direction-major [mx][nx_total] (A operand of the generic stage 2) for a tensor grid,
// sample-major [nx_total][mx] for a pair list (column dot)
int need_tw_x(ml_ctx *ctx) {
    FarfieldPlan &pl = ctx->plan;
    if (pl.tw_x_ready) return ML_OK;
    if (pl.pair_list)
        ML_TRY(launch_twiddle(ctx, pl.tw_x.as<double>(), pl.nx_total, pl.mx, 1, pl.nx_total, pl.dxp,
                              pl.wavelength, pl.n_glass, pl.ux.as<double>()));
    else
        ML_TRY(launch_twiddle(ctx, pl.tw_x.as<double>(), pl.mx, pl.nx_total, 0, pl.nx_total, pl.dxp,
                              pl.wavelength, pl.n_glass, pl.ux.as<double>()));
    pl.tw_x_ready = true;
    return ML_OK;
}

// called by ml_fields_download: give the host the plain fields
int fields_unmodulate(ml_ctx *ctx) {
    if (ctx->fields.premod_serial < 0) return ML_OK;
    FarfieldPlan &pl = ctx->plan;
    if (ctx->fields.premod_serial != pl.serial) {
        set_error("the resident fields carry the input modulation of an earlier far-field plan and "
                  "cannot be restored");
        return ML_ESTATE;
    }
    const size_t n = (size_t)4 * ctx->fields.n_sets * ctx->fields.nx * ctx->fields.ny;   // every resident set
    hipLaunchKernelGGL(zunmodulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       ctx->stream, ctx->fields.buf.as<double2>(), pl.fold_y.E.as<double2>(), ctx->fields.ny, n);
    ML_HIP(hipGetLastError());
    ctx->fields.premod_serial = -1;
    return ML_OK;
}

}  // namespace ml

using namespace ml;

extern "C" {

int ml_farfield_set_method(ml_ctx *ctx, int method) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(method == ML_METHOD_AUTO || method == ML_METHOD_GEMM || method == ML_METHOD_FFT_STREAMED ||
                   method == ML_METHOD_FFT_MIXED,
               "unknown method %d", method);
    ctx->ff_method = method;
    return ML_OK;
}

int ml_farfield_set_precision(ml_ctx *ctx, int precision) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ML_REQUIRE(precision == ML_PRECISION_F64 || precision == ML_PRECISION_F32_GEMM,
               "unknown precision %d", precision);
    ctx->gemm_f32 = precision == ML_PRECISION_F32_GEMM;
    return ML_OK;
}

int ml_nearfield_premodulate(ml_ctx *ctx, int on) {
    ML_REQUIRE(ctx, "ctx is NULL");
    ctx->premod_enabled = on != 0;
    return ML_OK;
}

int ml_farfield_plan(ml_ctx *ctx, int nx_total, int ny, double dxp, double dyp, double wavelength,
                     double n_glass, const double *ux, int mx, const double *uy, int my,
                     int pair_list) {
    ML_REQUIRE(ctx && ux && uy, "NULL argument");
    ML_REQUIRE(nx_total >= 1 && ny >= 1 && mx >= 1 && my >= 1, "empty plan");
    ML_REQUIRE(!pair_list || mx == my, "a pair list needs len(ux) == len(uy)");
    ML_REQUIRE(wavelength > 0 && n_glass > 0 && dxp != 0 && dyp != 0, "bad geometry");
    ML_HIP(hipSetDevice(ctx->device));
    FarfieldPlan &pl = ctx->plan;
    pl.unfold.pending = false;   // vectors of the previous plan that nobody asked for
    // Same geometry as the active plan (a sweep over sources re-plans every pass): its phase
    // tables depend on nothing else, keep them.  ML_NO_PLAN_CACHE=1 rebuilds them every call.
    // the fp32 GEMM mode is a request for the matrix-core path: it keeps the GEMMs
    const int method = ctx->gemm_f32 ? ML_METHOD_GEMM : ctx->ff_method;
    if (pl.ready && !plan_cache_disabled() && pl.method == method &&
        pl.nx_total == nx_total && pl.ny == ny &&
        pl.mx == mx && pl.my == my && pl.pair_list == pair_list && pl.dxp == dxp &&
        pl.dyp == dyp && pl.wavelength == wavelength && pl.n_glass == n_glass &&
        pl.h_ux.size() == (size_t)mx && pl.h_uy.size() == (size_t)my &&
        memcmp(pl.h_ux.data(), ux, mx * sizeof(double)) == 0 &&
        memcmp(pl.h_uy.data(), uy, my * sizeof(double)) == 0) {
        pl.have_vectors = false;
        pl.amplitudes_reduced = false;
        return ML_OK;
    }
    ML_TRY(comm_join(ctx, true));   // a reduction of the old plan may still use its buffers
    pl.ready = false;
    ++pl.serial;
    pl.have_vectors = false;
    pl.amplitudes_reduced = false;
    pl.nx_total = nx_total;
    pl.ny = ny;
    pl.mx = mx;
    pl.my = my;
    pl.pair_list = pair_list;
    pl.dxp = dxp;
    pl.dyp = dyp;
    pl.wavelength = wavelength;
    pl.n_glass = n_glass;
    pl.method = method;
    ML_TRY(upload_if_changed(ctx, pl.ux, pl.h_ux, ux, mx));
    ML_TRY(upload_if_changed(ctx, pl.uy, pl.h_uy, uy, my));
    ML_TRY(pl.tw_x.reserve((size_t)mx * nx_total * 2 * sizeof(double)));
    const size_t out_elems = pl.directions();
    ML_TRY(pl.vectors.reserve(4 * out_elems * 2 * sizeof(double)));
    ML_TRY(pl.power.reserve(out_elems * sizeof(double)));
    ML_TRY(pl.amplitudes.reserve(2 * 2 * out_elems * 2 * sizeof(double)));   // two slots
    // direction grids on the aperture's FFT lattice: that axis runs as an output-pruned FFT
    pl.fft_y.ok = pl.fft_x.ok = false;
    if (method != ML_METHOD_GEMM && !pair_list) {
        ML_TRY(plan_fft_axis(ctx, pl.fft_y, ny, dyp, uy, my));
        ML_TRY(plan_fft_axis(ctx, pl.fft_x, nx_total, dxp, ux, mx));
    }
    // stage 1 operand otherwise: the folded cos/sin tables when uy is centre-symmetric, else the
    // complex twiddles tw_y[k][j] (sample-major, B operand of the generic GEMM)
    pl.fold = false;
    if (!pl.fft_y.ok) ML_TRY(plan_fold(ctx, uy));
    if (!pl.fold && !pl.fft_y.ok) {
        ML_TRY(pl.tw_y.reserve((size_t)ny * my * 2 * sizeof(double)));
        ML_TRY(launch_twiddle(ctx, pl.tw_y.as<double>(), ny, my, 1, ny, dyp, wavelength, n_glass,
                              pl.uy.as<double>()));
    }
    // the complex x twiddles are only needed by the generic stage 2 / the pair-list column dot;
    // they are built on first use (need_tw_x) after each plan call
    pl.tw_x_ready = false;
    ML_TRY(plan_fold2(ctx, ux));
    pl.ready = true;
    return ML_OK;
}

int ml_farfield_plan_info(ml_ctx *ctx, int *stage1_kernel) {
    ML_REQUIRE(ctx && stage1_kernel, "NULL argument");
    if (!ctx->plan.ready) {
        set_error("ml_farfield_plan has not been called");
        return ML_ESTATE;
    }
    *stage1_kernel = ctx->plan.fft_y.ok ? 2 : ctx->plan.fold ? 1 : 0;
    return ML_OK;
}

int ml_farfield_plan_kernels(ml_ctx *ctx, int *stage1_kernel, int *stage2_kernel) {
    ML_REQUIRE(ctx && stage1_kernel && stage2_kernel, "NULL argument");
    ML_TRY(ml_farfield_plan_info(ctx, stage1_kernel));
    const FarfieldPlan &pl = ctx->plan;
    if (pl.fft_y.ok && pl.fft_y.A) *stage1_kernel = 3;
    *stage2_kernel = (pl.fft_x.ok && !pl.pair_list) ? (pl.fft_x.A ? 3 : 2) : pl.fold2 ? 1 : 0;
    return ML_OK;
}

}  // extern "C"
