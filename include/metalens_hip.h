/*
 * metalens_hip.h - C ABI of libmetalens_hip.so, the MI355X (gfx950) implementation of
 * the metalens near-field synthesis + near-to-far-field hot path.
 *
 * The reference (sbyrnes321/metalens) has no FFI or plugin interface for this path
 * (SURVEY.md D6): the boundary is three plain Python functions working on NumPy arrays
 * and duck-typed table objects.  The entry points below are therefore what a ctypes
 * binding of those functions needs - each one cites the reference lines it replaces -
 * and INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative ML_E* code on failure;
 *     ml_last_error() gives the message of the calling thread's last failure;
 *   - all pointers are HOST pointers owned by the caller unless a name ends in _dev;
 *     complex arrays are interleaved (re, im) float64 pairs = numpy complex128;
 *   - 2-D arrays are C-ordered [nx][ny] with y fastest, as numpy.meshgrid(indexing='ij')
 *     gives in the reference (nearfield.py:117);
 *   - one ml_ctx per GPU and per host thread; calls on one context are stream-ordered
 *     on the context's own HIP stream and return after the work is complete unless the
 *     function is documented as asynchronous.
 */
#ifndef METALENS_HIP_H
#define METALENS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ML_ABI_VERSION 1

enum {
    ML_OK = 0,
    ML_EINVAL = -1,   /* bad argument (shape, null pointer, order of calls)          */
    ML_EHIP = -2,     /* a HIP runtime call failed; message carries hipGetErrorString */
    ML_ENOMEM = -3,   /* device allocation failed                                     */
    ML_ESTATE = -4,   /* required upload / plan missing                               */
    ML_ERCCL = -5     /* RCCL failure or librccl not loadable                         */
};

typedef struct ml_ctx ml_ctx;

/* ---- context -------------------------------------------------------------------- */
int ml_abi_version(void);
const char *ml_last_error(void);
int ml_device_count(int *count);
int ml_ctx_create(int device, ml_ctx **out);
void ml_ctx_destroy(ml_ctx *ctx);
/* name[] receives the gcnArchName; cu_count / hbm_bytes may be NULL */
int ml_device_info(ml_ctx *ctx, char *name, int name_len, int *cu_count, int64_t *hbm_bytes);

/* Page-locked host memory for arrays that cross PCIe: copies to and from it run at the link's
 * rate (pageable memory is staged at about a fifth of it).  The Python binding gives
 * build_nearfield's output arrays such storage and recycles it when they are garbage-collected. */
int ml_host_alloc(uint64_t bytes, void **ptr);
int ml_host_free(void *ptr);

/* ---- tables: GratingCollection.interpolators / HexGridSet.interpolators ------------
 * Replaces the scipy RegularGridInterpolator objects built by the reference at
 * grating.py:1186-1232 and lens_center.py:188-226 and evaluated at nearfield.py:310-311
 * and :424-425.  slot >= 0 is the index in lens_periphery_summary['gratingcollection_list'],
 * slot == -1 is the HexGridSet of the lens centre.
 *   axis0[n0], axis1[n1], axis2[n2] : ux, uy and grating-period (or cell-index) nodes
 *   orders[n_orders][2]             : (ox, oy), in the order the host wants them summed
 *   order_k[n_orders][2]            : ox*2*pi and oy*2*pi as evaluated by the host
 *   values[n_orders][n0][n1][n2][4] : complex128; last index = (x,ampfy) (x,ampfx)
 *                                     (y,ampfy) (y,ampfx) for incident polarisation x|y
 *   bounds[6]                       : interpolator_bounds (only [0..3] used for slot -1)
 *   center_periods[2]               : slot -1 only: grating_list[0].grating_period,
 *                                     .lateral_period (nearfield.py:391-392)            */
int ml_upload_table(ml_ctx *ctx, int slot,
                    const double *axis0, int n0, const double *axis1, int n1,
                    const double *axis2, int n2,
                    const int32_t *orders, const double *order_k, int n_orders,
                    const double *values, const double *bounds, const double *center_periods);

/* ---- layout: lens_periphery_summary + lens_center_summary --------------------------
 * Replaces the per-call geometry set-up of nearfield.py:87-94,125-128,148-167,363-367.
 *   ring_boundaries[n_rings+1] = hstack(r_min_list, r_max_list[-1])  (nearfield.py:125)
 *   ring_r_center, ring_period, ring_dphi (= 2*pi/num_around_circle), ring_lateral
 *   (= r_center * dphi), all [n_rings] float64 evaluated by the host in the reference's
 *   operation order; ring_gc[n_rings] = gratingcollection_index_here_list.
 *   cells[n_cells][3] = lens_center_summary rows (x, y, index into the HexGridSet).
 *   rot_table[rot_len][2]: (cos, sin) of every possible grating rotation
 *   sector*dphi (nearfield.py:169-171), evaluated by the HOST's NumPy so that the
 *   rotation enters the large phases bit-identically to the reference on that host;
 *   ring_rot_center[r] is the table index of sector 0 for ring r and ring_rot_half[r]
 *   the largest |sector| tabulated (entries run from sector -half-1 to +half).
 *   tie_table[rot_len][6]: for the sector boundary (k + 1/2)*dphi stored at the index of
 *   sector k: the angle, its cosine and its sine, each as (hi, lo) float64 pairs from an
 *   extended-precision evaluation; used to settle round(arctan2(y,x)/dphi) for samples
 *   that sit within 1e-9 of a tie (samples on the diagonals of a symmetric grid).
 * Limits (ML_EINVAL beyond them): fewer than 2^19 rings; the rings may use at most 16 different
 * grating collections (slots 0 ... 31); cells[.][2], the HexGridSet index, in 0 ... 2047.      */
int ml_upload_layout(ml_ctx *ctx, int n_rings, const double *ring_boundaries,
                     const double *ring_r_center, const double *ring_period,
                     const double *ring_dphi, const double *ring_lateral,
                     const int32_t *ring_gc, const double *rot_table,
                     const double *tie_table, int rot_len,
                     const int32_t *ring_rot_center, const int32_t *ring_rot_half,
                     int n_cells, const double *cells);

/* ---- near-field synthesis: nearfield.build_nearfield (nearfield.py:66-480) ---------
 * Scalars are evaluated by the host with the reference's own expressions so that they
 * are bit-identical to what the reference would use.  A finite source whose largest
 * distance to a sample of the lens exceeds 1e9 / kvac is refused with ML_EINVAL (the
 * phase arithmetic covers k R <= 1e9); the plane wave has no such limit.               */
typedef struct ml_nearfield_params {
    double source_x, source_y;
    double source_z;          /* < 0; -inf selects the normally incident plane wave     */
    double dz;                /* 0 - source_z                               (:174)      */
    double dz2;               /* dz**2                                      (:175)      */
    double source_z2;         /* source_z**2                                (:340)      */
    double pol[3];            /* unit dipole / field vector for 'x','y','z' (:215)      */
    double kvac, kvac2;       /* 2*pi/wavelength and its square             (:115,279)  */
    double k_glass, k_glass2; /* 2*pi*n_glass/wavelength and its square     (:114,287)  */
    double n_glass;
    double Z0;                /* impedance of free space used by the caller (:221,308)  */
    double H_coef;            /* c0*(2*pi/wavelength)**2*dipole_moment/(4*pi) (:213)    */
    double dipole_moment;     /* plane wave: |E| of the incident wave       (:225-228)  */
    int32_t plane_wave;       /* 1 if source_z == -inf                                  */
    int32_t reserved;
} ml_nearfield_params;

/* Bound-check report, one entry per (slot, order, check) that was violated; the host
 * turns the first one (in the reference's check order) into the reference's ValueError
 * (nearfield.py:294-305,412-419).                                                       */
typedef struct ml_bound_violation {
    int32_t slot;      /* collection index, -1 = centre                                 */
    int32_t order;     /* index into the slot's orders                                  */
    int32_t check;     /* 0 ux<min 1 ux>max 2 uy<min 3 uy>max 4 period<min 5 period>max */
    int32_t reserved;
    double value;      /* extreme offending value                                       */
    double bound;
} ml_bound_violation;

/* Synthesise Ex,Ey,Hx,Hy on the tensor grid x_pts[nx] x y_pts[ny] into the context's
 * resident field set (device memory).  power receives the incident power through the
 * lens (nearfield.py:474-477).  On return *n_violations is the number of entries written
 * to violations[0..max_violations).                                                    */
int ml_nearfield(ml_ctx *ctx, const ml_nearfield_params *p,
                 const double *x_pts, int nx, const double *y_pts, int ny,
                 double *power, ml_bound_violation *violations, int max_violations,
                 int *n_violations);

/* Copy the resident field set to / from host complex128 [nx][ny] arrays.  Any output
 * pointer may be NULL.  ml_fields_upload makes caller-supplied fields resident (for the
 * far-field entry points when the near field was produced elsewhere).                   */
int ml_fields_download(ml_ctx *ctx, double *Ex, double *Ey, double *Hx, double *Hy);
int ml_fields_upload(ml_ctx *ctx, int nx, int ny, const double *Ex, const double *Ey,
                     const double *Hx, const double *Hy);
int ml_fields_shape(ml_ctx *ctx, int *nx, int *ny);

/* ---- far field on the FFT lattice: nearfield_farfield.farfield_from_nearfield_helper
 * (nearfield_farfield.py:77-191).  Inputs are the caller's fft2(fftshift(F)) arrays,
 * ux_list[nx] / uy_list[ny] the un-shifted direction cosines of :35-39; P[nx][ny] is
 * P_here_times_r2_over_uz before the caller's fftshift.                                 */
int ml_farfield_lattice_power(ml_ctx *ctx, int nx, int ny,
                              const double *fftEx, const double *fftEy,
                              const double *fftHx, const double *fftHy,
                              const double *ux_list, const double *uy_list,
                              double dxp, double dyp, double wavelength, double n_glass,
                              double Z0, double *P);

/* ---- far field by direct aperture -> direction summation --------------------------
 * Evaluates N(ux,uy) = dx'dy' sum J exp(-ik(x'ux + y'uy)) (nearfield_farfield.py:111-120)
 * for an arbitrary tensor grid ux[mx] x uy[my] (or a list of mx direction pairs if
 * pair_list != 0, then my must equal mx) as dense complex GEMMs on the fp64 matrix
 * cores, instead of the caller-side fft2(fftshift(F)) of nearfield_farfield.py:18-20.
 *
 * The resident field set is rows [row0, row0+nx_local) of an nx_total x ny aperture
 * (row0 = 0, nx_total = nx_local for a single GPU); sample j of an axis of n samples
 * sits at (j - ceil(n/2)) * step, which is what fftshift + FFT imply on the lattice.
 *
 *   ml_farfield_plan      : set the geometry and directions, build the phase tables.  Called
 *                           again with the arguments of the active plan it keeps that plan
 *                           (tables depend on the geometry only; a sweep over sources
 *                           re-plans every pass); any other argument starts a new plan
 *   ml_farfield_transform : radiation vectors Nx,Ny,Lx,Ly [mx][my] of the resident rows
 *                           (a partial sum when the aperture is sharded); accumulate != 0
 *                           adds to the previous result instead of overwriting
 *   ml_farfield_allreduce : sum the partial radiation vectors over all ranks (RCCL)
 *   ml_farfield_project   : projection + power of :153-189 on the (reduced) vectors
 * Any host output pointer may be NULL.                                                  */
int ml_farfield_plan(ml_ctx *ctx, int nx_total, int ny, double dxp, double dyp,
                     double wavelength, double n_glass,
                     const double *ux, int mx, const double *uy, int my, int pair_list);
int ml_farfield_transform(ml_ctx *ctx, int row0, int accumulate);
/* Same for a MIRRORED shard: the resident rows are [row0, row0+h) followed by
 * [nx_total-row0-h, nx_total-row0), h = resident rows / 2 - the row pairs +/-x' of one rank.
 * Both transform stages then run folded; needs a tensor grid with centre-symmetric ux.      */
int ml_farfield_transform_mirrored(ml_ctx *ctx, int row0, int accumulate);
int ml_farfield_allreduce(ml_ctx *ctx);
/* Multi-GPU shortcut: the projection (nearfield_farfield.py:158-185) is linear up to the two
 * complex amplitudes L_phi + Z N_theta and L_theta - Z N_phi, so instead of summing the four
 * partial radiation vectors over the ranks (ml_farfield_allreduce, 4 complex planes) and then
 * projecting, each rank projects its partial sums, ONE all-reduce sums the 2 amplitude planes,
 * and the power is taken afterwards (asynchronous, on the context's stream).  A following
 * ml_farfield_project[_async] returns these results; the radiation vectors stay local partial
 * sums.  Without a communicator it is the plain projection.                                  */
int ml_farfield_project_reduce(ml_ctx *ctx, double Z0);
int ml_farfield_project(ml_ctx *ctx, double Z0, double *P, double *a_theta, double *a_phi);
int ml_farfield_download(ml_ctx *ctx, double *Nx, double *Ny, double *Lx, double *Ly);
/* which stage-1 kernel the current plan uses: *stage1_kernel = 0 generic complex GEMM (3M),
 * 1 folded even/odd real-kernel GEMM (centre-symmetric uy grid).                          */
int ml_farfield_plan_info(ml_ctx *ctx, int *stage1_kernel);
/* The same for both stages: 0 generic complex GEMM, 1 folded GEMM, 2 output-pruned FFT in LDS
 * (the axis' direction grid is a run of consecutive bins of an FFT lattice of the aperture axis,
 * kappa * step * du = 1 / N with N >= the number of samples - the reference's own far-field grid,
 * nearfield_farfield.py:35-39, any window of it, and finer ones.  N need not be a multiple of 256:
 * the reference's default grids are 2^a 3^b 5^c long, nearfield.py:30-36 - 400, 1920, 2000 ... -
 * and run on the 256 / gcd(N, 256) times finer lattice, the aperture zero-padded, of which every
 * such bin is wanted; lattices of up to 16 x 8192 samples, in interleaved sub-sequences beyond
 * 8192; the GEMMs take over where the odd part of N has no divisor that brings it to <= 32),
 * 3 output-pruned FFT on a mixed-radix lattice (ML_METHOD_FFT_MIXED).                            */
int ml_farfield_plan_kernels(ml_ctx *ctx, int *stage1_kernel, int *stage2_kernel);
/* How ml_farfield_plan chooses: ML_METHOD_AUTO (default) takes the FFT on every axis whose grid
 * sits on a lattice that is a multiple of 64 samples long (padded at most 4-fold) and the GEMMs
 * elsewhere - measured, profiles/r06_padded_fft_sweep.txt: the 2- and 4-fold padded lattices (1920,
 * 3200, 960, 1600 samples) run 1.1 to 5 times faster as FFTs than as folded GEMMs, the 8-fold padded
 * ones (800, 1440, 2400) 0.5 to 1.1 times, the 16- to 128-fold padded ones (400, 2000, 3600, 1000,
 * 250) 0.1 to 0.7 times; ML_METHOD_GEMM always takes the GEMMs (arbitrary grids need them anyway;
 * this makes them testable on lattice grids too).  Takes effect at the next ml_farfield_plan.    */
#define ML_METHOD_AUTO 0
#define ML_METHOD_GEMM 1
/* ML_METHOD_FFT_STREAMED: the FFT on every axis whose grid sits on a lattice, HOWEVER padded, and where
 * both axes run as one-level FFTs stage 1 writes its result transposed for a streaming stage 2
 * whatever the aperture's size (AUTO does so from 96 MiB of geometry records + stage-1 result on:
 * DESIGN.md 4.2)                                                                                  */
#define ML_METHOD_FFT_STREAMED 2
/* ML_METHOD_FFT_MIXED: as ML_METHOD_FFT_STREAMED, except that an axis whose lattice of N samples is NOT
 * a multiple of 256 long runs on that lattice itself, or the twice finer one, factored N s = A x B x R
 * with two legs A, B from {9, 10, 12, 15, 16}, s <= 2 and R <= 32 residues (plan kernel 3), instead of on
 * the 256 / gcd(N, 256) times finer one: the method for the reference's default grids (the smallest
 * 2^a 3^b 5^c at or above a goal, nearfield.py:30-36: 400, 1000, 1440, 2000, 3000, 3600 ...).  A lattice
 * with no such factorisation (4374 = 2 3^7, 6561 = 3^8), one beyond 8192 samples, a multiple of 256 and
 * any axis of a context with more than one rank take exactly what ML_METHOD_FFT_STREAMED takes.        */
#define ML_METHOD_FFT_MIXED 3
int ml_farfield_set_method(ml_ctx *ctx, int method);
/* Arithmetic of the aperture -> direction GEMMs (BASELINE.json: "1e-12 (fp64) / 1e-4 (fp32)",
 * configs[4] "fp32 GEMM-cast MFMA path").  ML_PRECISION_F64 (default): fp64 matrix cores.
 * ML_PRECISION_F32_GEMM: the folded GEMMs of both stages round their operands to fp32 and
 * accumulate in fp32 on v_mfma_f32_16x16x4_f32 (twice the matrix rate); near-field synthesis,
 * phase reduction of the twiddle seeds, storage and the projection stay fp64.  Direction grids
 * that are not centre-symmetric (generic complex GEMM) are always computed in fp64.  The
 * setting belongs to the context and persists across ml_farfield_plan calls.
 * NORMALISATION of the 1e-4: max |dE| <= 1e-4 max |E| over the direction grid (rounding of an
 * N-term fp32 sum is absolute).  It is NOT a pointwise bound: a direction 1000 x dimmer than the peak
 * carries up to ~1e-3 relative at 16384^2 (tests/test_gpu_parity.py POINTWISE holds the measured
 * figures per size); dim side lobes that matter belong to ML_PRECISION_F64 (pointwise 0.7e-12 at
 * 4096^2, 1.6e-12 at 2048^2 against the fp64 oracle).                                         */
#define ML_PRECISION_F64 0
#define ML_PRECISION_F32_GEMM 1
int ml_farfield_set_precision(ml_ctx *ctx, int precision);
/* Opt-in fusion for the GPU-resident pipeline (plan -> synthesis -> transform on one context).
 * A direction grid that is centre-symmetric about u_c != 0 (e.g. the FFT sub-lattice, bins
 * -M/2 .. M/2-1) needs the input modulation exp(-i kappa y' u_c) in front of stage 1, which
 * costs that kernel ~11 %.  With this on, ml_nearfield[_async] multiplies it into the sample's
 * propagation phasor (one more phasor product per sample, no extra pass) whenever a folded
 * plan with the same ny is active, and the transform skips it.  The resident fields are then
 * F[i][j] * E[j]; ml_fields_download undoes that first, so the host always sees the plain near
 * field.  Re-planning between synthesis and transform makes the transform fail with
 * ML_ESTATE instead of computing with the wrong modulation.  Default off.                    */
int ml_nearfield_premodulate(ml_ctx *ctx, int on);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI -----------------------------------
 * ml_comm_unique_id fills id[128] on rank 0; the host passes it to the other ranks by
 * any side channel; every rank then calls ml_comm_init.  ml_comm_allreduce is exposed
 * for the benchmark's barrier / max-over-ranks timing (op: 0 sum, 1 max).               */
int ml_comm_unique_id(uint8_t id[128]);
int ml_comm_init(ml_ctx *ctx, const uint8_t id[128], int n_ranks, int rank);
int ml_comm_allreduce_host(ml_ctx *ctx, double *values, int count, int op);
int ml_comm_barrier(ml_ctx *ctx);
/* ranks of the communicator as the backend itself reports them (RCCL: ncclCommCount), this rank,
 * and the backend: 0 none (single process), 1 RCCL, 2 the file communicator of the tests          */
int ml_comm_info(ml_ctx *ctx, int *n_ranks, int *rank, int *backend);
/* How ml_farfield_project_reduce sums the ranks' amplitudes.  ML_REDUCE_SCATTER (default): a
 * reduce-scatter over blocks of direction rows - rank r ends up with the sum of block r and takes the
 * power of that block; (G - 1) / G of the payload crosses the links per rank, half of what an
 * all-reduce moves; ml_farfield_gather completes every rank's picture when the host wants the
 * whole map.  ML_REDUCE_ALL: the all-reduce (every rank holds everything after every step); also
 * what runs when the direction rows do not divide by the rank count.                              */
#define ML_REDUCE_SCATTER 0
#define ML_REDUCE_ALL 1
int ml_comm_set_reduce(ml_ctx *ctx, int mode);
/* Channels (workgroups) RCCL may use for this context's collectives: the step's one collective moves a
 * few MB beside the next step's synthesis, and every CU it occupies is one the synthesis loses.  Set
 * BEFORE ml_comm_init; applies to the communicator that call creates and to nothing else
 * (ncclConfig_t::maxCTAs through ncclCommInitRankConfig - the process environment is not touched, so
 * other RCCL users in the process keep their own settings; an RCCL without that entry point runs
 * uncapped).  Default 4; 0 = leave the choice to RCCL.                                              */
int ml_comm_set_max_channels(ml_ctx *ctx, int channels);
/* all-gather of the reduced amplitude blocks and power rows (collective: every rank calls it);
 * a no-op when every rank already holds everything                                                */
int ml_farfield_gather(ml_ctx *ctx);

/* ---- measurement -----------------------------------------------------------------------
 * Per-kernel HIP-event timing on the context's stream.  Kernel ids: */
enum {
    ML_K_NEARFIELD = 0,
    ML_K_TWIDDLE = 1,
    ML_K_ZGEMM_STAGE1 = 2,
    ML_K_ZGEMM_STAGE2 = 3,
    ML_K_PROJECT = 4,
    ML_K_LATTICE_POWER = 5,
    ML_K_COLDOT = 6,
    /* multi-GPU steps (ml_farfield_project_reduce): what the main stream waits for a reduction
     * that still holds the amplitude slot it wants, and the collective itself on its own stream */
    ML_K_COMM_WAIT = 7,
    ML_K_COLLECTIVE = 8,
    ML_K_COUNT = 9
};
int ml_profile_enable(ml_ctx *ctx, int on);
/* which kernels are timed while profiling is on: bit k = kernel id k (default: all).  Every
 * timed launch costs two event records on the stream (~4 us of serialisation per pair on
 * MI355X), so a benchmark that only needs its dominant kernels selects those.               */
int ml_profile_select(ml_ctx *ctx, unsigned mask);
/* time only every `period`-th launch of each selected kernel (default 1 = every launch): the
 * averages are then over a sample of the launches and the instrumentation costs 1/period     */
int ml_profile_sample(ml_ctx *ctx, int period);
int ml_profile_reset(ml_ctx *ctx);
int ml_profile_get(ml_ctx *ctx, int kernel, int64_t *launches, double *total_ms);
/* wait for everything queued on the context's stream */
int ml_sync(ml_ctx *ctx);
/* asynchronous variants used by the benchmark's timed region: queue the same work as
 * ml_nearfield / ml_farfield_transform / ml_farfield_project without host copies or
 * synchronisation (results stay resident; fetch them afterwards).                       */
int ml_nearfield_async(ml_ctx *ctx, const ml_nearfield_params *p,
                       const double *x_pts, int nx, const double *y_pts, int ny);
int ml_farfield_transform_async(ml_ctx *ctx, int row0, int accumulate);
int ml_farfield_transform_mirrored_async(ml_ctx *ctx, int row0, int accumulate);
/* INTERLEAVED row shards (multi-GPU; the aperture sum of nearfield_farfield.py:
 * 111-138 is linear in the rows, so any partition of them is exact).  Rank r of n_ranks holds the
 * rows n = block (n_ranks m + r) + i, i < block: blocks of `block` rows dealt round robin, resident
 * in that order.  With the rows dealt this way a rank's partial sum along x is `block` short DFTs of
 * nx_total / (block n_ranks) samples on the plan's own bins (decimation in time), so the column pass
 * costs every rank 1 / n_ranks of the whole aperture's - a contiguous or mirrored block of rows
 * costs each rank the full-length pass - and the ranks' loads balance by construction (every rank
 * crosses the centre disc and the rim alike).  ml_farfield_interleave_block: the block size for
 * the ACTIVE plan and n_ranks - 8 rows, the synthesis' patch height, wherever nx_total divides by
 * 8 n_ranks and the short transforms fit (they run zero-stuffed below 256 samples) - or 0 if the
 * plan cannot be sharded this way (x axis not on the pruned FFT, nx_total not a multiple of
 * block n_ranks, lattice length / (block n_ranks) times 1, 2, 4 or 8 not a multiple of 256): shard
 * by mirrored or contiguous rows then.  A lattice longer than the aperture (direction grids finer
 * than the aperture's own) is fine: the rows beyond nx_total are zeros that no rank holds.       */
int ml_farfield_interleave_block(ml_ctx *ctx, int n_ranks, int *block);
int ml_farfield_transform_interleaved_async(ml_ctx *ctx, int block, int n_ranks, int rank, int accumulate);
int ml_farfield_project_async(ml_ctx *ctx, double Z0);
/* ---- batched sources --------------------------------------------
 * The reference's use of this path is the INCOHERENT sum over x-, y- and z-polarised dipoles,
 * possibly at several positions or wavelengths (nearfield.py:69-73).  Sources that differ only in
 * polarisation / dipole moment share everything per aperture sample except the two weights the
 * incident H enters with, so ml_nearfield_batch_async synthesises up to three of them in ONE pass
 * over the cached per-sample geometry (p[0..n): same position, wavelength and constants); member m
 * becomes resident field set m.  Members at DIFFERENT positions (a field-of-view sweep; same
 * wavelength, substrate and source kind) are accepted as well: they are synthesised one after the
 * other into their field sets, bit-identical to n single calls, with geometry, lists and tables set
 * up once and the geometry records still cached from member to member.  ml_fields_select picks the set that ml_farfield_transform*,
 * ml_fields_download work on; ml_nearfield_powers returns the incident power of every member.
 * ml_nearfield_async / ml_nearfield are the n = 1 case.                                       */
int ml_nearfield_batch_async(ml_ctx *ctx, const ml_nearfield_params *p, int n, const double *x_pts,
                             int nx, const double *y_pts, int ny);
/* As ml_nearfield_batch_async, but EVERY member goes through the single-source kernels one after the other, also
 * when the members share one position: field set m then has the bits ml_nearfield_async gives for member m alone
 * (members at one position synthesised together share the per-sample evaluation and round differently, by a few
 * 1e-16 of the field's scale - nearfield.py has one source per call, so this is the reference's granularity).
 * keep_powers != 0: a re-synthesis of the batch that is resident (same n, nx, ny; ML_ESTATE otherwise) - the
 * incident powers stay those of the synthesis before, ml_nearfield_powers returns them unchanged.  Used by the
 * image of a sweep (ml_propagate_sets), whose per-source fields are those of the source alone.           */
int ml_nearfield_members_async(ml_ctx *ctx, const ml_nearfield_params *p, int n, const double *x_pts,
                               int nx, const double *y_pts, int ny, int keep_powers);
int ml_fields_select(ml_ctx *ctx, int set);
int ml_nearfield_powers(ml_ctx *ctx, double *power, int n);
/* Sums over the sources of a sweep, kept on the GPU: after ml_farfield_project[_async],
 *   P_sum (+)= weight * P                              (reset != 0 starts a new sum)
 *   slot's total_P = sum of finite P * dux * duy       (nearfield_farfield.py:74)
 *   slot's cone_P  = the same over (ux - cone_ux0)^2 + (uy - cone_uy0)^2 <= cone_u^2  (encircled power)
 * asynchronous; ml_farfield_sums downloads P_sum [mx][my] (or NULL) and the first n_slots pairs.
 * Only P_sum and two scalars per source cross PCIe, whatever the sweep's length.
 * P_sum belongs to the plan it was started on (its direction count, and tensor grid or pair list):
 * ml_farfield_accumulate with reset == 0 is refused with ML_ESTATE when the context has no sums yet
 * (the first call needs reset != 0) or when the active plan's direction count or kind differs, and
 * ml_farfield_sums with P_sum != NULL is refused likewise under such a plan; the slot scalars stay
 * readable (P_sum == NULL).  A refused call leaves the sums as they were.                    */
#define ML_MAX_SWEEP_SLOTS 4096
int ml_farfield_accumulate(ml_ctx *ctx, double weight, double cone_u, double cone_ux0, double cone_uy0,
                           int slot, int reset);
int ml_farfield_sums(ml_ctx *ctx, double *P_sum, double *total_P, double *cone_P, int n_slots);
/* total_P of the CURRENT projection alone (nearfield_farfield.py:74), same fixed-order sum, without
 * touching P_sum or any sweep slot: a one-off far field on a context that is also running a sweep
 * leaves the sweep's sums as they were.  Synchronises.                                          */
int ml_farfield_total_power(ml_ctx *ctx, double *total_P);
/* Beam metrics of a far-field map, reduced on the GPU (csrc/farfield_beam.hip): where the beam points, how wide it is and
 * how much power falls inside n_cones cones - one record per call, queued into a slot of the context, so that a sweep reads
 * a record per source at its end instead of downloading a map per source.  The far-field counterpart of ml_propagate_focus.
 *   source           : 0: the active plan's current projection (after ml_farfield_project[_async]); -1: the P_sum of
 *                      ml_farfield_accumulate as it is stored
 *   centre           : {cx, cy}, direction cosines; NULL: the map's own peak direction, read on the device
 *   cones, n_cones   : 0 <= n_cones <= ML_BEAM_CONES_MAX sines of half-angles, finite, >= 0 and not decreasing
 *   slot             : in [0, ML_MAX_SWEEP_SLOTS); the records are a buffer of their own, not the slots of
 *                      ml_farfield_accumulate, released with the context
 * The map has n directions - mx my of a tensor grid, direction (i, j) at i my + j, or mx of a pair list, i = j - and is NaN
 * outside the unit circle: every sum and the peak run over the finite P only.  With dx = ux[i] - cx, dy = uy[j] - cy and
 * cell = dux duy as ml_farfield_accumulate takes it (the axes' first steps, 1 for an axis of one direction, 1 for a pair
 * list) the terms of a direction are t0 = P cell, t1 = t0 dx, t2 = t0 dy, t3 = t0 (dx dx), t4 = t0 (dy dy), t5 = t0 (dx dy),
 * and it is inside cone c iff dx dx + dy dy <= c c - every operation rounded on its own, what NumPy computes from the same
 * doubles.  A record has ML_BEAM_RECORD doubles, K = n_cones:
 *   [0] peak_P, the largest finite P (NaN if no direction is finite)  [1] its flat index, the lowest of equals (-1 if none)
 *   [2] the number of finite directions  [3 ... 8] sum t0, t1, t2, t3, t4, t5  [9] cx [10] cy, the centre used (NaN if it is
 *   the peak and nothing is finite; the sums are then 0)  [11] K  [12 + r] sum of t0 inside cones[r], r < K; zeros behind K
 * (csrc/farfield_beam.h BEAM_*).  The moments are taken about the centre, so the central second moment of a narrow beam
 * far off axis does not cancel.
 * Order of summation: fp64, no atomics.  Chunks of the map (1024 directions, doubled until there are at most 1024 chunks:
 * of n alone) are reduced by a workgroup each - a lane adds every 256th direction in ascending order, a butterfly over the
 * wave, the four waves in their order -, and a last launch adds the chunks' partials in index order in two levels, tiles of
 * 32 chunks and then the tiles.  Every cone has a sum of its own.  So a record is repeatable bit for bit, does not depend
 * on the slot or on the other cones, and the record of source k of a sweep is that of the same map reduced alone.
 * ML_ESTATE with the wording of ml_farfield_accumulate if nothing is projected or the power map is reduce-scattered and
 * not gathered, and for source = -1 if the context has no sums or they were started on a plan of another direction count or
 * kind; ML_EINVAL with the numbers in ml_last_error for a source other than 0 or -1, a slot out of range, more than 32
 * cones, cones == NULL with n_cones > 0, a cone that is negative, not finite or below the one before it, a centre that is
 * not finite.  A refused call leaves every slot, P_sum, the sweep's scalars and the plan as they were; an accepted one
 * writes its own slot and nothing else of those.  Asynchronous.  Replaces no reference lines (the reference's callers
 * form these from the downloaded P).
 * ml_farfield_beams: records = HOST, [n_slots][ML_BEAM_RECORD], the slots first_slot ... first_slot + n_slots - 1; a slot
 * never written reads zeros.  ML_EINVAL for first_slot outside [0, ML_MAX_SWEEP_SLOTS), n_slots < 0 or first_slot +
 * n_slots > ML_MAX_SWEEP_SLOTS, records == NULL with n_slots > 0.  Synchronises.  Replaces no reference lines.          */
#define ML_BEAM_CONES_MAX 32
#define ML_BEAM_RECORD (12 + ML_BEAM_CONES_MAX)
int ml_farfield_beam(ml_ctx *ctx, int source, const double *centre, const double *cones, int n_cones, int slot);
int ml_farfield_beams(ml_ctx *ctx, int first_slot, int n_slots, double *records);

/* Exact ties of the nearest-cell search.  A centre-region sample that is exactly equidistant
 * from two cells (it sits on a mirror line of the cell lattice: the x = 0 row of a symmetric
 * grid with an odd number of samples) has no defined nearest cell; the reference takes the one
 * scipy's cKDTree.query (nearfield.py:363-364) meets first, which depends on how that tree was
 * built and cannot be restated.  The kernels therefore REPORT such samples (provisionally
 * taking the lowest cell index) and look the answer up in a list the host supplies:
 *   ml_nearfield_ties        : *n_ties = samples the last synthesis could not settle; up to
 *                              max_ids of them (sample id = local row * ny + column) are
 *                              written to sample_ids (at most ML_TIE_CAPACITY are kept)
 *   ml_nearfield_tie_answers : for these sample ids take these cells (row index into
 *                              lens_center_summary, what cKDTree.query returned); replaces the
 *                              previous list, belongs to the current grid and layout and is
 *                              dropped when either changes.  A synthesis run afterwards is exact.
 * metalens_amd/nearfield.py does this round trip (scipy on the host) whenever ties are reported. */
#define ML_TIE_CAPACITY 1048576
int ml_nearfield_ties(ml_ctx *ctx, int64_t *sample_ids, int max_ids, int *n_ties);
int ml_nearfield_tie_answers(ml_ctx *ctx, const int64_t *sample_ids, const int32_t *cell_index, int n);
/* power and bound violations of the LAST synthesis queued on this context (each launch has its
 * own violation record; the incident power is reduced here unless a projection already did) */
int ml_nearfield_result(ml_ctx *ctx, double *power, ml_bound_violation *violations,
                        int max_violations, int *n_violations);

/* Which synthesis kernels the LAST synthesis on this context took (the tables decide; replaces the
 * per-order loops of nearfield.py:263-327 and :390-441 either way):
 *   *family           1: every table in use holds orders (ox, 0), |ox| <= 5 only - what characterize()
 *                        emits for a round lens (grating.lua:417-423) - and the kernels that build an
 *                        order's phasor as E0 X^ox run, each grating collection over its OWN order list;
 *                     0: NO table is of that kind (an order with oy != 0 or |ox| > 5 in each): the general
 *                        kernel, which evaluates every order's phase argument on its own
 *                     2: MIXED - the decision is per table: the samples of the ring collections (and of the
 *                        centre table) whose order sets are simple take the kernels of family 1, the others the
 *                        general kernel, each from the list of the patches that hold its samples
 *                        (characterize() searches (ox, oy) in [-5, 5]^2, grating.lua:406-423: one collection with
 *                        an order (ox, +-1) costs its own samples the general kernel, not the whole lens)
 *   *ring_orders_max  family 1, 2: order slots of the widest SIMPLE ring collection - its lowest to its highest
 *                     order, a hole in the list counted (0 for family 0)
 *   *centre_orders    family 1, 2: order slots of the centre table (0: it is a general one)
 * Any pointer may be NULL.                                                                       */
int ml_nearfield_kernel_info(ml_ctx *ctx, int *family, int *ring_orders_max, int *centre_orders);

/* Which FORM of the family-1 kernels the last synthesis launched (after a batch of members at different
 * positions: for its last member).  Tables of exactly three present order slots on uniform axes, lit by one
 * dipole without premodulation, have fixed-shape kernels for the steady-state launch from the patch lists;
 * their results are bit-identical to the general form's, which takes every other launch - the first
 * synthesis into a buffer, polarisation batches, plane waves, any other table.  METALENS_HIP_FIXED_SYNTH=0
 * in the environment (read once per process) keeps the general form for every call.
 *   *ring_form     the ring samples of collections of up to four order slots: 0 no such launch, 1 general,
 *                  2 fixed-shape
 *   *centre_form   the centre samples, likewise
 * Either pointer may be NULL.                                                                    */
int ml_nearfield_synth_info(ml_ctx *ctx, int *ring_form, int *centre_form);

/* ---- propagation to points at finite distance ---------------------------------------------
 * The field at targets r = (x, y, z), z > 0, behind the aperture plane z = 0: the Stratton-Chu / Franz
 * sum over the equivalent currents of the SELECTED resident field set (ml_fields_select),
 *   E(r) = dx'dy' sum g { i k Z   [a J - b Rhat (Rhat.J)] - c Rhat x M }
 *   H(r) = dx'dy' sum g { i (k/Z) [a M - b Rhat (Rhat.M)] + c Rhat x J }
 *   R = |r - r'|, g = exp(ikR) / (4 pi R), a = 1 + i/(kR) - 1/(kR)^2, b = 1 + 3i/(kR) - 3/(kR)^2, c = ik - 1/R,
 * a direct fp64 pair sum, valid at any distance (the far field of the entries above needs 2 D^2 / lambda,
 * metres for a millimetre lens).  Samples outside the row extents of a synthesised field are skipped;
 * uploaded fields are summed whole.  Bit-for-bit repeatable.  Refused on a context with more than one rank.
 * The propagator owns its targets and result: the far-field plan, the radiation vectors, the sweep sums,
 * the method and the precision of the context are not touched.
 *
 * ml_propagate_plan replaces no reference lines: the reference ends in direction space.  Its
 * convention is the reference's far field's (nearfield_farfield.py:94-101, 183-185): J = (-Hy, Hx),
 * M = (Ey, -Ex), k = 2 pi n_glass / wavelength, Z = Z0 / n_glass, exp(-i omega t).
 *   x0, y0, dxp, dyp : aperture sample [i][j] of the resident field set sits at (x0 + i dxp, y0 + j dyp);
 *                      the shape is the resident set's when ml_propagate runs (ml_fields_shape)
 *   point_list == 0  : targets on the tensor grid x[nx_t] x y[ny_t] in the plane z[0] (nz == 1), C-ordered
 *   point_list != 0  : the nx_t points (x[d], y[d], z[d]) (ny_t == nz == nx_t), e.g. a cut through a focus
 *   want_h == 0      : E only (about 40 % less arithmetic)
 * Every z must be > 0 (ML_EINVAL otherwise).  The phase arithmetic covers k R <= 1e9: a plan whose targets' bounding
 * box and largest z allow a larger k R over the resident aperture is refused with ML_EINVAL (distance, k R and limit in
 * ml_last_error; the previous plan stays as it was), and so is a pass that meets such a shape - by ml_propagate /
 * ml_propagate_sets, for the plans of the ml_propagate_plan_grid* entries below as well.                     */
int ml_propagate_plan(ml_ctx *ctx, double x0, double y0, double dxp, double dyp,
                      double wavelength, double n_glass,
                      const double *x, int nx_t, const double *y, int ny_t, const double *z, int nz,
                      int point_list, int want_h);
/* Queue the sum for the active propagation plan on the context's stream (asynchronous).  Replaces no
 * reference lines; Z0 enters as in nearfield_farfield.py:183-185 (Z = Z0 / n_glass).     */
int ml_propagate(ml_ctx *ctx, double Z0);
/* The result of the last ml_propagate: E, H complex128 [3][targets] (x, y, z components; targets in the
 * plan's order).  H may be NULL, and must be for a plan with want_h == 0.  Synchronises.  Replaces no
 * reference lines (convention: nearfield_farfield.py:94-101, 183-185).                    */
int ml_propagate_download(ml_ctx *ctx, double *E, double *H);
/* Several resident field sets in ONE pass: the sets first_set ... first_set + n_sets - 1 of the last synthesis
 * batch (ml_nearfield_batch_async; 1 <= n_sets <= 3, inside the resident sets) for the active propagation plan,
 * queued on the context's stream.  What depends on the (sample, target) pair alone - R, Rhat, the sincos of k R -
 * is computed once for all sets; the fields of every set have the bits that ml_fields_select(set) + ml_propagate
 * give.  The result is complex128 [n_sets][6 or 3][targets] on the device (ml_propagate_download_set,
 * ml_propagate_accumulate).  Checks as ml_propagate; the selected set (ml_fields_select) is not changed.
 * Replaces no reference lines; Z0 as for ml_propagate.                                     */
int ml_propagate_sets(ml_ctx *ctx, double Z0, int first_set, int n_sets);
/* How many field sets are resident (the members of the last ml_nearfield_batch_async; 1 after a single
 * synthesis or ml_fields_upload): what ml_propagate_sets may range over.  Replaces no reference lines.   */
int ml_fields_sets(ml_ctx *ctx, int *n_sets);
/* E, H of member `set` (0 ... n_sets - 1) of the last ml_propagate_sets, laid out as for
 * ml_propagate_download (which returns member 0).  H may be NULL, and must be for a plan with want_h == 0.
 * Synchronises.  Replaces no reference lines.                                             */
int ml_propagate_download_set(ml_ctx *ctx, int set, double *E, double *H);
/* Image-plane sums kept on the GPU, double [2][targets] of the active propagation plan: with
 *   i_m = (|Ex|^2 + |Ey|^2) + |Ez|^2   and   s_m = 0.5 ((Re Ex Hy* ) - (Re Ey Hx*))   of member m of the last pass,
 *   I += weights[0] i_0 + ... + weights[n - 1] i_(n - 1),   Sz += weights[0] s_0 + ...   (plans with H only):
 * the pass's own sum is formed in member order and then added ONCE to the running sum (reset != 0: to zero, so
 * the sums then hold this pass alone).  n = 1 ... the sets of the last pass.  The first call on a plan needs
 * reset != 0 (ML_ESTATE otherwise); ml_propagate_plan drops results and sums.  Asynchronous, no atomics:
 * repeatable bit for bit.  Replaces no reference lines: the reference sums powers in direction
 * space only (nearfield.py:69-73), this is the same incoherent sum on an image plane.                    */
int ml_propagate_accumulate(ml_ctx *ctx, const double *weights, int n, int reset);
/* The sums of ml_propagate_accumulate: I, Sz double [targets].  Sz may be NULL, and must be for a plan with
 * want_h == 0.  ML_ESTATE if no accumulation has run on the active propagation plan.  Synchronises.
 * Replaces no reference lines.                                                            */
int ml_propagate_sums(ml_ctx *ctx, double *I, double *Sz);
/* Focus metrics of the resident image, reduced on the GPU (csrc/propagate_focus.hip): per plane the peak of |E|^2 and its
 * place, the zeroth to second moments of |E|^2 and of Sz, and the sums of both inside n_radii radii about a centre - what
 * a focusing efficiency, a centroid, a spot size or a depth of focus are made of, without the image crossing PCIe.
 *   source           : >= 0: member `source` of the last pass (ml_propagate: 0), weights I = (|Ex|^2 + |Ey|^2) + |Ez|^2 and
 *                      Sz = 0.5 (Re Ex Hy* - Re Ey Hx*) as ml_propagate_accumulate forms them; -1: the sums of
 *                      ml_propagate_accumulate as they are stored
 *   mx, my, planes   : the targets as `planes` planes of mx x my, target (i, j) of plane p at (p mx + i) my + j; mx my planes
 *                      must be the plan's targets (planes = 1 unless the plan is a stack)
 *   dx, dy           : the targets' pitch, in the unit of the radii
 *   centre           : [planes][2], (ci, cj) in INDEX units, fractions allowed; NULL: every plane's own peak, read on the
 *                      device
 *   radii, n_radii   : 0 <= n_radii <= 32 radii, finite, >= 0 and not decreasing.  Target (i, j) is inside radius R iff
 *                      fx fx + fy fy <= R R with fx = dx (i - ci), fy = dy (j - cj), every operation rounded on its own
 *   records          : HOST, [planes][record_doubles], record_doubles >= 16 + 2 n_radii.  A record, K = n_radii:
 *                      [0] peak_I  [1] peak_index = i my + j, the lowest of equals
 *                      [2 ... 7] sum w, sum w i, sum w j, sum w i^2, sum w j^2, sum w i j with w = I  [8 ... 13] with w = Sz
 *                      [14] ci [15] cj, the centre used  [16 + r] sum of I inside radii[r]  [16 + K + r] sum of Sz inside it
 *                      (csrc/propagate_focus.h FOCUS_*; the Sz entries are 0 for a plan with want_h == 0)
 * ML_ESTATE with the wording of ml_propagate_download if no pass has run on the active plan, with that of
 * ml_propagate_sums if source = -1 and nothing has been accumulated; ML_EINVAL with the numbers in ml_last_error for a
 * member the last pass does not hold, mx my planes != targets, a pitch that is not > 0, more than 32 radii, a radius that
 * is negative, not finite or below the one before it, a centre that is not finite, record_doubles too small.  A
 * refused call leaves result, sums and plan as they were; so does an accepted one.  fp64, no atomics: chunks of a plane
 * are reduced by a workgroup each in a fixed order and added in index order by a second launch; the cut depends on
 * (mx, my) alone, so a record is repeatable bit for bit and plane p of a stack has the record of that plane planned
 * alone.  Synchronises.  Replaces no reference lines; the far-field counterparts are ml_farfield_accumulate and
 * ml_farfield_beam. */
int ml_propagate_focus(ml_ctx *ctx, int source, int mx, int my, int planes, double dx, double dy,
                       const double *centre, const double *radii, int n_radii, double *records, int record_doubles);
/* Stokes records of the resident image, reduced on the GPU (csrc/propagate_stokes.hip): per plane the peak of I = |E|^2 and
 * its place, and the sums of the Stokes parameters and of the longitudinal intensity over the plane and inside n_radii radii
 * about a centre - the polarisation purity of a spot, its cross-polarised share, the |Ez|^2 share of a high-NA focus, the
 * degree of polarisation of an unpolarised emitter's image - without the vector field crossing PCIe.  Per target, every
 * operation rounded on its own, from Ex, Ey, Ez alone (H is never read; plans with and without H are served):
 *     a = Ex.r Ex.r + Ex.i Ex.i,  b = Ey.r Ey.r + Ey.i Ey.i,  Iz = Ez.r Ez.r + Ez.i Ez.i,   S0 = a + b,   S1 = a - b,
 *     S2 = 2 (Ex.r Ey.r + Ex.i Ey.i) = 2 Re(Ex conj Ey),   S3 = 2 (Ex.r Ey.i - Ex.i Ey.r) = 2 Im(conj(Ex) Ey),   I = S0 + Iz
 * (I has the bits of ml_propagate_focus's).  Sign of S3: S3 = +S0 for E proportional to x^ + i y^.  Under the project's
 * exp(-i omega t), for a wave travelling to +z, that is the field rotating counter-clockwise seen looking towards the
 * source (positive helicity).
 *   source           : >= 0: member `source` of the last pass (ml_propagate: 0); -1: the Stokes sums of
 *                      ml_propagate_accumulate_stokes, the stored doubles taken as they are, the peak that of stored
 *                      S0_sum + Iz_sum
 *   mx, my, planes, dx, dy : as for ml_propagate_focus
 *   centre           : [planes][2], (ci, cj) in INDEX units, fractions allowed; may be NULL only when n_radii == 0 (the
 *                      record then names the peak's (i, j) as its centre)
 *   radii, n_radii   : as for ml_propagate_focus, with its membership rule
 *   record           : HOST, [planes][record_doubles], record_doubles >= 9 + 5 n_radii.  A record:
 *                      [0] peak I  [1] its flat index i my + j, the lowest of equals
 *                      [2 + q] the plane's sum of component q = 0 ... 4 for S0, S1, S2, S3, Iz
 *                      [7] ci [8] cj, the centre  [9 + 5 r + q] the sum of component q inside radii[r]
 *                      (csrc/propagate_stokes.h STOKES_*)
 * States and refusals as ml_propagate_focus (ML_ESTATE for source = -1 before ml_propagate_accumulate_stokes), and ML_EINVAL
 * for centre == NULL with n_radii > 0.  Reads the result (or the Stokes sums) and changes neither.  fp64, no atomics, the
 * cut of a plane into chunks and the two launches of ml_propagate_focus: a record is repeatable bit for bit, plane p of a
 * stack has the record of that plane planned alone, and the sum inside a radius does not depend on the other radii of the
 * call.  Synchronises.  Replaces no reference lines. */
int ml_propagate_stokes(ml_ctx *ctx, int source, int mx, int my, int planes, double dx, double dy,
                        const double *centre, const double *radii, int n_radii, double *record, int record_doubles);
/* Stokes maps kept on the GPU, double [5][targets] of the active propagation plan - S0, S1, S2, S3, Iz as
 * ml_propagate_stokes forms them per target: map q += weights[0] S_q of member 0 + ... of the last pass, the pass's own
 * sum formed in member order and then added ONCE to the running sum (reset != 0: to zero), as ml_propagate_accumulate.  The
 * incoherent sum over an unpolarised emitter's dipoles.  The first call on a plan needs reset != 0 (ML_ESTATE otherwise);
 * every ml_propagate_plan* entry drops the maps.  The sums of ml_propagate_accumulate are not touched.  Asynchronous, no
 * atomics.  Replaces no reference lines. */
int ml_propagate_accumulate_stokes(ml_ctx *ctx, const double *weights, int n, int reset);
/* The maps of ml_propagate_accumulate_stokes: out double [5][targets].  ML_ESTATE if none has run on the active
 * propagation plan.  Synchronises.  Replaces no reference lines. */
int ml_propagate_stokes_sums(ml_ctx *ctx, double *out);
/* The transfer function of the resident image, contracted on the GPU (csrc/propagate_otf.hip): per plane and per weight
 * w (0: I = |E|^2, 1: Sz, formed as ml_propagate_focus forms them)
 *     O_w[p][a][b] = sum_i sum_j w(p, i, j) exp(-2 pi i (u[a] i + v[b] j)),   a < nu, b < nv
 * - the Fourier transform of the point-spread function at chosen frequencies, whose modulus over O_w(0, 0) is the
 * modulation transfer function -, without the image crossing PCIe.
 *   source, mx, my, planes : as for ml_propagate_focus; mx, my >= 1, no pitch enters ((i, j) are target indices)
 *   u, nu, v, nv           : 1 <= nu, nv <= ML_OTF_FREQ_MAX frequencies per axis in CYCLES PER TARGET SAMPLE, finite,
 *                            |u|, |v| <= 0.5 (Nyquist included), in any order, repeats allowed
 *   otf                    : HOST, complex128 [planes][2][nu][nv] as (re, im) pairs; the blocks of weight 1 are zeros for
 *                            a plan with want_h == 0
 * The phase 2 pi frac(u i) is formed so that the rounding of u i does not reach it (csrc/propagate_otf.h
 * otf_phase_fraction: an FMA takes the product's rounding error) and the quarter turns come off the fraction exactly, so a
 * phasor at a fraction of 0, +-1/4, +-1/2 is exactly 0 or +-1; each component of a phasor is within 16 x 2^-53 of the exact
 * one.  fp64, no atomics: rows, then columns, each in segments of 32 indices added in ascending order; the order
 * depends on (mx, my) alone, so an entry is repeatable bit for bit, plane p of a stack has the bits of that plane
 * planned alone, and an entry does not depend on nu, nv, the other frequencies or their order.
 * ML_ESTATE with the wording of ml_propagate_download if no pass has run on the active plan, with that of
 * ml_propagate_sums if source = -1 and nothing has been accumulated; ML_EINVAL with the numbers in ml_last_error for a
 * member the last pass does not hold, mx my planes != targets, more than 65535 planes, nu or nv outside [1, 64], a NULL pointer, a frequency
 * that is not finite or beyond +-0.5 (axis, index and value), more than 2^24 = mx nu + my nv tabulated phasors, more than
 * 2^26 = planes mx nv row sums per weight, a context of more than one rank.  A refused call leaves result, sums, plan and
 * focus records as they were; so does an accepted one.  Synchronises.  Replaces no reference lines.  */
#define ML_OTF_FREQ_MAX 64
int ml_propagate_otf(ml_ctx *ctx, int source, int mx, int my, int planes, const double *u, int nu, const double *v,
                     int nv, double *otf);
/* The overlap of the resident image with separable modes, contracted on the GPU (csrc/propagate_modes.hip): per plane and
 * per component F (0: Ex, 1: Ey, 2: Hx, 3: Hy) of one member of the last pass
 *     O_F[p][a][b] = sum_i sum_j conj(mode_x[a][i]) conj(mode_y[b][j]) F(p, i, j),   a < nu, b < nv
 * - the amplitude with which the field enters the mode psi_ab(x, y) = mode_x[a](x) mode_y[b](y): a fibre mode, a Gaussian
 * beam, a Hermite-Gauss order -, without the image crossing PCIe.  The sums of ml_propagate_accumulate carry no phase and
 * have no overlap.  Three entries, on the pattern of ml_farfield_beam / ml_farfield_beams, so that a sweep queues one call per
 * source and reads every slot at its end:
 * ml_propagate_modes_plan: checks, conjugates the tables on the host (a sign: exact), uploads them index-major (Tx[mx][nu],
 * Ty[my][nv]) and reserves the row sums and n_slots output slots of planes 4 nu nv complex each, all of them zeros.
 *   mx, my, planes   : as for ml_propagate_focus; mx my planes must be the plan's targets
 *   mode_x, nu       : HOST, complex128 [nu][mx] as (re, im) pairs, finite; 1 <= nu <= ML_MODES_MAX; likewise mode_y [nv][my].
 *                      In any order, repeats allowed; the arrays are not read after the call returns
 *   n_slots          : 1 <= n_slots <= ML_MAX_SWEEP_SLOTS
 * The tables belong to the active propagation plan: every ml_propagate_plan* entry that plans drops them; a pass
 * (ml_propagate, ml_propagate_sets) does not.  Caps: mx nu + my nv <= 2^24 table entries, planes mx nv <= 2^25 row sums per
 * component, n_slots planes 4 nu nv <= 2^24 output entries, planes <= 65535.  Synchronises.
 * ml_propagate_modes_queue: member source >= 0 of the last pass into slot `slot`: two launches, no synchronisation, no
 * download.  It writes its own slot and nothing else; for a plan with want_h == 0 the blocks of Hx and Hy are zeros.
 * ml_propagate_modes_fetch: out = HOST, complex128 [n_slots][planes][4][nu][nv] as (re, im) pairs, the slots first_slot ...
 * first_slot + n_slots - 1; a slot never written since the plan reads zeros.  Synchronises.
 * fp64, no atomics: rows, then columns, each in segments of 32 indices added in ascending order; a complex product x t is
 * re = x.r t.r - x.i t.i, im = x.r t.i + x.i t.r, every operation rounded on its own.  The order depends on (mx, my) alone,
 * so an entry is repeatable bit for bit, plane p of a stack has the bits of that plane planned alone, and an entry does
 * not depend on nu, nv, the other modes, their order, the slot or the member index; a mode that is 1 at one index and 0
 * elsewhere on either axis returns the field at that target as it is stored (csrc/propagate_modes.h).
 * ML_EINVAL with the numbers in ml_last_error for mx my planes != targets, more than 65535 planes, nu or nv outside
 * [1, 64], a NULL pointer, a table entry that is not finite (axis, mode, index and value), n_slots outside [1,
 * ML_MAX_SWEEP_SLOTS], a total above the caps, a member the last pass does not hold, source < 0, a slot out of the planned
 * range, a context of more than one rank.  ML_ESTATE with the wording of ml_propagate_download if no pass has run on the
 * active plan (queue), with "ml_propagate_modes_plan has not run on the active propagation plan" if no tables are planned
 * on it (queue, fetch).  A refused call leaves result, sums, focus records, transfer function, the slots and the plan as they
 * were; so does an accepted one, apart from its own slot (the plan entry: the tables and all slots).  The one exception: a plan call that fails with ML_ENOMEM
 * or a HIP error while a buffer grows or the tables are uploaded has given up the earlier tables and slots (queue and fetch
 * then answer ML_ESTATE); with buffers that are large enough already nothing is given up before the upload.  Replaces no reference
 * lines; the aperture's counterparts are ml_fields_zones and ml_fields_zernike.  */
#define ML_MODES_MAX 64
int ml_propagate_modes_plan(ml_ctx *ctx, int mx, int my, int planes, const double *mode_x, int nu, const double *mode_y,
                            int nv, int n_slots);
int ml_propagate_modes_queue(ml_ctx *ctx, int source, int slot);
int ml_propagate_modes_fetch(ml_ctx *ctx, int first_slot, int n_slots, double *out);
/* Per-zone power and wavefront overlap of the resident near field, reduced on the GPU (csrc/fields_zones.hip): for every
 * zone of a list of ring edges about a centre - with the edges of a lens layout, zone 0 is the centre and zone z ring
 * z - 1 - and for n_sets field sets in one pass the members, the sums of Sz, |Ex|^2, |Ey|^2 and the overlaps sum Ex conj(w),
 * sum Ey conj(w) with a reference wave w = exp(i phi): which rings lose power or sit off phase, without the fields
 * crossing PCIe.
 *   first_set, n_sets : the resident sets first_set ... first_set + n_sets - 1, 1 <= n_sets <= 3 (a synthesis batch); zone,
 *                       phase and sincos of a sample are computed once for all of them
 *   x2, nx, y2, ny    : X2[i] = (x[i] - xc)^2 and Y2[j] = (y[j] - yc)^2 as the host formed them; nx, ny must be the resident
 *                       shape; finite, >= 0, and y2 must fall to its minimum and rise again (an axis in order)
 *   e2, n_edges       : 1 <= n_edges <= ML_ZONES_EDGES_MAX squared edges, finite, >= 0, not decreasing.  Sample (i, j) has
 *                       r2 = X2[i] + Y2[j] (one rounded addition) and lies in zone searchsorted(e2, r2, side = 'left'): zone 0
 *                       is the disc r2 <= e2[0], zone z the ring e2[z - 1] < r2 <= e2[z], a sample on an edge belongs to
 *                       the inner zone, a sample beyond the last edge to none
 *   ref_mode, ra, rb, ref_c, k : the reference phase from two per-axis arrays [nx], [ny] and two scalars.
 *                       ML_ZONES_REF_PLANE: phi = ra[i] + rb[j] (ref_c and k are not read).  ML_ZONES_REF_FOCUS:
 *                       phi = -sign(ref_c) (k sqrt((ra[i] + rb[j]) + ref_c ref_c)) with ra, rb >= 0 the squared distances to the
 *                       focus per axis, ref_c = zf != 0 its distance behind (> 0) or in front of the aperture, k > 0; the
 *                       square root is correctly rounded.  (cos phi, sin phi) by the Cody-Waite reduction of the propagators
 *   records           : HOST, [n_sets][n_edges][record_doubles], record_doubles >= ML_ZONES_RECORD.  A record:
 *                       [0] the members  [1] sum S, S = 0.5 ((Ex.r Hy.r + Ex.i Hy.i) - (Ey.r Hx.r + Ey.i Hx.i))
 *                       [2] sum Ex.r^2 + Ex.i^2  [3] the same of Ey  [4] [5] Re, Im of sum Cx, Cx = (Ex.r c + Ex.i s,
 *                       Ex.i c - Ex.r s)  [6] [7] the same of Ey - every operation rounded on its own (csrc/fields_zones.h ZONES_*)
 * Undoes ml_nearfield_premodulate first, as ml_fields_download does.  fp64, no atomics.  A wave walks a line of contiguous
 * samples in blocks of 64 and leaves one partial record per run of samples of one zone on one side of the line's vertex; a
 * second launch adds the runs of a zone in the order of (line, side).  The sum of a zone is a fixed tree over the grid
 * positions, of (nx, ny) and the vertex alone, in which the other samples add +0.0: a record is repeatable bit for bit, the
 * record of a set does not depend on the other sets of the call, and the record of zone (e_a, e_b] does not depend on the
 * other edges.  Scratch: at most n_sets nx min(ny + 2, 2 n_edges + 2) 64 bytes, reserved on first use; ML_ENOMEM with the
 * bytes asked for in ml_last_error if the device cannot give them.
 * ML_ESTATE if no field set is resident; ML_EINVAL with the numbers in ml_last_error for a context of more than one rank,
 * n_sets outside [1, 3], sets that are not resident, axes that differ from the resident shape, n_edges outside [1, 4096], an
 * entry of x2, y2, e2 that is negative or not finite, edges that decrease, a y2 with more than one valley, an unknown
 * ref_mode, ra or rb not finite (focus: or negative), ref_c = 0 or k <= 0 for a focus, a reference phase beyond 1e9 rad on
 * the grid (the value is named), record_doubles < 8, a NULL pointer.  A refused call changes nothing.  Synchronises.
 * Replaces no reference lines (phase continuity is "checked by eye").                   */
#define ML_ZONES_EDGES_MAX 4096
#define ML_ZONES_RECORD 8
#define ML_ZONES_REF_PLANE 0
#define ML_ZONES_REF_FOCUS 1
int ml_fields_zones(ml_ctx *ctx, int first_set, int n_sets, const double *x2, int nx, const double *y2, int ny,
                    const double *e2, int n_edges, int ref_mode, const double *ra, const double *rb, double ref_c,
                    double k, double *records, int record_doubles);
/* Per-zone contributions to the field at points behind the aperture (csrc/fields_zone_fields.hip): the direct pair sum of
 * ml_propagate left un-added across the zones of ml_fields_zones.  For every slot z - the n_edges zones and, as slot
 * n_edges, everything beyond the last edge -, every target t and n_sets field sets
 *     E_z(t) = Z k^2 / (4 pi) dx' dy' sum over the samples of slot z of w { i D(J) - (i - q) Rhat x m }
 * and H_z(t) likewise, so that E(t) = sum_z E_z(t): how much each ring adds at a focus and with which phase - the phasor
 * diagram of the focus, the exact re-phasing pupil, the gradient of the focal intensity with respect to every ring's
 * phase - in one pass over the aperture per four targets instead of one pupil and one propagation per zone.
 *   first_set, n_sets : as for ml_fields_zones; the sets are walked one after the other
 *   x0, y0, dxp, dyp, wavelength, n_glass : the aperture, as for ml_propagate_plan: sample [i][j] lies at (x0 + i dxp,
 *                       y0 + j dyp, 0); k = 2 pi n_glass / wavelength, Z = Z0 / n_glass; all finite, all but x0, y0 > 0
 *   x2, nx, y2, ny, e2, n_edges : the zones, as for ml_fields_zones - the same membership to the letter
 *   tx, ty, tz, n_targets : HOST, 1 <= n_targets <= ML_ZONE_FIELDS_TARGETS_MAX points (x, y, z), finite, z > 0
 *   want_h            : 0: E only, 6 doubles per record; else E and H, 12 doubles
 *   records           : HOST, [n_sets][n_edges + 1][n_targets][6 or 12]: Re, Im of Ex, Ey, Ez (then of Hx, Hy, Hz)
 *   samples           : HOST, [n_edges + 1]: the members of every slot
 * A pair's term is formed by the inlined functions of the propagator's kernel in its order (csrc/propagate_pair.h), the
 * currents from the fields as that kernel forms them, and the two scales multiply a finished sum once.  Undoes
 * ml_nearfield_premodulate first, as ml_fields_download does.  fp64, no atomics; the sums run in the order of
 * ml_fields_zones (csrc/fields_zone_fields.h): runs of one slot on one side of a line's vertex, then the runs of a slot
 * over the lines.  A record is repeatable bit for bit and depends neither on the other sets of the call, nor on the other
 * edges, nor on the other targets, and the E records do not depend on want_h.  Scratch: at most
 * nx min(ny + 2, 2 n_edges + 4) (8 + 32 (12 or 6)) bytes whatever n_sets and n_targets are, reserved on first use.  Fields,
 * plans, results and sums of the context are left as they are.
 * ML_ESTATE if no field set is resident; ML_EINVAL with the numbers in ml_last_error for a context of more than one rank,
 * n_sets outside [1, 3], sets that are not resident, axes that differ from the resident shape, n_edges outside [1, 4096],
 * n_targets outside [1, 64], an entry of x2, y2, e2 that is negative or not finite, edges that decrease, a y2 with more than
 * one valley, a target that is not finite or has z <= 0, a geometry that is not finite and > 0, a pair whose k R can
 * exceed 1e9 (the wording of ml_propagate_plan), a NULL pointer.  A refused call changes nothing.  Synchronises.  Replaces
 * no reference lines.                                                                      */
#define ML_ZONE_FIELDS_TARGETS_MAX 64
int ml_fields_zone_fields(ml_ctx *ctx, int first_set, int n_sets, double x0, double y0, double dxp, double dyp,
                          double wavelength, double n_glass, double Z0, const double *x2, int nx, const double *y2, int ny,
                          const double *e2, int n_edges, const double *tx, const double *ty, const double *tz,
                          int n_targets, int want_h, double *records, long long *samples);
/* Zernike moments of the resident near field's wavefront, reduced on the GPU (csrc/fields_wavefront.hip): over a circular
 * pupil of radius R about a centre, and for n_sets field sets in one pass, the members, the sums of Sz, |Ex|^2, |Ey|^2
 * and the complex moments sum Ex conj(w) Z_j, sum Ey conj(w) Z_j of the aperture field against a reference wave
 * w = exp(i phi), for the Zernike terms up to radial order n_max - what the aberrations are (tilt, defocus, astigmatism,
 * coma, spherical ...), without the fields crossing PCIe.
 *   first_set, n_sets : as for ml_fields_zones
 *   x2, xi, nx        : X2[i] = (x[i] - xc)^2 and xi[i] = (x[i] - xc) / R as the host formed them; nx, ny must be the
 *   y2, eta, ny         resident shape; x2, y2 finite and >= 0, xi, eta finite, and y2 must fall to its minimum and rise again
 *   r2                : R R, finite and > 0.  Sample (i, j) is a member iff X2[i] + Y2[j] <= r2 (one rounded addition; a
 *                       sample on the rim is inside): the rule of ml_fields_zones
 *   n_max             : 0 <= n_max <= ML_ZERNIKE_ORDER_MAX.  J = (n_max + 1)(n_max + 2) / 2 terms in OSA/ANSI order,
 *                       j = (n (n + 2) + m) / 2, m = -n, -n + 2, ... n, m < 0 the sine term, Noll-normalised (sqrt(n + 1) for
 *                       m = 0, sqrt(2 (n + 1)) otherwise): (1 / pi) int Z_j Z_k d^2 rho = delta_jk on the unit disc
 *   ref_mode, ra, rb, ref_c, k : the reference phase, as for ml_fields_zones (ML_ZONES_REF_PLANE, ML_ZONES_REF_FOCUS)
 *   records           : HOST, [n_sets][record_doubles], record_doubles >= ML_ZERNIKE_RECORD(n_max) = 4 + 4 J.  A record:
 *                       [0] the members  [1] sum S  [2] sum |Ex|^2  [3] sum |Ey|^2 (the terms of ml_fields_zones), then per
 *                       term j at 4 + 4 j: Re, Im of sum Cx Z_j and Re, Im of sum Cy Z_j, Cx = Ex conj(w), without dA
 * The method fixes the bits (csrc/fields_wavefront.h): Z_j / N_j is a polynomial in (xi, eta) with integer coefficients
 * A_j,pq, so sum C Z_j = N_j sum_pq A_j,pq M_pq with the separable monomial moments M_pq = sum_i xi[i]^p sum_j C(i, j) eta[j]^q.
 * A wave walks a line in blocks of 64 and leaves sum_j C eta^q, q <= n_max, per line; a second launch adds xi^p times the
 * lines' sums in a fixed order; the host adds A M in ascending (p, then q) order and multiplies by N_j.  fp64, no
 * atomics: a record is repeatable bit for bit, does not depend on the other sets of the call, and its terms up to order
 * n' do not depend on n_max >= n'.  Undoes ml_nearfield_premodulate first, as ml_fields_download does.  Scratch:
 * n_sets nx (4 + 4 (n_max + 1)) doubles, reserved on first use.
 * ML_ESTATE if no field set is resident; ML_EINVAL with the numbers in ml_last_error for a context of more than one rank,
 * n_sets outside [1, 3], sets that are not resident, axes that differ from the resident shape, n_max outside [0, 8], r2
 * not finite or <= 0, an entry of x2, y2 that is negative or not finite, of xi, eta that is not finite, a y2 with more
 * than one valley, an unknown ref_mode, ra or rb not finite (focus: or negative), ref_c = 0 or k <= 0 for a focus, a
 * reference phase beyond 1e9 rad on the grid (the value is named), record_doubles < 4 + 4 J, a NULL pointer.  A refused
 * call changes nothing.  Synchronises.  Replaces no reference lines.                         */
#define ML_ZERNIKE_ORDER_MAX 8
#define ML_ZERNIKE_RECORD(n_max) (4 + 2 * ((n_max) + 1) * ((n_max) + 2))
int ml_fields_zernike(ml_ctx *ctx, int first_set, int n_sets, const double *x2, const double *xi, int nx,
                      const double *y2, const double *eta, int ny, double r2, int n_max, int ref_mode, const double *ra,
                      const double *rb, double ref_c, double k, double *records, int record_doubles);
/* A pupil function multiplied into the resident near field where it lies (csrc/fields_pupil.hip): an aperture stop, one
 * complex factor per zone and a Zernike phase plate.  Everything that reads the resident sets afterwards - the transform,
 * ml_propagate*, ml_fields_zones, ml_fields_zernike, a download - sees the modified aperture.  Two entries: the plan
 * checks the call and uploads its arrays once, the pass queues ONE launch and returns.
 * ml_fields_pupil_plan:
 *   x2, xi, nx, y2, eta, ny, r2 : the pupil, as for ml_fields_zernike (the shape is held against the resident sets by the
 *                       pass, not here: a plan does not depend on the fields).  Sample (i, j) has r2' = X2[i] + Y2[j], one
 *                       rounded addition, and is a member iff r2' <= r2; a sample on the rim is inside
 *   stop              : 1: all four fields of a non-member become +0.0 + 0.0i; 0: a non-member takes its zone factor only
 *   n_max, c          : c = NULL for no phase; else J = (n_max + 1)(n_max + 2) / 2 coefficients in radians in the order of
 *                       ml_fields_zernike's terms, 0 <= n_max <= ML_ZERNIKE_ORDER_MAX: a member takes exp(+i psi),
 *                       psi = sum_j c_j Z_j(xi, eta) - the pupil ADDS the aberration c, so c = -wavefront flattens what
 *                       ml_fields_zernike measured.  A non-member takes no phase
 *   e2, n_edges, g    : 0 <= n_edges = K <= ML_ZONES_EDGES_MAX ascending squared edges (NULL for K = 0) and K complex factors
 *                       g[z] = (re, im): a sample in zone z = searchsorted(e2, r2', 'left') < K - the rule of ml_fields_zones -
 *                       takes g[z]; outside every edge, and without edges, the zone factor is exactly 1
 * The values are fixed by the method (csrc/fields_pupil.h): the host forms B_pq = sum_j (c_j N_j) A_j,pq, j ascending onto
 * +0.0, and per line b_q(i) = sum_p B_pq xi^p by Horner, p descending; a member's psi is Horner in eta, q descending;
 * (cs, sn) = sincos_cw(psi); f = g (cs + i sn) = (g.r cs - g.i sn) + i (g.r sn + g.i cs), f = g without a phase; every
 * field becomes (E.r f.r - E.i f.i) + i (E.r f.i + E.i f.r), every operation rounded on its own.  A sample whose factor
 * is exactly 1 - no phase applies to it and no zone factor is given for it - is neither read nor written.
 * ML_EINVAL with the numbers in ml_last_error, before any device work, for a context of more than one rank, stop other than
 * 0 or 1, n_max outside [0, 8], n_edges outside [0, 4096], an empty axis, a NULL pointer, r2 not finite or <= 0, an entry of
 * x2, y2, e2 that is negative or not finite, of xi, eta, c, g that is not finite, a y2 with more than one valley, edges that
 * decrease, sum_pq |B_pq| - what |psi| can reach on the unit disc - beyond 1e9 rad.  A refused call changes nothing.  May
 * synchronise.  The plan stays until the next plan or ml_ctx_destroy.
 * ml_fields_pupil_apply: the planned pupil on the field sets first_set ... first_set + n_sets - 1, 1 <= n_sets <= 3, in one
 * launch; membership, zone, psi and its sincos are computed once per sample for all sets, and every set has the bits of
 * the set taken alone.  Undoes ml_nearfield_premodulate first, as ml_fields_download does.  Queued on the context's stream:
 * no host synchronisation, no download, no atomics.  Afterwards the fields count as supplied by the caller, as after
 * ml_fields_upload.  ML_ESTATE without a plan, without a resident field set, or when the plan's shape is not the resident
 * one; ML_EINVAL for n_sets outside [1, 3], sets that are not resident, a context of more than one rank.  Replaces no
 * reference lines.                                                                     */
int ml_fields_pupil_plan(ml_ctx *ctx, const double *x2, const double *xi, int nx, const double *y2, const double *eta,
                         int ny, double r2, int stop, int n_max, const double *c, const double *e2, int n_edges,
                         const double *g);
int ml_fields_pupil_apply(ml_ctx *ctx, int first_set, int n_sets);

/* The same fields for a tensor grid of targets ON THE APERTURE'S PITCH, by FFT convolution
 * (csrc/propagate_grid_plan.hip; the pass: csrc/propagate_grid.hip): targets (tx0 + i dxp, ty0 + j dyp, z), i < mx, j < my, target t = i my + j; the
 * origin (tx0 - x0, ty0 - y0) is arbitrary.  Every factor of a (sample, target) pair of the direct sum depends on
 * the lag (i_t - i_s, j_t - j_s) alone, so the sum is a discrete convolution of the four currents with eight
 * kernels; it is computed as a zero-padded circular convolution of Lx x Ly points, L = the smallest power of two
 * >= max(16, n + m - 1) per axis - the same sum in another order, not an approximation.  The aperture's shape
 * n is the resident set's when a pass runs (as for ml_propagate_plan): the first pass on a shape reserves the
 * workspace and computes the eight kernel spectra, which are kept until the plan is dropped or the shape changes.
 * L > 8192 is refused with ML_EINVAL: by this call if a field set is resident - n is then that set's shape, so
 * upload or synthesise the field first - and the previous plan stays as it was; by the pass otherwise, and
 * whenever a pass meets another shape.  The other arguments and checks as for ml_propagate_plan, which this call
 * replaces as the active plan: it drops results and sums, and ml_propagate, ml_propagate_sets,
 * ml_propagate_download[_set], ml_propagate_accumulate and ml_propagate_sums serve it with the same layouts and
 * scales.  fp64, no atomics, bit-for-bit repeatable; the sets of a pass run one after another and each has the
 * bits of that set propagated alone.  Replaces no reference lines.                         */
int ml_propagate_plan_grid(ml_ctx *ctx, double x0, double y0, double dxp, double dyp,
                           double wavelength, double n_glass,
                           double tx0, double ty0, int mx, int my, double z, int want_h);
/* ml_propagate_plan_grid with padded axes of up to L = 16384 (arguments, checks, layouts and scales as there; L >
 * 16384 is refused in the same way, with n, m and L in the message): apertures of 4097 ... 8192 samples a side, which
 * ml_propagate_plan_grid can give one target per axis at the most.  An axis of L <= 8192 is transformed as there and
 * the results of a plan both entries accept have the same bits; an axis of L = 16384 takes one streaming pass more
 * per transform (csrc/propagate_grid.h grid_axis_route).  A call of its own because of what it may reserve: the
 * workspace of (12 + 6 or 3) Lx Ly complex128 is up to 77 GB (E only: 64 GB) where ml_propagate_plan_grid never
 * reserves more than 18 GB; the first pass reserves it and fails with ML_ENOMEM and the bytes asked for in
 * ml_last_error if the device cannot give them.  At most 2^26 targets per plan, as there.  ml_propagate_plan_info
 * reports ML_PROPAGATE_FFT_LONG.  Replaces no reference lines.                              */
int ml_propagate_plan_grid_long(ml_ctx *ctx, double x0, double y0, double dxp, double dyp,
                                double wavelength, double n_glass,
                                double tx0, double ty0, int mx, int my, double z, int want_h);
/* ml_propagate_plan_grid by overlap-add over TILES of the aperture, for a small patch of targets behind a large
 * aperture (arguments, checks, layouts and scales as there).  Per axis of n samples and m targets the tile length L is
 * a power of two in [16, 8192] with L >= m; the samples are cut into c = ceil(n / B) tiles of B = L - m + 1, each
 * tile is convolved at the padded length L and the tiles' products are added in the spectral domain, in ascending
 * order of the tile and without atomics, in front of one inverse transform: the padded length of the axis is c L
 * instead of up to 2 n, and n is not bounded by the padding (a 16384^2 aperture has an FFT form).  tile_lx, tile_ly:
 * the tile lengths, 0 for the default - the admissible L that minimises c L times the measured cost of a padded sample
 * at that length (flat up to 512, growing beyond: csrc/propagate_grid.h grid_tile_weight), the larger one of equals.  A
 * length that is no power of two in [16, 8192] or below m, and m > 8192 on an axis, are refused with ML_EINVAL and n, m
 * and the length in ml_last_error; the previous plan stays as it was.  A plan of one tile (the default where a
 * tile of at most 512 holds the axis and shorter tiles would pad it no less) has the bits of ml_propagate_plan_grid.  The first pass on a
 * shape reserves (8 cx cy + 4 batch + 6 or 3) Lx Ly complex128 - every tile's eight kernel spectra are kept for the
 * life of the plan - and fails with ML_ENOMEM and the bytes asked for if the device cannot give them.
 * ml_propagate_plan_info reports ML_PROPAGATE_FFT_TILED and the TILE lengths as lx, ly.
 * Replaces no reference lines.                                                             */
int ml_propagate_plan_grid_tiled(ml_ctx *ctx, double x0, double y0, double dxp, double dyp,
                                 double wavelength, double n_glass,
                                 double tx0, double ty0, int mx, int my, double z, int want_h,
                                 int tile_lx, int tile_ly);
/* The tiles of the active tiled plan: tiles per axis cx, cy, samples per tile bx, by and the tiles that go through
 * the transforms together (batch); zeros while the plan has met no resident field set.  ML_ESTATE unless a tiled,
 * a fine or a stack plan is active.  Any pointer may be NULL.  Replaces no reference lines.        */
int ml_propagate_plan_tiles(ml_ctx *ctx, int *cx, int *cy, int *bx, int *by, int *batch);
/* ml_propagate_plan_grid_tiled for a tensor grid of targets FINER than the aperture's pitch: mx x my targets
 * (tx[0] + i dxp / sx, ty[0] + j dyp / sy, z) with integer ratios sx, sy in [1, 8], target t = i my + j.  Per axis the
 * targets a, a + s, a + 2 s, ... are lattice a, on the aperture's pitch: min(s, m) lattices hold a target, lattice a
 * holds ceil((m - a) / s).  tx_first, ty_first: the first min(sx, mx) and min(sy, my) coordinates of the fine axes, the
 * lattices' origins - strictly ascending and spanning less than the pitch.  Every lattice is the tiled convolution of
 * ml_propagate_plan_grid_tiled with tx0 = tx_first[a], ty0 = ty_first[b] and m_c = ceil(m / s) targets per axis (tile_lx,
 * tile_ly and their default are checked against m_c), and has its bits where it holds m_c targets per axis; the
 * targets of a shorter lattice beyond its own are computed and dropped.  One plan: the currents of a field set are
 * padded and transformed once, tile by tile, and kept for the pass; the lattices are contracted two per read of the
 * currents, transformed back and scattered into the result, which has the layout of every other plan - [6 or 3][mx my],
 * so ml_propagate, ml_propagate_sets, ml_propagate_download[_set], ml_propagate_accumulate and ml_propagate_sums serve
 * it unchanged.  cache_kernels != 0: the kernel spectra of all lattices are filled by the first pass and kept while the
 * plan and the shape stay, a workspace of (8 A tiles + 4 tiles + 2 (6 or 3)) Lx Ly complex128 with A the lattices;
 * cache_kernels == 0: those of two lattices and one batch of tiles are filled and transformed in every pass,
 * (16 batch + 4 tiles + 2 (6 or 3)) Lx Ly complex128; the same bits.  The first pass on a shape reserves the workspace
 * and fails with ML_ENOMEM and the bytes asked for (and, caching, those of cache_kernels == 0) if the device cannot give
 * them.  A ratio outside [1, 8], m_c > 8192, a tile length that is no power of two in [16, 8192] or below m_c, more than
 * 2^26 fine targets, origins that do not ascend or span the pitch, and the refusals of ml_propagate_plan_grid_tiled end
 * in ML_EINVAL with this entry's name in ml_last_error; the previous plan stays as it was.  ml_propagate_plan_info
 * reports ML_PROPAGATE_FFT_FINE and the TILE lengths; ml_propagate_plan_tiles serves this plan too.
 * Replaces no reference lines.                                                             */
int ml_propagate_plan_grid_fine(ml_ctx *ctx, double x0, double y0, double dxp, double dyp,
                                double wavelength, double n_glass,
                                const double *tx_first, int sx, const double *ty_first, int sy,
                                int mx, int my, double z, int want_h, int tile_lx, int tile_ly,
                                int cache_kernels);
/* The lattices of the active fine plan: the ratios sx, sy, the targets per lattice as planned mcx, mcy and whether
 * the kernel spectra are kept (cached).  ML_ESTATE unless a fine or a stack plan is
 * active.  Any pointer may be NULL.
 * Replaces no reference lines.                                                             */
int ml_propagate_plan_lattices(ml_ctx *ctx, int *sx, int *sy, int *mcx, int *mcy, int *cached);
/* ml_propagate_plan_grid_fine for a STACK of nz planes z[0 ... nz - 1]: the mx x my fine targets of that entry in every
 * plane, target t = (p mx + i) my + j, T = nz mx my - a through-focus volume in one plan.  The arguments are those of
 * ml_propagate_plan_grid_fine with `const double *z, int nz` in place of `double z`; the planes may come in any order and
 * repeat.  The fine plan does not depend on z: the currents of a field set are padded and transformed ONCE for all
 * planes, and every (plane, lattice) is one more layer of kernel spectra contracted against them, two per read, in the
 * order l = p A + a Ay + b (A = Ax Ay active lattices; a pair may straddle two planes).  Plane p has the bits of
 * ml_propagate_plan_grid_fine planned at z[p].  The result keeps the layout of every other plan - [6 or 3][T] - so
 * ml_propagate, ml_propagate_sets, ml_propagate_download[_set], ml_propagate_accumulate and ml_propagate_sums serve it
 * unchanged.  cache_kernels != 0: the kernel spectra of all nz A layers are filled by the first pass and kept while the
 * plan and the shape stay, a workspace of (8 nz A tiles + 4 tiles + 2 (6 or 3)) Lx Ly complex128; cache_kernels == 0: those
 * of two layers and one batch of tiles are filled and transformed in every pass, (16 batch + 4 tiles + 2 (6 or 3)) Lx Ly
 * complex128 whatever nz is; the same bits.  The first pass on a shape reserves the workspace and fails with ML_ENOMEM and
 * the bytes asked for (and, caching, those of cache_kernels == 0) if the device cannot give them.  nz outside [1, 4096],
 * nz mx my > 2^26, a z[p] that is not finite or not > 0 (p and the value in the message) and every refusal of
 * ml_propagate_plan_grid_fine end in ML_EINVAL with this entry's name in ml_last_error; the previous plan stays as it
 * was.  k R <= 1e9 is checked with the largest z.  ml_propagate_plan_info reports ML_PROPAGATE_FFT_STACK and the TILE
 * lengths; ml_propagate_plan_tiles and ml_propagate_plan_lattices serve this plan too.
 * Replaces no reference lines.                                                             */
int ml_propagate_plan_grid_stack(ml_ctx *ctx, double x0, double y0, double dxp, double dyp,
                                 double wavelength, double n_glass,
                                 const double *tx_first, int sx, const double *ty_first, int sy,
                                 int mx, int my, const double *z, int nz, int want_h, int tile_lx, int tile_ly,
                                 int cache_kernels);
/* The planes of the active stack plan.  ML_ESTATE unless a stack plan is active.  nz may be NULL.
 * Replaces no reference lines.                                                             */
int ml_propagate_plan_planes(ml_ctx *ctx, int *nz);
#define ML_PROPAGATE_DIRECT 0
#define ML_PROPAGATE_FFT 1
#define ML_PROPAGATE_FFT_LONG 2
#define ML_PROPAGATE_FFT_TILED 3
#define ML_PROPAGATE_FFT_FINE 4
#define ML_PROPAGATE_FFT_STACK 5
/* The active propagation plan: method (ML_PROPAGATE_*), the padded lengths lx, ly (0 for a direct plan, and for
 * an fft plan that has met no resident field set yet; the tile lengths of a tiled or a fine plan) and the bytes of device
 * workspace it holds besides targets,
 * result and sums (direct: the row-set partial sums of the last pass; fft: spectra, currents and outputs, from
 * the first pass on).  ML_ESTATE without a plan.  Any pointer may be NULL.
 * Replaces no reference lines.                                                             */
int ml_propagate_plan_info(ml_ctx *ctx, int *method, int *lx, int *ly, int64_t *workspace_bytes);

/* ---- test surface: the device arithmetic of the hot kernels, one function per lane ----------
 * csrc/nearfield_math.h is inlined into the synthesis and propagation kernels; this entry applies ONE of its
 * functions (or a bare hardware estimate) to n arguments of the caller's, with the library's own compiler flags, so
 * that tests can hold each against an exact reference over its documented range (tests/test_gpu_device_math.py).
 * No product path calls it.  x, kq, out0, out1, outk are HOST arrays of n entries, 1 <= n <= 2^24.
 *   op                    reads        writes
 *   ML_PROBE_SINCOS       x            out0 = sin, out1 = cos          (sincos_cw)
 *   ML_PROBE_SINCOS_Q     x, kq        out0 = sin, out1 = cos of x + kq pi/2   (sincos_cw_q)
 *   ML_PROBE_REDUCE       x            out0 = r, outk = k, x = r + k pi/2      (reduce_pio2)
 *   ML_PROBE_SQRT         x            out0                            (sqrt_exact)
 *   ML_PROBE_RECIP        x            out0                            (recip)
 *   ML_PROBE_RSQRT        x            out0                            (rsqrt_fast)
 *   ML_PROBE_RAW_RCP      x            out0: the hardware's reciprocal estimate alone
 *   ML_PROBE_RAW_RSQ      x            out0: the hardware's reciprocal-root estimate alone
 *   ML_PROBE_OTF_PHASOR   x, kq        out0 = sin, out1 = cos of 2 pi frac(x kq), x = a frequency (|x| <= 0.5), kq = an
 *                                      index >= 0, as the kernels of ml_propagate_otf form them (csrc/propagate_otf.h)
 * (op 8 is reserved.)
 * Pointers an op does not use may be NULL.  An unknown op, a NULL pointer the op needs and n out of range end in
 * ML_EINVAL.  Synchronises.  Replaces no reference lines.                                                  */
#define ML_PROBE_SINCOS 0
#define ML_PROBE_SINCOS_Q 1
#define ML_PROBE_REDUCE 2
#define ML_PROBE_SQRT 3
#define ML_PROBE_RECIP 4
#define ML_PROBE_RSQRT 5
#define ML_PROBE_RAW_RCP 6
#define ML_PROBE_RAW_RSQ 7
#define ML_PROBE_OTF_PHASOR 9
int ml_math_probe(ml_ctx *ctx, int op, const double *x, const int *kq, int n,
                  double *out0, double *out1, int *outk);

/* ---- test surface: the discrete decisions of the synthesis, one point per lane ---------------
 * Which ring a sample lies in, which sector of the ring, which centre cell: sample_geometry (csrc/nearfield_geometry.hip)
 * decides them once per (grid, layout) and every synthesis reuses the records.  This entry runs the same function on n
 * points (x[i], y[i]) of the caller's against the layout now on the context (ml_upload_layout; no tables, grid or source
 * are needed), so that tests can place points on every edge of every decision (tests/test_gpu_geometry_cases.py).
 * No product path calls it.  x, y, ring, pick, path are HOST arrays of n entries, 1 <= n <= 2^20.
 *   ring[i]   0: the centre disc, 1 ... n_rings: a ring, n_rings + 1: outside the lens
 *   pick[i]   ring sample: the sector (round(arctan2(y, x) / dphi) of the ring); centre sample: the ORIGINAL index of the
 *             nearest cell, the lowest among equidistant ones, -1 for a layout without cells; outside: -1
 *   path[i]   the stages that decided, ML_GEO_* below.  Exactly one of the two RING bits is set.
 * The probe keeps tie scratch of its own and takes no tie answers: pending ties, tie answers, geometry records, patch
 * lists and caches of the context stay as they are.  A NULL argument, n out of range and a coordinate that is not
 * finite end in ML_EINVAL, a context without a layout in ML_ESTATE, each with a message and without a launch.
 * Synchronises.  Replaces no reference lines.                                                              */
#define ML_GEO_RING_RECORD 1      /* ring settled by the bucket record (or r beyond the outer radius) */
#define ML_GEO_RING_SEARCH 2      /* ring by the search from the uniform table */
#define ML_GEO_SECTOR_EXACT 4     /* sector: the near-tie recomputation from the extended table was taken */
#define ML_GEO_SECTOR_CLAMPED 8   /* sector: a clamp to the tabulated range acted */
#define ML_GEO_CELL_NODE 16       /* cell accepted from the lattice node the sample is nearest to */
#define ML_GEO_CELL_FOUR 32       /* cell among the four nodes around the sample */
#define ML_GEO_CELL_BINS 64       /* cell from the 3 x 3 bin runs */
#define ML_GEO_CELL_MORE 128      /* ... a run longer than one batch of candidates was finished one by one */
#define ML_GEO_CELL_GROW 256      /* the ring-growing search over the bins was entered */
#define ML_GEO_TIE 512            /* the nearest cell shares its distance with another */
int ml_geometry_probe(ml_ctx *ctx, const double *x, const double *y, int n,
                      int32_t *ring, int32_t *pick, int32_t *path);

#ifdef __cplusplus
}
#endif
#endif /* METALENS_HIP_H */
