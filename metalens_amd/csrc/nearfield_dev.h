// What the near-field synthesis kernels share: the kernel arguments, bound reports, power partials, stores, and the
// launch declarations.  (The decisions of a sample - ring, sector, nearest cell - are nearfield_geometry.hip's.)
#pragma once
#include "nearfield_math.h"

namespace ml {

constexpr int REC_TYPE_SHIFT = 20;   // geometry records: cell type (centre) / collection (rings) above the ring index (rings < 2^19, ctx.hip)
constexpr int MAX_POL = 3;   // members of a polarisation batch (three span every orientation)

struct NfArgs {
    ml_nearfield_params p;      // member 0; position, wavelength and constants are the batch's
    // polarisation batch (ml_nearfield_batch_async): unit vector, H_coef and dipole moment of
    // every member; member m writes field set m and power partials [m][n_partials]
    int n_pol, n_partials;
    double pol[MAX_POL][3], hcoef[MAX_POL], dmom[MAX_POL];
    double e_from_h;   // Z0 / (n_glass k_glass): the source-independent part of the E-from-H factors
    // per member, worked out on the host (nearfield_simple.hip):
    //   plane wave (nearfield.py:223-228): incident H along x, y and Ex Hy - Ey Hx, constants of the launch;
    //   dipole: Z0 H_coef^2, the constant of the incident power density Z0 uz |H|^2
    double pw_Hx[MAX_POL], pw_Hy[MAX_POL], pw_power[MAX_POL], pcoef[MAX_POL];
    const double *x_pts, *y_pts;
    int nx, ny;
    // rings
    int n_rings;
    const double *B, *rc, *period, *dphi, *lateral;
    const int *gc, *lut, *rot_center, *rot_half;
    const double2 *rot_table;
    const double *tie_table;   // [rot_len][6]: boundary angle, cos, sin as (hi, lo) pairs
    int lut_buckets;
    double lut_inv_h;
    const RingBucket *lutrec;
    int lutrec_buckets;
    double lutrec_inv_h, r_outer;
    // centre cells
    int n_cells;
    const double *cx, *cy;
    const int *cwhich, *cindex, *bin_start;
    const double2 *cxy;
    const double2 *center_tab;   // centre table re-laid out [order][n0][n1][4][K] (fast kernel)   // (x, y) of the bin-sorted cells, one 16-byte load per candidate
    int bins_x, bins_y;
    // Exact ties of the nearest-cell search (a sample equidistant from two cells: it sits on a
    // mirror line of the lattice, e.g. the x = 0 row of a symmetric grid with an odd sample
    // count).  The reference takes whichever cell scipy's cKDTree meets first, which only scipy
    // can tell: the kernel records such samples (tie_list, up to tie_cap) and, once the host has
    // asked cKDTree about them, finds the answer in the sorted override list.
    int *tie_count;   // samples the geometry kernel could not settle (zeroed before its launch)
    long long *tie_list;
    int tie_cap;
    const long long *ovr_key;   // sorted sample ids (row * ny + column)
    const int *ovr_slot;        // the cell (bin-sorted slot) to take there
    int n_ovr;
    double bx0, by0, bh, inv_bh;   // inv_bh = 1 / bh, rounded (fast kernel's bin lookup)
    // lattice shortcut (lens_pack.h fit_lattice), fast kernel: lat_map == nullptr if the cells are not
    // the nodes of one lattice
    const int *lat_map;            // [lat_na][lat_nb] -> sorted slot or -1
    // the same node map carrying the cell itself: x, y, (which, original index) - one load
    // instead of map -> position -> type; a NaN position marks an empty node
    const CellRec *lat_rec;
    double lat_c0x, lat_c0y, lat_inv[4], lat_accept_r2;
    double lat_g[3], lat_guard;    // metric b1.b1, b1.b2, b2.b2 and the ambiguity guard (in d^2)
    int lat_amin, lat_bmin, lat_na, lat_nb;
    // tables
    // the centre table's descriptor by value: its fields are then kernel arguments (scalar loads
    // at known offsets) instead of a pointer chase through `tables`
    TableDesc center_desc;
    const TableDesc *tables;
    // per-ring tables for the fast kernel: period axis already interpolated, complex
    // [order][n0][n1][4] per ring at ring_tab + the offset in the ring's record; per-ring order
    // wavenumbers (ox*2*pi/period, oy*2*pi/lateral) at ring_ok + ring_ok_off[ring] (general order sets)
    const double2 *ring_rec;   // [n_rings][2]: (r_center, period), (2 pi / period, bits) - common.h
    const int *ring_coll;      // [n_rings]: dense number of the ring's grating collection
    CollDesc coll[MAX_RING_COLLS];   // in the kernel arguments: read with scalar loads
    const double2 *ring_tab;
    const double *ring_ok;
    const int *ring_ok_off;
    // per-sample geometry records (nearfield_geometry.hip writes, the field kernels read)
    int2 *geo_ix;      // [patch][64]: patch = by * patches_x + bx, 8 x 8 samples each
    // lists of 8 x 8 patches (written behind kernel 1, nearfield_geometry_launch): list k at
    // active_list + k list_stride with n_active[k] entries - 0: patches with a lens sample (general
    // kernels), 1: with a ring sample of a NARROW collection, 2: with a centre sample, 3: with a ring
    // sample of a WIDE collection (nearfield_simple.hip: wide_mask); use_active: the field kernels'
    // grids are the lists instead of all patches
    int2 *active_list;
    int *active_count, *active_flag;
    int list_stride, count_stride;
    int use_active, n_active[4], patches_x;
    // the first synthesis into a buffer runs the ring kernel over the WHOLE grid (it stores the zeros
    // outside the lens and sums every patch's incident power) and the centre kernel from its list with
    // the entry count read on the device (list_count; the host has not seen it yet): first_pass tells
    // the listed centre kernel that the power is not its business this time
    const int *list_count;
    int first_pass;
    // upper bound on the centre list's length the host can give before it has seen the lists: the patches
    // that hold a sample with |x| and |y| within the centre disc's radius (first pass only)
    int centre_patch_bound;
    // every table of the lens holds orders (ox, 0), |ox| <= 5, only: the kernels that build an
    // order's phasor by products run (nearfield_simple.hip), else the general ones
    int simple_orders;
    // simple order sets: bit c = dense collection c holds more than SIMPLE_NARROW_SLOTS orders (its samples are
    // the wide ring instantiation's); narrow_exists: some collection does not
    int wide_mask, narrow_exists;
    int narrow_mask;   // bit c = dense collection c is the narrow instantiation's (simple, at most SIMPLE_NARROW_SLOTS orders)
    // simple_orders and SOME tables are not simple: bit c = the ring samples of dense collection c are the general
    // kernel's (nearfield_general.hip nearfield_field_kernel), centre_general: so are the centre samples; the general kernel
    // then runs from list 0 = the patches that hold such samples (flag bit 4 of the geometry kernel)
    int general_mask, centre_general;
    int narrow_pitch, narrow_cap;   // narrow ring instantiation: complex between staged blocks (16 x its widest collection's orders + 1), blocks per round
    int center_n_slots, center_lo, center_present;   // centre table, simple order sets: as CollDesc::n_slots / ox_lo / present
    // a listed steady-state launch of these arguments takes the fixed-shape kernels of three-order tables: bit 0 the
    // ring launch, bit 1 the centre launch (lens_pack.h fixed3_takes; read by the launch code, not by a kernel)
    int fixed3;
    // the (ux', uy') range every ring table covers (intersection of their bounds: lo0, hi0, lo1, hi1);
    // a sample inside it cannot trip a table bound, and only the others read their ring's own bounds
    double ring_bounds_all[4];
    // outputs
    // outside_is_zero: the samples outside the lens already hold zeros in `fields` (the previous
    // launch wrote them for the same grid, layout and buffer) and are not stored again
    int outside_is_zero;
    double *fields;
    double *partial_power;
    int *row_first;   // per aperture row: smallest min(j, ny-1-j) over samples inside the lens
    unsigned long long *viol;        // keys of this launch
    unsigned long long *viol_next;   // keys of the next launch: cleared by block (0, 0)
    int n_viol_keys;
    // fast kernel, opt-in (ml_nearfield_premodulate): column phasors E[ny] of the active far-field
    // plan; the stored fields are F[i][j] * premod[j], which is what the plan's stage 1 needs
    const double2 *premod;
};
// kernel arguments travel in a 4 KB segment: the patch-list pointer + this
static_assert(sizeof(NfArgs) + 8 <= 4096, "NfArgs no longer fits the kernel-argument segment");

// monotone map double -> uint64 (so that integer max == floating max)
__device__ __forceinline__ unsigned long long ordered_key(double v) {
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}

// Record an out-of-table sample.  Rare path: only violators touch memory.  "min" checks
// store the complemented key so that every slot is a plain atomicMax starting from 0.
__device__ __forceinline__ void report(unsigned long long *viol, int slot, int order, int check,
                                    double v) {
    unsigned long long k = ordered_key(v);
    if ((check & 1) == 0) k = ~k;
    atomicMax(&viol[((size_t)slot * MAX_ORDERS + order) * 6 + check], k);
}

__device__ __forceinline__ void check_bounds(const NfArgs &a, const TableDesc &T, int slot,
                                             int order, double u, double v, double g,
                                             bool with_period) {
    if (u < T.bounds[0]) report(a.viol, slot, order, 0, u);
    if (u > T.bounds[1]) report(a.viol, slot, order, 1, u);
    if (v < T.bounds[2]) report(a.viol, slot, order, 2, v);
    if (v > T.bounds[3]) report(a.viol, slot, order, 3, v);
    if (with_period) {
        if (g < T.bounds[4]) report(a.viol, slot, order, 4, g);
        if (g > T.bounds[5]) report(a.viol, slot, order, 5, g);
    }
}

// incident power: FOUR partials per wave (= per 8 x 8 patch), one per row of sixteen lanes, no
// barrier; fixed order downstream.  The row sums by data-parallel-primitive moves (row_shr 1, 2,
// 4, 8: twelve operations, the sums in lanes 15, 31, 47, 63, which store them side by side) -
// the two row_bcast steps that would make one number of them cost ten operations more per wave
// than the spare block of the projection kernel pays for summing four times as many partials.
__device__ __forceinline__ void wave_power(const NfArgs &a, double power_here, int bx, int by, int member) {
    power_here = dpp_add<0x111, 0xf>(power_here);
    power_here = dpp_add<0x112, 0xf>(power_here);
    power_here = dpp_add<0x114, 0xf>(power_here);
    power_here = dpp_add<0x118, 0xf>(power_here);
    const int lane = threadIdx.x & 63;
    if ((lane & 15) == 15)
        a.partial_power[(size_t)member * a.n_partials + ((size_t)by * a.patches_x + bx) * 4 + (lane >> 4)] = power_here;
    // (workgroup 0 exists in the full and in the listed grid alike; wave 0 of it clears the keys)
    if (blockIdx.x == 0 && blockIdx.y == 0 && member == 0 && threadIdx.x < 64)
        for (int k = threadIdx.x; k < a.n_viol_keys; k += 64) a.viol_next[k] = 0ull;
}

__device__ __forceinline__ void store_fields(const NfArgs &a, int member, int i, int j, c2 Ex, c2 Ey,
                                             c2 Hx, c2 Hy) {
    // 16 B per lane per plane, coalesced along y; field set `member` = 4 planes
    const size_t plane = (size_t)a.nx * a.ny;
    const size_t at = (size_t)i * a.ny + j;
    // streamed (non-temporal): 64 B per sample that this kernel never reads again
    typedef double double2v __attribute__((ext_vector_type(2)));
    double2v *F = reinterpret_cast<double2v *>(a.fields) + (size_t)member * 4 * plane;
    __builtin_nontemporal_store((double2v){Ex.r, Ex.i}, F + at);
    __builtin_nontemporal_store((double2v){Ey.r, Ey.i}, F + plane + at);
    __builtin_nontemporal_store((double2v){Hx.r, Hx.i}, F + 2 * plane + at);
    __builtin_nontemporal_store((double2v){Hy.r, Hy.i}, F + 3 * plane + at);
}

void fill_nf_args(ml_ctx *ctx, const ml_nearfield_params *p, int n, int nx, int ny, NfArgs &a);
// the part of it that states the uploaded LAYOUT (rings, sectors, cells): all that sample_geometry reads
void fill_layout_args(const ml_ctx *ctx, NfArgs &a);
// nearfield_simple.hip: the kernels of a round lens' order sets (orders (ox, 0), |ox| <= 5, per collection)
int nearfield_simple_launch(ml_ctx *ctx, const NfArgs &a);
// nearfield_general.hip: the kernel of any other order set, over `grid` (the whole grid, or a.active_list: list 0)
int nearfield_general_launch(ml_ctx *ctx, const NfArgs &a, dim3 grid);
// nearfield_geometry.hip: the source-independent records of the current (grid, layout, tie answers) and the patch lists
int nearfield_geometry_launch(ml_ctx *ctx, const NfArgs &a);

}  // namespace ml
