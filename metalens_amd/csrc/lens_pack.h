// How a lens is laid out for the near-field kernels: table descriptors, per-ring tables and records, the centre
// table's blocks, the ring-search tables, the binned cells and their lattice - each a pure function from plain arrays
// to a struct of vectors and scalars.  ctx.hip validates, calls these, uploads what they return and copies the
// scalars each returns as one small struct (its `facts`); nothing here knows of either.
//
// Host code without HIP types: compiled by hipcc into ctx.hip and by the host compiler into tools/lens_pack.cpp,
// which runs these functions over a file of arrays and writes every buffer and scalar (tests/test_lens_pack.py).
#pragma once
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "metalens_hip.h"

namespace ml {

constexpr int MAX_SLOTS = 32;      // grating collections per lens (+1 centre)
constexpr int MAX_ORDERS = 32;     // diffraction orders per table
constexpr int PACKED_AXIS = 8;     // nodes of an inline (ux or uy) table axis, see TableDesc

// Device-side view of one packed table (GratingCollection or HexGridSet).
struct TableDesc {
    const double *axis0;   // ux nodes [n0]
    const double *axis1;   // uy nodes [n1]
    const double *values;  // complex [n_orders][n0][n1][n2][4]
    const double *order_k; // [n_orders][2]  (ox*2*pi, oy*2*pi)
    int n0, n1, n2, n_orders;
    double bounds[6];
    double center_kx[MAX_ORDERS];  // centre only: ox*2*pi/x_period, per order
    double center_ky[MAX_ORDERS];
    // ... the orders themselves and the two reciprocal-lattice steps 2*pi/x_period, 2*pi/y_period:
    // the field kernel builds an order's phasor as E0 * Ex^ox (* exp(i oy Gy y') when oy != 0)
    int center_ox[MAX_ORDERS], center_oy[MAX_ORDERS];
    double center_g[2];
    // (ux, uy) axes inline for the fast kernel when both have <= PACKED_AXIS nodes: node a for
    // a <= n-2 (+inf beyond, so a running compare never selects a padded node) and
    // 1 / (node[a+1] - node[a]); one round of independent loads instead of a pointer chase
    // followed by a dependent search loop
    int packed;   // 0 no, 1 both axes <= 5 nodes, 2 both <= PACKED_AXIS
    // both axes uniformly spaced to a few ulp (np.linspace, what characterize() produces): the
    // cell is floor((x - first) / step); uni_ax = {first0, step0, 1/step0, first1, step1, 1/step1}
    int uniform;
    double uni_ax[6];
    double ax0[PACKED_AXIS], inv0[PACKED_AXIS], ax1[PACKED_AXIS], inv1[PACKED_AXIS];
};

// What the field kernel needs to know about a periphery sample's RING: 32 bytes per ring
// (ring_rec: two 16-byte loads per lane),
//   r_center, period | 2 pi / period, bits: offset of the ring's table in ring_tab (general order
//   sets: bits 0-39, bit 40 = the period lies outside its table's period range, nearfield.py:302-305)
// SIMPLE order sets (every table of the lens: orders (ox, 0) with |ox| <= 5 - what characterize()
// emits for a round lens, grating.lua:417-423; nearfield_simple.hip): ring_tab holds CELL BLOCKS
// instead, complex [ring][i0 < n0 - 1][i1 < n1 - 1][order slot < n_slots][node 2 x 2][amplitude 4] - the
// 16 n_slots complex a sample in table cell (i0, i1) interpolates from, contiguous, n_slots = the
// orders of the ring's OWN collection, lowest first (CollDesc::ox_lo).  Blocks are
// addressed in UNITS of 16 complex (256 bytes): bits 0-31 of `bits` = the ring's first unit,
// bit 32 = the period flag; the block of cell c starts at unit first + c n_slots.
// and about the ring's GRATING COLLECTION, which almost every wave shares among all its lanes: a
// CollDesc per collection IN USE (dense numbering, dense_collections), held in the kernel arguments
// so that a wave reads it with scalar loads - the geometry records carry the dense number.
// ring_ok holds 4 doubles per order of the ring's table (general order sets only):
//   ox 2 pi / period, oy 2 pi / lateral, ox, oy;  ring_ok_off[ring] = the ring's offset in it.
constexpr int MAX_RING_COLLS = 16;   // grating collections in use by the rings of one lens
constexpr int SIMPLE_MAX_OX = 5;                       // |ox| of a simple order set (grating.lua:417 searches -5 ... 5)
constexpr int SIMPLE_MAX_SLOTS = 2 * SIMPLE_MAX_OX + 1;
constexpr int SIMPLE_NARROW_SLOTS = 4;                 // up to here a collection's blocks are staged whole, six at a fixed pitch (nearfield_simple.hip)
struct CollDesc {
    double uni_ax[6];   // uniform (ux', uy') axes: first, step, 1 / step per axis (flags bit 0)
    int n0, n1, n_orders;
    int flags;          // bit 0 = axes uniform
    // simple order sets (nearfield_simple.hip): the collection's orders are (ox, 0), ox = ox_lo ...
    // ox_lo + n_slots - 1; slot s of a cell block is order ox_lo + s, and `present` bit s says whether
    // the collection's data holds it (a list with holes has all-zero blocks in them; characterize()
    // produces none: the orders that propagate at a direction are a contiguous run)
    double lim0, lim1;  // n0 - 2, n1 - 2: the last table cell per axis
    int n_slots, ox_lo, present, pad;
};
constexpr int UNIT = 16;                               // complex per unit of a cell block: [node 2 x 2][amplitude 4] of one order
// centre table, simple order sets: complex [order slot][i0 < n0 - 1][i1 < n1 - 1][group of 20 types][node 2 x 2][amplitude 4][20]
// - per order, table cell and group of CENTER_GROUP cell types the 16 x 20 complex the samples of that
// cell and group interpolate from, contiguous (5 KiB: five wave-wide loads stage a block); types past
// the table's K are zeros
constexpr int CENTER_GROUP = 20;                       // (the reference's default K, lens_center.py:28)
constexpr int CENTER_BLOCK = 16 * CENTER_GROUP;        // complex per centre block

// One bucket of the fast kernel's ring search: the number of boundaries strictly below the
// bucket's lower edge and the boundaries just around it, so that searchsorted needs ONE load
// (boundaries_below: LUT entry, then two to three dependent boundary loads).
struct RingBucket {
    double bm1, b0, b1;   // B[first - 1] (-inf if none), B[first], B[first + 1] (+inf past the end)
    int first, pad;
};

// a centre cell as the fast kernel's lattice shortcut reads it (nearfield_geometry.hip lattice_pick)
struct CellRec {
    double x, y;          // cell centre (NaN for an empty lattice node)
    int which, index;     // grating type, original index in lens_center_summary
    double pad;
};

// (uploaded as bytes: none of them has padding the compiler could leave unset)
static_assert(sizeof(TableDesc) == 4 * sizeof(void *) + 16 + 48 + MAX_ORDERS * 24 + 16 + 8 + 48 + PACKED_AXIS * 32 &&
                  sizeof(CollDesc) == 96 && sizeof(RingBucket) == 32 && sizeof(CellRec) == 32,
              "a record the kernels read changed its layout");

// The host's copy of one uploaded table (ml_upload_table's arguments).
struct HostTable {
    bool present = false;
    int n0 = 0, n1 = 0, n2 = 0, n_orders = 0;
    std::vector<double> h_axis0, h_axis1, h_axis2;
    std::vector<double> h_order_k;
    std::vector<double> h_values;   // host copy, for the per-ring pre-interpolation
    double bounds[6] = {0, 0, 0, 0, 0, 0};
    double center_periods[2] = {0, 0};
};

// A status of include/metalens_hip.h and the message ml_last_error is to return; ML_OK: none.
struct PackError {
    int code = ML_OK;
    std::string msg;
};
inline PackError pack_error(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return {code, buf};
}
#define ML_PACK_REQUIRE(out, cond, ...)                       \
    do {                                                      \
        if (!(cond)) {                                        \
            (out).err = ml::pack_error(ML_EINVAL, __VA_ARGS__); \
            return out;                                       \
        }                                                     \
    } while (0)

// ---- table descriptors ---------------------------------------------------------------------
inline void inline_axis(const std::vector<double> &axis, double *node, double *inv) {
    const int n = (int)axis.size();
    for (int a = 0; a < PACKED_AXIS; ++a) {
        node[a] = a <= n - 2 ? axis[a] : INFINITY;
        inv[a] = a <= n - 2 ? 1.0 / (axis[a + 1] - axis[a]) : 0.0;
    }
}

inline bool uniform_axis(const std::vector<double> &axis, double *out) {
    const int n = (int)axis.size();
    if (n < 2) return false;
    const double step = (axis[n - 1] - axis[0]) / (n - 1);
    if (!(step > 0)) return false;
    double scale = 0;
    for (double v : axis) scale = std::max(scale, std::fabs(v));
    for (int a = 0; a < n; ++a)
        if (std::fabs(axis[a] - (axis[0] + a * step)) > 4e-15 * std::max(scale, step)) return false;
    out[0] = axis[0];
    out[1] = step;
    out[2] = 1.0 / step;
    return true;
}

// The TableDesc of a table, its four device pointers left null (the caller's to set).
inline TableDesc describe_table(const HostTable &t, bool is_centre) {
    TableDesc d;
    memset(&d, 0, sizeof d);
    d.n0 = t.n0;
    d.n1 = t.n1;
    d.n2 = t.n2;
    d.n_orders = t.n_orders;
    for (int k = 0; k < 6; ++k) d.bounds[k] = t.bounds[k];
    d.packed = (t.n0 < 2 || t.n1 < 2 || t.n0 > PACKED_AXIS || t.n1 > PACKED_AXIS) ? 0
               : (t.n0 <= 5 && t.n1 <= 5) ? 1 : 2;
    if (d.packed) {
        inline_axis(t.h_axis0, d.ax0, d.inv0);
        inline_axis(t.h_axis1, d.ax1, d.inv1);
    }
    d.uniform = uniform_axis(t.h_axis0, d.uni_ax) && uniform_axis(t.h_axis1, d.uni_ax + 3) ? 1 : 0;
    if (is_centre) {
        // nearfield.py:395-396: ox * 2*pi/x_period - a scalar in the reference
        for (int o = 0; o < t.n_orders; ++o) {
            d.center_kx[o] = t.h_order_k[2 * o] / t.center_periods[0];
            d.center_ky[o] = t.h_order_k[2 * o + 1] / t.center_periods[1];
            d.center_ox[o] = (int)std::lrint(t.h_order_k[2 * o] / (2 * M_PI));
            d.center_oy[o] = (int)std::lrint(t.h_order_k[2 * o + 1] / (2 * M_PI));
        }
        d.center_g[0] = 2 * M_PI / t.center_periods[0];
        d.center_g[1] = 2 * M_PI / t.center_periods[1];
    }
    return d;
}

// ---- per-ring tables -----------------------------------------------------------------------
// Location of a period on a table's period axis: scipy's find_indices arithmetic, evaluated once per
// ring instead of once per sample (the period is a per-ring constant, nearfield.py:154).
struct PeriodLocation {
    int i2;
    double t2;
};
inline PeriodLocation period_location(const std::vector<double> &ax, double x) {
    int i = 0;
    for (int a = 1; a < (int)ax.size() - 1; ++a)
        if (ax[a] <= x) i = a;
    return {i, (x - ax[i]) / (ax[i + 1] - ax[i])};
}

// ... of every ring on the period axis of its own table (slots[MAX_SLOTS]: the uploaded ring tables)
struct RingLocations {
    PackError err;
    std::vector<int32_t> i2;
    std::vector<double> t2;
};
inline RingLocations locate_rings(const HostTable *const *slots, const int32_t *ring_gc, const double *period, int n_rings) {
    RingLocations out;
    out.i2.assign(n_rings, 0);
    out.t2.assign(n_rings, 0.0);
    for (int r = 0; r < n_rings; ++r) {
        const int slot = ring_gc[r];
        if (slot < 0 || slot >= MAX_SLOTS || !slots[slot] || !slots[slot]->present) {
            out.err = pack_error(ML_ESTATE, "ring %d uses grating collection %d, which has no uploaded table", r, slot);
            return out;
        }
        const PeriodLocation at = period_location(slots[slot]->h_axis2, period[r]);
        out.i2[r] = at.i2;
        out.t2[r] = at.t2;
    }
    return out;
}

// A lens is SIMPLE when some table it uses - the collections of its rings and, if it has centre
// cells, the centre table - holds orders (ox, 0) with |ox| <= SIMPLE_MAX_OX only.
struct Canon {
    int n = 0, lo = 0, present = 0;   // slots lo ... lo + n - 1; bit s: the data holds order lo + s
    int idx[SIMPLE_MAX_SLOTS];        // slot -> index in the table's own order list, -1: a hole (zeros)
};
inline bool canon_orders(const HostTable &t, Canon &L) {   // false: not a simple order set
    L = Canon();
    int lo = SIMPLE_MAX_OX + 1, hi = -SIMPLE_MAX_OX - 1;
    for (int o = 0; o < t.n_orders; ++o) {
        const long ox = std::lrint(t.h_order_k[2 * o] / (2 * M_PI)), oy = std::lrint(t.h_order_k[2 * o + 1] / (2 * M_PI));
        if (oy != 0 || ox < -SIMPLE_MAX_OX || ox > SIMPLE_MAX_OX) return false;
        lo = std::min(lo, (int)ox);
        hi = std::max(hi, (int)ox);
    }
    L.lo = lo;
    L.n = hi - lo + 1;
    for (int s = 0; s < L.n; ++s) L.idx[s] = -1;
    for (int o = 0; o < t.n_orders; ++o) {
        const int s = (int)std::lrint(t.h_order_k[2 * o] / (2 * M_PI)) - lo;
        if (L.idx[s] >= 0) return false;   // (an order listed twice)
        L.idx[s] = o;
        L.present |= 1 << s;
    }
    // the restricted kernels name an order in a bound report by the number of present slots below it
    // (nearfield_simple.hip report_orders), i.e. they take the table's own list to be ascending in ox - what
    // grating.py:1186-1232 and the packers produce.  A caller of the C ABI that lists them otherwise gets the
    // general kernels, which carry every order's own index.
    for (int s = 0, last = -1; s < L.n; ++s) {
        if (L.idx[s] < 0) continue;
        if (L.idx[s] < last) return false;
        last = L.idx[s];
    }
    return true;
}

// PER TABLE: the collections (and the centre table) whose order sets are simple take the kernels of
// nearfield_simple.hip, the others - an order with oy != 0 (grating.lua:406-423 searches (ox, oy) in [-5, 5]^2), a
// list that is not ascending - the general kernel of nearfield_general.hip, each over the patches that hold its
// samples: one table with an order (ox, +-1) no longer sends the whole lens through the general kernel.
struct LensClass {
    Canon canon[MAX_RING_COLLS], canon_center;
    bool simple_c[MAX_RING_COLLS] = {}, centre_simple = false;
    bool simple = false;                         // some table in use is simple
    int general_mask = 0, centre_general = 0;    // bit c: dense collection c is general; the centre table (both 0 unless `simple`)
    // which ring collections go to the wide instantiation of the ring kernel (nearfield_simple.hip): part of
    // what the patch lists were built for (list_word below, synth_caches.h geometry_key)
    int narrow_mask = 0, wide_mask = 0, narrow_exists = 0, narrow_slots_max = 1;
    // one word of the above for the key of the patch lists; -2: the general kernel alone
    long list_word() const { return simple ? (long)wide_mask | (long)general_mask << 20 | (long)centre_general << 40 : -2; }
    // the lists and what a synthesis leaves outside the lens were made for another assignment of samples to kernels
    bool lists_differ(const LensClass &o) const {
        return simple != o.simple || general_mask != o.general_mask || (simple && centre_general != o.centre_general);
    }
};
// colls[c]: the table of dense collection c; centre: null or not present = none.  force_general sends a lens that
// qualifies through the general kernels, force_general_coll = mask of dense collection numbers, bit 16 = the centre
// table: those only (the diagnostic build's ML_FORCE_GENERAL, ML_FORCE_GENERAL_COLL)
inline LensClass classify_lens(const HostTable *const *colls, int n_colls, const HostTable *centre, bool force_general,
                               int force_general_coll) {
    LensClass K;
    for (int c = 0; c < n_colls; ++c) {
        K.simple_c[c] = canon_orders(*colls[c], K.canon[c]) && !force_general && !((force_general_coll >> c) & 1);
        K.simple = K.simple || K.simple_c[c];
        if (!K.simple_c[c]) K.general_mask |= 1 << c;
    }
    const bool have_centre = centre && centre->present;
    if (have_centre) {
        K.centre_simple = canon_orders(*centre, K.canon_center) && !force_general && !((force_general_coll >> 16) & 1);
        K.simple = K.simple || K.centre_simple;
    }
    K.centre_general = K.simple && have_centre && !K.centre_simple ? 1 : 0;
    if (!K.simple) K.general_mask = 0;   // (the general kernel alone: nothing to tell apart)
    for (int c = 0; c < n_colls; ++c) {
        if (!K.simple_c[c]) continue;
        if (K.canon[c].n > SIMPLE_NARROW_SLOTS) {
            K.wide_mask |= 1 << c;
        } else {
            K.narrow_exists = 1;
            K.narrow_mask |= 1 << c;
            K.narrow_slots_max = std::max(K.narrow_slots_max, K.canon[c].n);
        }
    }
    return K;
}

// The FIXED-SHAPE synthesis kernels (nearfield_simple.hip, FIXED3): the narrow ring instantiation and the centre kernel
// compiled for tables of exactly three present order slots on uniform axes - the three-order tables of SURVEY.md 8(d),
// the outer collections of a real lens - lit by one dipole.  Same arithmetic in the same order as the general
// instantiations, which keep everything else; which one a launch takes is decided here, from facts alone.
struct Fixed3Facts {
    const CollDesc *coll;   // the lens' dense collections (RingTables::coll)
    int narrow_mask;        // LensClass::narrow_mask: the collections of the narrow ring instantiation
    int center_n_slots, center_present, center_uniform;   // centre table: CentreSlots, TableDesc::uniform (0, 0, 0: none)
    // the launch
    int n_pol;              // members of the polarisation batch
    int use_active, first_pass;   // from the patch lists with their lengths known on the host; the first synthesis into a buffer
    int plane_wave, premod;       // the source is a plane wave; the fields are stored premodulated
};
struct Fixed3 {
    bool ring = false, centre = false;   // the ring launch over list 1, the centre launch over list 2
};
// the lens' part: what its tables allow
inline Fixed3 fixed3_lens(const Fixed3Facts &f) {
    Fixed3 t;
    t.ring = f.narrow_mask != 0;
    for (int c = 0; c < MAX_RING_COLLS; ++c)
        if ((f.narrow_mask >> c) & 1)
            t.ring = t.ring && f.coll[c].n_slots == 3 && f.coll[c].present == 7 && (f.coll[c].flags & 1) != 0;
    // (ox_lo may differ between the collections: it stays a wave-uniform scalar of the kernel)
    t.centre = f.center_n_slots == 3 && f.center_present == 7 && f.center_uniform != 0;
    return t;
}
inline Fixed3 fixed3_takes(const Fixed3Facts &f) {
    Fixed3 t = fixed3_lens(f);
    const bool launch = f.n_pol == 1 && f.use_active && !f.first_pass && !f.plane_wave && !f.premod;
    t.ring = t.ring && launch;
    t.centre = t.centre && launch;
    return t;
}
// (three slots per collection: the narrow instantiation's pitch and capacity are then synth_staging.h's
// narrow_pitch(3) = 49 and narrow_cap(49) = 8, asserted where the kernel names them)

// the collections the rings use, numbered densely in slot order: what the geometry records
// carry and the field kernel's CollDesc array is indexed by
struct DenseColls {
    PackError err;
    int n_colls = 0;
    int32_t coll_slot[MAX_RING_COLLS] = {0};   // dense collection number -> slot
    std::vector<int32_t> ring_coll;            // dense collection number per ring
};
inline DenseColls dense_collections(const int32_t *ring_gc, int n_rings) {
    DenseColls out;
    int dense_of[MAX_SLOTS];
    for (int k = 0; k < MAX_SLOTS; ++k) dense_of[k] = -1;
    for (int r = 0; r < n_rings; ++r) {
        ML_PACK_REQUIRE(out, ring_gc[r] >= 0 && ring_gc[r] < MAX_SLOTS, "ring %d uses grating collection %d: 0 ... %d are supported",
                        r, (int)ring_gc[r], MAX_SLOTS - 1);
        dense_of[ring_gc[r]] = 0;
    }
    for (int k = 0; k < MAX_SLOTS; ++k)
        if (dense_of[k] == 0) {
            ML_PACK_REQUIRE(out, out.n_colls < MAX_RING_COLLS, "the rings use more than %d grating collections", MAX_RING_COLLS);
            out.coll_slot[out.n_colls] = k;
            dense_of[k] = out.n_colls++;
        }
    out.ring_coll.resize(n_rings);
    for (int r = 0; r < n_rings; ++r) out.ring_coll[r] = dense_of[ring_gc[r]];
    return out;
}

// the period axis interpolated at a ring's location, v[..., i2] * (1 - t2) + v[..., i2 + 1] * t2, over the four
// complex amplitudes of one table node: lo = the node's amplitudes at i2, those at i2 + 1 follow them
inline void lerp8(const double *lo, double w0, double w1, double *&dst) {
    const double *hi = lo + 8;
    for (int q = 0; q < 8; ++q) *dst++ = lo[q] * w0 + hi[q] * w1;
}

// The fast kernels' per-ring tables with the period axis already interpolated, and the per-ring order wavenumbers
// ox*2*pi/grating_period, oy*2*pi/lateral_period (nearfield.py:268-269: per-sample expressions of per-ring constants).
// One array `tab`, every ring's table in the form of the kernel that takes its collection: cell blocks (above),
// addressed in UNITS of 16 complex, the collection's orders from the lowest ox upwards, or complex
// [order][n0][n1][4], addressed by the element.
struct RingTables {
    PackError err;
    std::vector<double> tab, ok, rec;   // ring_tab, ring_ok, ring_rec (4 doubles per ring)
    std::vector<int32_t> ok_off;
    CollDesc coll[MAX_RING_COLLS] = {};
    double ring_bounds_all[4] = {0, 0, 0, 0};   // intersection of the ring tables' (ux', uy') bounds
};
// the rings of a layout, per ring: dense collection number, grating period, lateral period, centre radius
struct RingInputs {
    int n_rings;
    const int32_t *coll;
    const double *period, *lateral, *rc;
};
// colls[c], desc[c], coll_slot[c]: table, descriptor and slot of dense collection c; at: locate_rings' result
inline RingTables pack_ring_tables(const HostTable *const *colls, const TableDesc *const *desc, const int32_t *coll_slot,
                                   int n_colls, const LensClass &K, const RingInputs &rings, const RingLocations &at) {
    const int n_rings = rings.n_rings;
    const int32_t *ring_coll = rings.coll;
    const double *ring_period = rings.period, *ring_lateral = rings.lateral, *ring_rc = rings.rc;
    RingTables out;
    // at_el counts complex elements of `tab`.
    std::vector<long long> tab_off(n_rings);
    out.ok_off.resize(n_rings);
    size_t at_el = 0, ok_total = 0, simple_units_end = 0;
    for (int r = 0; r < n_rings; ++r) {
        const int c = ring_coll[r];
        const HostTable &t = *colls[c];
        out.ok_off[r] = (int32_t)ok_total;
        if (K.simple_c[c]) {
            at_el = (at_el + UNIT - 1) / UNIT * UNIT;
            tab_off[r] = (long long)(at_el / UNIT);
            at_el += (size_t)std::max(t.n0 - 1, 0) * std::max(t.n1 - 1, 0) * K.canon[c].n * UNIT;
            simple_units_end = at_el / UNIT;
        } else {
            tab_off[r] = (long long)at_el;
            at_el += (size_t)t.n_orders * t.n0 * t.n1 * 4;
        }
        ok_total += (size_t)t.n_orders * 4;
    }
    const size_t tab_total = at_el;
    // (nearfield_simple.hip: a sample's block = the ring's first unit + its cell, a 31-bit key - `blk`, -1 = none -
    // and the cell itself a 24-bit product (i0 (n1 - 1) + i1) n_slots: v_mad_u32_u24 / v_mul_u32_u24)
    if (K.simple) {
        ML_PACK_REQUIRE(out, simple_units_end + SIMPLE_MAX_SLOTS + 1 < (1ull << 31), "ring tables of %zu block units: too large", simple_units_end);
        for (int c = 0; c < n_colls; ++c) {
            if (!K.simple_c[c]) continue;
            const HostTable &t = *colls[c];
            ML_PACK_REQUIRE(out, (long long)std::max(t.n0 - 1, 1) * std::max(t.n1 - 1, 1) * K.canon[c].n < (1ll << 24) && t.n0 < (1 << 12) &&
                                t.n1 < (1 << 12),
                            "table of collection %d is too large for the 24-bit cell arithmetic (%d x %d nodes, %d orders)",
                            coll_slot[c], t.n0, t.n1, K.canon[c].n);
        }
    }
    // (simple: a wave that straddles two collections stages every block at the larger one's size -
    // the tail of the array is padded by a largest block so that the surplus stays inside it)
    out.tab.assign((tab_total + (K.simple ? (size_t)(SIMPLE_MAX_SLOTS + 1) * UNIT : 0)) * 2, 0.0);
    out.ok.resize(ok_total);
    for (int r = 0; r < n_rings; ++r) {
        const HostTable &t = *colls[ring_coll[r]];
        const double w1 = at.t2[r], w0 = 1 - at.t2[r];
        const bool rs = K.simple_c[ring_coll[r]];
        if (rs) {
            const Canon &L = K.canon[ring_coll[r]];
            double *dst = out.tab.data() + (size_t)tab_off[r] * UNIT * 2;
            for (int c0 = 0; c0 < t.n0 - 1; ++c0)
                for (int c1 = 0; c1 < t.n1 - 1; ++c1)
                    for (int oc = 0; oc < L.n; ++oc)
                        for (int nd = 0; nd < 4; ++nd) {
                            const int a = (c0 + (nd >> 1)) * t.n1 + c1 + (nd & 1);
                            if (L.idx[oc] < 0) {   // a hole in the list
                                for (int q = 0; q < 8; ++q) *dst++ = 0.0;
                                continue;
                            }
                            lerp8(t.h_values.data() + ((((size_t)L.idx[oc] * t.n0 * t.n1 + a) * t.n2 + at.i2[r]) * 4) * 2, w0, w1, dst);
                        }
        }
        double *dst = out.tab.data() + (size_t)tab_off[r] * 2;
        for (int o = 0; o < t.n_orders; ++o) {
            for (int a = 0; !rs && a < t.n0 * t.n1; ++a)
                lerp8(t.h_values.data() + ((((size_t)o * t.n0 * t.n1 + a) * t.n2 + at.i2[r]) * 4) * 2, w0, w1, dst);
            out.ok[out.ok_off[r] + 4 * o] = t.h_order_k[2 * o] / ring_period[r];
            out.ok[out.ok_off[r] + 4 * o + 1] = t.h_order_k[2 * o + 1] / ring_lateral[r];
            out.ok[out.ok_off[r] + 4 * o + 2] = std::rint(t.h_order_k[2 * o] / (2 * M_PI));       // ox
            out.ok[out.ok_off[r] + 4 * o + 3] = std::rint(t.h_order_k[2 * o + 1] / (2 * M_PI));   // oy
        }
    }
    // per-ring records and per-collection descriptors (ring_rec, CollDesc above)
    out.rec.assign((size_t)n_rings * 4, 0.0);
    out.ring_bounds_all[0] = out.ring_bounds_all[2] = -INFINITY;
    out.ring_bounds_all[1] = out.ring_bounds_all[3] = INFINITY;
    for (int c = 0; c < n_colls; ++c) {
        const HostTable &t = *colls[c];
        const TableDesc &d = *desc[c];
        // the field kernel addresses a ring's table with 24-bit products (nearfield_general.hip)
        ML_PACK_REQUIRE(out, (long long)t.n0 * t.n1 * 4 < (1ll << 24), "table of collection %d is too large (%d x %d nodes)",
                        coll_slot[c], t.n0, t.n1);
        CollDesc &C = out.coll[c];
        for (int k = 0; k < 6; ++k) C.uni_ax[k] = d.uni_ax[k];
        C.n0 = t.n0;
        C.n1 = t.n1;
        C.n_orders = t.n_orders;
        C.flags = d.uniform ? 1 : 0;
        C.lim0 = t.n0 - 2;
        C.lim1 = t.n1 - 2;
        C.n_slots = K.simple_c[c] ? K.canon[c].n : 0;
        C.ox_lo = K.simple_c[c] ? K.canon[c].lo : 0;
        C.present = K.simple_c[c] ? K.canon[c].present : 0;
        C.pad = 0;
        for (int k = 0; k < 4; k += 2) {   // a NaN bound leaves the range empty: every sample then reads its own
            out.ring_bounds_all[k] = t.bounds[k] >= out.ring_bounds_all[k] ? t.bounds[k]
                                     : t.bounds[k] == t.bounds[k] ? out.ring_bounds_all[k] : INFINITY;
            out.ring_bounds_all[k + 1] = t.bounds[k + 1] <= out.ring_bounds_all[k + 1] ? t.bounds[k + 1]
                                         : t.bounds[k + 1] == t.bounds[k + 1] ? out.ring_bounds_all[k + 1] : -INFINITY;
        }
    }
    ML_PACK_REQUIRE(out, tab_total < (1ull << 40), "ring tables of %zu elements: too large", tab_total);
    for (int r = 0; r < n_rings; ++r) {
        const HostTable &t = *colls[ring_coll[r]];
        double *q = out.rec.data() + (size_t)r * 4;
        q[0] = ring_rc[r];
        q[1] = ring_period[r];
        q[2] = 2 * M_PI / ring_period[r];
        long long bits = tab_off[r];
        // the ring's period outside its table's period range: every evaluated sample of the ring
        // reports (nearfield.py:302-305)
        if (ring_period[r] < t.bounds[4] || ring_period[r] > t.bounds[5])
            bits |= 1ll << (K.simple_c[ring_coll[r]] ? 32 : 40);
        memcpy(q + 3, &bits, 8);
    }
    return out;
}

// centre table for the fast kernel: [order][n0][n1][4][K] instead of [order][n0][n1][K][4],
// so that the K cell types of one amplitude are contiguous (lanes of a wave hold many
// different cell types; this way one load instruction touches 3 cache lines, not 12)
// Simple order sets: CELL BLOCKS (CENTER_BLOCK above) - complex [order slot][i0][i1][group][node 4][amplitude 4][20]:
// the table's orders from the lowest ox upwards, per table cell and group of 20 cell types the 320
// complex its samples interpolate from, contiguous (a hole in the list: zeros).
struct CentreSlots {
    int n_slots = 0, lo = 0, present = 0;   // simple order sets: as CollDesc::n_slots / ox_lo / present
};
struct CentreTable {
    std::vector<double> cq;
    CentreSlots slots;
};
inline CentreTable pack_centre_table(const HostTable &t, bool centre_simple, const Canon &L) {
    CentreTable out;
    if (centre_simple) {
        out.slots = {L.n, L.lo, L.present};
        const int groups = (t.n2 + CENTER_GROUP - 1) / CENTER_GROUP;
        const size_t cells = (size_t)std::max(t.n0 - 1, 0) * std::max(t.n1 - 1, 0);
        out.cq.assign((size_t)L.n * cells * groups * CENTER_BLOCK * 2, 0.0);
        for (int oc = 0; oc < L.n; ++oc) {
            const int o = L.idx[oc];
            if (o < 0) continue;
            for (int c0 = 0; c0 < t.n0 - 1; ++c0)
                for (int c1 = 0; c1 < t.n1 - 1; ++c1)
                    for (int g = 0; g < groups; ++g) {
                        double *blk = out.cq.data() + ((((size_t)oc * cells + (size_t)c0 * (t.n1 - 1) + c1) * groups + g) * CENTER_BLOCK) * 2;
                        for (int nd = 0; nd < 4; ++nd) {
                            const size_t node = ((size_t)o * t.n0 + c0 + (nd >> 1)) * t.n1 + c1 + (nd & 1);
                            for (int q = 0; q < 4; ++q)
                                for (int k = g * CENTER_GROUP; k < std::min(t.n2, (g + 1) * CENTER_GROUP); ++k) {
                                    const double *src = t.h_values.data() + ((node * t.n2 + k) * 4 + q) * 2;
                                    double *dst = blk + ((size_t)(nd * 4 + q) * CENTER_GROUP + (k - g * CENTER_GROUP)) * 2;
                                    dst[0] = src[0];
                                    dst[1] = src[1];
                                }
                        }
                    }
        }
    } else {
        const size_t nodes = (size_t)t.n_orders * t.n0 * t.n1;
        out.cq.resize(nodes * t.n2 * 4 * 2);
        for (size_t nd = 0; nd < nodes; ++nd)
            for (int k = 0; k < t.n2; ++k)
                for (int q = 0; q < 4; ++q) {
                    const double *src = t.h_values.data() + ((nd * t.n2 + k) * 4 + q) * 2;
                    double *dst = out.cq.data() + ((nd * 4 + q) * t.n2 + k) * 2;
                    dst[0] = src[0];
                    dst[1] = src[1];
                }
    }
    return out;
}

// ---- layout --------------------------------------------------------------------------------
// The two tables searchsorted(boundaries, r, 'left') starts from, B = the n_rings + 1 ring boundaries.
struct RingSearchFacts {
    int lut_buckets = 0, lutrec_buckets = 0;
    double lut_inv_h = 0, lutrec_inv_h = 0;
    double r_outer = 0, r_centre = 0;   // (r_centre: inner boundary of ring 0 = radius of the centre disc)
};
struct RingSearch {
    PackError err;
    RingSearchFacts facts;
    // uniform-in-r lookup: lut[b] = number of boundaries strictly below the lower edge of bucket b
    std::vector<int32_t> lut;
    // fast kernel: buckets about half the narrowest ring wide (so that a bucket rarely holds
    // more than one boundary), each carrying the boundaries around its lower edge
    std::vector<RingBucket> rec;
};
inline RingSearch pack_ring_search(const double *B, int n_rings) {
    RingSearch out;
    const int buckets = 16384;
    const double r_max = B[n_rings];
    ML_PACK_REQUIRE(out, r_max > 0, "outer lens radius must be positive");
    const double h = r_max / buckets;
    out.lut.resize(buckets);
    int idx = 0;
    for (int b = 0; b < buckets; ++b) {
        const double edge = b * h;
        while (idx <= n_rings && B[idx] < edge) ++idx;
        out.lut[b] = idx;
    }
    out.facts.lut_buckets = buckets;
    out.facts.lut_inv_h = 1.0 / h;
    double narrowest = r_max;
    for (int k = 1; k <= n_rings; ++k)
        if (B[k] > B[k - 1]) narrowest = std::min(narrowest, B[k] - B[k - 1]);
    const int nb = (int)std::min(65536.0, std::max(1024.0, std::ceil(2.0 * r_max / narrowest)));
    const double hb = r_max / nb;
    out.rec.resize(nb);
    int at = 0;
    for (int b = 0; b < nb; ++b) {
        const double edge = b * hb;
        while (at <= n_rings && B[at] < edge) ++at;
        out.rec[b].first = at;
        out.rec[b].pad = 0;
        out.rec[b].bm1 = at > 0 ? B[at - 1] : -INFINITY;
        out.rec[b].b0 = at <= n_rings ? B[at] : INFINITY;
        out.rec[b].b1 = at + 1 <= n_rings ? B[at + 1] : INFINITY;
    }
    out.facts.lutrec_buckets = nb;
    out.facts.lutrec_inv_h = 1.0 / hb;
    out.facts.r_outer = r_max;
    out.facts.r_centre = B[0];
    return out;
}

// centre cells (x, y, type per cell) -> uniform grid of bins (about one cell per bin), cells stored in bin
// order; within a bin the original order is kept (ties resolve to the lowest index)
struct BinFacts {
    int bins_x = 0, bins_y = 0;
    double x0 = 0, y0 = 0, h = 0;
};
struct CellBins {
    PackError err;
    BinFacts facts;
    std::vector<double> sx, sy, sxy;         // sorted cells: x, y, and (x, y) interleaved
    std::vector<int32_t> sw, si;             // ... their types and original indices
    std::vector<int32_t> start;              // [bins_x bins_y + 1]: first sorted slot of every bin
    std::vector<int32_t> slot_of_cell;       // original cell index -> sorted slot
};
inline CellBins bin_cells(const double *cells, int n_cells) {
    CellBins out;
    double x0 = cells[0], x1 = cells[0], y0 = cells[1], y1 = cells[1];
    for (int c = 0; c < n_cells; ++c) {
        x0 = std::min(x0, cells[3 * c]);
        x1 = std::max(x1, cells[3 * c]);
        y0 = std::min(y0, cells[3 * c + 1]);
        y1 = std::max(y1, cells[3 * c + 1]);
    }
    double wx = x1 - x0, wy = y1 - y0;
    double hbin = std::sqrt(std::max(wx * wy, 1e-300) / n_cells);
    if (!(hbin > 0) || !std::isfinite(hbin)) hbin = 1.0;
    if (wx <= 0 && wy <= 0) hbin = 1.0;
    int bxn = (int)std::min<double>(std::floor(wx / hbin) + 1, 8192);
    int byn = (int)std::min<double>(std::floor(wy / hbin) + 1, 8192);
    bxn = std::max(bxn, 1);
    byn = std::max(byn, 1);
    // if the bin count was clipped, grow the bin so that the grid still covers the box
    hbin = std::max(hbin, std::max(wx / bxn, wy / byn) * (1 + 1e-12));
    std::vector<int32_t> bin_of(n_cells);
    out.start.assign((size_t)bxn * byn + 1, 0);
    for (int c = 0; c < n_cells; ++c) {
        int bx = std::min(std::max((int)std::floor((cells[3 * c] - x0) / hbin), 0), bxn - 1);
        int by = std::min(std::max((int)std::floor((cells[3 * c + 1] - y0) / hbin), 0), byn - 1);
        bin_of[c] = bx * byn + by;
        out.start[bin_of[c] + 1]++;
    }
    for (size_t b = 0; b < (size_t)bxn * byn; ++b) out.start[b + 1] += out.start[b];
    std::vector<int32_t> fill(out.start.begin(), out.start.end() - 1);
    out.sx.resize(n_cells);
    out.sy.resize(n_cells);
    out.sw.resize(n_cells);
    out.si.resize(n_cells);
    for (int c = 0; c < n_cells; ++c) {
        const int at = fill[bin_of[c]]++;
        out.sx[at] = cells[3 * c];
        out.sy[at] = cells[3 * c + 1];
        out.sw[at] = (int32_t)cells[3 * c + 2];   // .astype(int): truncation (nearfield.py:367)
        // (the geometry records carry the type in 11 bits above the ring index)
        ML_PACK_REQUIRE(out, out.sw[at] >= 0 && out.sw[at] < 2048, "centre cell %d has grating index %d: 0 ... 2047 are supported",
                        c, (int)out.sw[at]);
        out.si[at] = c;
    }
    out.sxy.resize(2 * (size_t)n_cells);
    for (int c = 0; c < n_cells; ++c) {
        out.sxy[2 * (size_t)c] = out.sx[c];
        out.sxy[2 * (size_t)c + 1] = out.sy[c];
    }
    out.slot_of_cell.assign(n_cells, 0);
    for (int c = 0; c < n_cells; ++c) out.slot_of_cell[out.si[c]] = c;
    out.facts = {bxn, byn, x0, y0, hbin};
    return out;
}

// The centre cells are, in every design this code has seen, the nodes of a 2-D lattice (a
// hexagonal grid, design_collimator.py:74-118), although the contract only promises "a list of
// points in arbitrary order" (design_collimator.py:124-125).  If - and only if - every cell sits
// within `tol` of a node of ONE lattice and no two cells share a node, the nearest-cell search
// can start from the four nodes around the sample instead of scanning bins.  The result is
// accepted only when it is provably nearest (see nearest_cell_fast), so a wrong fit can cost
// time but never correctness; anything irregular simply reports `ok = false`.
struct LatticeFacts {
    bool ok = false;
    double c0x = 0, c0y = 0, inv[4] = {0, 0, 0, 0};   // (u, v) = inv * (p - c0)
    int amin = 0, bmin = 0, na = 0, nb = 0;
    double accept_r2 = 0;
    double g[3] = {0, 0, 0}, guard = 0;   // metric of the basis; ambiguity guard for the analytic pick
};
struct LatticeFit {
    LatticeFacts facts;
    std::vector<int32_t> map;                          // [na][nb] -> sorted slot, -1 empty
};

inline double seg_dist(double px, double py, double ax, double ay, double bx, double by) {
    const double dx = bx - ax, dy = by - ay, l2 = dx * dx + dy * dy;
    double t = l2 > 0 ? ((px - ax) * dx + (py - ay) * dy) / l2 : 0.0;
    t = std::min(1.0, std::max(0.0, t));
    return std::hypot(px - (ax + t * dx), py - (ay + t * dy));
}

inline LatticeFit fit_lattice(const std::vector<double> &sx, const std::vector<double> &sy) {
    LatticeFit L;
    const int n = (int)sx.size();
    if (n < 16) return L;
    // origin: the cell nearest to the centroid; basis: its nearest neighbour and the nearest
    // neighbour that is not collinear with it (brute force, once per layout)
    double mx = 0, my = 0;
    for (int c = 0; c < n; ++c) {
        mx += sx[c];
        my += sy[c];
    }
    mx /= n;
    my /= n;
    int o = 0;
    double best = INFINITY;
    for (int c = 0; c < n; ++c) {
        const double d = (sx[c] - mx) * (sx[c] - mx) + (sy[c] - my) * (sy[c] - my);
        if (d < best) {
            best = d;
            o = c;
        }
    }
    int i1 = -1;
    best = INFINITY;
    for (int c = 0; c < n; ++c) {
        if (c == o) continue;
        const double d = (sx[c] - sx[o]) * (sx[c] - sx[o]) + (sy[c] - sy[o]) * (sy[c] - sy[o]);
        if (d < best) {
            best = d;
            i1 = c;
        }
    }
    if (i1 < 0 || !(best > 0)) return L;
    double b1x = sx[i1] - sx[o], b1y = sy[i1] - sy[o];
    const double l1 = b1x * b1x + b1y * b1y;
    int i2 = -1;
    best = INFINITY;
    for (int c = 0; c < n; ++c) {
        if (c == o) continue;
        const double dx = sx[c] - sx[o], dy = sy[c] - sy[o];
        if (std::fabs(b1x * dy - b1y * dx) < 0.25 * l1) continue;   // (nearly) collinear with b1
        const double d = dx * dx + dy * dy;
        if (d < best) {
            best = d;
            i2 = c;
        }
    }
    if (i2 < 0) return L;
    double b2x = sx[i2] - sx[o], b2y = sy[i2] - sy[o];
    // Gauss reduction: |b1| <= |b2|, |b1.b2| <= |b1|^2 / 2
    for (int it = 0; it < 8; ++it) {
        if (b2x * b2x + b2y * b2y < b1x * b1x + b1y * b1y) {
            std::swap(b1x, b2x);
            std::swap(b1y, b2y);
        }
        const double k = std::rint((b1x * b2x + b1y * b2y) / (b1x * b1x + b1y * b1y));
        if (k == 0) break;
        b2x -= k * b1x;
        b2y -= k * b1y;
    }
    const double det = b1x * b2y - b1y * b2x;
    if (!(std::fabs(det) > 0)) return L;
    const double pitch = std::sqrt(b1x * b1x + b1y * b1y);
    const double inv[4] = {b2y / det, -b2x / det, -b1y / det, b1x / det};
    // every cell on a node?
    std::vector<int> ia(n), ib(n);
    int amin = INT32_MAX, amax = INT32_MIN, bmin = INT32_MAX, bmax = INT32_MIN;
    double eps_max = 0;
    const double tol = 1e-6 * pitch;
    for (int c = 0; c < n; ++c) {
        const double dx = sx[c] - sx[o], dy = sy[c] - sy[o];
        const double u = std::rint(inv[0] * dx + inv[1] * dy), v = std::rint(inv[2] * dx + inv[3] * dy);
        if (std::fabs(u) > 1e8 || std::fabs(v) > 1e8) return L;
        const double rx = dx - (u * b1x + v * b2x), ry = dy - (u * b1y + v * b2y);
        const double e = std::hypot(rx, ry);
        if (!(e <= tol)) return L;
        eps_max = std::max(eps_max, e);
        ia[c] = (int)u;
        ib[c] = (int)v;
        amin = std::min(amin, ia[c]);
        amax = std::max(amax, ia[c]);
        bmin = std::min(bmin, ib[c]);
        bmax = std::max(bmax, ib[c]);
    }
    // the map also answers the corner at (a + 1, b + 1): no padding needed, lookups are range-checked
    const long na = (long)amax - amin + 1, nb = (long)bmax - bmin + 1;
    if (na * nb > 16L * n + 1024) return L;            // too sparse to be worth a dense map
    L.map.assign((size_t)(na * nb), -1);
    for (int c = 0; c < n; ++c) {
        int32_t &slot = L.map[(size_t)(ia[c] - amin) * nb + (ib[c] - bmin)];
        if (slot != -1) return LatticeFit();           // two cells on one node
        slot = c;
    }
    // smallest distance from the unit parallelogram to a lattice node that is not one of its corners
    double h_min = INFINITY;
    const double cx[4] = {0, b1x, b1x + b2x, b2x}, cy[4] = {0, b1y, b1y + b2y, b2y};
    for (int i = -2; i <= 3; ++i)
        for (int j = -2; j <= 3; ++j) {
            if ((i == 0 || i == 1) && (j == 0 || j == 1)) continue;
            const double px = i * b1x + j * b2x, py = i * b1y + j * b2y;
            for (int e = 0; e < 4; ++e)
                h_min = std::min(h_min, seg_dist(px, py, cx[e], cy[e], cx[(e + 1) & 3], cy[(e + 1) & 3]));
        }
    // cells sit within eps_max of their nodes; the sample is within ~1e-12 pitch of the
    // parallelogram picked by floor(); keep a margin for both
    const double r = h_min - 2 * eps_max - 1e-9 * pitch;
    if (!(r > 0.5 * pitch)) return L;                  // degenerate lattice: not worth it
    LatticeFacts &F = L.facts;
    F.ok = true;
    F.c0x = sx[o];
    F.c0y = sy[o];
    for (int k = 0; k < 4; ++k) F.inv[k] = inv[k];
    F.amin = amin;
    F.bmin = bmin;
    F.na = (int)na;
    F.nb = (int)nb;
    F.accept_r2 = r * r;
    F.g[0] = b1x * b1x + b1y * b1y;
    F.g[1] = b1x * b2x + b1y * b2y;
    F.g[2] = b2x * b2x + b2y * b2y;
    // |d^2(cell) - d^2(node)| <= 2 d eps + eps^2 with d <= ~2 pitch, for each of two candidates,
    // plus the rounding of the lattice-coordinate expressions (coordinates up to ~1e4 pitches
    // at 1e-16): a few 1e-12 pitch^2; generous factor on top
    F.guard = 8.0 * pitch * (eps_max + 1e-11 * pitch) + 1e-9 * pitch * pitch;
    return L;
}

// the lattice's nodes as the fast kernel reads them: the sorted cell on each node, or an empty record
inline std::vector<CellRec> lattice_records(const LatticeFit &L, const CellBins &cells) {
    std::vector<CellRec> rec(L.map.size());
    for (size_t n = 0; n < L.map.size(); ++n) {
        const int32_t slot = L.map[n];
        rec[n].x = slot >= 0 ? cells.sx[slot] : NAN;
        rec[n].y = slot >= 0 ? cells.sy[slot] : NAN;
        rec[n].which = slot >= 0 ? cells.sw[slot] : -1;
        rec[n].index = slot >= 0 ? cells.si[slot] : -1;
        rec[n].pad = 0.0;
    }
    return rec;
}

}  // namespace ml
