// The source-INDEPENDENT decisions of every aperture sample - which ring, which sector of it, which centre cell
// (reference nearfield.py:119-128, 169, 363-367), exact - as per-sample records, and the lists of 8 x 8 patches the
// field kernels (nearfield_simple.hip, nearfield_general.hip) launch from; at the end the test surface ml_geometry_probe.
#include "nearfield_dev.h"

namespace ml {

// one candidate of the nearest-cell search: ties go to the lowest original index (provisional,
// see settle_tie) and are remembered
__device__ __forceinline__ void consider_cell(const NfArgs &a, double d2, int s, double &best,
                                              int &best_slot, bool &tied) {
    if (d2 < best) {
        best = d2;
        best_slot = s;
        tied = false;
    } else if (d2 == best) {
        tied = true;
        if (a.cindex[s] < a.cindex[best_slot]) best_slot = s;
    }
}

// the winner shared its distance with another cell: take the host's answer if there is one,
// else keep the provisional winner and report the sample
// (`trace`, here and below: where a decision was made, for ml_geometry_probe - ML_GEO_* of metalens_hip.h; the product's
// call sites leave it at nullptr and every mention of it folds away)
__device__ __forceinline__ int settle_tie(const NfArgs &a, long long sample_id, int best_slot, int *trace = nullptr) {
    if (trace) *trace |= ML_GEO_TIE;
    int lo = 0, hi = a.n_ovr;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.ovr_key[mid] < sample_id)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo < a.n_ovr && a.ovr_key[lo] == sample_id) return a.ovr_slot[lo];
    const int at = atomicAdd(a.tie_count, 1);
    if (at < a.tie_cap) a.tie_list[at] = sample_id;
    return best_slot;
}

// exact nearest centre cell (nearfield.py:363-364) through a uniform grid of bins
__device__ __forceinline__ int nearest_cell(const NfArgs &a, double x, double y,
                                            long long sample_id, int *trace = nullptr) {
    int bx = (int)floor((x - a.bx0) / a.bh);
    int by = (int)floor((y - a.by0) / a.bh);
    bx = min(max(bx, 0), a.bins_x - 1);
    by = min(max(by, 0), a.bins_y - 1);
    double best = INFINITY;
    int best_slot = -1;
    bool tied = false;
    const int kmax = max(a.bins_x, a.bins_y);
    for (int k = 0; k <= kmax; ++k) {
        const int x_lo = bx - k, x_hi = bx + k, y_lo = by - k, y_hi = by + k;
        for (int gx = max(x_lo, 0); gx <= min(x_hi, a.bins_x - 1); ++gx) {
            const bool edge_col = (gx == x_lo) || (gx == x_hi);
            const int step = edge_col ? 1 : max(2 * k, 1);
            for (int gy = y_lo; gy <= y_hi; gy += step) {
                if (gy < 0 || gy >= a.bins_y) continue;
                const int b = gx * a.bins_y + gy;
                for (int s = a.bin_start[b]; s < a.bin_start[b + 1]; ++s) {
                    const double ex = x - a.cx[s], ey = y - a.cy[s];
                    consider_cell(a, ex * ex + ey * ey, s, best, best_slot, tied);
                }
            }
        }
        // every cell not yet visited is at least k*bh away
        const double reach = k * a.bh;
        if (best_slot >= 0 && best <= reach * reach) break;
    }
    return tied ? settle_tie(a, sample_id, best_slot, trace) : best_slot;
}

// Lattice shortcut, first try: the sample lies in (or within rounding of) the lattice
// parallelogram (ia, ib); pick the nearest of its four corner NODES analytically (squared
// distances in lattice coordinates).  Returns that node's index in the dense node map if it
// beats the runner-up by more than the guard - which covers the cells' offsets from their nodes
// and the rounding of these expressions - and lies inside the map, else -1.
__device__ __forceinline__ int lattice_pick(const NfArgs &a, double x, double y, int &ia, int &ib) {
    const double dx = x - a.lat_c0x, dy = y - a.lat_c0y;
    const double u = a.lat_inv[0] * dx + a.lat_inv[1] * dy, v = a.lat_inv[2] * dx + a.lat_inv[3] * dy;
    const double fu = floor(u), fv = floor(v);
    ia = (int)fu - a.lat_amin;
    ib = (int)fv - a.lat_bmin;
    const double ru = u - fu, rv = v - fv;           // in [0, 1)
    double d2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double pu = ru - (k >> 1), pv = rv - (k & 1);
        d2[k] = a.lat_g[0] * pu * pu + 2.0 * a.lat_g[1] * pu * pv + a.lat_g[2] * pv * pv;
    }
    int kb = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) kb = d2[k] < d2[kb] ? k : kb;
    double second = INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) second = (k != kb && d2[k] < second) ? d2[k] : second;
    const int ca = ia + (kb >> 1), cb = ib + (kb & 1);
    if (second - d2[kb] > a.lat_guard && ca >= 0 && ca < a.lat_na && cb >= 0 && cb < a.lat_nb)
        return ca * a.lat_nb + cb;
    return -1;
}

// Nearest centre cell, fast path: the 3 x 3 bin neighbourhood of the sample is three
// contiguous runs of the bin-sorted cell array (one per bin column), so the search is 6 loads of
// run bounds + one 16-byte load per candidate (~10) instead of ~50 scattered loads.  Exactness
// is kept: the result is accepted only if it is provably nearest (distance <= one bin width,
// same rule as nearest_cell), otherwise the ring-growing search runs; ties resolve to the
// lowest original index.
__device__ __forceinline__ int nearest_cell_fast(const NfArgs &a, double x, double y,
                                                 long long sample_id, int *trace = nullptr) {
    // Lattice shortcut: the sample lies in (or within rounding of) the lattice parallelogram
    // (a0, b0); its four corner nodes are the candidates.  Every cell that is NOT one of them
    // sits on another node, i.e. at least lat_accept_r away from anywhere in that parallelogram
    // (margins for the cells' offsets from their nodes and for the rounding of floor() are in
    // lat_accept_r), so a candidate closer than that is the nearest cell - also when corners are
    // empty.  Ties between equidistant candidates go to the lowest original index, as below.
    if (a.lat_map) {
        int ia, ib;
        const int node = lattice_pick(a, x, y, ia, ib);
        if (node >= 0) {
            const int s = a.lat_map[node];
            if (s >= 0) {
                const double2 q = a.cxy[s];
                const double ex = x - q.x, ey = y - q.y;
                if (ex * ex + ey * ey <= a.lat_accept_r2) {
                    if (trace) *trace |= ML_GEO_CELL_NODE;
                    return s;
                }
            }
        }
        int cand[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ca = ia + (k >> 1), cb = ib + (k & 1);
            const bool in = ca >= 0 && ca < a.lat_na && cb >= 0 && cb < a.lat_nb;
            cand[k] = in ? a.lat_map[(size_t)ca * a.lat_nb + cb] : -1;
        }
        double2 p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = a.cxy[max(cand[k], 0)];
        double best = INFINITY;
        int best_slot = -1;
        bool tied = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (cand[k] < 0) continue;
            const double ex = x - p[k].x, ey = y - p[k].y;
            consider_cell(a, ex * ex + ey * ey, cand[k], best, best_slot, tied);
        }
        if (best_slot >= 0 && best <= a.lat_accept_r2) {
            if (trace) *trace |= ML_GEO_CELL_FOUR;
            return tied ? settle_tie(a, sample_id, best_slot, trace) : best_slot;
        }
    }
    // bin of the sample by multiplication with 1/bh (two fp64 divisions saved).  A sample within
    // an ulp of a bin edge may land in the neighbouring bin; the acceptance test below allows
    // for that by requiring the winner to be closer than bh (1 - 1e-9).
    int bx = (int)floor((x - a.bx0) * a.inv_bh);
    int by = (int)floor((y - a.by0) * a.inv_bh);
    bx = min(max(bx, 0), a.bins_x - 1);
    by = min(max(by, 0), a.bins_y - 1);
    const int gy_lo = max(by - 1, 0), gy_hi = min(by + 1, a.bins_y - 1);
    int lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int gx = bx - 1 + c;
        const bool ok = gx >= 0 && gx < a.bins_x;
        const int base = (ok ? gx : bx) * a.bins_y;
        lo[c] = a.bin_start[base + gy_lo];
        hi[c] = ok ? a.bin_start[base + gy_hi + 1] : lo[c];
    }
    double best = INFINITY;
    int best_slot = -1;
    bool tied = false;
    // candidates are fetched four per run at a time, all twelve loads in flight together
    // (a one-candidate-per-iteration loop would serialise ~10 L1 latencies per sample)
    constexpr int BATCH = 4;
    int more = 0;
    {
        double2 p[3][BATCH];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < BATCH; ++k)
                p[c][k] = a.cxy[min(lo[c] + k, a.n_cells - 1)];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int k = 0; k < BATCH; ++k) {
                const int s = lo[c] + k;
                if (s < hi[c]) {
                    const double ex = x - p[c][k].x, ey = y - p[c][k].y;
                    consider_cell(a, ex * ex + ey * ey, s, best, best_slot, tied);
                }
            }
            more |= (hi[c] - lo[c] > BATCH);
        }
    }
    if (more) {   // denser bins than usual: finish the runs one by one
        if (trace) *trace |= ML_GEO_CELL_MORE;
        for (int c = 0; c < 3; ++c)
            for (int s = lo[c] + BATCH; s < hi[c]; ++s) {
                const double2 q = a.cxy[s];
                const double ex = x - q.x, ey = y - q.y;
                consider_cell(a, ex * ex + ey * ey, s, best, best_slot, tied);
            }
    }
    const double reach = a.bh * (1.0 - 1e-9);
    if (best_slot < 0 || !(best <= reach * reach)) {
        if (trace) *trace |= ML_GEO_CELL_GROW;
        return nearest_cell(a, x, y, sample_id, trace);
    }
    if (trace) *trace |= ML_GEO_CELL_BINS;
    return tied ? settle_tie(a, sample_id, best_slot, trace) : best_slot;
}

// Sector of a sample: round(arctan2(y, x) / dphi) (nearfield.py:119,169), clamped to the
// tabulated range.  If phi / dphi comes within 1e-9 of a tie the decision would hang on the
// last bit of atan2 (samples on or one ulp off the diagonals of a symmetric grid do this when
// num_around_circle = 4 mod 8), so phi is then recomputed to ~1e-19 about the boundary angle
// theta = (k + 1/2) dphi from the host's extended-precision table,
//   phi = theta + atan((y cos theta - x sin theta) / (x cos theta + y sin theta)),
// and rounded: the kernel follows the CORRECTLY ROUNDED arctan2.  NumPy's agrees with it on the diagonals and axes
// and wherever a sample lies 1e-12 sectors or more from a tie; closer than that it may differ in its last bit and
// so in the sector (counted in profiles/geometry_probe.txt; tests/test_gpu_geometry_cases.py holds the kernel to
// the correctly rounded decision at such points through ml_geometry_probe).
// `inv_dphi` != 0 (fast kernel): the first quotient is phi * inv_dphi; it differs from phi / dphi by
// ~1e-16 relative, 1e7 times less than the width of the tie window, so the decision is the same.
__device__ __forceinline__ int sector_of(const NfArgs &a, int ring, double x, double y,
                                         double dphi, double inv_dphi = 0.0) {
    const int half = a.rot_half[ring];
    double q = inv_dphi != 0.0 ? atan2(y, x) * inv_dphi : atan2(y, x) / dphi;
    const double fl = floor(q);
    if (fabs((q - fl) - 0.5) < 1e-9) {
        const int k = min(max((int)fl, -half - 1), half);
        const double *e = a.tie_table + (size_t)(a.rot_center[ring] + k) * 6;
        const double th_hi = e[0], th_lo = e[1], c_hi = e[2], c_lo = e[3], s_hi = e[4], s_lo = e[5];
        const double p1 = y * c_hi, e1 = fma(y, c_hi, -p1);
        const double p2 = x * s_hi, e2 = fma(x, s_hi, -p2);
        const double num = (p1 - p2) + ((e1 - e2) + (y * c_lo - x * s_lo));
        const double den = x * c_hi + y * s_hi;
        const double phi = th_hi + (th_lo + num / den);
        q = phi / dphi;
    }
    return min(max((int)rint(q), -half), half);
}

// which ring: number of ring boundaries strictly below r, i.e.
// searchsorted(boundaries, r, 'left') (nearfield.py:125-128), through the uniform-in-r LUT
__device__ __forceinline__ int boundaries_below(const NfArgs &a, double r) {
    if (r > a.B[a.n_rings]) return a.n_rings + 1;
    int bucket = (int)(r * a.lut_inv_h);
    bucket = min(max(bucket, 0), a.lut_buckets - 1);
    int idx = a.lut[bucket];
    while (idx <= a.n_rings && a.B[idx] < r) ++idx;
    while (idx > 0 && a.B[idx - 1] >= r) --idx;
    return idx;
}

// the same answer from one 32-byte bucket record whenever the record settles it (at most one
// boundary inside the bucket below r), else by the search above
__device__ __forceinline__ int boundaries_below_fast(const NfArgs &a, double r, int *trace = nullptr) {
    if (trace) *trace |= ML_GEO_RING_RECORD;   // (r_outer is the record table's too; the search below takes the bit back)
    if (r > a.r_outer) return a.n_rings + 1;
    int bucket = (int)(r * a.lutrec_inv_h);
    bucket = min(max(bucket, 0), a.lutrec_buckets - 1);
    // the record as ONE 32-byte vector load: read field by field the compiler fetches two
    // fields, waits, branches, and only then fetches the other two
    typedef double rec_t __attribute__((ext_vector_type(4)));
    const rec_t q = *reinterpret_cast<const rec_t *>(a.lutrec + bucket);   // bm1, b0, b1, (first, pad)
    const int first = (int)(__double_as_longlong(q.w) & 0xffffffffll);
    const bool below0 = q.y < r, below1 = q.z < r;
    if (q.x < r && !below1) return first + (below0 ? 1 : 0);
    if (trace) *trace ^= ML_GEO_RING_RECORD | ML_GEO_RING_SEARCH;
    return boundaries_below(a, r);
}

// arctan2(y, x) to ~2 ulp for finite (x, y) != (0, 0): atan(a) = a Q(a^2) on [0, 1] (degree-20
// least-squares-at-Chebyshev-nodes fit, 2.6e-17 from atan with these rounded coefficients),
// reciprocal by Newton steps, octant fix-ups by selects.  The device libm's atan2 costs ~160
// vector instructions here (44 of them v_mov pairs for its coefficients, two divisions, class
// tests); this is ~45.  Used for the sector decision only, whose near-ties are re-decided
// exactly (sector_of_fast), so 2 ulp is 1e6 times finer than needed.
__device__ __forceinline__ double atan2_fast(double y, double x) {
    const double ax = fabs(x), ay = fabs(y);
    const double mx = fmax(ax, ay), mn = fmin(ax, ay);
    const double t = mn * recip(mx);
    const double z = t * t;
    double q = horner(z, 1.26311784304774261e-05, -1.46170881636250135e-04);
    q = horner(z, q, 8.03360418162602668e-04);
    q = horner(z, q, -2.80476555317013152e-03);
    q = horner(z, q, 7.03864620298981329e-03);
    q = horner(z, q, -1.36741392883994780e-02);
    q = horner(z, q, 2.17402138307581337e-02);
    q = horner(z, q, -2.97007177362342313e-02);
    q = horner(z, q, 3.65108135272103479e-02);
    q = horner(z, q, -4.21257239638553257e-02);
    q = horner(z, q, 4.71972399232111206e-02);
    q = horner(z, q, -5.25272555732257465e-02);
    q = horner(z, q, 5.88034200240154306e-02);
    q = horner(z, q, -6.66637118772109849e-02);
    q = horner(z, q, 7.69227555520562989e-02);
    q = horner(z, q, -9.09090660565689823e-02);
    q = horner(z, q, 1.11111109820871259e-01);
    q = horner(z, q, -1.42857142815926930e-01);
    q = horner(z, q, 1.99999999999299460e-01);
    q = horner(z, q, -3.33333333333328596e-01);
    // atan(t) = t + t z q'  keeps the leading term exact
    double r = fma(t * z, q, t);
    r = ay > ax ? 1.57079632679489655800e+00 - r : r;
    r = x < 0.0 ? 3.14159265358979311600e+00 - r : r;
    // the sign as atan2 takes it: y = -0.0 with x < 0 is -pi, a different sector from +pi when num_around_circle is odd
    return copysign(r, y);
}

// sector_of (above) with the ring's constants already in registers and the fast
// arctangent; the near-tie branch is the same exact recomputation
__device__ __forceinline__ int sector_of_fast(const NfArgs &a, int half, int rot_center, double x,
                                              double y, double dphi, double inv_dphi, int *trace = nullptr) {
    double q = atan2_fast(y, x) * inv_dphi;
    const double fl = floor(q);
    if (fabs((q - fl) - 0.5) < 1e-9) {
        const int k = min(max((int)fl, -half - 1), half);
        if (trace) *trace |= ML_GEO_SECTOR_EXACT | (k != (int)fl ? ML_GEO_SECTOR_CLAMPED : 0);
        const double *e = a.tie_table + (size_t)(rot_center + k) * 6;
        const double th_hi = e[0], th_lo = e[1], c_hi = e[2], c_lo = e[3], s_hi = e[4], s_lo = e[5];
        const double p1 = y * c_hi, e1 = fma(y, c_hi, -p1);
        const double p2 = x * s_hi, e2 = fma(x, s_hi, -p2);
        const double num = (p1 - p2) + ((e1 - e2) + (y * c_lo - x * s_lo));
        const double den = x * c_hi + y * s_hi;
        const double phi = th_hi + (th_lo + num / den);
        q = phi / dphi;
    }
    if (trace && ((int)rint(q) < -half || (int)rint(q) > half)) *trace |= ML_GEO_SECTOR_CLAMPED;
    return min(max((int)rint(q), -half), half);
}

// ---- the records: the source-INDEPENDENT decisions of every sample ---------------------------
// Ring (nearfield.py:125-128), sector and rotated local coordinates (:169,200-201), nearest
// centre cell (:363-367) depend on the sample grid and the layout only.  They are evaluated once
// per (grid, layout, tie answers) into an 8-byte record per sample (stored patch by patch),
//     geo_ix = (idx | collection << 20, index into the rotation table)     periphery, idx = ring + 1,
//                  collection = dense number of the ring's grating collection (ml_upload_layout)
//              (cell type << 20, slot of the nearest cell; -1: no cells) centre: the cell's type
//                  rides in the bits above the ring index (rings < 2^19) - one gather fewer
//                  behind the record in the field kernels
//              (n_rings + 1, -)                           outside the lens
// (the rotated coordinates and the cell centre follow from these with one table load each: a
// 24-byte record that carried them cost 10 % more per extra 16 bytes - the kernel is sensitive
// to the bytes it streams from HBM, not to arithmetic in the shadow of its loads)
// and every synthesis on that geometry - a sweep over sources, the steps of a benchmark - starts
// from the records.  Same thread -> sample map as the field kernels (8 x 8 patch per wave).
// the decisions of one sample (see the geometry kernel below): idx, aux
__device__ __forceinline__ void sample_geometry(const NfArgs &a, double x, double y, long long sample_id,
                                                int &idx, int &aux, int *trace = nullptr) {
    const double r = sqrt(x * x + y * y);
    idx = boundaries_below_fast(a, r, trace);
    aux = -1;
    if (idx >= 1 && idx <= a.n_rings) {
        const int ring = idx - 1;
        const double dphi = a.dphi[ring];
        const int rot_half = a.rot_half[ring], rot_center = a.rot_center[ring];
        // sector decision: exact (nearfield.py:169)
        const int sector = sector_of_fast(a, rot_half, rot_center, x, y, dphi, recip(dphi), trace);
        aux = rot_center + sector;
    } else if (idx == 0 && a.n_cells > 0) {
        // nearest cell: the lattice shortcut settles almost every sample from the node map (two
        // loads); anything it cannot settle goes through nearest_cell_fast
        bool have_cell = false;
        if (a.lat_rec) {
            int ia, ib;
            const int node = lattice_pick(a, x, y, ia, ib);
            if (node >= 0) {
                typedef double rec_t __attribute__((ext_vector_type(4)));
                const rec_t q = *reinterpret_cast<const rec_t *>(a.lat_rec + node);
                const double ex = x - q.x, ey = y - q.y;
                if (ex * ex + ey * ey <= a.lat_accept_r2) {   // false for a NaN (empty) node
                    aux = a.lat_map[node];
                    have_cell = true;
                    if (trace) *trace |= ML_GEO_CELL_NODE;
                }
            }
        }
        if (!have_cell) aux = nearest_cell_fast(a, x, y, sample_id, trace);
        aux = max(aux, 0);   // a (never produced) negative slot would read as "no cells"
    }
}

#ifndef ML_GEO_OCC
#define ML_GEO_OCC 8   // (8: 64 registers, the spills sit in nearest_cell_fast's cold search; 102 us against 117 at 4 on 4096^2)
#endif
__global__ __launch_bounds__(64, ML_GEO_OCC) void nearfield_geometry_kernel(const NfArgs a) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.y * 8 + (lane >> 3);
    const int j = blockIdx.x * 8 + (lane & 7);
    int idx = a.n_rings + 1, aux = -1;
    if (j < a.ny && i < a.nx) {
        const size_t at = (size_t)i * a.ny + j;
        sample_geometry(a, a.x_pts[i], a.y_pts[j], (long long)at, idx, aux);
        // patch-major: the 64 records of a wave are 512 contiguous bytes
        const size_t rec = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 64 + lane;
        const int type = (idx == 0 && aux >= 0) ? a.cwhich[aux] : (idx >= 1 && idx <= a.n_rings) ? a.ring_coll[idx - 1] : 0;
        a.geo_ix[rec] = make_int2(idx | (type << REC_TYPE_SHIFT), aux);
    }
    // patches with at least one sample inside the lens: the field kernels visit only these once
    // the zeros of the others are in place.  Flags per patch here - bit 0 any lens sample, bit 1 any
    // ring sample of a narrow collection, bit 2 any centre sample, bit 3 any ring sample of a wide
    // collection - compacted into lists by active_compact_kernel (190 k
    // waves adding to ONE counter took 2 ms)
    // (ring samples by the instantiation of nearfield_simple.hip that takes their collection: NfArgs::wide_mask)
    // (bit 4: any sample of a table that is NOT simple while others are - the general kernel's patches of a mixed
    // lens, NfArgs::general_mask / centre_general; such samples count for neither ring instantiation nor the centre kernel)
    const bool ring = idx >= 1 && idx <= a.n_rings;
    const int coll = a.ring_coll[min(max(idx, 1), a.n_rings) - 1];
    const bool gen = a.simple_orders && ((ring && ((a.general_mask >> coll) & 1)) || (idx == 0 && a.centre_general));
    const bool wide = ring && !gen && ((a.wide_mask >> coll) & 1);
    const int any_ring = __any(ring), any_centre = __any(idx == 0);   // all lanes vote
    const int any_narrow = __any(ring && !wide && !gen), any_wide = __any(wide), any_gen = __any(gen);
    const int any_simple_centre = __any(idx == 0 && !gen);
    if (lane == 0)
        a.active_flag[(size_t)blockIdx.y * gridDim.x + blockIdx.x] =
            ((any_ring | any_centre) ? 1 : 0) | (any_narrow ? 2 : 0) | (any_simple_centre ? 4 : 0) | (any_wide ? 8 : 0) |
            (any_gen ? 16 : 0);
}

// flags -> list of (bx, by) of the patches whose flags meet `mask`, in patch order.  Two small
// kernels over chunks of 1024 patches: listed patches per chunk, then (per chunk) the sum of the
// chunks before it + a scan of its own flags + the writes.  count[0] = total, count[1 + c] = chunk c.
constexpr int COMPACT_CHUNK = 1024;

__device__ __forceinline__ int chunk_scan(int mine, int *s_wave, int &total) {
    // exclusive prefix of `mine` (0 / 1) over the 1024 threads of the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long votes = __ballot(mine);
    const int before = __popcll(votes & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < COMPACT_CHUNK / 64; ++w) {
        const int v = s_wave[w];
        base += w < wave ? v : 0;
        total += v;
    }
    return base + before;
}

// blockIdx.y = which list: mask = masks[y] (0: a list nobody launches from - its count is written as 0),
// count / list = the y-th of arrays count_stride / list_stride apart
struct CompactLists {
    int mask[4], first, n;   // lists first ... first + n - 1
};

__global__ __launch_bounds__(COMPACT_CHUNK) void active_count_kernel(const int *flag, CompactLists L, int n_patches, int *count,
                                                                     int count_stride) {
    __shared__ int s_wave[COMPACT_CHUNK / 64];
    const int mask = L.mask[blockIdx.y];
    count += (size_t)(L.first + blockIdx.y) * count_stride;
    const int k = blockIdx.x * COMPACT_CHUNK + threadIdx.x;
    int total;
    chunk_scan(k < n_patches ? (flag[k] & mask) != 0 : 0, s_wave, total);
    if (threadIdx.x == 0) count[1 + blockIdx.x] = total;
}

__global__ __launch_bounds__(COMPACT_CHUNK) void active_compact_kernel(const int *flag, CompactLists L, int n_patches,
                                                                       int patches_x, int2 *list, int list_stride,
                                                                       int *count, int count_stride) {
    __shared__ int s_wave[COMPACT_CHUNK / 64];
    __shared__ int s_before[COMPACT_CHUNK / 64];
    const int mask = L.mask[blockIdx.y];
    count += (size_t)(L.first + blockIdx.y) * count_stride;
    list += (size_t)(L.first + blockIdx.y) * list_stride;
    // lens patches in the chunks before this one (a few hundred chunks at most)
    int part = 0;
    for (int c = threadIdx.x; c < (int)blockIdx.x; c += COMPACT_CHUNK) part += count[1 + c];
    for (int off = 32; off; off >>= 1) part += __shfl_down(part, off);
    if ((threadIdx.x & 63) == 0) s_before[threadIdx.x >> 6] = part;
    const int k = blockIdx.x * COMPACT_CHUNK + threadIdx.x;
    const int mine = k < n_patches ? (flag[k] & mask) != 0 : 0;
    int total;
    const int at = chunk_scan(mine, s_wave, total);   // (its barrier also covers s_before)
    int before = 0;
#pragma unroll
    for (int w = 0; w < COMPACT_CHUNK / 64; ++w) before += s_before[w];
    if (mine) list[before + at] = make_int2(k % patches_x, k / patches_x);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) count[0] = before + total;
}

int nearfield_geometry_launch(ml_ctx *ctx, const NfArgs &a) {
    const dim3 grid((a.ny + 7) / 8, (a.nx + 7) / 8);
    hipLaunchKernelGGL(nearfield_geometry_kernel, grid, dim3(64), 0, ctx->stream, a);
    ML_HIP(hipGetLastError());
    // the lists the field kernels of this lens launch from (NfArgs::active_list): every lens patch
    // for the general kernels; ring patches and centre patches for the two kernels of nearfield_simple.hip
    const int n_patches = (int)(grid.x * grid.y), chunks = (n_patches + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
    // (all the lists of the lens in ONE launch of each of the two kernels: blockIdx.y = list.  A list nobody
    // launches from - narrow ring patches of a lens without narrow collections, wide ones of a lens without
    // wide collections - gets the mask 0: nothing listed, count 0)
    const bool mixed = a.simple_orders && (a.general_mask || a.centre_general);
    CompactLists L;
    L.first = a.simple_orders && !mixed ? 1 : 0;
    L.n = mixed ? 4 : a.simple_orders ? 3 : 1;
    for (int y = 0; y < 4; ++y) L.mask[y] = 0;
    for (int y = 0; y < L.n; ++y) {
        const int k = L.first + y;
        L.mask[y] = ((k == 1 && !a.narrow_exists) || (k == 3 && !a.wide_mask)) ? 0 : 1 << k;
        if (k == 0 && mixed) L.mask[y] = 16;   // (list 0 of a mixed lens: the patches with samples of general tables)
        if (k == 2 && a.simple_orders && a.centre_general) L.mask[y] = 0;   // (no centre kernel: the centre table is general)
    }
    hipLaunchKernelGGL(active_count_kernel, dim3(chunks, L.n), dim3(COMPACT_CHUNK), 0, ctx->stream, a.active_flag, L, n_patches,
                       a.active_count, a.count_stride);
    ML_HIP(hipGetLastError());
    hipLaunchKernelGGL(active_compact_kernel, dim3(chunks, L.n), dim3(COMPACT_CHUNK), 0, ctx->stream, a.active_flag, L,
                       n_patches, (int)grid.x, a.active_list, a.list_stride, a.active_count, a.count_stride);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

// ---- test surface (ml_geometry_probe): the decisions of sample_geometry at points of the caller's ------------------
// One lane per point, against the layout on the context, with the trace the product's instantiation compiles out.
// Down here so that no product kernel of this file moves.  No product code launches it.
constexpr int GEO_PROBE_MAX_N = 1 << 20;
constexpr int GEO_PROBE_TIES = 4096;   // entries of the probe's own tie list (the count goes on beyond it)

__global__ __launch_bounds__(64) void geometry_probe_kernel(const NfArgs a, const double *x, const double *y, int n, int *ring,
                                                            int *pick, int *path) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    int idx, aux, trace = 0;
    sample_geometry(a, x[i], y[i], (long long)i, idx, aux, &trace);
    int p = -1;
    if (idx >= 1 && idx <= a.n_rings)
        p = aux - a.rot_center[idx - 1];
    else if (idx == 0 && a.n_cells > 0)
        p = a.cindex[aux];
    ring[i] = idx;
    pick[i] = p;
    path[i] = trace;
}

}  // namespace ml

using namespace ml;

extern "C" int ml_geometry_probe(ml_ctx *ctx, const double *x, const double *y, int n, int32_t *ring, int32_t *pick,
                                 int32_t *path) {
    ML_REQUIRE(ctx && x && y && ring && pick && path, "ml_geometry_probe: NULL argument");
    ML_REQUIRE(n >= 1 && n <= GEO_PROBE_MAX_N, "ml_geometry_probe: n = %d points, 1 ... 2^20 are taken", n);
    for (int i = 0; i < n; ++i)
        ML_REQUIRE(std::isfinite(x[i]) && std::isfinite(y[i]), "ml_geometry_probe: point %d is not finite (%g, %g)", i, x[i], y[i]);
    if (!ctx->lens.have_layout) {
        set_error("ml_geometry_probe: ml_upload_layout has not been called");
        return ML_ESTATE;
    }
    ML_HIP(hipSetDevice(ctx->device));
    const size_t nd = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int32_t);
    // [x][y] doubles, [tie list] 64-bit integers, [ring][pick][path][tie count] integers - all the probe's own
    DevBuf buf;
    ML_TRY(buf.reserve(2 * nd + GEO_PROBE_TIES * sizeof(long long) + 3 * ni + sizeof(int)));
    double *dx = buf.as<double>(), *dy = dx + n;
    long long *tie_list = reinterpret_cast<long long *>(dy + n);
    int *dring = reinterpret_cast<int *>(tie_list + GEO_PROBE_TIES), *dpick = dring + n, *dpath = dpick + n, *tie_count = dpath + n;
    NfArgs a{};
    fill_layout_args(ctx, a);
    a.tie_count = tie_count;
    a.tie_list = tie_list;
    a.tie_cap = GEO_PROBE_TIES;
    a.n_ovr = 0;   // no answers: every tie keeps the lowest original index
    ML_HIP(hipMemcpyAsync(dx, x, nd, hipMemcpyHostToDevice, ctx->stream));
    ML_HIP(hipMemcpyAsync(dy, y, nd, hipMemcpyHostToDevice, ctx->stream));
    ML_HIP(hipMemsetAsync(tie_count, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(geometry_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, a, dx, dy, n, dring, dpick, dpath);
    ML_HIP(hipGetLastError());
    ML_HIP(hipMemcpyAsync(ring, dring, ni, hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipMemcpyAsync(pick, dpick, ni, hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipMemcpyAsync(path, dpath, ni, hipMemcpyDeviceToHost, ctx->stream));
    ML_HIP(hipStreamSynchronize(ctx->stream));
    return ML_OK;
}
