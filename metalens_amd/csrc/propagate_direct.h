// Launch arithmetic of the direct pair sum of the finite-distance propagator (propagate.hip propagate_kernel,
// propagate_sets), on the host and free of HIP types (as propagate_focus.h and fields_wavefront.h):
// tools/propagate_direct_plan.cpp and tests/test_propagate_direct_cases.py run it without a GPU.
//
// A lane is a target, a workgroup PROP_THREADS of them: prop_tiles(T) target tiles.  The nx rows of the aperture are
// dealt round robin to prop_splits(T, nx) workgroups per target tile - workgroup s sums the rows s, s + splits, ... -
// so that about PROP_BLOCKS workgroups run whatever T is; splits depends on T and nx alone, never on the field sets of
// a pass or on H.  A row's ny samples go through the LDS in tiles of PROP_TILE.  Every workgroup leaves a partial sum
// per (set, component, target), the second pass adds the `splits` partials in their order.
#pragma once

#include <cstddef>

namespace ml {

constexpr int PROP_THREADS = 256;   // targets per workgroup
constexpr int PROP_TILE = 128;      // aperture samples per LDS tile (8 KiB per field set)
constexpr int PROP_MAX_SETS = 3;    // field sets per pass (the members of a synthesis batch, nearfield_dev.h MAX_POL)
constexpr int PROP_BLOCKS = 2048;   // workgroups aimed at: eight per compute unit

// target tiles of T targets
inline int prop_tiles(int T) { return (T + PROP_THREADS - 1) / PROP_THREADS; }

// workgroups per target tile (of T and nx alone)
inline int prop_splits(int T, int nx) {
    const int tiles = prop_tiles(T), aimed = (PROP_BLOCKS + tiles - 1) / tiles;
    const int least = nx < aimed ? nx : aimed;
    return least > 1 ? least : 1;
}

// rows of the aperture that workgroup s of `splits` sums: s, s + splits, ... below nx
inline int prop_rows_of(int nx, int splits, int s) { return s < nx ? (nx - s + splits - 1) / splits : 0; }

// doubles per target and field set in `partial`: re and im of E (and H)
inline int prop_partial_doubles(bool want_h) { return want_h ? 12 : 6; }

// bytes of `partial` [splits][sets][12 or 6][T] doubles and of `result` [sets][6 or 3][T] complex
inline size_t prop_partial_bytes(int T, int nx, int sets, bool want_h) {
    return (size_t)prop_splits(T, nx) * sets * prop_partial_doubles(want_h) * T * sizeof(double);
}

inline size_t prop_result_bytes(int T, int sets, bool want_h) {
    return (size_t)sets * (prop_partial_doubles(want_h) / 2) * T * 2 * sizeof(double);
}

// A target's coordinate against the aperture's origin, x - x0, as two doubles: hi = fl(x - x0) and lo = (x - x0) - hi
// exactly (the two-sum of x and -x0, six roundings none of which may be contracted: -ffp-contract=off).  The kernel forms
// dx = fma(-i, dx', hi) + lo, so the distance to the sample under a target is as good as the distance to any other:
// with hi alone it is off by up to u |x - x0|, 1e-22 m at a micrometre - 1e-14 of a field 30 nm behind the aperture.
inline double prop_two_diff(double x, double x0, double *lo) {
    const double c = -x0, s = x + c;
    const double cp = s - x, xp = s - cp;
    *lo = (x - xp) + (c - cp);
    return s;
}

// doubles of the plan's target buffer: [5][T] - hi of x - x0, hi of y - y0, z, lo of x - x0, lo of y - y0
constexpr int PROP_TARGET_ROWS = 5;

}  // namespace ml
