// Plan arithmetic of the Stokes records of a propagated image (propagate_stokes.hip), on the host and free of HIP types
// (as propagate_focus.h): tools/propagate_stokes_plan.cpp and tests/test_propagate_stokes_host.py run it without a GPU.
//
// Per target of the resident result, from Ex, Ey, Ez alone (H is never read), every operation rounded on its own:
//   a  = Ex.r Ex.r + Ex.i Ex.i      b = Ey.r Ey.r + Ey.i Ey.i      Iz = Ez.r Ez.r + Ez.i Ez.i
//   S0 = a + b                      S1 = a - b
//   S2 = 2 (Ex.r Ey.r + Ex.i Ey.i)            (= 2 Re(Ex conj Ey))
//   S3 = 2 (Ex.r Ey.i - Ex.i Ey.r)            (= 2 Im(conj(Ex) Ey))
//   I  = S0 + Iz                               (the bits of ml_propagate_focus's I = (a + b) + c)
// The sign of S3: S3 = +S0 for E proportional to x^ + i y^.  Under the project's exp(-i omega t), for a wave travelling
// to +z, that is the field rotating counter-clockwise seen looking towards the source (positive helicity).
//
// The cut of a plane into chunks, the two launches and the membership rule of a radius are those of propagate_focus.h
// (focus_chunk_targets of P = mx my alone; a target is inside radius R iff (dx (i - ci))^2 + (dy (j - cj))^2 <= R R).
//
// The record of a plane, in doubles (what ml_propagate_stokes returns; K = n_radii):
//   [STOKES_PEAK_I]             the largest I of the plane (the sums: the largest stored S0_sum + Iz_sum)
//   [STOKES_PEAK_INDEX]         its flat index i my + j within the plane, the lowest one of equals
//   [STOKES_SUMS + q]           q = 0 ... 4: the sums of S0, S1, S2, S3, Iz over the plane
//   [STOKES_CENTRE]             ci, cj: the centre the radii were taken about, in index units (no centre given: the peak's)
//   [STOKES_ENC + 5 r + q]      r < K: the sum of component q over the targets inside radius r
// stokes_record_doubles(K) = STOKES_ENC + 5 K = 9 + 5 K.
//
// A partial record of a chunk has STOKES_PARTIAL doubles: the chunk's peak and its index, the five sums, and behind them
// [radius][component] for STOKES_RADII_MAX radii - the sum inside every radius itself, not of the annulus in front of it:
// the second launch adds nothing across radii, so a radius' sum does not depend on the other radii of the call.
#pragma once

#include "propagate_focus.h"

namespace ml {

constexpr int STOKES_THREADS = FOCUS_THREADS;
constexpr int STOKES_STEP = FOCUS_STEP;
constexpr int STOKES_RADII_MAX = FOCUS_RADII_MAX;
constexpr int STOKES_COMPONENTS = 5;   // S0, S1, S2, S3, Iz
constexpr int STOKES_FINISH_THREADS = 256;
constexpr int STOKES_FINISH_TILE = FOCUS_FINISH_TILE;

constexpr int STOKES_PEAK_I = 0, STOKES_PEAK_INDEX = 1, STOKES_SUMS = 2, STOKES_CENTRE = 7, STOKES_ENC = 9;
constexpr int STOKES_PARTIAL_RADII = 7;                                                          // where the radii of a partial record begin
constexpr int STOKES_PARTIAL = STOKES_PARTIAL_RADII + STOKES_COMPONENTS * STOKES_RADII_MAX;      // doubles of a partial record

static_assert(STOKES_PARTIAL <= STOKES_FINISH_THREADS, "the second launch has a lane per double of a partial record");

inline int stokes_record_doubles(int n_radii) { return STOKES_ENC + STOKES_COMPONENTS * n_radii; }

// What the entry knows of the active plan when it checks a call.
struct StokesState {
    bool have_result = false, have_stokes = false;
    int T = 0, result_sets = 0;
};

// The argument checks of ml_propagate_stokes.  -> 0; -1: an argument error, -2: the state does not allow the call; `why`
// is filled then.  source >= 0: member of the last pass, -1: the Stokes sums.  centre: [planes][2], or NULL where no
// radius asks for one.
inline int stokes_check(const StokesState &s, int source, int mx, int my, int planes, double dx, double dy, const double *centre,
                        const double *radii, int n_radii, int record_doubles, char *why, size_t why_len) {
    if (!s.have_result) {
        snprintf(why, why_len, "ml_propagate has not run on the active propagation plan");
        return -2;
    }
    if (source < -1) {
        snprintf(why, why_len, "ml_propagate_stokes: source %d: a member of the last pass (>= 0) or -1 for the Stokes sums", source);
        return -1;
    }
    if (source == -1 && !s.have_stokes) {
        snprintf(why, why_len, "ml_propagate_accumulate_stokes has not run on the active propagation plan");
        return -2;
    }
    if (source >= s.result_sets) {
        snprintf(why, why_len, "ml_propagate_stokes: member %d asked for, the last pass propagated %d field sets", source,
                 s.result_sets);
        return -1;
    }
    if (mx < 1 || my < 1 || planes < 1 || (long long)mx * my * planes != s.T) {
        snprintf(why, why_len, "ml_propagate_stokes: %d planes of %d x %d targets are %lld targets, the active propagation plan "
                 "has %d", planes, mx, my, (long long)mx * my * planes, s.T);
        return -1;
    }
    if (!(dx > 0) || !(dy > 0) || !std::isfinite(dx) || !std::isfinite(dy)) {
        snprintf(why, why_len, "ml_propagate_stokes: the targets' pitch must be finite and > 0, got dx = %g, dy = %g", dx, dy);
        return -1;
    }
    if (n_radii < 0 || n_radii > STOKES_RADII_MAX) {
        snprintf(why, why_len, "ml_propagate_stokes: %d radii: 0 to %d are taken", n_radii, STOKES_RADII_MAX);
        return -1;
    }
    if (n_radii > 0 && !radii) {
        snprintf(why, why_len, "ml_propagate_stokes: %d radii asked for, radii is NULL", n_radii);
        return -1;
    }
    if (n_radii > 0 && !centre) {
        snprintf(why, why_len, "ml_propagate_stokes: %d radii asked for, centre is NULL (it may be only where n_radii = 0)", n_radii);
        return -1;
    }
    for (int r = 0; r < n_radii; ++r) {
        if (!std::isfinite(radii[r]) || radii[r] < 0) {
            snprintf(why, why_len, "ml_propagate_stokes: radii[%d] = %g: a radius must be finite and >= 0", r, radii[r]);
            return -1;
        }
        if (r > 0 && radii[r] < radii[r - 1]) {
            snprintf(why, why_len, "ml_propagate_stokes: the radii must not decrease: radii[%d] = %g < radii[%d] = %g", r,
                     radii[r], r - 1, radii[r - 1]);
            return -1;
        }
    }
    if (centre)
        for (int p = 0; p < planes; ++p)
            if (!std::isfinite(centre[2 * p]) || !std::isfinite(centre[2 * p + 1])) {
                snprintf(why, why_len, "ml_propagate_stokes: the centre of plane %d is (%g, %g): it must be finite", p,
                         centre[2 * p], centre[2 * p + 1]);
                return -1;
            }
    if (record_doubles < stokes_record_doubles(n_radii)) {
        snprintf(why, why_len, "ml_propagate_stokes: a record of %d radii has %d doubles, record_doubles = %d", n_radii,
                 stokes_record_doubles(n_radii), record_doubles);
        return -1;
    }
    return 0;
}

}  // namespace ml
