// What the passes over the resident near field share on the host - the per-zone sums (fields_zones.h), the Zernike moments
// (fields_wavefront.h) and the pupil function (fields_pupil.h): the state an entry checks a call against, the constants of a
// line launch, the vertex and the reach of the reference wave, the argument checks with their wording, and the packing of
// several host arrays into one upload.  Free of HIP types, as the three headers that build on it.
//
// Every pass walks the aperture the same way: line i (fixed x, j contiguous) belongs to one wave, PASS_LINE_THREADS / 64
// lines to a workgroup, and the wave takes the line in blocks of PASS_BLOCK = 64 samples in ascending order, lane l the sample
// 64 b + l.  A sample's squared distance from the centre is X2[i] + Y2[j] - one rounded addition - and Y2 falls to one
// minimum, the vertex, and rises again (pass_check_vertex), so the samples inside a radius are one interval of a line.
//
// The reference wave of the zone sums and the Zernike moments has the phase  phi = ra[i] + rb[j]  (PASS_REF_PLANE)  or
// phi = sk sqrt((ra[i] + rb[j]) + ref_c ref_c), sk = -sign(ref_c) k, by the correctly rounded square root (PASS_REF_FOCUS).
//
// A check hands back 0, or -1 for an argument error or -2 where the state does not allow the call, with the message in
// the caller's buffer; the message begins with the entry's name.  An entry's check function is a sequence of them in a
// fixed order: the first that fails decides the message.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#if defined(__HIPCC__)
#define ML_PASS_HD __host__ __device__
#else
#define ML_PASS_HD
#endif

namespace ml {

constexpr int PASS_SETS_MAX = 3;         // field sets per call (the members of a synthesis batch)
constexpr int PASS_BLOCK = 64;           // samples of a block: one per lane of a wave
constexpr int PASS_LINE_THREADS = 256;   // lanes of a workgroup of a line launch: four lines
constexpr int PASS_REF_PLANE = 0, PASS_REF_FOCUS = 1;
constexpr double PASS_PHASE_LIMIT = 1e9; // common.h PHASE_LIMIT (fields_dev.h asserts that they agree)

// blocks of a line of ny samples
ML_PASS_HD inline int pass_blocks(int ny) { return (ny + PASS_BLOCK - 1) / PASS_BLOCK; }

// the first minimum of y2 (the vertex of every line)
inline int pass_vertex(const double *y2, int ny) {
    int jv = 0;
    for (int j = 1; j < ny; ++j)
        if (y2[j] < y2[jv]) jv = j;
    return jv;
}

// the largest |phi| the reference wave reaches over the grid: |phi| is monotone in ra[i] + rb[j], a rounded sum
inline double pass_phase_max(int ref_mode, const double *ra, int nx, const double *rb, int ny, double ref_c, double k) {
    double a_lo = ra[0], a_hi = ra[0], b_lo = rb[0], b_hi = rb[0];
    for (int i = 1; i < nx; ++i) {
        a_lo = ra[i] < a_lo ? ra[i] : a_lo;
        a_hi = ra[i] > a_hi ? ra[i] : a_hi;
    }
    for (int j = 1; j < ny; ++j) {
        b_lo = rb[j] < b_lo ? rb[j] : b_lo;
        b_hi = rb[j] > b_hi ? rb[j] : b_hi;
    }
    if (ref_mode == PASS_REF_PLANE) return std::fmax(std::fabs(a_lo + b_lo), std::fabs(a_hi + b_hi));
    return k * std::sqrt((a_hi + b_hi) + ref_c * ref_c);
}

// What an entry knows of the context when it checks a call.
struct PassState {
    int n_ranks = 1;
    int nx = 0, ny = 0, n_sets = 0;   // the resident field sets (nx = 0: none)
};

// Several host arrays in one upload: add() appends n doubles - copies of v, or room to be filled where v is NULL - and
// hands back where they begin.  An entry states its layout once, as its sequence of add(): the host vector and the device
// pointers come from the same offsets.
struct PassPack {
    std::vector<double> h;
    size_t add(const double *v, size_t n) {
        const size_t at = h.size();
        h.resize(at + n);
        if (v) std::copy(v, v + n, h.begin() + at);
        return at;
    }
    size_t bytes() const { return h.size() * sizeof(double); }
};

// Where a refusal goes: the entry's name, which leads the message, and the caller's buffer.
struct PassWhy {
    const char *who;
    char *why;
    size_t len;
};

// "<entry>: <message>" -> rc
#if defined(__GNUC__)
__attribute__((format(printf, 3, 4)))
#endif
static inline int pass_refuse(const PassWhy &w, int rc, const char *fmt, ...) {
    const int at = snprintf(w.why, w.len, "%s: ", w.who);
    if (at >= 0 && (size_t)at < w.len) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(w.why + at, w.len - at, fmt, ap);
        va_end(ap);
    }
    return rc;
}

// every v[i] finite, and >= 0 where nonneg
static inline int pass_check_range(const PassWhy &w, const char *name, const double *v, int n, bool nonneg, const char *what) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i]) || (nonneg && v[i] < 0)) return pass_refuse(w, -1, "%s[%d] = %g: %s", name, i, v[i], what);
    return 0;
}

static inline int pass_check_comm(const PassWhy &w, int n_ranks) {
    return n_ranks > 1 ? pass_refuse(w, -1, "this context belongs to a communicator of %d ranks", n_ranks) : 0;
}

static inline int pass_check_set_count(const PassWhy &w, int n_sets) {
    if (n_sets < 1 || n_sets > PASS_SETS_MAX) return pass_refuse(w, -1, "a pass takes 1 to %d field sets, got %d", PASS_SETS_MAX, n_sets);
    return 0;
}

static inline int pass_check_edge_count(const PassWhy &w, int n_edges, int least, int most) {
    if (n_edges < least || n_edges > most) return pass_refuse(w, -1, "%d edges: %d to %d are taken", n_edges, least, most);
    return 0;
}

static inline int pass_check_ref_mode(const PassWhy &w, int ref_mode) {
    if (ref_mode != PASS_REF_PLANE && ref_mode != PASS_REF_FOCUS)
        return pass_refuse(w, -1, "ref_mode %d: %d for a plane wave or %d for a focus", ref_mode, PASS_REF_PLANE, PASS_REF_FOCUS);
    return 0;
}

static inline int pass_check_axes(const PassWhy &w, int nx, int ny) {
    return nx < 1 || ny < 1 ? pass_refuse(w, -1, "the axes have %d x %d samples: at least one each", nx, ny) : 0;
}

// a field set is resident (the one message without the entry's name)
static inline int pass_check_resident(const PassWhy &w, const PassState &s) {
    if (s.nx != 0 && s.ny != 0) return 0;
    snprintf(w.why, w.len, "no resident field set");
    return -2;
}

static inline int pass_check_shape(const PassWhy &w, const PassState &s, int nx, int ny) {
    if (nx != s.nx || ny != s.ny)
        return pass_refuse(w, -1, "the axes have %d x %d samples, the resident field sets %d x %d", nx, ny, s.nx, s.ny);
    return 0;
}

static inline int pass_check_set_range(const PassWhy &w, const PassState &s, int first_set, int n_sets) {
    if (first_set < 0 || first_set + n_sets > s.n_sets)
        return pass_refuse(w, -1, "field sets %d ... %d asked for, %d resident", first_set, first_set + n_sets - 1, s.n_sets);
    return 0;
}

static inline int pass_check_squared_axes(const PassWhy &w, const double *x2, int nx, const double *y2, int ny) {
    const char *sq = "a squared distance must be finite and >= 0";
    if (int rc = pass_check_range(w, "x2", x2, nx, true, sq)) return rc;
    return pass_check_range(w, "y2", y2, ny, true, sq);
}

// y2 falls to its vertex and rises again
static inline int pass_check_vertex(const PassWhy &w, const double *y2, int ny) {
    const int jv = pass_vertex(y2, ny);
    for (int j = 1; j < ny; ++j)
        if (j <= jv ? y2[j] > y2[j - 1] : y2[j] < y2[j - 1])
            return pass_refuse(w, -1, "y2 must fall to its minimum y2[%d] = %g and rise again (a y axis in ascending or descending "
                               "order): y2[%d] = %g follows y2[%d] = %g", jv, y2[jv], j, y2[j], j - 1, y2[j - 1]);
    return 0;
}

// squared edges, ascending (none: nothing to check)
static inline int pass_check_edges(const PassWhy &w, const double *e2, int n_edges) {
    if (int rc = pass_check_range(w, "e2", e2, n_edges, true, "a squared edge must be finite and >= 0")) return rc;
    for (int z = 1; z < n_edges; ++z)
        if (e2[z] < e2[z - 1])
            return pass_refuse(w, -1, "the edges must not decrease: e2[%d] = %g < e2[%d] = %g", z, e2[z], z - 1, e2[z - 1]);
    return 0;
}

static inline int pass_check_radius(const PassWhy &w, double r2) {
    if (!(std::isfinite(r2) && r2 > 0)) return pass_refuse(w, -1, "r2 = %g: the squared radius of the pupil must be finite and > 0", r2);
    return 0;
}

static inline int pass_check_pupil_axes(const PassWhy &w, const double *xi, int nx, const double *eta, int ny) {
    const char *co = "a pupil coordinate must be finite";
    if (int rc = pass_check_range(w, "xi", xi, nx, false, co)) return rc;
    return pass_check_range(w, "eta", eta, ny, false, co);
}

// the reference wave of an accepted ref_mode: its per-axis arrays, ref_c and k of a focus, and the phase it reaches
static inline int pass_check_ref_wave(const PassWhy &w, int ref_mode, const double *ra, int nx, const double *rb, int ny, double ref_c,
                                      double k) {
    const bool focus = ref_mode == PASS_REF_FOCUS;
    const char *rw = focus ? "a squared distance to the focus must be finite and >= 0" : "a reference phase must be finite";
    if (int rc = pass_check_range(w, "ra", ra, nx, focus, rw)) return rc;
    if (int rc = pass_check_range(w, "rb", rb, ny, focus, rw)) return rc;
    if (focus && (!std::isfinite(ref_c) || ref_c == 0))
        return pass_refuse(w, -1, "ref_c = %g: the focus lies at a finite distance zf != 0 from the aperture", ref_c);
    if (focus && !(std::isfinite(k) && k > 0)) return pass_refuse(w, -1, "k = %g: the wave number must be finite and > 0", k);
    const double phi = pass_phase_max(ref_mode, ra, nx, rb, ny, ref_c, k);
    if (!(phi <= PASS_PHASE_LIMIT))
        return pass_refuse(w, -1, "the reference phase reaches %.6g rad on this grid: the phase arithmetic covers up to %g", phi,
                           PASS_PHASE_LIMIT);
    return 0;
}

}  // namespace ml
