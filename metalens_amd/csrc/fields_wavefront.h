// Plan arithmetic, coefficient table, host conversion and argument checks of the Zernike moments of the resident near
// field's wavefront (fields_wavefront.hip, ml_fields_zernike), on the host and free of HIP types (as fields_zones.h):
// tools/fields_wavefront_plan.cpp and tests/test_fields_wavefront_host.py run it without a GPU.
//
// Pupil.  A disc of radius R > 0 about centre = (xc, yc).  The host hands over X2[i] = (x[i] - xc)^2, Y2[j] = (y[j] - yc)^2 and
// R2 = R R, and xi[i] = (x[i] - xc) / R, eta[j] = (y[j] - yc) / R.  Sample (i, j) is a member iff X2[i] + Y2[j] <= R2 - one
// rounded addition, a sample on the rim is inside.  Y2 must fall to one minimum and rise again (fields_pass.h), so a line's
// members are one interval of j.
//
// Terms of a member, per field set, every operation rounded on its own (nothing is contracted into an FMA): S, Ix, Iy,
// Cx = Ex conj(w) and Cy as fields_zones.h defines them (the device forms them by the same functions, fields_dev.h), with the
// reference waves, ra, rb, ref_c, k and the refusal of a phase beyond PASS_PHASE_LIMIT of fields_pass.h.
//
// Zernike terms up to radial order n_max, 0 <= n_max <= WF_ORDER_MAX = 8: J = (n_max + 1)(n_max + 2) / 2 terms, 45 at the
// most, in OSA/ANSI order, j = (n (n + 2) + m) / 2 with m = -n, -n + 2, ... n, m < 0 the sine term, with Noll normalisation
// N_j = sqrt(n + 1) for m = 0 and sqrt(2 (n + 1)) otherwise: (1 / pi) int Z_j Z_k d^2 rho = delta_jk on the unit disc.
//
// The record of a field set has 4 + 4 J doubles: [WF_N] the members, [WF_S] sum S, [WF_IX] sum Ix, [WF_IY] sum Iy, then per
// term j at WF_HEAD + 4 j: Re, Im of sum Cx Z_j and Re, Im of sum Cy Z_j over the members, without the factor dA.
//
// How the sums are formed - part of the definition, because it fixes the bits.  Z_j / N_j is a polynomial in (xi, eta) with
// integer coefficients A_j,pq (wf_coefficients; all far below 2^53, exact in a double), so
//   sum C Z_j = N_j sum_pq A_j,pq M_pq,   M_pq = sum_i xi[i]^p T_q(i),   T_q(i) = sum_j C(i, j) eta[j]^q :
// per sample n_max + 1 multiply-adds per real component instead of J, no atan2 and no per-term trigonometry.
//   1. Line i (fixed x, j contiguous) is taken by one wave in blocks of PASS_BLOCK = 64 samples in ascending order; lane l
//      holds the samples l + 64 b.  Per member the powers eta^0 = 1, eta^q = eta^(q - 1) eta come by repeated multiplication,
//      and the lane adds C eta^q (and S, Ix, Iy) onto accumulators that start at +0.0; a non-member adds nothing.
//   2. At the line's end one butterfly per accumulator over the 64 lanes (lanes 32, 16, 8, 4, 2, 1 apart); the line record
//      has WF_HEAD + 4 (n_max + 1) doubles per set: [n, sum S, sum Ix, sum Iy], then per q Re, Im T_q of Cx and of Cy.  A
//      line whose vertex - the first minimum of Y2 - lies outside the pupil stores zeros.
//   3. A second launch takes one workgroup of WF_SUM_THREADS = 256 lanes per (set, q), and one more per set for the
//      header sums: lane l visits the lines l, l + 256, ... that hold members in ascending order, forms xi^0 = 1,
//      xi^p = xi^(p - 1) xi by repeated multiplication and adds xi^p T_q, for every p <= n_max - q, onto +0.0; then a
//      butterfly over each wave and the four waves in their order, ((w0 + w1) + w2) + w3.
//   4. The host (wf_convert) adds A_j,pq M_pq over the non-zero coefficients of term j in ascending (p, then q) order onto
//      +0.0 and multiplies once by the correctly rounded N_j.
// No step depends on n_max beyond which (p, q) exist, on the other sets of the call or on an earlier call: the first J'
// terms of a call of higher order have the bits of the call of order n' alone, the record of a set the same bits whatever
// the other sets are, and two calls agree to the bit.
#pragma once

#include "fields_zones.h"

namespace ml {

constexpr int WF_ORDER_MAX = 8;          // n_max at the most
constexpr int WF_TERMS_MAX = 45;         // J at n_max = 8
constexpr int WF_SUM_THREADS = 256;      // lanes of a workgroup of the second launch
constexpr int WF_N = 0, WF_S = 1, WF_IX = 2, WF_IY = 3;
constexpr int WF_HEAD = 4;               // doubles of the header sums

// terms up to radial order n_max, and the doubles of a record
ML_PASS_HD inline int wf_terms(int n_max) { return (n_max + 1) * (n_max + 2) / 2; }
inline int wf_record(int n_max) { return WF_HEAD + 4 * wf_terms(n_max); }

// doubles of a line record of one set: the header sums and Re, Im of T_q of Cx and Cy for q = 0 ... n_max
ML_PASS_HD inline int wf_line_record(int n_max) { return WF_HEAD + 4 * (n_max + 1); }

// where the monomial moment M_pq, p + q <= n_max, lies among the wf_terms(n_max) moments of a set: ascending p, then q
ML_PASS_HD inline int wf_monomial(int n_max, int p, int q) { return p * (n_max + 1) - p * (p - 1) / 2 + q; }

// bytes of scratch of a call: the line records of every set
inline long long wf_scratch_bytes(int sets, int nx, int n_max) { return (long long)sets * nx * wf_line_record(n_max) * 8; }

// OSA/ANSI: the radial order and azimuthal frequency of term j, and back
inline void wf_term(int j, int &n, int &m) {
    n = 0;
    while ((n + 1) * (n + 2) / 2 <= j) ++n;
    m = 2 * j - n * (n + 2);
}
inline int wf_index(int n, int m) { return (n * (n + 2) + m) / 2; }

// N_j, correctly rounded (the square root of a small integer)
inline double wf_norm(int n, int m) { return std::sqrt(m == 0 ? (double)(n + 1) : 2.0 * (n + 1)); }

static inline long long wf_factorial(int v) {
    long long f = 1;
    for (int i = 2; i <= v; ++i) f *= i;
    return f;
}
static inline long long wf_binomial(int n, int k) { return wf_factorial(n) / (wf_factorial(k) * wf_factorial(n - k)); }

// The integer coefficients of Z_j / N_j = R_n^|m|(rho) cos(m phi) (m >= 0) or R_n^|m|(rho) sin(|m| phi) (m < 0) as a
// polynomial in xi = rho cos phi, eta = rho sin phi: A[p][q] multiplies xi^p eta^q.  From
//   R_n^a(rho) = sum_s (-1)^s (n - s)! / (s! ((n + a) / 2 - s)! ((n - a) / 2 - s)!) rho^(n - 2 s),
//   rho^(n - 2 s) cos / sin(a phi) = (xi^2 + eta^2)^t Re / Im (xi + i eta)^a,  t = (n - a) / 2 - s.
inline void wf_coefficients(int n, int m, long long A[WF_ORDER_MAX + 1][WF_ORDER_MAX + 1]) {
    for (int p = 0; p <= WF_ORDER_MAX; ++p)
        for (int q = 0; q <= WF_ORDER_MAX; ++q) A[p][q] = 0;
    const int a = m < 0 ? -m : m;
    for (int s = 0; s <= (n - a) / 2; ++s) {
        const int t = (n - a) / 2 - s;
        long long rad = wf_factorial(n - s) / (wf_factorial(s) * wf_factorial((n + a) / 2 - s) * wf_factorial(t));
        if (s & 1) rad = -rad;
        for (int i = 0; i <= t; ++i)                                   // (xi^2 + eta^2)^t: C(t, i) xi^(2 i) eta^(2 (t - i))
            for (int k = m < 0 ? 1 : 0; k <= a; k += 2) {              // Re: even k, Im: odd k, of C(a, k) xi^(a - k) (i eta)^k
                const long long sign = ((k >> 1) & 1) ? -1 : 1;
                A[2 * i + a - k][2 * (t - i) + k] += rad * wf_binomial(t, i) * sign * wf_binomial(a, k);
            }
    }
}

// The record of one field set from its monomial moments: mono = [WF_HEAD header sums][wf_terms(n_max)][4], the moments in the
// order of wf_monomial; rec gets wf_record(n_max) doubles.
inline void wf_convert(const double *mono, int n_max, double *rec) {
    for (int c = 0; c < WF_HEAD; ++c) rec[c] = mono[c];
    long long A[WF_ORDER_MAX + 1][WF_ORDER_MAX + 1];
    for (int j = 0; j < wf_terms(n_max); ++j) {
        int n, m;
        wf_term(j, n, m);
        wf_coefficients(n, m, A);
        const double norm = wf_norm(n, m);
        for (int c = 0; c < 4; ++c) {
            double acc = 0.0;
            for (int p = 0; p <= n; ++p)
                for (int q = 0; p + q <= n; ++q)
                    if (A[p][q] != 0) acc += (double)A[p][q] * mono[WF_HEAD + 4 * wf_monomial(n_max, p, q) + c];
            rec[WF_HEAD + 4 * j + c] = norm * acc;
        }
    }
}

static inline int wf_check_order(const PassWhy &w, int n_max) {
    if (n_max < 0 || n_max > WF_ORDER_MAX) return pass_refuse(w, -1, "n_max = %d: radial orders 0 to %d are taken", n_max, WF_ORDER_MAX);
    return 0;
}

// The argument checks of ml_fields_zernike.  -> 0; -1: an argument error, -2: the state does not allow the call; `why` is
// filled then.
inline int wf_check(const PassState &s, int first_set, int n_sets, const double *x2, const double *xi, int nx, const double *y2,
                    const double *eta, int ny, double r2, int n_max, int ref_mode, const double *ra, const double *rb, double ref_c,
                    double k, int record_doubles, char *why, size_t why_len) {
    const PassWhy w{"ml_fields_zernike", why, why_len};
    if (int rc = pass_check_comm(w, s.n_ranks)) return rc;
    if (int rc = pass_check_set_count(w, n_sets)) return rc;
    if (int rc = wf_check_order(w, n_max)) return rc;
    if (int rc = pass_check_ref_mode(w, ref_mode)) return rc;
    if (record_doubles < wf_record(n_max))
        return pass_refuse(w, -1, "record_doubles = %d: a record of order %d has %d doubles", record_doubles, n_max, wf_record(n_max));
    if (int rc = pass_check_axes(w, nx, ny)) return rc;
    if (!x2 || !xi || !y2 || !eta || !ra || !rb) return pass_refuse(w, -1, "NULL argument");
    if (int rc = pass_check_resident(w, s)) return rc;
    if (int rc = pass_check_shape(w, s, nx, ny)) return rc;
    if (int rc = pass_check_set_range(w, s, first_set, n_sets)) return rc;
    if (int rc = pass_check_radius(w, r2)) return rc;
    if (int rc = pass_check_squared_axes(w, x2, nx, y2, ny)) return rc;
    if (int rc = pass_check_pupil_axes(w, xi, nx, eta, ny)) return rc;
    if (int rc = pass_check_vertex(w, y2, ny)) return rc;
    return pass_check_ref_wave(w, ref_mode, ra, nx, rb, ny, ref_c, k);
}

}  // namespace ml
