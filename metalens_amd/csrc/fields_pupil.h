// Plan arithmetic and argument checks of the pupil function applied to the resident near field (fields_pupil.hip,
// ml_fields_pupil_plan / ml_fields_pupil_apply), on the host and free of HIP types (as fields_wavefront.h):
// tools/fields_pupil_plan.cpp and tests/test_fields_pupil_host.py run it without a GPU.
//
// Pupil.  A disc of radius R > 0 about centre = (xc, yc), with X2, Y2, xi, eta and R2 = R R as fields_wavefront.h forms
// them.  Sample (i, j) has r2 = X2[i] + Y2[j] - one rounded addition - and is a member iff r2 <= R2; a sample on the rim is
// inside.  Y2 must fall to one minimum and rise again.
//
// The pupil function has three parts, each optional:
//   stop     every field of a non-member becomes +0.0 + 0.0i.
//   zones    K <= PUPIL_EDGES_MAX ascending squared edges E2 with K complex factors g[z]: sample (i, j) lies in zone
//            z = searchsorted(E2, r2, 'left') - the rule of fields_zones.h, a sample on an edge belongs to the inner zone -
//            and takes g[z] for z < K.  Outside every edge (z = K), and without edges, the zone factor is exactly 1.
//   phase    J = (n_max + 1)(n_max + 2) / 2 real coefficients c_j in radians, in the order of wf_term, n_max <= 8: a
//            member takes exp(+i psi), psi = sum_j c_j Z_j(xi, eta).  A non-member takes no phase: a Zernike polynomial
//            means nothing outside its disc.
// Which samples change:
//   a stopped non-member (stop)                                        -> +0.0 + 0.0i, never read
//   a member with a phase, or any sample left standing in a zone z < K -> E f, f as below
//   every other sample - its factor is exactly 1 -                     -> neither read nor written: it keeps its bytes
//
// How psi and the product are formed - part of the definition, because it fixes the values; every operation is rounded
// on its own (nothing is contracted into an FMA):
//   1. pupil_monomials: B_pq = sum_j (c_j N_j) A_j,pq over the terms whose A_j,pq is not 0, j ascending, onto +0.0, with
//      A = wf_coefficients and N = wf_norm; p + q <= n_max.
//   2. pupil_line_table: per line i and q = 0 ... n_max, b_q(i) = sum_p B_pq xi[i]^p by Horner, p descending from
//      n_max - q: b = B_(n_max - q)q, then b = b xi + B_pq.  A line holds PUPIL_NQ = 9 entries, +0.0 beyond n_max.
//   3. per member psi = sum_q b_q(i) eta[j]^q by Horner, q descending (leading +0.0 entries change nothing), and
//      (cs, sn) = sincos_cw(psi).
//   4. f = g (cs + i sn): fr = g.r cs - g.i sn, fi = g.r sn + g.i cs, with g = 1 + 0i where the zone factor is exactly 1;
//      without a phase f = g.
//   5. each of Ex, Ey, Hx, Hy becomes (E.r fr - E.i fi) + i (E.r fi + E.i fr).
// |psi| <= sum_pq |B_pq| on the unit disc; a plan whose sum exceeds PUPIL_PHASE_LIMIT is refused.
#pragma once

#include "fields_wavefront.h"

namespace ml {

constexpr int PUPIL_ORDER_MAX = WF_ORDER_MAX;
constexpr int PUPIL_NQ = WF_ORDER_MAX + 1;     // entries of a line of the table
constexpr int PUPIL_EDGES_MAX = ZONES_EDGES_MAX;
constexpr int PUPIL_SETS_MAX = WF_SETS_MAX;    // field sets per launch (the members of a synthesis batch)
constexpr int PUPIL_BLOCK = 64;                // samples of a block: one per lane of a wave
constexpr int PUPIL_LINE_THREADS = 256;        // lanes of a workgroup: four lines
constexpr double PUPIL_PHASE_LIMIT = WF_PHASE_LIMIT;

// B[p * PUPIL_NQ + q] = B_pq; every entry is written (+0.0 where p + q > n_max).  c: wf_terms(n_max) coefficients, or
// nullptr for no phase (all +0.0)
inline void pupil_monomials(int n_max, const double *c, double *B) {
    for (int k = 0; k < PUPIL_NQ * PUPIL_NQ; ++k) B[k] = 0.0;
    if (!c) return;
    long long A[WF_ORDER_MAX + 1][WF_ORDER_MAX + 1];
    for (int j = 0; j < wf_terms(n_max); ++j) {
        int n, m;
        wf_term(j, n, m);
        wf_coefficients(n, m, A);
        const double cn = c[j] * wf_norm(n, m);
        for (int p = 0; p <= n; ++p)
            for (int q = 0; p + q <= n; ++q)
                if (A[p][q] != 0) B[p * PUPIL_NQ + q] += cn * (double)A[p][q];
    }
}

// sum_pq |B_pq|: what |psi| cannot exceed on the unit disc
inline double pupil_phase_bound(const double *B) {
    double s = 0.0;
    for (int k = 0; k < PUPIL_NQ * PUPIL_NQ; ++k) s += std::fabs(B[k]);
    return s;
}

// table[i * PUPIL_NQ + q] = b_q(i)
inline void pupil_line_table(int n_max, const double *B, const double *xi, int nx, double *table) {
    for (int i = 0; i < nx; ++i)
        for (int q = 0; q < PUPIL_NQ; ++q) {
            double b = 0.0;
            if (q <= n_max) {
                b = B[(n_max - q) * PUPIL_NQ + q];
                for (int p = n_max - q - 1; p >= 0; --p) b = b * xi[i] + B[p * PUPIL_NQ + q];
            }
            table[(size_t)i * PUPIL_NQ + q] = b;
        }
}

// doubles a plan uploads: x2 [nx], y2, eta [ny], the line table [nx][PUPIL_NQ], e2 [K], g [K][2]
inline long long pupil_plan_doubles(int nx, int ny, int K) { return (long long)nx * (1 + PUPIL_NQ) + 2LL * ny + 3LL * K; }

// What a plan leaves in the context besides its arrays.
struct PupilPlan {
    bool valid = false;
    int nx = 0, ny = 0, K = 0, jv = 0;
    int nq = 0;   // 0: no phase; 5: n_max <= 4; 9: the orders up to 8 - the instantiations of the kernel
    int stop = 0;
    double r2 = 0.0;
};

static inline bool pupil_bad(const char *name, const double *v, int n, bool nonneg, const char *what, char *why, size_t why_len) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i]) || (nonneg && v[i] < 0)) {
            snprintf(why, why_len, "ml_fields_pupil_plan: %s[%d] = %g: %s", name, i, v[i], what);
            return true;
        }
    return false;
}

// The argument checks of ml_fields_pupil_plan; B gets pupil_monomials of an accepted call.  -> 0, or -1 with `why` filled.
inline int pupil_check(int n_ranks, const double *x2, const double *xi, int nx, const double *y2, const double *eta, int ny, double r2,
                       int stop, int n_max, const double *c, const double *e2, int n_edges, const double *g, double *B, char *why,
                       size_t why_len) {
    if (n_ranks > 1) {
        snprintf(why, why_len, "ml_fields_pupil_plan: this context belongs to a communicator of %d ranks", n_ranks);
        return -1;
    }
    if (stop != 0 && stop != 1) {
        snprintf(why, why_len, "ml_fields_pupil_plan: stop = %d: 0 to leave the samples outside the pupil standing or 1 to clear them", stop);
        return -1;
    }
    if (n_max < 0 || n_max > PUPIL_ORDER_MAX) {
        snprintf(why, why_len, "ml_fields_pupil_plan: n_max = %d: radial orders 0 to %d are taken", n_max, PUPIL_ORDER_MAX);
        return -1;
    }
    if (n_edges < 0 || n_edges > PUPIL_EDGES_MAX) {
        snprintf(why, why_len, "ml_fields_pupil_plan: %d edges: 0 to %d are taken", n_edges, PUPIL_EDGES_MAX);
        return -1;
    }
    if (nx < 1 || ny < 1) {
        snprintf(why, why_len, "ml_fields_pupil_plan: the axes have %d x %d samples: at least one each", nx, ny);
        return -1;
    }
    if (!x2 || !xi || !y2 || !eta || (n_edges > 0 && (!e2 || !g))) {
        snprintf(why, why_len, "ml_fields_pupil_plan: NULL argument");
        return -1;
    }
    if (!(std::isfinite(r2) && r2 > 0)) {
        snprintf(why, why_len, "ml_fields_pupil_plan: r2 = %g: the squared radius of the pupil must be finite and > 0", r2);
        return -1;
    }
    const char *sq = "a squared distance must be finite and >= 0";
    if (pupil_bad("x2", x2, nx, true, sq, why, why_len) || pupil_bad("y2", y2, ny, true, sq, why, why_len)) return -1;
    const char *co = "a pupil coordinate must be finite";
    if (pupil_bad("xi", xi, nx, false, co, why, why_len) || pupil_bad("eta", eta, ny, false, co, why, why_len)) return -1;
    const int jv = zones_vertex(y2, ny);
    for (int j = 1; j < ny; ++j)
        if (j <= jv ? y2[j] > y2[j - 1] : y2[j] < y2[j - 1]) {
            snprintf(why, why_len, "ml_fields_pupil_plan: y2 must fall to its minimum y2[%d] = %g and rise again (a y axis in ascending or "
                     "descending order): y2[%d] = %g follows y2[%d] = %g", jv, y2[jv], j, y2[j], j - 1, y2[j - 1]);
            return -1;
        }
    if (n_edges > 0) {
        if (pupil_bad("e2", e2, n_edges, true, "a squared edge must be finite and >= 0", why, why_len)) return -1;
        for (int z = 1; z < n_edges; ++z)
            if (e2[z] < e2[z - 1]) {
                snprintf(why, why_len, "ml_fields_pupil_plan: the edges must not decrease: e2[%d] = %g < e2[%d] = %g", z, e2[z], z - 1,
                         e2[z - 1]);
                return -1;
            }
        for (int z = 0; z < n_edges; ++z)
            if (!std::isfinite(g[2 * z]) || !std::isfinite(g[2 * z + 1])) {
                snprintf(why, why_len, "ml_fields_pupil_plan: g[%d] = (%g, %g): a zone factor must be finite", z, g[2 * z], g[2 * z + 1]);
                return -1;
            }
    }
    if (c && pupil_bad("c", c, wf_terms(n_max), false, "a phase coefficient must be finite", why, why_len)) return -1;
    pupil_monomials(n_max, c, B);
    const double psi = pupil_phase_bound(B);
    if (!(psi <= PUPIL_PHASE_LIMIT)) {
        snprintf(why, why_len, "ml_fields_pupil_plan: the phase plate can reach %.6g rad on the unit disc: the phase arithmetic covers up "
                 "to %g", psi, PUPIL_PHASE_LIMIT);
        return -1;
    }
    return 0;
}

// The checks of ml_fields_pupil_apply against the plan and the resident field sets (fields_zones.h ZonesState).  -> 0; -1: an
// argument error, -2: the state does not allow the call; `why` is filled then.
inline int pupil_apply_check(const ZonesState &s, const PupilPlan &plan, int first_set, int n_sets, char *why, size_t why_len) {
    if (s.n_ranks > 1) {
        snprintf(why, why_len, "ml_fields_pupil_apply: this context belongs to a communicator of %d ranks", s.n_ranks);
        return -1;
    }
    if (n_sets < 1 || n_sets > PUPIL_SETS_MAX) {
        snprintf(why, why_len, "ml_fields_pupil_apply: a pass takes 1 to %d field sets, got %d", PUPIL_SETS_MAX, n_sets);
        return -1;
    }
    if (!plan.valid) {
        snprintf(why, why_len, "ml_fields_pupil_apply: no pupil has been planned on this context (ml_fields_pupil_plan)");
        return -2;
    }
    if (s.nx == 0 || s.ny == 0) {
        snprintf(why, why_len, "no resident field set");
        return -2;
    }
    if (plan.nx != s.nx || plan.ny != s.ny) {
        snprintf(why, why_len, "ml_fields_pupil_apply: the pupil was planned for %d x %d samples, the resident field sets have %d x %d",
                 plan.nx, plan.ny, s.nx, s.ny);
        return -2;
    }
    if (first_set < 0 || first_set + n_sets > s.n_sets) {
        snprintf(why, why_len, "ml_fields_pupil_apply: field sets %d ... %d asked for, %d resident", first_set, first_set + n_sets - 1,
                 s.n_sets);
        return -1;
    }
    return 0;
}

}  // namespace ml
