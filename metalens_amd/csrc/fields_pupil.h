// Plan arithmetic and argument checks of the pupil function applied to the resident near field (fields_pupil.hip,
// ml_fields_pupil_plan / ml_fields_pupil_apply), on the host and free of HIP types (as fields_wavefront.h):
// tools/fields_pupil_plan.cpp and tests/test_fields_pupil_host.py run it without a GPU.
//
// Pupil.  A disc of radius R > 0 about centre = (xc, yc), with X2, Y2, xi, eta and R2 = R R as fields_wavefront.h forms
// them.  Sample (i, j) has r2 = X2[i] + Y2[j] - one rounded addition - and is a member iff r2 <= R2; a sample on the rim is
// inside.  Y2 must fall to one minimum and rise again (fields_pass.h).
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
// |psi| <= sum_pq |B_pq| on the unit disc; a plan whose sum exceeds PASS_PHASE_LIMIT is refused.
#pragma once

#include "fields_wavefront.h"

namespace ml {

constexpr int PUPIL_ORDER_MAX = WF_ORDER_MAX;
constexpr int PUPIL_NQ = WF_ORDER_MAX + 1;     // entries of a line of the table
constexpr int PUPIL_EDGES_MAX = ZONES_EDGES_MAX;

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
    size_t x2 = 0, y2 = 0, eta = 0, table = 0, e2 = 0, g = 0;   // where the arrays begin in the upload, in doubles (PassPack)
};

// The argument checks of ml_fields_pupil_plan; B gets pupil_monomials of an accepted call.  -> 0, or -1 with `why` filled.
inline int pupil_check(int n_ranks, const double *x2, const double *xi, int nx, const double *y2, const double *eta, int ny, double r2,
                       int stop, int n_max, const double *c, const double *e2, int n_edges, const double *g, double *B, char *why,
                       size_t why_len) {
    const PassWhy w{"ml_fields_pupil_plan", why, why_len};
    if (int rc = pass_check_comm(w, n_ranks)) return rc;
    if (stop != 0 && stop != 1)
        return pass_refuse(w, -1, "stop = %d: 0 to leave the samples outside the pupil standing or 1 to clear them", stop);
    if (int rc = wf_check_order(w, n_max)) return rc;
    if (int rc = pass_check_edge_count(w, n_edges, 0, PUPIL_EDGES_MAX)) return rc;
    if (int rc = pass_check_axes(w, nx, ny)) return rc;
    if (!x2 || !xi || !y2 || !eta || (n_edges > 0 && (!e2 || !g))) return pass_refuse(w, -1, "NULL argument");
    if (int rc = pass_check_radius(w, r2)) return rc;
    if (int rc = pass_check_squared_axes(w, x2, nx, y2, ny)) return rc;
    if (int rc = pass_check_pupil_axes(w, xi, nx, eta, ny)) return rc;
    if (int rc = pass_check_vertex(w, y2, ny)) return rc;
    if (int rc = pass_check_edges(w, e2, n_edges)) return rc;
    for (int z = 0; z < n_edges; ++z)
        if (!std::isfinite(g[2 * z]) || !std::isfinite(g[2 * z + 1]))
            return pass_refuse(w, -1, "g[%d] = (%g, %g): a zone factor must be finite", z, g[2 * z], g[2 * z + 1]);
    if (c)
        if (int rc = pass_check_range(w, "c", c, wf_terms(n_max), false, "a phase coefficient must be finite")) return rc;
    pupil_monomials(n_max, c, B);
    const double psi = pupil_phase_bound(B);
    if (!(psi <= PASS_PHASE_LIMIT))
        return pass_refuse(w, -1, "the phase plate can reach %.6g rad on the unit disc: the phase arithmetic covers up to %g", psi,
                           PASS_PHASE_LIMIT);
    return 0;
}

// The checks of ml_fields_pupil_apply against the plan and the resident field sets.  -> 0; -1: an argument error, -2: the
// state does not allow the call; `why` is filled then.
inline int pupil_apply_check(const PassState &s, const PupilPlan &plan, int first_set, int n_sets, char *why, size_t why_len) {
    const PassWhy w{"ml_fields_pupil_apply", why, why_len};
    if (int rc = pass_check_comm(w, s.n_ranks)) return rc;
    if (int rc = pass_check_set_count(w, n_sets)) return rc;
    if (!plan.valid) return pass_refuse(w, -2, "no pupil has been planned on this context (ml_fields_pupil_plan)");
    if (int rc = pass_check_resident(w, s)) return rc;
    if (plan.nx != s.nx || plan.ny != s.ny)
        return pass_refuse(w, -2, "the pupil was planned for %d x %d samples, the resident field sets have %d x %d", plan.nx, plan.ny,
                           s.nx, s.ny);
    return pass_check_set_range(w, s, first_set, n_sets);
}

}  // namespace ml
