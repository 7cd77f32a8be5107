// The plan of the pupil function applied to the resident near field (csrc/fields_pupil.h) on the host:
//   fields_pupil_plan nx ny K [nx ny K ...]
//        -> per shape a line  nx=... ny=... edges=... doubles=...   (doubles: what the plan uploads)
//   fields_pupil_plan layout
//        -> order_max=... nq=... edges_max=... sets_max=... block=... line_threads=... phase_limit=...
//   fields_pupil_plan monomials n_max c0,c1,...
//        -> per (p, q), p + q <= n_max, a line  p=... q=... B=<B_pq, %.17g>, then  reach=<sum |B_pq|>
//   fields_pupil_plan table n_max c0,c1,... xi0,xi1,...
//        -> per line i the PUPIL_NQ entries b_q(i) of the line table, %.17g, separated by blanks
//   fields_pupil_plan check n_ranks stop n_max r2 x2 xi y2 eta c e2 g
//        -> ok=1 reach=<sum |B_pq|>, or refused=-1 followed by the message on a line of its own; x2 ... g: lists "a,b,c"
//           (nx, ny and the edges are the lengths of x2, y2 and e2; g: re,im per edge), "null" for NULL
//   fields_pupil_plan apply n_ranks res_nx res_ny res_sets plan_valid plan_nx plan_ny first_set n_sets
//        -> ok=1, or refused=-1 (an argument) / refused=-2 (the state) followed by the message
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fields_pupil.h"

static bool parse_list(const char *arg, std::vector<double> &out) {
    out.clear();
    if (!strcmp(arg, "null")) return false;
    const char *p = arg;
    while (*p) {
        char *end = nullptr;
        const double v = strtod(p, &end);
        if (end == p) break;
        out.push_back(v);
        p = *end == ',' ? end + 1 : end;
    }
    return true;
}

static bool order_ok(int n_max) {
    if (n_max >= 0 && n_max <= ml::PUPIL_ORDER_MAX) return true;
    fprintf(stderr, "0 <= n_max <= %d\n", ml::PUPIL_ORDER_MAX);
    return false;
}

int main(int argc, char **argv) {
    using namespace ml;
    if (argc == 2 && !strcmp(argv[1], "layout")) {
        printf("order_max=%d nq=%d edges_max=%d sets_max=%d block=%d line_threads=%d phase_limit=%g\n", PUPIL_ORDER_MAX, PUPIL_NQ,
               PUPIL_EDGES_MAX, PASS_SETS_MAX, PASS_BLOCK, PASS_LINE_THREADS, PASS_PHASE_LIMIT);
        return 0;
    }
    if ((argc == 4 && !strcmp(argv[1], "monomials")) || (argc == 5 && !strcmp(argv[1], "table"))) {
        const int n_max = atoi(argv[2]);
        if (!order_ok(n_max)) return 2;
        std::vector<double> c, xi;
        if (!parse_list(argv[3], c) || (int)c.size() != wf_terms(n_max)) {
            fprintf(stderr, "%d coefficients for order %d\n", wf_terms(n_max), n_max);
            return 2;
        }
        double B[PUPIL_NQ * PUPIL_NQ];
        pupil_monomials(n_max, c.data(), B);
        if (argc == 4) {
            for (int p = 0; p <= n_max; ++p)
                for (int q = 0; p + q <= n_max; ++q) printf("p=%d q=%d B=%.17g\n", p, q, B[p * PUPIL_NQ + q]);
            printf("reach=%.17g\n", pupil_phase_bound(B));
            return 0;
        }
        if (!parse_list(argv[4], xi) || xi.empty()) {
            fprintf(stderr, "table: at least one xi\n");
            return 2;
        }
        std::vector<double> table(xi.size() * PUPIL_NQ);
        pupil_line_table(n_max, B, xi.data(), (int)xi.size(), table.data());
        for (size_t i = 0; i < xi.size(); ++i)
            for (int q = 0; q < PUPIL_NQ; ++q) printf("%.17g%c", table[i * PUPIL_NQ + q], q + 1 < PUPIL_NQ ? ' ' : '\n');
        return 0;
    }
    if (argc == 13 && !strcmp(argv[1], "check")) {
        const int n_ranks = atoi(argv[2]), stop = atoi(argv[3]), n_max = atoi(argv[4]);
        const double r2 = atof(argv[5]);
        std::vector<double> v[7];   // x2 xi y2 eta c e2 g
        const double *ptr[7];
        for (int q = 0; q < 7; ++q) ptr[q] = parse_list(argv[6 + q], v[q]) ? v[q].data() : nullptr;
        const int nx = (int)v[0].size(), ny = (int)v[2].size(), K = (int)v[5].size();
        // the other arrays have the lengths the entry takes them with: another length is a usage error
        if ((ptr[1] && (int)v[1].size() != nx) || (ptr[3] && (int)v[3].size() != ny) || (ptr[6] && (int)v[6].size() != 2 * K) ||
            (ptr[4] && n_max >= 0 && n_max <= PUPIL_ORDER_MAX && (int)v[4].size() != wf_terms(n_max))) {
            fprintf(stderr, "check: xi has the length of x2, eta that of y2, g two numbers per edge, c the terms of n_max\n");
            return 2;
        }
        char why[400];
        double B[PUPIL_NQ * PUPIL_NQ];
        const int rc = pupil_check(n_ranks, ptr[0], ptr[1], nx, ptr[2], ptr[3], ny, r2, stop, n_max, ptr[4], ptr[5], K, ptr[6], B, why, sizeof why);
        if (rc != 0)
            printf("refused=%d\n%s\n", rc, why);
        else
            printf("ok=1 reach=%.17g\n", pupil_phase_bound(B));
        return 0;
    }
    if (argc == 11 && !strcmp(argv[1], "apply")) {
        PassState s;
        s.n_ranks = atoi(argv[2]);
        s.nx = atoi(argv[3]);
        s.ny = atoi(argv[4]);
        s.n_sets = atoi(argv[5]);
        PupilPlan plan;
        plan.valid = atoi(argv[6]) != 0;
        plan.nx = atoi(argv[7]);
        plan.ny = atoi(argv[8]);
        char why[400];
        const int rc = pupil_apply_check(s, plan, atoi(argv[9]), atoi(argv[10]), why, sizeof why);
        if (rc != 0)
            printf("refused=%d\n%s\n", rc, why);
        else
            printf("ok=1\n");
        return 0;
    }
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: fields_pupil_plan nx ny K [...] | layout | monomials n_max c | table n_max c xi | "
                        "check n_ranks stop n_max r2 x2 xi y2 eta c e2 g | apply n_ranks res_nx res_ny res_sets plan_valid plan_nx plan_ny "
                        "first_set n_sets\n");
        return 2;
    }
    for (int i = 1; i + 2 < argc; i += 3) {
        const int nx = atoi(argv[i]), ny = atoi(argv[i + 1]), K = atoi(argv[i + 2]);
        if (nx < 1 || ny < 1 || K < 0 || K > PUPIL_EDGES_MAX) {
            fprintf(stderr, "nx, ny >= 1, 0 <= K <= %d\n", PUPIL_EDGES_MAX);
            return 2;
        }
        printf("nx=%d ny=%d edges=%d doubles=%lld\n", nx, ny, K, pupil_plan_doubles(nx, ny, K));
    }
    return 0;
}
