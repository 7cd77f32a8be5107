// The plan of the Zernike moments of the resident near field's wavefront (csrc/fields_wavefront.h) on the host:
//   fields_wavefront_plan sets nx n_max [sets nx n_max ...]
//        -> per shape a line  sets=... nx=... n_max=... terms=... record=... line_record=... scratch=...
//           (terms: J; record: doubles of a record; line_record: doubles a line leaves per set; scratch: bytes the call reserves)
//   fields_wavefront_plan layout
//        -> n=... s=... ix=... iy=... head=... order_max=... terms_max=... sets_max=... block=... line_threads=... sum_threads=... plane=... focus=...
//   fields_wavefront_plan table n_max
//        -> per term a line  j=... n=... m=... index=... nonzero=... sum=... abs=... norm=<N_j>  (the coefficient table's
//           checksums: the count of non-zero A_j,pq, their sum and the sum of their magnitudes), then  worst_abs=...
//   fields_wavefront_plan monomials n_max
//        -> per (p, q), p + q <= n_max, in the order of the moments a line  p=... q=... at=...
//   fields_wavefront_plan convert n_max v0,v1,...
//        -> the record wf_convert makes of 4 + 4 J monomial doubles, one value per line (%.17g)
//   fields_wavefront_plan check n_ranks res_nx res_ny res_sets first_set n_sets n_max ref_mode ref_c k r2 record_doubles x2 xi y2 eta ra rb
//        -> ok=1 phase=<the largest |phi|>, or refused=-1 (an argument) / refused=-2 (the state) followed by the message on a line
//           of its own; x2 ... rb: lists "a,b,c" (nx and ny are the lengths of x2 and y2), "null" for NULL
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fields_wavefront.h"

static bool parse_list(const char *arg, std::vector<double> &out) {
    out.clear();
    if (!strcmp(arg, "null")) return false;
    const char *p = arg;
    while (*p) {
        char *end = nullptr;
        out.push_back(strtod(p, &end));
        if (end == p) break;
        p = *end == ',' ? end + 1 : end;
    }
    return true;
}

static bool order_ok(int n_max) {
    if (n_max >= 0 && n_max <= ml::WF_ORDER_MAX) return true;
    fprintf(stderr, "0 <= n_max <= %d\n", ml::WF_ORDER_MAX);
    return false;
}

int main(int argc, char **argv) {
    using namespace ml;
    if (argc == 2 && !strcmp(argv[1], "layout")) {
        printf("n=%d s=%d ix=%d iy=%d head=%d order_max=%d terms_max=%d sets_max=%d block=%d line_threads=%d sum_threads=%d plane=%d focus=%d\n",
               WF_N, WF_S, WF_IX, WF_IY, WF_HEAD, WF_ORDER_MAX, WF_TERMS_MAX, PASS_SETS_MAX, PASS_BLOCK, PASS_LINE_THREADS, WF_SUM_THREADS,
               PASS_REF_PLANE, PASS_REF_FOCUS);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "table")) {
        const int n_max = atoi(argv[2]);
        if (!order_ok(n_max)) return 2;
        long long A[WF_ORDER_MAX + 1][WF_ORDER_MAX + 1], worst = 0;
        for (int j = 0; j < wf_terms(n_max); ++j) {
            int n, m, nonzero = 0;
            long long sum = 0, abs_sum = 0;
            wf_term(j, n, m);
            wf_coefficients(n, m, A);
            for (int p = 0; p <= WF_ORDER_MAX; ++p)
                for (int q = 0; q <= WF_ORDER_MAX; ++q) {
                    nonzero += A[p][q] != 0;
                    sum += A[p][q];
                    abs_sum += A[p][q] < 0 ? -A[p][q] : A[p][q];
                }
            worst = abs_sum > worst ? abs_sum : worst;
            printf("j=%d n=%d m=%d index=%d nonzero=%d sum=%lld abs=%lld norm=%.17g\n", j, n, m, wf_index(n, m), nonzero, sum, abs_sum,
                   wf_norm(n, m));
        }
        printf("worst_abs=%lld\n", worst);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "monomials")) {
        const int n_max = atoi(argv[2]);
        if (!order_ok(n_max)) return 2;
        for (int p = 0; p <= n_max; ++p)
            for (int q = 0; p + q <= n_max; ++q) printf("p=%d q=%d at=%d\n", p, q, wf_monomial(n_max, p, q));
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "convert")) {
        const int n_max = atoi(argv[2]);
        if (!order_ok(n_max)) return 2;
        std::vector<double> mono;
        if (!parse_list(argv[3], mono) || (int)mono.size() != wf_record(n_max)) {
            fprintf(stderr, "convert: %d monomial doubles for order %d\n", wf_record(n_max), n_max);
            return 2;
        }
        std::vector<double> rec(wf_record(n_max));
        wf_convert(mono.data(), n_max, rec.data());
        for (double v : rec) printf("%.17g\n", v);
        return 0;
    }
    if (argc == 20 && !strcmp(argv[1], "check")) {
        PassState s;
        s.n_ranks = atoi(argv[2]);
        s.nx = atoi(argv[3]);
        s.ny = atoi(argv[4]);
        s.n_sets = atoi(argv[5]);
        const int first = atoi(argv[6]), n_sets = atoi(argv[7]), n_max = atoi(argv[8]), mode = atoi(argv[9]);
        const double ref_c = atof(argv[10]), k = atof(argv[11]), r2 = atof(argv[12]);
        const int rd = atoi(argv[13]);
        std::vector<double> v[6];   // x2 xi y2 eta ra rb
        const double *ptr[6];
        for (int q = 0; q < 6; ++q) ptr[q] = parse_list(argv[14 + q], v[q]) ? v[q].data() : nullptr;
        const int nx = (int)v[0].size(), ny = (int)v[2].size();
        // the other arrays have the axes' lengths, as the entry takes them: another length is a usage error
        if ((ptr[1] && (int)v[1].size() != nx) || (ptr[4] && (int)v[4].size() != nx) || (ptr[3] && (int)v[3].size() != ny) ||
            (ptr[5] && (int)v[5].size() != ny)) {
            fprintf(stderr, "check: xi and ra have the length of x2, eta and rb that of y2\n");
            return 2;
        }
        char why[400];
        const int rc = wf_check(s, first, n_sets, ptr[0], ptr[1], nx, ptr[2], ptr[3], ny, r2, n_max, mode, ptr[4], ptr[5], ref_c, k, rd, why,
                                sizeof why);
        if (rc != 0)
            printf("refused=%d\n%s\n", rc, why);
        else
            printf("ok=1 phase=%.17g\n", pass_phase_max(mode, ptr[4], nx, ptr[5], ny, ref_c, k));
        return 0;
    }
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: fields_wavefront_plan sets nx n_max [...] | layout | table n_max | monomials n_max | convert n_max values | "
                        "check n_ranks res_nx res_ny res_sets first_set n_sets n_max ref_mode ref_c k r2 record_doubles x2 xi y2 eta ra rb\n");
        return 2;
    }
    for (int i = 1; i + 2 < argc; i += 3) {
        const int sets = atoi(argv[i]), nx = atoi(argv[i + 1]), n_max = atoi(argv[i + 2]);
        if (sets < 1 || sets > PASS_SETS_MAX || nx < 1 || !order_ok(n_max)) {
            fprintf(stderr, "1 <= sets <= %d, nx >= 1\n", PASS_SETS_MAX);
            return 2;
        }
        printf("sets=%d nx=%d n_max=%d terms=%d record=%d line_record=%d scratch=%lld\n", sets, nx, n_max, wf_terms(n_max), wf_record(n_max),
               wf_line_record(n_max), wf_scratch_bytes(sets, nx, n_max));
    }
    return 0;
}
