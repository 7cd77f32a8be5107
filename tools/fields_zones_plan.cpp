// The plan of the per-zone sums of the resident near field (csrc/fields_zones.h) on the host:
//   fields_zones_plan sets nx ny K [sets nx ny K ...]
//        -> per shape a line  sets=... nx=... ny=... k=... blocks=... capacity=... scratch=... bound=...
//           (blocks: blocks of 64 samples of a line; capacity: runs a line can leave; scratch: bytes the call reserves;
//           bound: the bytes the interface promises not to exceed, sets nx min(ny + 2, 2 K + 2) 64)
//   fields_zones_plan layout
//        -> n=... s=... ix=... iy=... cx=... cy=... record=... terms=... run_bytes=... edges_max=... sets_max=... block=... plane=... focus=...
//   fields_zones_plan vertex y2
//        -> jv=... (the first minimum of the list)
//   fields_zones_plan check n_ranks res_nx res_ny res_sets first_set n_sets ref_mode ref_c k record_doubles x2 y2 e2 ra rb
//        -> ok=1 phase=<the largest |phi|>, or refused=-1 (an argument) / refused=-2 (the state) followed by the message on a line
//           of its own; x2 ... rb: lists "a,b,c" (nx and ny are the lengths of x2 and y2, n_edges that of e2), "null" for NULL
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fields_zones.h"

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

int main(int argc, char **argv) {
    using namespace ml;
    if (argc == 2 && !strcmp(argv[1], "layout")) {
        printf("n=%d s=%d ix=%d iy=%d cx=%d cy=%d record=%d terms=%d run_bytes=%d edges_max=%d sets_max=%d block=%d plane=%d focus=%d\n",
               ZONES_N, ZONES_S, ZONES_IX, ZONES_IY, ZONES_CX, ZONES_CY, ZONES_RECORD, ZONES_TERMS, ZONES_RUN_BYTES, ZONES_EDGES_MAX,
               PASS_SETS_MAX, PASS_BLOCK, PASS_REF_PLANE, PASS_REF_FOCUS);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "vertex")) {
        std::vector<double> y2;
        if (!parse_list(argv[2], y2) || y2.empty()) {
            fprintf(stderr, "vertex: a list of numbers\n");
            return 2;
        }
        printf("jv=%d\n", pass_vertex(y2.data(), (int)y2.size()));
        return 0;
    }
    if (argc == 17 && !strcmp(argv[1], "check")) {
        PassState s;
        s.n_ranks = atoi(argv[2]);
        s.nx = atoi(argv[3]);
        s.ny = atoi(argv[4]);
        s.n_sets = atoi(argv[5]);
        const int first = atoi(argv[6]), n_sets = atoi(argv[7]), mode = atoi(argv[8]);
        const double ref_c = atof(argv[9]), k = atof(argv[10]);
        const int rd = atoi(argv[11]);
        std::vector<double> v[5];
        const double *ptr[5];
        for (int q = 0; q < 5; ++q) ptr[q] = parse_list(argv[12 + q], v[q]) ? v[q].data() : nullptr;
        const int nx = (int)v[0].size(), ny = (int)v[1].size(), K = (int)v[2].size();
        // the reference's arrays have the axes' lengths, as the entry takes them: a shorter list is a usage error
        if ((ptr[3] && (int)v[3].size() != nx) || (ptr[4] && (int)v[4].size() != ny)) {
            fprintf(stderr, "check: ra and rb have the lengths of x2 and y2\n");
            return 2;
        }
        char why[400];
        const int rc = zones_check(s, first, n_sets, ptr[0], nx, ptr[1], ny, ptr[2], K, mode, ptr[3], ptr[4], ref_c, k, rd, why, sizeof why);
        if (rc != 0)
            printf("refused=%d\n%s\n", rc, why);
        else
            printf("ok=1 phase=%.17g\n", pass_phase_max(mode, ptr[3], nx, ptr[4], ny, ref_c, k));
        return 0;
    }
    if (argc < 5 || (argc - 1) % 4 != 0) {
        fprintf(stderr, "usage: fields_zones_plan sets nx ny K [...] | layout | vertex y2 | check n_ranks res_nx res_ny res_sets first_set "
                        "n_sets ref_mode ref_c k record_doubles x2 y2 e2 ra rb\n");
        return 2;
    }
    for (int i = 1; i + 3 < argc; i += 4) {
        const int sets = atoi(argv[i]), nx = atoi(argv[i + 1]), ny = atoi(argv[i + 2]), K = atoi(argv[i + 3]);
        if (sets < 1 || sets > PASS_SETS_MAX || nx < 1 || ny < 1 || K < 1 || K > ZONES_EDGES_MAX) {
            fprintf(stderr, "1 <= sets <= %d, nx, ny >= 1, 1 <= K <= %d\n", PASS_SETS_MAX, ZONES_EDGES_MAX);
            return 2;
        }
        printf("sets=%d nx=%d ny=%d k=%d blocks=%d capacity=%lld scratch=%lld bound=%lld\n", sets, nx, ny, K, pass_blocks(ny),
               zones_run_capacity(ny, K), zones_scratch_bytes(sets, nx, ny, K), zones_scratch_bound(sets, nx, ny, K));
    }
    return 0;
}
