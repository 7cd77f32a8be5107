// The plan of the per-zone contributions to the field at points behind the aperture (csrc/fields_zone_fields.h) on the host:
//   fields_zone_fields_plan nx ny K want_h [nx ny K want_h ...]
//        -> per shape a line  nx=... ny=... k=... h=... blocks=... capacity=... run_doubles=... scratch=... bound=...
//           (capacity: runs a line can leave; run_doubles: doubles of a run; scratch: bytes the call reserves, whatever its
//           sets and targets are; bound: the bytes the interface promises not to exceed)
//   fields_zone_fields_plan layout
//        -> targets_max=... tg=... e_doubles=... eh_doubles=... edges_max=... sets_max=... block=...
//   fields_zone_fields_plan groups n_targets
//        -> groups=...
//   fields_zone_fields_plan check n_ranks res_nx res_ny res_sets first_set n_sets dxp dyp wavelength n_glass Z0 x2 y2 e2 tx ty tz
//        -> ok=1, or refused=-1 (an argument) / refused=-2 (the state) followed by the message on a line of its own;
//           x2 ... tz: lists "a,b,c" (nx, ny, n_edges and n_targets are the lengths of x2, y2, e2 and tx), "null" for NULL
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fields_zone_fields.h"

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
        printf("targets_max=%d tg=%d e_doubles=%d eh_doubles=%d edges_max=%d sets_max=%d block=%d\n", ZF_TARGETS_MAX, ZF_TG, ZF_E_DOUBLES,
               ZF_EH_DOUBLES, ZONES_EDGES_MAX, PASS_SETS_MAX, PASS_BLOCK);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "groups")) {
        printf("groups=%d\n", zf_groups(atoi(argv[2])));
        return 0;
    }
    if (argc == 19 && !strcmp(argv[1], "check")) {
        PassState s;
        s.n_ranks = atoi(argv[2]);
        s.nx = atoi(argv[3]);
        s.ny = atoi(argv[4]);
        s.n_sets = atoi(argv[5]);
        const int first = atoi(argv[6]), n_sets = atoi(argv[7]);
        const double dxp = atof(argv[8]), dyp = atof(argv[9]), wl = atof(argv[10]), ng = atof(argv[11]), Z0 = atof(argv[12]);
        std::vector<double> v[6];
        const double *ptr[6];
        for (int q = 0; q < 6; ++q) ptr[q] = parse_list(argv[13 + q], v[q]) ? v[q].data() : nullptr;
        const int nx = (int)v[0].size(), ny = (int)v[1].size(), K = (int)v[2].size(), T = (int)v[3].size();
        // ty and tz have the length of tx, as the entry takes them: a shorter list is a usage error
        if ((ptr[4] && (int)v[4].size() != T) || (ptr[5] && (int)v[5].size() != T)) {
            fprintf(stderr, "check: ty and tz have the length of tx\n");
            return 2;
        }
        char why[400];
        const int rc = zf_check(s, first, n_sets, dxp, dyp, wl, ng, Z0, ptr[0], nx, ptr[1], ny, ptr[2], K, ptr[3], ptr[4], ptr[5], T, why,
                                sizeof why);
        if (rc != 0)
            printf("refused=%d\n%s\n", rc, why);
        else
            printf("ok=1\n");
        return 0;
    }
    if (argc < 5 || (argc - 1) % 4 != 0) {
        fprintf(stderr, "usage: fields_zone_fields_plan nx ny K want_h [...] | layout | groups n_targets | check n_ranks res_nx res_ny "
                        "res_sets first_set n_sets dxp dyp wavelength n_glass Z0 x2 y2 e2 tx ty tz\n");
        return 2;
    }
    for (int i = 1; i + 3 < argc; i += 4) {
        const int nx = atoi(argv[i]), ny = atoi(argv[i + 1]), K = atoi(argv[i + 2]), h = atoi(argv[i + 3]);
        if (nx < 1 || ny < 1 || K < 1 || K > ZONES_EDGES_MAX) {
            fprintf(stderr, "nx, ny >= 1, 1 <= K <= %d\n", ZONES_EDGES_MAX);
            return 2;
        }
        printf("nx=%d ny=%d k=%d h=%d blocks=%d capacity=%lld run_doubles=%d scratch=%lld bound=%lld\n", nx, ny, K, h != 0, pass_blocks(ny),
               zf_run_capacity(ny, K), zf_run_doubles(h != 0), zf_scratch_bytes(nx, ny, K, h != 0), zf_scratch_bound(nx, ny, K, h != 0));
    }
    return 0;
}
