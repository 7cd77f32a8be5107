// The host side of the transfer function of a propagated image (csrc/propagate_otf.h), without a GPU:
//   propagate_otf_plan fraction u i [u i ...]
//        -> per pair a line  fraction=<hex double> naive=<hex double> quarters=<q> rest=<hex double>: otf_phase_fraction(u, i),
//           what a plain product gives, and otf_phase_quarters of the fraction
//           (u: any spelling strtod reads, hexadecimal included; 0 <= i < 2^53)
//   propagate_otf_plan plan mx my planes nu nv
//        -> table=... rows=... segments_x=... segments_y=... segment=... freq_max=...  (phasors tabulated, row sums per
//           weight, segments of 32 indices along either axis)
//   propagate_otf_plan shape mx my nv
//        -> rows=... tile=... tiles=... batch=... last_segments=... last_segment=... groups=... last_rows=... col_tile=...
//           col_tiles=... col_last_segments=... col_last_segment=...  (the row pass: rows of a plane per workgroup, targets
//           of each per tile, tiles per row, frequencies per batch, segments of the last tile and indices of its last
//           segment, workgroups along x and live rows of the last; the column pass: rows per tile, tiles, the last tile's
//           segments and the indices of its last segment)
//   propagate_otf_plan check have_result have_sums T sets source mx my planes null nu nv ku kv [u ... v ...]
//        -> ok=1, or refused=-1 (an argument) / refused=-2 (the state) followed by the message on a line of its own;
//           null: 1 = u is NULL, 2 = v, 4 = otf (added up); ku and kv values follow, nu and nv are what the call claims
#include <cstdlib>
#include <cstring>
#include <vector>

#include "propagate_otf.h"

int main(int argc, char **argv) {
    using namespace ml;
    if (argc >= 4 && argc % 2 == 0 && !strcmp(argv[1], "fraction")) {
        for (int a = 2; a + 1 < argc; a += 2) {
            const double u = strtod(argv[a], nullptr), i = (double)atoll(argv[a + 1]);
            double rest;
            const int q = otf_phase_quarters(otf_phase_fraction(u, i), rest);
            printf("fraction=%a naive=%a quarters=%d rest=%a\n", otf_phase_fraction(u, i), otf_phase_fraction_naive(u, i), q, rest);
        }
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "plan")) {
        const int mx = atoi(argv[2]), my = atoi(argv[3]), planes = atoi(argv[4]), nu = atoi(argv[5]), nv = atoi(argv[6]);
        if (mx < 1 || my < 1 || planes < 1 || nu < 1 || nv < 1) {
            fprintf(stderr, "plan: mx, my, planes, nu, nv >= 1\n");
            return 2;
        }
        printf("table=%lld rows=%lld segments_x=%d segments_y=%d segment=%d freq_max=%d\n", (long long)mx * nu + (long long)my * nv,
               (long long)planes * mx * nv, otf_segments(mx), otf_segments(my), OTF_SEGMENT, OTF_FREQ_MAX);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "shape")) {
        const int mx = atoi(argv[2]), my = atoi(argv[3]), nv = atoi(argv[4]);
        if (mx < 1 || my < 1 || nv < 1 || nv > OTF_FREQ_MAX) {
            fprintf(stderr, "shape: mx, my >= 1, 1 <= nv <= %d\n", OTF_FREQ_MAX);
            return 2;
        }
        const OtfRowsShape r = otf_rows_shape(mx, my, nv);
        const OtfColumnsShape c = otf_columns_shape(mx);
        printf("rows=%d tile=%d tiles=%d batch=%d last_segments=%d last_segment=%d groups=%d last_rows=%d col_tile=%d col_tiles=%d "
               "col_last_segments=%d col_last_segment=%d\n", r.rows, r.tile, r.tiles, r.batch, r.last_segments, r.last_segment,
               r.groups, r.last_rows, OTF_TILE, c.tiles, c.last_segments, c.last_segment);
        return 0;
    }
    if (argc >= 15 && !strcmp(argv[1], "check")) {
        FocusState s;
        s.have_result = atoi(argv[2]) != 0;
        s.have_sums = atoi(argv[3]) != 0;
        s.T = atoi(argv[4]);
        s.result_sets = atoi(argv[5]);
        const int source = atoi(argv[6]), mx = atoi(argv[7]), my = atoi(argv[8]), planes = atoi(argv[9]), null = atoi(argv[10]);
        const int nu = atoi(argv[11]), nv = atoi(argv[12]), ku = atoi(argv[13]), kv = atoi(argv[14]);
        if (ku < 0 || kv < 0 || argc != 15 + ku + kv || (nu > ku && !(null & 1)) || (nv > kv && !(null & 2))) {
            fprintf(stderr, "check: ku + kv values follow, and an axis that is not NULL holds the frequencies the call claims\n");
            return 2;
        }
        std::vector<double> u, v;
        for (int a = 0; a < ku; ++a) u.push_back(strtod(argv[15 + a], nullptr));
        for (int a = 0; a < kv; ++a) v.push_back(strtod(argv[15 + ku + a], nullptr));
        u.push_back(0.0);   // (data() of an empty vector may be NULL)
        v.push_back(0.0);
        double out = 0.0;
        char why[320];
        const int rc = otf_check(s, source, mx, my, planes, (null & 1) ? nullptr : u.data(), nu, (null & 2) ? nullptr : v.data(), nv,
                                 (null & 4) ? nullptr : &out, why, sizeof why);
        if (rc != 0)
            printf("refused=%d\n%s\n", rc, why);
        else
            printf("ok=1\n");
        return 0;
    }
    fprintf(stderr, "usage: propagate_otf_plan fraction u i [...] | plan mx my planes nu nv | shape mx my nv | check have_result have_sums T sets source "
                    "mx my planes null nu nv ku kv [u ... v ...]\n");
    return 2;
}
