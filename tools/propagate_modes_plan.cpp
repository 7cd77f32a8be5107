// The host side of the mode overlaps of a propagated image (csrc/propagate_modes.h), without a GPU:
//   propagate_modes_plan plan mx my planes nu nv n_slots
//        -> table=... rows=... out=... segments_x=... segments_y=... segment=... modes_max=...  (table entries, row sums per
//           component, output entries of all slots, segments of 32 indices along either axis)
//   propagate_modes_plan shape mx my nv
//        -> rows=... tile=... tiles=... last_segments=... last_segment=... groups=... last_rows=... col_tile=... col_tiles=...
//           col_last_segments=... col_last_segment=...  (the row pass: rows of a plane per workgroup, targets of each per
//           tile, tiles per row, segments of the last tile and indices of its last segment, workgroups along x and live rows
//           of the last; the column pass: rows per tile, tiles, the last tile's segments and the indices of its last segment)
//   propagate_modes_plan check_plan T mx my planes null nu nv n_slots [axis mode index part value]
//        -> ok=1, or refused=-1 followed by the message on a line of its own.  The tables are filled here with (1, -0.5);
//           null: 1 = mode_x is NULL, 2 = mode_y (added up); the optional five put `value` (any spelling strtod reads) into
//           the real (part 0) or imaginary (part 1) part of entry [mode][index] of axis 0 (x) or 1 (y)
//   propagate_modes_plan check_queue have_result planned sets n_slots source slot
//   propagate_modes_plan check_fetch planned n_slots first_slot n null
//        -> ok=1, or refused=-1 (an argument) / refused=-2 (the state) and the message
#include <cstdlib>
#include <cstring>
#include <vector>

#include "propagate_modes.h"

static void report(int rc, const char *why) {
    if (rc != 0)
        printf("refused=%d\n%s\n", rc, why);
    else
        printf("ok=1\n");
}

int main(int argc, char **argv) {
    using namespace ml;
    char why[320];
    if (argc == 8 && !strcmp(argv[1], "plan")) {
        const int mx = atoi(argv[2]), my = atoi(argv[3]), planes = atoi(argv[4]), nu = atoi(argv[5]), nv = atoi(argv[6]), n_slots = atoi(argv[7]);
        if (mx < 1 || my < 1 || planes < 1 || nu < 1 || nv < 1 || n_slots < 1) {
            fprintf(stderr, "plan: mx, my, planes, nu, nv, n_slots >= 1\n");
            return 2;
        }
        printf("table=%lld rows=%lld out=%lld segments_x=%d segments_y=%d segment=%d modes_max=%d\n", (long long)mx * nu + (long long)my * nv,
               (long long)planes * mx * nv, (long long)n_slots * planes * MODES_COMPONENTS * nu * nv, modes_segments(mx), modes_segments(my),
               MODES_SEGMENT, MODES_MAX);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "shape")) {
        const int mx = atoi(argv[2]), my = atoi(argv[3]), nv = atoi(argv[4]);
        if (mx < 1 || my < 1 || nv < 1 || nv > MODES_MAX) {
            fprintf(stderr, "shape: mx, my >= 1, 1 <= nv <= %d\n", MODES_MAX);
            return 2;
        }
        const ModesRowsShape r = modes_rows_shape(mx, my, nv);
        const ModesColumnsShape c = modes_columns_shape(mx);
        printf("rows=%d tile=%d tiles=%d last_segments=%d last_segment=%d groups=%d last_rows=%d col_tile=%d col_tiles=%d "
               "col_last_segments=%d col_last_segment=%d\n", r.rows, r.tile, r.tiles, r.last_segments, r.last_segment, r.groups,
               r.last_rows, MODES_COLUMN_TILE, c.tiles, c.last_segments, c.last_segment);
        return 0;
    }
    if ((argc == 10 || argc == 15) && !strcmp(argv[1], "check_plan")) {
        const long long T = atoll(argv[2]);
        const int mx = atoi(argv[3]), my = atoi(argv[4]), planes = atoi(argv[5]), null = atoi(argv[6]), nu = atoi(argv[7]), nv = atoi(argv[8]);
        const int n_slots = atoi(argv[9]);
        // the tables are read only where the counts are in range: hold what such a call can read, never less than one entry
        const bool sane = mx >= 1 && my >= 1 && nu >= 1 && nu <= MODES_MAX && nv >= 1 && nv <= MODES_MAX;
        std::vector<double> x(sane ? 2 * (size_t)nu * mx : 2), y(sane ? 2 * (size_t)nv * my : 2);
        for (size_t e = 0; e < x.size(); ++e) x[e] = e % 2 ? -0.5 : 1.0;
        for (size_t e = 0; e < y.size(); ++e) y[e] = e % 2 ? -0.5 : 1.0;
        if (argc == 15) {
            const int axis = atoi(argv[10]), mode = atoi(argv[11]), index = atoi(argv[12]), part = atoi(argv[13]);
            std::vector<double> &t = axis ? y : x;
            const size_t at = 2 * ((size_t)mode * (axis ? my : mx) + index) + (part ? 1 : 0);
            if (!sane || mode < 0 || index < 0 || mode >= (axis ? nv : nu) || index >= (axis ? my : mx)) {
                fprintf(stderr, "check_plan: the entry to overwrite lies outside the tables\n");
                return 2;
            }
            t[at] = strtod(argv[14], nullptr);
        }
        const int rc = modes_plan_check(T, mx, my, planes, (null & 1) ? nullptr : x.data(), nu, (null & 2) ? nullptr : y.data(), nv, n_slots,
                                        why, sizeof why);
        report(rc, why);
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "check_queue")) {
        FocusState s;
        s.have_result = atoi(argv[2]) != 0;
        ModesState m;
        m.planned = atoi(argv[3]) != 0;
        s.result_sets = atoi(argv[4]);
        m.n_slots = atoi(argv[5]);
        report(modes_queue_check(s, m, atoi(argv[6]), atoi(argv[7]), why, sizeof why), why);
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "check_fetch")) {
        ModesState m;
        m.planned = atoi(argv[2]) != 0;
        m.n_slots = atoi(argv[3]);
        double out = 0.0;
        report(modes_fetch_check(m, atoi(argv[4]), atoi(argv[5]), atoi(argv[6]) ? nullptr : &out, why, sizeof why), why);
        return 0;
    }
    fprintf(stderr, "usage: propagate_modes_plan plan mx my planes nu nv n_slots | shape mx my nv | check_plan T mx my planes null nu nv "
                    "n_slots [axis mode index part value] | check_queue have_result planned sets n_slots source slot | check_fetch planned "
                    "n_slots first_slot n null\n");
    return 2;
}
