// The launch of the direct pair sum of the finite-distance propagator (csrc/propagate_direct.h) for given shapes, on the
// host:
//   propagate_direct_plan T nx sets want_h [T nx sets want_h ...]
//        -> per shape a line  T=... tiles=... splits=... rows_min=... rows_max=... partial_bytes=... result_bytes=...
//           (tiles: workgroups along the targets; splits: workgroups per target tile, each of which sums the aperture rows
//           s, s + splits, ...; rows_min, rows_max: rows of the least and the most loaded of them, counted row by row)
//   propagate_direct_plan constants
//        -> threads=... tile=... max_sets=... blocks=... target_rows=...
//   propagate_direct_plan diff x x0 [x x0 ...]          (hexadecimal floats, as Python's float.hex() writes them)
//        -> per pair a line  hi lo  in hexadecimal floats: x - x0 as the plan stores a target's coordinate (prop_two_diff)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "propagate_direct.h"

int main(int argc, char **argv) {
    using namespace ml;
    if (argc == 2 && !strcmp(argv[1], "constants")) {
        printf("threads=%d tile=%d max_sets=%d blocks=%d target_rows=%d\n", PROP_THREADS, PROP_TILE, PROP_MAX_SETS, PROP_BLOCKS,
               PROP_TARGET_ROWS);
        return 0;
    }
    if (argc >= 4 && argc % 2 == 0 && !strcmp(argv[1], "diff")) {
        for (int i = 2; i + 1 < argc; i += 2) {
            double lo = 0.0;
            const double hi = prop_two_diff(strtod(argv[i], nullptr), strtod(argv[i + 1], nullptr), &lo);
            printf("%a %a\n", hi, lo);
        }
        return 0;
    }
    if (argc < 5 || (argc - 1) % 4 != 0) {
        fprintf(stderr, "usage: propagate_direct_plan T nx sets want_h [...] | constants | diff x x0 [...]\n");
        return 2;
    }
    for (int i = 1; i + 3 < argc; i += 4) {
        const int T = atoi(argv[i]), nx = atoi(argv[i + 1]), sets = atoi(argv[i + 2]), want_h = atoi(argv[i + 3]);
        if (T < 1 || T > (1 << 26) || nx < 1 || nx > (1 << 20) || sets < 1 || sets > PROP_MAX_SETS || (want_h != 0 && want_h != 1)) {
            fprintf(stderr, "1 <= T <= 2^26, 1 <= nx <= 2^20, 1 <= sets <= %d, want_h 0 or 1\n", PROP_MAX_SETS);
            return 2;
        }
        const int splits = prop_splits(T, nx);
        // the kernel's own loop, row by row: for (i = blockIdx.y; i < nx; i += splits)
        std::vector<int> rows(splits, 0);
        for (int s = 0; s < splits; ++s)
            for (int r = s; r < nx; r += splits) ++rows[s];
        int rows_min = rows[0], rows_max = rows[0], total = 0;
        for (int s = 0; s < splits; ++s) {
            if (rows[s] != prop_rows_of(nx, splits, s)) {
                fprintf(stderr, "prop_rows_of(%d, %d, %d) = %d, counted %d\n", nx, splits, s, prop_rows_of(nx, splits, s), rows[s]);
                return 1;
            }
            rows_min = rows[s] < rows_min ? rows[s] : rows_min;
            rows_max = rows[s] > rows_max ? rows[s] : rows_max;
            total += rows[s];
        }
        if (total != nx) {
            fprintf(stderr, "the workgroups sum %d rows of %d\n", total, nx);
            return 1;
        }
        printf("T=%d tiles=%d splits=%d rows_min=%d rows_max=%d partial_bytes=%zu result_bytes=%zu\n", T, prop_tiles(T), splits,
               rows_min, rows_max, prop_partial_bytes(T, nx, sets, want_h != 0), prop_result_bytes(T, sets, want_h != 0));
    }
    return 0;
}
