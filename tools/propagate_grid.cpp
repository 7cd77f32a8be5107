// The plan of the FFT form of the finite-distance propagator (csrc/propagate_grid.h) for given sizes, on the host:
//   propagate_grid nx ny mx my want_h   ->  Lx=... Ly=... outputs=... plane_bytes=... workspace_bytes=...
//                                           or  refused=1 followed by the message on a line of its own
//   propagate_grid nx ny mx my want_h cap   the same with `cap` as the longest padded axis (16384: the long plan),
//                                           followed by the route of each axis (grid_axis_route), a line per axis:
//                                           route axis=rows L=... top_stages=... lds_len=... forward=top,lds back=lds,top
//   propagate_grid lag L m              ->  the lag held by every index of a padded axis, and back
//   propagate_grid twiddles L           ->  max |table - cosl / sinl| over the table, in units of 2^-53
#include <cstdlib>
#include <cstring>

#include "propagate_grid.h"

int main(int argc, char **argv) {
    using namespace ml;
    if (argc == 4 && !strcmp(argv[1], "lag")) {
        const int L = atoi(argv[2]), m = atoi(argv[3]);
        for (int p = 0; p < L; ++p) {
            const int lag = grid_index_lag(p, m, L);
            if (grid_lag_index(lag, L) != p) return 1;
            printf("%d%c", lag, p + 1 < L ? ' ' : '\n');
        }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "twiddles")) {
        const int L = atoi(argv[2]);
        const std::vector<double> t = grid_twiddles(L);
        long double worst = 0;
        for (int j = 0; j < L / 2; ++j) {
            const long double phi = 8.0L * atanl(1.0L) * j / L;
            worst = fmaxl(worst, fmaxl(fabsl(t[2 * j] - cosl(phi)), fabsl(t[2 * j + 1] - sinl(phi))));
        }
        printf("entries=%d worst_ulp53=%.3Lf\n", L / 2, worst * 9007199254740992.0L);
        return 0;
    }
    if (argc != 6 && argc != 7) {
        fprintf(stderr, "usage: propagate_grid nx ny mx my want_h [cap] | lag L m | twiddles L\n");
        return 2;
    }
    GridPlanFacts f;
    char why[320];
    const int cap = argc == 7 ? atoi(argv[6]) : GRID_L_MAX;
    if (cap < GRID_L_MIN || cap > GRID_L_LONG_MAX) {
        fprintf(stderr, "cap must lie in [%d, %d]\n", GRID_L_MIN, GRID_L_LONG_MAX);
        return 2;
    }
    if (grid_plan_facts(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), &f, why, sizeof why, cap) != 0) {
        printf("refused=1\n%s\n", why);
        return 0;
    }
    printf("Lx=%d Ly=%d outputs=%d plane_bytes=%lld workspace_bytes=%lld\n", f.Lx, f.Ly, f.outputs, (long long)f.plane_bytes,
           (long long)f.workspace_bytes);
    if (argc == 7)
        for (int columns = 0; columns < 2; ++columns) {
            const int L = columns ? f.Lx : f.Ly;
            const GridAxisRoute r = grid_axis_route(L, columns != 0);
            printf("route axis=%s L=%d top_stages=%d lds_len=%d forward=%s back=%s\n", columns ? "columns" : "rows", L,
                   r.top_stages, r.lds_len, grid_route_order(r, false), grid_route_order(r, true));
        }
    return 0;
}
