// The tiled plan of the FFT form of the finite-distance propagator (csrc/propagate_grid.h GridTilePlan) for given sizes,
// on the host:
//   propagate_grid_tiled nx ny mx my want_h [tile_lx tile_ly [batch_mib]]
//                                        ->  Lx=... Ly=... cx=... cy=... bx=... by=... tiles=... batch=... outputs=...
//                                            plane_bytes=... workspace_bytes=...   (tile lengths of 0: the default)
//                                            or  refused=1 followed by the message on a line of its own
//   propagate_grid_tiled default n m     ->  L=... B=... c=...: the default tile length of one axis
//   propagate_grid_tiled lag L m a B     ->  the true lag held by every index of the kernel plane of tile a
#include <cstdlib>
#include <cstring>

#include "propagate_grid.h"

int main(int argc, char **argv) {
    using namespace ml;
    if (argc == 4 && !strcmp(argv[1], "default")) {
        const int n = atoi(argv[2]), m = atoi(argv[3]);
        if (n < 1 || m < 1 || m > GRID_L_MAX) {
            fprintf(stderr, "default: n >= 1 and 1 <= m <= %d\n", GRID_L_MAX);
            return 2;
        }
        const GridTileAxis t = grid_tile_axis(n, m, grid_tile_default(n, m));
        printf("L=%d B=%d c=%d\n", t.L, t.B, t.c);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "lag")) {
        const int L = atoi(argv[2]), m = atoi(argv[3]), a = atoi(argv[4]), B = atoi(argv[5]);
        for (int p = 0; p < L; ++p) printf("%d%c", grid_index_lag(p, m, L) - a * B, p + 1 < L ? ' ' : '\n');
        return 0;
    }
    if (argc != 6 && argc != 8 && argc != 9) {
        fprintf(stderr, "usage: propagate_grid_tiled nx ny mx my want_h [tile_lx tile_ly [batch_mib]] | default n m | lag L m a B\n");
        return 2;
    }
    const int tile_lx = argc >= 8 ? atoi(argv[6]) : 0, tile_ly = argc >= 8 ? atoi(argv[7]) : 0;
    const int64_t batch_bytes = argc == 9 ? (int64_t)atoi(argv[8]) << 20 : GRID_TILE_BATCH_BYTES;
    GridTilePlan t;
    char why[400];
    if (grid_tile_plan(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), tile_lx, tile_ly, batch_bytes, &t,
                       why, sizeof why) != 0) {
        printf("refused=1\n%s\n", why);
        return 0;
    }
    printf("Lx=%d Ly=%d cx=%d cy=%d bx=%d by=%d tiles=%d batch=%d outputs=%d plane_bytes=%lld workspace_bytes=%lld\n", t.x.L, t.y.L,
           t.x.c, t.y.c, t.x.B, t.y.B, t.tiles, t.batch, t.outputs, (long long)t.plane_bytes, (long long)t.workspace_bytes);
    return 0;
}
