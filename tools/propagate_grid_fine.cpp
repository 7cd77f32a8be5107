// The fine plan of the FFT form of the finite-distance propagator (csrc/propagate_grid.h GridFinePlan) for given sizes, on
// the host:
//   propagate_grid_fine nx ny mx my sx sy want_h cache_kernels [tile_lx tile_ly]
//                                        ->  sx=... sy=... ax=... ay=... mcx=... mcy=... cached=... Lx=... Ly=... cx=... cy=...
//                                            bx=... by=... tiles=... batch=... outputs=... plane_bytes=... workspace_bytes=...
//                                            (mx, my: the fine targets; tile lengths of 0: the default)
//                                            or  refused=1 followed by the message on a line of its own
//   propagate_grid_fine lattice m s      ->  a=... m_a=... per active lattice of one axis, a line each
#include <cstdlib>
#include <cstring>

#include "propagate_grid.h"

int main(int argc, char **argv) {
    using namespace ml;
    if (argc == 4 && !strcmp(argv[1], "lattice")) {
        const int m = atoi(argv[2]), s = atoi(argv[3]);
        if (m < 1 || s < 1 || s > GRID_FINE_S_MAX) {
            fprintf(stderr, "lattice: m >= 1 and 1 <= s <= %d\n", GRID_FINE_S_MAX);
            return 2;
        }
        for (int a = 0; a < grid_fine_active(m, s); ++a) printf("a=%d m_a=%d\n", a, grid_fine_lattice_count(m, s, a));
        return 0;
    }
    if (argc != 9 && argc != 11) {
        fprintf(stderr, "usage: propagate_grid_fine nx ny mx my sx sy want_h cache_kernels [tile_lx tile_ly] | lattice m s\n");
        return 2;
    }
    const int mx = atoi(argv[3]), my = atoi(argv[4]);
    if (mx < 1 || my < 1) {
        fprintf(stderr, "mx, my >= 1\n");
        return 2;
    }
    const int tile_lx = argc == 11 ? atoi(argv[9]) : 0, tile_ly = argc == 11 ? atoi(argv[10]) : 0;
    GridFinePlan p;
    char why[480];
    if (grid_fine_plan(atoi(argv[1]), atoi(argv[2]), mx, my, atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), tile_lx, tile_ly,
                       atoi(argv[8]), GRID_TILE_BATCH_BYTES, &p, why, sizeof why) != 0) {
        printf("refused=1\n%s\n", why);
        return 0;
    }
    const GridTilePlan &t = p.tile;
    printf("sx=%d sy=%d ax=%d ay=%d mcx=%d mcy=%d cached=%d Lx=%d Ly=%d cx=%d cy=%d bx=%d by=%d tiles=%d batch=%d outputs=%d "
           "plane_bytes=%lld workspace_bytes=%lld\n",
           p.sx, p.sy, p.ax, p.ay, p.m_cx, p.m_cy, p.cache_kernels, t.x.L, t.y.L, t.x.c, t.y.c, t.x.B, t.y.B, t.tiles, t.batch,
           t.outputs, (long long)t.plane_bytes, (long long)p.workspace_bytes);
    return 0;
}
