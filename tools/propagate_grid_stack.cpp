// The stack plan of the FFT form of the finite-distance propagator (csrc/propagate_grid.h GridStackPlan) for given sizes
// and planes, on the host:
//   propagate_grid_stack nx ny mx my sx sy want_h cache_kernels tile_lx tile_ly [z ...]
//                                        ->  nz=... layers=... sx=... sy=... ax=... ay=... mcx=... mcy=... cached=... Lx=... Ly=...
//                                            cx=... cy=... bx=... by=... tiles=... batch=... outputs=... plane_bytes=...
//                                            workspace_bytes=... fill_layers=...
//                                            (fill_layers: the layers per fill launch of a streamed pair and batch)
//                                            (mx, my: the fine targets of one plane; tile lengths of 0: the default; a z
//                                            written COUNT*VALUE stands for COUNT planes at VALUE)
//                                            or  refused=1 followed by the message on a line of its own
//   propagate_grid_stack layers nz ax ay ->  l=... p=... a=... b=... per layer in contraction order, a line each, then
//                                            pair=l0,l1 (or pair=l0 for the single remainder) per contraction, a line each
#include <cstdlib>
#include <cstring>

#include "propagate_grid.h"

int main(int argc, char **argv) {
    using namespace ml;
    if (argc == 5 && !strcmp(argv[1], "layers")) {
        const int nz = atoi(argv[2]), ax = atoi(argv[3]), ay = atoi(argv[4]);
        if (nz < 1 || nz > GRID_STACK_PLANES_MAX || ax < 1 || ax > GRID_FINE_S_MAX || ay < 1 || ay > GRID_FINE_S_MAX) {
            fprintf(stderr, "layers: 1 <= nz <= %d and 1 <= ax, ay <= %d\n", GRID_STACK_PLANES_MAX, GRID_FINE_S_MAX);
            return 2;
        }
        const int layers = nz * ax * ay;
        for (int l = 0; l < layers; ++l) {
            const GridStackLayer s = grid_stack_layer(l, ax, ay);
            printf("l=%d p=%d a=%d b=%d\n", l, s.p, s.a, s.b);
        }
        for (int l0 = 0; l0 < layers; l0 += GRID_FINE_PAIR) {
            printf("pair=%d", l0);
            for (int l = l0 + 1; l < l0 + GRID_FINE_PAIR && l < layers; ++l) printf(",%d", l);
            printf("\n");
        }
        return 0;
    }
    if (argc < 11) {
        fprintf(stderr, "usage: propagate_grid_stack nx ny mx my sx sy want_h cache_kernels tile_lx tile_ly [z ...] | layers nz ax ay\n");
        return 2;
    }
    const int mx = atoi(argv[3]), my = atoi(argv[4]);
    if (mx < 1 || my < 1) {
        fprintf(stderr, "mx, my >= 1\n");
        return 2;
    }
    std::vector<double> z;
    for (int i = 11; i < argc; ++i) {
        const char *star = strchr(argv[i], '*');
        const long count = star ? atol(argv[i]) : 1;
        if (count < 1 || count > 2 * GRID_STACK_PLANES_MAX) {
            fprintf(stderr, "COUNT*VALUE: 1 <= COUNT <= %d\n", 2 * GRID_STACK_PLANES_MAX);
            return 2;
        }
        z.insert(z.end(), (size_t)count, atof(star ? star + 1 : argv[i]));
    }
    GridStackPlan s;
    char why[480];
    if (grid_stack_plan(atoi(argv[1]), atoi(argv[2]), mx, my, atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[9]), atoi(argv[10]),
                        atoi(argv[8]), GRID_TILE_BATCH_BYTES, z.data(), (int)z.size(), &s, why, sizeof why) != 0) {
        printf("refused=1\n%s\n", why);
        return 0;
    }
    const GridFinePlan &p = s.fine;
    const GridTilePlan &t = p.tile;
    printf("nz=%d layers=%d sx=%d sy=%d ax=%d ay=%d mcx=%d mcy=%d cached=%d Lx=%d Ly=%d cx=%d cy=%d bx=%d by=%d tiles=%d batch=%d "
           "outputs=%d plane_bytes=%lld workspace_bytes=%lld fill_layers=%d\n",
           s.nz, s.layers, p.sx, p.sy, p.ax, p.ay, p.m_cx, p.m_cy, p.cache_kernels, t.x.L, t.y.L, t.x.c, t.y.c, t.x.B, t.y.B, t.tiles,
           t.batch, t.outputs, (long long)t.plane_bytes, (long long)s.workspace_bytes,
           grid_stack_fill_layers(s.layers < GRID_FINE_PAIR ? s.layers : GRID_FINE_PAIR, t.batch, t.plane_bytes));
    return 0;
}
