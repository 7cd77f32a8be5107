// Host emulation of the tiled stage-1 result and of the column pass over it (metalens_amd/csrc/zfft_core.h tile_off,
// tl_*; zfft.hip zfft_tiles_kernel): rows are stored into tiles by tile_off, then the kernel's per-thread phases run
// thread by thread, round by round, on one tile and are checked against a direct DFT of every column in long double.
// Also reports the LDS cycles of one round against the conflict-free count.
// Build + run:  make -C tools zfft_tiles_emul && tools/zfft_tiles_emul
// With arguments, one column pass of tests/fft_cases.py instead of the built-in cases (resident samples [a0, a0 + h0)
// of the columns):  tools/zfft_tiles_emul R3 a0 h0 M j0
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metalens_amd/csrc/zfft_core.h"

using zf::cd;

static cd expi(long double a) { return zf::mk((double)cosl(a), (double)sinl(a)); }

// N = 256 R3 lattice, resident samples [a0, a0 + h0) (the rest read as zero), M wanted bins from j0; two tiles of a
// plane (16 columns), tile 1 transformed.  Returns the error relative to the largest output.
static double run(int R3, int a0, int h0, int M, int j0, int ld_skew) {
    const int N = 256 * R3, n_res = h0, ld = n_res + ld_skew;
    const long long tile = 8LL * ld;
    srand(R3 * 131 + M + a0);
    // stage 1's rows: 16 bins per resident row n1 (q = n1 - a0), stored as the PASS 4 kernel does
    std::vector<cd> buf(2 * tile, zf::mk(NAN, NAN));
    std::vector<std::vector<cd>> col(16, std::vector<cd>(N, zf::mk(0, 0)));
    for (int q = 0; q < n_res; ++q)
        for (int j = 0; j < 16; ++j) {
            const cd x = zf::mk(rand() / (double)RAND_MAX - 0.5, rand() / (double)RAND_MAX - 0.5);
            buf[q * 8 + zf::tile_off(j, tile)] = x;
            col[j][a0 + q] = x;
        }
    // the column pass on tile 1
    constexpr int S = zf::TL_SLOTS, NT = zf::TL_NT;
    const cd *in = buf.data() + tile;
    std::vector<cd> lds((size_t)S * zf::TL_SS, zf::mk(NAN, NAN));
    std::vector<std::vector<cd>> acc(M, std::vector<cd>(8, zf::mk(0, 0)));
    std::vector<int> kb(M);
    std::vector<cd> wk(M);
    for (int o = 0; o < M; ++o) {
        kb[o] = (((o + j0) % N) + N) % N;
        wk[o] = expi(-2 * M_PIl * kb[o] / N);
    }
    const int rounds = (R3 + S - 1) / S;
    for (int i = 0; i < rounds; ++i) {
        for (int tid = 0; tid < NT; ++tid) {
            const int s = zf::tl_slot(tid), c = zf::tl_col(tid), m1 = zf::tl_sub(tid), n0 = R3 - 1 - S * i - s;
            cd v[16], ta[4], tb[4];
            for (int m2 = 0; m2 < 16; ++m2) {
                const int n = n0 + R3 * (m1 + 16 * m2);
                v[m2] = (n0 >= 0 && n >= a0 && n < a0 + h0) ? in[8 * (n - a0) + c] : zf::mk(0, 0);
            }
            for (int q = 0; q < 4; ++q) {
                tb[q] = expi(-2 * M_PIl * ((m1 * q) % 256) / 256);
                ta[q] = expi(-2 * M_PIl * ((m1 * 4 * q) % 256) / 256);
            }
            zf::tl_phaseA(tid, v, ta, tb, lds.data());
        }
        // phase B in place: thread by thread, no barrier in between
        for (int tid = 0; tid < NT; ++tid) {
            cd u[16];
            zf::tl_phaseB(tid, u, lds.data());
        }
        for (int o = 0; o < M; ++o)
            for (int s = 0; s < S && R3 - 1 - S * i - s >= 0; ++s)
                for (int c = 0; c < 8; ++c) acc[o][c] = zf::cmac(acc[o][c], wk[o], zf::tl_bin(s, c, kb[o], lds.data()));
    }
    double worst = 0, scale = 0;
    for (int c = 0; c < 8; ++c)
        for (int o = 0; o < M; ++o) {
            long double re = 0, im = 0;
            for (int n = 0; n < N; ++n) {
                const cd x = col[8 + c][n];
                if (x.x == 0 && x.y == 0) continue;
                const long double a = -2 * M_PIl * (long double)(((long long)kb[o] * n) % N) / N;
                re += x.x * cosl(a) - x.y * sinl(a);
                im += x.x * sinl(a) + x.y * cosl(a);
            }
            worst = fmax(worst, (double)hypotl(acc[o][c].x - re, acc[o][c].y - im));
            scale = fmax(scale, (double)hypotl(re, im));
        }
    const zf::TileCost tc = zf::tile_cost(M, j0);
    const double rel = worst / scale;
    printf("tiles: N= %d resident= [%d, %d) M= %d j0= %d  rel err %.3e  LDS cycles per round a/b_r/b_w/horner "
           "%ld/%ld/%ld/%ld = %ld (conflict-free %ld)\n",
           N, a0, a0 + h0, M, j0, rel, tc.a_write, tc.b_read, tc.b_write, tc.horner,
           tc.a_write + tc.b_read + tc.b_write + tc.horner, tc.ideal);
    return rel;
}

int main(int argc, char **argv) {
    double worst = 0;
    if (argc > 1) {
        if (argc != 6) return fprintf(stderr, "usage: %s [R3 a0 h0 M j0]\n", argv[0]), 2;
        int v[5];
        for (int k = 0; k < 5; ++k) v[k] = atoi(argv[k + 1]);
        if (v[0] < 1 || v[1] < 0 || v[2] < 1 || v[1] + v[2] > 256 * v[0] || v[3] < 1 || v[3] > zf::TL_NT)
            return fprintf(stderr, "no such column pass\n"), 2;
        worst = run(v[0], v[1], v[2], v[3], v[4], 8);
        printf("worst rel err %.3e -> %s\n", worst, worst <= 1e-15 ? "OK" : "FAIL");
        return worst <= 1e-15 ? 0 : 1;
    }
    worst = fmax(worst, run(16, 0, 4096, 512, -256, 8));    // the benchmark's geometry
    worst = fmax(worst, run(16, 150, 3796, 512, -250, 8));  // trimmed rows, a window not on a 256 boundary
    worst = fmax(worst, run(8, 0, 2000, 256, 3, 8));        // a lattice longer than the aperture
    worst = fmax(worst, run(5, 7, 1270, 500, 0, 8));        // residues not a multiple of TL_SLOTS
    const bool ok = worst <= 1e-15;
    printf("worst rel err %.3e -> %s\n", worst, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}
