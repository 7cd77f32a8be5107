// Host check of what zfft_rows_kernel (csrc/zfft_rows.hip) decides without arithmetic per lane and load, through the
// functions the kernel itself calls (csrc/zfft_core.h): the residency of every sample against load_row's predicate,
// the rows a workgroup walks and their quotients and remainders against plain division, and which calls the kernel
// takes.  Plain host code (tests/test_zfft_rows_host.py builds it under the address and undefined-behaviour
// sanitizers); prints one line per part, exit status 1 on the first disagreement.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "zfft_core.h"

static int fail(const char *what, long a, long b, long c, long d) {
    std::printf("FAIL %s: %ld %ld %ld %ld\n", what, a, b, c, d);
    return 1;
}

// every lane of every load of every wave, as rows_load computes it, against min(n, n_valid - 1 - n) >= first
static int check_residency() {
    long lanes = 0, loads = 0, skipped = 0;
    const int n_valids[] = {2048, 1900, 4096, 3793};
    for (int n_valid : n_valids)
        for (int NT : {128, 256}) {
            if (n_valid > 16 * NT) continue;
            std::vector<int> firsts;
            for (int f = 0; f <= n_valid / 2; ++f) firsts.push_back(f);
            firsts.push_back(n_valid / 2 + 1);
            firsts.push_back(n_valid);
            firsts.push_back(0x7f7f7f7f);   // row_extent_kernel's value for a row outside the lens
            for (int first : firsts) {
                int lo, hi;
                zf::row_run(first, n_valid, lo, hi);
                if (lo > hi || lo < 0 || hi > n_valid) return fail("run", n_valid, first, lo, hi);
                for (int wave = 0; wave < NT / 64; ++wave)
                    for (int n2 = 0; n2 < 16; ++n2) {
                        bool any = false;
                        for (int lane = 0; lane < 64; ++lane) {
                            const int tid = 64 * wave + lane, rel = tid - lo, n = tid + NT * n2;
                            const bool got = zf::piece_lane(rel + NT * n2, 0, hi - lo);
                            const bool want = std::min(n, n_valid - 1 - n) >= first;
                            if (got != want) return fail("lane", n_valid, first, n, got);
                            if (got && n >= n_valid) return fail("bounds", n_valid, first, n, got);
                            any |= got;
                            ++lanes;
                        }
                        ++loads;
                        skipped += !any;
                    }
            }
        }
    std::printf("residency ok: %ld lanes, %ld loads, %ld skipped\n", lanes, loads, skipped);
    return 0;
}

// every workgroup of a launch: its rows, and (q, r) of the four divisors along them
static int check_walk() {
    long turns = 0, zero = 0, one = 0, odd = 0, even = 0;
    for (int n : {24, 40, 23, 37, 3796})
        for (int grid : {0, 8, 16, 24, 40, 512}) {
            const int rows = 4 * n, chunk = (rows + 7) / 8;
            int g = grid ? std::min(grid, chunk * 8) : std::min(512, chunk * 8);   // (zfft.hip zfft_run)
            g = (g + 7) / 8 * 8;
            const int step = g / 8;
            const int divisors[4] = {n, n + 3, rows, 7};   // in_rb, out_rb != in_rb, alpha_rb, a short rf_mod
            std::vector<int> seen(rows, 0);
            for (int b = 0; b < g; ++b) {
                const int end = zf::rows_end(b, chunk, rows);
                int row = zf::rows_begin(b, chunk), t = 0;
                if (row < end) {
                    zf::RowWalk w[4];
                    for (int k = 0; k < 4; ++k) w[k] = zf::walk_init(row, divisors[k], step);
                    for (; row < end; row += step, ++t) {
                        if (row < 0 || row >= rows) return fail("row", n, g, b, row);
                        ++seen[row];
                        for (int k = 0; k < 4; ++k) {
                            if (w[k].q != row / divisors[k] || w[k].r != row % divisors[k])
                                return fail("walk", n, g, row, divisors[k]);
                            zf::walk_step(w[k]);
                        }
                    }
                }
                turns += t;
                zero += t == 0, one += t == 1, odd += t > 1 && t % 2, even += t > 1 && t % 2 == 0;
            }
            for (int r = 0; r < rows; ++r)
                if (seen[r] != 1) return fail("coverage", n, g, r, seen[r]);
        }
    if (!zero || !one || !odd || !even) return fail("turn patterns", zero, one, odd, even);
    std::printf("walk ok: %ld turns; workgroups with 0 / 1 / odd / even turns: %ld %ld %ld %ld\n", turns, zero, one, odd,
                even);
    return 0;
}

static int check_takes() {
    zf::RowsFacts f;
    f.family_one = f.ip = true;
    f.PASS = 4, f.R3 = 16, f.M = 512, f.n_valid = 4096, f.h0 = 4096, f.out_last = 63 * 8 * 4104 + 7;
    int bad = 0, n = 0;
    auto want = [&](zf::RowsFacts g, bool takes) { ++n, bad += zf::rows_kernel_takes(g) != takes; };
    auto with = [&](auto set) { zf::RowsFacts g = f; set(g); return g; };
    want(f, true);
    want(with([](zf::RowsFacts &g) { g.PASS = 1; }), true);
    want(with([](zf::RowsFacts &g) { g.R3 = 8, g.M = 256, g.n_valid = g.h0 = 2048; }), true);
    want(with([](zf::RowsFacts &g) { g.n_valid = 3793; }), true);
    want(with([](zf::RowsFacts &g) { g.PASS = 2; }), false);
    want(with([](zf::RowsFacts &g) { g.PASS = 3; }), false);
    want(with([](zf::RowsFacts &g) { g.family_one = false; }), false);
    want(with([](zf::RowsFacts &g) { g.ip = false; }), false);
    want(with([](zf::RowsFacts &g) { g.R3 = 4, g.M = 128; }), false);
    want(with([](zf::RowsFacts &g) { g.R3 = 32, g.M = 1024; }), false);
    want(with([](zf::RowsFacts &g) { g.M = 300; }), false);
    want(with([](zf::RowsFacts &g) { g.sub_s = 2; }), false);
    want(with([](zf::RowsFacts &g) { g.sub_i = 1; }), false);
    want(with([](zf::RowsFacts &g) { g.in_es = 8; }), false);
    want(with([](zf::RowsFacts &g) { g.a0 = 1; }), false);
    want(with([](zf::RowsFacts &g) { g.h0 = 4000; }), false);
    want(with([](zf::RowsFacts &g) { g.a1 = 2048, g.h1 = 100; }), false);   // two resident runs
    want(with([](zf::RowsFacts &g) { g.accumulate = 1; }), false);
    want(with([](zf::RowsFacts &g) { g.n_valid = g.h0 = 4097; }), false);
    want(with([](zf::RowsFacts &g) { g.out_last = 1LL << 27; }), false);
    if (bad) return fail("takes", bad, n, 0, 0);
    std::printf("takes ok: %d calls\n", n);
    return 0;
}

int main() { return check_residency() || check_walk() || check_takes(); }
