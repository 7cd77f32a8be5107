// Host emulation of the mixed-radix pruned FFT (metalens_amd/csrc/zfft_core.h mx_*, zfft.hip zfft_mixed_kernel): the
// factor chooser picks N s = A B R, then the kernel's per-thread phases run thread by thread against a direct DFT on
// the lattice asked for, in long double.  Prints per case the relative error and the LDS cycles of the chosen
// padding next to the conflict-free count, the error of the 16 x 16 x R3 programme on the same kind of input (the
// yardstick for the mixed cases), and the chooser's answer for every 2^a 3^b 5^c in [256, 8192].
// With arguments it runs the cases named there instead and prints their `mixed:` lines only:
//     --case N valid M j0 a0 h0 a1 h1     (repeatable; tests/mixed_cases.py holds the table the suite passes)
// Build + run:  make -C tools zfft_mixed_emul && tools/zfft_mixed_emul
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metalens_amd/csrc/zfft_core.h"

using zf::cd;

static cd expi(long double a) { return zf::mk((double)cosl(a), (double)sinl(a)); }

// samples n in [a0, a0 + h0) and [a1, a1 + h1) below n_valid are resident, everything else reads as zero
static std::vector<cd> make_input(int N, int n_valid, int a0, int h0, int a1, int h1, unsigned seed) {
    std::vector<cd> in(N, zf::mk(0, 0));
    srand(seed);
    for (int n = 0; n < N; ++n) {
        const bool res = (n >= a0 && n < a0 + h0) || (n >= a1 && n < a1 + h1);
        if (n < n_valid && res) in[n] = zf::mk(rand() / (double)RAND_MAX - 0.5, rand() / (double)RAND_MAX - 0.5);
    }
    return in;
}

// largest component error of out[j] against sum_n in[n] W_N^(n (j + j0)), relative to the largest component
static double rel_err(const std::vector<cd> &in, int N, const std::vector<cd> &out, int j0) {
    double worst = 0, scale = 0;
    for (size_t j = 0; j < out.size(); ++j) {
        const long long k = ((((long long)j + j0) % N) + N) % N;
        long double re = 0, im = 0;
        for (int n = 0; n < N; ++n) {
            if (in[n].x == 0 && in[n].y == 0) continue;
            const long double a = -2 * M_PIl * (long double)((n * k) % N) / N;
            re += in[n].x * cosl(a) - in[n].y * sinl(a);
            im += in[n].x * sinl(a) + in[n].y * cosl(a);
        }
        worst = fmax(worst, fmax(fabs((double)(re - out[j].x)), fabs((double)(im - out[j].y))));
        scale = fmax(scale, (double)fmaxl(fabsl(re), fabsl(im)));
    }
    return worst / scale;
}

template <int A, int B>
static double run_pair(const zf::MixChoice &ch, int N, int n_valid, int M, int j0, const std::vector<cd> &in,
                       zf::MixCost *cost, int *pad) {
    zf::Geo g{ch.R, n_valid, M, j0, 0, 0, 0, ch.s};
    zf::mixed_choose_pad<A, B>(g);
    const int R = ch.R, Ne = A * B * R;
    std::vector<cd> lds(zf::mx_lds_elems<A, B>(g), zf::mk(NAN, NAN)), tw(A * B);
    for (int k2 = 0; k2 < A; ++k2)
        for (int n1 = 0; n1 < B; ++n1) tw[k2 * B + n1] = expi(-2 * M_PIl * ((n1 * k2) % (A * B)) / (A * B));
    for (int t = 0; t < B * R; ++t) {
        cd v[A];
        for (int n2 = 0; n2 < A; ++n2) {
            const int n = t + B * R * n2;   // sample of the (s-fold padded) lattice = sample of the aperture
            v[n2] = n < N ? in[n] : zf::mk(0, 0);
        }
        zf::mx_stage1<A, B>(g, t, v, tw.data(), lds.data());
    }
    for (int u = 0; u < A * R; ++u) {   // in place, thread by thread, no barrier in between
        cd v[B];
        zf::mx_stage2<A, B>(g, u, v, lds.data());
    }
    std::vector<cd> out(M);
    for (int j = 0; j < M; ++j) {
        const int k = zf::mx_bin_of<A, B>(g, j);
        out[j] = zf::mx_stage3<A, B>(g, k, expi(-2 * M_PIl * k / Ne), lds.data());
    }
    *cost = zf::mixed_cost<A, B>(g);
    *pad = g.pad1;
    return rel_err(in, N, out, j0);
}

static double run_mixed(int N, int n_valid, int M, int j0, int a0, int h0, int a1, int h1) {
    const zf::MixChoice ch = zf::mixed_choose(N, M);
    if (!ch.s) {
        printf("mixed: N= %d M= %d: no factorisation\n", N, M);
        return 1.0;
    }
    const std::vector<cd> in = make_input(N, n_valid, a0, h0, a1, h1, N * 7919 + M);
    zf::MixCost c;
    int pad = 0;
    double rel = 1.0;
#define RUN(AA, BB) \
    if (ch.A == AA && ch.B == BB) rel = run_pair<AA, BB>(ch, N, n_valid, M, j0, in, &c, &pad);
    ZF_MX_PAIRS(RUN)
#undef RUN
    printf("mixed: N= %d valid= %d resident= [%d, %d) + [%d, %d) M= %d j0= %d  s= %d A= %d B= %d R= %d pad= %d  rel err %.3e  "
           "LDS cycles s1_w/s2_r/s2_w/horner %ld/%ld/%ld/%ld = %ld (conflict-free %ld)\n",
           N, n_valid, a0, a0 + h0, a1, a1 + h1, M, j0, ch.s, ch.A, ch.B, ch.R, pad, rel, c.s1_write, c.s2_read,
           c.s2_write, c.horner, c.total(), c.ideal);
    return rel;
}

// the 16 x 16 x R3 programme (stage1_regs, gather2, scatter2, stage3) on the same kind of input
static double run_base(int R3, int M, int j0) {
    zf::Geo g{R3, 256 * R3, M, j0, 0, 0};
    zf::choose_pads(g);
    const int NT = 16 * R3, N = 256 * R3;
    const std::vector<cd> in = make_input(N, N, 0, N, 0, 0, N * 7919 + M);
    std::vector<cd> lds(zf::lds_elems(g));
    std::vector<std::vector<cd>> v(NT, std::vector<cd>(16));
    for (int t = 0; t < NT; ++t) {
        cd ta[4], tb[4];
        const int n1 = t / R3;
        for (int q = 0; q < 4; ++q) {
            tb[q] = expi(-2 * M_PIl * ((n1 * q) % 256) / 256);
            ta[q] = expi(-2 * M_PIl * ((n1 * 4 * q) % 256) / 256);
        }
        for (int n2 = 0; n2 < 16; ++n2) v[t][n2] = in[t + NT * n2];
        zf::stage1_regs(g, t, v[t].data(), ta, tb, lds.data());
    }
    for (int u = 0; u < NT; ++u) zf::gather2(g, u, v[u].data(), lds.data());
    for (int u = 0; u < NT; ++u) zf::scatter2(g, u, v[u].data(), lds.data());
    std::vector<cd> out(M);
    for (int j = 0; j < M; ++j) {
        const int k = zf::bin_of(g, j);
        out[j] = zf::stage3(g, k, expi(-2 * M_PIl * k / N), lds.data());
    }
    const double rel = rel_err(in, N, out, j0);
    printf("base16: N= %d M= %d j0= %d  rel err %.3e\n", N, M, j0, rel);
    return rel;
}

// the cases of the command line; 0 when every one ran, 2 on a malformed argument or a lattice without factorisation
static int run_cases(int argc, char **argv) {
    int status = 0;
    for (int i = 1; i < argc; i += 9) {
        if (strcmp(argv[i], "--case") || i + 8 >= argc) {
            fprintf(stderr, "usage: %s [--case N valid M j0 a0 h0 a1 h1]...\n", argv[0]);
            return 2;
        }
        int v[8];
        for (int k = 0; k < 8; ++k) v[k] = atoi(argv[i + 1 + k]);
        if (v[0] < 1 || v[1] < 1 || v[1] > v[0] || v[2] < 1 || v[2] > v[0]) {
            fprintf(stderr, "--case %d %d %d ...: need 1 <= valid <= N and 1 <= M <= N\n", v[0], v[1], v[2]);
            return 2;
        }
        if (!zf::mixed_choose(v[0], v[2]).s) status = 2;
        run_mixed(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
    }
    return status;
}

int main(int argc, char **argv) {
    if (argc > 1) return run_cases(argc, argv);
    const double base = fmax(run_base(16, 512, -256), run_base(32, 1024, -512));
    double worst = 0;
    worst = fmax(worst, run_mixed(400, 400, 400, -200, 0, 400, 0, 0));
    worst = fmax(worst, run_mixed(1000, 1000, 256, -128, 0, 1000, 0, 0));
    worst = fmax(worst, run_mixed(1440, 1440, 1440, -720, 0, 1440, 0, 0));
    worst = fmax(worst, run_mixed(2000, 2000, 64, -30, 0, 2000, 0, 0));       // straddles bin 0
    worst = fmax(worst, run_mixed(3000, 3000, 300, 100, 0, 3000, 0, 0));      // a window without bin 0
    worst = fmax(worst, run_mixed(3600, 3600, 512, -256, 0, 3600, 0, 0));
    worst = fmax(worst, run_mixed(3600, 3600, 3600, -1800, 0, 3600, 0, 0));
    worst = fmax(worst, run_mixed(3600, 90, 3600, -1800, 0, 3600, 0, 0));     // an aperture shorter than its lattice
    worst = fmax(worst, run_mixed(2400, 2300, 500, -250, 100, 700, 1500, 700));   // two resident runs (a mirrored shard)
    worst = fmax(worst, run_mixed(729, 729, 729, -364, 0, 729, 0, 0));        // R = 9 is not 5-smooth-limited: 9 x 9 x 9
    worst = fmax(worst, run_mixed(1920, 1920, 240, -120, 0, 1920, 0, 0));
    // the chooser on every 2^a 3^b 5^c in [256, 8192], all bins wanted
    for (int N = 256; N <= 8192; ++N) {
        int r = N;
        for (int p : {2, 3, 5})
            while (r % p == 0) r /= p;
        if (r != 1) continue;
        const zf::MixChoice ch = zf::mixed_choose(N, N);
        if (ch.s)
            printf("choose: N= %d s= %d A= %d B= %d R= %d\n", N, ch.s, ch.A, ch.B, ch.R);
        else
            printf("choose: N= %d none\n", N);
    }
    const bool ok = worst <= 2 * base;
    printf("worst mixed rel err %.3e, 16 x 16 x R3 rel err %.3e -> %s\n", worst, base, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}
