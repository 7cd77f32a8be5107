// Output-pruned FFT along one aperture axis: the per-thread programme of zfft.hip.
//
// For a direction grid that sits ON the FFT lattice of the aperture - u_j = (j + j0) du with
// kappa * step * du = 1 / N_eff (N_eff >= the number of samples; the reference's own far field is
// exactly this lattice, nearfield_farfield.py:35-39) - the aperture -> direction sum along one
// axis
//
//     G[j] = sum_n F[n] exp(-2 pi i (n - c)(j + j0) / N_eff)            (nearfield_farfield.py:111-120)
//
// is M consecutive bins of an N_eff-point DFT.  N_eff = 256 R3 is factored 16 x 16 x R3:
//
//     n = n0 + R3 n1 + 16 R3 n2      (n0 < R3, n1 < 16, n2 < 16)
//     k = k2 + 16 k1 + 256 k0        (k2 < 16, k1 < 16, k0 < R3)
//     n k = 16 R3 n2 k2  +  R3 n1 k2 + 16 R3 n1 k1  +  n0 k      (mod N_eff)
//
//   stage 1  (thread t = n0 + R3 n1 holds its 16 samples n2)   A[k2]  = DFT16 over n2, times W_256^(n1 k2)
//   exchange 1 through LDS
//   stage 2  (thread u = n0 + R3 k2 holds n1 = 0..15)          B[k1]  = DFT16 over n1
//   exchange 2 through LDS
//   stage 3  (one thread per WANTED bin k)                      X[k]   = sum_n0 B[n0,k1,k2] (W_N^k)^n0
//
// The last stage is where the pruning happens: only the M wanted bins are evaluated, each by a
// Horner sum over the R3 residues (a full radix-R3 butterfly would produce R3 bins per group of
// which M / 256 are wanted).  Everything before it is an ordinary FFT: 2 x 16-point butterflies
// per 16 samples instead of M / 2 real multiply-adds per sample in the folded GEMM (zfold.hip).
//
// This header is compiled twice: by hipcc into zfft.hip (device), and by the host compiler into
// tools/zfft_emul.cpp, which runs the same per-thread functions thread by thread, phase by phase,
// against a direct DFT and counts LDS bank conflicts (there is no GPU in the build container).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ZF_HD __host__ __device__ __forceinline__
#else
#define ZF_HD inline
#include <cmath>
#endif

namespace zf {

struct alignas(16) cd {
    double x, y;
};

ZF_HD cd mk(double x, double y) {
    cd r;
    r.x = x;
    r.y = y;
    return r;
}
ZF_HD cd cadd(cd a, cd b) { return mk(a.x + b.x, a.y + b.y); }
ZF_HD cd csub(cd a, cd b) { return mk(a.x - b.x, a.y - b.y); }
// explicit fma: the translation units are built with -ffp-contract=off
ZF_HD cd cmul(cd a, cd b) {
    return mk(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x));
}
// a * b + c
ZF_HD cd cmac(cd a, cd b, cd c) {
    return mk(fma(a.x, b.x, fma(-a.y, b.y, c.x)), fma(a.x, b.y, fma(a.y, b.x, c.y)));
}
ZF_HD cd mul_mi(cd a) { return mk(a.y, -a.x); }   // a * (-i)

// forward 4-point DFT in place: (a, b, c, d) <- (X0, X1, X2, X3), X_k = sum x_n (-i)^(n k)
ZF_HD void dft4(cd &a, cd &b, cd &c, cd &d) {
    const cd t0 = cadd(a, c), t1 = csub(a, c), t2 = cadd(b, d), t3 = mul_mi(csub(b, d));
    a = cadd(t0, t2);
    c = csub(t0, t2);
    b = cadd(t1, t3);
    d = csub(t1, t3);
}

// forward 16-point DFT in place.  Input v[n]; output bin k = d + 4 c ends up in v[c + 4 d]
// (digit-reversed: use bin16()).
constexpr double C1 = 0.92387953251128673848;   // cos(pi/8)
constexpr double S1 = 0.38268343236508978178;   // sin(pi/8)
constexpr double RH = 0.70710678118654757274;   // sqrt(1/2)

ZF_HD void dft16(cd *v) {
#pragma unroll
    for (int a = 0; a < 4; ++a) dft4(v[a], v[a + 4], v[a + 8], v[a + 12]);
    // v[a + 4 d] *= W_16^(a d)
    v[1 + 4] = cmul(v[1 + 4], mk(C1, -S1));                              // W^1
    v[1 + 8] = mk((v[1 + 8].x + v[1 + 8].y) * RH, (v[1 + 8].y - v[1 + 8].x) * RH);   // W^2 = (1 - i) / sqrt 2
    v[1 + 12] = cmul(v[1 + 12], mk(S1, -C1));                            // W^3
    v[2 + 4] = mk((v[2 + 4].x + v[2 + 4].y) * RH, (v[2 + 4].y - v[2 + 4].x) * RH);   // W^2
    v[2 + 8] = mul_mi(v[2 + 8]);                                         // W^4 = -i
    v[2 + 12] = mk((v[2 + 12].y - v[2 + 12].x) * RH, -(v[2 + 12].x + v[2 + 12].y) * RH);   // W^6 = (-1 - i) / sqrt 2
    v[3 + 4] = cmul(v[3 + 4], mk(S1, -C1));                              // W^3
    v[3 + 8] = mk((v[3 + 8].y - v[3 + 8].x) * RH, -(v[3 + 8].x + v[3 + 8].y) * RH);       // W^6
    v[3 + 12] = cmul(v[3 + 12], mk(-C1, S1));                            // W^9
#pragma unroll
    for (int d = 0; d < 4; ++d) dft4(v[4 * d], v[4 * d + 1], v[4 * d + 2], v[4 * d + 3]);
}
// register index that holds bin k after dft16
ZF_HD constexpr int bin16(int k) { return (k >> 2) + 4 * (k & 3); }

// forward 8-point DFT in place, natural order: v[k] <- sum_n v[n] W_8^(n k)   (the column pass of an interleaved
// row shard whose short transforms have 128 = 16 x 8 samples: zfft.hip zfft_cols128_kernel)
ZF_HD void dft8(cd *v) {
    // even / odd halves as 4-point transforms (dft4 returns natural order)
    cd e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6], o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
    dft4(e0, e1, e2, e3);
    dft4(o0, o1, o2, o3);
    o1 = mk((o1.x + o1.y) * RH, (o1.y - o1.x) * RH);    // W_8^1 = (1 - i) / sqrt 2
    o2 = mul_mi(o2);                                    // W_8^2 = -i
    o3 = mk((o3.y - o3.x) * RH, -(o3.x + o3.y) * RH);   // W_8^3 = (-1 - i) / sqrt 2
    v[0] = cadd(e0, o0);
    v[4] = csub(e0, o0);
    v[1] = cadd(e1, o1);
    v[5] = csub(e1, o1);
    v[2] = cadd(e2, o2);
    v[6] = csub(e2, o2);
    v[3] = cadd(e3, o3);
    v[7] = csub(e3, o3);
}

// ---- geometry of one transform ------------------------------------------------------------
struct Geo {
    int R3;        // N_eff = 256 R3, threads per workgroup NT = 16 R3
    int n_valid;   // samples that exist (n >= n_valid reads as zero)
    int M;         // wanted bins
    int j0;        // bin of output 0 (may be negative)
    int pad1;      // LDS: exchange 1 element (t, k2) lives at t + (NT + pad1) k2
    int pad2;      //      exchange 2 element (n0, k1, k2) at k2 + 16 k1 + (256 + pad2) n0
    // ip != 0: exchange 2 IN PLACE - thread u = n0 + R3 k2 of stage 2 writes its sixteen results
    // (k1 = 0..15) back to the sixteen slots it read (n1 = 0..15): element (n0, k1, k2) lives at
    // exchange 1's address of (t = n0 + R3 k1, k2).  Nobody else touches those slots between the
    // read and the write, so the barrier between them goes, and the last stage finds the R3 residues
    // of a bin in R3 CONSECUTIVE elements.
    int ip;
    // wanted bin of output j = (j + j0) jstep: 1 on the aperture's own lattice padded to 256 R3 samples;
    // s > 1 when the aperture's lattice of N samples is NOT a multiple of 256 long and the transform runs
    // on the s-times finer lattice of N s = 256 R3 samples (the aperture zero-padded), of which every
    // s-th bin is a bin of the aperture's own (zfft.hip zfft_commensurate)
    int jstep = 1;
};
ZF_HD int lds_elems(const Geo &g) {
    const int e1 = (16 * g.R3 + g.pad1) * 16, e2 = (256 + g.pad2) * g.R3;
    return (g.ip || e1 > e2) ? e1 : e2;
}
ZF_HD int ex1_addr(const Geo &g, int t, int k2) { return t + (16 * g.R3 + g.pad1) * k2; }
ZF_HD int ex2_addr(const Geo &g, int n0, int k1, int k2) { return k2 + 16 * k1 + (256 + g.pad2) * n0; }
ZF_HD int ex2ip_addr(const Geo &g, int n0, int k1, int k2) { return ex1_addr(g, n0 + g.R3 * k1, k2); }
// wanted bin of output j, reduced to [0, N_eff)
ZF_HD int bin_of(const Geo &g, int j) {
    const int N = 256 * g.R3;
    long long k = ((long long)(j + g.j0) * g.jstep) % N;
    return (int)(k < 0 ? k + N : k);
}

// ---- the phases, one thread each -------------------------------------------------------------
// stage 1 on the 16 samples v[n2] of thread t: butterflies, the W_256^(n1 k2) twiddles, result to
// exchange 1.  The twiddles W^(k2), W = W_256^(n1), are built from six tabulated powers of the
// thread's W (tb[b] = W^b, ta[a] = W^(4 a), a, b = 1..3; k2 = 4 a + b needs one product): the LDS
// pipe is what bounds the transform and the vector pipe has room, so the kernel keeps tb in
// registers and reads only ta from LDS (3 reads per row instead of 15)
ZF_HD void stage1_regs(const Geo &g, int t, cd *v, const cd *ta, const cd *tb, cd *lds) {
    dft16(v);
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) {
        const int hi = k2 >> 2, lo = k2 & 3;
        cd a = v[bin16(k2)];
        if (hi && lo)
            a = cmul(a, cmul(ta[hi], tb[lo]));
        else if (hi)
            a = cmul(a, ta[hi]);
        else if (lo)
            a = cmul(a, tb[lo]);
        lds[ex1_addr(g, t, k2)] = a;
    }
}
// the same with the twiddles applied IN PLACE in two steps, W^(4a) then W^b (two products per
// element instead of one product of two tabulated values and one per element - the same 24
// complex multiplications per thread, no temporaries): the form of the multi-row and interleaved kernels, whose
// register budget has no room for the nine products.  tw = the [k2][n1] twiddle table in LDS.
ZF_HD void stage1_inplace(const Geo &g, int t, cd *v, const cd *tw, int n1, cd *lds) {
    dft16(v);
#pragma unroll
    for (int lo = 1; lo < 4; ++lo) {
        const cd w = tw[lo * 16 + n1];
#pragma unroll
        for (int hi = 0; hi < 4; ++hi) v[bin16(4 * hi + lo)] = cmul(v[bin16(4 * hi + lo)], w);
    }
#pragma unroll
    for (int hi = 1; hi < 4; ++hi) {
        const cd w = tw[(4 * hi) * 16 + n1];
#pragma unroll
        for (int lo = 0; lo < 4; ++lo) v[bin16(4 * hi + lo)] = cmul(v[bin16(4 * hi + lo)], w);
    }
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) lds[ex1_addr(g, t, k2)] = v[bin16(k2)];
}
// stage 2 for thread u = n0 + R3 k2: gather n1 = 0..15, butterflies, result to exchange 2.
// The caller puts a barrier between gather2() and scatter2() (the two exchanges share the buffer).
ZF_HD void gather2(const Geo &g, int u, cd *v, const cd *lds) {
    const int n0 = u % g.R3, k2 = u / g.R3;
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) v[n1] = lds[ex1_addr(g, n0 + g.R3 * n1, k2)];
    dft16(v);
}
ZF_HD void scatter2(const Geo &g, int u, const cd *v, cd *lds) {
    const int n0 = u % g.R3, k2 = u / g.R3;
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) lds[ex2_addr(g, n0, k1, k2)] = v[bin16(k1)];
}
// exchange 2 in place (Geo::ip): no barrier between gather2() and this
ZF_HD void scatter2_ip(const Geo &g, int u, const cd *v, cd *lds) {
    const int n0 = u % g.R3, k2 = u / g.R3;
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) lds[ex2ip_addr(g, n0, k1, k2)] = v[bin16(k1)];
}
ZF_HD cd stage3_ip(const Geo &g, int k, cd w, const cd *lds) {
    const cd *b = lds + ex2ip_addr(g, 0, (k >> 4) & 15, k & 15);   // the bin's residues: b[0 .. R3)
    cd x = b[g.R3 - 1];
    for (int n0 = g.R3 - 2; n0 >= 0; --n0) x = cmac(x, w, b[n0]);
    return x;
}
ZF_HD void stage3_pair_ip(const Geo &g, int k, cd wa, cd wb, const cd *lds, cd &xa, cd &xb) {
    const cd *b = lds + ex2ip_addr(g, 0, (k >> 4) & 15, k & 15);
    xa = xb = b[g.R3 - 1];
    for (int n0 = g.R3 - 2; n0 >= 0; --n0) {
        const cd t = b[n0];
        xa = cmac(xa, wa, t);
        xb = cmac(xb, wb, t);
    }
}
// stage 3 for ONE wanted bin k: Horner over the residues with ratio w = W_N^k
ZF_HD cd stage3(const Geo &g, int k, cd w, const cd *lds) {
    const int k2 = k & 15, k1 = (k >> 4) & 15;
    cd x = lds[ex2_addr(g, g.R3 - 1, k1, k2)];
    for (int n0 = g.R3 - 2; n0 >= 0; --n0) x = cmac(x, w, lds[ex2_addr(g, n0, k1, k2)]);
    return x;
}

// ... for TWO wanted bins k and kb with kb = k (mod 256): they differ in k0 only and sum the same
// R3 values with different ratios, so each value is read from LDS once
ZF_HD void stage3_pair(const Geo &g, int k, cd wa, cd wb, const cd *lds, cd &xa, cd &xb) {
    const int k2 = k & 15, k1 = (k >> 4) & 15;
    xa = xb = lds[ex2_addr(g, g.R3 - 1, k1, k2)];
    for (int n0 = g.R3 - 2; n0 >= 0; --n0) {
        const cd t = lds[ex2_addr(g, n0, k1, k2)];
        xa = cmac(xa, wa, t);
        xb = cmac(xb, wb, t);
    }
}

// ---- the column pass over a TILED stage-1 result (zfft.hip zfft_tiles_kernel) ---------------------
// Tiled G: bin j of row n1 sits at (j / 8) * tile + n1 * 8 + j % 8 (tile = 8 x the pitch along n1), so a
// 128-byte line holds 8 consecutive bins of one row and 8 consecutive lanes of the row pass store a whole line.
ZF_HD long long tile_off(int j, long long tile) { return (long long)(j >> 3) * tile + (j & 7); }
// One workgroup of TL_NT threads transforms the 8 columns of one tile, TL_SLOTS residues n0 of the N = 256 R3
// lattice at a time: slot s holds the sub-sequence n = n0 + R3 m, m = m1 + 16 m2 < 256, of all 8 columns, whose
// 256-point DFT B_n0[k mod 256] is what Horner sums over n0 (X[k] = sum_n0 (W_N^k)^n0 B_n0[k mod 256]).
//   phase A  thread (s, m1, c): DFT16 over m2 of its 16 loaded samples, times W_256^(m1 k2)  -> LDS (s, c, k2, m1)
//   phase B  thread (s, k2, c): DFT16 over m1, result IN PLACE                              -> LDS (s, c, k2, k1)
//   Horner   thread = bin: 8 columns x TL_SLOTS residues
// Strides from the LDS conflict model below (tools/zfft_tiles_emul.cpp reports the cycles).
constexpr int TL_NT = 512, TL_SLOTS = 4, TL_KS = 18, TL_CS = 289, TL_SS = 8 * TL_CS;
ZF_HD int tl_addr(int s, int c, int k2, int m1) { return s * TL_SS + c * TL_CS + k2 * TL_KS + m1; }
ZF_HD int tl_slot(int tid) { return tid >> 7; }
ZF_HD int tl_col(int tid) { return tid & 7; }
ZF_HD int tl_sub(int tid) { return (tid >> 3) & 15; }   // m1 in phase A, k2 in phase B
// phase A; ta / tb: W^(4 a) and W^b of the thread's W = W_256^(m1) (stage1_regs)
ZF_HD void tl_phaseA(int tid, cd *v, const cd *ta, const cd *tb, cd *lds) {
    const int s = tl_slot(tid), c = tl_col(tid), m1 = tl_sub(tid);
    dft16(v);
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) {
        const int hi = k2 >> 2, lo = k2 & 3;
        cd a = v[bin16(k2)];
        if (hi && lo)
            a = cmul(a, cmul(ta[hi], tb[lo]));
        else if (hi)
            a = cmul(a, ta[hi]);
        else if (lo)
            a = cmul(a, tb[lo]);
        lds[tl_addr(s, c, k2, m1)] = a;
    }
}
// phase B: a thread overwrites only the sixteen slots it has just read (no barrier in between)
ZF_HD void tl_phaseB(int tid, cd *v, cd *lds) {
    const int s = tl_slot(tid), c = tl_col(tid), k2 = tl_sub(tid);
#pragma unroll
    for (int m1 = 0; m1 < 16; ++m1) v[m1] = lds[tl_addr(s, c, k2, m1)];
    dft16(v);
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) lds[tl_addr(s, c, k2, k1)] = v[bin16(k1)];
}
// B_n0[k mod 256] of slot s, column c
ZF_HD cd tl_bin(int s, int c, int k, const cd *lds) { return lds[tl_addr(s, c, k & 15, (k >> 4) & 15)]; }


// ---- mixed-radix lattices: N = A x B x R (zfft.hip zfft_mixed_kernel) ------------------------------
// The reference's default grids are the smallest 2^a 3^b 5^c at or above a goal (nearfield.py:30-36): 400, 1000,
// 1440, 2000, 3000, 3600 ... samples, which the 16 x 16 x R3 scheme above only reaches on a 16- or 32-fold padded
// lattice.  The same three stages with two legs A, B from {9, 10, 12, 15, 16} run on the lattice itself:
//
//     n = n0 + R n1 + B R n2      (n0 < R, n1 < B, n2 < A)
//     k = k2 + A k1 + A B k0      (k2 < A, k1 < B, k0 < R)
//     n k = B R n2 k2  +  R n1 k2 + A R n1 k1  +  n0 k      (mod N)
//
//   stage 1  (thread t = n0 + R n1 holds its A samples n2)   A-point DFT over n2, times W_AB^(n1 k2)
//   stage 2  (thread u = n0 + R k2 gathers n1 = 0..B-1)      B-point DFT over n1, result IN PLACE (k1 takes n1's slot)
//   stage 3  (wanted bins only)                              Horner over the R consecutive residues
//
// The legs are compile-time (template arguments), R is Geo::R3 at run time; max(A, B) R threads per workgroup, of
// which B R work in stage 1 and A R in stage 2.  One exchange layout, one padding (Geo::pad1).

// W_L^m = exp(-2 pi i m / L) for the odd legs, correctly rounded
template <int L>
ZF_HD cd wroot(int m) {
    if constexpr (L == 9) {
        constexpr double C[9] = {1.0, 0.766044443118978, 0.17364817766693036, -0.5, -0.9396926207859084,
                                 -0.9396926207859084, -0.5, 0.17364817766693036, 0.766044443118978};
        constexpr double S[9] = {0.0, -0.6427876096865394, -0.984807753012208, -0.8660254037844386, -0.3420201433256687,
                                 0.3420201433256687, 0.8660254037844386, 0.984807753012208, 0.6427876096865394};
        return mk(C[m], S[m]);
    } else if constexpr (L == 10) {
        constexpr double C[10] = {1.0, 0.8090169943749475, 0.30901699437494745, -0.30901699437494745, -0.8090169943749475,
                                  -1.0, -0.8090169943749475, -0.30901699437494745, 0.30901699437494745, 0.8090169943749475};
        constexpr double S[10] = {0.0, -0.5877852522924731, -0.9510565162951535, -0.9510565162951535, -0.5877852522924731,
                                  0.0, 0.5877852522924731, 0.9510565162951535, 0.9510565162951535, 0.5877852522924731};
        return mk(C[m], S[m]);
    } else if constexpr (L == 12) {
        constexpr double C[12] = {1.0, 0.8660254037844386, 0.5, 0.0, -0.5, -0.8660254037844386,
                                  -1.0, -0.8660254037844386, -0.5, 0.0, 0.5, 0.8660254037844386};
        constexpr double S[12] = {0.0, -0.5, -0.8660254037844386, -1.0, -0.8660254037844386, -0.5,
                                  0.0, 0.5, 0.8660254037844386, 1.0, 0.8660254037844386, 0.5};
        return mk(C[m], S[m]);
    } else {
        static_assert(L == 15, "no twiddle table for this leg");
        constexpr double C[15] = {1.0, 0.9135454576426009, 0.6691306063588582, 0.30901699437494745, -0.10452846326765347,
                                  -0.5, -0.8090169943749475, -0.9781476007338057, -0.9781476007338057, -0.8090169943749475,
                                  -0.5, -0.10452846326765347, 0.30901699437494745, 0.6691306063588582, 0.9135454576426009};
        constexpr double S[15] = {0.0, -0.4067366430758002, -0.7431448254773942, -0.9510565162951535, -0.9945218953682733,
                                  -0.8660254037844386, -0.5877852522924731, -0.20791169081775934, 0.20791169081775934,
                                  0.5877852522924731, 0.8660254037844386, 0.9945218953682733, 0.9510565162951535,
                                  0.7431448254773942, 0.4067366430758002};
        return mk(C[m], S[m]);
    }
}
// a * W_L^m (m is a compile-time value once the callers' loops are unrolled: the trivial factors cost nothing)
template <int L>
ZF_HD cd mul_w(cd a, int m) {
    m %= L;
    if (m == 0) return a;
    if (2 * m == L) return mk(-a.x, -a.y);
    if (4 * m == L) return mul_mi(a);
    if (4 * m == 3 * L) return mk(-a.y, a.x);
    return cmul(a, wroot<L>(m));
}
// forward P-point DFT in place, natural order, P = 2, 3, 4, 5
template <int P>
ZF_HD void dft_small(cd *x) {
    if constexpr (P == 2) {
        const cd t = x[0];
        x[0] = cadd(t, x[1]);
        x[1] = csub(t, x[1]);
    } else if constexpr (P == 3) {
        constexpr double H3 = 0.8660254037844386;   // sin(2 pi / 3)
        const cd t = cadd(x[1], x[2]), d = csub(x[1], x[2]);
        const cd m1 = mk(fma(-0.5, t.x, x[0].x), fma(-0.5, t.y, x[0].y));
        const cd e = mul_mi(mk(d.x * H3, d.y * H3));
        x[0] = cadd(x[0], t);
        x[1] = cadd(m1, e);
        x[2] = csub(m1, e);
    } else if constexpr (P == 4) {
        dft4(x[0], x[1], x[2], x[3]);
    } else {
        static_assert(P == 5, "no butterfly of this radix");
        constexpr double C1_5 = 0.30901699437494745, C2_5 = -0.8090169943749475;   // cos(2 pi / 5), cos(4 pi / 5)
        constexpr double S1_5 = 0.9510565162951535, S2_5 = 0.5877852522924731;     // sin(2 pi / 5), sin(4 pi / 5)
        const cd t1 = cadd(x[1], x[4]), t2 = cadd(x[2], x[3]), t3 = csub(x[1], x[4]), t4 = csub(x[2], x[3]);
        const cd m1 = mk(fma(C1_5, t1.x, fma(C2_5, t2.x, x[0].x)), fma(C1_5, t1.y, fma(C2_5, t2.y, x[0].y)));
        const cd m2 = mk(fma(C2_5, t1.x, fma(C1_5, t2.x, x[0].x)), fma(C2_5, t1.y, fma(C1_5, t2.y, x[0].y)));
        const cd n1 = mul_mi(mk(fma(S1_5, t3.x, S2_5 * t4.x), fma(S1_5, t3.y, S2_5 * t4.y)));
        const cd n2 = mul_mi(mk(fma(S2_5, t3.x, -(S1_5 * t4.x)), fma(S2_5, t3.y, -(S1_5 * t4.y))));
        x[0] = cadd(x[0], cadd(t1, t2));
        x[1] = cadd(m1, n1);
        x[4] = csub(m1, n1);
        x[2] = cadd(m2, n2);
        x[3] = csub(m2, n2);
    }
}
// forward (P Q)-point DFT in place, natural order in and out: n = Q n_p + n_q, k = k_p + P k_q
template <int P, int Q>
ZF_HD void dft_ct(cd *v) {
    cd y[P * Q];
#pragma unroll
    for (int nq = 0; nq < Q; ++nq) {
        cd x[P];
#pragma unroll
        for (int np = 0; np < P; ++np) x[np] = v[np * Q + nq];
        dft_small<P>(x);
#pragma unroll
        for (int kp = 0; kp < P; ++kp) y[kp * Q + nq] = mul_w<P * Q>(x[kp], nq * kp);
    }
#pragma unroll
    for (int kp = 0; kp < P; ++kp) {
        cd x[Q];
#pragma unroll
        for (int nq = 0; nq < Q; ++nq) x[nq] = y[kp * Q + nq];
        dft_small<Q>(x);
#pragma unroll
        for (int kq = 0; kq < Q; ++kq) v[kp + P * kq] = x[kq];
    }
}
// one leg: forward L-point DFT in place, natural order in and out
template <int L>
ZF_HD void dft_leg(cd *v) {
    if constexpr (L == 16) {
        dft16(v);
        cd t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = v[bin16(k)];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = t[k];
    } else if constexpr (L == 9) {
        dft_ct<3, 3>(v);
    } else if constexpr (L == 10) {
        dft_ct<5, 2>(v);
    } else if constexpr (L == 12) {
        dft_ct<4, 3>(v);
    } else {
        static_assert(L == 15, "no leg of this size");
        dft_ct<5, 3>(v);
    }
}

// Geometry: Geo with R3 = R (N_eff = A B R), pad1 = the padding of the one exchange layout, jstep = s in {1, 2}
// (the lattice of the aperture, or the twice finer one); pad2 and ip are not used.
template <int A, int B>
ZF_HD int mx_threads(const Geo &g) { return (A > B ? A : B) * g.R3; }
// exchange element (t, k2), t = n0 + R n1 < B R; after stage 2 the same slot holds (n0, k1 = n1's place, k2)
template <int A, int B>
ZF_HD int mx_addr(const Geo &g, int t, int k2) { return t + (B * g.R3 + g.pad1) * k2; }
template <int A, int B>
ZF_HD int mx_lds_elems(const Geo &g) { return (B * g.R3 + g.pad1) * A; }
// wanted bin of output j, reduced to [0, N_eff)
template <int A, int B>
ZF_HD int mx_bin_of(const Geo &g, int j) {
    const int N = A * B * g.R3;
    long long k = ((long long)(j + g.j0) * g.jstep) % N;
    return (int)(k < 0 ? k + N : k);
}
// stage 1 on the A samples v[n2] of thread t < B R; tw: the [k2][n1] table of W_AB^(n1 k2)
template <int A, int B>
ZF_HD void mx_stage1(const Geo &g, int t, cd *v, const cd *tw, cd *lds) {
    const int n1 = t / g.R3;
    dft_leg<A>(v);
    lds[mx_addr<A, B>(g, t, 0)] = v[0];
#pragma unroll
    for (int k2 = 1; k2 < A; ++k2) lds[mx_addr<A, B>(g, t, k2)] = cmul(v[k2], tw[k2 * B + n1]);
}
// stage 2 for thread u = n0 + R k2 < A R: a thread overwrites only the B slots it has just read (no barrier between)
template <int A, int B>
ZF_HD void mx_stage2(const Geo &g, int u, cd *v, cd *lds) {
    const int k2 = u / g.R3, n0 = u - k2 * g.R3;
#pragma unroll
    for (int n1 = 0; n1 < B; ++n1) v[n1] = lds[mx_addr<A, B>(g, n0 + g.R3 * n1, k2)];
    dft_leg<B>(v);
#pragma unroll
    for (int k1 = 0; k1 < B; ++k1) lds[mx_addr<A, B>(g, n0 + g.R3 * k1, k2)] = v[k1];
}
// stage 3 for ONE wanted bin k: Horner over its R consecutive residues with ratio w = W_N^k
template <int A, int B>
ZF_HD cd mx_stage3(const Geo &g, int k, cd w, const cd *lds) {
    const cd *b = lds + mx_addr<A, B>(g, g.R3 * ((k / A) % B), k % A);
    cd x = b[g.R3 - 1];
    for (int n0 = g.R3 - 2; n0 >= 0; --n0) x = cmac(x, w, b[n0]);
    return x;
}

// The (A, B) pairs that exist as kernels, and the factorisation of one axis: N s = A B R with s in {1, 2} and
// R <= 32, the one with the least estimated work - waves x (3 LDS accesses per sample of both legs + the Horner steps
// of a thread's share of the M wanted bins) - or s = 0: none (the caller keeps the 256 R3 scheme or the GEMMs).
// With these pairs 81 of the 97 lattices 2^a 3^b 5^c in [256, 8192] that are not multiples of 256 have one.  The 16
// without - no pair divides N or 2 N <= 8192 and leaves 32 residues or fewer: 384 (2^7 3) and 625 (5^4), which no
// pair divides at all, and 3125, 3645, 4374, 4860, 5000, 5184, 5832, 6250, 6561, 7290, 7500, 7776, 8000, 8100, whose
// powers of 2, 3 or 5 are too large for two legs (tests/test_zfft_mixed_emul.py pins the list).
#define ZF_MX_PAIRS(X) X(16, 15) X(15, 15) X(16, 10) X(15, 10) X(10, 10) X(12, 9) X(9, 9) X(16, 9)
struct MixChoice {
    int s = 0, A = 0, B = 0, R = 0;
};
ZF_HD MixChoice mixed_choose(int N, int M) {
    MixChoice best;
    long long best_cost = -1;
#define ZF_MX_TRY(AA, BB)                                                                              \
    for (int s = 1; s <= 2; ++s) {                                                                     \
        const long long Ne = (long long)N * s;                                                         \
        if (N < 1 || Ne > 8192 || Ne % (AA * BB)) continue;                                            \
        const int R = (int)(Ne / (AA * BB)), NT = (AA > BB ? AA : BB) * R;                             \
        if (R < 1 || R > 32) continue;                                                                 \
        const long long waves = (NT + 63) / 64, cost = waves * (3 * (AA + BB) + (long long)((M + NT - 1) / NT) * R); \
        if (best_cost < 0 || cost < best_cost) {                                                       \
            best_cost = cost;                                                                          \
            best.s = s, best.A = AA, best.B = BB, best.R = R;                                          \
        }                                                                                              \
    }
    ZF_MX_PAIRS(ZF_MX_TRY)
#undef ZF_MX_TRY
    return best;
}

// ---- whole aperture rows in one resident run (zfft_rows.hip zfft_rows_kernel) --------------------------------------
// The row pass of the default route reads rows that lie contiguous and whole: sample n of the transform is element n
// of the row, and it is resident where first <= n < n_valid - first (zfft.hip load_row with sub_s = 1, sub_i = 0,
// in_es = 1, one run from sample 0: its predicate min(n, n_valid - 1 - n) >= first).  The run's two ends are scalars
// of the row, and a sample's residency one compare against them.
// the resident run [lo, hi) of a row; a row with nothing resident (first past the half row, up to 0x7f7f7f7f for a row
// outside the lens) gets the empty run [0, 0)
ZF_HD void row_run(int first, int n_valid, int &lo, int &hi) {
    lo = first, hi = n_valid - first;
    if (hi <= lo) lo = hi = 0;
}
// is sample n in [lo, hi)?  One unsigned compare (lo <= hi)
ZF_HD bool piece_lane(int n, int lo, int hi) { return (unsigned)(n - lo) < (unsigned)(hi - lo); }

// The rows of a launch are dealt in 8 chunks, one per XCD (zfft.hip row_of_turn): workgroup b of a grid of G
// (a multiple of 8) takes rows xcd chunk + idx, idx = b / 8, b / 8 + G / 8, ... below the chunk's end.
ZF_HD int rows_begin(int block, int chunk) { return (block & 7) * chunk + (block >> 3); }
ZF_HD int rows_end(int block, int chunk, int rows) {
    const int e = ((block & 7) + 1) * chunk;
    return e < rows ? e : rows;
}
// row = q d + r followed along a workgroup's rows, which advance by the constant step G / 8: no division per row
struct RowWalk {
    int q, r, d, dq, dr;
};
ZF_HD RowWalk walk_init(int row, int d, int step) {
    RowWalk w;
    w.q = row / d, w.r = row % d, w.d = d, w.dq = step / d, w.dr = step % d;
    return w;
}
ZF_HD void walk_step(RowWalk &w) {
    w.q += w.dq;
    w.r += w.dr;
    if (w.r >= w.d) w.r -= w.d, ++w.q;
}

// What a call must look like for zfft_rows_kernel (zfft.hip zfft_run asks; everything else keeps zfft_kernel)
struct RowsFacts {
    bool family_one = false, ip = false;   // zfft_launch_rule's answer
    int PASS = 0, R3 = 0, M = 0;
    int sub_s = 1, sub_i = 0, a0 = 0, h0 = 0, a1 = 0, h1 = 0, n_valid = 0, accumulate = 0;
    long long in_es = 1;
    long long out_last = 0;   // element offset of the last bin in its row (the stores take 32-bit byte offsets)
};
ZF_HD bool rows_kernel_takes(const RowsFacts &f) {
    if (!f.family_one || !f.ip || (f.PASS != 1 && f.PASS != 4) || (f.R3 != 8 && f.R3 != 16)) return false;
    // every thread owns two bins, NT apart.  With 256 threads they are a pair (equal mod 256: stage3_pair_ip, as
    // zfft_kernel takes them); with 128 they are not and each is summed on its own, again as zfft_kernel does
    if (f.M != 2 * 16 * f.R3) return false;
    if (f.sub_s != 1 || f.sub_i != 0 || f.in_es != 1) return false;
    if (f.h1 != 0 || f.a0 != 0 || f.h0 < f.n_valid || f.n_valid < 0 || f.n_valid > 256 * f.R3) return false;
    if (f.accumulate) return false;
    return f.out_last >= 0 && f.out_last < (1LL << 27);   // x 16 bytes < 2^31
}

}  // namespace zf

// ---- host side: LDS bank-conflict model and the choice of the two paddings ---------------------
// MI355X_MICROARCH.md (LDS): a wave's 16-byte accesses are served in fixed lane groups, one LDS
// cycle per group when conflict-free; ds_read_b128: four non-contiguous groups of 16 lanes over 16
// slots of 16 bytes; ds_write_b128: eight contiguous groups of 8 lanes over 8 slots.  Lanes of a
// group that hit one slot at DIFFERENT addresses cost one extra cycle each.
namespace zf {

// LDS cycles of one wave-wide 16-byte access; addr[lane] in elements, < 0 = lane inactive
inline int lds_cycles(const int *addr, bool is_read) {
    static const int rd_groups[4][16] = {
        {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
        {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
        {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
        {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    int total = 0;
    const int n_groups = is_read ? 4 : 8, per = is_read ? 16 : 8, slots = is_read ? 16 : 8;
    for (int gidx = 0; gidx < n_groups; ++gidx) {
        int worst = 1;
        for (int s = 0; s < slots; ++s) {
            int seen[16], n_seen = 0;
            for (int q = 0; q < per; ++q) {
                const int lane = is_read ? rd_groups[gidx][q] : gidx * 8 + q;
                const int a = addr[lane];
                if (a < 0 || a % slots != s) continue;
                bool dup = false;
                for (int z = 0; z < n_seen; ++z) dup |= (seen[z] == a);
                if (!dup) seen[n_seen++] = a;
            }
            if (n_seen > worst) worst = n_seen;
        }
        total += worst;
    }
    return total;
}

// total LDS cycles of the four access patterns of one transform (all waves, all 16 steps) and what
// they would be without conflicts
struct LdsCost {
    long ex1_write = 0, ex1_read = 0, ex2_write = 0, ex2_read = 0, ideal_rw = 0;
};
inline LdsCost lds_cost(const Geo &g) {
    LdsCost c;
    const int NT = 16 * g.R3;
    int addr[64];
    for (int w0 = 0; w0 < NT; w0 += 64) {
        for (int s = 0; s < 16; ++s) {
            for (int l = 0; l < 64; ++l) addr[l] = w0 + l < NT ? ex1_addr(g, w0 + l, s) : -1;
            c.ex1_write += lds_cycles(addr, false);
            for (int l = 0; l < 64; ++l) {
                const int u = w0 + l;
                addr[l] = u < NT ? ex1_addr(g, u % g.R3 + g.R3 * s, u / g.R3) : -1;
            }
            c.ex1_read += lds_cycles(addr, true);
            for (int l = 0; l < 64; ++l) {
                const int u = w0 + l;
                addr[l] = u >= NT ? -1 : g.ip ? ex2ip_addr(g, u % g.R3, s, u / g.R3) : ex2_addr(g, u % g.R3, s, u / g.R3);
            }
            c.ex2_write += lds_cycles(addr, false);
            c.ideal_rw += 4 + 8;
        }
    }
    for (int o0 = 0; o0 < g.M; o0 += 64)
        for (int n0 = 0; n0 < g.R3; ++n0) {
            for (int l = 0; l < 64; ++l) {
                if (o0 + l >= g.M) {
                    addr[l] = -1;
                    continue;
                }
                const int k = bin_of(g, o0 + l);
                addr[l] = g.ip ? ex2ip_addr(g, n0, (k >> 4) & 15, k & 15) : ex2_addr(g, n0, (k >> 4) & 15, k & 15);
            }
            c.ex2_read += lds_cycles(addr, true);
        }
    return c;
}

// paddings with the fewest conflict cycles (exchange 1 is read strided, exchange 2 written
// strided).  The two exchanges do not interact, so each padding is searched on its own.
inline void choose_pads(Geo &g) {
    long best = -1;
    int b1 = 0, b2 = 0;
    for (int p1 = 0; p1 <= 16; ++p1) {   // smaller paddings win ties (LDS footprint)
        Geo t = g;
        t.pad1 = p1;
        t.pad2 = 0;
        const LdsCost c = lds_cost(t);
        // (in place, all four patterns live in exchange 1's layout and answer to pad1)
        const long cost = (c.ex1_write + c.ex1_read + (g.ip ? c.ex2_write + c.ex2_read : 0)) * 64 + p1;
        if (best < 0 || cost < best) {
            best = cost;
            b1 = p1;
        }
    }
    best = -1;
    for (int p2 = 0; p2 <= 16; ++p2) {
        Geo t = g;
        t.pad1 = b1;
        t.pad2 = p2;
        const LdsCost c = lds_cost(t);
        const long cost = (c.ex2_write + c.ex2_read) * 64 + p2;
        if (best < 0 || cost < best) {
            best = cost;
            b2 = p2;
        }
    }
    g.pad1 = b1;
    g.pad2 = b2;
}

// LDS cycles of the mixed-radix transform's four access patterns (all waves, all steps) and the conflict-free count
struct MixCost {
    long s1_write = 0, s2_read = 0, s2_write = 0, horner = 0, ideal = 0;
    long total() const { return s1_write + s2_read + s2_write + horner; }
};
template <int A, int B>
inline MixCost mixed_cost(const Geo &g) {
    MixCost c;
    const int R = g.R3, NT = mx_threads<A, B>(g);
    int addr[64];
    for (int w0 = 0; w0 < NT; w0 += 64) {
        for (int k2 = 0; k2 < A; ++k2) {
            bool any = false;
            for (int l = 0; l < 64; ++l) any |= (addr[l] = w0 + l < B * R ? mx_addr<A, B>(g, w0 + l, k2) : -1) >= 0;
            if (any) c.s1_write += lds_cycles(addr, false), c.ideal += 8;
        }
        for (int n1 = 0; n1 < B; ++n1) {
            bool any = false;
            for (int l = 0; l < 64; ++l) {
                const int u = w0 + l;
                any |= (addr[l] = u < A * R ? mx_addr<A, B>(g, u % R + R * n1, u / R) : -1) >= 0;
            }
            if (any) c.s2_read += lds_cycles(addr, true), c.s2_write += lds_cycles(addr, false), c.ideal += 4 + 8;
        }
    }
    for (int o0 = 0; o0 < g.M; o0 += 64)
        for (int n0 = 0; n0 < R; ++n0) {
            for (int l = 0; l < 64; ++l) {
                const int k = o0 + l < g.M ? mx_bin_of<A, B>(g, o0 + l) : -1;
                addr[l] = k < 0 ? -1 : mx_addr<A, B>(g, n0 + R * ((k / A) % B), k % A);
            }
            c.horner += lds_cycles(addr, true);
            c.ideal += 4;
        }
    return c;
}
// the padding with the fewest conflict cycles (smaller paddings win ties)
template <int A, int B>
inline void mixed_choose_pad(Geo &g) {
    long best = -1;
    int bp = 0;
    for (int p = 0; p <= 16; ++p) {
        g.pad1 = p;
        const long cost = mixed_cost<A, B>(g).total();
        if (best < 0 || cost < best) best = cost, bp = p;
    }
    g.pad1 = bp;
}

// LDS cycles of the tile column pass for one round (TL_SLOTS residues) of one workgroup, and the conflict-free
// count: phase A writes, phase B reads and in-place writes, and the Horner reads of bins j0 .. j0 + M
struct TileCost {
    long a_write = 0, b_read = 0, b_write = 0, horner = 0, ideal = 0;
};
inline TileCost tile_cost(int M, int j0) {
    TileCost c;
    int addr[64];
    for (int w0 = 0; w0 < TL_NT; w0 += 64) {
        for (int q = 0; q < 16; ++q) {
            for (int l = 0; l < 64; ++l) addr[l] = tl_addr(tl_slot(w0 + l), tl_col(w0 + l), q, tl_sub(w0 + l));
            c.a_write += lds_cycles(addr, false);
            for (int l = 0; l < 64; ++l) addr[l] = tl_addr(tl_slot(w0 + l), tl_col(w0 + l), tl_sub(w0 + l), q);
            c.b_read += lds_cycles(addr, true);
            c.b_write += lds_cycles(addr, false);
            c.ideal += 8 + 4 + 8;
        }
    }
    for (int o0 = 0; o0 < M; o0 += 64)
        for (int s = 0; s < TL_SLOTS; ++s)
            for (int col = 0; col < 8; ++col) {
                for (int l = 0; l < 64; ++l) {
                    const int k = ((o0 + l + j0) % 256 + 256) % 256;
                    addr[l] = o0 + l < M ? tl_addr(s, col, k & 15, k >> 4) : -1;
                }
                c.horner += lds_cycles(addr, true);
                c.ideal += 4;
            }
    return c;
}

}  // namespace zf
