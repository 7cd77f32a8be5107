// The row transform of the default route as a kernel of its own: zfft_kernel's per-thread programme (zfft_core.h,
// the in-place form) on rows that lie whole and contiguous in one resident run - what stage 1 of a far-field
// transform reads (farfield.hip stage1_fft) - without the address and residency arithmetic the general kernel does
// per lane and per load:
//   - one row base per turn; each of the 16 loads takes that base, advanced by NT 16 bytes per n2 in scalar
//     registers, and one 32-bit lane offset that never changes (no 64-bit address arithmetic per lane);
//   - the resident samples of a row are one run [first, n_valid - first) whose ends are scalars of the row
//     (zfft_core.h row_run): one unsigned compare per load (piece_lane), and a wave whose 64 samples all lie outside
//     the run skips the load; row_first[row] arrives by a scalar load issued one turn ahead;
//   - the turn loop is unrolled by two and the two register sets swap roles (no copy of the prefetched row);
//   - row / in_rb, row % in_rb, row % rf_mod, row / out_rb and row / alpha_rb follow the row counter, which advances
//     by a constant step (zfft_core.h RowWalk);
//   - the two stores take a scalar row base and 32-bit lane offsets.
// The arithmetic, its order and the store offsets are zfft_kernel's: the result is bit-identical
// (tests/test_gpu_fft_rows.py).  zfft.hip zfft_run decides which of the two a call takes.
#include <type_traits>

#include "zfft_rows.h"
#include "zfft_core.h"

namespace ml {

using zf::cd;

struct RowsArgs {
    int n_valid, pad1;
    const cd *in;              // row r starts at in + (r / in_rb) * in_s1 + (r % in_rb) * in_s2
    int64_t in_s1, in_s2;
    int in_rb;
    const int *row_first;      // sample n of row r is read where first <= n < n_valid - first, first =
    int rf_mod;                // row_first[r % rf_mod] (nullptr: 0)
    cd *out;                   // bin j of row r at out + (r / out_rb) * out_s1 + (r % out_rb) * out_s2 + its offset:
    int64_t out_s1, out_s2, out_es;   // j * out_es, or (TILED) zf::tile_off(j, out_es)
    int out_rb;
    const cd *tw1, *wk, *pj;
    const int *kbin;
    double alpha[4];           // row r is scaled by alpha[r / alpha_rb]
    int alpha_rb;
    int rows, chunk;
};

typedef double double2v __attribute__((ext_vector_type(2)));

// A 32-bit lane offset as a value born where it is used: its widening to 64 bits then happens beside the access, which
// takes "scalar base + 32-bit lane offset" as its address form (widened once at the kernel's top, every access adds a
// 64-bit lane offset to its base in vector registers)
__device__ __forceinline__ uint32_t here(uint32_t off) {
    asm volatile("" : "+v"(off));
    return off;
}

// one row's 16 samples of thread `tid` from the row at `src` (block-uniform) with the resident run [lo, hi)
// (zfft_core.h row_run): sample n = tid + NT n2 is loaded where lo <= n < hi and reads as zero elsewhere - the zero /
// non-zero pattern of load_row (zfft.hip).  One compare per load decides it (zfft_core.h piece_lane, on rel = tid - lo
// and span = hi - lo); a wave none of whose lanes passes skips the load.
// pitch: NT 16, the bytes between a thread's loads, as a value the compiler cannot fold - the base then advances in
// scalar registers and each load takes it beside the 32-bit lane offset (folded, the compiler adds the lane offset to
// the row base once and every load pays a 64-bit add per lane for its constant)
template <int NT>
__device__ __forceinline__ void rows_load(const cd *src, int lo, int hi, int tid, uint32_t lane_off, int pitch, cd *v) {
    const char *base = reinterpret_cast<const char *>(src);
    const int rel = tid - lo;
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) {
        double2v t = {0.0, 0.0};
        if (zf::piece_lane(rel + NT * n2, 0, hi - lo))
            t = __builtin_nontemporal_load(reinterpret_cast<const double2v *>(base + here(lane_off)));
        v[n2] = zf::mk(t.x, t.y);
        base += pitch;
    }
}

// R3T residues: 16 R3T threads, two workgroups per CU as zfft_kernel<R3T, 16 R3T, 2, ., true>.  M = 32 R3T bins:
// thread t evaluates bins t and t + NT.  TILED: the store of PASS 4 (zfft_core.h tile_off), else bins out_es apart.
template <int R3T, bool TILED>
__global__ __launch_bounds__(16 * R3T, 2) void zfft_rows_kernel(const RowsArgs a) {
    extern __shared__ __align__(16) unsigned char zfft_rows_lds_raw[];
    cd *lds = reinterpret_cast<cd *>(zfft_rows_lds_raw);
    constexpr int NT = 16 * R3T;
    const int tid = threadIdx.x;
    const int step = gridDim.x >> 3, row_end = zf::rows_end(blockIdx.x, a.chunk, a.rows);
    int row = zf::rows_begin(blockIdx.x, a.chunk);   // block-uniform
    if (row >= row_end) return;                      // (no turn at all: more workgroups than rows)
    zf::Geo g;
    g.R3 = R3T, g.n_valid = a.n_valid, g.M = 2 * NT, g.j0 = 0, g.pad1 = a.pad1, g.pad2 = 0, g.ip = 1;
    cd *s_tw = lds + zf::lds_elems(g);   // [16][16] behind the exchange buffer
    for (int e = tid; e < 256; e += NT) s_tw[(e & 15) * 16 + (e >> 4)] = a.tw1[e];   // e = n1 * 16 + k2
    const int n1 = tid / R3T;
    cd tb[4];
    tb[0] = zf::mk(1.0, 0.0);
#pragma unroll
    for (int b = 1; b < 4; ++b) tb[b] = a.tw1[n1 * 16 + b];
    const int bin0 = tid, bin1 = tid + NT;
    const cd w0 = a.wk[bin0], p0 = a.pj[bin0], w1 = a.wk[bin1], p1 = a.pj[bin1];
    const int k0 = a.kbin[bin0], k1 = a.kbin[bin1];
    // byte offsets of the two bins in their row (zfft_run has checked that they fit 32 bits)
    const uint32_t off0 = (uint32_t)((TILED ? zf::tile_off(bin0, a.out_es) : (long long)bin0 * a.out_es) * 16);
    const uint32_t off1 = (uint32_t)((TILED ? zf::tile_off(bin1, a.out_es) : (long long)bin1 * a.out_es) * 16);
    const uint32_t lane_off = (uint32_t)tid * 16;
    int pitch = NT * 16;
    asm volatile("" : "+s"(pitch));   // (rows_load)
    __syncthreads();

    // the row being loaded (wi), the row whose row_first is being fetched (wf: one turn further), the row being
    // transformed (wo, wa)
    zf::RowWalk wi = zf::walk_init(row, a.in_rb, step), wf = zf::walk_init(row, a.rf_mod, step);
    zf::RowWalk wo = zf::walk_init(row, a.out_rb, step), wa = zf::walk_init(row, a.alpha_rb, step);
    // (row_first was written by an earlier kernel: read through the constant address space, a scalar load)
    typedef const int __attribute__((address_space(4))) * const_int_ptr;
    const const_int_ptr rf = (const_int_ptr)(uintptr_t)a.row_first;
    cd va[16], vb[16];
    int lo, hi;
    zf::row_run(rf ? rf[wf.r] : 0, a.n_valid, lo, hi);
    rows_load<NT>(a.in + wi.q * a.in_s1 + wi.r * a.in_s2, lo, hi, tid, lane_off, pitch, va);
    zf::walk_step(wi);
    zf::walk_step(wf);
    int row_n = row + step;
    int first_n = rf && row_n < row_end ? rf[wf.r] : 0;

    // one turn: v holds the samples of `row`; the next row's loads go to nx before this row's arithmetic.
    // Returns whether nx holds a row.
    auto turn = [&](auto first_turn, cd *v, cd *nx) __attribute__((always_inline)) -> bool {
        const bool more = row_n < row_end;
        // v's loads have had the last turn to arrive: wait for them here, before the next row's loads are issued,
        // and not where stage 1 first reads v - some of the 16 loads behind them are skipped, how many only the run
        // time knows, so a wait placed there has to be for all of them and the prefetch would overlap nothing.
        // The last turn's two stores were issued after v's loads and may stay in flight (vmcnt(2)); the first turn
        // has none before it, hence its own copy of the turn
        if (decltype(first_turn)::value)
            __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
        else
            __builtin_amdgcn_s_waitcnt(0x0f72);   // vmcnt(2)
        if (more) {
            zf::row_run(first_n, a.n_valid, lo, hi);
            rows_load<NT>(a.in + wi.q * a.in_s1 + wi.r * a.in_s2, lo, hi, tid, lane_off, pitch, nx);
            zf::walk_step(wi);
            // row_first of the row after, for the next turn (fetched after this turn's use of first_n: scalar loads
            // return out of order, a wait for first_n would be a wait for this one too)
            zf::walk_step(wf);
            first_n = rf && row_n + step < row_end ? rf[wf.r] : 0;
        }
        {
            cd ta[4];
            ta[0] = tb[0];
#pragma unroll
            for (int q = 1; q < 4; ++q) ta[q] = s_tw[(4 * q) * 16 + n1];
            zf::stage1_regs(g, tid, v, ta, tb, lds);
        }
        __syncthreads();
        zf::gather2(g, tid, v, lds);
        zf::scatter2_ip(g, tid, v, lds);   // (a thread overwrites only the slots it has just read)
        __syncthreads();
        char *dst = reinterpret_cast<char *>(a.out + wo.q * a.out_s1 + wo.r * a.out_s2);
        const double al = a.alpha[wa.q];
        cd xa, xb;
        if (NT % 256 == 0) {   // the two bins share their LDS operands
            zf::stage3_pair_ip(g, k0, w0, w1, lds, xa, xb);
        } else {
            xa = zf::stage3_ip(g, k0, w0, lds);
            xb = zf::stage3_ip(g, k1, w1, lds);
        }
        xa = zf::cmul(xa, p0);
        xb = zf::cmul(xb, p1);
        xa.x *= al;
        xa.y *= al;
        xb.x *= al;
        xb.y *= al;
        *reinterpret_cast<cd *>(dst + here(off0)) = xa;
        *reinterpret_cast<cd *>(dst + here(off1)) = xb;
        __syncthreads();   // the next row's stage 1 overwrites the buffer
        zf::walk_step(wo);
        zf::walk_step(wa);
        row = row_n;
        row_n += step;
        return more;
    };
    if (turn(std::true_type(), va, vb))
        for (;;) {
            if (!turn(std::false_type(), vb, va)) break;
            if (!turn(std::false_type(), va, vb)) break;
        }
}

template <int R3T, bool TILED>
static int launch_rows(hipStream_t stream, const RowsArgs &a, int grid, size_t lds_bytes) {
    auto kern = zfft_rows_kernel<R3T, TILED>;
    static bool attr_done = false;   // per instantiation
    if (!attr_done) {
        ML_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024));
        attr_done = true;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(16 * R3T), lds_bytes, stream, a);
    ML_HIP(hipGetLastError());
    return ML_OK;
}

int zfft_rows_run(hipStream_t stream, const ZfftCall &c, int pad1, int grid, size_t lds_bytes) {
    const int R3 = c.N_eff / 256;
    ML_REQUIRE((R3 == 8 || R3 == 16) && c.M == 32 * R3 && grid > 0 && grid % 8 == 0 && c.in_rb > 0 && c.out_rb > 0 &&
                   c.alpha_rb > 0 && c.rows <= 4 * (int64_t)c.alpha_rb,
               "fixed-shape row transform: %d samples, %d bins, %d rows", c.N_eff, c.M, c.rows);
    RowsArgs a;
    a.n_valid = c.n_valid;
    a.pad1 = pad1;
    a.in = reinterpret_cast<const cd *>(c.in);
    a.in_s1 = c.in_s1;
    a.in_s2 = c.in_s2;
    a.in_rb = c.in_rb;
    a.row_first = c.row_first;
    a.rf_mod = c.rf_mod > 0 ? c.rf_mod : 1;
    a.out = reinterpret_cast<cd *>(c.out);
    a.out_s1 = c.out_s1;
    a.out_s2 = c.out_s2;
    a.out_es = c.out_es;
    a.out_rb = c.out_rb;
    a.tw1 = reinterpret_cast<const cd *>(c.tw1);
    a.wk = reinterpret_cast<const cd *>(c.wk);
    a.pj = reinterpret_cast<const cd *>(c.pj);
    a.kbin = c.kbin;
    for (int k = 0; k < 4; ++k) a.alpha[k] = c.alpha[k];
    a.alpha_rb = c.alpha_rb;
    a.rows = c.rows;
    a.chunk = (c.rows + 7) / 8;
    if (R3 == 16)
        return c.tiled_out ? launch_rows<16, true>(stream, a, grid, lds_bytes)
                           : launch_rows<16, false>(stream, a, grid, lds_bytes);
    return c.tiled_out ? launch_rows<8, true>(stream, a, grid, lds_bytes)
                       : launch_rows<8, false>(stream, a, grid, lds_bytes);
}

}  // namespace ml
