// The device arithmetic that every FFT form of the finite-distance propagator shares, stated once: the eight kernels of a
// lag, a field sample as a padded current, the contraction's term table, the scaled store of a target.  Functions only -
// the kernels that call them, their index arithmetic and their launches are in propagate_grid.hip, propagate_grid_tiled.hip, propagate_grid_fine.hip and propagate_stack.hip.
// The cross-method equalities of the suite (a one-tile plan and 'fft', a full lattice and 'fft-tiled', a plane of a stack
// and 'fft-fine', kept and streamed spectra) hold because both sides run these functions.
#pragma once

#include "nearfield_math.h"

namespace ml {

// The eight kernels (the table on top of propagate_grid.hip) of the integer lag (lx, ly) on the pitch (dxp, dyp) from the
// origin (tx_off, ty_off) at the height z: o[c plane_stride], c = Kxx Kxy Kyy Kzx Kzy Cx Cy Cz.  R, 1 / R, the sincos of
// k R, q, w, a, b and Rhat are the inlined functions of propagate_kernel in its order.
__device__ __forceinline__ void grid_green(int lx, int ly, double dxp, double dyp, double tx_off, double ty_off, double z, double k,
                                           double inv_k, double2 *o, size_t plane_stride) {
    const double dx = fma((double)lx, dxp, tx_off), dy = fma((double)ly, dyp, ty_off);
    const double s_row = fma(dx, dx, z * z);
    const double R = sqrt_exact(fma(dy, dy, s_row));
    const double iR = recip(R);
    const double ux = dx * iR, uy = dy * iR, uz = z * iR;
    const double q = iR * inv_k, q2 = q * q;
    double sn, cs;
    sincos_cw(k * R, sn, cs);
    const c2 w = {cs * q, sn * q};
    const c2 ca = {1.0 - q2, q}, cb = {fma(-3.0, q2, 1.0), 3.0 * q};
    const c2 wb = cmulf(w, cb);
    const c2 txx = {fma(-(ux * ux), cb.r, ca.r), fma(-(ux * ux), cb.i, ca.i)};
    const c2 tyy = {fma(-(uy * uy), cb.r, ca.r), fma(-(uy * uy), cb.i, ca.i)};
    const c2 wxx = cmulf(w, txx), wyy = cmulf(w, tyy);
    const c2 ci = {fma(-q, w.r, -w.i), fma(-q, w.i, w.r)};   // w (i - q)
    const double gxy = ux * uy, gzx = uz * ux, gzy = uz * uy;
    o[0] = make_double2(-wxx.i, wxx.r);                              // i w (a - b ux^2)
    o[plane_stride] = make_double2(wb.i * gxy, -(wb.r * gxy));       // -i w b ux uy
    o[2 * plane_stride] = make_double2(-wyy.i, wyy.r);
    o[3 * plane_stride] = make_double2(wb.i * gzx, -(wb.r * gzx));
    o[4 * plane_stride] = make_double2(wb.i * gzy, -(wb.r * gzy));
    o[5 * plane_stride] = make_double2(ci.r * ux, ci.i * ux);
    o[6 * plane_stride] = make_double2(ci.r * uy, ci.i * uy);
    o[7 * plane_stride] = make_double2(ci.r * uz, ci.i * uz);
}

// Current c of the sample (i, j) of one field set [4][nx][ny]: Jx = -Hy, Jy = Hx, Mx / Z = Ey / Z, My / Z = -Ex / Z (the
// conversion of propagate_kernel's staging: field f = 3 - c, the same signs, the same division); zero outside the aperture
// and outside the row extents of a synthesised field (row_first, or NULL)
__device__ __forceinline__ double2 grid_current(const double2 *fields, const int *row_first, int nx, int ny, int i, int j, int c,
                                                double Z) {
    double2 v = make_double2(0.0, 0.0);
    if (i < nx && j < ny) {
        const int first = row_first ? row_first[i] : 0;   // (0x7f7f7f7f: no sample of the row is inside)
        if (j >= first && j < ny - first) {
            const int f = 3 - c;
            const double sg = (f == 0 || f == 3) ? -1.0 : 1.0, den = f < 2 ? Z : 1.0;
            const double2 s = fields[((size_t)f * nx + i) * ny + j];
            v = make_double2(sg * s.x / den, sg * s.y / den);
        }
    }
    return v;
}

// acc += k v
__device__ __forceinline__ void zfma(double2 &acc, double2 k, double2 v) {
    acc.x = fma(-k.y, v.y, fma(k.x, v.x, acc.x));
    acc.y = fma(k.y, v.x, fma(k.x, v.y, acc.y));
}
__device__ __forceinline__ double2 zmul(double2 k, double2 v) {
    return make_double2(fma(k.x, v.x, -(k.y * v.y)), fma(k.x, v.y, k.y * v.x));
}
__device__ __forceinline__ double2 zneg(double2 v) { return make_double2(-v.x, -v.y); }

// e = k v (START) or e += k v
template <bool START>
__device__ __forceinline__ void zterm(double2 &e, double2 k, double2 v) {
    if (START)
        e = zmul(k, v);
    else
        zfma(e, k, v);
}

// a kernel spectrum that is read once per pass: a streaming load
__device__ __forceinline__ double2 ld_stream(const double2 *p) {
    typedef double double2v __attribute__((ext_vector_type(2)));
    const double2v t = __builtin_nontemporal_load(reinterpret_cast<const double2v *>(p));
    return make_double2(t.x, t.y);
}

// the eight kernel spectra of one bin
struct GridKernels8 {
    double2 Kxx, Kxy, Kyy, Kzx, Kzy, Cx, Cy, Cz;
};

// ... of bin id (planes ps apart) by streaming loads: the tile and the fine contraction, which read a spectrum once per
// pass.  (grid_contract_kernel reads its eight with plain loads, in its own body: through a function the compiler sets up
// their addresses with 15 to 24 more scalar instructions.)
__device__ __forceinline__ GridKernels8 grid_load_kernels(const double2 *K, size_t ps, size_t id) {
    return {ld_stream(K + id),          ld_stream(K + ps + id),     ld_stream(K + 2 * ps + id), ld_stream(K + 3 * ps + id),
            ld_stream(K + 4 * ps + id), ld_stream(K + 5 * ps + id), ld_stream(K + 6 * ps + id), ld_stream(K + 7 * ps + id)};
}

// The term table of one bin (on top of propagate_grid.hip): the 6 (3) output spectra e from the eight kernel spectra and
// the four current spectra, 20 (10) complex products in this order.  START: a sum starts from its first product; otherwise
// the products are added to what e holds.
template <bool WANT_H, bool START>
__device__ __forceinline__ void grid_products(double2 (&e)[6], const GridKernels8 &k, double2 Jx, double2 Jy, double2 mx, double2 my) {
    const double2 Kxx = k.Kxx, Kxy = k.Kxy, Kyy = k.Kyy, Kzx = k.Kzx, Kzy = k.Kzy, Cx = k.Cx, Cy = k.Cy, Cz = k.Cz;
    zterm<START>(e[0], Kxx, Jx);
    zfma(e[0], Kxy, Jy);
    zfma(e[0], Cz, my);
    zterm<START>(e[1], Kxy, Jx);
    zfma(e[1], Kyy, Jy);
    zfma(e[1], zneg(Cz), mx);
    zterm<START>(e[2], Kzx, Jx);
    zfma(e[2], Kzy, Jy);
    zfma(e[2], Cy, mx);
    zfma(e[2], zneg(Cx), my);
    if (WANT_H) {
        zterm<START>(e[3], Kxx, mx);
        zfma(e[3], Kxy, my);
        zfma(e[3], zneg(Cz), Jy);
        zterm<START>(e[4], Kxy, mx);
        zfma(e[4], Kyy, my);
        zfma(e[4], Cz, Jx);
        zterm<START>(e[5], Kzx, mx);
        zfma(e[5], Kzy, my);
        zfma(e[5], Cx, Jy);
        zfma(e[5], zneg(Cy), Jx);
    }
}

// component m of a target: v times scale_e (E, m < 3) or scale_h
__device__ __forceinline__ void grid_store_scaled(double2 *dst, double2 v, int m, double scale_e, double scale_h) {
    const double scale = m < 3 ? scale_e : scale_h;
    *dst = make_double2(scale * v.x, scale * v.y);
}

}  // namespace ml
