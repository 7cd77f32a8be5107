// The arithmetic of ONE (aperture sample, target) pair of the direct Stratton-Chu sum, shared by the kernels that form it:
// propagate_kernel (propagate.hip: a lane is a target, the pairs' terms are added over the samples) and zf_line_kernel
// (fields_zone_fields.hip: a lane is a sample, the terms are added zone by zone).  Both call the same inlined functions in
// the same order, nothing is contracted and only the explicit fma() are fused: a pair's term has the same bits in both.
//
// With R = r - r', q = 1 / (k R), w = e^{i k R} / (k R), a = 1 + i q - q^2, b = 1 + 3 i q - 3 q^2, m = M / Z and
// D(V) = a V - b Rhat (Rhat . V) a pair adds  w { i D(J) - (i - q) Rhat x m }  to E and  w { i D(m) + (i - q) Rhat x J }  to H;
// the scales Z k^2 / (4 pi) dx' dy' and k^2 / (4 pi) dx' dy' belong to the finished sums.  Include after nearfield_math.h.
#pragma once

namespace ml {

// a target's coordinate against sample i of an axis: hi and lo are the two doubles of x - x0 (propagate_direct.h
// prop_two_diff); the low part is added behind the fma
__device__ __forceinline__ double pair_offset(int i, double pitch, double hi, double lo) { return fma(-(double)i, pitch, hi) + lo; }

// a field component as the current it stands for: Ex -> My / Z = -Ex / Z, Ey -> Mx / Z, Hx -> Jy, Hy -> Jx = -Hy
// (sg = -1 for Ex and Hy, den = Z for Ex and Ey; a division: exact for Z = 1, and x 2 commutes)
__device__ __forceinline__ double2 pair_current(double sg, double den, double2 v) { return make_double2(sg * v.x / den, sg * v.y / den); }

// what depends on the pair alone and serves every field set: Rhat, q, w, a, b
struct PairGeom {
    double ux, uy, uz, q;
    c2 w, a, b;
};

// s_row = dx dx + z z of the row
__device__ __forceinline__ PairGeom pair_geom(double dx, double dy, double z, double s_row, double k, double inv_k) {
    PairGeom g;
    const double R = sqrt_exact(fma(dy, dy, s_row));
    const double iR = recip(R);
    g.ux = dx * iR;
    g.uy = dy * iR;
    g.uz = z * iR;
    g.q = iR * inv_k;
    const double q2 = g.q * g.q;
    double sn, cs;
    sincos_cw(k * R, sn, cs);
    g.w = c2{cs * g.q, sn * g.q};
    g.a = c2{1.0 - q2, g.q};
    g.b = c2{fma(-3.0, q2, 1.0), 3.0 * g.q};
    return g;
}

// acc += w t
__device__ __forceinline__ void cfma(c2 &acc, c2 w, double tr, double ti) {
    acc.r = fma(-w.i, ti, fma(w.r, tr, acc.r));
    acc.i = fma(w.i, tr, fma(w.r, ti, acc.i));
}

// acc[0..3) += w { i D(V) + sgn (i - q) Rhat x U },  D(V) = a V - b Rhat (Rhat . V);  V, U tangential
template <int SGN>
__device__ __forceinline__ void pair_term(c2 acc[3], c2 w, double q, c2 a, c2 b, double ux, double uy, double uz, c2 Vx,
                                          c2 Vy, c2 Ux, c2 Uy) {
    const c2 dot = {fma(ux, Vx.r, uy * Vy.r), fma(ux, Vx.i, uy * Vy.i)};
    const c2 bd = cmulf(b, dot);
    const c2 Dx = {fma(-ux, bd.r, fma(a.r, Vx.r, -(a.i * Vx.i))), fma(-ux, bd.i, fma(a.r, Vx.i, a.i * Vx.r))};
    const c2 Dy = {fma(-uy, bd.r, fma(a.r, Vy.r, -(a.i * Vy.i))), fma(-uy, bd.i, fma(a.r, Vy.i, a.i * Vy.r))};
    const c2 Dz = {-uz * bd.r, -uz * bd.i};
    const c2 Xx = {-uz * Uy.r, -uz * Uy.i};
    const c2 Xy = {uz * Ux.r, uz * Ux.i};
    const c2 Xz = {fma(ux, Uy.r, -(uy * Ux.r)), fma(ux, Uy.i, -(uy * Ux.i))};
    // i D = (-D.i, D.r);  (i - q) X = (-q X.r - X.i, X.r - q X.i)
    const double s = (double)SGN;
    cfma(acc[0], w, fma(s, fma(-q, Xx.r, -Xx.i), -Dx.i), fma(s, fma(-q, Xx.i, Xx.r), Dx.r));
    cfma(acc[1], w, fma(s, fma(-q, Xy.r, -Xy.i), -Dy.i), fma(s, fma(-q, Xy.i, Xy.r), Dy.r));
    cfma(acc[2], w, fma(s, fma(-q, Xz.r, -Xz.i), -Dz.i), fma(s, fma(-q, Xz.i, Xz.r), Dz.r));
}

}  // namespace ml
