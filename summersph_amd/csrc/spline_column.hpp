// spline_column.hpp -- F(p): the renders' cubic spline integrated along the line of sight in closed form (include/summersph.h,
// "spectral cubes", has the formulas).  The footprint of sph_cube (cube.hip) and of sph_transfer (transfer.hip).
#pragma once
#include <cmath>

// the definition fixes the order of every sum; no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

// L(t) = p^2 ln(t + r), 0 at p == 0
// I1 = (t r + L) / 2, I2 = p^2 t + t^3 / 3, I3 = t r^3 / 4 + 3 p^2 t r / 8 + 3 p^2 L / 8
__device__ __forceinline__ void spline_ints(double p2, double t, double &I1, double &I2, double &I3) {
    const double r = sqrt(p2 + t * t);
    const double L = p2 > 0.0 ? p2 * log(t + r) : 0.0;
    I1 = 0.5 * (t * r + L);
    I2 = p2 * t + (t * t * t) / 3.0;
    I3 = (0.25 * t * (r * r * r) + 0.375 * p2 * t * r) + 0.375 * p2 * L;
}
__device__ __forceinline__ double g_in(double p2, double t) {
    double I1, I2, I3;
    spline_ints(p2, t, I1, I2, I3);
    return (t - 1.5 * I2) + 0.75 * I3;
}
__device__ __forceinline__ double g_out(double p2, double t) {
    double I1, I2, I3;
    spline_ints(p2, t, I1, I2, I3);
    return ((2.0 * t - 3.0 * I1) + 1.5 * I2) - 0.25 * I3;
}
// the cubic spline (W h^3 pi) integrated along the line of sight at impact parameter p h, in units of h: F(0) = 1.5
__device__ __forceinline__ double spline_column(double p) {
    const double p2 = p * p;
    if (!(p < 2.0)) return 0.0;
    const double t2 = sqrt(4.0 - p2);
    if (p < 1.0) {
        const double t1 = sqrt(1.0 - p2);
        return 2.0 * (((g_in(p2, t1) - g_in(p2, 0.0)) + g_out(p2, t2)) - g_out(p2, t1));
    }
    return 2.0 * (g_out(p2, t2) - g_out(p2, 0.0));
}

}  // namespace sph
