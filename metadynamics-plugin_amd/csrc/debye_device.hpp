// debye_device.hpp — the device arithmetic of debye.hip (cv.debye_structure_factor): sine and cosine of a bounded argument, and the pair
// term of one list entry.  Host-callable too, so that the arithmetic can be compiled and checked on a CPU.
#pragma once

#include "mtd_device.hpp"

#include <cmath>

namespace mtd
{

// sin(y) and cos(y) for the arguments of this unit: x = pi r / r_cut in [0, pi] and y = Q r <= Q r_cut (a few tens in any physical
// case).  Cody-Waite reduction by pi/2 in two parts with FMAs (the product n pi/2 enters unrounded: the reduced argument is good to
// ~1e-16 + n 1e-33), then the kernel polynomials of degree 13 and 14 on |r| <= pi/4 (the minimax coefficients of fdlibm's k_sin.c and
// k_cos.c, truncation below 1e-17) and the quadrant.  No table, no branch, no large-argument path: ~22 fp64 operations and a dozen
// integer and select instructions for the pair, where the library routine carries a Payne-Hanek branch with a private array.  Within
// 2.2e-16 of the host library's sine and cosine over [0, 1e6]; beyond |y| ~ 1e9 the reduction loses digits gracefully (the result stays
// in [-1, 1]); a non-finite y gives NaN.
__host__ __device__ __forceinline__ void dsf_sincos(const double y, double &sn, double &cs)
    {
    const double n = rint(y * 0.63661977236758134308);               // 2 / pi
    double r = fma(-n, 1.57079632679489655800e+00, y);               // pi/2, its double
    r = fma(-n, 6.12323399573676603587e-17, r);                      // pi/2 minus that double
    const double z = r * r;
    double s = 1.58969099521155010221e-10;
    s = fma(s, z, -2.50507602534068634195e-08);
    s = fma(s, z, 2.75573137070700676789e-06);
    s = fma(s, z, -1.98412698298579493134e-04);
    s = fma(s, z, 8.33333333332248946124e-03);
    s = fma(s, z, -1.66666666666666324348e-01);
    const double sin_r = fma(r * z, s, r);
    double c = -1.13596475577881948265e-11;
    c = fma(c, z, 2.08757232129817482790e-09);
    c = fma(c, z, -2.75573143513906633035e-07);
    c = fma(c, z, 2.48015872894767294178e-05);
    c = fma(c, z, -1.38888888888741095749e-03);
    c = fma(c, z, 4.16666666666666019037e-02);
    const double cos_r = fma(z * z, c, fma(-0.5, z, 1.0));
    const long long k = (long long)n;
    const bool swap = (k & 1) != 0;
    const double a = swap ? cos_r : sin_r, b = swap ? sin_r : cos_r;
    sn = (k & 2) ? -a : a;
    cs = ((k + 1) & 2) ? -b : b;
    }

// the window of one entry at distance r = 1 / inv_r > 0: w = sin x / x and cos x, x = pi r / r_cut
__host__ __device__ __forceinline__ void dsf_window(const double r, const double inv_r, const double pi_over_rc, const double rc_over_pi, double &w,
                                                    double &cx)
    {
    double sx;
    dsf_sincos(r * pi_over_rc, sx, cx);
    w = sx * (inv_r * rc_over_pi);
    }

}
