// orb_rotate.h — the rotation arithmetic of rotated BRIEF (orb_kernels.hip: orb_describe_kernel), host-pure: the sine and cosine of
// the key-point angle as computeOrbDescriptors forms them, (float)cos / (float)sin of the float radians in double precision, and the
// rotation of one pattern point with cvRound of FLOAT products.  No HIP types: tests/cpp/orb_rotate_host_main.cpp compiles this file
// with the host compiler and holds it to the C library and to the plain form (every float angle in [0, 360] degrees, every int8 pair).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ORB_HD __host__ __device__ __forceinline__
#else
#define ORB_HD inline
#endif

// no fused multiply-adds: OpenCV rounds every product (host builds pass -ffp-contract=off)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace stvo {

// sine and cosine of a float angle in [0, 2 pi] in double precision (the routine of lsd_kernels.hip / oracle/stvo_lsd_oracle.c)
ORB_HD void orb_sincos(float xf, double& s, double& c) {
    const double x = (double)xf;
    const double PIO2_HI = 1.57079632679489655800e+00, PIO2_LO = 6.12323399573676603587e-17, TWO_OVER_PI = 6.36619772367581382433e-01;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double k = __builtin_rint(x * TWO_OVER_PI);
    double r = __builtin_fma(-k, PIO2_HI, x);
    r = __builtin_fma(-k, PIO2_LO, r);
    const double z = r * r;
    const double sn = r + (z * r) * (S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))));
    const double cs = 1.0 - (0.5 * z - z * (z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))));
    const int q = (int)k & 3;
    s = q == 0 ? sn : (q == 1 ? cs : (q == 2 ? -sn : -cs));
    c = q == 0 ? cs : (q == 1 ? -sn : (q == 2 ? -cs : sn));
}

// the key-point's rotation from its angle in degrees: a = (float)cos(rad), b = (float)sin(rad), rad = angle * (float)(pi / 180).
// One Cody-Waite + kernel-polynomial evaluation (within an ulp of the library's double results) instead of two library calls of
// ~100 instructions each; the host sweep finds the same floats as the library for every float angle in [0, 360]
ORB_HD void orb_rotation(float angle_deg, float& a, float& b) {
    const float rad = angle_deg * (float)(3.14159265358979323846 / 180.0);
    double sd, cd;
    orb_sincos(rad, sd, cd);
    a = (float)cd;
    b = (float)sd;
}

// cvRound of a float: to the nearest integer, halves to the even one
ORB_HD int orb_cv_round(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float2int_rn(v);
#else
    return (int)__builtin_rintf(v);  // (the default rounding mode)
#endif
}

}  // namespace stvo

// One pattern point (px, py) rotated by (a, b) = (cos, sin): two float products and one float sum per coordinate, then cvRound.
// Macros, not functions: wrapped in an inline function the same expressions reach the gfx950 scheduler in another order and
// orb_describe_kernel's code changes (same results, other instruction order); as text the kernel's code is what it was.
#define ORB_ROTATE_X(px, py, a, b) stvo::orb_cv_round((px) * (a) - (py) * (b))
#define ORB_ROTATE_Y(px, py, a, b) stvo::orb_cv_round((px) * (b) + (py) * (a))
