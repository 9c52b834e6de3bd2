// line_common.h — device helpers the two key-line detectors share (lsd_kernels.hip, fld_kernels.hip): the deterministic double
// sine / cosine of the statements (oracle/stvo_lsd_oracle.c: orc_sincos_det) and cv::LineIterator's count (KeyLine::numOfPixels).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace stvo {

// orc_sincos_det (oracle/stvo_lsd_oracle.c), operation for operation
__device__ __forceinline__ void sincos_det(double x, double& s, double& c) {
    const double PIO2_HI = 1.57079632679489655800e+00, PIO2_LO = 6.12323399573676603587e-17, TWO_OVER_PI = 6.36619772367581382433e-01;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double k = __builtin_rint(x * TWO_OVER_PI);
    double r = __builtin_fma(-k, PIO2_HI, x);
    r = __builtin_fma(-k, PIO2_LO, r);
    const double z = r * r;
    const double ps = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    const double sn = r + (z * r) * (S1 + z * ps);
    const double pc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double cs = 1.0 - (0.5 * z - z * pc);
    const int q = (int)((long long)k & 3);
    s = q == 0 ? sn : (q == 1 ? cs : (q == 2 ? -sn : -cs));
    c = q == 0 ? cs : (q == 1 ? -sn : (q == 2 ? -cs : sn));
}

// cv::LineIterator(img, Point2f(sx, sy), Point2f(ex, ey)).count (LSDDetector_custom.cpp:286-287): Point2f -> Point by cvRound, then
// cv::clipLine on the image's rectangle (64-bit integers, the intersections through a double quotient truncated towards zero — the
// statement of oracle/stvo_lsd_oracle.c: clip_line), then max(|dx|, |dy|) + 1 for the 8-connected raster; 0 when nothing is left.
__device__ __forceinline__ int line_iterator_count(int cols, int rows, float sx, float sy, float ex, float ey) {
    long long x1 = __float2int_rn(sx), y1 = __float2int_rn(sy), x2 = __float2int_rn(ex), y2 = __float2int_rn(ey);
    const long long right = cols - 1, bottom = rows - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    if ((c1 | c2) != 0) return 0;
    const long long dx = x2 > x1 ? x2 - x1 : x1 - x2, dy = y2 > y1 ? y2 - y1 : y1 - y2;
    return (int)((dx > dy ? dx : dy) + 1);
}

}  // namespace stvo
