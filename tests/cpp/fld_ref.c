/* fld_ref.c — the CPU statement of the FLD key-line front-end: what StereoFrame::detectLineFeatures computes with
 * use_fld_lines = true (reference src/stereoFrame.cpp:244-303) through cv::ximgproc::FastLineDetector (OpenCV contrib 3.x,
 * ximgproc/src/fast_line_detector.cpp — third-party code the reference does not hold), restated in the structure of that
 * implementation.  Test infrastructure: tests/test_fld_host.py and tests/test_gpu_fld.py compile it at test time
 * (gcc -O2 -ffp-contract=off) and call it through ctypes; stvo-pl_amd/csrc/fld_kernels.hip follows it bit for bit.
 * Parity with OpenCV is unpinned (no OpenCV on the build machines), as for LSD.
 *
 * The stages:
 *   Canny        OpenCV 3.4's portable path, aperture 3, L1 gradient: Sobel 3 x 3 (BORDER_REPLICATE, int16), m = |dx| + |dy|
 *                (0 outside the image), non-maximum suppression with TG22 = 13573 in three direction cases, edge = m > floor(th1)
 *                and NMS passed.  Only th1 == th2 is built: hysteresis then adds nothing and the edge map is per pixel.
 *   corner quirk lineDetection clears canny(0..5, 0..5) and canny(rows-5..rows-1, cols-5..cols-1), not the border strips
 *   chains       raster scan (rows outer), every set pixel is a seed, getPointChain walks on; chains under L + 1 points are dropped
 *   segments     extractSegments, the length and border filters of lineDetection, additionalOperationsOnSegment
 *   key-lines    the top-N cut by double length (stable), KeyLine angle / response / numOfPixels (stereoFrame.cpp:258-298)
 *
 * Points this statement defines (the kernels follow them either way):
 *   (1) atan2, cos and sin are deterministic functions evaluated identically on host and device, not libm / OCML: atan2 is
 *       fld_atan2_det below (fdlibm's e_atan2.c / s_atan.c, within 1 ulp of libm), sin / cos are orc_sincos_det, fastAtan2 is
 *       orc_fast_atan2.  The KeyLine angle is (float)atan2_det((double)dy, (double)dx) of the float differences; whether the
 *       reference's atan2 of two floats resolves to the float overload (atan2f) is uncertain — the statement takes the double form.
 *   (2) no fused multiply-adds (-ffp-contract=off here, #pragma clang fp contract(off) in the kernels); the two inside
 *       orc_sincos_det's argument reduction are written out on both sides.
 *   (3) cvRound rounds half to even (lrint / lrintf); square roots and divisions are correctly rounded.
 *   (4) equal lengths at the top-N cut keep detection order (std::sort leaves that unspecified).
 *   (5) Canny follows OpenCV's portable C++ path; an IPP build may give a different edge map (unpinned).
 *   (6) getPointChain keeps the chain direction in a float: direction = (direction * step + d) / (step + 1).  Whether the
 *       OpenCV version the reference was built against keeps it in an int (integer division) is uncertain.
 *   (7) fitLine (DIST_L2, fitLine2D_wods): double sums in point order of float coordinates, x * x a float product, the sums
 *       divided by w = (float)count, t = (float)atan2(2 dxy, dx2 - dy2) / 2 in float, (cos t, sin t) and the centroid rounded
 *       to float.  The line through it is p0 x p1 with p0 = (x0, y0, 1) and p1 = (x0 + vx, y0 + vy, 1), the sums in float.
 *   (8) distPointLine normalises the line in place on every call (w = sqrt(l0^2 + l1^2), all three components divided by w)
 *       and returns l0 p0 + l1 p1 + l2 p2 summed in that order.
 *   (9) incidentPoint: lk = (x, y, 1) x (l0, l1, 0), xk = lk x l, xk * (1.0 / xk[2]) + 0.0 (convertTo's scale and shift),
 *       each coordinate rounded to float and clamped to [0, cols - 1] / [0, rows - 1] in float; for ps the result rounds to
 *       Point2i (cvRound).
 *  (10) length_threshold < 1 is refused (extractSegments would divide by a zero line norm).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

float orc_fast_atan2(float y, float x);                                          /* oracle/liboracle.so */
void orc_sincos_det(double x, double* s, double* c);
int orc_line_iterator_count(int cols, int rows, float sx, float sy, float ex, float ey);

#define FLD_PI 3.14159265358979323846

/* ---- (1) atan2: fdlibm 5.3 e_atan2.c + s_atan.c, the bit tests on the high / low words ---- */
static uint32_t hi_word(double x) { uint64_t u; memcpy(&u, &x, 8); return (uint32_t)(u >> 32); }
static uint32_t lo_word(double x) { uint64_t u; memcpy(&u, &x, 8); return (uint32_t)u; }

static double atan_det(double x) {
    static const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01,
                                     1.57079632679489655800e+00};
    static const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17,
                                     6.12323399573676603587e-17};
    static const double aT[11] = {3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01,
                                  -1.11111104054623557880e-01, 9.09088713343650656196e-02, -7.69187620504482999495e-02,
                                  6.66107313738753120669e-02, -5.83357013379057348645e-02, 4.97687799461593236017e-02,
                                  -3.65315727442169155270e-02, 1.62858201153657823623e-02};
    const int32_t hx = (int32_t)hi_word(x), ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x44100000) {  /* |x| >= 2^66 */
        if (ix > 0x7ff00000 || (ix == 0x7ff00000 && lo_word(x) != 0)) return x + x;
        return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3fdc0000) {   /* |x| < 0.4375 */
        if (ix < 0x3e400000) return x;  /* |x| < 2^-27 */
        id = -1;
    } else {
        x = fabs(x);
        if (ix < 0x3ff30000) {
            if (ix < 0x3fe60000) { id = 0; x = (2.0 * x - 1.0) / (2.0 + x); }
            else { id = 1; x = (x - 1.0) / (x + 1.0); }
        } else {
            if (ix < 0x40038000) { id = 2; x = (x - 1.5) / (1.0 + 1.5 * x); }
            else { id = 3; x = -1.0 / x; }
        }
    }
    const double z = x * x, w = z * z;
    const double s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const double s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) return x - x * (s1 + s2);
    const double r = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return hx < 0 ? -r : r;
}

double fld_atan2_det(double y, double x) {
    const double pi_o_4 = 7.8539816339744827900e-01, pi_o_2 = 1.5707963267948965580e+00, pi = 3.1415926535897931160e+00,
                 pi_lo = 1.2246467991473531772e-16;
    const int32_t hx = (int32_t)hi_word(x), ix = hx & 0x7fffffff, hy = (int32_t)hi_word(y), iy = hy & 0x7fffffff;
    const uint32_t lx = lo_word(x), ly = lo_word(y);
    if (ix > 0x7ff00000 || (ix == 0x7ff00000 && lx != 0) || iy > 0x7ff00000 || (iy == 0x7ff00000 && ly != 0)) return x + y;
    if (hx == 0x3ff00000 && lx == 0) return atan_det(y);  /* x = 1.0 */
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);    /* 2 sign(x) + sign(y) */
    if ((iy | ly) == 0) {                                 /* y = +-0 */
        if (m < 2) return y;
        return m == 2 ? pi : -pi;
    }
    if ((ix | lx) == 0) return hy < 0 ? -pi_o_2 : pi_o_2;  /* x = +-0 */
    if (ix == 0x7ff00000) {
        if (iy == 0x7ff00000) {
            switch (m) {
                case 0: return pi_o_4;
                case 1: return -pi_o_4;
                case 2: return 3.0 * pi_o_4;
                default: return -3.0 * pi_o_4;
            }
        }
        switch (m) {
            case 0: return 0.0;
            case 1: return -0.0;
            case 2: return pi;
            default: return -pi;
        }
    }
    if (iy == 0x7ff00000) return hy < 0 ? -pi_o_2 : pi_o_2;
    const int k = (iy - ix) >> 20;
    double z;
    if (k > 60) z = pi_o_2 + 0.5 * pi_lo;
    else if (hx < 0 && k < -60) z = 0.0;
    else z = atan_det(fabs(y / x));
    switch (m) {
        case 0: return z;
        case 1: return -z;
        case 2: return pi - (z - pi_lo);
        default: return (z - pi_lo) - pi;
    }
}

void fld_atan2_det_n(const double* y, const double* x, double* out, int n) {
    for (int i = 0; i < n; ++i) out[i] = fld_atan2_det(y[i], x[i]);
}

/* ---- Canny (th1 == th2, aperture 3, L1) + the corner quirk ---- */
static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static void sobel_at(const uint8_t* img, int cols, int rows, int x, int y, int* dx, int* dy) {
    const int xm = clampi(x - 1, 0, cols - 1), xp = clampi(x + 1, 0, cols - 1);
    const int ym = clampi(y - 1, 0, rows - 1), yp = clampi(y + 1, 0, rows - 1);
    const uint8_t *r0 = img + (size_t)ym * cols, *r1 = img + (size_t)y * cols, *r2 = img + (size_t)yp * cols;
    *dx = (r0[xp] + 2 * r1[xp] + r2[xp]) - (r0[xm] + 2 * r1[xm] + r2[xm]);
    *dy = (r2[xm] + 2 * r2[x] + r2[xp]) - (r0[xm] + 2 * r0[x] + r0[xp]);
}

/* edges [rows][cols] = 0 / 255; returns 0, or -1 for what is not built */
int fld_edges(const uint8_t* img, int cols, int rows, double th1, double th2, uint8_t* edges) {
    if (th1 != th2) return -1;
    const int low = (int)floor(th1);
    const int TG22 = (int)(0.4142135623730950488 * (1 << 15) + 0.5);
    const size_t npx = (size_t)cols * rows;
    int* gx = (int*)malloc(npx * sizeof(int));
    int* gy = (int*)malloc(npx * sizeof(int));
    int* mag = (int*)malloc(npx * sizeof(int));
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const size_t p = (size_t)y * cols + x;
            sobel_at(img, cols, rows, x, y, &gx[p], &gy[p]);
            mag[p] = abs(gx[p]) + abs(gy[p]);
        }
#define MAG(xx, yy) (((xx) < 0 || (yy) < 0 || (xx) >= cols || (yy) >= rows) ? 0 : mag[(size_t)(yy) * cols + (xx)])
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const size_t p = (size_t)y * cols + x;
            const int m = mag[p];
            int e = 0;
            if (m > low) {
                const int xs = abs(gx[p]), ys = abs(gy[p]) << 15;
                const int tg22x = xs * TG22;
                if (ys < tg22x) {
                    e = m > MAG(x - 1, y) && m >= MAG(x + 1, y);
                } else {
                    const int tg67x = tg22x + (xs << 16);
                    if (ys > tg67x) {
                        e = m > MAG(x, y - 1) && m >= MAG(x, y + 1);
                    } else {
                        const int s = (gx[p] ^ gy[p]) < 0 ? -1 : 1;
                        e = m > MAG(x - s, y - 1) && m > MAG(x + s, y + 1);
                    }
                }
            }
            edges[p] = e ? 255 : 0;
        }
#undef MAG
    for (int y = 0; y < 6 && y < rows; ++y)
        for (int x = 0; x < 6 && x < cols; ++x) edges[(size_t)y * cols + x] = 0;
    for (int y = rows - 5 < 0 ? 0 : rows - 5; y < rows; ++y)
        for (int x = cols - 5 < 0 ? 0 : cols - 5; x < cols; ++x) edges[(size_t)y * cols + x] = 0;
    free(gx); free(gy); free(mag);
    return 0;
}

/* ---- getPointChain ---- */
static const int NB_DY[8] = {1, 1, 1, 0, -1, -1, -1, 0}, NB_DX[8] = {1, 0, -1, -1, -1, 0, 1, 1};

static int get_point_chain(const uint8_t* e, int cols, int rows, int* px, int* py, float* direction, int step) {
    float min_dir_diff = 7.0f;
    int cx = 0, cy = 0, cdir = 0;
    for (int i = 0; i < 8; ++i) {
        const int ci = *px + NB_DX[i], ri = *py + NB_DY[i];
        if (ri < 0 || ri == rows || ci < 0 || ci == cols) continue;
        if (e[(size_t)ri * cols + ci] == 0) continue;
        const int d = i > 4 ? i - 8 : i;
        if (step == 0) {
            *px = ci; *py = ri;
            *direction = (float)d;
            return 1;
        }
        float dir_diff = fabsf((float)d - *direction);
        dir_diff = dir_diff > 4 ? 8 - dir_diff : dir_diff;
        if (dir_diff <= min_dir_diff) {
            min_dir_diff = dir_diff;
            cx = ci; cy = ri; cdir = d;
        }
    }
    if (min_dir_diff < 2) {
        *px = cx; *py = cy;
        *direction = (*direction * (float)step + (float)cdir) / (float)(step + 1);
        return 1;
    }
    return 0;
}

/* test hook: lineDetection's raster scan + getPointChain on a given 0 / 255 edge map (modified): every chain, short ones
 * included; xy [cap][2] the points in order, lens [max_chains]; returns the number of chains */
int fld_walk_edges(uint8_t* e, int cols, int rows, int32_t* xy, int cap, int32_t* lens, int max_chains) {
    int nch = 0, used = 0;
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) {
            if (e[(size_t)r * cols + c] == 0) continue;
            int x = c, y = r, total = 0;
            if (used < cap) { xy[2 * used] = x; xy[2 * used + 1] = y; }
            used++; total++;
            e[(size_t)y * cols + x] = 0;
            float direction = 0.0f;
            int step = 0;
            while (get_point_chain(e, cols, rows, &x, &y, &direction, step)) {
                if (used < cap) { xy[2 * used] = x; xy[2 * used + 1] = y; }
                used++; total++;
                step++;
                e[(size_t)y * cols + x] = 0;
            }
            if (nch < max_chains) lens[nch] = total;
            nch++;
        }
    return nch;
}

/* ---- extractSegments ---- */
typedef struct { int x, y; } pt2i;

static void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

static double dist_point_line(double* l, double px, double py) {
    const double x = l[0], y = l[1], w = sqrt(x * x + y * y);
    l[0] = x / w; l[1] = y / w; l[2] = l[2] / w;
    return l[0] * px + l[1] * py + l[2] * 1.0;
}

/* fitLine(DIST_L2) over pts[0 .. n) and the homogeneous line through the fit */
static void fit_line(const pt2i* pts, int n, double* l) {
    double x = 0, y = 0, x2 = 0, y2 = 0, xy = 0;
    for (int i = 0; i < n; ++i) {
        const float fx = (float)pts[i].x, fy = (float)pts[i].y;
        x += fx; y += fy;
        x2 += fx * fx; y2 += fy * fy; xy += fx * fy;
    }
    const double w = (float)n;
    x /= w; y /= w; x2 /= w; y2 /= w; xy /= w;
    const double dx2 = x2 - x * x, dy2 = y2 - y * y, dxy = xy - x * y;
    const float t = (float)fld_atan2_det(2 * dxy, dx2 - dy2) / 2;
    double s, c;
    orc_sincos_det((double)t, &s, &c);
    const float vx = (float)c, vy = (float)s, x0 = (float)x, y0 = (float)y;
    const double a[3] = {x0, y0, 1.0}, b[3] = {(double)(x0 + vx), (double)(y0 + vy), 1.0};
    cross3(a, b, l);
}

static void incident_point(const double* l, float* px, float* py, int cols, int rows) {
    const double a[3] = {(double)*px, (double)*py, 1.0}, b[3] = {l[0], l[1], 0.0};
    double lk[3], xk[3];
    cross3(a, b, lk);
    cross3(lk, l, xk);
    const double sc = 1.0 / xk[2];
    const float fx = (float)(xk[0] * sc + 0.0), fy = (float)(xk[1] * sc + 0.0);
    const float wm = (float)cols - 1.0f, hm = (float)rows - 1.0f;
    *px = fx < 0.0f ? 0.0f : (fx >= wm ? wm : fx);
    *py = fy < 0.0f ? 0.0f : (fy >= hm ? hm : fy);
}

/* the segments of one chain, appended to seg (4 floats each); returns the number appended */
static int extract_segments(const pt2i* P, int total, int L, float dist_th, int cols, int rows, float* seg) {
    int ns = 0;
    for (int i = 0; i + L < total; i++) {
        double l[3];
        {
            const double a[3] = {P[i].x, P[i].y, 1.0}, b[3] = {P[i + L].x, P[i + L].y, 1.0};
            cross3(a, b, l);
        }
        int fail = 0;
        for (int j = 1; j < L; j++)
            if (fabs(dist_point_line(l, P[i + j].x, P[i + j].y)) > dist_th) { fail = 1; break; }
        if (fail) continue;
        int cnt = L + 1;  /* l_points = P[i .. i + cnt) */
        pt2i pe = P[i + L];
        fit_line(P + i, cnt, l);
        float psx = (float)P[i].x, psy = (float)P[i].y;
        incident_point(l, &psx, &psy, cols, rows);
        const pt2i ps = {(int)lrintf(psx), (int)lrintf(psy)};
        int j;
        for (j = L + 1; i + j < total; j++) {
            const pt2i pt = P[i + j];
            double d = dist_point_line(l, pt.x, pt.y);
            if (fabs(d) > dist_th) {
                fit_line(P + i, cnt, l);
                d = dist_point_line(l, pt.x, pt.y);
                if (fabs(d) > dist_th) { j--; break; }
            }
            pe = pt;
            cnt++;
        }
        fit_line(P + i, cnt, l);
        float e1x = (float)ps.x, e1y = (float)ps.y, e2x = (float)pe.x, e2y = (float)pe.y;
        incident_point(l, &e1x, &e1y, cols, rows);
        incident_point(l, &e2x, &e2y, cols, rows);
        seg[4 * ns + 0] = e1x; seg[4 * ns + 1] = e1y; seg[4 * ns + 2] = e2x; seg[4 * ns + 3] = e2y;
        ns++;
        i = i + j;
    }
    return ns;
}

/* ---- lineDetection's filters + additionalOperationsOnSegment ---- */
static float get_angle(float x1, float y1, float x2, float y2) {
    return (float)(orc_fast_atan2(y2 - y1, x2 - x1) / 180.0f * FLD_PI);
}

static int keep_segment(const float* s, int L, int cols, int rows) {
    const float len = sqrtf((s[0] - s[2]) * (s[0] - s[2]) + (s[1] - s[3]) * (s[1] - s[3]));
    if (len < (float)L) return 0;
    if ((s[0] <= 5.0f && s[2] <= 5.0f) || (s[1] <= 5.0f && s[3] <= 5.0f) || (s[0] >= (float)cols - 5.0f && s[2] >= (float)cols - 5.0f) ||
        (s[1] >= (float)rows - 5.0f && s[3] >= (float)rows - 5.0f))
        return 0;
    return 1;
}

static void orient_segment(const uint8_t* img, int cols, int rows, float* s) {
    const double ang = (double)get_angle(s[0], s[1], s[2], s[3]);
    const double dx = (double)s[2] - (double)s[0], dy = (double)s[3] - (double)s[1];
    float qx[10], qy[10];
    qx[0] = s[0]; qy[0] = s[1]; qx[9] = s[2]; qy[9] = s[3];
    for (int i = 1; i < 9; ++i) {
        qx[i] = qx[0] + ((float)dx / (float)9 * (float)i);
        qy[i] = qy[0] + ((float)dy / (float)9 * (float)i);
    }
    double sn, cs;
    orc_sincos_det(90.0 * FLD_PI / 180.0 + ang, &sn, &cs);
    int iR = 0, iL = 0;
    for (int i = 0; i < 10; ++i) {
        int rx = (int)lrint(qx[i] + 1.0 * cs), ry = (int)lrint(qy[i] + 1.0 * sn);
        int lx = (int)lrint(qx[i] - 1.0 * cs), ly = (int)lrint(qy[i] - 1.0 * sn);
        rx = rx <= 5 ? 5 : (rx >= cols - 5 ? cols - 5 : rx);
        ry = ry <= 5 ? 5 : (ry >= rows - 5 ? rows - 5 : ry);
        lx = lx <= 5 ? 5 : (lx >= cols - 5 ? cols - 5 : lx);
        ly = ly <= 5 ? 5 : (ly >= rows - 5 ? rows - 5 : ly);
        iR += img[(size_t)ry * cols + rx];
        iL += img[(size_t)ly * cols + lx];
    }
    if (iR > iL) {
        float t = s[0]; s[0] = s[2]; s[2] = t;
        t = s[1]; s[1] = s[3]; s[3] = t;
    }
}

/* FastLineDetector::detect: the segments [n][4] in detection order (at most cap stored); returns the number found, or < 0 */
int fld_segments(const uint8_t* img, int cols, int rows, int L, float dist_th, double th1, double th2, float* out, int cap) {
    if (L < 1 || cols < 16 || rows < 16) return -2;
    const size_t npx = (size_t)cols * rows;
    uint8_t* e = (uint8_t*)malloc(npx);
    if (fld_edges(img, cols, rows, th1, th2, e) != 0) { free(e); return -1; }
    pt2i* P = (pt2i*)malloc(npx * sizeof(pt2i));
    float* seg = (float*)malloc((npx / (L + 1) + 1) * 4 * sizeof(float));
    int n = 0;
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) {
            if (e[(size_t)r * cols + c] == 0) continue;
            int x = c, y = r, total = 0;
            P[total++] = (pt2i){x, y};
            e[(size_t)y * cols + x] = 0;
            float direction = 0.0f;
            int step = 0;
            while (get_point_chain(e, cols, rows, &x, &y, &direction, step)) {
                P[total++] = (pt2i){x, y};
                step++;
                e[(size_t)y * cols + x] = 0;
            }
            if (total < L + 1) continue;
            const int ns = extract_segments(P, total, L, dist_th, cols, rows, seg);
            for (int k = 0; k < ns; ++k) {
                float* s = seg + 4 * k;
                if (!keep_segment(s, L, cols, rows)) continue;
                orient_segment(img, cols, rows, s);
                if (n < cap) memcpy(out + 4 * (size_t)n, s, 16);
                n++;
            }
        }
    free(e); free(P); free(seg);
    return n;
}

/* the double length of sort_flines_by_length (auxiliar.h:149-154) */
double fld_sort_length(const float* s) {
    const double dx = (double)(s[0] - s[2]), dy = (double)(s[1] - s[3]);
    return sqrt(pow(dx, 2.0) + pow(dy, 2.0));
}

typedef struct {
    float sx, sy, ex, ey, angle;
    int32_t num_pixels;
} fld_keyline;

/* stereoFrame.cpp:244-298 for one image: at most K key-lines (the longest when nfeatures or K cuts, else detection order) among the
 * first rank_cap segments (the device ranks 8192: the rest are counted, not ranked), responses; returns the number of key-lines,
 * *n_found = segments found before the cuts. */
int fld_keylines(const uint8_t* img, int cols, int rows, int L, float dist_th, double th1, double th2, int nfeatures, int K,
                 int rank_cap, fld_keyline* lines, float* response, int* n_found) {
    int cap = 4096;
    float* seg = NULL;
    int n;
    for (;;) {
        seg = (float*)malloc((size_t)cap * 16);
        n = fld_segments(img, cols, rows, L, dist_th, th1, th2, seg, cap);
        if (n <= cap) break;
        free(seg);
        cap = n;
    }
    if (n < 0) { free(seg); return n; }
    if (n_found) *n_found = n;
    if (n > rank_cap) n = rank_cap;
    int n_out = nfeatures != 0 && nfeatures < n ? nfeatures : n;
    if (n_out > K) n_out = K;
    int* order = (int*)malloc((size_t)(n > 0 ? n : 1) * sizeof(int));
    double* len = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
    for (int i = 0; i < n; ++i) { order[i] = i; len[i] = fld_sort_length(seg + 4 * (size_t)i); }
    if (n > n_out) {  /* stable: insertion sort by descending length */
        for (int i = 1; i < n; ++i) {
            const int v = order[i];
            int j = i - 1;
            while (j >= 0 && len[order[j]] < len[v]) { order[j + 1] = order[j]; --j; }
            order[j + 1] = v;
        }
    }
    const float mx = (float)(cols > rows ? cols : rows);
    for (int k = 0; k < n_out; ++k) {
        const float* s = seg + 4 * (size_t)order[k];
        fld_keyline q;
        q.sx = s[0]; q.sy = s[1]; q.ex = s[2]; q.ey = s[3];
        q.angle = (float)fld_atan2_det((double)(q.ey - q.sy), (double)(q.ex - q.sx));
        q.num_pixels = orc_line_iterator_count(cols, rows, s[0], s[1], s[2], s[3]);
        lines[k] = q;
        const float line_length = (float)len[order[k]];
        if (response) response[k] = line_length / mx;
    }
    free(order); free(len); free(seg);
    return n_out;
}
