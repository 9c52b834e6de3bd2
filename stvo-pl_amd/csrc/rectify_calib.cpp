// rectify_calib.cpp — stereo calibration -> rectification, on the host, once per camera (stvo_rectify_compute).
//
// The three branches of the reference's YAML constructor (src/pinholeStereoCamera.cpp:30-125): KITTI-style undistortion only,
// stereoRectify + initUndistortRectifyMap (rad-tan), stereoRectify + fisheye::initUndistortRectifyMap.  stereoRectify follows
// OpenCV 3.4's cvStereoRectify in the form DESIGN.md §9 states (k1-adjusted minimum focal length, `width` terms), with
// CALIB_ZERO_DISPARITY and alpha = 0; the maps follow the scalar loops of initUndistortRectifyMap in their order of operations and
// the CV_16SC2 encoding.  Built with -ffp-contract=off: the maps must match tests/np_rectify.py bit for bit, and a fused
// multiply-add rounds differently from the multiply and the add it replaces.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include "../../include/stvo_hip.h"

namespace {

// c = a b (3 x 3, row-major), each entry summed left to right
void mul3(const double* a, const double* b, double* c) {
    double t[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t[i * 3 + j] = a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j] + a[i * 3 + 2] * b[2 * 3 + j];
    std::memcpy(c, t, sizeof(t));
}
// c = a b^T
void mul3_bt(const double* a, const double* b, double* c) {
    double t[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t[i * 3 + j] = a[i * 3 + 0] * b[j * 3 + 0] + a[i * 3 + 1] * b[j * 3 + 1] + a[i * 3 + 2] * b[j * 3 + 2];
    std::memcpy(c, t, sizeof(t));
}
void mulv(const double* a, const double* v, double* o) {
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = a[i * 3 + 0] * v[0] + a[i * 3 + 1] * v[1] + a[i * 3 + 2] * v[2];
    std::memcpy(o, t, sizeof(t));
}
double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// cv::invert(DECOMP_LU) of a 3 x 3 double matrix: the cofactor form OpenCV takes for n = 3
bool inv3(const double* m, double* t) {
    auto S = [m](int i, int j) { return m[i * 3 + j]; };
    double d = S(0, 0) * (S(1, 1) * S(2, 2) - S(1, 2) * S(2, 1)) - S(0, 1) * (S(1, 0) * S(2, 2) - S(1, 2) * S(2, 0)) +
               S(0, 2) * (S(1, 0) * S(2, 1) - S(1, 1) * S(2, 0));
    if (d == 0.) return false;
    d = 1. / d;
    t[0] = (S(1, 1) * S(2, 2) - S(1, 2) * S(2, 1)) * d;
    t[1] = (S(0, 2) * S(2, 1) - S(0, 1) * S(2, 2)) * d;
    t[2] = (S(0, 1) * S(1, 2) - S(0, 2) * S(1, 1)) * d;
    t[3] = (S(1, 2) * S(2, 0) - S(1, 0) * S(2, 2)) * d;
    t[4] = (S(0, 0) * S(2, 2) - S(0, 2) * S(2, 0)) * d;
    t[5] = (S(0, 2) * S(1, 0) - S(0, 0) * S(1, 2)) * d;
    t[6] = (S(1, 0) * S(2, 1) - S(1, 1) * S(2, 0)) * d;
    t[7] = (S(0, 1) * S(2, 0) - S(0, 0) * S(2, 1)) * d;
    t[8] = (S(0, 0) * S(1, 1) - S(0, 1) * S(1, 0)) * d;
    return true;
}

// cvRodrigues2, vector -> matrix
void rodrigues_v2m(const double* rv, double* R) {
    double theta = norm3(rv);
    if (theta < DBL_EPSILON) {
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        std::memcpy(R, I, sizeof(I));
        return;
    }
    const double c = std::cos(theta), s = std::sin(theta), c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
    const double x = rv[0] * itheta, y = rv[1] * itheta, z = rv[2] * itheta;
    const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
    const double rx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) R[k] = c * I[k] + c1 * rrt[k] + s * rx[k];
}

// cvRodrigues2, matrix -> vector.  OpenCV first replaces R by U V^T of its SVD (the orthogonal polar factor); the Newton iteration
// X <- (X + X^-T) / 2 converges to the same factor (quadratically, from a matrix that is already nearly a rotation).
void rodrigues_m2v(const double* R0, double* rv) {
    double R[9];
    std::memcpy(R, R0, sizeof(R));
    for (int it = 0; it < 8; ++it) {
        double iv[9];
        if (!inv3(R, iv)) break;
        double dmax = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double nv = 0.5 * (R[i * 3 + j] + iv[j * 3 + i]);
                dmax = std::fmax(dmax, std::fabs(nv - R[i * 3 + j]));
                R[i * 3 + j] = nv;
            }
        if (dmax < 1e-17) break;
    }
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = std::sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1. ? 1. : c < -1. ? -1. : c;
    double theta = std::acos(c);
    if (s < 1e-5) {
        if (c > 0) {
            rx = ry = rz = 0;
        } else {
            double t = (R[0] + 1) * 0.5;
            rx = std::sqrt(std::fmax(t, 0.));
            t = (R[4] + 1) * 0.5;
            ry = std::sqrt(std::fmax(t, 0.)) * (R[1] < 0 ? -1. : 1.);
            t = (R[8] + 1) * 0.5;
            rz = std::sqrt(std::fmax(t, 0.)) * (R[2] < 0 ? -1. : 1.);
            if (std::fabs(rx) < std::fabs(ry) && std::fabs(rx) < std::fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
            const double v[3] = {rx, ry, rz};
            theta /= norm3(v);
            rx *= theta; ry *= theta; rz *= theta;
        }
    } else {
        double vth = 1 / (2 * s);
        vth *= theta;
        rx *= vth; ry *= vth; rz *= vth;
    }
    rv[0] = rx; rv[1] = ry; rv[2] = rz;
}

// rad-tan coefficients in cvUndistortPoints' k[] order: k1 k2 p1 p2 k3 k4 k5 k6 (s1..s4, tau: 0)
struct Dist {
    double k[12];
};
Dist radtan(const double* D, int n) {
    Dist d;
    std::memset(&d, 0, sizeof(d));
    for (int i = 0; i < n && i < 8; ++i) d.k[i] = D[i];
    return d;
}

// cvUndistortPoints on float32 points (5 fixed-point iterations), RR = P[:, :3] R or I; the result rounded to float32
void undistort_points(const float* in, float* out, int n, const double* K, const Dist& dk, const double* RR) {
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3], ifx = 1. / fx, ify = 1. / fy;
    const double* k = dk.k;
    for (int i = 0; i < n; ++i) {
        double x = in[2 * i], y = in[2 * i + 1];
        x = (x - cx) * ifx;
        y = (y - cy) * ify;
        const double x0 = x, y0 = y;
        for (int j = 0; j < 5; ++j) {
            const double r2 = x * x + y * y;
            const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
            const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
            const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
            x = (x0 - deltaX) * icdist;
            y = (y0 - deltaY) * icdist;
        }
        const double xx = RR[0] * x + RR[1] * y + RR[2];
        const double yy = RR[3] * x + RR[4] * y + RR[5];
        const double ww = 1. / (RR[6] * x + RR[7] * y + RR[8]);
        out[2 * i] = (float)(xx * ww);
        out[2 * i + 1] = (float)(yy * ww);
    }
}

// icvGetRectangles: a 9 x 9 grid of float32 points over [0, width] x [0, height] through undistortion, R and P; inner = the
// rectangle inside the outermost rows / columns, outer = the bounding box.  Rectangles as (x, y, w, h) in float32.
void get_rectangles(const double* K, const Dist& dk, const double* R, const double* P, int w, int h, float inner[4], float outer[4]) {
    const int N = 9;
    float pts[2 * N * N];
    for (int y = 0, k = 0; y < N; ++y)
        for (int x = 0; x < N; ++x, ++k) {
            pts[2 * k] = (float)x * (float)w / (float)(N - 1);
            pts[2 * k + 1] = (float)y * (float)h / (float)(N - 1);
        }
    const double P3[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    double RR[9];
    mul3(P3, R, RR);
    undistort_points(pts, pts, N * N, K, dk, RR);
    float iX0 = -FLT_MAX, iX1 = FLT_MAX, iY0 = -FLT_MAX, iY1 = FLT_MAX;
    float oX0 = FLT_MAX, oX1 = -FLT_MAX, oY0 = FLT_MAX, oY1 = -FLT_MAX;
    for (int y = 0, k = 0; y < N; ++y)
        for (int x = 0; x < N; ++x, ++k) {
            const float px = pts[2 * k], py = pts[2 * k + 1];
            oX0 = std::fmin(oX0, px); oX1 = std::fmax(oX1, px);
            oY0 = std::fmin(oY0, py); oY1 = std::fmax(oY1, py);
            if (x == 0) iX0 = std::fmax(iX0, px);
            if (x == N - 1) iX1 = std::fmin(iX1, px);
            if (y == 0) iY0 = std::fmax(iY0, py);
            if (y == N - 1) iY1 = std::fmin(iY1, py);
        }
    inner[0] = iX0; inner[1] = iY0; inner[2] = iX1 - iX0; inner[3] = iY1 - iY0;
    outer[0] = oX0; outer[1] = oY0; outer[2] = oX1 - oX0; outer[3] = oY1 - oY0;
}

// cvStereoRectify(CALIB_ZERO_DISPARITY, alpha = 0, newImageSize = imageSize) in the form of DESIGN.md §9
void stereo_rectify(const double* K1, const Dist& d1, const double* K2, const Dist& d2, int width, int height, const double* Rm,
                    const double* T, double* R1, double* R2, double* P1, double* P2) {
    const double nx = width, ny = height;
    double om[3], r_r[9], t[3];
    rodrigues_m2v(Rm, om);
    for (int i = 0; i < 3; ++i) om[i] *= -0.5;  // half the rotation for each camera
    rodrigues_v2m(om, r_r);
    mulv(r_r, T, t);
    const int idx = std::fabs(t[0]) > std::fabs(t[1]) ? 0 : 1;
    const double c = t[idx], nt = norm3(t);
    double uu[3] = {0, 0, 0};
    uu[idx] = c > 0 ? 1 : -1;
    // the global rotation that takes the rotated baseline onto the axis
    double ww[3] = {t[1] * uu[2] - t[2] * uu[1], t[2] * uu[0] - t[0] * uu[2], t[0] * uu[1] - t[1] * uu[0]};
    const double nw = norm3(ww);
    if (nw > 0.0) {
        const double sc = std::acos(std::fabs(c) / nt) / nw;
        for (int i = 0; i < 3; ++i) ww[i] *= sc;
    }
    double wR[9];
    rodrigues_v2m(ww, wR);
    mul3_bt(wR, r_r, R1);
    mul3(wR, r_r, R2);
    mulv(R2, T, t);

    // focal length: the smaller of the two, each reduced by its k1 when k1 < 0 (fy for horizontal stereo)
    double fc_new = DBL_MAX;
    for (int k = 0; k < 2; ++k) {
        const double* A = k == 0 ? K1 : K2;
        const double dk1 = (k == 0 ? d1 : d2).k[0];
        double fc = A[idx ^ 1];  // K = (fx, fy, cx, cy): A(idx^1, idx^1)
        if (dk1 < 0) fc *= 1 + dk1 * (nx * nx + ny * ny) / (4 * fc * fc);
        fc_new = std::fmin(fc_new, fc);
    }
    // principal points: the image corners undistorted, rotated and projected with fc_new; the shift that centres their mean
    double ccx[2], ccy[2];
    for (int k = 0; k < 2; ++k) {
        float pts[8];
        for (int i = 0; i < 4; ++i) {
            const int j = i < 2 ? 0 : 1;
            pts[2 * i] = (float)((i % 2) * (nx - 1));
            pts[2 * i + 1] = (float)(j * (ny - 1));
        }
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        undistort_points(pts, pts, 4, k == 0 ? K1 : K2, k == 0 ? d1 : d2, I);
        const double* Rk = k == 0 ? R1 : R2;
        double sx = 0, sy = 0;
        for (int i = 0; i < 4; ++i) {
            const double X = pts[2 * i], Y = pts[2 * i + 1], Z = 1.0f;
            double x = Rk[0] * X + Rk[1] * Y + Rk[2] * Z + 0.0;
            double y = Rk[3] * X + Rk[4] * Y + Rk[5] * Z + 0.0;
            double z = Rk[6] * X + Rk[7] * Y + Rk[8] * Z + 0.0;
            z = z ? 1. / z : 1;
            x *= z;
            y *= z;
            sx += (double)(float)(x * fc_new + 0.0);
            sy += (double)(float)(y * fc_new + 0.0);
        }
        ccx[k] = (nx - 1) / 2 - sx * 0.25;
        ccy[k] = (ny - 1) / 2 - sy * 0.25;
    }
    // CALIB_ZERO_DISPARITY: one principal point for both
    ccx[0] = ccx[1] = (ccx[0] + ccx[1]) * 0.5;
    ccy[0] = ccy[1] = (ccy[0] + ccy[1]) * 0.5;

    std::memset(P1, 0, 12 * sizeof(double));
    P1[0] = P1[5] = fc_new;
    P1[2] = ccx[0];
    P1[6] = ccy[0];
    P1[10] = 1;
    std::memcpy(P2, P1, 12 * sizeof(double));
    P2[2] = ccx[1];
    P2[6] = ccy[1];
    P2[idx * 4 + 3] = t[idx] * fc_new;

    const double alpha = 0.0;
    float in1[4], out1[4], in2[4], out2[4];
    get_rectangles(K1, d1, R1, P1, width, height, in1, out1);
    get_rectangles(K2, d2, R2, P2, width, height, in2, out2);
    const double cx1_0 = ccx[0], cy1_0 = ccy[0], cx2_0 = ccx[1], cy2_0 = ccy[1];
    const double cx1 = width * cx1_0 / width, cy1 = height * cy1_0 / height;
    const double cx2 = width * cx2_0 / width, cy2 = height * cy2_0 / height;
    double s0 = std::fmax(std::fmax(std::fmax(cx1 / (cx1_0 - in1[0]), cy1 / (cy1_0 - in1[1])),
                                    (width - cx1) / ((double)(float)(in1[0] + in1[2]) - cx1_0)),
                          (height - cy1) / ((double)(float)(in1[1] + in1[3]) - cy1_0));
    s0 = std::fmax(std::fmax(std::fmax(std::fmax(cx2 / (cx2_0 - in2[0]), cy2 / (cy2_0 - in2[1])),
                                       (width - cx2) / ((double)(float)(in2[0] + in2[2]) - cx2_0)),
                             (height - cy2) / ((double)(float)(in2[1] + in2[3]) - cy2_0)),
                   s0);
    double s1 = std::fmin(std::fmin(std::fmin(cx1 / (cx1_0 - out1[0]), cy1 / (cy1_0 - out1[1])),
                                    (width - cx1) / ((double)(float)(out1[0] + out1[2]) - cx1_0)),
                          (height - cy1) / ((double)(float)(out1[1] + out1[3]) - cy1_0));
    s1 = std::fmin(std::fmin(std::fmin(std::fmin(cx2 / (cx2_0 - out2[0]), cy2 / (cy2_0 - out2[1])),
                                       (width - cx2) / ((double)(float)(out2[0] + out2[2]) - cx2_0)),
                             (height - cy2) / ((double)(float)(out2[1] + out2[3]) - cy2_0)),
                   s1);
    const double s = s0 * (1 - alpha) + s1 * alpha;
    fc_new *= s;
    P1[0] = P1[5] = fc_new;
    P1[2] = cx1;
    P1[6] = cy1;
    P2[0] = P2[5] = fc_new;
    P2[2] = cx2;
    P2[6] = cy2;
    P2[idx * 4 + 3] = s * P2[idx * 4 + 3];
}

// cvRound of the fixed-point coordinate (round half to even), clamped to int
inline int round_fix(double v) {
    v *= 32;
    if (!(v > -2147483648.0)) return INT_MIN;  // -inf and NaN
    if (v > 2147483647.0) return INT_MAX;
    return (int)std::nearbyint(v);
}
inline void encode(double u, double v, int16_t* m1, uint16_t* m2) {
    const int iu = round_fix(u), iv = round_fix(v);
    m1[0] = (int16_t)(iu >> 5);
    m1[1] = (int16_t)(iv >> 5);
    *m2 = (uint16_t)((iv & 31) * 32 + (iu & 31));
}

// initUndistortRectifyMap (rad-tan), CV_16SC2: the scalar loop of OpenCV 3.4, accumulation order included
void map_radtan(const double* K, const Dist& dk, const double* R, const double* P, int w, int h, int16_t* m1, uint16_t* m2) {
    const double P3[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    double PR[9], ir[9];
    mul3(P3, R, PR);
    inv3(PR, ir);
    const double u0 = K[2], v0 = K[3], fx = K[0], fy = K[1];
    const double* k = dk.k;
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    for (int i = 0; i < h; ++i) {
        double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
        for (int j = 0; j < w; ++j, _x += ir[0], _y += ir[3], _w += ir[6]) {
            const double ww = 1. / _w, x = _x * ww, y = _y * ww;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
            const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
            const double u = fx * xd + u0, v = fy * yd + v0;
            const size_t o = (size_t)i * w + j;
            encode(u, v, m1 + 2 * o, m2 + o);
        }
    }
}

// fisheye::initUndistortRectifyMap (equidistant), CV_16SC2.  OpenCV inverts P R by SVD; the cofactor inverse here agrees with it
// to rounding.
void map_fisheye(const double* K, const double* D, const double* R, const double* P, int w, int h, int16_t* m1, uint16_t* m2) {
    const double P3[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    double PR[9], iR[9];
    mul3(P3, R, PR);
    inv3(PR, iR);
    const double f0 = K[0], f1 = K[1], c0 = K[2], c1 = K[3];
    for (int i = 0; i < h; ++i) {
        double _x = i * iR[1] + iR[2], _y = i * iR[4] + iR[5], _w = i * iR[7] + iR[8];
        for (int j = 0; j < w; ++j) {
            double u, v;
            if (_w <= 0) {
                u = (_x > 0) ? -INFINITY : INFINITY;
                v = (_y > 0) ? -INFINITY : INFINITY;
            } else {
                const double x = _x / _w, y = _y / _w;
                const double r = std::sqrt(x * x + y * y);
                const double theta = std::atan(r);
                const double theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
                const double theta_d = theta * (1 + D[0] * theta2 + D[1] * theta4 + D[2] * theta6 + D[3] * theta8);
                const double scale = (r == 0) ? 1.0 : theta_d / r;
                u = f0 * x * scale + c0;
                v = f1 * y * scale + c1;
            }
            const size_t o = (size_t)i * w + j;
            encode(u, v, m1 + 2 * o, m2 + o);
            _x += iR[0];
            _y += iR[3];
            _w += iR[6];
        }
    }
}

inline double f32(double v) { return (double)(float)v; }

}  // namespace

extern "C" int stvo_rectify_compute(const stvo_rect_calib* c, stvo_rect_camera* out, int16_t* map1, uint16_t* map2) {
    if (!c || !out || c->width <= 0 || c->height <= 0 || c->width > 32767 || c->height > 32767) return STVO_ERR_INVALID_ARG;
    const int w = c->width, h = c->height;
    const size_t npx = (size_t)w * h;
    std::memset(out, 0, sizeof(*out));
    out->width = w;
    out->height = h;
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (c->form == STVO_RECT_FORM_KITTI) {
        // src/pinholeStereoCamera.cpp:99-121: Kl, Dl, Pl are Mat_<float>; P repeats fx on the diagonal (:114); R = I
        const double fx = std::fabs(c->fx), fy = std::fabs(c->fy);
        out->dist = c->d[0] != 0.0;
        const double K[4] = {f32(fx), f32(fy), f32(c->cx), f32(c->cy)};
        const double D[5] = {f32(c->d[0]), f32(c->d[1]), f32(c->d[2]), f32(c->d[3]), 0.0};
        std::memcpy(out->R1, I, sizeof(I));
        std::memcpy(out->R2, I, sizeof(I));
        const double P[12] = {K[0], 0, K[2], 0, 0, K[0], K[3], 0, 0, 0, 1, 0};
        std::memcpy(out->P1, P, sizeof(P));
        std::memcpy(out->P2, P, sizeof(P));
        out->cam = stvo_cam{fx, fy, c->cx, c->cy, c->b};
        if (map1 || map2) {
            int16_t* m1 = map1 ? map1 : new int16_t[2 * npx];
            uint16_t* m2 = map2 ? map2 : new uint16_t[npx];
            map_radtan(K, radtan(D, 5), I, P, w, h, m1, m2);
            if (map1) std::memcpy(map1 + 2 * npx, map1, 2 * npx * sizeof(int16_t));  // undistmap1r = undistmap1l (:119-120)
            if (map2) std::memcpy(map2 + npx, map2, npx * sizeof(uint16_t));
            if (!map1) delete[] m1;
            if (!map2) delete[] m2;
        }
        return STVO_OK;
    }
    if (c->form != STVO_RECT_FORM_RADTAN && c->form != STVO_RECT_FORM_FISHEYE) return STVO_ERR_INVALID_ARG;
    const bool fisheye = c->form == STVO_RECT_FORM_FISHEYE;
    if (fisheye ? c->n_dist != 4 : (c->n_dist != 4 && c->n_dist != 5 && c->n_dist != 8)) return STVO_ERR_INVALID_ARG;
    // Kl / Kr are Mat_<float> (:55-56): rounded before anything reads them
    const double K1[4] = {f32(c->Kl[0]), f32(c->Kl[1]), f32(c->Kl[2]), f32(c->Kl[3])};
    const double K2[4] = {f32(c->Kr[0]), f32(c->Kr[1]), f32(c->Kr[2]), f32(c->Kr[3])};
    if (!(K1[0] > 0 && K1[1] > 0 && K2[0] > 0 && K2[1] > 0)) return STVO_ERR_INVALID_ARG;
    // the rectification is the rad-tan one for both forms: the fisheye form feeds its coefficients to it as k1 k2 p1 p2 (:82)
    const Dist d1 = radtan(c->Dl, c->n_dist), d2 = radtan(c->Dr, c->n_dist);
    stereo_rectify(K1, d1, K2, d2, w, h, c->R, c->t, out->R1, out->R2, out->P1, out->P2);
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(out->P1[k]) || !std::isfinite(out->P2[k])) return STVO_ERR_INVALID_ARG;
    out->dist = 1;
    out->cam = stvo_cam{out->P1[0], out->P1[5], out->P1[2], out->P1[6], c->b};  // :89-92; b = cam_bl
    for (int side = 0; side < 2; ++side) {
        if (!map1 && !map2) break;
        int16_t* m1 = map1 ? map1 + side * 2 * npx : new int16_t[2 * npx];
        uint16_t* m2 = map2 ? map2 + side * npx : new uint16_t[npx];
        const double* K = side ? K2 : K1;
        const double* R = side ? out->R2 : out->R1;
        const double* P = side ? out->P2 : out->P1;
        if (fisheye)
            map_fisheye(K, side ? c->Dr : c->Dl, R, P, w, h, m1, m2);
        else
            map_radtan(K, side ? d2 : d1, R, P, w, h, m1, m2);
        if (!map1) delete[] m1;
        if (!map2) delete[] m2;
    }
    return STVO_OK;
}
