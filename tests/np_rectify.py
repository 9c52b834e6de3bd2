"""Second statement of the stereo rectification (csrc/rectify_calib.cpp, csrc/rectify_kernels.hip) in Python / numpy.

Scalar calibration maths in Python floats (IEEE double, no fused multiply-add, the same libm), float32 steps through numpy float32
scalars; the maps vectorised with numpy in the C loop's order of operations (np.add.accumulate is sequential, so the per-pixel
`_x += ir[0]` accumulation is reproduced exactly).  The rotation that OpenCV orthogonalises with an SVD is orthogonalised here
with numpy's SVD (the library uses a Newton iteration to the same polar factor): R1, R2, P1, P2 agree to rounding, and the maps
are compared bit for bit when built from the SAME R / P (maps_from_camera).

Follows OpenCV 3.4's cvStereoRectify in the form DESIGN.md §9 states (k1-adjusted minimum of the focal lengths, `width` terms in
icvGetRectangles and in the alpha scale), initUndistortRectifyMap / fisheye::initUndistortRectifyMap, the CV_16SC2 encoding and
remapBilinear's fixed-point arithmetic."""
import math

import numpy as np

F32 = np.float32


def f32(v):
    return float(F32(v))


def mul3(a, b):
    return [[a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def mul3_bt(a, b):
    return [[a[i][0] * b[j][0] + a[i][1] * b[j][1] + a[i][2] * b[j][2] for j in range(3)] for i in range(3)]


def mulv(a, v):
    return [a[i][0] * v[0] + a[i][1] * v[1] + a[i][2] * v[2] for i in range(3)]


def norm3(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def inv3(S):
    """cv::invert(DECOMP_LU) for 3 x 3: the cofactor form."""
    d = (S[0][0] * (S[1][1] * S[2][2] - S[1][2] * S[2][1]) - S[0][1] * (S[1][0] * S[2][2] - S[1][2] * S[2][0]) +
         S[0][2] * (S[1][0] * S[2][1] - S[1][1] * S[2][0]))
    d = 1. / d
    t = [(S[1][1] * S[2][2] - S[1][2] * S[2][1]) * d, (S[0][2] * S[2][1] - S[0][1] * S[2][2]) * d, (S[0][1] * S[1][2] - S[0][2] * S[1][1]) * d,
         (S[1][2] * S[2][0] - S[1][0] * S[2][2]) * d, (S[0][0] * S[2][2] - S[0][2] * S[2][0]) * d, (S[0][2] * S[1][0] - S[0][0] * S[1][2]) * d,
         (S[1][0] * S[2][1] - S[1][1] * S[2][0]) * d, (S[0][1] * S[2][0] - S[0][0] * S[2][1]) * d, (S[0][0] * S[1][1] - S[0][1] * S[1][0]) * d]
    return [t[0:3], t[3:6], t[6:9]]


def rodrigues_v2m(r):
    theta = norm3(r)
    if theta < 2.220446049250313e-16:
        return [[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]
    c, s = math.cos(theta), math.sin(theta)
    c1, it = 1. - c, 1. / theta
    x, y, z = r[0] * it, r[1] * it, r[2] * it
    rrt = [[x * x, x * y, x * z], [x * y, y * y, y * z], [x * z, y * z, z * z]]
    rx = [[0, -z, y], [z, 0, -x], [-y, x, 0]]
    eye = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    return [[c * eye[i][j] + c1 * rrt[i][j] + s * rx[i][j] for j in range(3)] for i in range(3)]


def rodrigues_m2v(R):
    U, _, Vt = np.linalg.svd(np.array(R, np.float64))
    R = (U @ Vt).tolist()
    r = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    s = math.sqrt((r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * 0.25)
    c = min(1., max(-1., (R[0][0] + R[1][1] + R[2][2] - 1) * 0.5))
    theta = math.acos(c)
    if s < 1e-5:
        if c > 0:
            return [0., 0., 0.]
        rx = math.sqrt(max((R[0][0] + 1) * 0.5, 0.))
        ry = math.sqrt(max((R[1][1] + 1) * 0.5, 0.)) * (-1. if R[0][1] < 0 else 1.)
        rz = math.sqrt(max((R[2][2] + 1) * 0.5, 0.)) * (-1. if R[0][2] < 0 else 1.)
        if abs(rx) < abs(ry) and abs(rx) < abs(rz) and (R[1][2] > 0) != (ry * rz > 0):
            rz = -rz
        theta /= norm3([rx, ry, rz])
        return [rx * theta, ry * theta, rz * theta]
    vth = 1 / (2 * s) * theta
    return [r[0] * vth, r[1] * vth, r[2] * vth]


def dist12(D):
    k = [0.] * 12
    for i, v in enumerate(list(D)[:8]):
        k[i] = float(v)
    return k


def undistort_points(pts, K, k, RR):
    """cvUndistortPoints on float32 points, 5 iterations; K = (fx, fy, cx, cy); -> list of float32-rounded (x, y)."""
    fx, fy, cx, cy = K
    ifx, ify = 1. / fx, 1. / fy
    out = []
    for px, py in pts:
        x, y = (float(px) - cx) * ifx, (float(py) - cy) * ify
        x0, y0 = x, y
        for _ in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
        xx = RR[0][0] * x + RR[0][1] * y + RR[0][2]
        yy = RR[1][0] * x + RR[1][1] * y + RR[1][2]
        ww = 1. / (RR[2][0] * x + RR[2][1] * y + RR[2][2])
        out.append((F32(xx * ww), F32(yy * ww)))
    return out


def get_rectangles(K, k, R, P, w, h):
    N = 9
    pts = [(F32(x) * F32(w) / F32(N - 1), F32(y) * F32(h) / F32(N - 1)) for y in range(N) for x in range(N)]
    RR = mul3([P[0][:3], P[1][:3], P[2][:3]], R)
    pts = undistort_points(pts, K, k, RR)
    a = np.array(pts, np.float32).reshape(N, N, 2)
    iX0, iX1 = a[:, 0, 0].max(), a[:, N - 1, 0].min()
    iY0, iY1 = a[0, :, 1].max(), a[N - 1, :, 1].min()
    oX0, oX1, oY0, oY1 = a[..., 0].min(), a[..., 0].max(), a[..., 1].min(), a[..., 1].max()
    return (iX0, iY0, F32(iX1 - iX0), F32(iY1 - iY0)), (oX0, oY0, F32(oX1 - oX0), F32(oY1 - oY0))


def stereo_rectify(K1, D1, K2, D2, w, h, R, T):
    """cvStereoRectify(CALIB_ZERO_DISPARITY, alpha = 0) -> R1, R2 (3x3 lists), P1, P2 (3x4 lists)."""
    nx, ny = float(w), float(h)
    k1, k2 = dist12(D1), dist12(D2)
    om = [v * -0.5 for v in rodrigues_m2v(R)]
    r_r = rodrigues_v2m(om)
    t = mulv(r_r, T)
    idx = 0 if abs(t[0]) > abs(t[1]) else 1
    c, nt = t[idx], norm3(t)
    uu = [0., 0., 0.]
    uu[idx] = 1. if c > 0 else -1.
    ww = [t[1] * uu[2] - t[2] * uu[1], t[2] * uu[0] - t[0] * uu[2], t[0] * uu[1] - t[1] * uu[0]]
    nw = norm3(ww)
    if nw > 0.0:
        sc = math.acos(abs(c) / nt) / nw
        ww = [v * sc for v in ww]
    wR = rodrigues_v2m(ww)
    R1, R2 = mul3_bt(wR, r_r), mul3(wR, r_r)
    t = mulv(R2, T)
    fc_new = float("inf")
    for A, k in ((K1, k1), (K2, k2)):
        fc = A[idx ^ 1]
        if k[0] < 0:
            fc *= 1 + k[0] * (nx * nx + ny * ny) / (4 * fc * fc)
        fc_new = min(fc_new, fc)
    cc = []
    for A, k, Rk in ((K1, k1, R1), (K2, k2, R2)):
        corners = [(F32((i % 2) * (nx - 1)), F32((0 if i < 2 else 1) * (ny - 1))) for i in range(4)]
        und = undistort_points(corners, A, k, [[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]])
        sx = sy = 0.
        for X, Y in und:
            X, Y, Z = float(X), float(Y), 1.0
            x = Rk[0][0] * X + Rk[0][1] * Y + Rk[0][2] * Z + 0.0
            y = Rk[1][0] * X + Rk[1][1] * Y + Rk[1][2] * Z + 0.0
            z = Rk[2][0] * X + Rk[2][1] * Y + Rk[2][2] * Z + 0.0
            z = 1. / z if z else 1.
            x *= z
            y *= z
            sx += f32(x * fc_new + 0.0)
            sy += f32(y * fc_new + 0.0)
        cc.append([(nx - 1) / 2 - sx * 0.25, (ny - 1) / 2 - sy * 0.25])
    ccx = (cc[0][0] + cc[1][0]) * 0.5
    ccy = (cc[0][1] + cc[1][1]) * 0.5
    P1 = [[fc_new, 0., ccx, 0.], [0., fc_new, ccy, 0.], [0., 0., 1., 0.]]
    P2 = [row[:] for row in P1]
    P2[idx][3] = t[idx] * fc_new
    in1, out1 = get_rectangles(K1, k1, R1, P1, w, h)
    in2, out2 = get_rectangles(K2, k2, R2, P2, w, h)
    cx1 = w * ccx / w
    cy1 = h * ccy / h
    cx2, cy2 = cx1, cy1

    def terms(cxa, cya, cx0, cy0, r):
        return [cxa / (cx0 - float(r[0])), cya / (cy0 - float(r[1])), (w - cxa) / (float(F32(r[0] + r[2])) - cx0),
                (h - cya) / (float(F32(r[1] + r[3])) - cy0)]

    s0 = max(terms(cx1, cy1, ccx, ccy, in1) + terms(cx2, cy2, ccx, ccy, in2))
    s1 = min(terms(cx1, cy1, ccx, ccy, out1) + terms(cx2, cy2, ccx, ccy, out2))
    alpha = 0.0
    s = s0 * (1 - alpha) + s1 * alpha
    fc_new *= s
    for P in (P1, P2):
        P[0][0] = P[1][1] = fc_new
        P[0][2], P[1][2] = cx1, cy1
    P2[idx][3] = s * P2[idx][3]
    return R1, R2, P1, P2


def rectify_calib(c):
    """A capi.RectCalib (or anything with its fields) -> dict(R1, R2, P1, P2 as numpy arrays, cam, dist)."""
    eye = [[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]
    if c.form == 0:
        fx, fy = abs(c.fx), abs(c.fy)
        P = [[f32(fx), 0., f32(c.cx), 0.], [0., f32(fx), f32(c.cy), 0.], [0., 0., 1., 0.]]
        return dict(R1=np.array(eye), R2=np.array(eye), P1=np.array(P), P2=np.array(P), dist=int(c.d[0] != 0.0),
                    cam=dict(fx=fx, fy=fy, cx=c.cx, cy=c.cy, b=c.b))
    K1 = [f32(v) for v in c.Kl[:4]]
    K2 = [f32(v) for v in c.Kr[:4]]
    nd = c.n_dist
    R = [list(c.R[0:3]), list(c.R[3:6]), list(c.R[6:9])]
    R1, R2, P1, P2 = stereo_rectify(K1, list(c.Dl[:nd]), K2, list(c.Dr[:nd]), c.width, c.height, R, list(c.t[:3]))
    return dict(R1=np.array(R1), R2=np.array(R2), P1=np.array(P1), P2=np.array(P2), dist=1,
                cam=dict(fx=P1[0][0], fy=P1[1][1], cx=P1[0][2], cy=P1[1][2], b=c.b))


# ---- maps -----------------------------------------------------------------------------------------------------------------------

def _ir(P, R):
    return inv3(mul3([list(P[0][:3]), list(P[1][:3]), list(P[2][:3])], [list(r) for r in R]))


def _accumulate(w, h, a0, a1, a2):
    """_x of pixel (i, j): i * a1 + a2, then j additions of a0 — sequentially, as the C loop does."""
    start = np.arange(h, dtype=np.float64) * a1 + a2
    steps = np.empty((h, w), np.float64)
    steps[:, 0] = start
    steps[:, 1:] = a0
    return np.add.accumulate(steps, axis=1)


def encode(u, v):
    """CV_16SC2: cvRound(u * 32) (half to even) -> (iu >> 5, iv >> 5) int16 and (iv & 31) * 32 + (iu & 31) uint16."""
    def rnd(a):
        a = a * 32
        out = np.empty(a.shape, np.int64)
        bad = ~(a > -2147483648.0)
        big = a > 2147483647.0
        ok = ~bad & ~big
        out[ok] = np.rint(a[ok]).astype(np.int64)
        out[bad] = -2147483648
        out[big] = 2147483647
        return out
    iu, iv = rnd(u), rnd(v)
    m1 = np.stack([(iu >> 5).astype(np.int16), (iv >> 5).astype(np.int16)], axis=-1)
    m2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return m1, m2


def map_radtan(K, D, R, P, w, h):
    ir = _ir(P, R)
    _x = _accumulate(w, h, ir[0][0], ir[0][1], ir[0][2])
    _y = _accumulate(w, h, ir[1][0], ir[1][1], ir[1][2])
    _w = _accumulate(w, h, ir[2][0], ir[2][1], ir[2][2])
    k = dist12(D)
    k1, k2, p1, p2, k3, k4, k5, k6 = k[:8]
    fx, fy, u0, v0 = K
    ww = 1. / _w
    x, y = _x * ww, _y * ww
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
    yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
    return encode(fx * xd + u0, fy * yd + v0)


def map_fisheye(K, D, R, P, w, h):
    iR = _ir(P, R)
    _x = _accumulate(w, h, iR[0][0], iR[0][1], iR[0][2])
    _y = _accumulate(w, h, iR[1][0], iR[1][1], iR[1][2])
    _w = _accumulate(w, h, iR[2][0], iR[2][1], iR[2][2])
    f0, f1, c0, c1 = K
    d = [float(v) for v in D[:4]]
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y = _x / _w, _y / _w
        r = np.sqrt(x * x + y * y)
        theta = np.arctan(r)
        t2 = theta * theta
        t4 = t2 * t2
        t6, t8 = t4 * t2, t4 * t4
        theta_d = theta * (1 + d[0] * t2 + d[1] * t4 + d[2] * t6 + d[3] * t8)
        scale = np.where(r == 0, 1.0, theta_d / r)
        u = f0 * x * scale + c0
        v = f1 * y * scale + c1
    neg = _w <= 0
    u = np.where(neg, np.where(_x > 0, -np.inf, np.inf), u)
    v = np.where(neg, np.where(_y > 0, -np.inf, np.inf), v)
    return encode(u, v)


def maps_from_camera(c, cam):
    """The maps of both sides built from the camera `cam` (R1, R2, P1, P2 — e.g. the library's own) and the calibration c."""
    w, h = c.width, c.height
    if c.form == 0:
        K = [f32(abs(c.fx)), f32(abs(c.fy)), f32(c.cx), f32(c.cy)]
        D = [f32(v) for v in c.d[:4]] + [0.0]
        m1, m2 = map_radtan(K, D, np.eye(3), cam["P1"], w, h)
        return np.stack([m1, m1]), np.stack([m2, m2])
    out1, out2 = [], []
    for side in range(2):
        K = [f32(v) for v in (c.Kr if side else c.Kl)[:4]]
        D = list((c.Dr if side else c.Dl)[:c.n_dist])
        R, P = cam["R2" if side else "R1"], cam["P2" if side else "P1"]
        m1, m2 = (map_fisheye if c.form == 2 else map_radtan)(K, D, R, P, w, h)
        out1.append(m1)
        out2.append(m2)
    return np.stack(out1), np.stack(out2)


def map_coords(map1, map2):
    """Source coordinates (float64) a CV_16SC2 map encodes: (x + ax / 32, y + ay / 32)."""
    return (map1[..., 0].astype(np.float64) + (map2 & 31) / 32.0, map1[..., 1].astype(np.float64) + ((map2 >> 5) & 31) / 32.0)


# ---- remap ----------------------------------------------------------------------------------------------------------------------

def remap(img, map1, map2):
    """cv::remap(img, map1, map2, INTER_LINEAR, BORDER_CONSTANT 0) for 8-bit images [rows, cols] (or [n, rows, cols])."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 3:
        return np.stack([remap(im, map1, map2) for im in img])
    rows, cols = img.shape
    x = map1[..., 0].astype(np.int64)
    y = map1[..., 1].astype(np.int64)
    ax = (map2 & 31).astype(np.int64)
    ay = ((map2 >> 5) & 31).astype(np.int64)

    def tap(xx, yy):
        ok = (xx >= 0) & (xx < cols) & (yy >= 0) & (yy < rows)
        return np.where(ok, img[np.clip(yy, 0, rows - 1), np.clip(xx, 0, cols - 1)].astype(np.int64), 0)

    w00, w01 = (32 - ax) * (32 - ay) * 32, ax * (32 - ay) * 32
    w10, w11 = (32 - ax) * ay * 32, ax * ay * 32
    acc = tap(x, y) * w00 + tap(x + 1, y) * w01 + tap(x, y + 1) * w10 + tap(x + 1, y + 1) * w11
    return ((acc + 16384) >> 15).astype(np.uint8)
