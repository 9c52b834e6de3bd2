"""One optimizeFunctions[Robust] evaluation in extended precision — TEST INFRASTRUCTURE ONLY.

The judge of the per-feature terms: written from the reference's formulas (src/stereoFrameHandler.cpp:549-962,
src/stereoFrame.cpp:510-616, src/pinholeStereoCamera.cpp:231-237), one feature after the other, in numpy.longdouble
(x87 80-bit: 64 mantissa bits, eps 1.08e-19) — eleven more bits than any FP64 statement of the same sums, the oracle's
and the kernels' alike.  Every input is a double and converts exactly; every max / min is the reference's std::max /
std::min (a comparison, so a NaN operand falls where it falls there).

The robust scales follow the reference's own precision: vector_stdv_mad truncates the deviations to float, so the
residual norms are computed here in extended precision, rounded to double and handed to np_model.stdv_mad (equal to the
oracle's, tests/test_oracle_optimizer.py) and the [1e-4, sqrt(7.815)] clamp of :744-745."""
import numpy as np

import np_model

LD = np.longdouble
if np.finfo(LD).eps < 1e-18:
    BACKEND = "longdouble"
    _sqrt = np.sqrt
else:  # a platform whose long double is a double: 40 decimal digits through mpmath
    import mpmath
    mpmath.mp.dps = 40
    BACKEND = "mpmath"
    LD = mpmath.mpf
    _sqrt = mpmath.sqrt


def _x(v):
    return LD(float(v))


def _max(a, b):   # std::max(a, b)
    return b if a < b else a


def _min(a, b):   # std::min(a, b)
    return a if not (b < a) else b


def _div(a, b):
    """IEEE division (mpmath raises on a zero divisor; longdouble follows the hardware)."""
    if BACKEND == "longdouble":
        return a / b
    if b == 0:   # (mpf has no signed zero: the divisor counts as +0)
        return LD("nan") if (a == 0 or a != a) else (LD("inf") if a > 0 else LD("-inf"))
    return a / b


def _project(DT, cam, P):
    g = [DT[i][0] * P[0] + DT[i][1] * P[1] + DT[i][2] * P[2] + DT[i][3] for i in range(3)]
    uv = (cam["cx"] + _div(cam["fx"] * g[0], g[2]), cam["cy"] + _div(cam["fy"] * g[1], g[2]))
    return g, uv


def _grad(g, dx, dy, fx, hth):
    gx, gy, gz = g
    f = fx / _max(hth, gz * gz)
    return [+f * dx * gz, +f * dy * gz, -f * (gx * dx + gy * dy), -f * (gx * gy * dx + gy * gy * dy + gz * gz * dy),
            +f * (gx * gx * dx + gz * gz * dx + gx * gy * dy), +f * (gx * gz * dy - gy * gz * dx)]


def _from_lambdas(ls, le):
    lmin, lmax = _min(ls, le), _max(ls, le)
    if lmin < 0 and lmax > 1:
        return LD(1)
    if lmax < 0 or lmin > 1:
        return LD(0)
    if lmin < 0:
        return lmax
    if lmax > 1:
        return 1 - lmin
    return lmax - lmin


def line_overlap(so, eo, sp, ep):
    """StereoFrame::lineSegmentOverlap: observed segment (so, eo), projected end points (sp, ep)."""
    lx, ly = eo[0] - so[0], eo[1] - so[1]
    if abs(so[0] - eo[0]) < 1:
        return _from_lambdas(_div(sp[1] - so[1], ly), _div(ep[1] - so[1], ly))
    if abs(so[1] - eo[1]) < 1:
        return _from_lambdas(_div(sp[0] - so[0], lx), _div(ep[0] - so[0], lx))
    a, b, c = so[1] - eo[1], eo[0] - so[0], so[0] * eo[1] - eo[0] * so[1]
    lxy = 1 / (a * a + b * b)
    fs = (b * (b * sp[0] - a * sp[1]) - a * c) * lxy
    fe = (b * (b * ep[0] - a * ep[1]) - a * c) * lxy
    return _from_lambdas(_div(fs - so[0], lx), _div(fe - so[0], lx))


def _conv(a):
    a = np.asarray(a, np.float64)
    return [[_x(v) for v in row] for row in a.reshape(len(a), a.size // max(len(a), 1))]


def evaluate(DT, cam, homog_th, rec, robust=False):
    """H [6, 6], g [6], e / n, n of one evaluation, as longdouble (or mpf) objects in numpy object / longdouble arrays,
    plus the two robust scales used (doubles; 1.0 when not robust)."""
    T = _conv(np.asarray(DT, np.float64).reshape(4, 4))
    c = {k: _x(cam[k]) for k in ("fx", "fy", "cx", "cy")}
    hth = _x(homog_th)
    ip = np.asarray(rec["inlier_p"]) > 0
    il = np.asarray(rec["inlier_l"]) > 0
    P, obs, s2p = _conv(rec["P"]), _conv(rec["pl_obs"]), [_x(v) for v in rec["sigma2p"]]
    sP, eP, le = _conv(rec["sP"]), _conv(rec["eP"]), _conv(rec["le_obs"])
    spl, epl, s2l = _conv(rec["spl"]), _conv(rec["epl"]), [_x(v) for v in rec["sigma2l"]]
    with np.errstate(all="ignore"):
        pts, lns = [], []
        for i in np.nonzero(ip)[0]:
            g, uv = _project(T, c, P[i])
            dx, dy = uv[0] - obs[i][0], uv[1] - obs[i][1]
            pts.append((i, g, dx, dy, _sqrt(dx * dx + dy * dy)))
        for i in np.nonzero(il)[0]:
            gs, s = _project(T, c, sP[i])
            ge, t = _project(T, c, eP[i])
            ds = le[i][0] * s[0] + le[i][1] * s[1] + le[i][2]
            de = le[i][0] * t[0] + le[i][1] * t[1] + le[i][2]
            lns.append((i, gs, ge, s, t, ds, de, _sqrt(ds * ds + de * de)))
        s_p = s_l = 1.0
        if robust:
            clamp = lambda s: min(max(s, 1e-4), float(np.sqrt(7.815)))
            s_p = clamp(np_model.stdv_mad(np.array([float(p[4]) for p in pts])))
            s_l = clamp(np_model.stdv_mad(np.array([float(q[7]) for q in lns])))
        H = [[LD(0)] * 6 for _ in range(6)]
        gv = [LD(0)] * 6
        e = LD(0)

        def add(J, r, w):
            nonlocal e
            for a in range(6):
                for b in range(6):
                    H[a][b] = H[a][b] + J[a] * J[b] * w
                gv[a] = gv[a] + J[a] * r * w
            e = e + r * r * w

        for i, g, dx, dy, nrm in pts:
            den = _max(hth, nrm)
            J = [v / den for v in _grad(g, dx, dy, c["fx"], hth)]
            if robust:
                r = nrm
                xx = r / _x(s_p)
            else:
                r = nrm * _sqrt(s2p[i])
                xx = r
            add(J, r, 1 / (1 + xx * xx))
        for i, gs, ge, s, t, ds, de, nrm in lns:
            Js = _grad(gs, le[i][0], le[i][1], c["fx"], hth)
            Je = _grad(ge, le[i][0], le[i][1], c["fx"], hth)
            den = _max(hth, nrm)
            J = [(a * ds + b * de) / den for a, b in zip(Js, Je)]
            if robust:
                r = nrm
                xx = r / _x(s_l)
            else:
                r = nrm * _sqrt(s2l[i])
                xx = r
            w = 1 / (1 + xx * xx)
            add(J, r, w * line_overlap(spl[i], epl[i], s, t))
        n = len(pts) + len(lns)
        e = _div(e, LD(n))
    dt = np.longdouble if BACKEND == "longdouble" else object
    return np.array(H, dtype=dt), np.array(gv, dtype=dt), e, n, s_p, s_l


def deviation(H, g, e, xH, xg, xe):
    """(max|dH| / max|H|, max|dg| / max|g|, |de| / |e|) of a double result from the extended one; an exactly equal entry
    deviates by 0 (so an all-zero H compares), anything non-finite on either side by inf."""
    def rel(a, x):
        a = np.asarray(a, np.float64).reshape(-1)
        x = np.asarray(x).reshape(-1)
        xf = np.array([float(v) for v in x])
        if not (np.all(np.isfinite(a)) and np.all(np.isfinite(xf))):
            return np.inf
        d = max(abs(_x(p) - q) for p, q in zip(a, x))
        if d == 0:
            return 0.0
        return float(d / max(abs(q) for q in x))
    return rel(H, xH), rel(g, xg), rel([e], [xe])
