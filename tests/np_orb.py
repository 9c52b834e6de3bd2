"""The ORB point front-end as ONE plain numpy statement — TEST INFRASTRUCTURE ONLY.

Written from the published algorithm (the numbered list at the top of oracle/stvo_orb_oracle.c names the OpenCV routines), not from
the oracle's loops and not from the kernels: whole-image array expressions, integers in int64, floating point in np.float32 one
operation at a time (a numpy float32 array operation rounds once per element, like a C float expression without contraction).

    detect_levels(img, ...) -> dict(kp, response, angle, desc, octave, n_total, trace)

`trace` is what the planned cases (tests/orb_edge_cases.py) compute their "this input really sits on the edge" facts from:
    trace["levels"][l] = dict(scale, cols, rows, budget, image, score, blur, n)      (score / blur: None for a level that yields nothing)
    trace["m01"], trace["m10"]   int64 [n]       the intensity-centroid moments of every key-point
    trace["rot"]                 int64 [n, 256, 4]  the rotated test coordinates (x0, y0, x1, y1) of every key-point
    trace["level_xy"]            int64 [n, 2]    the key-point in pixels of ITS level
"""
import math

import numpy as np

F = np.float32
HALF_PATCH = 15
# Bresenham circle of radius 3 in OpenCV's order (dx, dy): index 0 is straight below, 4 right, 8 above, 12 left
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3))


def cv_round(v):
    """cvRound: to the nearest integer, halves to the even one."""
    return np.rint(v).astype(np.int64)


def ring_differences(img):
    """[16, rows - 6, cols - 6] int64: ring pixel minus centre for every pixel that has its whole ring inside the image."""
    I = np.asarray(img).astype(np.int64)
    rows, cols = I.shape
    c = I[3:rows - 3, 3:cols - 3]
    return np.stack([I[3 + dy:rows - 3 + dy, 3 + dx:cols - 3 + dx] - c for dx, dy in CIRCLE])


def fast_side_scores(img):
    """(bright, dark) int64 [rows, cols]: per pixel the largest t >= 0 at which 9 contiguous ring pixels are all > I + t (bright) or
    all < I - t (dark); -1 where there is no such t (and on the 3-pixel rim, where the ring leaves the image).
    An arc is "all > I + t" exactly for t <= (smallest difference of the arc) - 1, so the largest t over the 16 arcs is the largest
    arc minimum, minus 1."""
    rows, cols = np.asarray(img).shape
    bright = np.full((rows, cols), -1, np.int64)
    dark = np.full((rows, cols), -1, np.int64)
    if rows < 7 or cols < 7:
        return bright, dark
    d = ring_differences(img)
    best_b = np.full(d.shape[1:], -255, np.int64)
    best_d = np.full(d.shape[1:], -255, np.int64)
    for k in range(16):                                        # arc k = ring pixels k .. k + 8
        arc = d[[(k + j) % 16 for j in range(9)]]
        best_b = np.maximum(best_b, arc.min(axis=0))           # its weakest member on the bright side
        best_d = np.maximum(best_d, (-arc).min(axis=0))        # ... and on the dark side
    bright[3:rows - 3, 3:cols - 3] = np.maximum(best_b - 1, -1)
    dark[3:rows - 3, 3:cols - 3] = np.maximum(best_d - 1, -1)
    return bright, dark


def fast_score_image(img, threshold):
    """The FAST-9/16 score of every corner at `threshold` (>= 1), 0 elsewhere."""
    b, d = fast_side_scores(img)
    s = np.maximum(b, d)
    return np.where(s >= threshold, s, 0)


def strict_maxima(score):
    """Corners whose score is strictly greater than the scores of all 8 neighbours (non-corners count as 0)."""
    rows, cols = score.shape
    p = np.pad(score, 1, constant_values=0)
    keep = score > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= score > p[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols]
    return keep


def inside_border(shape, edge):
    """KeyPointsFilter::runByImageBorder: x in [edge, cols - edge), y in [edge, rows - edge)."""
    rows, cols = shape
    yy, xx = np.mgrid[0:rows, 0:cols]
    return (xx >= edge) & (xx < cols - edge) & (yy >= edge) & (yy < rows - edge)


def retain_best(responses, n):
    """KeyPointsFilter::retainBest: boolean mask of the key-points whose response is >= the n-th largest (ties at the cut all stay)."""
    responses = np.asarray(responses)
    if n <= 0:
        return np.zeros(len(responses), bool)
    if len(responses) <= n:
        return np.ones(len(responses), bool)
    return responses >= np.sort(responses)[::-1][n - 1]


def umax_table():
    """ORB's umax: the half-width of the circular patch in row |v| (quarter circle by rounding, made symmetric about the diagonal)."""
    hp = HALF_PATCH
    vmax, vmin = int(math.floor(hp * math.sqrt(2.0) / 2 + 1)), int(math.ceil(hp * math.sqrt(2.0) / 2))
    u = [0] * (hp + 2)
    for v in range(vmax + 1):
        u[v] = int(cv_round(math.sqrt(float(hp * hp - v * v))))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return np.array(u[:hp + 1], np.int64)


def disc_mask():
    """[31, 31] bool: the circular patch, mask[v + 15, u + 15] = |u| <= umax[|v|]."""
    um = umax_table()
    r = np.arange(-HALF_PATCH, HALF_PATCH + 1)
    return np.abs(r)[None, :] <= um[np.abs(r)][:, None]


def moments(img, xy):
    """(m01, m10) int64 [n]: sum of v I and of u I over the circular patch around every (x, y)."""
    I = np.asarray(img).astype(np.int64)
    r = np.arange(-HALF_PATCH, HALF_PATCH + 1)
    mask = disc_mask().astype(np.int64)
    m01, m10 = np.zeros(len(xy), np.int64), np.zeros(len(xy), np.int64)
    for i, (x, y) in enumerate(xy):
        P = I[y - HALF_PATCH:y + HALF_PATCH + 1, x - HALF_PATCH:x + HALF_PATCH + 1] * mask
        m01[i] = (P.sum(axis=1) * r).sum()
        m10[i] = (P.sum(axis=0) * r).sum()
    return m01, m10


def fast_atan2(y, x):
    """cv::fastAtan2 in degrees: float32, a 7th-order odd polynomial on [0, 1] and octant folding, one rounding per operation."""
    y, x = np.asarray(y, F), np.asarray(x, F)
    scale = F(180.0 / math.pi)
    p1, p3, p5, p7 = F(0.9997878412794807) * scale, F(-0.3258083974640975) * scale, F(0.1555786518463281) * scale, F(-0.04432655554792128) * scale
    ax, ay = np.abs(x), np.abs(y)
    eps = F(2.2204460492503131e-16)
    x_major = ax >= ay
    c = np.where(x_major, ay, ax) / (np.where(x_major, ax, ay) + eps)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(x_major, a, F(90.0) - a)
    a = np.where(x < 0, F(180.0) - a, a)
    a = np.where(y < 0, F(360.0) - a, a)
    return a.astype(F)


def gaussian_blur7(img):
    """GaussianBlur(7 x 7, sigma 2, BORDER_REFLECT_101) in 8-bit fixed point: weights * 2^8 rounded, two integer passes, one rounding
    shift by 16."""
    I = np.asarray(img).astype(np.int64)
    rows, cols = I.shape
    k = np.exp(-(np.arange(7) - 3.0) ** 2 / (2.0 * 2.0 * 2.0))
    ki = cv_round((k / k.sum()).astype(F).astype(np.float64) * 256.0)

    def reflect(p, n):   # BORDER_REFLECT_101 for any n >= 2 (numpy's pad refuses a pad wider than the array)
        p = np.abs(p) % (2 * n - 2)
        return np.where(p >= n, 2 * n - 2 - p, p)
    cx = reflect(np.arange(-3, cols + 3), cols)
    ry = reflect(np.arange(-3, rows + 3), rows)
    h = sum(ki[i] * I[:, cx[i:i + cols]] for i in range(7))
    v = sum(ki[i] * h[ry[i:i + rows], :] for i in range(7))
    return np.clip((v + (1 << 15)) >> 16, 0, 255).astype(np.uint8)


def rotated_pattern(pattern, angle_deg):
    """[n, 256, 4] int64: the pattern's (x0, y0, x1, y1) rotated by every angle — a = (float)cos, b = (float)sin of the float radians in
    double precision, x' = cvRound(x a - y b), y' = cvRound(x b + y a) with float32 products and a float32 sum."""
    pat = np.asarray(pattern, np.int8).reshape(256, 4).astype(F)
    rad = np.asarray(angle_deg, F) * F(math.pi / 180.0)
    a = np.array([math.cos(float(r)) for r in rad], np.float64).astype(F)[:, None]
    b = np.array([math.sin(float(r)) for r in rad], np.float64).astype(F)[:, None]
    out = np.zeros((len(rad), 256, 4), np.int64)
    for j in (0, 2):
        px, py = pat[None, :, j], pat[None, :, j + 1]
        out[:, :, j] = cv_round(px * a - py * b)
        out[:, :, j + 1] = cv_round(px * b + py * a)
    return out


def resize_linear(src, dcols, drows):
    """resize(src, dst, Size(dcols, drows), 0, 0, INTER_LINEAR) for 8-bit images: sample position (d + 0.5) / inv_scale - 0.5 in double,
    rounded to float; weights cvRound((1 - f) 2048), cvRound(f 2048); horizontal pass exact in integers; rows combined as
    (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2."""
    S = np.asarray(src).astype(np.int64)
    srows, scols = S.shape

    def taps(dn, sn, clamp_weight):
        scale = 1.0 / (float(dn) / float(sn))
        f = ((np.arange(dn) + 0.5) * scale - 0.5).astype(F)
        s = np.floor(f).astype(np.int64)
        f = f - s.astype(F)
        if clamp_weight:   # columns: a position outside the row takes the border pixel alone
            f = np.where((s < 0) | (s >= sn - 1), F(0), f)
            s = np.clip(s, 0, sn - 1)
        w0, w1 = cv_round((F(1) - f) * F(2048)), cv_round(f * F(2048))
        return np.clip(s, 0, sn - 1), np.clip(s + 1, 0, sn - 1), w0, w1   # rows: the row index alone is clipped, the weights stay
    x0, x1, a0, a1 = taps(dcols, scols, True)
    y0, y1, b0, b1 = taps(drows, srows, False)
    H = S[:, x0] * a0[None, :] + S[:, x1] * a1[None, :]
    v = (((b0[:, None] * (H[y0] >> 4)) >> 16) + ((b1[:, None] * (H[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def levels(cols, rows, nfeatures, nlevels, scale_factor):
    """ORB_Impl's level geometry and budgets: scale_l = (float)pow(f, l); size = cvRound(size / scale_l) in float; budget
    n_l = cvRound(nfeatures (1 - q) / (1 - q^nlevels) q^l) with float q = 1 / f, accumulated by n *= q; the last level takes the rest."""
    scale = [F(math.pow(scale_factor, l)) for l in range(nlevels)]
    lc = [int(cv_round(F(cols) / s)) for s in scale]
    lr = [int(cv_round(F(rows) / s)) for s in scale]
    q = F(1.0 / scale_factor)
    nd = F(nfeatures) * (F(1) - q) / (F(1) - F(math.pow(float(q), float(nlevels))))
    nf, total = [], 0
    for _ in range(nlevels - 1):
        nf.append(int(cv_round(nd)))
        total += nf[-1]
        nd = nd * q
    nf.append(max(nfeatures - total, 0))
    return scale, lc, lr, nf


def detect_level(img, nfeatures, fast_th, edge_th, pattern):
    """Steps 1-6 on one level image.  Key-points in row-major order, uncapped."""
    img = np.asarray(img, np.uint8)
    score = fast_score_image(img, fast_th)
    kp_mask = strict_maxima(score) & inside_border(img.shape, edge_th)
    ys, xs = np.nonzero(kp_mask)                               # row-major
    keep = retain_best(score[ys, xs], nfeatures)
    xy = np.stack([xs[keep], ys[keep]], axis=1).astype(np.int64).reshape(-1, 2)
    resp = score[xy[:, 1], xy[:, 0]].astype(F)
    m01, m10 = moments(img, xy)
    ang = fast_atan2(m01.astype(F), m10.astype(F)).reshape(-1)
    blur = gaussian_blur7(img)
    rot = rotated_pattern(pattern, ang)
    B = blur.astype(np.int64)
    t0 = B[xy[:, 1:2] + rot[:, :, 1], xy[:, 0:1] + rot[:, :, 0]]
    t1 = B[xy[:, 1:2] + rot[:, :, 3], xy[:, 0:1] + rot[:, :, 2]]
    desc = np.packbits((t0 < t1).astype(np.uint8), axis=1, bitorder="little").reshape(-1, 32)
    return dict(xy=xy, response=resp, angle=ang, desc=desc, m01=m01, m10=m10, rot=rot, score=score, blur=blur)


def detect_levels(img, nfeatures=2000, nlevels=1, scale_factor=1.2, fast_th=20, edge_th=19, pattern=None, cap=4096):
    assert pattern is not None and edge_th >= 19 and 1 <= fast_th <= 254
    img = np.ascontiguousarray(img, np.uint8)
    rows, cols = img.shape
    scale, lc, lr, nf = levels(cols, rows, nfeatures, nlevels, scale_factor)
    out = dict(kp=[], response=[], angle=[], desc=[], octave=[])
    tr = dict(levels=[], m01=[], m10=[], rot=[], level_xy=[])
    cur, n, n_total = img, 0, 0
    for l in range(nlevels):
        if l:
            cur = resize_linear(cur, lc[l], lr[l])
        info = dict(scale=scale[l], cols=lc[l], rows=lr[l], budget=nf[l], image=cur, score=None, blur=None, n=0)
        # a level with no budget keeps nothing (retainBest(0)); one not larger than twice the border has no admissible pixel
        if nf[l] > 0 and 2 * edge_th < lc[l] and 2 * edge_th < lr[l]:
            r = detect_level(cur, nf[l], fast_th, edge_th, pattern)
            n_total += len(r["xy"])
            take = max(min(len(r["xy"]), cap - n), 0)
            pt = r["xy"][:take].astype(F)
            out["kp"].append(pt * scale[l] if l else pt)      # pt *= scale
            out["response"].append(r["response"][:take]); out["angle"].append(r["angle"][:take]); out["desc"].append(r["desc"][:take])
            out["octave"].append(np.full(take, l, np.int32))
            tr["m01"].append(r["m01"][:take]); tr["m10"].append(r["m10"][:take]); tr["rot"].append(r["rot"][:take])
            tr["level_xy"].append(r["xy"][:take])
            info.update(score=r["score"], blur=r["blur"], n=take)
            n += take
        tr["levels"].append(info)

    def cat(parts, shape, dtype):
        return np.concatenate(parts).astype(dtype) if parts else np.zeros(shape, dtype)
    res = dict(kp=cat(out["kp"], (0, 2), F), response=cat(out["response"], (0,), F), angle=cat(out["angle"], (0,), F),
               desc=cat(out["desc"], (0, 32), np.uint8), octave=cat(out["octave"], (0,), np.int32), n_total=n_total)
    res["trace"] = dict(levels=tr["levels"], m01=cat(tr["m01"], (0,), np.int64), m10=cat(tr["m10"], (0,), np.int64),
                        rot=cat(tr["rot"], (0, 256, 4), np.int64), level_xy=cat(tr["level_xy"], (0, 2), np.int64))
    return res
