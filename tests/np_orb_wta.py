"""The ORB descriptor for every orb_wta_k (2, 3, 4) and orb_patch_size (2 .. 63) as a plain numpy statement — TEST INFRASTRUCTURE ONLY.

Written from the published algorithm (OpenCV 3's features2d/src/orb.cpp: makeRandomPattern, initializeOrbPattern, ICAngles,
computeOrbDescriptors; core's RNG), not from csrc/orb_pattern.h and not from the kernels.  What does not depend on either value —
FAST, the suppression, the border filter, retainBest, the blur, the pyramid, fastAtan2, the rotation of a point — is imported from
tests/np_orb.py unchanged.

    detect_levels(img, ..., pool=..., wta_k=2, patch_size=31) -> the dict of np_orb.detect_levels; trace["rot"] is [n, points, 2]
        (the rotated effective pattern, x then y), trace["tuples"] the blurred intensities [n, tuples, wta_k] the tests compared
"""
import math

import numpy as np

import np_harris
import np_orb
from np_orb import F, cv_round

M32 = 0xFFFFFFFF


class Rng:
    """cv::RNG: a 64-bit multiply-with-carry state whose low word is the draw."""

    def __init__(self, seed):
        self.state = seed if seed else M32

    def next(self):
        self.state = ((self.state & M32) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & M32

    def uniform(self, a, b):
        return a if a == b else self.next() % (b - a) + a


def random_pool(patch_size):
    """makeRandomPattern: 512 points (x, y), every coordinate uniform in [-P / 2, P / 2] (integer division), x drawn before y."""
    rng, h = Rng(0x34985739), patch_size // 2
    return np.array([[rng.uniform(-h, h + 1), rng.uniform(-h, h + 1)] for _ in range(512)], np.int64)


def effective_pattern(wta_k, patch_size, pool31=None):
    """[points, 2] int64: the point list the descriptor reads.  pool31 [512, 2] (or [256, 4]) is the pool of patch size 31."""
    assert wta_k in (2, 3, 4) and 2 <= patch_size <= 63
    pool = np.asarray(pool31, np.int64).reshape(512, 2) if patch_size == 31 else random_pool(patch_size)
    if wta_k == 2:
        return pool.copy()
    rng, out = Rng(0x12345678), []
    for _ in range(128):
        tup = []
        while len(tup) < wta_k:
            p = tuple(pool[rng.uniform(0, 512)])
            if p not in tup:                                   # equal points at different pool indices count as equal
                tup.append(p)
        out += tup
    return np.array(out, np.int64)


def reach(patch_size):
    """How far a rotated point of the pattern can lie from the key-point: what the border must leave free."""
    return 19 if patch_size == 31 else int(math.ceil((patch_size // 2) * math.sqrt(2.0)))


def umax_table(h):
    """ORB's umax for half patch h (np_orb.umax_table with h in place of 15): quarter circle by rounding, then the symmetry pass."""
    vmax, vmin = int(math.floor(h * math.sqrt(2.0) / 2 + 1)), int(math.ceil(h * math.sqrt(2.0) / 2))
    u = [0] * (h + 2)
    for v in range(vmax + 1):
        u[v] = int(cv_round(math.sqrt(float(h * h - v * v))))
    v0 = 0
    for v in range(h, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return np.array(u[:h + 1], np.int64)


def disc_mask(h):
    um = umax_table(h)
    r = np.arange(-h, h + 1)
    return np.abs(r)[None, :] <= um[np.abs(r)][:, None]


def moments(img, xy, h):
    """(m01, m10) int64 [n] on the disc of half patch h."""
    I = np.asarray(img).astype(np.int64)
    r = np.arange(-h, h + 1)
    mask = disc_mask(h).astype(np.int64)
    m01, m10 = np.zeros(len(xy), np.int64), np.zeros(len(xy), np.int64)
    for i, (x, y) in enumerate(xy):
        P = I[y - h:y + h + 1, x - h:x + h + 1] * mask
        m01[i] = (P.sum(axis=1) * r).sum()
        m10[i] = (P.sum(axis=0) * r).sum()
    return m01, m10


def rotated_points(points, angle_deg):
    """[n, points, 2] int64: every point rotated by every angle, with np_orb's arithmetic (float32 products and sum, cvRound)."""
    pts = np.asarray(points, np.int64).astype(F)
    rad = np.asarray(angle_deg, F) * F(math.pi / 180.0)
    a = np.array([math.cos(float(r)) for r in rad], np.float64).astype(F)[:, None]
    b = np.array([math.sin(float(r)) for r in rad], np.float64).astype(F)[:, None]
    px, py = pts[None, :, 0], pts[None, :, 1]
    return np.stack([cv_round(px * a - py * b), cv_round(px * b + py * a)], axis=2).reshape(len(rad), len(pts), 2)


def wta2_bits(t):
    """[n, 256, 2] intensities -> [n, 256] bits: t0 < t1."""
    return (t[..., 0] < t[..., 1]).astype(np.uint8)


def wta3_values(t):
    """[n, 128, 3] -> [n, 128] values 0 .. 2: t2 > t1 ? (t2 > t0 ? 2 : 0) : (t1 > t0)."""
    t0, t1, t2 = t[..., 0], t[..., 1], t[..., 2]
    return np.where(t2 > t1, np.where(t2 > t0, 2, 0), (t1 > t0).astype(np.int64)).astype(np.uint8)


def wta4_values(t):
    """[n, 128, 4] -> [n, 128] values 0 .. 3: the larger of (t0, t1) against the larger of (t2, t3), every comparison strict."""
    t0, t1, t2, t3 = t[..., 0], t[..., 1], t[..., 2], t[..., 3]
    a = (t1 > t0).astype(np.int64)
    u = np.where(t1 > t0, t1, t0)
    b = np.where(t3 > t2, 3, 2)
    v = np.where(t3 > t2, t3, t2)
    return np.where(u > v, a, b).astype(np.uint8)


def pack(values, bits_per_value):
    """[n, m] values of 1 or 2 bits -> [n, 32] bytes, the first value in the lowest bits of byte 0."""
    v = np.asarray(values, np.uint8)
    if bits_per_value == 1:
        return np.packbits(v, axis=1, bitorder="little").reshape(len(v), 32)
    bits = np.stack([v & 1, v >> 1], axis=2).reshape(len(v), 2 * v.shape[1])
    return np.packbits(bits, axis=1, bitorder="little").reshape(len(v), 32)


def describe(blur, xy, angle, points, wta_k):
    """(desc [n, 32], rot [n, points, 2], tuples [n, points / wta_k, wta_k])."""
    rot = rotated_points(points, angle)
    B = np.asarray(blur).astype(np.int64)
    t = B[xy[:, 1:2] + rot[:, :, 1], xy[:, 0:1] + rot[:, :, 0]].reshape(len(xy), len(points) // wta_k, wta_k)
    if wta_k == 2:
        desc = pack(wta2_bits(t), 1)
    else:
        desc = pack(wta3_values(t) if wta_k == 3 else wta4_values(t), 2)
    return desc.reshape(-1, 32), rot, t


def detect_level(img, nfeatures, fast_th, edge_th, points, wta_k, patch_size, score_type=1):
    """np_orb.detect_level with the orientation on the disc of patch_size // 2 and the descriptor of (wta_k, points).  score_type 0: the
    Harris ranking (tests/np_harris.py: retainBest(2 n) by FAST score, HarrisResponses, retainBest(n) on them)."""
    img = np.asarray(img, np.uint8)
    h = patch_size // 2
    score = np_orb.fast_score_image(img, fast_th)
    kp_mask = np_orb.strict_maxima(score) & np_orb.inside_border(img.shape, edge_th)
    ys, xs = np.nonzero(kp_mask)
    if score_type == 0:
        keep = np_orb.retain_best(score[ys, xs], 2 * nfeatures)
        xs, ys = xs[keep], ys[keep]
        hr = np_harris.responses(img, xs.astype(np.int64), ys.astype(np.int64))
        keep = np_orb.retain_best(hr, nfeatures)
        xy = np.stack([xs[keep], ys[keep]], axis=1).astype(np.int64).reshape(-1, 2)
        resp = hr[keep].astype(F)
    else:
        keep = np_orb.retain_best(score[ys, xs], nfeatures)
        xy = np.stack([xs[keep], ys[keep]], axis=1).astype(np.int64).reshape(-1, 2)
        resp = score[xy[:, 1], xy[:, 0]].astype(F)
    m01, m10 = moments(img, xy, h)
    ang = np_orb.fast_atan2(m01.astype(F), m10.astype(F)).reshape(-1)
    blur = np_orb.gaussian_blur7(img)
    desc, rot, tup = describe(blur, xy, ang, points, wta_k)
    return dict(xy=xy, response=resp, angle=ang, desc=desc, m01=m01, m10=m10, rot=rot, tuples=tup, score=score, blur=blur)


def detect_levels(img, nfeatures=2000, nlevels=1, scale_factor=1.2, fast_th=20, edge_th=19, pool=None, cap=4096, wta_k=2, patch_size=31,
                  score=1):
    assert edge_th >= 19 and 1 <= fast_th <= 254 and edge_th >= reach(patch_size)
    points = effective_pattern(wta_k, patch_size, pool)
    img = np.ascontiguousarray(img, np.uint8)
    rows, cols = img.shape
    scale, lc, lr, nf = np_orb.levels(cols, rows, nfeatures, nlevels, scale_factor)
    keys = ("kp", "response", "angle", "desc", "octave", "m01", "m10", "rot", "tuples", "level_xy")
    parts = {k: [] for k in keys}
    infos, cur, n, n_total = [], img, 0, 0
    for l in range(nlevels):
        if l:
            cur = np_orb.resize_linear(cur, lc[l], lr[l])
        info = dict(scale=scale[l], cols=lc[l], rows=lr[l], budget=nf[l], image=cur, score=None, blur=None, n=0)
        if nf[l] > 0 and 2 * edge_th < lc[l] and 2 * edge_th < lr[l]:
            r = detect_level(cur, nf[l], fast_th, edge_th, points, wta_k, patch_size, score)
            n_total += len(r["xy"])
            take = max(min(len(r["xy"]), cap - n), 0)
            pt = r["xy"][:take].astype(F)
            parts["kp"].append(pt * scale[l] if l else pt)
            parts["octave"].append(np.full(take, l, np.int32))
            parts["level_xy"].append(r["xy"][:take])
            for k in ("response", "angle", "desc", "m01", "m10", "rot", "tuples"):
                parts[k].append(r[k][:take])
            info.update(score=r["score"], blur=r["blur"], n=take)
            n += take
        infos.append(info)
    npt = len(points)

    def cat(k, shape, dtype):
        return np.concatenate(parts[k]).astype(dtype) if parts[k] else np.zeros(shape, dtype)
    res = dict(kp=cat("kp", (0, 2), F), response=cat("response", (0,), F), angle=cat("angle", (0,), F), desc=cat("desc", (0, 32), np.uint8),
               octave=cat("octave", (0,), np.int32), n_total=n_total)
    res["trace"] = dict(levels=infos, m01=cat("m01", (0,), np.int64), m10=cat("m10", (0,), np.int64), rot=cat("rot", (0, npt, 2), np.int64),
                        tuples=cat("tuples", (0, npt // wta_k, wta_k), np.int64), level_xy=cat("level_xy", (0, 2), np.int64),
                        points=points)
    return res
