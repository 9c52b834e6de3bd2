"""A numpy statement of OpenCV's HarrisResponses (features2d/src/orb.cpp, blockSize 7, harris_k 0.04) and of the orb_score 0 ranking
built on it — test infrastructure, independent of csrc/orb_kernels.hip and of tests/cpp/harris_ref.c.

responses(): the Sobel-like sums Ix, Iy of the 49 pixels of the block whose top-left corner is (x - 3, y - 3), summed as integers
(int64), then the float32 formula one operation at a time — numpy rounds every float32 operation once, and never contracts.

detect_levels(): the expected output of the Harris-ranked ORB front-end, composed from the UNCHANGED oracle: per pyramid level the
oracle's FAST-ranked detector with twice the level's budget gives the candidates with their angles and descriptors (neither depends on
the ranking); their Harris responses are ranked here, cut at the level's budget with ties kept, in the oracle's row-major order."""
import numpy as np

BLOCK, R = 7, 3
HARRIS_K = np.float32(0.04)


def responses(img, xs, ys):
    """img uint8 [rows, cols]; xs, ys integer arrays (every block inside the image, one pixel of margin) -> float32 responses."""
    p = np.asarray(img, np.uint8).astype(np.int64)
    xs = np.asarray(xs, np.int64).reshape(-1); ys = np.asarray(ys, np.int64).reshape(-1)
    a = np.zeros(len(xs), np.int64); b = np.zeros(len(xs), np.int64); c = np.zeros(len(xs), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            y, x = ys + dy, xs + dx
            ix = (p[y, x + 1] - p[y, x - 1]) * 2 + (p[y - 1, x + 1] - p[y - 1, x - 1]) + (p[y + 1, x + 1] - p[y + 1, x - 1])
            iy = (p[y + 1, x] - p[y - 1, x]) * 2 + (p[y + 1, x - 1] - p[y - 1, x - 1]) + (p[y + 1, x + 1] - p[y - 1, x + 1])
            a += ix * ix; b += iy * iy; c += ix * iy
    return response_of_sums(a, b, c)


def response_of_sums(a, b, c):
    """((float)a * b - (float)c * c - harris_k * ((float)a + b) * ((float)a + b)) * scale^4 in float32, operation by operation."""
    assert np.all(np.abs(a) < 2 ** 31) and np.all(np.abs(b) < 2 ** 31) and np.all(np.abs(c) < 2 ** 31)   # they are C ints
    fa, fb, fc = np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32), np.asarray(c).astype(np.float32)
    scale = np.float32(1.0) / (np.float32(4 * BLOCK) * np.float32(255.0))
    scale4 = scale * scale * scale * scale
    ab = fa * fb
    cc = fc * fc
    tr = fa + fb
    k = HARRIS_K * tr
    k = k * tr
    r = ab - cc
    r = r - k
    r = r * scale4
    assert r.dtype == np.float32 and scale4.dtype == np.float32
    return r


def retain_best(values, n):
    """KeyPointsFilter::retainBest: the indices (ascending) of the values >= the n-th largest — ties at the cut are all kept."""
    values = np.asarray(values)
    if n <= 0:
        return np.zeros(0, np.int64)
    if len(values) <= n:
        return np.arange(len(values))
    cut = np.sort(values)[::-1][n - 1]
    return np.nonzero(values >= cut)[0]


def detect_level(oracle, img, n, fast_th=20, edge_th=19, pattern=None, cap=4096, info=None):
    """One level: retainBest(2 n) by FAST score (the oracle, uncapped), Harris responses, retainBest(n), the first `cap` in row-major order."""
    cand = oracle.orb_detect(img, nfeatures=2 * n, fast_th=fast_th, edge_th=edge_th, pattern=pattern, cap=1 << 18)
    assert len(cand["kp"]) < 1 << 18
    x, y = cand["kp"][:, 0].astype(np.int64), cand["kp"][:, 1].astype(np.int64)
    assert np.all(np.diff(y * 65536 + x) > 0)   # the oracle's row-major order
    resp = responses(img, x, y)
    keep = retain_best(resp, n)
    if info is not None:
        fast_keep = retain_best(cand["response"], n)   # what orb_score 1 keeps with the same budget
        info.append(dict(n=n, n_cand=len(x), n_keep=len(keep), differs=not np.array_equal(keep, fast_keep)))
    n_total = len(keep)
    keep = keep[:cap]
    return dict(kp=cand["kp"][keep], response=resp[keep], angle=cand["angle"][keep], desc=cand["desc"][keep], n_total=n_total)


def detect_levels(oracle, img, nfeatures=2000, nlevels=1, scale_factor=1.2, fast_th=20, edge_th=19, pattern=None, cap=4096, info=None, score=0):
    """All levels in level order, coordinates times the level scale (float32), octave = level — as orc_orb_detect_levels composes them.
    score=1 composes the oracle's own FAST ranking the same way (a check of this composition against orc_orb_detect_levels)."""
    img = np.ascontiguousarray(img, np.uint8)
    rows, cols = img.shape
    sc, lc, lr, nf = oracle.orb_levels(cols, rows, nfeatures, nlevels, scale_factor)
    out = dict(kp=[], response=[], angle=[], desc=[], octave=[])
    cur, n, n_total = img, 0, 0
    for l in range(nlevels):
        if l:
            cur = oracle.resize_linear(cur, int(lc[l]), int(lr[l]))
        if not (nf[l] > 0 and 2 * edge_th < lc[l] and 2 * edge_th < lr[l]):
            continue
        if score == 0:
            d = detect_level(oracle, cur, int(nf[l]), fast_th, edge_th, pattern, cap, info)
        else:
            d = oracle.orb_detect(cur, nfeatures=int(nf[l]), fast_th=fast_th, edge_th=edge_th, pattern=pattern, cap=1 << 18)
            d["n_total"] = len(d["kp"])   # (uncapped; the first `cap` of the row-major order are taken below)
        n_total += d["n_total"]
        m = max(0, min(len(d["kp"]), cap - n))
        kp = d["kp"][:m].astype(np.float32)
        if l:
            kp = kp * np.float32(sc[l])
        out["kp"].append(kp); out["octave"].append(np.full(m, l, np.int32))
        for k in ("response", "angle", "desc"):
            out[k].append(d[k][:m])
        n += m
    res = {k: np.concatenate(v) if v else np.zeros(0) for k, v in out.items()}
    if not out["kp"]:
        res = dict(kp=np.zeros((0, 2), np.float32), response=np.zeros(0, np.float32), angle=np.zeros(0, np.float32),
                   desc=np.zeros((0, 32), np.uint8), octave=np.zeros(0, np.int32))
    res["n_total"] = n_total
    return res
