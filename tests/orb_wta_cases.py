"""Planned images for the ORB descriptor settings other than (WTA_K 2, patch 31) — TEST INFRASTRUCTURE ONLY.  A case is a dict
    name, images uint8 [B, rows, cols], prm (wta_k, patch_size, edge_th, nfeatures, fast_th, nlevels, scale_factor, max_keypoints, score),
    pool int8 [256, 4] (the pattern of patch size 31 handed to stvo_orb_set_pattern), facts(case, exp)
`exp` is the list of np_orb_wta.detect_levels results of the case's images (expected(c): computed once per process, shared by the host
and the GPU test, never modified).  facts() asserts from the images and the statement's trace alone that the case hits the edge it was
planned for.  expected() itself asserts for every case that no read of the statement leaves the level image (numpy would wrap a
negative index silently).

Two edges the plan names exist only in part and are stated as what can be had:
  * "a rotated point on the last row / column the blurred patch holds" (reach R = ceil(h sqrt 2)) needs a pattern point on a corner
    (+-h, +-h) of the patch and round(h sqrt 2) = R.  At P = 63 (h = 31: 43.84 -> 44 = R) the WTA_K 2 pattern holds such a point and the
    case reads row 0 / column 0 of the image through it.  At P = 27 (h = 13: 18.38 -> 18, R = 19) no rotation reaches row 19: the case
    reaches 18, the farthest any point can get, i.e. image row / column 1;
  * "a flat patch, so that every tuple is all equal": a key-point is a corner, and the blur spreads its own pixel over 7 x 7, so the
    tuples with a point within 3 pixels of the centre cannot be flat.  Every other tuple of the case is all equal (more than 100 of 128).
"""
import functools
import math

import numpy as np

import np_orb
import np_orb_wta as nw
import orb_edge_cases as ec


def make_pool(seed=977):
    """512 points in [-13, 13]^2 as [256, 4]; the two points of a pair differ."""
    rng = np.random.default_rng(seed)
    tests = []
    while len(tests) < 256:
        t = tuple(int(v) for v in rng.integers(-13, 14, 4))
        if t[:2] != t[2:]:
            tests.append(t)
    return np.array(tests, np.int8)


POOL = make_pool()
# settings stvo_orb_set_descriptor must refuse on a detector with this edge threshold: (wta_k, patch_size, edge_th, error code)
REFUSED = ((2, 28, 19, -1), (4, 29, 19, -1), (3, 63, 43, -1), (2, 42, 29, -1), (2, 32, 22, -1), (1, 31, 19, -1), (5, 31, 19, -1),
           (0, 27, 19, -1), (2, 1, 19, -1), (3, 0, 19, -1), (4, -31, 19, -1), (2, 64, 60, -5), (4, 100, 60, -5), (5, 64, 60, -1))


def prm(wta_k, patch_size, edge_th=19, nfeatures=4000, fast_th=20, nlevels=1, scale_factor=1.2, max_keypoints=512, score=1):
    assert edge_th >= max(19, nw.reach(patch_size))
    return dict(wta_k=wta_k, patch_size=patch_size, edge_th=edge_th, nfeatures=nfeatures, fast_th=fast_th, nlevels=nlevels,
                scale_factor=scale_factor, max_keypoints=max_keypoints, score=score)


def case(name, images, p, facts, pool=None):
    images = np.ascontiguousarray(images, np.uint8)
    assert images.ndim == 3 and 64 <= images.shape[1] <= 144 and 96 <= images.shape[2] <= 192
    return dict(name=name, images=images, prm=p, facts=facts, pool=POOL if pool is None else pool)


def reads(e):
    """(px, py) int64 [n, points]: the pixel of the key-point's LEVEL every rotated pattern point reads."""
    tr = e["trace"]
    return tr["level_xy"][:, 0:1] + tr["rot"][:, :, 0], tr["level_xy"][:, 1:2] + tr["rot"][:, :, 1]


_expected = {}


def expected(c):
    if c["name"] not in _expected:
        p = c["prm"]
        out = [nw.detect_levels(img, p["nfeatures"], p["nlevels"], p["scale_factor"], p["fast_th"], p["edge_th"], c["pool"], p["max_keypoints"],
                                p["wta_k"], p["patch_size"], p["score"]) for img in c["images"]]
        h, R = p["patch_size"] // 2, nw.reach(p["patch_size"])
        for e in out:
            px, py = reads(e)
            lv = e["trace"]["levels"]
            for l in range(p["nlevels"]):
                m = e["octave"] == l
                if m.any():
                    xy = e["trace"]["level_xy"][m]
                    assert xy.min() >= h and (xy[:, 0] + h).max() < lv[l]["cols"] and (xy[:, 1] + h).max() < lv[l]["rows"]
                    assert px[m].min() >= 0 and py[m].min() >= 0 and px[m].max() < lv[l]["cols"] and py[m].max() < lv[l]["rows"]
            assert np.abs(e["trace"]["rot"]).max(initial=0) <= R
        _expected[c["name"]] = out
    return _expected[c["name"]]


def noise(cols, rows, seed, lo=90, amp=16):
    """Texture no FAST corner can come from at t = 20 (differences <= 15) but which the moments and, blurred, the tests see."""
    return np.random.default_rng(seed).integers(lo, lo + amp, (rows, cols)).astype(np.uint8)


def scatter(img, seed, n, edge, value=(170, 251), avoid=()):
    """n isolated bright pixels, at least 8 apart (Chebyshev), inside the border: each is a corner (its ring is darker by > 60)."""
    rng = np.random.default_rng(seed)
    rows, cols = img.shape
    pts = list(avoid)
    k = len(pts)
    for _ in range(10000):
        if len(pts) - k >= n:
            break
        x, y = int(rng.integers(edge, cols - edge)), int(rng.integers(edge, rows - edge))
        if all(max(abs(x - a), abs(y - b)) >= 8 for a, b in pts):
            pts.append((x, y))
            img[y, x] = int(rng.integers(*value))
    assert len(pts) - k == n
    return pts[k:]


def tie_stats(e, wta_k):
    """How often the tuples of a result show each equality pattern / each output value."""
    t = e["trace"]["tuples"].reshape(-1, wta_k)
    if wta_k == 3:
        t0, t1, t2 = t.T
        eq = dict(e01=(t0 == t1) & (t1 != t2), e12=(t1 == t2) & (t0 != t1), e02=(t0 == t2) & (t0 != t1), all=(t0 == t1) & (t1 == t2),
                  none=(t0 != t1) & (t1 != t2) & (t0 != t2))
        val = nw.wta3_values(t)
    else:
        t0, t1, t2, t3 = t.T
        u, v = np.maximum(t0, t1), np.maximum(t2, t3)
        eq = dict(e01=t0 == t1, e23=t2 == t3, final=(u == v) & ~((t0 == t1) & (t2 == t3) & (t0 == t2)), all=(t0 == t1) & (t1 == t2) & (t2 == t3),
                  none=(t0 != t1) & (t2 != t3) & (u != v))
        val = nw.wta4_values(t)
    return {k: int(m.sum()) for k, m in eq.items()}, np.bincount(val.ravel(), minlength=wta_k)


# ---- the border ------------------------------------------------------------------------------------------------------------------------
def border_case(P, e, wta_k):
    """Image 0: key-points exactly on the border (x or y = e, cols - e - 1, rows - e - 1) and bright pixels one step outside it, which
    are not key-points; image 1: the same one pixel inside."""
    cols, rows = max(96, 2 * e + 12), max(64, 2 * e + 12)
    imgs = np.stack([noise(cols, rows, 100 + P), noise(cols, rows, 200 + P)])
    want = []
    for v in range(2):
        X, Y = (e + v, cols - e - 1 - v), (e + v, rows - e - 1 - v)
        pts = [(x, y) for x in X for y in Y]
        for x, y in pts:
            imgs[v, y, x] = 210
        if v == 0:
            imgs[0, rows // 2, e - 1] = 210
            imgs[0, rows // 2, cols - e] = 210
        want.append(set(pts))

    def facts(c, exp):
        R = nw.reach(P)
        assert e >= R and (e == R or (P, e) == (21, 19))
        for v, ex in enumerate(exp):
            assert ec.kp_set(ex) == want[v], (v, ec.kp_set(ex) ^ want[v])
            sc = ex["trace"]["levels"][0]["score"]
            if v == 0:
                assert sc[rows // 2, e - 1] > 0 and sc[rows // 2, cols - e] > 0          # corners the border filter removes
        xy = exp[0]["trace"]["level_xy"]
        # the staged blurred patch of the on-border key-points touches the image's first / last column and row when e == R
        assert xy[:, 0].min() - e == 0 and xy[:, 0].max() + e == cols - 1 and xy[:, 1].min() - e == 0 and xy[:, 1].max() + e == rows - 1
        assert len({ex["desc"].tobytes() for ex in exp}) == 2
    return case(f"border_P{P}_e{e}_k{wta_k}", imgs, prm(wta_k, P, e), facts)


# ---- patch sizes: even and odd, the smallest, the threshold between the two kernel instances -----------------------------------------------
def patch_case(P, wta_k, e=19, pool=None, name=None):
    cols, rows = (96, 64) if e <= 20 else ((112, 80) if e <= 23 else (160, 128))
    img = noise(cols, rows, 300 + 7 * P + wta_k)
    bx, by = cols // 2 + 8, rows // 2
    img[by - 2:by + 2, bx - 3:bx + 3] = 200                   # a block: corners with neighbours of nearly equal score
    pts = scatter(img, P, 9, e, avoid=[(bx, by)])

    def facts(c, exp):
        ex = exp[0]
        assert set(pts) <= ec.kp_set(ex)
        h = P // 2
        assert nw.disc_mask(h).shape == (2 * h + 1, 2 * h + 1) and len(ex["trace"]["points"]) == (512, 384, 512)[wta_k - 2]
        assert np.abs(ex["trace"]["points"]).max() <= (13 if P == 31 else h)
        assert len(np.unique(ex["angle"])) > 5 and np.any(ex["trace"]["m10"] != 0) and np.any(ex["trace"]["m01"] != 0)
        assert len({d.tobytes() for d in ex["desc"]}) > 5
        if wta_k > 2:
            eq, val = tie_stats(ex, wta_k)
            assert all(n > 0 for n in val), val                # every value of the 2-bit field occurs (3 never does under WTA_K 3)
    return case(name or f"patch_P{P}_k{wta_k}_e{e}", img[None], prm(wta_k, P, e), facts, pool)


# ---- the reach of the rotated pattern ----------------------------------------------------------------------------------------------------
def reach_case(P, wta_k):
    """One key-point per image on an admissible corner of the image, flat inside its disc but for one pixel on a diagonal (the angle is
    45 / 135 / 225 / 315 degrees), texture outside the disc (which the moments do not see): a pattern point on a corner of the patch
    lands on an axis, as far out as a rotated point can get."""
    h, e = P // 2, nw.reach(P)
    far = int(round(h * math.sqrt(2.0)))
    cols, rows = max(96, 2 * e + 16), max(64, 2 * e + 12)
    disc = nw.disc_mask(h)
    imgs, want = [], []
    for i, (x, y) in enumerate(((e, e), (cols - e - 1, e), (cols - e - 1, rows - e - 1), (e, rows - e - 1))):
        for u, v in ((5, 5), (-5, 5), (-5, -5), (5, -5)):
            img = noise(cols, rows, 400 + i, lo=43)
            patch = img[y - h:y + h + 1, x - h:x + h + 1]
            patch[disc] = 50
            img[y, x] = 200
            img[y + v, x + u] = 70
            imgs.append(img)
            want.append((x, y, u, v))

    def facts(c, exp):
        lo_x = lo_y = 10 ** 6
        hi_x = hi_y = -1
        for (x, y, u, v), ex in zip(want, exp):
            assert ec.kp_set(ex) == {(x, y)} and (int(ex["trace"]["m10"][0]), int(ex["trace"]["m01"][0])) == (20 * u, 20 * v)
            assert abs((np.degrees(np.arctan2(v, u)) - float(ex["angle"][0]) + 180) % 360 - 180) < 0.3
            px, py = reads(ex)
            lo_x, lo_y, hi_x, hi_y = min(lo_x, px.min()), min(lo_y, py.min()), max(hi_x, px.max()), max(hi_y, py.max())
        assert np.abs(np.concatenate([ex["trace"]["rot"] for ex in exp])).max() == far
        assert (lo_x, lo_y, hi_x, hi_y) == (e - far, e - far, cols - 1 - e + far, rows - 1 - e + far)
        assert e - far == (0 if P == 63 else 1)
    return case(f"reach_P{P}_k{wta_k}", np.stack(imgs), prm(wta_k, P, e), facts)


# ---- the largest moments ---------------------------------------------------------------------------------------------------------------------
def moment_case(axis, wta_k, P=63):
    """A half plane of 0 / 255 through the key-point (itself 128: nine ring pixels are darker), along x or y, either sign: m10 or m01 is
    +-255 times the sum of the positive coordinates over the disc — 5.1e6 at half patch 31 — and the other moment is 0."""
    h, e = P // 2, nw.reach(P)
    cols, rows = 2 * e + 16, 2 * e + 12
    x0, y0 = cols // 2, rows // 2
    yy, xx = np.mgrid[0:rows, 0:cols]
    d = (xx - x0) if axis == "x" else (yy - y0)
    imgs = np.stack([np.where(d > 0, 255, 0), np.where(d < 0, 255, 0)]).astype(np.uint8)
    imgs[:, y0, x0] = 128
    r = np.arange(-h, h + 1)
    S = int((nw.disc_mask(h) * np.maximum(r, 0)[None, :]).sum())

    def facts(c, exp):
        assert 255 * S > 5_000_000 and 255 * S > 2 ** 16 * 64
        for sgn, ex in zip((1, -1), exp):
            assert ec.kp_set(ex) == {(x0, y0)}
            big, zero = ("m10", "m01") if axis == "x" else ("m01", "m10")
            assert int(ex["trace"][big][0]) == sgn * 255 * S and int(ex["trace"][zero][0]) == 0
            assert float(ex["angle"][0]) == {("x", 1): 0.0, ("x", -1): 180.0, ("y", 1): 90.0, ("y", -1): 270.0}[(axis, sgn)]
            eq, val = tie_stats(ex, wta_k)
            assert eq["all"] > 0 and eq["none"] + eq["e01"] > 0
    return case(f"moments_{axis}_P{P}_k{wta_k}", imgs, prm(wta_k, P, e), facts)


# ---- a flat patch ------------------------------------------------------------------------------------------------------------------------------
def flat_case(wta_k, P=63):
    e = nw.reach(P)
    cols, rows = max(96, 2 * e + 12), max(64, 2 * e + 12)
    img = np.full((rows, cols), 50, np.uint8)
    x0, y0 = cols // 2, rows // 2
    img[y0, x0] = 200

    def facts(c, exp):
        ex = exp[0]
        assert ec.kp_set(ex) == {(x0, y0)} and float(ex["angle"][0]) == 0.0 and int(ex["trace"]["m10"][0]) == 0
        t = ex["trace"]["tuples"][0]
        near = (np.abs(ex["trace"]["rot"][0]).max(axis=1) <= 3).reshape(-1, wta_k).any(axis=1)
        flat = (t == t[:, :1]).all(axis=1)
        assert np.all(flat[~near]) and flat.sum() > 100 and not flat.all()
        v = (nw.wta3_values if wta_k == 3 else nw.wta4_values)(t[None])[0]
        assert np.all(v[flat] == (0 if wta_k == 3 else 2))       # all equal: every strict comparison fails
    return case(f"flat_P{P}_k{wta_k}", img[None], prm(wta_k, P, e), facts)


# ---- every branch in a real descriptor ---------------------------------------------------------------------------------------------------------
def branch_case(wta_k, P=31, pool=None, name=None, score=1, nfeatures=4000):
    """Blurred fine texture: neighbouring values differ by 0, 1 or 2, so the tuples show every pattern of equalities and every branch."""
    cols, rows = (128, 96) if nw.reach(P) <= 22 else (192, 144)
    img = noise(cols, rows, 500 + wta_k, amp=6)
    img[::2, ::2] += 9
    scatter(img, 50 + wta_k, 24, max(19, nw.reach(P)))

    def facts(c, exp):
        eq, val = tie_stats(exp[0], wta_k)
        assert all(n > 20 for n in eq.values()), eq
        assert all(n > 50 for n in val), val
        assert len(exp[0]["kp"]) >= 24
    return case(name or f"branches_P{P}_k{wta_k}", img[None], prm(wta_k, P, max(19, nw.reach(P)), score=score, nfeatures=nfeatures), facts, pool)


# ---- levels, batch, ranking ----------------------------------------------------------------------------------------------------------------------
def levels_case():
    img = ec.blobs(192, 144)
    img = (img.astype(np.int64) + noise(192, 144, 600, lo=0, amp=12)).astype(np.uint8)

    def facts(c, exp):
        lv = exp[0]["trace"]["levels"]
        assert [(l["cols"], l["rows"]) for l in lv] == [(192, 144), (160, 120), (133, 100), (111, 83)]
        assert all(l["n"] > 0 for l in lv) and set(exp[0]["octave"].tolist()) == {0, 1, 2, 3}
    return case("levels4_P27_k3", img[None], prm(3, 27, nfeatures=300, nlevels=4, fast_th=12), facts)


def batch9_case():
    imgs = np.stack([noise(96, 64, 700 + b, lo=40 + 15 * b) for b in range(9)])
    want = []
    for b in range(9):
        if b == 8:
            imgs[8, 40:44, 30:37] = 255                           # the image past the multiple of 8 is unlike every other
        pts = scatter(imgs[b], 70 + b, 1 + b % 4, 19, value=(230, 251), avoid=[(33, 41)] if b == 8 else ())
        want.append(set(pts))

    def facts(c, exp):
        assert all(w <= ec.kp_set(e) for w, e in zip(want, exp)) and len(ec.kp_set(exp[8])) > len(want[8])
        assert len({e["desc"].tobytes() + e["angle"].tobytes() for e in exp}) == 9
        assert len({len(e["kp"]) for e in exp}) >= 4
    return case("batch_of_9_P21_k4", imgs, prm(4, 21), facts)


def harris_case():
    img = ec.blobs(160, 120)
    img = (img.astype(np.int64) + noise(160, 120, 800, lo=0, amp=12)).astype(np.uint8)

    def facts(c, exp):
        ex = exp[0]
        fast = nw.detect_levels(img, 20, 1, 1.2, 12, 19, c["pool"], 512, 4, 31, 1)
        assert 20 <= len(ex["kp"]) < 30 and ex["n_total"] == len(ex["kp"])
        assert not np.array_equal(fast["kp"], ex["kp"])                          # the Harris cut keeps other key-points than the FAST cut
        assert np.any(ex["response"] != np.round(ex["response"]))               # responses are Harris responses
        assert all(n > 0 for n in tie_stats(ex, 4)[1])
    return case("harris_P31_k4", img[None], prm(4, 31, nfeatures=20, fast_th=12, score=0), facts)


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = [border_case(27, 19, 3), border_case(21, 19, 4), border_case(41, 29, 2), border_case(63, 44, 4)]
    cs += [patch_case(2, 4), patch_case(3, 3), patch_case(4, 2), patch_case(5, 4), patch_case(12, 3), patch_case(26, 2), patch_case(27, 4),
           patch_case(30, 3, 22), patch_case(32, 2, 23), patch_case(33, 4, 23), patch_case(62, 3, 44)]
    cs += [reach_case(27, 4), reach_case(63, 2)]
    cs += [moment_case("x", 4), moment_case("y", 3)]
    cs += [flat_case(3), flat_case(4)]
    cs += [branch_case(3), branch_case(4), branch_case(3, 21), branch_case(4, 63)]
    cs += [branch_case(3, 31, make_pool(31337), "caller_pool_P31_k3")]
    cs += [levels_case(), batch9_case(), harris_case()]
    assert len({c["name"] for c in cs}) == len(cs)
    return tuple(cs)


# the subset that also runs through stvo_orb_detect / _dev, the handler mirror and ImagePipeline (tests/test_gpu_orb_wta.py)
ENTRY_SUBSET = ("border_P63_e44_k4", "patch_P2_k4_e19", "branches_P31_k3", "batch_of_9_P21_k4")
