"""Planned images for the ORB point front-end, each sitting on an edge that random scenes almost never produce — TEST
INFRASTRUCTURE ONLY.  A case is a dict
    name, images uint8 [B, rows, cols] (one canvas), prm (nfeatures, fast_th, edge_th, nlevels, scale_factor, max_keypoints),
    thresholds (None, or one FAST threshold per image), pattern int8 [256, 4], facts(case, exp)
`exp` is the list of np_orb.detect_levels results of the case's images (expected(case), computed once per process and shared by the
host and the GPU test).  facts() asserts, from the images and the statement's trace alone — never from the code under test — that the
case really hits the edge it was planned for.  Every image is generated here; nothing is a committed fixture.

Three edges the plan names do not exist and are therefore stated as their absence:
  * a compass sum of 2 (t + 1) - 1 at a TRUE corner: a 9-arc holds two compass points, each differing by at least t + 1, so a corner's
    sum is at least 2 (t + 1).  The case holds that sum at near-corners only and asserts the implication on every pixel;
  * a saddle (two compass points brighter AND two darker than the centre by more than t) at t = 254: it needs v + 255 and v - 255 in one
    byte image.  Saddles are planted at t = 20 and t = 1;
  * a rotated pattern coordinate exactly on x.5 (cvRound's half-to-even rule): at 0 / 90 / 180 / 270 degrees the products are integers, and
    for none of the 464 angles one off-centre pixel can give does any int8 pair land on a half (tests/test_orb_edges_host.py asserts it;
    the rounding itself is held on the host, tests/cpp/orb_rotate_host_main.cpp).
Per-image thresholds t - 1, t, t + 1 are clipped to the 1 .. 254 the detector accepts (t = 1: 1, 1, 2; t = 254: 253, 254, 254).
"""
import functools

import numpy as np

import np_orb

S_, E_, N_, W_ = 0, 4, 8, 12          # ring indices of the compass points (below, right, above, left)


def make_pattern(first=()):
    """256 tests (x0, y0, x1, y1) in [-13, 13]: `first`, then seeded random ones; the two points of a test differ."""
    rng = np.random.default_rng(4242)
    tests = [tuple(t) for t in first]
    while len(tests) < 256:
        t = tuple(int(v) for v in rng.integers(-13, 14, 4))
        if t[:2] != t[2:]:
            tests.append(t)
    return np.array(tests[:256], np.int8)


PATTERN = make_pattern()


def prm(nfeatures=4000, fast_th=20, edge_th=19, nlevels=1, scale_factor=1.2, max_keypoints=4096):
    return dict(nfeatures=nfeatures, fast_th=fast_th, edge_th=edge_th, nlevels=nlevels, scale_factor=scale_factor, max_keypoints=max_keypoints)


def case(name, images, p, facts, thresholds=None, pattern=None):
    images = np.ascontiguousarray(images, np.uint8)
    assert images.ndim == 3 and images.shape[1] >= 64 and images.shape[2] >= 64 and p["max_keypoints"] <= 4096
    return dict(name=name, images=images, prm=p, facts=facts, thresholds=thresholds, pattern=PATTERN if pattern is None else pattern)


def threshold_of(c, b):
    return int(c["thresholds"][b]) if c["thresholds"] is not None else c["prm"]["fast_th"]


_expected = {}


def expected(c):
    """The statement's result for every image of the case (computed once, never modified)."""
    if c["name"] not in _expected:
        p = c["prm"]
        _expected[c["name"]] = [np_orb.detect_levels(c["images"][b], p["nfeatures"], p["nlevels"], p["scale_factor"], threshold_of(c, b),
                                                     p["edge_th"], c["pattern"], p["max_keypoints"]) for b in range(len(c["images"]))]
    return _expected[c["name"]]


def kp_set(e, level=None):
    xy = e["trace"]["level_xy"]
    if level is not None:
        xy = xy[e["octave"] == level]
    return {(int(x), int(y)) for x, y in xy}


def put_ring(img, x, y, v, diffs):
    """A flat 10 x 10 block of value v around (x, y), and the 16 ring pixels at v + diffs[k]."""
    img[y - 5:y + 5, x - 5:x + 5] = v
    for k, (dx, dy) in enumerate(np_orb.CIRCLE):
        img[y + dy, x + dx] = v + diffs[k]


def arc(start, length, value, other=0):
    d = [other] * 16
    for j in range(length):
        d[(start + j) % 16] = value
    return d


# ---- threshold cells -------------------------------------------------------------------------------------------------------------
def threshold_cells(t):
    """[(x, y, side score of the planted arc or -1, is saddle)] and the image: arcs of 8 / 9 / 10 / 16 from every start, bright and
    dark, at differences t and t + 1; for t <= 127 the 32 '9 one way + 7 the other way' saddles."""
    vb, vd = (0, 255) if t > 100 else (60, 190)
    cells = []
    for length in (8, 9, 10, 16):
        for start in range(16):
            for pol in (1, -1):
                for d in (t, t + 1):
                    cells.append((vb if pol > 0 else vd, arc(start, length, pol * d), d - 1 if length >= 9 else -1, False))
    if t <= 127:
        for start in range(16):
            for pol in (1, -1):
                cells.append((128, arc(start, 9, pol * (t + 1), -pol * (t + 1)), t, True))
    ncol = 24
    nrow = (len(cells) + ncol - 1) // ncol
    img = np.full((25 + 10 * nrow + 20, 25 + 10 * ncol + 20), 128, np.uint8)
    out = []
    for i, (v, diffs, s, saddle) in enumerate(cells):
        x, y = 25 + 10 * (i % ncol), 25 + 10 * (i // ncol)
        put_ring(img, x, y, v, diffs)
        out.append((x, y, s, saddle))
    return img, out


def compass_counts(img, x, y, t):
    I = img.astype(np.int64)
    d = [I[y + np_orb.CIRCLE[k][1], x + np_orb.CIRCLE[k][0]] - I[y, x] for k in (S_, E_, N_, W_)]
    return sum(v > t for v in d), sum(v < -t for v in d), sum(abs(v) for v in d)


def threshold_case(t, batch):
    img, cells = threshold_cells(t)
    ths = [int(np.clip(t + k, 1, 254)) for k in (-1, 0, 1)] if batch else None

    def facts(c, exp):
        for b, e in enumerate(exp):
            th = threshold_of(c, b)
            sc = e["trace"]["levels"][0]["score"]
            n_eq = n_saddle = 0
            for x, y, s, saddle in cells:
                assert sc[y, x] == (s if s >= th else 0), (t, th, x, y, sc[y, x], s)
                n_eq += sc[y, x] == th
                nb, nd, _ = compass_counts(c["images"][b], x, y, th)
                n_saddle += bool(saddle and nb >= 2 and nd >= 2 and sc[y, x] >= th)
            assert n_eq > 0 or th > t, (t, th)                       # score exactly at the threshold (t + 1: the cells fall just short)
            if th == t:
                assert n_eq == 16 * 2 * 3 + (32 if t <= 127 else 0) and sc.max() <= 254
                assert n_saddle == (24 if t <= 127 else 0)    # an arc from a compass point holds three of them and leaves one
            if t == 254:
                assert sc.max() == 254                                # the largest score the 8-bit response field holds
    return case(f"threshold_t{t}_{'batch3' if batch else 'scalar'}", np.stack([img] * (3 if batch else 1)), prm(fast_th=t), facts, ths)


# ---- the pre-test on its edge ------------------------------------------------------------------------------------------------------
def pretest_case(t=20):
    q = t + 1

    def with_(d, **kw):
        d = list(d)
        for k, v in kw.items():
            d[int(k[1:])] = v
        return d
    rings = [("corner", arc(1, 9, q)), ("corner", arc(5, 9, q)), ("corner", with_(arc(1, 9, q), k2=q + 5, k6=q + 9)),
             ("corner", arc(13, 9, q)), ("plain", arc(N_, 1, 2 * q)), ("plain", with_(arc(1, 9, q), k4=q + 3, k8=q - 3)),
             ("plain", with_([0] * 16, k4=q, k12=-q)), ("plain", arc(1, 8, q)),
             ("below", with_(arc(1, 9, q), k4=t)), ("below", with_(arc(5, 9, q), k8=t)), ("below", arc(N_, 1, 2 * q - 1)),
             ("below", with_(arc(1, 9, q + 30), k4=t, k8=q)), ("above", arc(0, 9, q))]
    cells = [(kind, pol, [pol * v for v in d]) for kind, d in rings for pol in (1, -1)]
    img = np.full((64, 25 + 10 * len(cells) // 2 + 20), 128, np.uint8)
    pos = []
    for i, (kind, pol, d) in enumerate(cells):
        x, y = 25 + 10 * (i // 2), 25 + 10 * (i % 2)
        put_ring(img, x, y, 100 if pol > 0 else 150, d)
        pos.append((x, y, kind))

    def facts(c, exp):
        sc = exp[0]["trace"]["levels"][0]["score"]
        seen = set()
        for x, y, kind in pos:
            s = compass_counts(img, x, y, t)[2]
            assert s == {"corner": 2 * q, "plain": 2 * q, "below": 2 * q - 1, "above": 3 * q}[kind], (x, y, kind, s)
            assert (sc[y, x] >= t) == (kind in ("corner", "above")), (x, y, kind, sc[y, x])
            seen.add((s - 2 * q, bool(sc[y, x])))
        assert {(0, True), (0, False), (-1, False)} <= seen
        # the necessary test itself, on every pixel: a compass sum below 2 (t + 1) never belongs to a corner
        I = img.astype(np.int64)
        sad = np.zeros(I.shape, np.int64)
        sad[3:-3, 3:-3] = sum(np.abs(I[3 + dy:I.shape[0] - 3 + dy, 3 + dx:I.shape[1] - 3 + dx] - I[3:-3, 3:-3])
                              for dx, dy in (np_orb.CIRCLE[k] for k in (S_, E_, N_, W_)))
        assert not np.any((sad < 2 * q) & (sc > 0))
    return case("pretest_equality", img[None], prm(fast_th=t), facts)


# ---- non-maximum ties and tile seams -------------------------------------------------------------------------------------------------
NMS_PAIRS = ([("x63", (63, y), (64, y)) for y in (30, 100, 160)] + [("x127", (127, y), (128, y)) for y in (30, 100, 160)] +
             [("y63", (x, 63), (x, 64)) for x in (30, 100, 160)] + [("y127", (x, 127), (x, 128)) for x in (30, 100, 160)] +
             [("c63_63", (63, 63), (64, 64)), ("c127_63", (127, 63), (128, 64)), ("c63_127", (63, 127), (64, 128)),
              ("c127_127", (127, 127), (128, 128))] +
             [("inside", (90, 30), (91, 30)), ("inside", (100, 90), (100, 91)), ("inside", (40, 40), (41, 41)), ("inside", (151, 40), (150, 41))])


def nms_case():
    pts = [p for _, a, b in NMS_PAIRS for p in (a, b)]
    for i in range(0, len(pts), 2):
        for j in range(i + 2, len(pts)):
            for p in pts[i:i + 2]:
                assert max(abs(p[0] - pts[j][0]), abs(p[1] - pts[j][1])) >= 8
    imgs = np.full((3, 192, 192), 50, np.uint8)
    for v, (da, db) in enumerate(((41, 41), (42, 41), (41, 42))):     # equal; the first larger by one; the second larger by one
        for _, a, b in NMS_PAIRS:
            imgs[v, a[1], a[0]] = 50 + da
            imgs[v, b[1], b[0]] = 50 + db

    def facts(c, exp):
        suppressed, survived = set(), set()
        for v, e in enumerate(exp):
            sc, kps, want = e["trace"]["levels"][0]["score"], kp_set(e), set()
            for seam, a, b in NMS_PAIRS:
                sa, sb = sc[a[1], a[0]], sc[b[1], b[0]]
                assert (sa, sb) == ((40, 40), (41, 40), (40, 41))[v]
                if v == 0:
                    suppressed.add(seam)
                else:
                    want.add(a if v == 1 else b)
                    survived.add(seam)
            assert kps == want, (v, kps ^ want)
        assert suppressed == survived == {s for s, _, _ in NMS_PAIRS}
    return case("nms_ties_and_seams", imgs, prm(), facts)


# ---- the border ----------------------------------------------------------------------------------------------------------------------
def border_case(cols, rows, e):
    imgs = np.full((4, rows, cols), 50, np.uint8)
    want = []
    for v in range(4):
        ix, iy = v & 1, v >> 1
        X, Y = (e - 1 + ix, cols - e - 1 + ix), (e - 1 + iy, rows - e - 1 + iy)
        pts = [(x, y) for x in X for y in Y] + [(cols // 2, y) for y in Y] + [(x, rows // 2) for x in X]
        for x, y in pts:
            imgs[v, y, x] = 110
        # a pair astride the left border: the outer one suppresses the inner one when it is the larger
        yp = rows // 2 + 12
        imgs[v, yp, e - 1], imgs[v, yp, e] = (111, 110) if ix == 0 else (110, 111)
        w = {(x, y) for x, y in pts if e <= x < cols - e and e <= y < rows - e}
        if ix == 1:
            w.add((e, yp))
        want.append(w)

    def facts(c, exp):
        for v, ex in enumerate(exp):
            assert kp_set(ex) == want[v], (v, kp_set(ex) ^ want[v])
            sc = ex["trace"]["levels"][0]["score"]
            assert sc[rows // 2 + 12, e - 1] > 0 and sc[rows // 2 + 12, e] > 0
        allk = set().union(*want)
        assert {(e, e), (cols - e - 1, e), (e, rows - e - 1), (cols - e - 1, rows - e - 1)} <= allk
        assert all(e <= x < cols - e and e <= y < rows - e for x, y in allk) and [len(w) for w in want] == [3, 4, 3, 4]
    return case(f"border_e{e}_{cols}x{rows}", imgs, prm(edge_th=e), facts)


# ---- orientation sweep ---------------------------------------------------------------------------------------------------------------
def orientation_case():
    R, pitch, org = 16, 34, 35
    n = 2 * R + 1
    size = org + pitch * (n - 1) + R + 21
    img = np.full((size, size), 50, np.uint8)
    cells = {}
    for j in range(n):
        for i in range(n):
            x, y, u, v = org + pitch * i, org + pitch * j, i - R, j - R
            img[y, x] = 150
            if u or v:
                img[y + v, x + u] = 70       # 20 above the background: not a corner at t = 20, but it sets the moments
            cells[(x, y)] = (u, v)

    def facts(c, exp):
        e = exp[0]
        assert kp_set(e) == set(cells) and len(e["kp"]) == n * n
        disc = np_orb.disc_mask()
        assert disc.sum() == 749                                  # the patch of radius 15 (umax), the centre included
        tr = e["trace"]
        n_in = n_out = 0
        angles = set()
        for k, (x, y) in enumerate(tr["level_xy"]):
            u, v = cells[(int(x), int(y))]
            inside = max(abs(u), abs(v)) <= 15 and disc[v + 15, u + 15] and (u or v)
            assert (tr["m01"][k], tr["m10"][k]) == ((20 * v, 20 * u) if inside else (0, 0)), (u, v)
            if inside:
                n_in += 1
                angles.add(float(e["angle"][k]))
                assert abs((np.degrees(np.arctan2(v, u)) - e["angle"][k] + 180) % 360 - 180) < 0.3
            else:
                n_out += 1
                assert e["angle"][k] == 0
        assert n_in == 748 and n_out == n * n - 748 and len(angles) > 400
        assert {0.0, 90.0, 180.0, 270.0} <= angles                               # octant boundaries on the axes ...
        assert all(any(abs(a - d) < 0.3 for a in angles) for d in (45, 135, 225, 315))   # ... and |m01| == |m10|
    return case("orientation_sweep", img[None], prm(max_keypoints=2048), facts)


# ---- descriptor reach and equal values -----------------------------------------------------------------------------------------------
def descriptor_case(cols=96, rows=96):
    """Key-points at the four admissible image corners at 45 / 135 / 225 / 315 degrees and a pattern whose points lie at (+-11 .. 13,
    +-11 .. 13): rotated they reach +-18, so the tests read the blurred rows and columns 1 .. 3 and their mirrors — where the blur's
    REFLECT_101 border decides the value — and most of them compare two NEIGHBOURING rim pixels, so a rim value that is off by one flips bits."""
    corner = [(13, 13), (12, 13), (13, 12), (12, 12), (13, 11), (11, 13), (12, 11), (11, 12)]
    first = []
    for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
        q = [(sx * x, sy * y) for x, y in corner]
        first += [q[i] + q[j] for i in range(len(q)) for j in range(i + 1, len(q))]                 # 4 x 28 rim-against-rim tests
    ext = [(13, 0), (-13, 0), (0, 13), (0, -13), (13, 13), (-13, -13), (13, -13), (-13, 13)]
    first += [p + (0, 0) for p in ext] + [ext[i] + ext[(i + 1) % len(ext)] for i in range(len(ext))] + [(1, 0, 2, 0), (0, 1, 0, 2)]
    pat = make_pattern(first)
    e = 19
    yy, xx = np.mgrid[0:rows, 0:cols]
    img = np.full((rows, cols), 100, np.uint8)
    band = (np.minimum(xx, cols - 1 - xx) < 4) | (np.minimum(yy, rows - 1 - yy) < 4)     # texture the moments never see (the disc reaches row 4)
    img[band] = (30 + (xx * 37 + yy * 101 + xx * yy * 7) % 201)[band]     # (its corners lie outside the border: never key-points)
    lo, hx, hy, mx, my = e, cols - e - 1, rows - e - 1, cols // 2, rows // 2
    kps = {(lo, lo): (5, 5), (hx, lo): (-5, 5), (hx, hy): (-5, -5), (lo, hy): (5, -5),       # 45, 135, 225, 315 degrees
           (mx, lo): (5, 0), (hx, my): (0, 5), (mx, hy): (-5, 0), (lo, my): (0, -5)}         # 0, 90, 180, 270 degrees
    for (x, y), (u, v) in kps.items():
        img[y, x] = 200
        img[y + v, x + u] = 120

    def facts(c, exp):
        ex = exp[0]
        tr = ex["trace"]
        assert kp_set(ex) == set(kps)
        ang = {(int(x), int(y)): float(a) for (x, y), a in zip(tr["level_xy"], ex["angle"])}
        for (x, y), (u, v) in kps.items():
            assert abs((np.degrees(np.arctan2(v, u)) - ang[(x, y)] + 180) % 360 - 180) < 0.3
        assert {ang[(mx, lo)], ang[(hx, my)], ang[(mx, hy)], ang[(lo, my)]} == {0.0, 90.0, 180.0, 270.0}
        rot = tr["rot"]
        assert np.abs(rot).max() == 18
        px = np.stack([tr["level_xy"][:, 0:1] + rot[:, :, 0], tr["level_xy"][:, 0:1] + rot[:, :, 2]])   # [2, n, 256]: both points of a test
        py = np.stack([tr["level_xy"][:, 1:2] + rot[:, :, 1], tr["level_xy"][:, 1:2] + rot[:, :, 3]])
        for a, n in ((px, cols), (py, rows)):
            assert {1, 2, 3, n - 2, n - 3, n - 4} <= set(a.ravel().tolist()) and a.min() == 1 and a.max() == n - 2
        B = tr["levels"][0]["blur"].astype(np.int64)
        t0, t1 = B[py[0], px[0]], B[py[1], px[1]]
        assert (t0 == t1).sum() > 0 and (t0 < t1).sum() > 50 and (t0 > t1).sum() > 50
        # tests with BOTH points in the outermost three blurred rows / columns: many, decided either way, some by a difference of 1 or 2
        rim = np.minimum(np.minimum(px, cols - 1 - px), np.minimum(py, rows - 1 - py)) <= 3
        both = rim[0] & rim[1]
        assert both.sum() > 200 and (both & (t0 < t1)).sum() > 25 and (both & (t0 > t1)).sum() > 25 and (both & (np.abs(t0 - t1) <= 2) & (t0 != t1)).sum() > 8
        assert np.ptp(B[1:4]) > 20 and np.ptp(B[:, 1:4]) > 20
    return case(f"descriptor_reach_{cols}x{rows}", img[None], prm(), facts, pattern=pat)


# ---- pyramid rounding ------------------------------------------------------------------------------------------------------------------
def blobs(cols, rows, pitch=13):
    """Bright squares of side 1 .. 8 on a lattice: corners at several scales."""
    img = np.full((rows, cols), 60, np.uint8)
    k = 0
    for y in range(8, rows - 16, pitch):
        for x in range(8, cols - 16, pitch):
            s = (1, 2, 3, 4, 6, 8)[k % 6]
            img[y:y + s, x:x + s] = 130 + (k * 37) % 110
            k += 1
    return img


def pyramid_case(cols, rows, nlevels, sf, nfeatures, sizes, budgets, counts, img=None, row19=None):
    img = blobs(cols, rows) if img is None else img

    def facts(c, exp):
        lv = exp[0]["trace"]["levels"]
        assert [(l["cols"], l["rows"]) for l in lv] == sizes, [(l["cols"], l["rows"]) for l in lv]
        assert [l["budget"] for l in lv] == budgets, [l["budget"] for l in lv]
        assert [l["n"] for l in lv] == counts, [l["n"] for l in lv]
        assert np.array_equal(np.bincount(exp[0]["octave"], minlength=nlevels), counts)
        if row19 is not None:                                    # the level's only admissible row holds key-points
            assert lv[row19]["rows"] == 39 and counts[row19] > 0 and {y for _, y in kp_set(exp[0], row19)} == {19}
    return case(f"pyramid_{cols}x{rows}_f{sf}_n{nfeatures}", img[None], prm(nfeatures=nfeatures, nlevels=nlevels, scale_factor=sf, fast_th=12), facts)


def one_row_image(cols, rows, level):
    """Blobs of 2^level x 2^level pixels that land on the single admissible row (19) of level `level`."""
    img = np.full((rows, cols), 60, np.uint8)
    s = 1 << level
    for x in range(19 * s, cols - 19 * s, 9 * s):
        img[19 * s:20 * s, x:x + s] = 200
    return img


# ---- coordinate range, batch index, retainBest -------------------------------------------------------------------------------------------
def range_case(cols, rows):
    img = np.full((rows, cols), 50, np.uint8)
    long_ = max(cols, rows)
    along, across = (19, 2040, 2048, long_ - 20), (19, 44)
    pts = {(a, b) if cols > rows else (b, a) for a in along for b in across}
    for x, y in pts:
        img[y, x] = 120

    def facts(c, exp):
        assert kp_set(exp[0]) == pts and max(max(p) for p in pts) == 4075
    return case(f"range_{cols}x{rows}", img[None], prm(), facts)


def batch9_case():
    imgs = np.full((9, 64, 64), 50, np.uint8)
    want = []
    for b in range(9):
        x, y = 19 + 3 * b, 44 - 3 * b
        imgs[b, y, x] = 130 + 10 * b
        imgs[b, y + 6, x - 5 + b] = 70
        want.append({(x, y)})
    imgs[8, 40, 22] = 222                                        # the image past the multiple of 8 is unlike every other
    imgs[8, 36, 25] = 70
    want[8].add((22, 40))

    def facts(c, exp):
        assert [kp_set(e) for e in exp] == want
        assert len({e["desc"].tobytes() + e["angle"].tobytes() for e in exp}) == 9
    return case("batch_of_9", imgs, prm(), facts)


def retain_case(nfeatures, kept):
    resp = [30, 60, 25, 50, 40, 30, 50, 60, 30, 40, 50, 30]
    img = np.full((64, 140), 50, np.uint8)
    for k, r in enumerate(resp):
        img[30, 24 + 8 * k] = 50 + r + 1

    def facts(c, exp):
        assert sorted(exp[0]["trace"]["levels"][0]["score"][30, 24:24 + 96:8].tolist()) == sorted(resp)
        assert sum(r >= 50 for r in resp) == 5 and len(exp[0]["kp"]) == kept == exp[0]["n_total"]
        assert np.all(np.diff(exp[0]["kp"][:, 0]) > 0)          # row-major, not by response
    return case(f"retain_best_{nfeatures}", img[None], prm(nfeatures=nfeatures), facts)


def dense_case():
    """Noise at t = 1: (almost) every position passes the compass pre-test and a large share the signed compass test, so the kernel's
    candidate lists run (nearly) full in every tile; binary noise gives masses of corners with the one score 254, neighbours included."""
    rng = np.random.default_rng(7)
    imgs = np.stack([rng.integers(0, 2, (128, 128)) * 255, rng.integers(0, 256, (128, 128))]).astype(np.uint8)

    def facts(c, exp):
        for b, e in enumerate(exp):
            I = c["images"][b].astype(np.int64)
            sad = sum(np.abs(I[3 + dy:125 + dy, 3 + dx:125 + dx] - I[3:125, 3:125]) for dx, dy in (np_orb.CIRCLE[k] for k in (S_, E_, N_, W_)))
            assert (sad >= 4).mean() > 0.9
            sc = e["trace"]["levels"][0]["score"]
            assert (sc > 0).sum() > (100, 4000)[b] and len(e["kp"]) > 20       # uniform noise: a third of all pixels are corners
        sc = exp[0]["trace"]["levels"][0]["score"]
        assert set(np.unique(sc)) == {0, 254} and ((sc[:, 1:] == 254) & (sc[:, :-1] == 254)).sum() > 0    # equal neighbours: neither survives
    return case("dense_noise_t1", imgs, prm(fast_th=1), facts)


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = []
    for t in (20, 1, 254):
        cs += [threshold_case(t, False), threshold_case(t, True)]
    cs += [pretest_case(), nms_case()]
    cs += [border_case(80 + k, 89 + k, 19) for k in range(4)] + [border_case(96 + k, 105, 31) for k in range(4)]
    cs += [border_case(84, 148, 19)]                               # 64 + 20, 128 + 20: the last admissible column / row is alone in its tile
    cs += [orientation_case()] + [descriptor_case(96 + k, 96 + (k + 2) % 4) for k in range(4)]      # widths and heights = 0 .. 3 (mod 4)
    cs += pyramid_cases()
    cs += [range_case(4095, 64), range_case(64, 4095), batch9_case(), dense_case(), retain_case(4, 5), retain_case(5, 5), retain_case(6, 7)]
    assert len({c["name"] for c in cs}) == len(cs)
    return tuple(cs)


def pyramid_cases():
    """scale_factor 2.0: odd sizes meet cvRound's half-to-even rule (65 -> 32, 67 -> 34, 131 -> 66, 157 -> 78 -> 39); 77 -> 38 and every
    size below 39 leave a level without an admissible pixel, 39 leaves one admissible row / column / pixel.  The level sizes and budgets
    below are hand arithmetic (e.g. 300 (1 - 1/2) / (1 - 1/8) = 171.43 -> 171, 85.7 -> 86, the rest 43); the counts were read off the
    statement once and are held here."""
    b3 = [171, 86, 43]
    cs = [pyramid_case(65, 78, 3, 2.0, 300, [(65, 78), (32, 39), (16, 20)], b3, [1, 0, 0]),
          pyramid_case(78, 65, 3, 2.0, 300, [(78, 65), (39, 32), (20, 16)], b3, [2, 0, 0]),
          pyramid_case(67, 77, 3, 2.0, 300, [(67, 77), (34, 38), (17, 19)], b3, [1, 0, 0]),
          pyramid_case(77, 67, 3, 2.0, 300, [(77, 67), (38, 34), (19, 17)], b3, [3, 0, 0]),
          pyramid_case(131, 157, 3, 2.0, 300, [(131, 157), (66, 78), (33, 39)], b3, [9, 11, 0]),
          pyramid_case(157, 131, 3, 2.0, 300, [(157, 131), (78, 66), (39, 33)], b3, [11, 10, 0]),
          # budgets in which a level's share is 0: 1 -> 1, 0, 0 and 3 -> 2, 1, 0
          pyramid_case(131, 157, 3, 2.0, 1, [(131, 157), (66, 78), (33, 39)], [1, 0, 0], [1, 0, 0]),
          pyramid_case(131, 157, 3, 2.0, 3, [(131, 157), (66, 78), (33, 39)], [2, 1, 0], [2, 1, 0]),
          # one admissible row on level 1, on level 2, and one admissible PIXEL on level 2: each holds a corner
          pyramid_case(157, 78, 2, 2.0, 300, [(157, 78), (78, 39)], [200, 100], [0, 5], one_row_image(157, 78, 1), row19=1),
          pyramid_case(160, 157, 3, 2.0, 300, [(160, 157), (80, 78), (40, 39)], b3, [0, 0, 1], one_row_image(160, 157, 2), row19=2),
          pyramid_case(157, 157, 3, 2.0, 300, [(157, 157), (78, 78), (39, 39)], b3, [0, 1, 1], one_row_image(157, 157, 2), row19=2),
          # the shipped factor and another one: 211 / 1.2^l = 175.8, 146.5, 122.1, 101.8; 173 / 1.2^l = 144.2, 120.1, 100.1, 83.4
          pyramid_case(211, 173, 5, 1.2, 120, [(211, 173), (176, 144), (147, 120), (122, 100), (102, 83)], [33, 28, 23, 19, 17], [22, 29, 23, 19, 17]),
          pyramid_case(203, 155, 3, 1.5, 80, [(203, 155), (135, 103), (90, 69)], [38, 25, 17], [18, 25, 17])]
    return cs
