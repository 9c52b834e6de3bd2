"""Planned images and key-lines for the LBD line descriptor, each sitting on an edge that random segments on random scenes almost never
reach — TEST INFRASTRUCTURE ONLY.  A case is a dict
    name, images uint8 [B, rows, cols], lines: B arrays [n_b, 5] float32 (sx, sy, ex, ey, direction), npx: B arrays [n_b] int32
    (KeyLine::numOfPixels), M (max_keylines), n_lines (None, or the B counts handed to the kernel in place of n_b: above M, negative),
    facts(tr)
`tr[b][l]` is the trace np_lbd.compute returns for line l of image b.  facts() asserts from the trace alone — never from the code under
test — that the case really hits the edge it is named after.  expected(case) is the statement's float32 result, computed once per
process and shared by the host and the GPU test.  as_crop(case) is the same case as the top-left crop of a larger slot with other
content outside the crop (stvo_lbd_set_image_sizes).

Everything is generated here except the hard angles (tests/golden/lbd_hard_angles.npz).  Images run from 8 x 8, the smallest
stvo_lbd_create takes, to 160 x 120; the 63-row support region is taller than most of them, so most lines clamp at the top and bottom.

Domain: every sample coordinate stays inside +-32767 before the clamp and every direction inside [-2 pi, 2 pi]; beyond that the source's
(short) cast of the rounded coordinate is undefined.  expected() asserts it for every case."""
import math
import os

import numpy as np

import np_lbd

F32 = np.float32
PI32 = F32(math.pi)                  # 3.14159274: cos is -1 exactly, sin is -8.7e-8
HALF_PI32 = F32(math.pi / 2)


def noise(seed, cols, rows, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (rows, cols)).astype(np.uint8)


def line(mx, my, angle, npx, span=None):
    """A key-line with mid-point exactly (mx, my): the endpoints are mid -+ an offset on the quarter-pixel grid along the direction
    (span: half its length; None: (npx - 1) / 2; 0: both endpoints at the mid-point)."""
    half = (npx - 1) / 2.0 if span is None else span
    ox, oy = round(half * math.cos(float(angle)) * 4) / 4, round(half * math.sin(float(angle)) * 4) / 4
    mx, my = F32(mx), F32(my)
    rec = [F32(mx - F32(ox)), F32(my - F32(oy)), F32(mx + F32(ox)), F32(my + F32(oy)), F32(angle)]
    if span == 0:
        rec[:4] = [mx, my, mx, my]
    return rec, int(npx)


def case(name, images, sets, facts, M=None, n_lines=None):
    images = np.ascontiguousarray(images, np.uint8)
    if images.ndim == 2:
        images = images[None]
    if sets and not isinstance(sets[0], list):
        sets = [sets]                                  # one image: a flat list of line() results
    assert len(sets) == len(images) <= 4 and 8 <= images.shape[1] <= 120 and 8 <= images.shape[2] <= 160
    lines = [np.array([s[0] for s in st], F32).reshape(-1, 5) for st in sets]
    npx = [np.array([s[1] for s in st], np.int64).astype(np.int32) for st in sets]
    M = max(max(len(l) for l in lines), 1) if M is None else M
    assert M <= 64
    return dict(name=name, images=images, lines=lines, npx=npx, M=M, n_lines=n_lines, facts=facts, size=None)


def counts(c):
    """the number of key-lines the kernel describes per image: n_lines clamped to [0, M]"""
    n = [len(l) for l in c["lines"]] if c["n_lines"] is None else c["n_lines"]
    return [min(max(int(v), 0), c["M"]) for v in n]


_expected = {}


def expected(c):
    """np_lbd.compute(float32) of every image of the case: a list of dicts (desc, desc_f, trace), computed once, never modified"""
    key = (c["name"], c["size"])
    if key not in _expected:
        out = []
        for b, n in enumerate(counts(c)):
            r = np_lbd.compute(c["images"][b], c["lines"][b][:n], c["npx"][b][:n], size=c["size"])
            assert all(t["out_of_domain"] == 0 for t in r["trace"]), (c["name"], b)
            assert np.all(np.abs(c["lines"][b][:, 4]) <= F32(2 * math.pi)), (c["name"], b)
            out.append(r)
        _expected[key] = out
    return _expected[key]


def as_crop(c, k):
    """The case as the top-left crop of a slot 5 + k % 4 columns wider and 3 rows taller, noise outside the crop."""
    B, rows, cols = c["images"].shape
    slot = noise(977 + k, cols + 5 + k % 4, (rows + 3) * B).reshape(B, rows + 3, cols + 5 + k % 4)
    slot[:, :rows, :cols] = c["images"]
    d = dict(c)
    d.update(name=c["name"] + "@crop", images=slot, size=(cols, rows))
    return d


def hard_angles():
    t = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lbd_hard_angles.npz"))
    return {k: t[k] for k in t.files}


# ---------------------------------------------------------------------------------------------------------------- the cases
def rounding_ties():
    img = noise(1, 64, 48)
    # direction 0: dL = (1, 0) exactly.  x = mid_x - halfWidth + w, y = mid_y - 31 + hID.
    x_ties = [line(30.5, 24, 0.0, 22), line(30.5, 24, 0.0, 21), line(9.5, 20, 0.0, 21),              # the last starts at x = -0.5
              line(np.nextafter(F32(20.5), F32(0)), 24, 0.0, 5, span=0)]                               # k + 0.5 - 1 ulp: no tie
    y_ties = [line(30, 24.5, 0.0, 9), line(31, 30.5, 0.0, 12),                                         # every row at k + 0.5, from -6.5 / -0.5
              line(30, np.nextafter(F32(24.5), F32(0)), 0.0, 9, span=0)]
    # direction pi as a float: dL0 = -1 exactly, dL1 = -8.7e-8, absorbed by every coordinate of 2 and more
    pi_ties = [line(30.5, 24.5, PI32, 9), line(30.5, 24.5, -PI32, 9), line(20.5, 30.5, PI32, 16)]

    def facts(tr):
        a, b, p = tr
        assert a[0]["tie_x"] == 63 * 22 and a[1]["tie_x"] == 63 * 21 and a[2]["tie_x"] == 63 * 21 and a[3]["tie_x"] == 0
        assert a[2]["x_m1"] == 63                          # -0.5 rounds to -1, away from zero
        assert all(t["tie_y"] == 0 for t in a)
        assert b[0]["tie_y"] == 63 * 9 and b[1]["tie_y"] == 63 * 12 and b[1]["y_m1"] == 12
        assert b[2]["tie_y"] == 24 * 9                     # one ulp below the tie until y reaches 32, where the ulp doubles and the sum rounds onto it
        assert all(t["tie_x"] == 0 for t in b)
        assert all(t["tie_y"] > 63 * t["length"] // 2 for t in p)   # the rows of |y| >= 2 stay on their tie along the whole walk
    return case("rounding_ties", np.stack([img, img, img]), [x_ties, y_ties, pi_ties], facts)


def clamps_each_border():
    img = noise(2, 160, 120)
    L = [line(2, 60, 0.0, 11), line(157, 60, 0.0, 11), line(80, 5, 0.0, 11), line(80, 114, 0.0, 11),          # left, right, top, bottom
         line(3, 4, 0.4, 9), line(156, 4, -0.4, 9), line(3, 115, -0.4, 9), line(156, 115, 0.4, 9),             # the four corners
         line(80, 60, 0.3, 31)]                                                                                  # none

    def facts(tr):
        want = ["l", "r", "t", "b", "lt", "rt", "lb", "rb", ""]
        for t, w in zip(tr[0], want):
            got = "".join(k[6] for k in ("clamp_left", "clamp_right", "clamp_top", "clamp_bottom") if t[k] > 0)
            assert got == w, (got, w)
    return case("clamps_each_border", img, L, facts)


def clamps_exact():
    cols, rows = 40, 72
    img = noise(3, cols, rows)
    L = [line(cols - 3, 36, 0.0, 7),      # x = cols - 6 .. cols
         line(2, 36, 0.0, 7),             # x = -1 .. 5
         line(20, rows - 31, 0.0, 5),     # y = rows - 62 .. rows
         line(20, 30, 0.0, 5)]            # y = -1 .. 61

    def facts(tr):
        a, b, c, d = tr[0]
        assert a["x_last"] == 63 and a["x_cols"] == 63 and a["clamp_right"] == 63
        assert b["x_m1"] == 63 and b["clamp_left"] == 63
        assert c["y_last"] == 5 and c["y_rows"] == 5 and c["clamp_bottom"] == 5 and c["clamp_top"] == 0
        assert d["y_m1"] == 5 and d["clamp_top"] == 5 and d["clamp_bottom"] == 0
    return case("clamps_exact", img, L, facts)


def lines_outside():
    img = noise(4, 24, 23)
    L = [line(-100, -80, 0.7, 15), line(74, 11, 0.0, 9), line(12, 300, 1.2, 20), line(-40, 11, HALF_PI32, 7)]

    def facts(tr):
        a, b, c, d = tr[0]
        assert a["clamp_left"] == a["clamp_top"] == 63 * 15          # every sample is the top-left pixel
        assert b["clamp_right"] == 63 * 9 and c["clamp_bottom"] == 63 * 20 and d["clamp_left"] == 63 * 7
    return case("lines_outside", img, L, facts)


WALKS = list(range(1, 18)) + [63, 64, 65]
WRAPS = [(0, 0), (-3, -3), (32768, -32768), (65537, 1), (-65533, 3)]


def walk_lengths():
    img = noise(5, 160, 120)
    L = [line(80, 60, 0.37, n) for n in WALKS]
    L += [line(80, 60, 0.37, 9, span=20), line(80, 60, 0.37, 41, span=4)]       # endpoints that contradict num_pixels: only their mid-point counts
    W = [line(80, 60, 0.37, n, span=4) for n, _ in WRAPS]                       # what the (short) cast makes of num_pixels

    def facts(tr):
        t = tr[0]
        assert [x["length"] for x in t] == WALKS + [9, 41]
        assert {x["length"] % 8 for x in t[:len(WALKS)]} == set(range(8))
        assert not any(x["nan"] for x in t)

    def wrap_facts(tr):
        assert [x["length"] for x in tr[0]] == [w for _, w in WRAPS]
        assert [x["nan"] for x in tr[0]] == [True, True, True, False, False]   # no sample: 0 / 0
    return [case("walk_lengths", img, L, facts), case("walk_wraps", img, W, wrap_facts)]


def gradient_words():
    # a patch whose blurred values differ by a level or two (small gradients, the all-ones halves among them: dx and
    # dy of a Sobel have one parity, so the words (-1, 0) and (0, -1) do not exist and (-2, 0), (0, -2), (-1, 1), (1, -1) stand for them), a bright block (all
    # four sign pairs around it) and a 0 / 255 seam (the largest step the blur leaves)
    cols, rows = 96, 64
    img = np.full((rows, cols), 100, np.uint8)
    img[:, :40] = noise(6, 40, rows, 98, 104)
    img[20:44, 50:66] = 230
    img[:, 80:] = 255
    img[:, 72:80] = 0
    L = [line(20, 32, 0.0, 31), line(58, 32, 0.3, 33), line(80, 32, 0.0, 15), line(80, 32, HALF_PI32, 15), line(79.5, 30, -HALF_PI32, 8)]
    dx, dy, _, _ = np_lbd.gradients(img)
    top = int(np.abs(dx).max())
    words = set(zip(dx[1:63, 5:36].reshape(-1).tolist(), dy[1:63, 5:36].reshape(-1).tolist()))   # what the first line walks over

    def facts(tr):
        t = tr[0]
        assert t[0]["w_neg_zero"] > 0 and t[0]["w_zero_neg"] > 0 and t[0]["w_m1_m1"] > 0
        assert (-2, 0) in words and (0, -2) in words and (-1, 1) in words and (1, -1) in words
        assert np.all((dx.astype(int) - dy) % 2 == 0)       # one parity: no (-1, 0), no (0, -1) from any image
        assert all(t[1][k] > 0 for k in ("pp", "pn", "np", "nn")) and all(t[0][k] > 0 for k in ("pp", "pn", "np", "nn"))
        assert top == 664 and all(x["max_abs_g"] == top for x in t[1:])   # 4 x (179 - 13) of the blurred step 0, 13, 76, 179, 241, 255
    return case("gradient_words", img, L, facts)


def statistics():
    cols, rows = 160, 120
    band4 = np.full((rows, cols), 90, np.uint8)
    band4[60:62] = noise(7, cols, 2)                        # blur and Sobel spread two rows over eight: the centre band and its neighbours
    band0 = np.full((rows, cols), 90, np.uint8)
    band0[30:32] = noise(8, cols, 2)                        # rows 27 .. 34: hID 0 .. 5 of a line at y = 58
    side = np.full((rows, cols), 90, np.uint8)
    side[:56] = noise(9, cols, 56)                          # texture above the line only
    flat = np.full((rows, cols), 77, np.uint8)
    seam = noise(10, cols, rows)
    seam[:, 80:] = 140                                      # a flat right half
    L = [line(80, 60, 0.0, 41), line(80, 60, PI32, 41), line(60, 60, 0.0, 9)]
    sets = [L, [line(80, 58, 0.0, 41)], [line(80, 60, 0.0, 41), line(80, 60, 0.05, 64)], [line(80, 60, 0.0, 12), line(30, 50, 1.0, 30)]]
    seam_set = [line(80, 60, HALF_PI32, 31), line(80, 60, -HALF_PI32, 31), line(84, 60, HALF_PI32, 31)]

    def facts(tr):
        for t in tr[0] + tr[1]:                             # one band: the clip fires, whole bands are exactly 0 and compare equal
            assert t["clipped"] > 0 and t["equal_cmp"] >= 8 * 3 and not t["nan"]
        for t in tr[2]:
            assert not t["nan"] and t["equal_cmp"] >= 8 * 3
        assert all(t["nan"] and t["nan_cmp"] == 256 for t in tr[3])

    def seam_facts(tr):
        assert not any(t["nan"] for t in tr[0]) and all(t["equal_cmp"] > 0 for t in tr[0][:2])
    return [case("statistics", np.stack([band4, band0, side, flat]), sets, facts),
            case("flat_half_at_the_seam", seam, seam_set, seam_facts)]


def directions():
    img = noise(11, 64, 48)
    down = lambda a: np.nextafter(F32(a), F32(0))           # one ulp towards zero
    ang = [0.0, -0.0, HALF_PI32, -HALF_PI32, PI32, -PI32, down(PI32), down(-PI32), F32(2 * math.pi), F32(-2 * math.pi), down(HALF_PI32)]
    L = [line(32, 24, a, 13, span=3) for a in ang]
    L += [line(32, 24, 1.0, 13, span=0), (np.array([26, 24, 38, 24, 1.0], F32).tolist(), 13),    # a direction that contradicts the endpoints
          (np.array([26, 24, 38, 24, 0.0], F32).tolist(), 13)]
    h = hard_angles()
    L += [line(32, 24, s * a, 9 + i, span=0) for i, a in enumerate(h["angle"]) for s in (1, -1)]

    def facts(tr):
        t = tr[0]
        assert len(t) == len(ang) + 3 + 2 * len(h["angle"]) and not any(x["nan"] for x in t)
        assert t[0]["tie_x"] == t[0]["tie_y"] == 0
    return case("directions", img, L, facts)


def launch_shapes():
    img = noise(12, 35, 21)
    small = noise(13, 8, 8)                                 # the smallest image stvo_lbd_create takes
    pool = [line(5 + 3 * i, 4 + 2 * (i % 7), 0.2 * i - 1.0, 3 + i) for i in range(8)]
    out = []
    for n in (1, 3, 4, 5):
        out.append(case(f"launch_{n}_lines", img, pool[:n], lambda tr, n=n: None, M=8))     # 1, 3, 4 and 1 live waves in the last workgroup
    out.append(case("launch_max_keylines", img, pool[:6], lambda tr: None, M=6))             # 2 live waves
    out.append(case("launch_one_image_without_lines", np.stack([img, img, img]), [pool[:2], [], pool[2:5]], lambda tr: None, M=7))
    # n_lines above max_keylines (clamped to it) and negative (none): the records hold M lines per image
    out.append(case("launch_n_lines_out_of_range", np.stack([img, img, img, img]), [pool[:5], pool[:5], pool[:5], pool[3:8]],
                    lambda tr: None, M=5, n_lines=[7, -2, 0, 3]))
    out.append(case("smallest_image", small, [line(4, 4, 0.3, 5), line(3.5, 3.5, -2.0, 9), line(7, 0, 0.0, 1)], lambda tr: None, M=4))
    return out


_cases = None


def all_cases():
    global _cases
    if _cases is None:
        _cases = [rounding_ties(), clamps_each_border(), clamps_exact(), lines_outside()] + walk_lengths() + [gradient_words()]
        _cases += statistics() + [directions()] + launch_shapes()
    return _cases


def crop_cases():
    """every case again as a crop, the slot widths running through every residue modulo 4"""
    out = [as_crop(c, k) for k, c in enumerate(all_cases())]
    assert {c["images"].shape[2] % 4 for c in out} == {0, 1, 2, 3}
    return out


def hard_angle_lines():
    """The hard angles and their negatives as key-lines of every length residue modulo 8 over a textured image: one case of 4 images."""
    img = noise(14, 96, 80)
    h = hard_angles()
    L = [line(48, 40, s * a, 9 + r, span=0) for a in h["angle"] for s in (1, -1) for r in range(8)]
    per = -(-len(L) // 4)
    sets = [L[i * per:(i + 1) * per] for i in range(4)]
    return case("hard_angles", np.stack([img] * 4), sets, lambda tr: None, M=per)
