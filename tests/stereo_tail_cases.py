"""Case frames for the tails of the stereo association, shared by tests/test_stereo_tail_host.py (CPU) and
tests/test_gpu_stereo_tail.py — TEST INFRASTRUCTURE ONLY.

A frame is built from a PLAN: every left feature either has no partner or a right feature with chosen coordinates.  Every feature
gets its own random 256-bit descriptor whose first four bytes are the feature's serial number in its frame; a partner carries its
left feature's row.  The right partner's distance is then 0, every other pair's is ~128 of 256 bits, and every right feature has a
partner: the grid matcher (ratio test, mutual check and its order dependence included, src/matching.cpp:111-258) returns exactly the
plan provided the partner lies in the left feature's window — same grid row, at most matching_s_ws cells to the left; for lines a
rasterised cell in the window of either left end-point cell and a direction within line_sim_th.  Unpartnered left features are the
distractors.  tests/test_stereo_tail_host.py asserts that the oracle's raw matches equal the plan for every frame.

A case SET is what one Sequences object runs: one camera, one set of match parameters, its frames side by side as streams."""
import functools

import numpy as np

import np_stereo_tail as st
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params

F32 = np.float32
# 2048 x 1536: a grid cell (64 x 48 cells) is 32 x 32 pixels, the pixel -> cell scale 1 / 32 is exact, the intrinsics are dyadic
GRID_CAM = dict(fx=512.0, fy=512.0, cx=1024.5, cy=768.25, b=0.5, width=2048, height=1536)
WIDE_CAM = dict(GRID_CAM, width=4096, cx=2048.5)  # 64-pixel columns: a 600-pixel disparity stays within matching_s_ws = 10 cells
ULP600 = 2.0 ** -14                                # float spacing in [512, 1024)


def nxt(x, k=1):
    """the k-th float32 above (k > 0) or below (k < 0) x"""
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf))
    return x


class FrameBuilder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pl, self.pr, self.po, self.pe, self.pn = [], [], [], [], []
        self.ll, self.lr, self.lo, self.le, self.ln = [], [], [], [], []

    def point(self, xl, yl, right=None, level=0, expect=-1, name=""):
        """right: None (no partner) or (xr, yr)"""
        self.pl.append((xl, yl)); self.pr.append(right); self.po.append(level); self.pe.append(expect); self.pn.append(name)

    def line(self, left, right=None, level=0, expect=-1, name=""):
        """left = (xs, ys, xe, ye); right: None or the same four of the right key-line"""
        self.ll.append(left); self.lr.append(right); self.lo.append(level); self.le.append(expect); self.ln.append(name)

    def _side(self, left, right, width):
        n = len(left)
        desc_l = self.rng.integers(0, 256, (n, 32), dtype=np.uint8)
        desc_l[:, :4] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)  # the serial number
        has = [i for i in range(n) if right[i] is not None]
        order = self.rng.permutation(len(has))  # right index != left index
        plan = np.full(n, -1, np.int32)
        xr = np.zeros((len(has), width), F32); desc_r = np.zeros((len(has), 32), np.uint8)
        for j, q in enumerate(order):
            i = has[q]
            plan[i] = j; xr[j] = np.asarray(right[i], F32); desc_r[j] = desc_l[i]
        return np.asarray(left, F32).reshape(n, width), desc_l, xr, desc_r, plan

    def build(self, name, exact):
        kp_l, desc_l, kp_r, desc_r, plan_p = self._side(self.pl, self.pr, 2)
        kl_l, ldesc_l, kl_r, ldesc_r, plan_l = self._side(self.ll, self.lr, 4)
        frame = dict(kp_l=kp_l, oct_l=np.asarray(self.po, np.int32), desc_l=desc_l, kp_r=kp_r, desc_r=desc_r,
                     kl_l=kl_l, oct_ll=np.asarray(self.lo, np.int32), ldesc_l=ldesc_l, kl_r=kl_r, ldesc_r=ldesc_r)
        return dict(name=name, frame=frame, plan_p=plan_p, plan_l=plan_l, exact=exact, expect_p=np.asarray(self.pe, np.int32),
                    expect_l=np.asarray(self.le, np.int32), names_p=list(self.pn), names_l=list(self.ln))


# ---- point filters ---------------------------------------------------------------------------------------------------------------
def point_filter_frame(seed, max_dist_epip):
    """|yl - yr| at 0, one float ulp, exactly max_dist_epip and the floats around it; the disparity at min_disp = 1, the floats around
    it, 0, negative; levels 0 .. 7.  Every coordinate pair is chosen so that the FLOAT difference is the number named."""
    fb = FrameBuilder(seed)
    t = float(max_dist_epip)
    K, D, E = st.KEPT, st.DISPARITY, st.EPIPOLAR
    col = iter(range(2, 62))

    def x0():
        return 32.0 * next(col) + 16.0

    def epi(yl, yr, expect, name):
        x = x0()
        fb.point(x, yl, (x - 5.0, yr), expect=expect, name=name)

    epi(100.0, 100.0, K, "dy = 0")
    epi(100.0, nxt(100.0), K if t > 0 else E, "dy = one ulp of the rows")
    epi(nxt(100.0), 100.0, K if t > 0 else E, "dy = minus one ulp of the rows")
    epi(0.0, nxt(0.0), K if t > 0 else E, "dy = the smallest subnormal float")
    if t > 0:
        tf = F32(t)
        for k in (-1, 0, 1):
            v = nxt(tf, k)
            keep = float(v) <= t  # the float widened against the double threshold: 0.3f > 0.3 drops, a float comparison would keep it
            epi(v, 0.0, K if keep else E, f"dy = float({t}) {k:+d} ulp, yl above")
            epi(0.0, v, K if keep else E, f"dy = float({t}) {k:+d} ulp, yr above")
    else:
        epi(nxt(0.0, 2), nxt(0.0), E, "dy = one subnormal step between two subnormal rows")
    epi(40.0, 41.5, E, "dy = 1.5")

    def dsp(xl, xr, expect, name, y=48.0):
        fb.point(xl, y, (xr, y), expect=expect, name=name)

    dsp(100.0, 99.0, K, "disparity = min_disp exactly")
    dsp(1.5, nxt(0.5), D, "disparity = the float below 1")       # 1.5 - (0.5 + 2^-24) = 1 - 2^-24 exactly
    dsp(nxt(1.0), 0.0, K, "disparity = the float above 1")
    dsp(164.0, 164.0, D, "disparity = 0")
    dsp(196.0, 198.0, D, "disparity = -2")
    dsp(260.0, 259.5, D, "disparity = 0.5")
    dsp(420.0, 120.0, K, "disparity = 300 (the whole window)")
    for lvl in range(8):
        x = 32.0 * (10 + 2 * lvl) + 8.0
        fb.point(x, 208.0, (x - 6.0 - lvl / 16.0, 208.0), level=lvl, expect=K, name=f"level {lvl}")
    for k in range(3):  # distractors: no partner
        fb.point(32.0 * (40 + k) + 4.0, 272.0)
    return fb.build(f"point filters, max_dist_epip {t}", True)


def point_disp600_frame(seed, variant):
    """xl ~ 900, xr ~ 300: xl - xr rounds in float, and the float and the double difference fall on opposite sides of min_disp.  The float
    one is the reference (:159).  variant 0: min_disp = 600, variant 1: min_disp = 600 + 2.25 float steps."""
    fb = FrameBuilder(seed)
    K, D = st.KEPT, st.DISPARITY
    u = ULP600
    if variant == 0:
        # true difference 600 - u / 2: a tie, rounds to the even 600.0f -> kept; in double it is below 600
        fb.point(900.0, 80.0, (300.0 + u / 2, 80.0), expect=K, name="float 600.0 (kept), double 600 - u/2")
        fb.point(900.0, 144.0, (300.0 + u, 144.0), expect=D, name="600 - u in both")
        fb.point(900.0, 208.0, (300.0, 208.0), expect=K, name="600 in both")
    else:
        # true difference 600 + 2.5 u: a tie, rounds to the even 600 + 2 u -> below 600 + 2.25 u; in double it is above
        fb.point(900.0, 80.0, (300.0 - 2.5 * u, 80.0), expect=D, name="float 600 + 2u (dropped), double 600 + 2.5u")
        fb.point(900.0, 144.0, (300.0 - 3 * u, 144.0), expect=K, name="600 + 3u in both")
        fb.point(900.0, 208.0, (300.0 - 2 * u, 208.0), expect=D, name="600 + 2u in both")
    for v in (300.0 + u / 2, 300.0 - 2.5 * u):
        assert float(F32(v)) == v  # the right abscissae are floats
    return fb.build(f"points, min_disp near 600, variant {variant}", True)


# ---- line filters ------------------------------------------------------------------------------------------------------------------
YS, YE = 264.0, 392.0  # left rows of the vertical test lines: grid rows 8.25 .. 12.25


def line_filter_frame(seed):
    """Ratio, horizontal and overlap filters and the horizontal right line, on dyadic coordinates: every product and sum in front of a
    division is exact in double and the first re-intersection divides by a power of two, so every decision and every value has
    one answer in any evaluation order."""
    fb = FrameBuilder(seed)
    K, D, R, H = st.KEPT, st.DISPARITY, st.RATIO, st.HORIZONTAL
    col = iter(range(2, 62))

    def vert(ds, de, right_rows, expect, name, level=0, rev=False):
        """left: vertical, rows YS .. YE; right: vertical-ish through (x - ds at YS, x - de at YE), cut at right_rows"""
        x = 32.0 * next(col) + 4.0
        y0, y1 = right_rows
        xa = x - ds - (de - ds) * (y0 - YS) / (YE - YS)
        xb = x - ds - (de - ds) * (y1 - YS) / (YE - YS)
        r = (xb, y1, xa, y0) if rev else (xa, y0, xb, y1)
        assert all(float(F32(v)) == v for v in r)
        fb.line((x, YS, x, YE), r, level=level, expect=expect, name=name)

    same = (YS, YE)
    vert(10.0, 10.0, same, K, "equal disparities")
    vert(10.0, 7.0, same, K, "ratio 7 / 10 = 0.7 exactly, ds > de")
    vert(7.0, 10.0, same, K, "ratio 7 / 10 = 0.7 exactly, ds < de")
    vert(10.0, 6.9375, same, R, "ratio just below 0.7, ds > de")
    vert(6.9375, 10.0, same, R, "ratio just below 0.7, ds < de")
    vert(10.0, -3.0, same, R, "one disparity negative")
    vert(-10.0, -7.0, same, D, "both negative (ratio 10 / 7: not reset)")
    vert(-7.0, -7.0, same, D, "both negative and equal")
    vert(0.5, 0.5, same, D, "both below min_disp")
    vert(1.0, 1.0, same, K, "both exactly min_disp")
    vert(1.0, 0.9375, same, D, "one just below min_disp")
    for lvl in range(4):
        vert(8.0 + lvl, 8.0 + lvl, same, K, f"level {lvl}", level=lvl)
    # (stored end first with the left rows, the right end row IS the left start row: :367 divides by sp_l.y - ep_r.y = 0 — the quirk)
    vert(9.0, 9.0, same, D, "right line stored end first: 0 / 0 in the second re-intersection", rev=True)
    vert(9.0, 9.0, (YS + 1.0, YE + 1.0), K, "right line stored end first, one row lower", rev=True)
    # ---- the branches of the overlap (left rows 264 .. 392; the reference divides by eln - spn, not by the left span)
    vert(6.0, 6.0, (YE + 0.0625, YE + 64.0625), st.OV_DISJOINT, "right below left: disjoint")
    vert(6.0, 6.0, (YS - 64.0625, YS - 0.0625), st.OV_DISJOINT, "right above left: disjoint")
    vert(6.0, 6.0, (200.0, 456.0), st.OV_SPANS, "right spans left, 128 / 192 < 0.75")
    vert(6.0, 6.0, (260.0, 516.0), K, "right spans left, 128 / 132 > 0.75")
    vert(6.0, 6.0, (328.0, 456.0), K, "partial, 64 / 64: kept though half the left span")
    vert(6.0, 6.0, (200.0, 328.0), st.OV_PARTIAL, "partial, 64 / 192")
    vert(6.0, 6.0, (232.0, 360.0), st.OV_PARTIAL, "partial, 96 / 160 = 0.6")
    vert(6.0, 6.0, (248.0, 376.0), K, "partial, 112 / 144 = 0.78")
    vert(6.0, 6.0, (YS + 8.0, YS + 72.0), st.OV_PARTIAL, "right inside left, 64 / 120 = 0.53")
    vert(6.0, 6.0, (YS, YS + 64.0), st.OV_PARTIAL, "right inside left from its top, 64 / 128")
    vert(6.0, 6.0, (200.0, 456.0), st.OV_SPANS, "right spans left, stored end first", rev=True)
    vert(6.0, 6.0, (YE - 0.0078125, YE - 0.0078125 + 64.0), st.OV_SHORT, "eln - spn = 1 / 128 <= 0.01f")
    vert(6.0, 6.0, (YE - 0.015625, YE - 0.015625 + 64.0), K, "eln - spn = 1 / 64 > 0.01f: overlap 1")
    # ---- |sp_l.y - ep_l.y| around line_horiz_th = 0.1 (not a float): shallow lines in grid row 0 / 2
    f01 = F32(0.1)
    for k, (dy, expect) in enumerate([(float(f01), K), (float(nxt(f01, -1)), H), (float(nxt(f01, 1)), K), (0.125, K), (0.0625, H)]):
        xs = 100.0 + 300.0 * k  # all start in row 0: 0 + a float is that float
        fb.line((xs, 0.0, xs + 256.0, dy), (xs - 12.0, 0.0, xs + 244.0, dy), expect=expect, name=f"left rows differ by {dy!r}")
    # a left line with no row difference at all: both re-intersections fall on the same row, so it is short enough (32 of 100 pixels)
    # for the ratio filter, and its right partner is not horizontal (that case is below)
    fb.line((1700.0, 0.0, 1732.0, 0.0), (1600.0, 0.0, 1632.0, 0.5), expect=H, name="left rows equal")
    # ---- a horizontal right line: x / 0, 0 / 0, inf * 0 (left: shallow, rows y .. y + 4, so that the direction gate passes)
    for k, (yr, name) in enumerate([(2.0, "x / 0 in both re-intersections"), (0.0, "0 / 0 in the first"), (4.0, "inf * 0 in the second")]):
        xs, y = 1100.0 + 8.0 * k, 640.0 + 64.0 * k
        fb.line((xs, y, xs + 256.0, y + 4.0), (xs - 20.0, y + yr, xs + 236.0, y + yr), expect=D, name="horizontal right line: " + name)
    fb.line((1500.0, 900.0, 1500.0, 1028.0))  # distractor
    return fb.build("line filters", True)


def line_quirk_frame(seed):
    """Right end rows different from the left ones: :367 reads the sp_r that :366 has just overwritten.  Both points lie on the right
    line's support, so away from a degenerate denominator the quirk changes ep_r.x by roundings only; where the LEFT START ROW EQUALS
    THE RIGHT END ROW its denominator sp_l.y - ep_r.y is 0 and the pair is lost (0 / 0), while the repaired form keeps it.
    Coordinates on the 1/16 grid, right row difference 128: the first division is exact, the numerator of the second too."""
    fb = FrameBuilder(seed)
    rng = np.random.default_rng(seed + 1)
    g = lambda lo, hi: float(rng.integers(int(lo * 16), int(hi * 16) + 1)) / 16.0  # noqa: E731
    col = iter(range(2, 62))
    for k in range(28):
        x = 32.0 * next(col) + 8.0
        ys = 264.0 + g(0, 8); ye = ys + 128.0 + g(-4, 4)
        xe = x + g(-6, 6)
        o = g(-6, 6)
        if o == 0.0:
            o = 0.5
        yrs = ys + o; yre = yrs + 128.0
        d1, d2 = g(4, 24), g(4, 24)
        fb.line((x, ys, xe, ye), (x - d1, yrs, xe - d2, yre), name=f"random right rows {k}")
    for k in range(4):  # the verdict flips: the right line is stored end first and its end row is the left start row
        x = 32.0 * next(col) + 8.0
        ys = 272.0 + k; ye = ys + 128.0
        d = 8.0 + k
        fb.line((x, ys, x, ye), (x - d, ys + 128.0 - 2.0 * k, x - d, ys), name=f"left start row = right end row {k}")
    return fb.build("line quirk", True)


# ---- compaction shapes ---------------------------------------------------------------------------------------------------------------
POINT_COUNTS = [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048]
LINE_COUNTS = [1, 63, 64, 65, 255, 256, 257, 320]
PATTERNS = ["all", "none", "alternating", "last lane", "rows >= 1024", "random"]


def keep_pattern(pattern, n, rng):
    """-> (matched [n], kept [n]); a matched row that is not kept fails a filter"""
    i = np.arange(n)
    matched = np.ones(n, bool)
    if pattern == "all":
        kept = np.ones(n, bool)
    elif pattern == "none":
        kept = np.zeros(n, bool)
    elif pattern == "alternating":
        kept = (i & 1) == 0
    elif pattern == "last lane":
        kept = (i & 63) == 63
    elif pattern == "rows >= 1024":
        kept = i >= 1024
    else:  # a seeded random half, a third of the rows unmatched
        matched = rng.random(n) >= 1.0 / 3.0
        kept = matched & (rng.random(n) < 0.5)
    return matched, kept


def compaction_frame(seed, n_pts, n_lines, pattern_p, pattern_l, name):
    """n_pts key-points, one per grid cell, and n_lines vertical key-lines; a kept row's coordinates and descriptor carry its serial
    number, so a swap of two kept rows shows in the record.  kitti parameters (rows must be equal, disparity >= 1)."""
    fb = FrameBuilder(seed)
    rng = np.random.default_rng(seed + 7)
    matched, kept = keep_pattern(pattern_p, n_pts, rng)
    for i in range(n_pts):
        x = 32.0 * (1 + (i // 48) % 62) + 16.0 + (i % 5) / 16.0
        y = 32.0 * (i % 48) + 16.0 + (i % 3) / 16.0
        right = None
        if matched[i]:
            if kept[i]:
                right = (x - 4.0 - (i % 8) / 16.0, y)
            elif i & 1:
                right = (x - 4.0, y + 0.0625)  # epipolar
            else:
                right = (x - 0.5, y)            # disparity
        fb.point(x, y, right, level=i % 8, expect=(st.KEPT if kept[i] else (st.EPIPOLAR if i & 1 else st.DISPARITY)) if matched[i] else st.NONE)
    matched, kept = keep_pattern(pattern_l, n_lines, rng)
    for i in range(n_lines):
        x = 64.0 + 32.0 * (i % 60) + 8.0 + (i % 3) / 16.0
        y = 32.0 * (1 + 7 * (i // 60)) + 8.0
        right = None
        if matched[i]:
            if kept[i]:
                d = 8.0 + (i % 8) / 16.0
                right = (x - d, y, x - d, y + 128.0)
            elif i & 1:
                right = (x - 8.0, y, x - 2.0, y + 128.0)   # ratio
            else:
                right = (x - 0.5, y, x - 0.5, y + 128.0)   # disparity
        fb.line((x, y, x, y + 128.0), right, level=i % 4, expect=(st.KEPT if kept[i] else (st.RATIO if i & 1 else st.DISPARITY)) if matched[i] else st.NONE)
    return fb.build(name, True)


# ---- generic position --------------------------------------------------------------------------------------------------------------
# Chosen seeds (tests/test_stereo_tail_host.py asserts both properties for every one of them): the matcher returns the plan — the
# reference's Bresenham walk over grid cells may put a right line one column beyond its true abscissa, out of the window of a left
# line with a small disparity (seeds 13 and 18 have such a line) — and no decision is closer than a relative 1e-9 to its threshold.
GENERIC_SEEDS = [11, 12, 14]


def generic_frame(seed, n_pts=400, n_lines=120, cam=synth.KITTI_CAM):
    """Seeded random FLOAT coordinates on the KITTI camera (19.4 x 7.8 pixel cells, non-dyadic intrinsics): right key-point rows off by up
    to +-1.5 pixels inside their grid row, right key-lines on a support of their own with end rows off by up to +-3 pixels."""
    fb = FrameBuilder(seed)
    rng = np.random.default_rng(seed)
    W, H = cam["width"], cam["height"]
    ch = H / 48.0
    for i in range(n_pts):
        row = int(rng.integers(1, 47))
        yl = F32((row + rng.uniform(0.3, 0.7)) * ch)
        yr = F32(float(yl) + rng.uniform(-1.5, 1.5))
        assert int(float(yr) * 48.0 / H) == row == int(float(yl) * 48.0 / H)
        xl = F32(rng.uniform(80.0, W - 10.0))
        xr = F32(float(xl) - rng.uniform(0.2, 60.0))
        fb.point(xl, yl, (xr, yr) if rng.random() > 0.1 else None, level=int(rng.integers(0, 8)))
    for i in range(n_lines):
        ys = rng.uniform(10.0, H - 120.0); ye = ys + rng.uniform(50.0, 100.0)
        xs = rng.uniform(120.0, W - 60.0); xe = xs + rng.uniform(-15.0, 15.0)
        if rng.random() < 0.5:
            xs, ys, xe, ye = xe, ye, xs, ys
        left = tuple(F32(v) for v in (xs, ys, xe, ye))
        d1 = rng.uniform(0.5, 30.0)
        d2 = d1 * rng.uniform(0.55, 1.6)
        # the right end rows: never both drawn inwards, so that one left end row is covered by the right line's rows
        o1, o2 = rng.uniform(-3.0, 3.0), rng.uniform(-3.0, 3.0)
        sgn = 1.0 if ye > ys else -1.0
        if sgn * o1 > 0 and sgn * o2 < 0:
            o2 = -o2
        right = tuple(F32(v) for v in (xs - d1, ys + o1, xe - d2, ye + o2))
        fb.line(left, right if rng.random() > 0.1 else None, level=int(rng.integers(0, 4)))
    return fb.build(f"generic {seed}", False)


# ---- the sets ------------------------------------------------------------------------------------------------------------------------
def _set(name, cam, mp_kw, frames, K, M):
    return dict(name=name, cam=cam, mp_kw=mp_kw, mp=match_params("kitti", **mp_kw), frames=frames, K=K, M=M)


@functools.lru_cache(maxsize=None)
def filter_sets():
    """the sets of the well-defined edges and of the generic position: few features, one to three frames each"""
    return [
        _set("kitti", GRID_CAM, dict(), [point_filter_frame(101, 0.0), line_filter_frame(102), line_quirk_frame(103)], 512, 128),
        _set("euroc", GRID_CAM, dict(max_dist_epip=1.0), [point_filter_frame(111, 1.0)], 512, 128),
        _set("epip 0.3", GRID_CAM, dict(max_dist_epip=0.3), [point_filter_frame(121, 0.3)], 512, 128),
        _set("min_disp 600", WIDE_CAM, dict(min_disp=600.0), [point_disp600_frame(131, 0)], 512, 128),
        _set("min_disp 600 + 2.25 ulp", WIDE_CAM, dict(min_disp=600.0 + 2.25 * ULP600), [point_disp600_frame(141, 1)], 512, 128),
        _set("generic", synth.KITTI_CAM, dict(max_dist_epip=1.0), [generic_frame(s) for s in GENERIC_SEEDS], 512, 128),
    ]


@functools.lru_cache(maxsize=None)
def compaction_set(M=320):
    """every point count x every keep pattern (54 frames); the line counts and patterns cycle through them so that every line count
    meets every pattern too (8 x 6 = 48 <= 54)"""
    frames = []
    combos_l = [(n, p) for n in LINE_COUNTS for p in PATTERNS]
    k = 0
    for n in POINT_COUNTS:
        for p in PATTERNS:
            nl, pl = combos_l[k % len(combos_l)]
            frames.append(compaction_frame(1000 + k, n, nl, p, pl, f"compaction: {n} points '{p}', {nl} lines '{pl}'"))
            k += 1
    return _set(f"compaction M={M}", GRID_CAM, dict(), frames, 2048, M)


@functools.lru_cache(maxsize=None)
def persistent_set(B):
    """B small frames (B = CUs + 3 on the device: a persistent workgroup of the point matcher then runs the tail for two frames in a
    row); counts and keep patterns differ from frame to frame, so a count left over from a workgroup's first frame shows in its second"""
    frames = []
    for k in range(B):
        n = [65, 1, 64, 100, 63, 128][k % 6]
        nl = [17, 64, 1, 33][k % 4]
        frames.append(compaction_frame(5000 + k, n, nl, PATTERNS[k % 6], PATTERNS[(k + k // 6) % 6], f"persistent {k}"))
    return _set(f"persistent B={B}", GRID_CAM, dict(), frames, 128, 64)


# ---- the oracle's answer for a set, computed once and shared ---------------------------------------------------------------------------
_ORACLE = {}


def oracle_results(orc, cs):
    """[(orc_stereo_points, orc_stereo_lines) per frame] of the set; cached by the set's name, never modified by its users"""
    if cs["name"] not in _ORACLE:
        cam, mp, out = cs["cam"], cs["mp"], []
        for cf in cs["frames"]:
            f = cf["frame"]
            p = orc.stereo_points(f["kp_l"], f["oct_l"], f["desc_l"], f["kp_r"], f["desc_r"], cam["width"], cam["height"], cam, mp)
            l = orc.stereo_lines(f["kl_l"], np.zeros(len(f["kl_l"]), F32), f["oct_ll"], f["ldesc_l"], f["kl_r"], f["ldesc_r"],
                                 cam["width"], cam["height"], cam, mp)
            out.append((p, l))
        _ORACLE[cs["name"]] = out
    return _ORACLE[cs["name"]]


def safe_copy_sigma2(s2l, levels, mp):
    """LineFeature::safeCopy's second scaling of the constructor's sigma2 (stereoFeatures.cpp:117-135): what matched_ls carries"""
    return np.array([st.level_sigma2(s, mp.lsd_scale, lv) for s, lv in zip(s2l, levels)], np.float64)
