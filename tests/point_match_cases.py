"""Case frames for the stereo point matcher of the device pipeline (grid_points_fused_kernel and the scan formulation behind it,
stvo-pl_amd/csrc/grid_kernels.hip, with point_cells.h in front), shared by tests/test_point_match_host.py (CPU) and
tests/test_gpu_point_match.py — TEST INFRASTRUCTURE ONLY.

Every frame is built from a plan on GRID_CAM (a grid cell is 32 x 32 pixels, the pixel -> cell scale is the exact double 1 / 32)
with explicit index order; descriptors are the thermometer rows of tests/line_match_cases.py — the distance of therm(a) and therm(b)
is |a - b| —, or rows of two thermometers (`two(a, b)`: a in bits 0 .. 127, b in bits 128 .. 255, distance |a - a'| + |b - b'|), so
that every distance is a number chosen in the plan.  A PROBE is a few left and right key-points that meet; it has a grid row of its
own or lies more than matching_s_ws columns from the next probe.  Every case records which left rows carry which edge (`edges`: flag of
stereo_point_trace -> left rows) and, where the plan fixes it, the raw match (`expect`: left row -> right index or -1).

stereo_point_trace is the plain statement: src/matching.cpp:111-177 and src/gridStructure.cpp:56-76 of the reference, word for word in
Python, with flags.  It calls neither the oracle nor np_model.match_grid; the host test holds all three against each other."""
import functools

import numpy as np

import np_model
import np_stereo_tail
import pipeline_ref
from line_match_cases import bits_row, rand_desc, therm
from stereo_tail_cases import GRID_CAM
from stvo_amd.ctypes_types import match_params

F32 = np.float32
INT_MAX = 2 ** 31 - 1
COLS, ROWS = 64, 48
# the one-workgroup route's capacities, restated to PLAN the frames (the GPU tests read the route a frame took from the device)
WIDE_OVER, REG_ELIG, KEY_CAP, WIDE_QUEUE, SCAN_ELIG = 16, 4, 8192, 256, 16
SMALL_CAP = 24   # STVO_GRID_FUSED_CAP of the P5 frames whose narrow eligible pairs beyond four sum to C and to C + 1


def two(a, b):
    """[thermometer of a <= 128 bits | thermometer of b <= 128 bits]"""
    return np.concatenate([therm(a)[:16], therm(b)[:16]])


# ---- the plain statement, with a trace -----------------------------------------------------------------------------------------------
def cells_of(kp, cam):
    """(int)(float * double) per coordinate: truncation toward zero (stereoFrame.cpp:132, :138)"""
    kp = np.asarray(kp, F32).reshape(-1, 2)
    iw, ih = COLS / float(cam["width"]), ROWS / float(cam["height"])
    return np.stack([np.trunc(kp[:, 0].astype(np.float64) * iw), np.trunc(kp[:, 1].astype(np.float64) * ih)], axis=1).astype(np.int64)


def stereo_point_trace(f, cam, mp):
    """matchGrid over the left rows in ascending order, the candidates of a row in ASCENDING order.
    -> dict: m12 [nl]; cands (lists); per left row: n_cand, n_elig, best, second, skipped (candidates dropped by the `else continue`
    of :149), lost_mutual, single (exactly one eligible candidate), no_cand, none_eligible, on_edge (best == second * ratio in
    double), tie, refused (ratio test failed with two eligible candidates), outside (the left cell is not a grid cell);
    per right key-point: r_cand (left rows it is a candidate of), r_chain (eligible pairs), r_owner (matches_21), r_outside."""
    ws, ratio, lr = int(mp.matching_s_ws), float(mp.min_ratio_12_p_d), bool(mp.best_lr_matches)
    c1, c2 = cells_of(f["kp_l"], cam), cells_of(f["kp_r"], cam)
    nl, nr = len(c1), len(c2)
    grid = {}
    r_outside = np.zeros(nr, np.int64)
    for j, (x, y) in enumerate(c2.tolist()):    # GridStructure::at: outside the grid -> the out_of_bounds sink, which get() never reads
        if 0 <= x < COLS and 0 <= y < ROWS:
            grid.setdefault((x, y), []).append(j)
        else:
            r_outside[j] = 1
    names = ("n_cand", "n_elig", "best", "second", "skipped", "lost_mutual", "single", "no_cand", "none_eligible", "on_edge", "tie",
             "refused", "outside")
    t = {k: np.zeros(nl, np.int64) for k in names}
    r_cand, r_chain = np.zeros(nr, np.int64), np.zeros(nr, np.int64)
    D = np_model.hamming_matrix(f["desc_l"], f["desc_r"]) if nl and nr else np.zeros((nl, nr), np.int32)
    m12 = -np.ones(nl, np.int32)
    m21 = -np.ones(nr, np.int64)
    dist = np.full(nr, INT_MAX, np.int64)
    cands = []
    for i1, (x, y) in enumerate(c1.tolist()):
        t["outside"][i1] = int(not (0 <= x < COLS and 0 <= y < ROWS))
        cs = set()
        for xx in range(max(0, x - ws), min(COLS, x + 0 + 1)):      # GridStructure::get with {ws, 0} x {0, 0}
            for yy in range(max(0, y - 0), min(ROWS, y + 0 + 1)):
                cs.update(grid.get((xx, yy), ()))
        cs = sorted(cs)
        cands.append(cs)
        t["n_cand"][i1] = len(cs)
        t["no_cand"][i1] = int(not cs)
        best = second = INT_MAX
        best_idx = -1
        for i2 in cs:
            r_cand[i2] += 1
            d = int(D[i1, i2])
            if lr:
                if d < dist[i2]:
                    dist[i2] = d
                    m21[i2] = i1
                else:
                    t["skipped"][i1] += 1
                    continue
            t["n_elig"][i1] += 1
            r_chain[i2] += 1
            if d < best:
                second, best, best_idx = best, d, i2
            elif d < second:
                second = d
        t["best"][i1], t["second"][i1] = best, second
        t["single"][i1] = int(best < INT_MAX and second == INT_MAX)
        t["none_eligible"][i1] = int(bool(cs) and best == INT_MAX)
        t["tie"][i1] = int(best == second and best < INT_MAX)
        t["on_edge"][i1] = int(second < INT_MAX and float(best) == float(second) * ratio)
        if cs and float(best) < float(second) * ratio:
            m12[i1] = best_idx
        else:
            t["refused"][i1] = int(second < INT_MAX)
    if lr:
        for i1 in range(nl):
            if m12[i1] >= 0 and m21[m12[i1]] != i1:
                m12[i1] = -1
                t["lost_mutual"][i1] = 1
    t.update(m12=m12, cands=cands, r_cand=r_cand, r_chain=r_chain, r_owner=m21, r_outside=r_outside)
    return t


def demand(t):
    """what a frame asks of the one-workgroup route: (keys, wide right key-points); it misfits if keys > cap or wide > 256"""
    wide = t["r_cand"] > WIDE_OVER
    keys = int(t["r_cand"][wide].sum()) + int(np.maximum(t["r_chain"][~wide] - REG_ELIG, 0).sum())
    return keys, int(wide.sum())


def planned_misfit(t, cap=None):
    keys, wide = demand(t)
    cap = KEY_CAP if cap is None else min(cap, KEY_CAP)
    return int(keys > cap or wide > WIDE_QUEUE)


def planned_ovf(t, mp):
    return int(bool(mp.best_lr_matches) and len(t["r_chain"]) > 0 and int(t["r_chain"].max()) > SCAN_ELIG)


# ---- frames from a plan ----------------------------------------------------------------------------------------------------------------
def px(c, off=16.0):
    return 32.0 * c + off


class PointFrame:
    """left() / right() append in index order; later() defers calls to build(), so that a probe can put its last left row at the
    end of the frame."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.L, self.R, self.dl, self.dr = [], [], [], []
        self.edges, self.expect, self.deferred = {}, {}, []

    def unique(self):
        return rand_desc(self.rng, 1)[0]

    def left(self, x, y, desc, edges=(), expect=None):
        self.L.append((x, y)); self.dl.append(np.asarray(desc, np.uint8))
        i = len(self.L) - 1
        for e in edges:
            self.edges.setdefault(e, []).append(i)
        if expect is not None:
            self.expect[i] = expect
        return i

    def right(self, x, y, desc):
        self.R.append((x, y)); self.dr.append(np.asarray(desc, np.uint8))
        return len(self.R) - 1

    def later(self, fn):
        self.deferred.append(fn)

    def pair(self, xl, yl, xr, yr, edges=(), hit=True):
        """one left and one right key-point with the same unique descriptor: matched iff the right one is a candidate"""
        d = self.unique()
        j = self.right(xr, yr, d)
        return self.left(xl, yl, d, edges, j if hit else -1)

    def build(self, name):
        for fn in self.deferred:
            fn()
        nl, nr = len(self.L), len(self.R)
        z4, zd = np.zeros((0, 4), F32), np.zeros((0, 32), np.uint8)
        f = dict(kp_l=np.asarray(self.L, F32).reshape(nl, 2), oct_l=(np.arange(nl, dtype=np.int32) % 3),
                 desc_l=np.ascontiguousarray(np.asarray(self.dl, np.uint8).reshape(nl, 32)),
                 kp_r=np.asarray(self.R, F32).reshape(nr, 2), desc_r=np.ascontiguousarray(np.asarray(self.dr, np.uint8).reshape(nr, 32)),
                 kl_l=z4, kl_r=z4.copy(), ldesc_l=zd, ldesc_r=zd.copy(), oct_ll=np.zeros(0, np.int32), ang_l=np.zeros(0, F32))
        return dict(name=name, frame=f, edges={k: list(v) for k, v in self.edges.items()}, expect=dict(self.expect))


def slots():
    """places for small probes: columns 12, 28, 44, 60 of every grid row — 16 columns apart, more than any matching_s_ws here"""
    return iter([(x, r) for r in range(ROWS) for x in (12, 28, 44, 60)])


# ---- P1: windows -----------------------------------------------------------------------------------------------------------------------
def sees(xl, yl, xr, yr, ws):
    """the plan's own reading of gridStructure.cpp:56-76 for one left and one right CELL"""
    return 0 <= xr < COLS and 0 <= yr < ROWS and yl == yr and max(0, xl - ws) <= xr <= min(COLS - 1, xl)


def window_frame(ws, seed):
    fb = PointFrame(seed)
    row = iter(range(1, ROWS - 1))

    def probe(xl, yl, xr, yr, edges=()):
        """a pair in pixels; whether it meets is the plan's reading of the window, on the truncated cells"""
        hit = sees(int(xl / 32.0), int(yl / 32.0), int(xr / 32.0), int(yr / 32.0), ws)
        return fb.pair(xl, yl, xr, yr, tuple(edges) + (() if hit else ("no_cand",)), hit)

    # left cells at the grid's columns, the partner ws and ws + 1 columns to the left and in the same column
    for x in sorted({0, max(ws - 1, 0), ws, ws + 1, 62, 63}):
        for c in (x - ws, x - ws - 1, x):
            r = next(row)
            probe(px(x, 20.0), px(r), px(c, 4.0) if c >= 0 else -40.0 + 4.0 * c, px(r))   # left of the grid: the reference's sink
    # grid rows 0 and 47; the partner one grid row up or down is never a candidate
    probe(px(30, 20.0), px(0), px(30, 4.0), px(0))
    probe(px(58, 20.0), px(0), px(58, 4.0), px(1))
    probe(px(5, 20.0), px(47), px(5, 4.0), px(47))
    probe(px(30, 20.0), px(47), px(30, 4.0), px(46))
    # left key-points outside the image
    r = next(row); probe(-5.0, px(r), 4.0, px(r), ("outside_trunc",))                # x in (-32, 0): (int) truncates to cell 0
    r = next(row); probe(-31.5, px(r), 20.0, px(r), ("outside_trunc",))
    r = next(row); probe(-32.0, px(r), 4.0, px(r), ("outside",))                     # cell -1: the window is empty
    r = next(row); probe(-40.0, px(r), 4.0, px(r), ("outside",))
    r = next(row); probe(2048.0, px(r), px(63), px(r), ("outside",))                 # column 64: sees the last columns unless ws = 0
    r = next(row); probe(px(63 + ws), px(r), px(63), px(r), ("outside",) if ws else ())   # column 63 + ws: sees column 63 alone
    r = next(row); probe(px(63 + ws), px(r), px(62), px(r), ("outside",) if ws else ())
    r = next(row); probe(px(64 + ws), px(r), px(63), px(r), ("outside",))            # column 64 + ws: nothing
    probe(px(40, 20.0), -5.0, px(40, 4.0), 10.0, ("outside_trunc",))                 # y in (-32, 0): row 0
    probe(px(20, 20.0), -32.0, px(20, 4.0), 10.0, ("outside",))
    probe(px(52, 20.0), 1536.0, px(52, 4.0), px(47), ("outside",))                   # y >= height: row 48
    # right key-points outside the grid on each of the four sides: never a candidate, whatever they hold; (-32, 0) truncates INTO it
    r = next(row); probe(px(3, 20.0), px(r), -33.0, px(r), ("r_outside",))
    r = next(row); probe(px(63, 20.0), px(r), 2050.0, px(r), ("r_outside",))
    probe(px(10, 20.0), 10.0, px(10, 4.0), -40.0, ("r_outside",))
    probe(px(40, 20.0), px(47), px(40, 4.0), 1540.0, ("r_outside",))
    r = next(row); probe(px(0, 20.0), px(r), -5.0, px(r))
    # row 47, columns 67 .. 77: left key-points whose partner sits in column 63 at distance 3, and right key-points OUTSIDE the grid
    # that hold exactly their descriptors.  A matcher that looked their candidates up in the table of the left cells under cell -1
    # would read the words of (row 47, columns 67 .. 77) of the stream before — these very rows — and match them at distance 0.
    for k, c in enumerate((67, 70, 73, 77)):
        j = fb.right(px(63, 2.0 + k), px(47), therm(100 + 10 * k))
        placed = c <= 63 + ws
        fb.left(px(c), px(47), therm(103 + 10 * k), ("outside", "bait") + (() if placed else ("no_cand",)), j if placed else -1)
        fb.right((-40.0, 2060.0, px(c), px(c))[k], (px(47), px(47), -40.0, 1540.0)[k], therm(103 + 10 * k))
    return fb.build(f"P1 windows, ws {ws}, seed {seed}")


# ---- P2: ratio edges -------------------------------------------------------------------------------------------------------------------
RATIO_PAIRS = {0.75: [(3, 4), (3, 5), (2, 3), (6, 8), (5, 7), (0, 0), (0, 1), (191, 256), (192, 256)],
               0.9: [(9, 10), (8, 9), (18, 20), (17, 19), (230, 256), (231, 256)],
               1.0: [(3, 3), (3, 4)],
               0.8: [(8, 10), (4, 5), (12, 15)]}


def ratio_probes(fb, slot, ratio, lr=True):
    for best, second in RATIO_PAIRS[ratio]:
        for swap in (False, True):   # the best candidate at the lower and at the higher right index
            x, r = next(slot)
            d = (second, best) if swap else (best, second)
            js = [fb.right(px(x - 1), px(r), therm(d[0])), fb.right(px(x - 2), px(r), therm(d[1]))]
            edges = (("tie",) if best == second else ()) + (("on_edge",) if float(best) == float(second) * ratio else ())
            ok = float(best) < float(second) * ratio
            fb.left(px(x, 20.0), px(r), therm(0), edges + (() if ok else ("refused",)), js[1 if swap else 0] if ok else -1)
    x, r = next(slot)   # a single candidate at distance 256: best_d2 stays INT_MAX, accepted
    j = fb.right(px(x - 3), px(r), therm(256))
    fb.left(px(x, 20.0), px(r), therm(0), ("single",), j)
    x, r = next(slot)   # no candidate
    fb.left(px(x, 20.0), px(r), therm(7), ("no_cand",), -1)
    # three eligible candidates of which only the THIRD in index order breaks the ratio (6 against 7), in every order of the three;
    # and the same with 9 in its place, which keeps it for every ratio here but 0.75 <= 6 / 9
    for third in (7, 9):
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            x, r = next(slot)
            ds = [(6, 20, third)[k] for k in order]
            js = [fb.right(px(x - 1 - k), px(r), therm(d)) for k, d in enumerate(ds)]
            ok = float(6) < float(third) * ratio
            fb.left(px(x, 20.0), px(r), therm(0), ("three",) + (() if ok else ("refused",)), js[ds.index(6)] if ok else -1)


def ratio_frame(ratio, seed):
    fb = PointFrame(seed)
    ratio_probes(fb, slots(), ratio)
    return fb.build(f"P2 ratio edges at {ratio}")


# ---- P3: order dependence -----------------------------------------------------------------------------------------------------------------
def order_probes(fb, slot, lr, far):
    """rows that share a right key-point R0 one column to the left of the first of them; R1, in the column of the second row, is seen by
    the second and third rows only.  far: the rows after the first are appended when the frame is built, i.e. at its end."""
    def group(lefts, rights):
        """lefts: (column offset, thermometer value, edges, expect with best_lr on, expect with it off) — expectations name rights by
        their position in `rights`: (column offset, value)"""
        x, r = next(slot)
        js = [fb.right(px(x + dx, 4.0), px(r), therm(v)) for dx, v in rights]

        def add(k):
            dx, v, e, on, off = lefts[k]
            exp = on if lr else off
            fb.left(px(x + dx, 20.0), px(r), therm(v), e if lr else (), -1 if exp is None else js[exp])
        add(0)
        for k in range(1, len(lefts)):
            if far:
                fb.later(lambda k=k: add(k))
            else:
                add(k)

    # equal distances 20, 20: the later row skips R0 entirely — also as a second best, where 20 against its 18 to R1 would fail the
    # ratio test — and so matches its other candidate
    group([(0, 80, (), 0, 0), (1, 120, ("skipped", "single"), 1, None)], [(-1, 100), (1, 138)])
    # ... three rows, the last two without another candidate
    group([(0, 80, (), 0, 0), (1, 120, ("skipped", "none_eligible"), None, 0), (2, 80, ("skipped", "none_eligible"), None, 0)], [(-1, 100)])
    # strictly descending 30, 20, 10: every row takes R0, the last one owns it
    group([(0, 70, ("lost_mutual",), None, 0), (1, 80, ("lost_mutual",), None, 0), (2, 90, (), 0, 0)], [(-1, 100)])
    group([(0, 70, ("lost_mutual",), None, 0), (1, 90, (), 0, 0)], [(-1, 100)])
    # ascending 10, 20, 30: only the first row ever sees it
    group([(0, 90, (), 0, 0), (1, 80, ("skipped",), None, 0), (2, 70, ("skipped",), None, 0)], [(-1, 100)])
    # a row whose best is later taken by a row that itself fails the ratio test (10 against 12): both end at -1
    group([(0, 80, ("lost_mutual",), None, 0), (1, 110, ("refused",), None, None)], [(-1, 100), (1, 122)])
    # interleaved: two rights, four rows
    group([(0, 10, ("refused",), None, None), (1, 30, ("refused",), None, None), (2, 44, ("lost_mutual",), None, 1), (3, 47, (), 1, 1)],
          [(-1, 50), (-2, 46)])


def order_frame(lr, far, seed, planned=True):
    """planned=False: a set with another ratio than 0.75 — the expectations and edges of the plan do not hold, the three statements
    still judge the frame"""
    fb = PointFrame(seed)
    slot = slots()
    order_probes(fb, slot, lr, far)
    if far:   # something between the first rows and the rest
        for _ in range(20):
            x, r = next(slot)
            fb.pair(px(x, 20.0), px(r), px(x - 3), px(r))
    out = fb.build(f"P3 order dependence, rows {'far apart' if far else 'adjacent'}")
    if not planned:
        out["edges"], out["expect"] = {}, {}
    return out


# ---- P4: counts ------------------------------------------------------------------------------------------------------------------------------
def chain_probe(fb, r, n, e, decisive, ws=10, c=20):
    """Grid row r: the right key-point R in cell c with n candidates — left rows spread over the cells c .. c + ws — of which the
    first e are its eligible chain (distances 70, 68, .. strictly descending over ascending left index; the other n - e stand at the
    chain's last distance and are skipped).  decisive: the chain's LAST pair decides a ratio test — that left row has a second right
    key-point Q (same cell) one bit nearer than R, so it is refused, (v - 1) against v; every earlier row of the chain has Q as an
    eligible second candidate far behind R.  Only the owner of R can match: the chain's last row, unless it is the refused one."""
    v = [70 - 2 * i for i in range(e)]
    jr = fb.right(px(c, 2.0), px(r), two(0, 0))
    jq = None
    if decisive:
        q = 2 * v[-1] - 1
        assert e >= 4 and q <= 128
        jq = fb.right(px(c, 3.0), px(r), two(0, q))
    for i in range(n):
        x = px(c + (i * (ws + 1)) // max(n, 1), 8.0 + (i % 23))
        if i < e:
            last = i == e - 1
            desc = two(0, v[i]) if (decisive and last) else two(v[i], 0)
            edges = ("chain",) + (("refused", "decisive") if decisive and last else ()) + (("lost_mutual",) if not last else ())
            fb.left(x, px(r), desc, edges, -1 if (decisive and last) or not last else jr)
        else:
            fb.left(x, px(r), two(v[-1], 0), ("skipped", "none_eligible"), -1)
    return jr, jq


P4_NARROW = [(0, 0, False), (1, 1, False), (4, 4, False), (15, 4, True), (15, 5, True), (16, 5, False), (16, 16, True), (16, 1, False)]
P4_WIDE = [(17, 1, False), (17, 4, False), (17, 5, True), (63, 16, True), (64, 5, True), (65, 16, False), (129, 4, True)]
P4_OVF = [(17, 17, True), (65, 17, False), (129, 17, True), (16, 16, True)]


def count_frame(plan, seed, name, riders=True):
    fb = PointFrame(seed)
    keys = {}
    for k, (n, e, dec) in enumerate(plan):
        jr, jq = chain_probe(fb, 2 + 2 * k, n, e, dec)
        keys[jr] = (n, e)
        if jq is not None:   # Q: every row of the chain is an eligible pair of its own, the last one its owner
            keys[jq] = (n, e)
    if riders:   # probes of P2 / P3 in the rows below: whatever route the frame takes is judged on content ("order": P3 alone)
        slot = iter([(x, r) for r in range(2 + 2 * len(plan), ROWS) for x in (12, 28, 44, 60)])
        order_probes(fb, slot, True, False)
        if riders is True:
            ratio_probes(fb, slot, 0.75)
    out = fb.build(name)
    out["right_counts"] = keys   # right index -> (candidates, eligible pairs) as planned
    return out


# ---- P5: capacities of the one-workgroup route ---------------------------------------------------------------------------------------
def crowd_frame(n_left, n_right, seed, name, c=20, r=30, ws=10):
    """n_left left key-points in the cells c .. c + ws of one grid row, n_right right key-points in the cell c: every right key-point
    has all n_left candidates.  Descriptors: about half of the right rows are left rows with a few bits flipped."""
    fb = PointFrame(seed)
    rng = fb.rng
    dl = rand_desc(rng, n_left)
    for i in range(n_left):
        fb.left(px(c + (i * (ws + 1)) // n_left, 8.0 + (i % 23)), px(r), dl[i])
    for j in range(n_right):
        d = rand_desc(rng, 1)[0]
        if j % 2 == 0:
            d = dl[int(rng.integers(n_left))] ^ bits_row(int(rng.integers(0, 250)), int(rng.integers(0, 4)))
        fb.right(px(c, 1.0 + (j % 29)), px(r), d)
    slot = iter([(x, rr) for rr in range(0, 24) for x in (12, 28, 44, 60)])
    order_probes(fb, slot, True, False)
    ratio_probes(fb, slot, 0.75)
    return fb.build(name)


def narrow_sum_frame(extra, seed, riders=True):
    """narrow right key-points only, whose eligible pairs beyond the four in registers sum to `extra`"""
    plan, left = [], extra
    while left > 0:
        e = min(16, 4 + left)
        plan.append((e, e, False))
        left -= e - 4
    return count_frame(plan, seed, f"P5 narrow right key-points, {extra} eligible pairs beyond four", riders)


TINY_CAP = 4   # ... and of the two frames of at most 64 key-points of the many-frames-per-workgroup test


@functools.lru_cache(maxsize=None)
def tiny_cap_frames():
    out = [narrow_sum_frame(TINY_CAP, 47, "order"), narrow_sum_frame(TINY_CAP + 1, 48, "order")]
    assert all(max(len(cf["frame"]["kp_l"]), len(cf["frame"]["kp_r"])) <= 64 for cf in out)
    return out


# ---- P6: the index range ---------------------------------------------------------------------------------------------------------------------
def range_frame(n, seed):
    """n left and n right key-points (n = 2048: the most the one-workgroup route takes).  Left row n - 1 and the last scan position —
    the right key-points of the grid's last cell — carry the probe (0, 256): the left row therm(0) against therm(0) and therm(256);
    left row 0 has its single candidate at distance 256."""
    fb = PointFrame(seed)
    rng = fb.rng
    j = fb.right(px(20), px(0), therm(256))
    fb.left(px(22, 20.0), px(0), therm(0), ("single",), j)
    for _ in range(n - 3):   # pairs anywhere in the rows 2 .. 45, the partner 40 pixels to the left
        x, y = float(rng.uniform(60.0, 2040.0)), float(rng.uniform(70.0, 1460.0))
        d = rand_desc(rng, 1)[0]
        fb.right(x - 40.0, y, d)
        fb.left(x, y, d)
    ja = fb.right(px(63, 2.0), px(47), therm(0))
    fb.right(px(63, 3.0), px(47), therm(256))
    fb.left(px(40, 20.0), px(47), therm(3), ("no_cand",), -1)
    fb.left(px(63, 20.0), px(47), therm(0), ("last_row",), ja)
    out = fb.build(f"P6 index range, {n} x {n} key-points")
    assert len(out["frame"]["kp_l"]) == n and len(out["frame"]["kp_r"]) == n
    return out


def tiny_frame(n, seed):
    fb = PointFrame(seed)
    for k in range(n):
        fb.pair(px(30 + k, 20.0), px(10), px(28 + k), px(10))
    return fb.build(f"{n} key-points")


# ---- the sets ----------------------------------------------------------------------------------------------------------------------------------
def _set(name, frames, mp_kw=None, K=512, cap=None):
    return dict(name=name, cam=GRID_CAM, mp=match_params("kitti", **dict(mp_kw or {})), frames=frames, K=K, M=64, cap=cap)


@functools.lru_cache(maxsize=None)
def point_sets():
    sets = []
    for ws in (10, 0, 16, 17):
        sets.append(_set(f"P1 windows ws={ws}", [window_frame(ws, 11), window_frame(ws, 12), window_frame(ws, 11)], dict(matching_s_ws=ws), K=128))
    sets.append(_set("P2+P3 kitti", [ratio_frame(0.75, 21), order_frame(True, False, 22), order_frame(True, True, 23)], K=256))
    sets.append(_set("P2+P3 kitti, best_lr off", [ratio_frame(0.75, 21), order_frame(False, False, 22), order_frame(False, True, 23)],
                     dict(best_lr_matches=0), K=256))
    sets.append(_set("P2 ratio 0.9", [ratio_frame(0.9, 24), order_frame(True, False, 22, False)], dict(min_ratio_12_p=0.9), K=256))
    sets.append(_set("P2 ratio 1.0", [ratio_frame(1.0, 25), order_frame(True, True, 23, False)], dict(min_ratio_12_p=1.0), K=256))
    sets.append(_set("P2 ratio 0.8 (double)", [ratio_frame(0.8, 26)], dict(min_ratio_12_p=0.8), K=256))
    sets.append(_set("P4 counts", [count_frame(P4_NARROW, 31, "P4 narrow right key-points"), count_frame(P4_WIDE, 32, "P4 wide right key-points"),
                                   count_frame(P4_OVF, 33, "P4 chains of 17")], K=512))
    sets.append(_set("P5 queue 256 / 257", [crowd_frame(17, 256, 41, "P5 256 right key-points with 17 candidates"),
                                            crowd_frame(17, 257, 42, "P5 257 right key-points with 17 candidates")], K=384))
    sets.append(_set("P5 keys 8192 / 8256", [crowd_frame(128, 64, 43, "P5 64 right key-points share 128 candidates"),
                                             crowd_frame(129, 64, 44, "P5 64 right key-points share 129 candidates")], K=256))
    sets.append(_set(f"P5 narrow sums, cap {SMALL_CAP}", [narrow_sum_frame(SMALL_CAP, 45), narrow_sum_frame(SMALL_CAP + 1, 46)], K=256, cap=SMALL_CAP))
    sets.append(_set("P6 index range", [range_frame(2048, 51)], K=2048))
    return sets


SMALL_SETS = ["P1 windows ws=10", "P2+P3 kitti", "P2 ratio 0.8 (double)"]   # run again in larger capacities


def get_set(name):
    return [s for s in point_sets() if s["name"] == name][0]


@functools.lru_cache(maxsize=None)
def cycle_frames():
    """the frames of P2 - P5 (kitti parameters) in one order, with an empty frame, a one-point frame, a natural misfit and a 257-wide
    frame interleaved: cycled over more streams than the device has compute units"""
    fr = []
    for name in ("P2+P3 kitti", "P4 counts", "P5 queue 256 / 257", "P5 keys 8192 / 8256", f"P5 narrow sums, cap {SMALL_CAP}"):
        fr += get_set(name)["frames"]
    wide257 = get_set("P5 queue 256 / 257")["frames"][1]
    misfit = get_set("P5 keys 8192 / 8256")["frames"][1]
    out = []
    for k, f in enumerate(fr):
        out.append(f)
        if k % 4 == 1:   # (the first of them a misfit, third in the cycle)
            out.append((misfit, tiny_frame(0, 61), tiny_frame(1, 62), wide257)[(k // 4) % 4])
    if len(out) % 2 == 0:   # an odd length: a workgroup that takes streams w, w + 256, .. then never meets the same frame twice in a row
        out.append(order_frame(True, True, 23))
    return out


_RES = {}


def results(orc, cs):
    """[(oracle raw matches, np_model raw matches, trace, what np_stereo_tail keeps) per frame], computed once per set"""
    if cs["name"] not in _RES:
        _RES[cs["name"]] = [frame_result(orc, cf, cs["cam"], cs["mp"]) for cf in cs["frames"]]
    return _RES[cs["name"]]


_FRAME_RES = {}


def frame_result(orc, cf, cam, mp):
    key = (cf["name"], int(mp.matching_s_ws), float(mp.min_ratio_12_p_d), int(mp.best_lr_matches))
    if key not in _FRAME_RES:
        f = cf["frame"]
        t = stereo_point_trace(f, cam, mp)
        ref = pipeline_ref.stereo_frame(orc, f, cam, mp, True, False)["m12_raw_p"]
        if len(f["kp_l"]) and len(f["kp_r"]):
            mdl = np_model.match_grid(t["cands"], f["desc_l"], f["desc_r"], float(mp.min_ratio_12_p_d), bool(mp.best_lr_matches))
        else:
            mdl = -np.ones(len(f["kp_l"]), np.int32)
        tail = np_stereo_tail.stereo_points(f["kp_l"], f["oct_l"], f["kp_r"], t["m12"], cam, mp)
        _FRAME_RES[key] = (ref, mdl, t, tail)
    return _FRAME_RES[key]
