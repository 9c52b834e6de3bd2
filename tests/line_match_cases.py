"""Case frames for the two key-line matchers of the device pipeline, shared by tests/test_line_match_host.py (CPU) and
tests/test_gpu_line_match.py — TEST INFRASTRUCTURE ONLY.

Stereo cases (line_stereo_fused_kernel and the general grid matcher behind it) are judged on the raw match indices of the FIRST
step of a Sequences object, which only builds the stereo sets: no pose kernel runs on them.  Every frame is built from a plan on
GRID_CAM (a grid cell is 32 x 32 pixels) with explicit index order; descriptors are "thermometer" rows — therm(k) has its k lowest
bits set, so the distance of therm(a) and therm(b) is |a - b| — and every probe (a few left and right lines that meet) has grid rows
of its own or lies more than matching_s_ws columns from the next one.  Every case records which left rows carry which edge
(`edges`: flag of stereo_trace -> rows) and, where the plan fixes it, the match (`expect`: row -> right index or -1).

Frame-to-frame cases (match_small_kernel and the general machinery behind it) need stereo sets whose content and order are known:
the SEPARATED layout gives every left line exactly one stereo candidate, its partner 40 pixels to the left with the same
descriptor, so the kept set of a frame is its left descriptor rows in left order whatever they hold.  A stream pushes frame A (the
previous set, the query rows) and then frame B (the current set, the train rows); both carry ~300 ordinary key-points of one
synth sequence, so optimizePose of the tracked step runs on sane records."""
import functools

import numpy as np

import np_model
import pipeline_ref
from stereo_tail_cases import GRID_CAM
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params

F32 = np.float32
INT_MAX = 2 ** 31 - 1
COLS, ROWS = 64, 48
COUNTS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 128, 129, 255, 256, 257, 511, 512]
F2F_SIZES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128]


# ---- descriptors -----------------------------------------------------------------------------------------------------------------
def bits_row(lo, k):
    """256-bit row with bits lo .. lo + k - 1 set"""
    b = np.zeros(256, np.uint8)
    b[lo:lo + k] = 1
    return np.packbits(b, bitorder="little")


def therm(k):
    return bits_row(0, k)


def rand_desc(rng, n, entropy_bits=256):
    d = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    if entropy_bits < 256:  # entropy-starved rows: many distance ties, as LBD descriptors have
        keep = np.zeros(32, np.uint8)
        keep[: entropy_bits // 8] = 0xFF
        d &= keep
    return d


def coded(code, k):
    """[16 bytes cluster code | thermometer of k <= 128 bits]: rows of one cluster differ by |ka - kb|, rows of two clusters by the
    distance of their codes (~64) at least"""
    return np.concatenate([code, therm(k)[:16]])


# ---- points ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def point_frames(cam_key, seed):
    cam = dict(cam_key)
    return synth.make_stereo_sequence(seed, n_frames=2, n_pts=250, n_lines=0, cam=cam)


def with_points(cam, seed, step, kl_l, ldesc_l, kl_r, ldesc_r):
    base = point_frames(tuple(sorted(cam.items())), seed)[step]
    f = {k: base[k] for k in ("kp_l", "oct_l", "desc_l", "kp_r", "desc_r")}
    kl_l = np.asarray(kl_l, F32).reshape(-1, 4); kl_r = np.asarray(kl_r, F32).reshape(-1, 4)
    f.update(kl_l=kl_l, kl_r=kl_r, ldesc_l=np.ascontiguousarray(np.asarray(ldesc_l, np.uint8).reshape(-1, 32)),
             ldesc_r=np.ascontiguousarray(np.asarray(ldesc_r, np.uint8).reshape(-1, 32)), oct_ll=np.zeros(len(kl_l), np.int32),
             ang_l=np.arctan2(kl_l[:, 3] - kl_l[:, 1], kl_l[:, 2] - kl_l[:, 0]).astype(F32))
    return f


# ---- the plain statement of the stereo line association, with a trace ------------------------------------------------------------------
def right_dir(kl, iw, ih):
    """unit direction of a right line in grid units: FLOAT difference of the end points, then double (stereoFrame.cpp:331)"""
    vx = float(F32(kl[2]) - F32(kl[0])) * iw
    vy = float(F32(kl[3]) - F32(kl[1])) * ih
    with np.errstate(all="ignore"):
        mag = np.sqrt(np.float64(vx * vx + vy * vy))
        return np.float64(vx) / mag, np.float64(vy) / mag


def stereo_trace(orc, f, cam, mp):
    """Windows (GridStructure::get with {ws, 0, 0, 0}), the oracle's Bresenham cells, the direction gate and matchGrid's loop with the
    candidates in ASCENDING order, flag by flag.  -> dict: cands (lists), gate (callable), flags as arrays over the left rows."""
    iw, ih = COLS / float(cam["width"]), ROWS / float(cam["height"])
    ws, th, ratio, lr = mp.matching_s_ws, mp.line_sim_th, mp.min_ratio_12_p_d, bool(mp.best_lr_matches)
    kl_l, kl_r = f["kl_l"], f["kl_r"]
    nl, nr = len(kl_l), len(kl_r)
    c1 = np.zeros((nl, 4), np.int64)
    for k in range(4):
        c1[:, k] = np.trunc(kl_l[:, k].astype(np.float64) * (iw if k % 2 == 0 else ih)).astype(np.int64)
    cover = np.zeros((ROWS, COLS, max(nr, 1)), bool)   # right line j has a cell (x, y)
    clipped_r = np.zeros(nr, bool)
    dir2 = np.zeros((nr, 2))
    for j in range(nr):
        k = kl_r[j].astype(np.float64)
        cells = orc.line_coords(k[0] * iw, k[1] * ih, k[2] * iw, k[3] * ih)
        inb = (cells[:, 0] >= 0) & (cells[:, 0] < COLS) & (cells[:, 1] >= 0) & (cells[:, 1] < ROWS)
        clipped_r[j] = not inb.all()
        cover[cells[inb, 1], cells[inb, 0], j] = True
        dir2[j] = right_dir(kl_r[j], iw, ih)
    nan_r = np.isnan(dir2).any(axis=1)
    with np.errstate(all="ignore"):
        v = (c1[:, 2:] - c1[:, :2]).astype(np.float64)
        dir1 = v / np.sqrt((v * v).sum(axis=1))[:, None]

    def window(x, y):
        lo, hi = max(0, x - ws), min(COLS, x + 1)
        if not (0 <= y < ROWS) or lo >= hi:
            return None
        return lo, hi

    def gate(i1, i2):
        with np.errstate(all="ignore"):
            return not (abs(dir1[i1] @ dir2[i2]) < th)

    names = ("nan_l", "win_absent", "win_clipped", "start_only", "end_only", "gated", "gate_margin", "nan_r_cand", "clipped_r_cand",
             "run_equal", "run_greater", "run_taken", "tie", "on_edge", "single", "none_eligible", "no_cand", "best", "second", "n_cand")
    t = {k: np.zeros(nl, np.float64 if k == "gate_margin" else np.int64) for k in names}
    t["gate_margin"][:] = np.inf
    D = np_model.hamming_matrix(f["ldesc_l"], f["ldesc_r"]) if nl and nr else np.zeros((nl, nr), np.int32)
    dist = np.full(nr, INT_MAX, np.int64)
    cands = []
    for i in range(nl):
        per_end = []
        for x, y in ((c1[i, 0], c1[i, 1]), (c1[i, 2], c1[i, 3])):
            w = window(int(x), int(y))
            if w is None:
                t["win_absent"][i] += 1
                per_end.append(set())
                continue
            if x - ws < 0 or x > COLS - 1:
                t["win_clipped"][i] += 1
            per_end.append(set(np.nonzero(cover[y, w[0]:w[1]].any(axis=0))[0].tolist()) if nr else set())
        cs = sorted(per_end[0] | per_end[1])
        cands.append(cs)
        t["nan_l"][i] = int(np.isnan(dir1[i]).any())
        t["n_cand"][i] = len(cs)
        t["no_cand"][i] = int(not cs)
        t["start_only"][i] = len(per_end[0] - per_end[1]); t["end_only"][i] = len(per_end[1] - per_end[0])
        best = second = INT_MAX
        n_gate_ok = 0
        for j in cs:
            with np.errstate(all="ignore"):
                dot = abs(dir1[i] @ dir2[j])
            if not np.isnan(dot):
                t["gate_margin"][i] = min(t["gate_margin"][i], abs(dot - th))
            t["nan_r_cand"][i] += int(nan_r[j]); t["clipped_r_cand"][i] += int(clipped_r[j])
            if dot < th:
                t["gated"][i] += 1
                continue
            n_gate_ok += 1
            d = int(D[i, j])
            if lr:
                if d < dist[j]:
                    t["run_taken"][i] += int(dist[j] != INT_MAX)
                    dist[j] = d
                else:
                    t["run_equal" if d == dist[j] else "run_greater"][i] += 1
                    continue
            if d < best:
                best, second = d, best
            elif d < second:
                second = d
        t["best"][i], t["second"][i] = best, second
        t["tie"][i] = int(best == second and best < INT_MAX)
        t["on_edge"][i] = int(second < INT_MAX and float(best) == float(second) * ratio)
        t["single"][i] = int(best < INT_MAX and second == INT_MAX)
        t["none_eligible"][i] = int(n_gate_ok > 0 and best == INT_MAX)
    t.update(cands=cands, gate=gate)
    return t


def stereo_expect(orc, f, cam, mp):
    """(the oracle's raw matches, np_model.match_grid on the plain candidate lists — visited in REVERSED order —, the trace)"""
    t = stereo_trace(orc, f, cam, mp)
    full = pipeline_ref.stereo_frame(orc, f, cam, mp, False, True)
    ref = full["m12_raw_l"]
    t["kept_ldesc"] = full["ldesc"]   # the descriptor rows of the stereo set the oracle builds from these matches
    if len(f["kl_l"]) and len(f["kl_r"]):
        mdl = np_model.match_grid(t["cands"], f["ldesc_l"], f["ldesc_r"], mp.min_ratio_12_p_d, bool(mp.best_lr_matches), t["gate"])
    else:
        mdl = -np.ones(len(f["kl_l"]), np.int32)
    return ref, mdl, t


# ---- stereo frames from a plan ---------------------------------------------------------------------------------------------------------
def cell_dot(x, r):
    """a short vertical line inside cell (x, r): as a left line its direction is NaN, as a right line it covers that one cell"""
    return (32.0 * x + 16.0, 32.0 * r + 4.0, 32.0 * x + 16.0, 32.0 * r + 28.0)


def cell_vert(x, r):
    """a vertical line through the cells (x, r) and (x, r + 1)"""
    return (32.0 * x + 16.0, 32.0 * r + 8.0, 32.0 * x + 16.0, 32.0 * r + 56.0)


class LineFrame:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.seed = seed
        self.L, self.R, self.dl, self.dr = [], [], [], []
        self.edges, self.expect = {}, {}

    def unique(self):
        return rand_desc(self.rng, 1)[0]

    def left(self, xy, desc, edges=(), expect=None):
        self.L.append(xy); self.dl.append(desc)
        i = len(self.L) - 1
        for e in edges:
            self.edges.setdefault(e, []).append(i)
        if expect is not None:
            self.expect[i] = expect
        return i

    def right(self, xy, desc):
        self.R.append(xy); self.dr.append(desc)
        return len(self.R) - 1

    def probe(self, left_xy, right_xy, edges=(), hit=True):
        """one left and one right line with the same unique descriptor, alone in their grid rows: matched iff the right line is a
        candidate that the gate lets through"""
        d = self.unique()
        j = self.right(right_xy, d)
        return self.left(left_xy, d, edges, j if hit else -1)

    def build(self, name, cam=GRID_CAM):
        f = with_points(cam, 9000 + self.seed, 0, self.L, self.dl, self.R, self.dr)
        return dict(name=name, frame=f, edges={k: list(v) for k, v in self.edges.items()}, expect=dict(self.expect))


def window_frames(ws=10):
    """S1: the window arithmetic at columns 0 and 63 and outside the grid; one probe per grid row"""
    frames = []
    fb = LineFrame(1); row = iter(range(ROWS))
    for x in (0, 1, ws - 1, ws, ws + 1, 62, 63):
        lo, hi = max(x - ws, 0), min(x, COLS - 1)
        for c, hit in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
            r = next(row)
            if c < 0:     # the right line lies wholly left of the grid: every cell of its run is dropped
                fb.probe(cell_dot(x, r), (-60.0, 32.0 * r + 4.0, -40.0, 32.0 * r + 28.0), ("nan_l", "no_cand") + (("win_clipped",) if x < ws else ()), False)
            elif c > 63:  # ... wholly right of it
                fb.probe(cell_dot(x, r), (2088.0, 32.0 * r + 4.0, 2100.0, 32.0 * r + 28.0), ("nan_l", "no_cand"), False)
            else:
                fb.probe(cell_dot(x, r), cell_dot(c, r), ("nan_l",) + (("win_clipped",) if x < ws else ()) + (() if hit else ("no_cand",)), hit)
    frames.append(fb.build("S1 window edges: run ends at lo - 1, lo, hi, hi + 1"))

    fb = LineFrame(2); band = iter(range(0, ROWS - 2, 2))
    for x0, x1, c in ((30, 42, 33), (5, 20, 12), (63, 50, 45)):   # reached only through the END point's window (row r + 1)
        r = next(band)
        dx = x1 - x0
        left = (32.0 * x0 + 16.0, 32.0 * r + 16.0, 32.0 * x1 + 16.0, 32.0 * r + 48.0)
        right = (32.0 * c + 16.0 - dx, 32.0 * (r + 1) + 15.0, 32.0 * c + 16.0 + dx, 32.0 * (r + 1) + 17.0)   # parallel, inside one cell
        fb.probe(left, right, ("end_only",), True)
    for x0, x1, c in ((42, 30, 33), (20, 5, 12), (50, 63, 45)):   # ... only through the START point's (row r)
        r = next(band)
        dx = x1 - x0
        left = (32.0 * x0 + 16.0, 32.0 * r + 16.0, 32.0 * x1 + 16.0, 32.0 * r + 48.0)
        right = (32.0 * c + 16.0 - abs(dx), 32.0 * r + 16.0 - np.sign(dx), 32.0 * c + 16.0 + abs(dx), 32.0 * r + 16.0 + np.sign(dx))
        fb.probe(left, right, ("start_only",), True)
    # left coordinates at -1 px: (int) truncates toward zero, cell 0 in both axes
    r = next(band)
    fb.probe((-1.0, 32.0 * r + 4.0, -1.0, 32.0 * r + 28.0), cell_dot(0, r), ("nan_l", "win_clipped"), True)
    fb.probe((400.0, -1.0, 400.0, -0.5), cell_dot(12, 0), ("nan_l",), True)
    # at -40 px (cell -1), at width + 40 (cell 65: columns 55 .. 63), rows -1 and 49: no window
    r = next(band)
    fb.probe((-40.0, 32.0 * r + 4.0, -40.0, 32.0 * r + 28.0), cell_dot(0, r), ("win_absent", "no_cand"), False)
    r = next(band)
    fb.probe((2088.0, 32.0 * r + 4.0, 2088.0, 32.0 * r + 28.0), cell_dot(63, r), ("win_clipped",), True)
    r = next(band)
    fb.probe((2088.0, 32.0 * r + 4.0, 2088.0, 32.0 * r + 28.0), cell_dot(54, r), ("win_clipped", "no_cand"), False)
    r = next(band)
    fb.probe((2400.0, 32.0 * r + 4.0, 2400.0, 32.0 * r + 28.0), cell_dot(63, r), ("win_absent", "no_cand"), False)   # cell 75: lo = 65 > hi
    fb.probe((1200.0, -40.0, 1200.0, -36.0), cell_dot(37, 0), ("win_absent", "no_cand"), False)
    fb.probe((1600.0, 1576.0, 1600.0, 1580.0), cell_dot(50, 47), ("win_absent", "no_cand"), False)
    # one end point outside (no window), the other inside: a vertical left line that leaves the image at the top
    r = next(band)
    fb.probe((800.0, -40.0, 800.0, 40.0), (784.0, 8.0, 784.0, 56.0), ("win_absent",), True)
    # right lines that leave the grid on each side: clipped runs, rows outside 0 .. 47
    r = next(band)
    fb.probe(cell_dot(0, r), (-100.0, 32.0 * r + 10.0, 20.0, 32.0 * r + 20.0), ("clipped_r_cand", "nan_l"), True)
    r = next(band)
    fb.probe(cell_dot(63, r), (2030.0, 32.0 * r + 10.0, 2150.0, 32.0 * r + 20.0), ("clipped_r_cand", "nan_l"), True)
    fb.probe(cell_vert(20, 0), (624.0, -100.0, 624.0, 40.0), ("clipped_r_cand",), True)
    fb.probe(cell_vert(30, 46), (944.0, 1480.0, 944.0, 1640.0), ("clipped_r_cand",), True)
    # a horizontal right line across 20 columns seen by NaN-direction left lines at its two ends and beyond them
    r = next(band)
    d = fb.unique()
    j = fb.right((32.0 * 20 + 16.0, 32.0 * r + 16.0, 32.0 * 40 + 16.0, 32.0 * r + 16.0), d)
    fb.left(cell_dot(19, r), fb.unique(), ("nan_l", "no_cand"), -1)
    fb.left(cell_dot(20, r), d, ("nan_l",), j)
    fb.left(cell_dot(50, r), fb.unique(), ("nan_l",), -1)      # lo = 40: a candidate, taken by the row before at distance 0
    fb.left(cell_dot(51, r), fb.unique(), ("nan_l", "no_cand"), -1)
    # a vertical right line over many rows, and a zero-length right line (NaN direction: the gate never skips it)
    r = next(band)
    fb.probe(cell_vert(10, r), (32.0 * 8 + 16.0, 32.0 * r - 200.0, 32.0 * 8 + 16.0, 32.0 * r + 300.0), (), True)
    r = next(band)
    fb.probe(cell_vert(25, r), (32.0 * 24 + 5.0, 32.0 * r + 9.0, 32.0 * 24 + 5.0, 32.0 * r + 9.0), ("nan_r_cand",), True)
    frames.append(fb.build("S1 second end point, outside the grid, clipped right lines"))
    return frames


def f32_flip(lo, hi, pred):
    """adjacent floats a < b in [lo, hi] with pred(a) != pred(b), by bisection over the float32 bit patterns (lo, hi > 0)"""
    a, b = np.array([lo, hi], F32).view(np.int32)
    pa = pred(F32(lo))
    assert pa != pred(F32(hi))
    while b - a > 1:
        m = (int(a) + int(b)) // 2
        if pred(np.array([m], np.int32).view(F32)[0]) == pa:
            a = m
        else:
            b = m
    return np.array([a, b], np.int32).view(F32)


def gate_frame(th):
    """S2: the direction gate at line_sim_th = th"""
    fb = LineFrame(3 if th == 0.75 else 4); band = iter(range(0, ROWS - 5, 2))
    iw = ih = 1.0 / 32.0
    # NaN directions on either side never skip, whatever the partner's direction
    r = next(band)
    fb.probe(cell_dot(10, r), (32.0 * 8 + 2.0, 32.0 * r + 16.0, 32.0 * 8 + 30.0, 32.0 * r + 16.0), ("nan_l",), True)
    fb.probe(cell_vert(30, r), (32.0 * 28 + 7.0, 32.0 * r + 7.0, 32.0 * 28 + 7.0, 32.0 * r + 7.0), ("nan_r_cand",), True)
    fb.probe((32.0 * 50 + 4.0, 32.0 * r + 16.0, 32.0 * 50 + 28.0, 32.0 * r + 16.5), cell_dot(49, r), ("nan_l",), True)
    # a vertical left line against right lines whose |dot| is the float nearest to th on either side, leaning right and leaning left
    c = 24.0 * np.sqrt(1.0 / (th * th) - 1.0)
    for sgn in (1.0, -1.0):
        x0 = F32(32.0 * 18 + (2.0 if sgn > 0 else 30.0))
        kept = lambda x2: not (abs(right_dir((x0, F32(4.0), x2, F32(28.0)), iw, ih)[1]) < th)  # noqa: E731
        lo, hi = (float(x0) + c - 0.5, float(x0) + c + 0.5) if sgn > 0 else (float(x0) - c - 0.5, float(x0) - c + 0.5)
        for x2 in f32_flip(lo, hi, kept):   # two adjacent floats: one is kept, the other gated
            r = next(band)
            fb.probe(cell_vert(20, r), (x0, 32.0 * r + 4.0, x2, 32.0 * r + 28.0), ("gate_close",) + (() if kept(x2) else ("gated",)), kept(x2))
    # plainly on either side
    r = next(band)
    fb.probe(cell_vert(12, r), (32.0 * 10 + 4.0, 32.0 * r + 4.0, 32.0 * 10 + 12.0, 32.0 * r + 28.0), (), True)
    fb.probe(cell_vert(40, r), (32.0 * 38 + 2.0, 32.0 * r + 6.0, 32.0 * 38 + 30.0, 32.0 * r + 26.0), ("gated",), th <= 0.58)
    # a left cell difference of (3, 4) against an exactly horizontal right line: dot = 3 / 5 (== 0.6, kept by the strict <) and of
    # (4, 3): 4 / 5
    for (dx, dy), x in (((3, 4), 10), ((4, 3), 40)):
        r = next(band); next(band); next(band)
        left = (32.0 * x + 16.0, 32.0 * r + 16.0, 32.0 * (x + dx) + 16.0, 32.0 * (r + dy) + 16.0)
        right = (32.0 * (x - 2) + 4.0, 32.0 * r + 16.0, 32.0 * x + 4.0, 32.0 * r + 16.0)
        dot = dx / 5.0
        fb.probe(left, right, ("dot_eq_th",) if dot == th else (("gated",) if dot < th else ()), not (dot < th))
    return fb.build(f"S2 direction gate, line_sim_th {th}")


def order_frame(seed=5):
    """S3: matchGrid's running minimum per right line, by the order of the left lines; one group per band of two grid rows"""
    fb = LineFrame(seed); band = iter(range(0, ROWS - 1, 2))

    def group(lefts, rights, r):
        """lefts: (column, thermometer value, edges); rights: (column, value)"""
        js = [fb.right(cell_vert(x, r), therm(v)) for x, v in rights]
        return [fb.left(cell_vert(x, r), therm(v), e) for x, v, e in lefts], js

    group([(20, 70, ()), (21, 80, ("run_taken",)), (22, 90, ("run_taken",))], [(19, 100)], next(band))      # falling 30, 20, 10
    group([(20, 80, ()), (21, 120, ("run_equal",)), (22, 80, ("run_equal",))], [(19, 100)], next(band))      # equal 20, 20, 20
    group([(20, 90, ()), (21, 80, ("run_greater",)), (22, 70, ("run_greater",))], [(19, 100)], next(band))   # rising 10, 20, 30
    # every candidate of the second line was taken at an equal or a lower distance: it stays without a match
    group([(20, 95, ()), (21, 105, ("none_eligible",))], [(18, 100), (19, 98)], next(band))
    # exactly one eligible candidate: the nearer one (10) was taken at 5, the other (12) is accepted with second = INT_MAX
    group([(20, 55, ()), (26, 50, ("single", "run_greater"))], [(18, 60), (24, 38)], next(band))
    # the same through an equal distance
    group([(20, 55, ()), (26, 65, ("single", "run_equal"))], [(18, 60), (24, 80)], next(band))
    # four left lines, two right lines, interleaved improvements
    group([(20, 10, ()), (21, 30, ("run_taken",)), (22, 44, ("run_taken",)), (23, 47, ("run_taken",))], [(18, 50), (19, 46)], next(band))
    return fb.build("S3 order dependence")


RATIO_PAIRS = {0.75: [(3, 4), (2, 4), (6, 8), (5, 8), (96, 128), (95, 128), (192, 256), (191, 256), (0, 4), (0, 256), (0, 0), (256, 256),
                      (4, 4), (1, 1)],
               1.0: [(5, 5), (5, 6), (0, 0), (0, 1), (256, 256), (255, 256), (128, 128)],
               0.9: [(9, 10), (8, 10), (90, 100), (89, 100), (18, 20), (17, 20), (225, 250), (224, 250), (0, 1)]}


def ratio_frame(ratio):
    """S4: (best, second) on the edge of the double ratio test, and S5: two right lines at the best distance in both index orders"""
    fb = LineFrame(6 + int(ratio * 100)); slot = iter([(x, r) for r in range(0, ROWS - 1, 2) for x in (12, 28, 44, 60)])
    for best, second in RATIO_PAIRS[ratio]:
        for swap in (False, True):   # the best candidate at the lower and at the higher right index
            x, r = next(slot)
            d = (second, best) if swap else (best, second)
            js = [fb.right(cell_vert(x - 1, r), therm(d[0])), fb.right(cell_vert(x - 2, r), therm(d[1]))]
            edges = (("tie",) if best == second else ()) + (("on_edge",) if float(best) == float(second) * ratio else ())
            ok = float(best) < float(second) * ratio
            fb.left(cell_vert(x, r), therm(0), edges, js[1 if swap else 0] if ok else -1)
    for best, third in ((7, 40), (0, 256), (31, 32)):   # S5 proper: equal bits at different positions, a third candidate behind them
        for swap in (False, True):
            x, r = next(slot)
            rows = [therm(best), bits_row(256 - best, best)]
            if swap:
                rows.reverse()
            fb.right(cell_vert(x - 1, r), rows[0]); fb.right(cell_vert(x - 3, r), therm(third)); fb.right(cell_vert(x - 2, r), rows[1])
            fb.left(cell_vert(x, r), therm(0), ("tie",), -1 if ratio <= 1.0 else None)
    for d in (0, 256, 77):   # a single candidate at any distance is accepted
        x, r = next(slot)
        j = fb.right(cell_vert(x - 1, r), therm(d))
        fb.left(cell_vert(x, r), therm(0), ("single",), j)
    return fb.build(f"S4 / S5 ratio test at {ratio}")


def random_lines(rng, n, W, H, leave=0.15):
    """test_gpu_grid.make_lines on the image W x H, a share of them running out of the image"""
    s = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    e = s + rng.uniform(-150, 150, (n, 2))
    inside = rng.random(n) >= leave
    e[inside, 0] = np.clip(e[inside, 0], 0, W - 1); e[inside, 1] = np.clip(e[inside, 1], 0, H - 1)
    return np.concatenate([s, e], 1).astype(F32)


def random_frame(seed, nl, nr, cam, ent):
    """S6 / S7: nl random left lines, nr right lines of which about half are a left line shifted 3 .. 40 px to the left with its
    descriptor; descriptors with `ent` random bits"""
    rng = np.random.default_rng(seed)
    L = random_lines(rng, nl, cam["width"], cam["height"])
    R = random_lines(rng, nr, cam["width"], cam["height"])
    dl, dr = rand_desc(rng, nl, ent), rand_desc(rng, nr, ent)
    k = min(nl, nr) // 2
    if k:
        src = rng.permutation(nl)[:k]; dst = rng.permutation(nr)[:k]
        R[dst] = L[src]
        R[dst, 0] -= rng.uniform(3, 40, k).astype(F32); R[dst, 2] = R[dst, 0] + (L[src, 2] - L[src, 0])
        dr[dst] = dl[src]
    if nl >= 12:
        L[:6, 2:] = L[:6, :2] + F32(1.0)   # same-cell end points: NaN direction
    f = with_points(cam, 9500 + seed % 7, 0, L, dl, R, dr)
    return dict(name=f"random {seed}: {nl} x {nr} lines, {ent} bits", frame=f, edges={}, expect={})


def _set(name, frames, mp_kw=None, preset="kitti", cam=GRID_CAM, M=128, K=512):
    mp_kw = dict(mp_kw or {})
    return dict(name=name, cam=cam, mp=match_params(preset, **mp_kw), frames=frames, K=K, M=M)


def count_pairs(values):
    """every value as nl and as nr, nl != nr within a frame"""
    v = list(values)
    return [(v[k], v[(k + 1) % len(v)]) for k in range(len(v))]


@functools.lru_cache(maxsize=None)
def stereo_sets():
    sets = [
        _set("S1 windows", window_frames()),
        _set("S2 gate 0.75", [gate_frame(0.75)]),
        _set("S2 gate 0.6", [gate_frame(0.6)], dict(line_sim_th=0.6)),
        _set("S3+S4 kitti", [order_frame(), ratio_frame(0.75)]),
        _set("S3+S4 kitti, best_lr off", [order_frame(), ratio_frame(0.75)], dict(best_lr_matches=0)),
        _set("S4 ratio 1.0", [ratio_frame(1.0), order_frame()], dict(min_ratio_12_p=1.0)),
        _set("S4 euroc", [ratio_frame(0.9), order_frame()], preset="euroc"),
    ]
    # S6: counts and capacities; several streams with different counts side by side, one without left and one without right lines
    s = 100
    for M, vals in ((64, [0, 1, 2, 31, 32, 33, 63, 64]), (128, [65, 128, 2, 64, 127, 0, 33]), (320, [129, 255, 256, 257, 1, 320, 64]),
                    (512, [511, 512, 257, 129, 65, 0, 31])):
        frames = []
        for nl, nr in count_pairs(vals):
            frames.append(random_frame(s, nl, nr, GRID_CAM, 16)); s += 1
        sets.append(_set(f"S6 counts M={M}", frames, M=M))
    # ... and 16 streams (the fused kernel's default route beyond 128 lines), the LDS sized by the largest
    vals = [257, 40, 129, 3, 300, 64, 128, 65, 1, 255, 0, 320, 200, 31, 256, 100]
    sets.append(_set("S6 counts M=320, 16 streams", [random_frame(200 + k, a, b, GRID_CAM, 24) for k, (a, b) in enumerate(count_pairs(vals))], M=320))
    # S7: seeded sweep, both cameras, both ratios
    s = 300
    for cam, cname in ((GRID_CAM, "grid camera"), (synth.KITTI_CAM, "kitti camera")):
        for preset in ("kitti", "euroc"):
            frames = []
            for k in range(9):
                rng = np.random.default_rng(s)
                frames.append(random_frame(s, int(rng.integers(20, 129)), int(rng.integers(20, 129)), cam, (8, 16, 24)[k % 3])); s += 1
            sets.append(_set(f"S7 sweep, {cname}, {preset} ratio", frames, preset=preset, cam=cam))
    return sets


_STEREO = {}


def stereo_results(orc, cs):
    """[(oracle raw matches, np_model raw matches, trace) per frame], computed once per set and never modified"""
    if cs["name"] not in _STEREO:
        _STEREO[cs["name"]] = [stereo_expect(orc, cf["frame"], cs["cam"], cs["mp"]) for cf in cs["frames"]]
    return _STEREO[cs["name"]]


# ---- frame-to-frame: the separated layout ------------------------------------------------------------------------------------------------
def separated_lines(n, dense):
    """n left lines none of which is a stereo candidate of another line's partner.  Sparse (matching_s_ws = 10): columns 3, 15, ..,
    63 x 24 bands of two grid rows (144 places); dense (matching_s_ws = 2): columns 3, 7, .., 63 x 48 grid rows (768 places)."""
    out = []
    if dense:
        places = [(c, r) for r in range(ROWS) for c in range(3, COLS, 4)]
        for c, r in places[:n]:
            out.append((32.0 * c + 16.0, 32.0 * r + 4.0, 32.0 * c + 20.0, 32.0 * r + 28.0))
    else:
        places = [(c, b) for b in range(24) for c in (3, 15, 27, 39, 51, 63)]
        for c, b in places[:n]:
            out.append((32.0 * c + 16.0, 64.0 * b + 8.0, 32.0 * c + 20.0, 64.0 * b + 56.0))
    assert len(out) == n, (n, dense)
    return np.asarray(out, F32).reshape(n, 4)


def separated_frame(seed, step, desc, dense):
    """the left lines of the layout with the rows of `desc`, every partner 40 px to the left, the right side shuffled"""
    rng = np.random.default_rng(seed * 2 + step)
    n = len(desc)
    L = separated_lines(n, dense)
    perm = rng.permutation(n)
    R = L.copy(); R[:, 0] -= F32(40.0); R[:, 2] -= F32(40.0)
    return with_points(GRID_CAM, 9700 + seed % 5, step, L, desc, R[perm], np.asarray(desc, np.uint8).reshape(n, 32)[perm])


def f2f_trace(A, B, nnr, lr):
    """flags over the query rows A against the train rows B from the distance matrix (float ratio test, src/matching.cpp:53-58)"""
    na, nb = len(A), len(B)
    names = ("tie", "on_edge", "claim", "rev_other", "rev_fail", "shared_equal", "shared_diff", "dup_train_best", "dup_query", "kept")
    t = {k: np.zeros(na, np.int64) for k in names}
    if na == 0 or nb < 2:
        return t
    D = np_model.hamming_matrix(A, B)
    i0, d0, d1 = np_model.knn2(D)
    nn = F32(nnr)
    ok = d0.astype(F32) < d1.astype(F32) * nn
    t["tie"][:] = d0 == d1
    t["on_edge"][:] = d0.astype(F32) == d1.astype(F32) * nn
    t["claim"][:] = ok
    t["dup_train_best"][:] = [(B == B[i0[i]]).all(axis=1).sum() > 1 for i in range(na)]
    t["dup_query"][:] = [(A == A[i]).all(axis=1).sum() > 1 for i in range(na)]
    if na >= 2:
        r0, e0, e1 = np_model.knn2(D.T.copy())
        rok = e0.astype(F32) < e1.astype(F32) * nn
        for i in np.nonzero(ok)[0]:
            j = i0[i]
            t["rev_fail"][i] = int(not rok[j])
            t["rev_other"][i] = int(r0[j] != i)
            others = [k for k in np.nonzero(ok)[0] if k != i and i0[k] == j]
            t["shared_equal"][i] = int(any(d0[k] == d0[i] for k in others))
            t["shared_diff"][i] = int(any(d0[k] != d0[i] for k in others))
    t["kept"][:] = np_model.match(A, B, nnr, lr) >= 0
    return t


class Stream:
    def __init__(self, name, A, B, edges=None):
        self.name = name
        self.A = np.ascontiguousarray(np.asarray(A, np.uint8).reshape(-1, 32)); self.B = np.ascontiguousarray(np.asarray(B, np.uint8).reshape(-1, 32))
        self.edges = edges or {}


def ties_stream(seed, reverse):
    """F1: duplicate rows in the train set and in the query set at low and high indices, best == second, and genuine pairs"""
    rng = np.random.default_rng(seed)
    nb, na = 40, 36
    B = rand_desc(rng, nb)
    B[1] = B[0]; B[39] = B[38]; B[21] = B[5]               # duplicates: low, high, far apart
    A = synth.flip_bits(rng, B[rng.permutation(nb)[:na]], 0.02)
    A[0] = B[0] ^ bits_row(3, 1); A[35] = B[38] ^ bits_row(200, 2); A[7] = B[5]     # their best is a duplicated train row: best == second
    A[2] = B[10] ^ bits_row(0, 1); A[3] = A[2]; A[33] = B[30]; A[34] = A[33]          # duplicate query rows claim one train row
    A[12] = B[15] ^ bits_row(0, 3); A[13] = B[16] ^ bits_row(9, 3)                   # plain
    edges = dict(tie=[0, 35, 7], dup_train_best=[0, 35, 7], dup_query=[2, 3, 33, 34], shared_equal=[2, 3, 33, 34])
    if reverse:   # everything the other way round: what was a tie in the forward scan is one in the reverse scan
        return Stream(f"F1 ties {seed}, reversed", B, A, dict(dup_query=[0, 1, 38, 39, 5, 21], tie=[10, 30], shared_equal=[0, 1, 38, 39, 5, 21]))
    return Stream(f"F1 ties {seed}", A, B, edges)


def ratio_cluster_stream(seed, pairs):
    """F2, small distances: query row k = (code k, 0), its two nearest train rows (code k, d0) and (code k, d1), shuffled"""
    rng = np.random.default_rng(seed)
    codes = rand_desc(rng, len(pairs))[:, :16]
    A = [coded(codes[k], 0) for k in range(len(pairs))]
    B = []
    for k, (d0, d1) in enumerate(pairs):
        B += [coded(codes[k], d0), coded(codes[k], d1)]
    B = np.asarray(B)[rng.permutation(len(B))]
    return Stream(f"F2 ratio edge, clusters {pairs}", A, B, dict(pairs=pairs))


def ratio_pair_stream(d0, d1):
    """F2, any distance: the query row 0 = zeros against therm(d0) and therm(d1); the second query row is the complement of
    therm(d0), so that the reverse scan keeps row 0's claim"""
    A = [therm(0), ~therm(d0)]
    return Stream(f"F2 ratio edge ({d0}, {d1})", A, [therm(d0), therm(d1)], dict(pair=(d0, d1)))


def mutual_stream(seed):
    """F3: claims that the mutual check has to judge"""
    rng = np.random.default_rng(seed)
    codes = rand_desc(rng, 8)[:, :16]
    A, B, e = [], [], dict(shared_diff=[], shared_equal=[], rev_other=[], rev_fail=[], kept=[])
    # two query rows claim one train row at different distances (2 and 5): the nearer keeps it
    A += [coded(codes[0], 10), coded(codes[0], 17)]; B += [coded(codes[0], 12)]
    e["shared_diff"] += [0, 1]; e["rev_other"] += [1]; e["kept"] += [0]
    # ... at equal distances (3 and 3): the reverse scan has best == second
    A += [coded(codes[1], 20), coded(codes[1], 26)]; B += [coded(codes[1], 23)]
    e["shared_equal"] += [2, 3]; e["rev_fail"] += [2, 3]
    # a claim whose reverse best is another row (the train row is nearer to query row 5)
    A += [coded(codes[2], 40), coded(codes[2], 60)]; B += [coded(codes[2], 58), coded(codes[2], 90)]
    e["rev_other"] += [4]; e["kept"] += [5]
    # a claim whose reverse ratio test fails: distances 9 and 10 from the train row
    A += [coded(codes[3], 30), coded(codes[3], 49)]; B += [coded(codes[3], 39)]
    e["rev_fail"] += [6]
    # plain pairs
    for k in range(4, 8):
        A.append(coded(codes[k], 5)); B.append(coded(codes[k], 6))
    e["kept"] += [8, 9, 10, 11]
    return Stream(f"F3 mutual check {seed}", A, B, e)


def sized_stream(seed, na, nb, ent):
    """F4 / F5: na query rows, nb train rows with `ent` random bits, about half of the train rows near copies of query rows"""
    rng = np.random.default_rng(seed)
    A, B = rand_desc(rng, na, ent), rand_desc(rng, nb, ent)
    k = min(na, nb) // 2
    if k:
        src, dst = rng.permutation(na)[:k], rng.permutation(nb)[:k]
        B[dst] = A[src] ^ (rand_desc(rng, k, ent) & rand_desc(rng, k, ent) & rand_desc(rng, k, ent) & rand_desc(rng, k, ent))
    return Stream(f"sizes {na} x {nb}, {ent} bits", A, B)


def _fset(name, streams, mp_kw=None, M=128, dense=False):
    mp_kw = dict(mp_kw or {})
    if dense:
        mp_kw.setdefault("matching_s_ws", 2)
    seeds = [1000 + 17 * k for k in range(len(streams))]
    steps = [[separated_frame(seeds[k], step, (s.A, s.B)[step], dense) for k, s in enumerate(streams)] for step in (0, 1)]
    return dict(name=name, cam=GRID_CAM, mp=match_params("kitti", **mp_kw), streams=streams, steps=steps, K=512, M=M)


F2F_SMALL_PAIRS = [(3, 4), (2, 4), (4, 4), (6, 8), (5, 8), (0, 3), (0, 0), (1, 2)]
F2F_BIG_PAIRS = [(96, 128), (95, 128), (97, 128), (192, 256), (191, 256), (193, 256), (0, 256), (256, 256), (255, 256)]


def _edge_streams():
    return ([ties_stream(1, False), ties_stream(1, True), ties_stream(2, False), mutual_stream(3), ratio_cluster_stream(4, F2F_SMALL_PAIRS)] +
            [ratio_pair_stream(a, b) for a, b in F2F_BIG_PAIRS])


@functools.lru_cache(maxsize=None)
def f2f_sets():
    size_pairs = [(0, 5), (1, 4), (2, 1), (3, 2), (4, 3), (5, 0), (63, 64), (64, 65), (65, 63), (127, 128), (128, 127), (5, 1), (1, 128), (128, 2)]
    sets = [
        _fset("F1-F3 edges, ratio 0.75", _edge_streams()),
        _fset("F1-F3 edges, best_lr off", _edge_streams(), dict(best_lr_matches=0)),
        # 0.9f: (9, 10) — the float product 10 * 0.9f rounds to 9.0f exactly, so 9 < 9 fails — and its neighbours
        _fset("F2 ratio 0.9", [ratio_cluster_stream(5, [(9, 10), (8, 10), (18, 20), (17, 20), (0, 1), (10, 10)]), ratio_pair_stream(90, 100),
                               ratio_pair_stream(89, 100), ratio_pair_stream(225, 250), ties_stream(6, False), mutual_stream(7)],
              dict(min_ratio_12_l=0.9)),
        _fset("F1 ratio 1.0", [ties_stream(8, False), ties_stream(8, True), ratio_cluster_stream(9, [(5, 5), (5, 6), (0, 0), (0, 1)]),
                               ratio_pair_stream(256, 256), ratio_pair_stream(255, 256)], dict(min_ratio_12_l=1.0)),
        _fset("F4 sizes", [sized_stream(20 + k, a, b, 16) for k, (a, b) in enumerate(size_pairs)]),
        _fset("F4 sizes, best_lr off", [sized_stream(40 + k, a, b, 16) for k, (a, b) in enumerate(size_pairs[:8])], dict(best_lr_matches=0)),
        _fset("F4 sizes M=320", [sized_stream(60 + k, a, b, 16) for k, (a, b) in
                                 enumerate([(129, 255), (255, 256), (256, 129), (5, 64), (64, 3)])], M=320, dense=True),
        _fset("F4 sizes M=512", [sized_stream(80 + k, a, b, 24) for k, (a, b) in
                                 enumerate([(511, 512), (512, 257), (257, 511), (3, 64), (40, 33)])], M=512, dense=True),
    ]
    s = 500
    for nnr in (0.5, 0.75, 0.9, 1.0):   # F5
        streams = []
        for k in range(8):
            rng = np.random.default_rng(s)
            streams.append(sized_stream(s, int(rng.integers(2, 129)), int(rng.integers(2, 129)), (8, 16, 24, 64)[k % 4])); s += 1
        sets.append(_fset(f"F5 sweep, ratio {nnr}", streams, dict(min_ratio_12_l=nnr)))
    return sets


_F2F = {}


def f2f_chunk(cs, a, b):
    """the streams a .. b - 1 of a set as a set of their own (the results are shared with the whole set's)"""
    return dict(cs, streams=cs["streams"][a:b], steps=[st[a:b] for st in cs["steps"]], chunk=(a, b))


def f2f_results(orc, cs, op):
    """per stream: dict(sets = the oracle's kept key-line rows after step 0 and step 1, stereo = its raw matches and counts, ref = the
    oracle pipeline's result of the tracked step); computed once per set"""
    if cs["name"] not in _F2F:
        out = []
        assert "chunk" not in cs
        for b in range(len(cs["streams"])):
            fr = [cs["steps"][0][b], cs["steps"][1][b]]
            st = [pipeline_ref.stereo_frame(orc, f, cs["cam"], cs["mp"], True, True) for f in fr]
            ref = pipeline_ref.run_sequence(orc, fr, cs["cam"], cs["mp"], op)[0]
            out.append(dict(sets=[s["ldesc"] for s in st], raw=[s["m12_raw_l"] for s in st], n_pts=[len(s["P"]) for s in st], ref=ref))
        _F2F[cs["name"]] = out
    a, b = cs.get("chunk", (0, len(_F2F[cs["name"]])))
    return _F2F[cs["name"]][a:b]
