"""Residual sets for removeOutliers and the robust scale, planned value by value — TEST INFRASTRUCTURE ONLY, shared by
tests/test_outlier_cut_host.py (CPU) and tests/test_gpu_outlier_cut.py.

A case is two PLANS, points and key-lines: lists of Feat(r, sigma2, inl, keep, name) — the weighted residual norm the feature has
at the initial pose, its sigma2, whether it arrives as an inlier, whether removeOutliers keeps it, a label.  records() turns the
plans into the matched records of stvo_optimize_pose such that every residual IS the planned double:

  * the camera is dyadic (stereo_tail_cases.GRID_CAM), the initial pose DT0 a dyadic translation (not I: a committed DT = I is the
    rejected solution), depths are powers of two, projections lie on the 1/4-pixel lattice — every product, quotient and sum of
    the projection is exact;
  * a point's observation differs from its projection along one axis only (sqrt(d d + 0) = |d|); a key-line is observed as
    (0, 1, -y0) or (1, 0, -x0), its end point projects onto that line (de = 0) and its start point d beside it;
  * sigma2 is 0.25, 1 or 4, so r = d sqrt(sigma2) is a scaling by a power of two;
  * a value that does not fit the lattice (a double with all its bits) goes to a feature whose projection is pixel 0 (points: the
    observation is the value itself) or, for a line, into the line equation (0, x, 0) with the start point projecting onto row 1 and
    the end point onto row 0; so does every key-line residual above 64, which keeps H well conditioned (asserted on the CPU).

With min_error = 1e30 stage 1 of optimizePose stops after its first evaluation with DT untouched, removeOutliers runs at DT0 on
exactly the planned multisets and the refinement stops the same way: the masks that come back are one cut.

`keep` is stated by expected(): the two order statistics BY COUNTING (the value v with #{x < v} <= k < #{x <= v}: no sort, no
selection), the gate, the mean, the strict cut — and, where a case is about a particular outcome, the case declares median, MAD
and the kind of mean in so many words and the builder asserts them.  Every sum that decides something is exact in any order
(asserted): the device sums by tree, the oracle in sequence."""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from stereo_tail_cases import GRID_CAM
from stvo_amd.ctypes_types import opt_params

CAM = GRID_CAM
T0_TRANS = (0.25, -0.5, 0.0)
DT0 = np.eye(4)
DT0[:3, 3] = T0_TRANS
DEPTHS = (2.0, 4.0, 8.0, 16.0)
MIN_ERROR = 1e30
PARAM_SETS = {"kitti": dict(preset="kitti"), "euroc": dict(preset="euroc"), "edge": dict(preset="default", inlier_k=4.0)}

Feat = namedtuple("Feat", "r sigma2 inl keep name")
Stats = namedtuple("Stats", "n med mad sigma ksel mean_kind mean th exact")   # mean_kind: "gated", "full", "nan", "none" (empty set)


def params(case, mode=0, **kw):
    d = dict(PARAM_SETS[case["prm"]])
    preset = d.pop("preset")
    d.update(min_error=MIN_ERROR, mode=mode, has_points=case["has_points"], has_lines=case["has_lines"])
    if case["min_features"] is not None:
        d["min_features"] = case["min_features"]
    d.update(kw)
    return opt_params(preset, **d)


# ---- the plain statement by counting ---------------------------------------------------------------------------------------------
def kth(values, k):
    """the k-th smallest (0-based) by counting: the v with #{x < v} <= k < #{x <= v}"""
    vals = np.asarray(values, np.float64)
    for v in np.unique(vals):
        if int((vals < v).sum()) <= k < int((vals <= v).sum()):
            return float(v)
    raise AssertionError("no such rank")


def _exact_in_any_order(vals):
    """every partial sum of these non-negative doubles is a double: they are multiples of one power of two q and add up to < 2^53 q"""
    fr = [Fraction(float(v)) for v in vals if v != 0]
    if not fr:
        return True
    q = min(Fraction(f.numerator & -f.numerator, f.denominator) for f in fr)
    return sum(fr) / q < 2 ** 53


def expected(r, inl, inlier_k):
    """(kept [n] bool, Stats) of one kind of feature: vector_mean_stdv_mad (src/auxiliar.cpp:387-430) on ALL matched residuals and the
    strict cut of removeOutliers (src/stereoFrameHandler.cpp:988-1067) on the inliers"""
    r = np.asarray(r, np.float64)
    inl = np.asarray(inl, bool)
    n = len(r)
    if n == 0:
        return inl.copy(), Stats(0, 0.0, 0.0, 0.0, 0, "none", 0.0, 0.0, True)
    med = kth(r, n // 2)
    dev = np.abs((r - med).astype(np.float32)).astype(np.float64)
    mad = kth(dev, n // 2)
    sigma = 1.4826 * mad
    gate = r < 2.0 * sigma
    ksel = int(gate.sum())
    if ksel >= int(0.2 * n):
        kind = "gated" if ksel else "nan"
        exact = _exact_in_any_order(r[gate])
        with np.errstate(invalid="ignore"):
            mean = np.float64(math.fsum(r[gate])) / np.float64(ksel)
    else:
        kind = "full"
        exact = _exact_in_any_order(r)
        mean = np.float64(math.fsum(r)) / np.float64(n)
    th = inlier_k * sigma
    with np.errstate(invalid="ignore"):
        kept = inl & ~(np.abs(r - mean) > th)
    return kept, Stats(n, med, mad, sigma, ksel, kind, float(mean), th, exact)


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def _lattice(rng, lo, hi):
    return lo + 0.25 * float(rng.integers(0, int(4 * (hi - lo)) + 1))


def _back(u, v, z, trans):
    """the camera-frame point that projects to (u, v) at depth z, exactly; and the previous-frame point DT0 carries there"""
    g = np.array([(u - CAM["cx"]) * z / CAM["fx"], (v - CAM["cy"]) * z / CAM["fy"], z])
    P = g - np.asarray(trans)
    assert np.array_equal(P + np.asarray(trans), g)
    assert CAM["cx"] + CAM["fx"] * g[0] / g[2] == u and CAM["cy"] + CAM["fy"] * g[1] / g[2] == v
    return P


def _point(rng, j, f, trans):
    sq = math.sqrt(f.sigma2)
    d = f.r / sq
    assert d * sq == f.r and f.sigma2 in (0.25, 1.0, 4.0)
    axis, sgn = j % 2, (1.0 if (j // 2) % 2 == 0 else -1.0)
    uv = [_lattice(rng, 64.0, 1984.0), _lattice(rng, 64.0, 1472.0)]
    z = DEPTHS[int(rng.integers(0, 4))]
    if uv[axis] - (uv[axis] - sgn * d) != sgn * d:   # the value does not fit the lattice: the projection goes to pixel 0
        uv[axis] = 0.0
    obs = list(uv)
    obs[axis] = uv[axis] - sgn * d
    assert uv[axis] - obs[axis] == sgn * d
    return _back(uv[0], uv[1], z, trans), obs


def _line(rng, j, f, trans):
    """-> sP, eP, le, spl, epl.  axis 1: the observed line is the row y0, axis 0: the column x0."""
    sq = math.sqrt(f.sigma2)
    d = f.r / sq
    assert d * sq == f.r and f.sigma2 in (0.25, 1.0, 4.0)
    axis, sgn = 1 - j % 2, (1.0 if (j // 2) % 2 == 0 else -1.0)
    hi_a, hi_b = (1472.0, 1984.0) if axis == 1 else (1984.0, 1472.0)   # a: across the line (carries d), b: along it
    a0 = _lattice(rng, 64.0, hi_a)
    b_s = _lattice(rng, 64.0, hi_b / 2)
    b_e = b_s + 64.0 + _lattice(rng, 0.0, hi_b / 2 - 128.0)
    zs, ze = DEPTHS[int(rng.integers(0, 4))], DEPTHS[int(rng.integers(0, 4))]
    a_s = a0 + sgn * d
    # (a start point that projects far outside the image has a gradient ~ d^2 against a weight ~ 1 / d^2: H would span 20 decades
    # and isGoodSolution hang on a rounding — large values go into the line equation as well, where the gradient is ~ d)
    fits = a_s - a0 == sgn * d and d <= 64.0
    if fits:
        try:
            _back(a_s, a_s, zs, trans)
        except AssertionError:
            fits = False
    if fits:
        l_a, l_c, a_e, a_obs = 1.0, -a0, a0, a0
    else:   # (0, x, 0): the start point projects onto row / column 1, the end point onto 0; ds = x 1 + 0, de = x 0 + 0
        l_a, l_c, a_s, a_e, a_obs = sgn * d, 0.0, 1.0, 0.0, 0.5
    if axis == 1:
        s_uv, e_uv, le = (b_s, a_s), (b_e, a_e), (0.0, l_a, l_c)
        spl, epl = (b_s, a_obs), (b_e, a_obs)
    else:
        s_uv, e_uv, le = (a_s, b_s), (a_e, b_e), (l_a, 0.0, l_c)
        spl, epl = (a_obs, b_s), (a_obs, b_e)
    return _back(s_uv[0], s_uv[1], zs, trans), _back(e_uv[0], e_uv[1], ze, trans), le, spl, epl


def _place(plan, placement, rng):
    """feature row i holds plan entry order[i]"""
    n = len(plan)
    if placement == "shuffle":
        return rng.permutation(n)
    by_r = np.argsort([f.r for f in plan], kind="stable")
    return by_r if placement == "ascending" else by_r[::-1].copy()


def records(case, trans=T0_TRANS):
    """-> (rec, order_p, order_l): the matched records of the case for the initial pose [I | trans]; rec row i of a kind is plan entry
    order[i]"""
    rng = np.random.default_rng(case["seed"])
    pp, pl = case["plan_p"], case["plan_l"]
    op, ol = _place(pp, case["placement"], rng), _place(pl, case["placement"], rng)
    n, m = len(pp), len(pl)
    rec = dict(P=np.zeros((n, 3)), pl_obs=np.zeros((n, 2)), sigma2p=np.zeros(n), inlier_p=np.zeros(n, np.int32), sP=np.zeros((m, 3)),
               eP=np.zeros((m, 3)), le_obs=np.zeros((m, 3)), spl=np.zeros((m, 2)), epl=np.zeros((m, 2)), sigma2l=np.zeros(m),
               inlier_l=np.zeros(m, np.int32))
    for i, j in enumerate(op):
        f = pp[j]
        rec["P"][i], rec["pl_obs"][i] = _point(rng, int(j), f, trans)
        rec["sigma2p"][i], rec["inlier_p"][i] = f.sigma2, int(f.inl)
    for i, j in enumerate(ol):
        f = pl[j]
        rec["sP"][i], rec["eP"][i], rec["le_obs"][i], rec["spl"][i], rec["epl"][i] = _line(rng, int(j), f, trans)
        rec["sigma2l"][i], rec["inlier_l"][i] = f.sigma2, int(f.inl)
    return rec, op, ol


def expect_masks(case, order_p, order_l):
    """the inlier flags removeOutliers leaves, in record order; a kind that is switched off keeps its flags"""
    ep = np.array([pp.keep if case["has_points"] else pp.inl for pp in case["plan_p"]], bool)[order_p] if len(order_p) else np.zeros(0, bool)
    el = np.array([pl.keep if case["has_lines"] else pl.inl for pl in case["plan_l"]], bool)[order_l] if len(order_l) else np.zeros(0, bool)
    return ep.astype(np.int32), el.astype(np.int32)


# ---- value sets: [(r, sigma2, inl, name)] ------------------------------------------------------------------------------------------
S2 = (1.0, 0.25, 4.0)


def vals(rs, name, s2=None, inl=None):
    return [(float(r), S2[i % 3] if s2 is None else s2, True if inl is None else bool(inl[i]), f"{name}[{i}]") for i, r in enumerate(rs)]


def spread(n, name="spread"):
    """a benign set: multiples of 1/8 in [1/8, 2], a few repeats, a tail of large residuals (a tenth of the set at 8 .. 40)"""
    out = []
    for i in range(n):
        out.append(8.0 + 4.0 * (i % 9) if i % 10 == 9 else 0.125 * (1 + (i * 7) % 16))
    return vals(out, name)


def geometric(n, lo=-20):
    """2^lo, 2^(lo + 1), ...: neighbouring order statistics differ by 2 x"""
    return vals([2.0 ** (lo + i) for i in range(n)], "geo")


def stepped(n):
    """lower part (0.5, 1], upper part [2, ...): sorted[n / 2] is 1 for n = 65 (33 lower values) and 2 for n = 64 (32 of them)"""
    lower = [1.0 - i * 2.0 ** -6 for i in range(33 if n % 2 else 32)]
    return vals(lower + [2.0 + i * 2.0 ** -5 for i in range(n - len(lower))], "stepped", s2=1.0)


def sensitive(n):
    """for the robust scale (sigma2 = 1, all inliers, sigma inside the clamp): the order statistics around rank n / 2 are far apart in
    the values (0.75 | 1 | 2 around the median 1) and in the deviations (0.25 | 0.5 | 1 around the MAD 0.5)"""
    h = n // 2
    # sorted values: 0.5, h - 1 times 0.75, the median 1 at rank h, then 2 and more; sorted deviations: 0, h - 1 times 0.25, ONE 0.5 at
    # rank h, then 1 and more
    below = [0.75] * (h - 1) + [0.5]
    above = [2.0 + 0.5 * (i % 3) for i in range(n - 1 - h)]
    return vals(below + [1.0] + above, "sens", s2=1.0)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _case(name, P, L, prm="kitti", placement="shuffle", min_features=None, has_points=1, has_lines=1, declare=None, robust=False, seed=None, inexact=""):
    return dict(name=name, P=P, L=L, prm=prm, placement=placement, min_features=min_features, has_points=has_points, has_lines=has_lines,
                declare=declare or {}, robust=robust, seed=seed, inexact=inexact)


def _edge_tail(base, inlier_k, name):
    """base + two features in the upper tail, outside the 2 sigma gate: one at fabs(r - mean) == inlier_k sigma exactly (kept), one a
    single ulp beyond (cut).  Median, MAD and mean are those of the base set with two placeholders in the tail; the two values are
    then chosen from the statement's own doubles and the statement is asked again."""
    rs = [b[0] for b in base]
    _, st = expected(rs + [1e6, 1e6], [True] * (len(rs) + 2), inlier_k)
    at = float(np.float64(st.mean) + np.float64(st.th))
    for _ in range(64):   # the double r with fl(r - mean) == th (r = fl(mean + th) unless that sum rounds)
        if abs(at - st.mean) == st.th:
            break
        at = float(np.nextafter(at, np.inf if abs(at - st.mean) < st.th else -np.inf))
    beyond = float(np.nextafter(at, np.inf))
    assert abs(at - st.mean) == st.th and abs(beyond - st.mean) > st.th and at >= 2.0 * st.sigma and at > st.med + st.mad
    out = list(base) + [(at, 1.0, True, name + "[at the threshold]"), (beyond, 1.0, True, name + "[one ulp beyond]")]
    _, st2 = expected([o[0] for o in out], [True] * len(out), inlier_k)
    assert (st2.med, st2.mad, st2.mean, st2.th) == (st.med, st.mad, st.mean, st.th)
    return out


def _float_collisions():
    """n = 65 around the median 600: 32 values just above 0 and 32 just above 1200, 2^-30 apart — as doubles all 64 deviations differ,
    as floats (spacing 2^-14 there) every one of them is 600: MAD = 600 whatever rank is taken, and only with the truncation"""
    lo = [i * 2.0 ** -30 for i in range(32)]
    hi = [1200.0 + i * 2.0 ** -30 for i in range(32)]
    return vals(lo + [600.0] + hi, "collide", s2=1.0)


def _low_bits():
    """n = 65: 20 zeros, 6 values below c = 1024 + 64 q (q = 2^-42, the spacing of doubles there), 33 copies of c, 6 above; the
    neighbours c -+ j q differ from c in the lowest 7 bits of the key only.  Median = c, 33 deviations are 0: MAD 0, no value is
    < 0, the full mean is ~709 and EVERYTHING is cut.  A median one key off makes the 33 deviations q: sigma > 0, the zeros
    pass the gate, the mean is 0 and the 20 zeros stay."""
    q = 2.0 ** -42
    c = 1024.0 + 64 * q
    return vals([0.0] * 20 + [c - j * q for j in range(1, 7)] + [c] * 33 + [c + j * q for j in range(1, 7)], "lowbits", s2=1.0)


def _one_bin(split):
    """2048 values 1 + j 2^-40 (split: the upper 1024 moved up by 0.25, into the bin that shares its counter word with the lower ones
    in the window of mantissa bits 56 .. 50 of the key)"""
    return vals([1.0 + (0.25 if split and j >= 1024 else 0.0) + (j % 1024 if split else j) * 2.0 ** -40 for j in range(2048)], "onebin", s2=1.0)


PAIRED = ("size-", "median-", "low-7-bits-", "exponent-only-", "threshold-edge-points", "threshold-edge-lines", "all-equal-3", "all-equal-4", "no-",
          "points-off", "lines-off")   # cases that come as a points / lines pair already


def _specs():
    c = []
    F61, F65 = lambda: spread(61, "fill"), lambda: spread(65, "fill")
    tiny = [1.0, 2.0, 4.0, 8.0, 16.0]
    # ---- sizes
    for m in range(1, 6):
        c.append(_case(f"size-p{m}-l65", vals(tiny[:m], "tiny"), F65()))
        c.append(_case(f"size-p61-l{m}", F61(), vals(tiny[:m], "tiny")))
    for n in (64, 65):
        c.append(_case(f"median-p{n}", stepped(n), spread(7), declare=dict(p=dict(med=2.0 if n == 64 else 1.0))))
        c.append(_case(f"median-l{n}", spread(61), stepped(n), declare=dict(l=dict(med=2.0 if n == 64 else 1.0))))
    for prm in ("kitti", "euroc"):
        for npts, nl in ((61, 7), (449, 65), (2048, 512)):
            c.append(_case(f"spread-{npts}-{nl}-{prm}", spread(npts), spread(nl), prm=prm))
    for npts in (896, 897, 1792, 1793):   # the eighth key of a thread: 7 x 128 + 1 (pose2p / pose2c, two waves), 7 x 256 + 1 (four waves)
        c.append(_case(f"eighth-key-{npts}", spread(npts), spread(7)))
    c.append(_case("lines-129", spread(61), spread(129)))   # one more than the solver wave holds (64 x LPT = 128 in pose_kernel)
    c.append(_case("no-lines", F61(), []))
    c.append(_case("no-points", [], F65()))
    c.append(_case("points-off", geometric(61), F65(), has_points=0))
    c.append(_case("lines-off", F61(), geometric(65), has_lines=0))
    # ---- rank
    for placement in ("ascending", "descending", "shuffle"):
        c.append(_case(f"geometric-{placement}", geometric(61), geometric(65), placement=placement, declare=dict(p=dict(med=2.0 ** 10), l=dict(med=2.0 ** 12))))
    for n, m in ((64, 65), (65, 64), (449, 128), (2047, 511)):
        c.append(_case(f"sensitive-{n}-{m}", sensitive(n), sensitive(m), robust=True, declare=dict(p=dict(med=1.0, mad=0.5), l=dict(med=1.0, mad=0.5))))
    # ---- ties
    c.append(_case("all-equal", vals([1.5] * 64, "eq", s2=1.0), vals([3.0] * 65, "eq"),
                   declare=dict(p=dict(med=1.5, mad=0.0, mean_kind="full", kept=64), l=dict(med=3.0, mad=0.0, mean_kind="full", kept=65))))
    c.append(_case("all-equal-3-nan", vals([3.0] * 3, "eq"), F65(), declare=dict(p=dict(mad=0.0, mean_kind="nan", kept=3))))
    c.append(_case("all-equal-4-nan", F61(), vals([0.75] * 4, "eq"), declare=dict(l=dict(mad=0.0, mean_kind="nan", kept=4))))
    half = [4.0] * 40 + [2.0] * 13 + [6.0] * 13   # the full mean is 4 exactly: the 40 stay, everything off the mean goes
    c.append(_case("half-equal", vals(half, "half"), vals(half[:-1] + [7.0], "half"),   # lines: the mean is off 4 by 1 / 66: ALL of them go
                   declare=dict(p=dict(med=4.0, mad=0.0, mean_kind="full", kept=40), l=dict(med=4.0, mad=0.0, mean_kind="full", kept=0))))
    dup = [1.0] * 20 + [2.0] * 25 + [4.0] * 20   # ranks 20 .. 44 are 2; deviations: 25 zeros, ranks 25 .. 44 are 1
    c.append(_case("duplicate-blocks", vals(dup, "dup"), vals(dup[1:], "dup"), declare=dict(p=dict(med=2.0, mad=1.0, kept=45), l=dict(med=2.0, mad=1.0, kept=44))))
    sym = [8.0] + [8.0 - j / 4 for j in range(1, 33)] + [8.0 + j / 4 for j in range(1, 33)]   # deviations tie pairwise: 0, 1/4, 1/4, 1/2, ...
    c.append(_case("symmetric", vals(sym, "sym"), vals(sym[:-1], "sym"), declare=dict(p=dict(med=8.0, mad=4.0), l=dict(med=8.0, mad=4.0))))
    # ---- key shape
    c.append(_case("low-7-bits-points", _low_bits(), F65(), declare=dict(p=dict(med=1024.0 + 2.0 ** -36, mad=0.0, mean_kind="full", kept=0)), inexact="p"))
    c.append(_case("low-7-bits-lines", F61(), _low_bits(), declare=dict(l=dict(med=1024.0 + 2.0 ** -36, mad=0.0, mean_kind="full", kept=0)), inexact="l"))
    far = [2.0 ** -32, 1.0, 2.0 ** 32]   # keys that differ in the top exponent bits: one key per bin in the first window
    c.append(_case("exponent-only-points", vals(far, "far", s2=1.0), F65(), declare=dict(p=dict(med=1.0, mad=1.0, kept=2))))
    c.append(_case("exponent-only-lines", F61(), vals(far + [2.0 ** 32, 2.0 ** -32], "far", s2=1.0), declare=dict(l=dict(med=1.0, mad=1.0, kept=3))))
    c.append(_case("one-bin-2048", _one_bin(False), spread(65), declare=dict(p=dict(med=1.0 + 2.0 ** -30, mad=2.0 ** -31, mean_kind="full"))))
    c.append(_case("shared-word-2048", _one_bin(True), spread(65), declare=dict(p=dict(med=1.25, mad=0.25, mean_kind="full", kept=2048))))
    c.append(_case("one-bin-512-lines", spread(61), _one_bin(False)[:512], declare=dict(l=dict(med=1.0 + 2.0 ** -32, mad=2.0 ** -33, mean_kind="full"))))
    zeros = [0.0] * 9 + [0.125 * (1 + i % 12) for i in range(52)]
    c.append(_case("zeros", vals(zeros, "zeros"), vals(zeros[:-2] + [0.0] * 6, "zeros")))
    c.append(_case("float-collisions", _float_collisions(), _float_collisions(), prm="euroc",
                   declare=dict(p=dict(med=600.0, mad=600.0, mean_kind="gated", kept=65), l=dict(med=600.0, mad=600.0, mean_kind="gated", kept=65))))
    # ---- gates (n = 61: int(0.2 n) = 12; n = 65: 13)
    def gate_at(ksel, n=61):
        """median 1024, MAD 1 (sigma 1.4826, 2 sigma = 2.9652): ksel values at 1 pass the gate, all others are 1023 .. 1025.
        ksel = int(0.2 n) = 12: the mean is 1; ksel = 11: the mean of everything, ~ 840"""
        h = n // 2
        rest = n - ksel
        # of the rest: the median 1024 sits at overall rank h = ksel + (h - ksel): h - ksel values at 1023 below it, the others 1025
        # deviations: 0 once, 1 for every 1023 / 1025, 1023 for the ones: rank h is 1 as long as 1 + (rest - 1) > h
        return [1.0] * ksel + [1023.0] * (h - ksel) + [1024.0] + [1025.0] * (rest - 1 - (h - ksel))
    for k in (12, 11):
        kind = "gated" if k == 12 else "full"
        c.append(_case(f"gate-count-{k}", vals(gate_at(k), "gate", s2=1.0), vals(gate_at(k + 1, 65), "gate", s2=1.0), prm="euroc",
                       declare=dict(p=dict(med=1024.0, mad=1.0, ksel=k, mean_kind=kind, kept=k if k == 12 else 0),
                                    l=dict(med=1024.0, mad=1.0, ksel=k + 1, mean_kind="gated" if k + 1 >= 13 else "full", kept=13 if k == 12 else 0))))
    # a value exactly at 2 sigma (strict <: it is NOT in the mean) beside 12 ones well below it.  Median 512, MAD 64: 2 sigma is the
    # double 2 * (1.4826 * 64) = 189.77..., the gated mean is 1 (with the gate value it would be 15.5).  The two features at 388 show
    # it: 387 from the right mean and beyond 4 sigma = 379.5 (cut), 372.5 from the wrong one (kept); nothing else is near a threshold
    two_sigma = 2.0 * (1.4826 * 64.0)
    at_gate = [1.0] * 12 + [two_sigma] + [388.0] * 2 + [448.0] * 15 + [512.0] + [576.0] * 30
    c.append(_case("at-two-sigma", vals(at_gate, "gate2", s2=1.0), F65(), prm="euroc",
                   declare=dict(p=dict(med=512.0, mad=64.0, ksel=12, mean_kind="gated", mean=1.0, kept=13))))
    # ---- threshold edges (inlier_k = 4)
    # (the base sets keep mean + 4 sigma inside the binade of 4 sigma, so that some double r has fl(r - mean) == 4 sigma)
    doubled = lambda n: vals([2.0 * v[0] for v in sensitive(n + 2)[:-2]], "sens2")   # with the two edge features: median 2, MAD 1, 4 sigma = 5.93
    c.append(_case("threshold-edge-points", _edge_tail(doubled(63), 4.0, "edge"), F65(), prm="edge"))
    c.append(_case("threshold-edge-lines", F61(), _edge_tail(doubled(62), 4.0, "edge"), prm="edge"))
    c.append(_case("threshold-edge-float-mad", _edge_tail(_float_collisions(), 4.0, "edge"), _edge_tail(sensitive(65)[:-2], 4.0, "edge"), prm="edge"))
    # ---- initial masks: matched features that arrive as outliers count in median, MAD and mean and are never re-admitted
    rs = [r for r, *_ in spread(61)]
    inl = [i % 3 != 0 for i in range(61)]
    c.append(_case("arrive-as-outliers", vals(rs, "mask", inl=inl), vals(rs + rs[:4], "mask", inl=[i % 4 != 1 for i in range(65)])))
    # the 20 lowest values arrive as outliers: without them the median would be another
    low_out = sorted(rs)
    c.append(_case("low-third-arrives-as-outliers", vals(low_out, "mask", s2=1.0, inl=[i >= 20 for i in range(61)]), F65()))
    # ---- a cut below min_features
    c.append(_case("cut-below-min-features", vals(half[:-1] + [7.0], "half"), [], declare=dict(p=dict(kept=0))))
    # ---- every plan on the other kind of feature as well (where it fits the 512 key-lines)
    flip = {"p": "l", "l": "p"}
    for k in list(c):
        if len(k["P"]) <= 512 and not k["name"].startswith(PAIRED):
            c.append(dict(k, name=k["name"] + "-swapped", P=k["L"], L=k["P"], has_points=k["has_lines"], has_lines=k["has_points"],
                          declare={flip[s]: d for s, d in k["declare"].items()}, inexact="".join(flip[s] for s in k["inexact"])))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """every case with its plans completed: `keep` stated by expected(), the declared statistics asserted"""
    out = []
    for k, c in enumerate(_specs()):
        c = dict(c)
        c["seed"] = 52000 + k if c["seed"] is None else c["seed"]
        ik = params(dict(c, has_points=1, has_lines=1)).inlier_k
        c["stats"] = {}
        for side, raw in (("p", c.pop("P")), ("l", c.pop("L"))):
            kept, st = expected([v[0] for v in raw], [v[2] for v in raw], ik)
            for key, want in c["declare"].get(side, {}).items():
                got = int(kept.sum()) if key == "kept" else getattr(st, key)
                assert got == want, (c["name"], side, key, got, want)
            # a mean whose sum rounds is admitted only where no decision can feel it: threshold 0 and nothing within 1 of the mean
            assert st.exact or (side in c["inexact"] and st.th == 0.0 and all(abs(v[0] - st.mean) > 1.0 for v in raw)), (c["name"], side)
            c["plan_" + side] = [Feat(v[0], v[1], v[2], bool(kp), v[3]) for v, kp in zip(raw, kept)]
            c["stats"][side] = st
        out.append(c)
    assert len({c["name"] for c in out}) == len(out)
    return out


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def built(name, at_identity=False):
    """(rec, order_p, order_l, expect_p, expect_l) of a case, built once and never modified by its users.  at_identity: the same plan
    for the initial pose I, which is what the batched entry and the device pipeline start from (the committed pose is then I, the
    rejected solution: status 3 — the cut and its flags are the same)"""
    c = by_name(name)
    rec, op, ol = records(c, (0.0, 0.0, 0.0) if at_identity else T0_TRANS)
    ep, el = expect_masks(c, op, ol)
    return rec, op, ol, ep, el


_ORACLE = {}


def oracle_pose(orc, name, mode=0, at_identity=False):
    """oracle.optimize_pose of a case at DT0 (or at I), once per (case, mode)"""
    key = (name, mode, at_identity)
    if key not in _ORACLE:
        _ORACLE[key] = orc.optimize_pose(np.eye(4) if at_identity else DT0, CAM, params(by_name(name), mode=mode), built(name, at_identity)[0])
    return _ORACLE[key]


# ---- point plans as stereo sequences: the way to pose2c_kernel (compact records) ---------------------------------------------------------
PIPELINE_CASES = ["sensitive-64-65", "duplicate-blocks", "all-equal", "half-equal", "symmetric", "zeros", "spread-449-65-kitti", "eighth-key-897"]


@functools.lru_cache(maxsize=None)
def pipeline_sequence(name):
    """(frames [2], r [n], keep [n]) — the residuals of the case's point plan as a two-frame stereo sequence for the device pipeline
    (stereo_tail_cases.FrameBuilder on GRID_CAM, kitti matching): left key-point i of the first frame has the disparity 64, 128 or
    256 (b / disp is a power of two: the back-projection is exact) and its own descriptor; the second frame's left key-point i
    carries the same descriptor and lies r[i] beside it along one axis, so at DT = I — where the pipeline starts — the residual
    of pair i is r[i] exactly.  Every key-point is on pyramid level 0: sigma2 = 1 (the plan's own sigma2 is not used).  keep[i]: what the
    cut leaves, stated by expected() for the kitti inlier_k."""
    from stereo_tail_cases import FrameBuilder
    c = by_name(name)
    r = np.array([f.r for f in c["plan_p"]], np.float64)
    n = len(r)
    assert n >= 10 and np.all(r * 4096.0 == np.rint(r * 4096.0)) and r.max() <= 64.0   # a float coordinate below 2048 carries it
    rng = np.random.default_rng(c["seed"] + 700000)
    order = rng.permutation(n)
    r = r[order]
    keep, _ = expected(r, np.ones(n, bool), opt_params("kitti").inlier_k)
    fb0, fb1 = FrameBuilder(c["seed"]), FrameBuilder(c["seed"])   # the same seed and counts: the same left descriptors in both frames
    for i in range(n):
        x, y = 384.0 + 0.25 * float(rng.integers(0, 4 * 1500)), 80.0 + 0.25 * float(rng.integers(0, 4 * 1360))
        disp = (64.0, 128.0, 256.0)[int(rng.integers(0, 3))]
        sgn = 1.0 if (i // 2) % 2 == 0 else -1.0
        xo, yo = (x + sgn * r[i], y) if i % 2 == 0 else (x, y + sgn * r[i])
        fb0.point(x, y, (x - disp, y), name=f"{name}[{order[i]}]")
        fb1.point(xo, yo, (xo - (64.0, 128.0, 256.0)[int(rng.integers(0, 3))], yo), name=f"{name}[{order[i]}]")
    f0, f1 = fb0.build(name + " frame 0", True), fb1.build(name + " frame 1", True)
    assert np.array_equal(f0["frame"]["desc_l"], f1["frame"]["desc_l"])
    for f in (f0, f1):
        f["frame"]["ang_l"] = np.zeros(0, np.float32)
    return [f0["frame"], f1["frame"]], r, keep
