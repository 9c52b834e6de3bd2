"""Problems that put every stop rule, branch and verdict of optimizePose where it is planned — TEST INFRASTRUCTURE ONLY, shared by
tests/test_pose_flow_host.py (CPU) and tests/test_gpu_pose_flow.py.

A case is a small problem (12 to 64 points, 0 to 8 key-lines: the flow does not depend on the count) from synth.make_matched_records
on one of the two cameras of pose_edge_cases, an initial pose, the optimiser parameters, and a PLAN: (status, path, iters), the rule
that ends each stage and the regime of each verdict (np_pose_flow).  The plans are written down in PLAN below; cases() builds every
case (on first use: importing this module builds nothing) and runs the extended statement on it once and the host test holds the statement, the oracle and np_model to the plan.

Thresholds are PLACED: the statement runs with min_error = min_error_change = 0 (both rules off), and the parameter becomes the
geometric mean of the two trace values it has to separate (_place_err_change, _place_step, min_error between err_k and err_k-1).
Both the error-change rule and the step rule read min_error_change; where the trace of sigma2 = 1 does not separate them the
feature weights do: sigma2 scales err by sigma2 and the step by sqrt(sigma2) (r = |e| sqrt(sigma2) at :589-591 / :658-660; the gradient carries no sigma2), so the
search walks a short list of sigma2 (robust GN ignores sigma2: it walks the pixel noise).  Edges in continuous quantities — lambda_max
and ||.||_inf of the covariance, |det H|, the robust err — are reached by bisection of ONE scene parameter (depth scale, pixel noise)
on the statement, landing between 1e-3 and 1e-2 beside the edge.  Seeds, lists and brackets are pinned here; a generator that cannot
reach its property fails (no case is skipped).

Not built, because not reachable or not stated anywhere:
  * GN's err > err_prev at the FIRST evaluation and err > 1 in modes 0 and 2: each term is r^2 w = r^2 / (1 + r^2) < 1, so err < 1 <
    999999999.9 for finite input; the host test asserts that bound on every trace instead;
  * a negative eigenvalue of the covariance;
  * GN or robust GN with max_iters = 0 (Eigen's inverse of the zero matrix is not stated);
  * log|det H| < 0 after a step FROM I: there the first robust step raises log|det H| by ~13 (the weights recover).  The edge after a
    step is placed from a start at the true motion instead (_lad_after_step_cases), where a step lowers it; those cases do not start
    at I, so they reach the kernels through stvo_optimize_pose only."""
import functools
import math

import numpy as np

import np_model
import np_pose_flow as npf
import pose_edge_cases as pec
from stvo_amd import synth
from stvo_amd.ctypes_types import opt_params

CAMS = (pec.CAM_A, pec.CAM_B)
I4 = np.eye(4)
OFF = dict(min_error=0.0, min_error_change=0.0)
REC_KEYS = ("P", "pl_obs", "sigma2p", "inlier_p", "sP", "eP", "le_obs", "spl", "epl", "sigma2l", "inlier_l")
EDGE_BELOW, EDGE_ABOVE = (1.0 - 1e-2, 1.0 - 1e-3), (1.0 + 1e-3, 1.0 + 1e-2)
DT_TINY = np.eye(4)
DT_TINY[0, 3] = 1e-12

# (status, path, iters), (rule of the first stage, rule of the second or None), (regime after stage 1, regime at the commit)
PLAN = {
    "gn-maxit-1": ((0, 2, (1, 3)), ('max_iters', 'max_iters'), ('C', 'A')),
    "gn-maxit-2": ((0, 5, (2, 3)), ('max_iters', 'max_iters'), ('A', 'A')),
    "gnr-maxit-1": ((0, 2, (1, 3)), ('max_iters', 'max_iters'), ('A', 'A')),
    "gnr-maxit-2": ((2, 1, (2, 0)), ('max_iters', None), ('A', 'A')),
    "gn-ref-maxit-1": ((0, 5, (4, 1)), ('max_iters', 'max_iters'), ('A', 'A')),
    "gnr-ref-maxit-1": ((3, 5, (4, 1)), ('max_iters', 'max_iters'), ('A', 'A')),
    "fallback-maxit-1": ((3, 2, (4, 1)), ('max_iters', 'max_iters'), ('C', 'C')),
    "lm-maxit-0": ((0, 5, (1, 1)), ('max_iters', 'max_iters'), ('A', 'A')),
    "lm-maxit-1": ((0, 5, (1, 1)), ('max_iters', 'max_iters'), ('A', 'A')),
    "lm-maxit-2": ((3, 5, (2, 1)), ('max_iters', 'max_iters'), ('A', 'C')),
    "gn-min-error-1": ((3, 5, (1, 1)), ('min_error', 'min_error'), ('A', 'A')),
    "gn-min-error-2": ((0, 5, (2, 2)), ('min_error', 'min_error'), ('A', 'A')),
    "gn-min-error-3": ((0, 5, (3, 2)), ('min_error', 'min_error'), ('A', 'A')),
    "gnr-min-error-1": ((3, 2, (1, 1)), ('min_error', 'min_error'), ('A', 'A')),
    "gnr-min-error-2": ((3, 2, (2, 2)), ('min_error', 'min_error'), ('A', 'A')),
    "gnr-min-error-3": ((0, 5, (3, 2)), ('min_error', 'min_error'), ('A', 'A')),
    "lm-min-error-1": ((0, 5, (2, 2)), ('min_error', 'min_error'), ('A', 'A')),
    "lm-min-error-2": ((0, 5, (2, 2)), ('min_error', 'min_error'), ('A', 'A')),
    "lm-min-error-3": ((0, 5, (3, 2)), ('min_error', 'min_error'), ('A', 'A')),
    "gn-err-change-4": ((0, 5, (4, 4)), ('err_change', 'err_up'), ('A', 'A')),
    "gn-step-2": ((0, 5, (2, 2)), ('step', 'step'), ('A', 'A')),
    "gnr-err-change-4": ((0, 5, (4, 3)), ('err_change', 'step'), ('A', 'A')),
    "gnr-step-2": ((3, 2, (2, 2)), ('step', 'step'), ('A', 'A')),
    "lm-err-change-4": ((0, 5, (4, 3)), ('err_change', 'step'), ('A', 'A')),
    "lm-step-2": ((0, 5, (2, 2)), ('step', 'step'), ('A', 'A')),
    "two-norm-t-dominated": ((0, 5, (2, 2)), ('max_iters', 'max_iters'), ('A', 'A')),
    "two-norm-r-dominated": ((0, 5, (2, 2)), ('step', 'step'), ('A', 'A')),
    "two-norm-lm-t-dominated": ((0, 5, (3, 2)), ('max_iters', 'max_iters'), ('A', 'A')),
    "two-norm-lm-r-dominated": ((0, 5, (3, 2)), ('max_iters', 'max_iters'), ('A', 'A')),
    "two-norm-both-below-gn": ((0, 5, (1, 2)), ('step', 'step'), ('A', 'A')),
    "two-norm-both-below-gnr": ((3, 5, (2, 2)), ('step', 'step'), ('A', 'A')),
    "gn-err-up-far": ((0, 5, (2, 2)), ('err_up', 'err_up'), ('A', 'A')),
    "gn-err-up-at-I": ((0, 5, (5, 6)), ('err_up', 'err_up'), ('A', 'A')),
    "lm-err-up-far": ((0, 5, (4, 4)), ('max_iters', 'max_iters'), ('A', 'A')),
    "lm-down-up-at-I": ((0, 5, (8, 8)), ('max_iters', 'max_iters'), ('A', 'A')),
    "gnr-lad-below": ((3, 2, (1, 1)), ('lad', 'lad'), ('A', 'A')),
    "fallback-lad-below": ((3, 2, (2, 1)), ('max_iters', 'lad'), ('C', 'A')),
    "gnr-lad-above": ((3, 2, (2, 2)), ('max_iters', 'max_iters'), ('C', 'C')),
    "fallback-lad-above": ((3, 2, (2, 2)), ('max_iters', 'max_iters'), ('C', 'C')),
    "gnr-lad-below-after-step": ((3, 2, (2, 2)), ('lad', 'lad'), ('A', 'A')),
    "fallback-lad-below-after-step": ((3, 2, (3, 2)), ('err_up', 'lad'), ('C', 'A')),
    "gnr-lad-above-after-step": ((3, 2, (3, 3)), ('lad', 'lad'), ('A', 'A')),
    "fallback-lad-above-after-step": ((3, 2, (3, 3)), ('err_up', 'lad'), ('C', 'A')),
    "verdict-stage1-A": ((0, 5, (2, 2)), ('max_iters', 'max_iters'), ('A', 'B')),
    "verdict-stage1-B": ((3, 5, (2, 2)), ('max_iters', 'max_iters'), ('B', 'C')),
    "verdict-stage1-C": ((3, 2, (2, 2)), ('max_iters', 'max_iters'), ('C', 'C')),
    "verdict-commit-A": ((0, 5, (2, 2)), ('max_iters', 'max_iters'), ('A', 'A')),
    "verdict-commit-B": ((0, 5, (2, 2)), ('max_iters', 'max_iters'), ('B', 'B')),
    "verdict-commit-C": ((3, 5, (2, 2)), ('max_iters', 'max_iters'), ('B', 'C')),
    "verdict-robust-err-below": ((0, 2, (1, 3)), ('max_iters', 'max_iters'), ('A', 'A')),
    "verdict-robust-err-above": ((3, 2, (1, 3)), ('max_iters', 'max_iters'), ('A', 'A')),
    "identity-1e-12": ((0, 5, (1, 1)), ('min_error', 'min_error'), ('A', 'A')),
    "identity-exact": ((3, 5, (1, 1)), ('min_error', 'min_error'), ('A', 'A')),
    "min-features-entry-exact": ((2, 1, (4, 0)), ('err_up', None), ('A', 'A')),
    "min-features-entry-one-fewer": ((1, 0, (0, 0)), (None, None), (None,)),
    "min-features-cut-exact": ((0, 5, (5, 5)), ('err_up', 'err_up'), ('A', 'A')),
    "min-features-cut-one-fewer": ((2, 1, (5, 0)), ('err_up', None), ('A', 'A')),
    "pts-gn-err-up": ((0, 5, (5, 5)), ('err_up', 'err_up'), ('A', 'A')),
    "pts-lm-down-up": ((0, 5, (8, 8)), ('max_iters', 'max_iters'), ('A', 'A')),
    "pts-gn-maxit-2": ((0, 5, (2, 3)), ('max_iters', 'max_iters'), ('A', 'A')),
    "pts-gn-step-3": ((0, 5, (3, 3)), ('step', 'step'), ('A', 'A')),
    "pts-gnr-lad-below": ((3, 2, (1, 1)), ('lad', 'lad'), ('A', 'A')),
    "pts-fallback-lad-below": ((3, 2, (2, 1)), ('max_iters', 'lad'), ('C', 'A')),
    "pts-gnr-lad-above": ((3, 2, (2, 2)), ('max_iters', 'max_iters'), ('C', 'C')),
    "pts-fallback-lad-above": ((3, 2, (2, 2)), ('max_iters', 'max_iters'), ('C', 'C')),
    "pts-verdict-stage1-A": ((3, 5, (3, 2)), ('err_up', 'max_iters'), ('A', 'C')),
    "pts-verdict-stage1-B": ((3, 5, (3, 2)), ('err_up', 'max_iters'), ('B', 'C')),
    "pts-verdict-stage1-C": ((3, 2, (3, 2)), ('err_up', 'max_iters'), ('C', 'C')),
    "pts-verdict-commit-A": ((0, 5, (3, 2)), ('err_up', 'max_iters'), ('A', 'A')),
    "pts-verdict-commit-B": ((0, 5, (3, 2)), ('err_up', 'max_iters'), ('A', 'B')),
    "pts-verdict-commit-C": ((3, 5, (3, 2)), ('err_up', 'max_iters'), ('A', 'C')),
    "default-gn": ((0, 5, (5, 6)), ('max_iters', 'err_up'), ('A', 'A')),
    "default-gnr": ((0, 5, (5, 10)), ('max_iters', 'max_iters'), ('A', 'A')),
    "default-lm": ((3, 2, (3, 10)), ('err_change', 'max_iters'), ('C', 'C')),
    "default-lm-lines": ((0, 5, (5, 7)), ('max_iters', 'err_change'), ('A', 'A')),
}


def scene(seed, npts, nl, cam=0, depth=1.0, noise=0.5, outliers=0.15, motion=None, sigma2=None):
    """make_matched_records with depths 4 .. 80 m times `depth`; motion: the se(3) vector of the true motion (None: random_motion)"""
    T = None if motion is None else np_model.expmap_se3(np.asarray(motion, float))
    rec = synth.make_matched_records(seed, n_pts=npts, n_lines=nl, cam=CAMS[cam], outlier_frac=outliers, noise_px=noise,
                                     depth=(4.0 * depth, 80.0 * depth), motion=T)
    rec = {k: rec[k] for k in REC_KEYS}
    if sigma2 is not None:
        rec["sigma2p"], rec["sigma2l"] = np.full(npts, float(sigma2)), np.full(nl, float(sigma2))
    return rec


def params(case):
    return opt_params(case["preset"], **case["prm"])


def _cam(cam):
    """a camera of CAMS by its index, or a camera dict of its own (stereo_scene: the baseline carries the depth scale)"""
    return cam if isinstance(cam, dict) else CAMS[cam]


def cam_of(case):
    return _cam(case["cam"])


def statement(rec, cam, DT0=I4, preset="kitti", **prm):
    return npf.optimize_pose(DT0, _cam(cam), np_model.prm_dict(opt_params(preset, **prm)), rec)


def _case(name, rec, cam, DT0=I4, preset="kitti", tags=(), src=None, **prm):
    n, nl = len(rec["sigma2p"]), len(rec["sigma2l"])
    assert 12 <= n <= 64 and 0 <= nl <= 8, (name, n, nl)
    return dict(name=name, rec=rec, cam=cam, DT0=np.array(DT0, float), preset=preset, prm=prm, tags=set(tags), src=src)


F32 = np.float32


def stereo_scene(seed, npts, depth=1.0, noise=0.5, outliers=0.15, motion=None):
    """A point-only scene AS THE DEVICE PIPELINE BUILDS IT from a two-frame stereo sequence (src/stereoFrame.cpp:152-167,
    src/pinholeStereoCamera.cpp:221-229): the previous frame's left key-points and the observations are floats, the disparity is a
    float difference, P = backProjection(u, v, disparity).  The depth scale goes into the BASELINE (b * depth: the whole scene grows
    with it), so the disparities stay those of the 4 .. 80 m scene — 5 to 97 pixels, no float cancellation — at any scale.  Features
    that leave the image in either frame are dropped.  -> (rec, camera dict, src = the float coordinates of both frames)"""
    cam = dict(CAMS[0], b=CAMS[0]["b"] * depth)
    full = scene(seed, npts, 0, cam=0, depth=depth, noise=noise, outliers=outliers, motion=motion)
    P = full["P"]
    u = (cam["cx"] + cam["fx"] * P[:, 0] / P[:, 2]).astype(F32)
    v = (cam["cy"] + cam["fy"] * P[:, 1] / P[:, 2]).astype(F32)
    xr = (u.astype(np.float64) - cam["b"] * cam["fx"] / P[:, 2]).astype(F32)
    obs = full["pl_obs"].astype(F32)
    inside = lambda x, y: (x >= 24) & (x <= cam["width"] - 4) & (y >= 4) & (y <= cam["height"] - 4)   # noqa: E731
    keep = inside(u, v) & inside(obs[:, 0], obs[:, 1]) & (u - xr >= 2)
    u, v, xr, obs = u[keep], v[keep], xr[keep], obs[keep]
    bd = cam["b"] / (u - xr).astype(np.float64)   # the float difference, widened (:159)
    ud, vd = u.astype(np.float64), v.astype(np.float64)
    n = len(u)
    z3, z2 = np.zeros((0, 3)), np.zeros((0, 2))
    rec = dict(P=np.ascontiguousarray(np.stack([bd * (ud - cam["cx"]), bd * (vd - cam["cy"]), bd * cam["fx"]], 1)),
               pl_obs=np.ascontiguousarray(obs.astype(np.float64)), sigma2p=np.ones(n), inlier_p=np.ones(n, np.int32), sP=z3, eP=z3.copy(),
               le_obs=z3.copy(), spl=z2, epl=z2.copy(), sigma2l=np.zeros(0), inlier_l=np.zeros(0, np.int32))
    return rec, cam, dict(kp0=np.stack([u, v], 1), xr0=xr, kp1=obs)


def _gm(a, b):
    return float(math.sqrt(float(a) * float(b)))


def _stage(tr, stage=0):
    return next(s for s in tr["stages"] if s["stage"] == stage)


def _d(ev):
    return float(abs(ev["err"] - ev["err_prev"]))


def _stepn(ev, alg):
    """the step norm the rule of `alg` has to see below the threshold"""
    return float(ev["n6"]) if alg == 1 else max(float(ev["nt"]), float(ev["nr"]))


def _place_err_change(evs, alg, k):
    """(ratio, threshold) for |err_k - err_k-1| < c while everything read before stays at or above c; evaluations count from 1"""
    first = 1 if alg == 2 else 0   # LM's first evaluation runs no rule
    if any(e["err"] > e["err_prev"] for e in evs[:k]):
        return 0.0, None
    lower = _d(evs[k - 1])
    upper = min([_d(evs[j]) for j in range(max(first, 1), k - 1)] + [_stepn(evs[j], alg) for j in range(first, k - 1)] + [16.0 * lower])
    return upper / lower, _gm(lower, upper)


def _place_step(evs, alg, k):
    first = 1 if alg == 2 else 0
    if any(e["err"] > e["err_prev"] for e in evs[:k]) or k - 1 < first:
        return 0.0, None
    lower = _stepn(evs[k - 1], alg)
    upper = min([_d(evs[j]) for j in range(max(first, 1), k)] + [_stepn(evs[j], alg) for j in range(first, k - 1)] + [16.0 * lower])
    return upper / lower, _gm(lower, upper)


def _bisect(f, lo, hi, window, steps=80):
    """x in [lo, hi] (geometric bisection) with f(x) inside `window`; f is monotone there"""
    flo, fhi = f(lo), f(hi)
    mid = 0.5 * (window[0] + window[1])
    assert (flo - mid) * (fhi - mid) < 0, ("the bracket does not hold the edge", flo, fhi, window)
    for _ in range(steps):
        x = math.sqrt(lo * hi)
        fx = f(x)
        if window[0] < fx < window[1]:
            return x
        if (fx - mid) * (flo - mid) > 0:
            lo, flo = x, fx
        else:
            hi = x
    raise AssertionError(("bisection did not land in the window", window, lo, hi))


# ---- the builders ------------------------------------------------------------------------------------------------------------------
MODE_TAG = {0: "gn", 1: "gnr", 2: "lm"}


def _max_iters_cases():
    c = []
    for mode in (0, 1):
        for m in (1, 2):
            c.append(_case(f"{MODE_TAG[mode]}-maxit-{m}", scene(101 + m, 24, 4, cam=mode), mode, preset="euroc", mode=mode, max_iters=m, max_iters_ref=3, **OFF))
    # a long stage 1, then ONE evaluation of the refinement: T_opt is one step from the INITIAL pose on the cut set
    c.append(_case("gn-ref-maxit-1", scene(105, 40, 6), 0, tags=["one_step"], mode=0, max_iters=4, max_iters_ref=1, **OFF))
    c.append(_case("gnr-ref-maxit-1", scene(106, 32, 0, cam=1), 1, tags=["one_step"], mode=1, max_iters=4, max_iters_ref=1, **OFF))
    # the robust fallback's restart: a scene ten times beyond the regime-C edge, a long stage 1, one evaluation of the fallback
    c.append(_case("fallback-maxit-1", scene(107, 24, 4, depth=150.0, outliers=0.05), 0, tags=["one_step"], mode=0, max_iters=4, max_iters_ref=1, **OFF))
    for m in (0, 1, 2):   # LM evaluates once and steps once even at 0 and 1
        c.append(_case(f"lm-maxit-{m}", scene(110 + m, 16, 8, cam=m % 2), m % 2, mode=2, max_iters=m, max_iters_ref=1, **OFF))
    return c


def _min_error_cases():
    c = []
    for mode in (0, 1, 2):
        rec = scene(120 + mode, 40, 6, cam=mode % 2)
        evs = _stage(statement(rec, mode % 2, mode=mode, max_iters=4, max_iters_ref=1, **OFF)[1])["evals"]
        assert all(evs[j]["err"] < evs[j - 1]["err"] for j in (1, 2)), "the error must fall over the first three evaluations"
        for k in (1, 2, 3):
            me = 4.0 * float(evs[0]["err"]) if k == 1 else _gm(evs[k - 1]["err"], evs[k - 2]["err"])
            # (LM runs no rule at its first evaluation: min_error above err_1 ends it at the second)
            c.append(_case(f"{MODE_TAG[mode]}-min-error-{k}", rec, mode % 2, mode=mode, max_iters=6, max_iters_ref=6, min_error=me, min_error_change=0.0))
    return c


SIGMA2_WALK = (1.0, 0.25, 4.0, 0.04, 25.0, 0.01, 1e-3, 1e-4)
NOISE_WALK = (0.5, 0.2, 1.0, 0.1, 2.0, 0.05)


def _change_and_step_cases():
    """the error-change rule at evaluation k with the steps above the shared threshold, the step rule with the error change above it"""
    c = []
    for mode in (0, 1, 2):
        for what, place, ks in (("err-change", _place_err_change, (3, 4, 5, 2)), ("step", _place_step, (2, 3, 4, 1))):
            found = []   # the first knob at which an evaluation of ks[:-1] separates the rules by 1.5 x; ks[-1] (always there) otherwise
            for knob in (NOISE_WALK if mode == 1 else SIGMA2_WALK):
                rec = scene(130 + mode, 48, 8, cam=(mode + 1) % 2, **(dict(noise=knob) if mode == 1 else dict(sigma2=knob)))
                evs = _stage(statement(rec, (mode + 1) % 2, mode=mode, max_iters=6, max_iters_ref=1, **OFF)[1])["evals"]
                for k in ks:
                    ratio, th = place(evs, mode, k) if k <= len(evs) else (0.0, None)
                    if ratio >= 1.5:
                        found.append((k == ks[-1], rec, k, th))
                if any(not last for last, *_ in found):
                    break
            assert found, (mode, what)
            _, rec, k, th = sorted(found, key=lambda f: f[0])[0]
            c.append(_case(f"{MODE_TAG[mode]}-{what}-{k}", rec, (mode + 1) % 2, tags=[what], mode=mode, max_iters=8, max_iters_ref=8, min_error=0.0, min_error_change=th))
    return c


def _two_norm_cases():
    """GN / LM stop when BOTH 3-norms are below c (:421, :539), robust GN when the 6-norm is (:462)"""
    c = []
    # translation-dominated and rotation-dominated first steps: c between the two norms, the loop goes on; max_iters = 2 ends it
    fwd = [((0.05, -0.1, -0.8, 0, 0, 0), 1.0)]
    yaw = [((0, 0, 0, 0, 0.01, 0), d) for d in (0.1, 0.3, 1.0)]   # near points pin the translation: metres against radians
    yaw_lm = [((0, 0, 0, 0, 0.03, 0), d) for d in (0.005, 0.002)]   # LM's first checked step is its second: the translation left by then shrinks with the depth
    for name, motions, mode in (("t-dominated", fwd, 0), ("r-dominated", yaw, 0), ("lm-t-dominated", fwd, 2), ("lm-r-dominated", yaw_lm, 2)):
        for motion, depth in motions:
            rec = scene(140, 40, 6, cam=1, motion=motion, depth=depth, noise=0.2, outliers=0.0)
            evs = _stage(statement(rec, 1, mode=mode, max_iters=3, max_iters_ref=1, **OFF)[1])["evals"]
            e = evs[1] if mode == 2 else evs[0]   # LM reads the norms from its second evaluation on
            nt, nr = float(e["nt"]), float(e["nr"])
            th = _gm(nt, nr)
            silent = all(_d(x) > 2 * th for x in (evs[1:3] if mode == 2 else evs[1:2]))   # the error-change rule stays silent
            if ((nt > 2 * nr) if "t-" in name else (nr > 2 * nt)) and silent:
                break
        else:
            raise AssertionError((name, nt, nr))
        c.append(_case(f"two-norm-{name}", rec, 1, tags=["two-norm-" + name.replace("lm-", "")], mode=mode, max_iters=3 if mode == 2 else 2, max_iters_ref=2,
                       min_error=0.0, min_error_change=th))
    # both 3-norms below c, the 6-norm above it: GN stops at its first evaluation, robust GN goes on
    depth = 0.3
    for _ in range(4):   # balance |inc_t| against |inc_r| of the first step: the translation that explains a rotation grows with the depth
        rec = scene(141, 48, 4, motion=(0.03, -0.02, -0.04, 0.01, 0.05, -0.02), depth=depth, noise=0.2, outliers=0.0)
        g = _stage(statement(rec, 0, mode=0, max_iters=1, max_iters_ref=1, **OFF)[1])["evals"][0]
        r = _stage(statement(rec, 0, mode=1, max_iters=1, max_iters_ref=1, **OFF)[1])["evals"][0]
        if 0.8 < float(g["nt"]) / float(g["nr"]) < 1.25:
            break
        depth *= float(g["nr"]) / float(g["nt"])
    lo = max(float(v[k]) for v in (g, r) for k in ("nt", "nr"))
    hi = min(float(g["n6"]), float(r["n6"]))
    assert hi > 1.1 * lo, (lo, hi)
    th = _gm(lo, hi)
    c.append(_case("two-norm-both-below-gn", rec, 0, tags=["both-below"], mode=0, max_iters=5, max_iters_ref=5, min_error=0.0, min_error_change=th))
    c.append(_case("two-norm-both-below-gnr", rec, 0, tags=["six-norm-above"], mode=1, max_iters=5, max_iters_ref=5, min_error=0.0, min_error_change=th))
    return c


def _err_up_cases():
    far = scene(7, 40, 6, cam=1, motion=np.zeros(6))
    c = [_case("gn-err-up-far", far, 1, DT0=pec.DT_FIXED, mode=0, max_iters=6, max_iters_ref=6, **OFF),            # started far off: stage 1 and the refinement both rise at evaluation 2
         _case("gn-err-up-at-I", scene(6, 40, 6), 0, mode=0, max_iters=10, max_iters_ref=10, **OFF),               # after four to six evaluations
         _case("lm-err-up-far", far, 1, DT0=pec.DT_FIXED, mode=2, max_iters=4, max_iters_ref=4, **OFF),            # lambda / 4 without a step, then * 4 with one
         _case("lm-down-up-at-I", scene(6, 40, 6), 0, tags=["lm-damped"], mode=2, max_iters=8, max_iters_ref=8, **OFF)]   # on GN's trace: err falls, rises, falls, rises
    return c


def _first(tr, stage):
    return _stage(tr, stage)["evals"][0]


def _plain(mk):
    """a maker of (rec, cam, src) from a maker of plain records on camera 0"""
    return lambda x: (mk(x), 0, None)


def _lad_cases(mk=None, prefix="", bracket=(300.0, 30000.0)):
    """|det H| of robust GN's first solve on each side of 1, in mode 1 and in the fallback of mode 0 (same scene: stage 1 of GN ends in
    regime C there)"""
    c = []
    mk = mk or _plain(lambda depth: scene(160, 24, 4, depth=depth, outliers=0.0))

    def det(x):
        rec, cam, _ = mk(x)
        return float(np.exp(_first(statement(rec, cam, mode=1, max_iters=1, max_iters_ref=1, **OFF)[1], 0)["lad"]))
    for side, window in (("below", EDGE_BELOW), ("above", EDGE_ABOVE)):
        rec, cam, src = mk(_bisect(det, bracket[0], bracket[1], window))
        c.append(_case(f"{prefix}gnr-lad-{side}", rec, cam, tags=["lad-" + side], src=src, mode=1, max_iters=2, max_iters_ref=2, **OFF))
        c.append(_case(f"{prefix}fallback-lad-{side}", rec, cam, tags=["lad-" + side], src=src, mode=0, max_iters=2, max_iters_ref=2, **OFF))
    return c


LAD_MOTION = (0.02, -0.01, -0.9, 0.004, -0.006, 0.003)


def _lad_after_step_cases():
    """|det H| of robust GN's SECOND solve on each side of 1 while the first is above it.  Started at the true motion the weights
    are as large as they get and the first step, pure noise, lowers log|det H| (by 0.41 in this scene, at any depth scale: it is the
    scene that scales); below 1 the pose that comes back must be the saved entry pose, not the stepped one."""
    c = []
    DT0 = np_model.expmap_se3(np.asarray(LAD_MOTION))
    mk = lambda depth: scene(162, 24, 4, depth=depth, outliers=0.0, motion=LAD_MOTION)   # noqa: E731

    def det(x):
        evs = _stage(statement(mk(x), 0, DT0=DT0, mode=1, max_iters=2, max_iters_ref=1, **OFF)[1])["evals"]
        return float(np.exp(evs[1]["lad"])) if len(evs) > 1 else 0.0   # (so far out that the FIRST solve is below 1 already)
    for side, window in (("below", EDGE_BELOW), ("above", EDGE_ABOVE)):
        rec = mk(_bisect(det, 3000.0, 3e6, window))
        c.append(_case(f"gnr-lad-{side}-after-step", rec, 0, DT0=DT0, tags=["lad-" + side, "lad-at-2"], mode=1, max_iters=3, max_iters_ref=3, **OFF))
        c.append(_case(f"fallback-lad-{side}-after-step", rec, 0, DT0=DT0, tags=["lad-" + side, "lad-at-2"], mode=0, max_iters=3, max_iters_ref=3, **OFF))
    return c


VERDICT_PRM = dict(mode=0, max_iters=2, max_iters_ref=2, **OFF)   # two evaluations a stage, both rules off


def _regime_cases(mk=None, prefix="", bracket=(1.0, 60.0), preset="euroc", prm=VERDICT_PRM):
    """lambda_max and ||.||_inf of the covariance beside 1, after stage 1 and at the commit"""
    c = []
    mk = mk or _plain(lambda depth: scene(170, 32, 4, depth=depth, outliers=0.05))

    def quantity(site, key):
        def f(x):
            rec, cam, _ = mk(x)
            out, tr = statement(rec, cam, preset=preset, **prm)
            if site == "commit" and out["path"] != 5:   # the commit of the REFINEMENT is wanted: beyond stage 1's own edge counts as above
                return 1e3
            v = [v for v in tr["verdicts"] if v["site"] == site][0]
            return float(v["eig"][5] if key == "lmax" else v["norm_inf"])
        return f
    for name, site, key, window in (("stage1-A", "stage1", "ninf", EDGE_BELOW), ("stage1-B", "stage1", "lmax", EDGE_BELOW),
                                    ("stage1-C", "stage1", "lmax", EDGE_ABOVE), ("commit-A", "commit", "ninf", EDGE_BELOW),
                                    ("commit-B", "commit", "lmax", EDGE_BELOW), ("commit-C", "commit", "lmax", EDGE_ABOVE)):
        rec, cam, src = mk(_bisect(quantity(site, key), bracket[0], bracket[1], window))
        c.append(_case(f"{prefix}verdict-{name}", rec, cam, preset=preset, tags=["verdict-" + name], src=src, **prm))
    return c


def _verdict_cases():
    c = _regime_cases()
    # the robust err at the commit on each side of 1: stage 1 (one evaluation at I, err ~ 7) fails, the fallback's third evaluation decides
    rprm = dict(mode=1, max_iters=1, max_iters_ref=3, **OFF)
    mkn = lambda noise: scene(171, 48, 6, cam=1, noise=noise, outliers=0.0)   # noqa: E731
    for side, window in (("below", EDGE_BELOW), ("above", EDGE_ABOVE)):
        noise = _bisect(lambda x: float(statement(mkn(x), 1, **rprm)[1]["verdicts"][-1]["err"]), 0.3, 30.0, window)
        c.append(_case(f"verdict-robust-err-{side}", mkn(noise), 1, tags=["robust-err-" + side], **rprm))
    # a commit that differs from I by 1e-12 is a solution; its twin that starts at I is "DT == Identity" (:372)
    still = scene(172, 40, 6, motion=np.zeros(6))
    c.append(_case("identity-1e-12", still, 0, DT0=DT_TINY, tags=["almost-identity"], mode=0, min_error=1e30))
    c.append(_case("identity-exact", still, 0, tags=["identity"], mode=0, min_error=1e30))
    return c


def _min_features_cases():
    """n_inliers counts the SET flags of points plus lines (:332, :345)"""
    rec = scene(180, 16, 4, cam=1, outliers=0.1)
    rec["inlier_p"] = rec["inlier_p"].copy()
    rec["inlier_l"] = rec["inlier_l"].copy()
    rec["inlier_p"][::4] = 0
    rec["inlier_l"][1] = 0
    n_set = int(rec["inlier_p"].sum() + rec["inlier_l"].sum())
    assert n_set == 15
    c = [_case("min-features-entry-exact", rec, 1, preset="euroc", tags=["mf"], mode=0, min_features=n_set),
         _case("min-features-entry-one-fewer", rec, 1, preset="euroc", tags=["mf"], mode=0, min_features=n_set + 1)]
    full = scene(181, 20, 8, outliers=0.2)
    out, _ = statement(full, 0, mode=0, min_features=1)
    m = out["n_inliers_pt"] + out["n_inliers_ls"]
    assert 6 <= m < 28 and out["n_inliers_ls"] > 0
    c += [_case("min-features-cut-exact", full, 0, tags=["mf"], mode=0, min_features=m),
          _case("min-features-cut-one-fewer", full, 0, tags=["mf"], mode=0, min_features=m + 1)]
    return c


PTS_VERDICT_PRM = dict(mode=0, max_iters=3, max_iters_ref=2, inlier_k=1e6, **OFF)


def _pipeline_cases():
    """Point-only cases as the device pipeline builds them (stereo_scene), all on camera A at DT = I: the subset that also runs
    through capi.Sequences, where pose2c_kernel and the lazy_eig commit live.  The regime cases share one parameter set, so four of
    them make a four-stream run."""
    c = []
    rec, cam, src = stereo_scene(201, 56)
    c.append(_case("pts-gn-err-up", rec, cam, src=src, mode=0, max_iters=10, max_iters_ref=10, **OFF))
    c.append(_case("pts-lm-down-up", rec, cam, src=src, mode=2, max_iters=8, max_iters_ref=8, **OFF))
    rec, cam, src = stereo_scene(202, 40)
    c.append(_case("pts-gn-maxit-2", rec, cam, preset="euroc", src=src, mode=0, max_iters=2, max_iters_ref=3, **OFF))
    rec, cam, src = stereo_scene(203, 64)
    evs = _stage(statement(rec, cam, mode=0, max_iters=6, max_iters_ref=1, **OFF)[1])["evals"]
    k = max((k for k in (2, 3, 4) if k <= len(evs)), key=lambda k: _place_step(evs, 0, k)[0])
    ratio, th = _place_step(evs, 0, k)
    assert ratio >= 1.5, ratio
    c.append(_case(f"pts-gn-step-{k}", rec, cam, tags=["step"], src=src, mode=0, max_iters=8, max_iters_ref=8, min_error=0.0, min_error_change=th))
    c += _lad_cases(lambda depth: stereo_scene(204, 28, depth=depth, outliers=0.0), "pts-")
    # (no cut, inlier_k = 1e6, so that every quantity is continuous in the depth; the refinement stops one evaluation short of stage 1,
    #  on an H with smaller weights: its covariance is the larger one, and stage 1 is good where the commit is at its edge)
    c += _regime_cases(lambda depth: stereo_scene(206, 36, depth=depth, outliers=0.05), "pts-", prm=PTS_VERDICT_PRM)
    return c


def _mode_cases():
    return [_case("default-gn", scene(190, 64, 8), 0, mode=0),
            _case("default-gnr", scene(191, 64, 8, cam=1), 1, preset="euroc", mode=1),
            _case("default-lm", scene(192, 12, 0), 0, preset="euroc", mode=2),
            _case("default-lm-lines", scene(193, 48, 8, cam=1), 1, mode=2)]


@functools.lru_cache(maxsize=None)
def cases():
    """every case with the statement's result and trace (case["out"], case["trace"]), built once and never modified"""
    out = []
    for build in (_max_iters_cases, _min_error_cases, _change_and_step_cases, _two_norm_cases, _err_up_cases, _lad_cases, _lad_after_step_cases, _verdict_cases,
                  _min_features_cases, _pipeline_cases, _mode_cases):
        out += build()
    assert len({c["name"] for c in out}) == len(out)
    for c in out:
        c["out"], c["trace"] = npf.optimize_pose(c["DT0"], cam_of(c), np_model.prm_dict(params(c)), c["rec"])
    return out


class _Lazy:
    """cases() as a sequence that is built when it is first read, not when a test module is imported"""
    def __iter__(self):
        return iter(cases())

    def __len__(self):
        return len(cases())

    def __getitem__(self, k):
        return cases()[k]


CASES = _Lazy()
ONE_STEP = ["gn-ref-maxit-1", "gnr-ref-maxit-1", "fallback-maxit-1"]   # the cases tagged "one_step" (held to the tags by the host test)


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def course(out, tr):
    """what PLAN states, read from a result and its trace"""
    rules = tuple(s["rule"] for s in tr["stages"]) + (None,) * (2 - len(tr["stages"]))
    regimes = tuple(v["regime"] for v in tr["verdicts"])
    return (out["status"], out["path"], tuple(out["iters"])), rules, regimes


_ORACLE = {}


def oracle_pose(orc, name):
    if name not in _ORACLE:
        c = by_name(name)
        _ORACLE[name] = orc.optimize_pose(c["DT0"], cam_of(c), params(c), c["rec"])
    return _ORACLE[name]


def rel_dev(a, x):
    """max |a - x| / max |x| of a double result from the extended one (0 for two zero arrays)"""
    a = np.asarray(a, np.float64).astype(npf.LD).reshape(-1)
    x = np.asarray(x, dtype=npf.LD).reshape(-1)
    m = float(np.max(np.abs(x)))
    d = float(np.max(np.abs(a - x)))
    return d / m if m > 0 else d


COMPARED = ("T_opt", "T", "cov", "cov_eig", "err")


def oracle_deviation(orc, name):
    """{field: relative deviation of the oracle from the statement} in the fields the GPU test compares"""
    c, ref = by_name(name), oracle_pose(orc, name)
    return {k: rel_dev(ref[k], c["out"][k]) for k in COMPARED}


def batchable(c):
    """usable by the batched entry and the device pipeline: they start at I with every matched feature an inlier"""
    return bool(np.array_equal(c["DT0"], I4) and c["rec"]["inlier_p"].all() and c["rec"]["inlier_l"].all()
                and params(c).has_points and params(c).has_lines)


@functools.lru_cache(maxsize=None)
def pipeline_frames(name):
    """The two-frame stereo sequence (the frame dicts of synth.make_stereo_sequence, points only) from which the device pipeline builds
    the records of a stereo_scene case: frame 0 carries the previous frame's key-points with their right partners on the same row,
    frame 1 the observations (any valid partner: 16 pixels to the left).  Both frames come from stereo_tail_cases.FrameBuilder with
    one seed, so left key-point i carries the same descriptor in both and the f2f match is the identity."""
    from stereo_tail_cases import FrameBuilder
    c = by_name(name)
    src = c["src"]
    seed = 7000 + [k["name"] for k in cases()].index(name)
    fb0, fb1 = FrameBuilder(seed), FrameBuilder(seed)
    for (u, v), xr, (ox, oy) in zip(src["kp0"], src["xr0"], src["kp1"]):
        fb0.point(float(u), float(v), (float(xr), float(v)), name=name)
        fb1.point(float(ox), float(oy), (float(ox) - 16.0, float(oy)), name=name)
    frames = [fb0.build(name + " frame 0", True)["frame"], fb1.build(name + " frame 1", True)["frame"]]
    assert np.array_equal(frames[0]["desc_l"], frames[1]["desc_l"])
    for f in frames:
        f["ang_l"] = np.zeros(0, np.float32)
    return frames


def pipeline_names():
    """the point-only cases of _pipeline_cases, from the pinned plans (no case is built for this)"""
    return [n for n in PLAN if n.startswith("pts-")]


# at least eight cases: err_up, the step rule, a max_iters bound, LM down / up, lad on both sides, regimes A, B and C at the commit
BATCH_CASES = ["gn-err-up-at-I", "gn-step-2", "gn-maxit-2", "lm-down-up-at-I", "gnr-lad-below", "fallback-lad-above", "verdict-commit-A",
               "verdict-commit-B", "verdict-commit-C", "verdict-stage1-B", "verdict-stage1-C", "default-gnr"]


if __name__ == "__main__":   # the plans as the statement gives them, for PLAN
    for c in cases():
        crs = course(c["out"], c["trace"])
        print(f'    "{c["name"]}": {crs},   # margin {c["trace"]["margin"]:.1e}')
