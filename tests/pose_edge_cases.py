"""Inputs that put the per-feature terms of optimizeFunctions[Robust] at their edges — TEST INFRASTRUCTURE ONLY.

(a) single_cases(): one-feature record sets, each at DT = I and (where the construction survives it) at a fixed DT of
    0.3 rad / 1.5 m: the homog_th selects on both sides, exact zeros, points behind / far from / almost in the camera plane,
    every return and every branch of lineSegmentOverlap, sigma2 of high pyramid levels; two cameras, one with fx != fy.
    degenerate_cases(): observed segments shorter than a pixel in both directions with dy = 0 (infinite or NaN lambdas).
(b) mixture(seed, npts, nl): synth.make_matched_records with those features overwritten at random positions.
(c) frame_from_records(rec, seed): the same records as a TrackBatch frame whose f2f match is a known permutation.
    still_rig_records(seed): a rig that stands still — every residual is rounding noise below homog_th."""
import numpy as np

import np_model
from stvo_amd import synth

HOMOG_TH = 1e-7   # src/config.cpp:83
CAM_A = synth.KITTI_CAM
CAM_B = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, b=0.110078, width=752, height=480)   # fx != fy: only fx enters the gradient
DT_FIXED = np_model.expmap_se3(np.array([0.9, -0.5, -1.1, 0.2, -0.15, 0.17]))   # |w| = 0.30 rad, |t| = 1.5 m
MIXTURE_SIZES = [(61, 7), (449, 65), (2048, 512)]


def level_sigma2(level, scale=1.2):
    return 1.0 / (scale ** float(level)) ** 2


def _empty():
    z3, z2 = np.zeros((0, 3)), np.zeros((0, 2))
    return dict(P=z3, pl_obs=z2, sigma2p=np.zeros(0), inlier_p=np.zeros(0, np.int32), sP=z3.copy(), eP=z3.copy(), le_obs=z3.copy(),
                spl=z2.copy(), epl=z2.copy(), sigma2l=np.zeros(0), inlier_l=np.zeros(0, np.int32))


def _to_prev(DT, Pc):
    """The previous-frame point whose transform by DT is Pc (to a rounding)."""
    Ti = np_model.inverse_se3(DT)
    return Ti[:3, :3] @ np.asarray(Pc, float) + Ti[:3, 3]


def _cam_point(cam, u, v, z):
    return np.array([z * (u - cam["cx"]) / cam["fx"], z * (v - cam["cy"]) / cam["fy"], z])


def _proj_ld(DT, cam, P):
    """Projection of P under DT in extended precision, rounded to double: the observation that leaves a residual of rounding size."""
    L = np.longdouble
    T = np.asarray(DT, np.float64).astype(L)
    g = T[:3, :3] @ np.asarray(P, np.float64).astype(L) + T[:3, 3]
    return np.array([L(cam["cx"]) + L(cam["fx"]) * g[0] / g[2], L(cam["cy"]) + L(cam["fy"]) * g[1] / g[2]], dtype=L)


def point_case(cam, DT, Pc, offset, sigma2=1.0, exact=False):
    rec = _empty()
    P = np.asarray(Pc, float) if exact else _to_prev(DT, Pc)
    obs = (_proj_ld(DT, cam, P) + np.asarray(offset, np.float64).astype(np.longdouble)).astype(np.float64)
    rec.update(P=P.reshape(1, 3), pl_obs=obs.reshape(1, 2), sigma2p=np.array([sigma2]), inlier_p=np.ones(1, np.int32))
    return rec


def line_case(cam, DT, s_px, t_px, zs, ze, so, eo, le_noise=(0.4, -0.3, 0.2, 0.5), sigma2=1.0, le=None, sP=None, eP=None):
    """A segment whose end points project to s_px / t_px at depths zs / ze under DT, observed in the previous frame as (so, eo) and in
    the current one as the line through the noisy end points (or `le`)."""
    rec = _empty()
    sP = _to_prev(DT, _cam_point(cam, s_px[0], s_px[1], zs)) if sP is None else np.asarray(sP, float)
    eP = _to_prev(DT, _cam_point(cam, t_px[0], t_px[1], ze)) if eP is None else np.asarray(eP, float)
    if le is None:
        n = np.asarray(le_noise, float)
        le = synth.line_eq(np.array([[s_px[0] + n[0], s_px[1] + n[1]]]), np.array([[t_px[0] + n[2], t_px[1] + n[3]]]))[0]
    rec.update(sP=sP.reshape(1, 3), eP=eP.reshape(1, 3), le_obs=np.asarray(le, float).reshape(1, 3), spl=np.asarray(so, float).reshape(1, 2),
               epl=np.asarray(eo, float).reshape(1, 2), sigma2l=np.array([sigma2]), inlier_l=np.ones(1, np.int32))
    return rec


def single_cases():
    """[(name, cam, DT, rec)].  The camera alternates by row: every third row uses CAM_B."""
    out = []
    row = [0]

    def cam_of():
        row[0] += 1
        return CAM_B if row[0] % 3 == 0 else CAM_A

    def both(name, build, dts=("I", "T")):
        cam = cam_of()
        for tag in dts:
            DT = np.eye(4) if tag == "I" else DT_FIXED
            out.append((f"{name}@{tag}", cam, DT, build(cam, DT)))

    # ---- points
    def zero_point(cam, DT):
        rec = _empty()
        rec.update(P=np.array([[0.0, 0.0, 12.5]]), pl_obs=np.array([[cam["cx"], cam["cy"]]]), sigma2p=np.ones(1), inlier_p=np.ones(1, np.int32))
        return rec
    both("pt-zero-residual", zero_point, dts=("I",))
    both("pt-e-below-th", lambda cam, DT: point_case(cam, DT, _cam_point(cam, 600.0, 200.0, 17.0), (0.6e-7, 0.0)))
    both("pt-e-above-th", lambda cam, DT: point_case(cam, DT, _cam_point(cam, 600.0, 200.0, 17.0), (0.0, 1.6e-7)))
    both("pt-gz2-below-th", lambda cam, DT: point_case(cam, DT, _cam_point(cam, 300.0, 100.0, 2e-4), (0.7, -0.4)))
    both("pt-gz2-above-th", lambda cam, DT: point_case(cam, DT, _cam_point(cam, 300.0, 100.0, 4e-4), (0.7, -0.4)))
    both("pt-gz2-below-th-neg", lambda cam, DT: point_case(cam, DT, _cam_point(cam, 500.0, 300.0, -2e-4), (-0.3, 0.9)))
    both("pt-behind", lambda cam, DT: point_case(cam, DT, _cam_point(cam, 420.0, 150.0, -9.0), (1.1, 0.6)))
    both("pt-far", lambda cam, DT: point_case(cam, DT, _cam_point(cam, 700.0, 90.0, 1e5), (0.2, -0.8)))
    both("pt-residual-1e4", lambda cam, DT: point_case(cam, DT, _cam_point(cam, 250.0, 220.0, 30.0), (1e4, -3e3)))
    both("pt-sigma2-level7", lambda cam, DT: point_case(cam, DT, _cam_point(cam, 333.3, 111.1, 8.0), (2.5, 1.5), sigma2=level_sigma2(7)))

    # ---- lines: every return of the lambda cases, in the general branch.  With d = t - s the observed segment is
    # (s + alpha d + e, s + beta d + e), e a small offset across d, so lambda_s ~ -alpha / (beta - alpha), lambda_e ~ (1 - alpha) / (beta - alpha)
    s_px, t_px = np.array([310.0, 95.0]), np.array([470.0, 215.0])
    d = t_px - s_px
    across = np.array([-d[1], d[0]]) / np.linalg.norm(d) * 1.7

    def lam(alpha, beta, **kw):
        return lambda cam, DT: line_case(cam, DT, s_px, t_px, 14.0, 19.0, s_px + alpha * d + across, s_px + beta * d + across, **kw)
    both("ln-covers", lam(0.25, 0.75))
    both("ln-inside", lam(-0.5, 1.5))
    both("ln-disjoint-low", lam(1.5, 2.5))
    both("ln-disjoint-high", lam(-2.0, -1.0))
    both("ln-partial-low", lam(0.5, 1.5))
    both("ln-partial-high", lam(-0.5, 0.5))
    both("ln-reversed", lam(1.5, 0.5))
    both("ln-sigma2-level4", lam(-0.25, 0.9, sigma2=level_sigma2(4)))
    # the 1 px thresholds of the observed segment
    both("ln-obs-dx-0", lambda cam, DT: line_case(cam, DT, (400.0, 80.0), (403.0, 260.0), 9.0, 11.0, (401.0, 60.0), (401.0, 200.0)))
    both("ln-obs-dx-0.999", lambda cam, DT: line_case(cam, DT, (400.0, 80.0), (403.0, 260.0), 9.0, 11.0, (401.0, 120.0), (401.999, 300.0)))
    both("ln-obs-dx-1.0", lambda cam, DT: line_case(cam, DT, (400.0, 80.0), (403.0, 260.0), 9.0, 11.0, (401.0, 120.0), (402.0, 300.0)))
    both("ln-obs-dy-0.999", lambda cam, DT: line_case(cam, DT, (150.0, 140.0), (420.0, 143.0), 25.0, 21.0, (100.0, 141.0), (330.0, 141.999)))
    both("ln-obs-dy-0.999-reversed", lambda cam, DT: line_case(cam, DT, (150.0, 140.0), (420.0, 143.0), 25.0, 21.0, (380.0, 141.999), (200.0, 141.0)))

    def zero_line(cam, DT):
        return line_case(cam, DT, None, None, None, None, (cam["cx"] - 20.0, cam["cy"] + 2.0), (cam["cx"] + 90.0, cam["cy"] - 6.0),
                         le=(0.0, 1.0, -cam["cy"]), sP=(0.0, 0.0, 6.0), eP=(1.25, 0.0, 6.0))
    both("ln-zero-residual", zero_line, dts=("I",))
    both("ln-both-behind", lambda cam, DT: line_case(cam, DT, s_px, t_px, -7.0, -12.0, s_px + 0.1 * d, s_px + 1.2 * d))
    both("ln-straddles", lambda cam, DT: line_case(cam, DT, s_px, t_px, 5.0, -3.0, s_px - 0.3 * d, s_px + 0.6 * d))
    both("ln-end-in-camera-plane", lambda cam, DT: line_case(cam, DT, s_px, t_px, 2.5e-4, 6.0, s_px - 0.3 * d, s_px + 0.6 * d))
    return out


def degenerate_cases():
    """Observed segments shorter than 1 px in both directions with dy = 0: lineSegmentOverlap divides by zero.  Compared device against
    oracle only (one rounding decides 0 / 0)."""
    out = []
    for tag, DT in (("I", np.eye(4)), ("T", DT_FIXED)):
        out.append((f"ln-short-same-side@{tag}", CAM_A, DT, line_case(CAM_A, DT, (400.0, 80.0), (403.0, 260.0), 9.0, 11.0, (401.0, 60.0), (401.3, 60.0))))
        out.append((f"ln-short-straddled@{tag}", CAM_B, DT, line_case(CAM_B, DT, (400.0, 80.0), (403.0, 260.0), 9.0, 11.0, (401.7, 170.0), (401.0, 170.0))))
    cam = CAM_A   # the projections sit exactly on the observed row: 0 / 0 for both end points
    out.append(("ln-short-on-the-row@I", cam, np.eye(4),
                line_case(cam, np.eye(4), None, None, None, None, (cam["cx"] - 0.25, cam["cy"]), (cam["cx"] + 0.5, cam["cy"]),
                          le=(0.6, 0.8, -(0.6 * cam["cx"] + 0.8 * cam["cy"]) + 0.3), sP=(0.0, 0.0, 6.0), eP=(1.25, 0.0, 6.0))))
    return out


def mixture(seed, npts, nl, cam=CAM_A):
    """make_matched_records with edge features written over random positions (so they land on every lane, on both components of the
    two-record form and on the weight-0 duplicate); rec["T_true"] is the motion the benign rest was generated with."""
    rec = synth.make_matched_records(seed, n_pts=npts, n_lines=nl, cam=cam, octave_probs=[.5, .25, .15, .1])
    rng = np.random.default_rng(seed + 90001)
    T = rec["T_true"]
    P, obs, s2 = rec["P"], rec["pl_obs"], rec["sigma2p"]
    order = rng.permutation(npts)
    cnt = lambda frac: max(1, int(round(frac * npts)))
    k = 0

    def take(frac):
        nonlocal k
        idx = order[k:k + cnt(frac)]
        k += len(idx)
        return idx
    idx = take(0.10)   # the exact projection under T_true: |e| is rounding noise at DT = T_true
    obs[idx] = synth.project(cam, P[idx] @ T[:3, :3].T + T[:3, 3])
    idx = take(0.02)   # almost in the camera plane at DT = I, either side of gz^2 = homog_th, either sign
    z = rng.uniform(2e-4, 4e-4, len(idx)) * rng.choice([-1.0, 1.0], len(idx))
    P[idx] *= (z / P[idx, 2])[:, None]
    # (their gradient is fx / |gz| ~ 2e6, 1e5 times a regular point's, so that a handful of them with a residual of a pixel would own H
    # and hold Gauss-Newton at DT = I, where no other feature is tested; observed 1e5 px away their Cauchy weight is ~1e-10 and their
    # share of H that of a regular point)
    a = rng.uniform(0.0, 2.0 * np.pi, len(idx))
    obs[idx] += rng.uniform(0.5e5, 2e5, len(idx))[:, None] * np.stack([np.cos(a), np.sin(a)], 1)
    idx = take(0.02)   # behind the camera
    P[idx] = -P[idx]
    idx = take(0.02)   # very far
    P[idx] = 1e4 * P[idx]
    idx = take(0.12)
    s2[idx] = level_sigma2(7)
    if nl:
        rec["sigma2l"][:] = [level_sigma2(v) for v in rng.integers(0, 4, nl)]
        lorder = rng.permutation(nl)
        fifth = max(1, nl // 5)
        a, b, c = lorder[:fifth], lorder[fifth:2 * fifth], lorder[2 * fifth:3 * fifth]
        rec["epl"][a, 0] = rec["spl"][a, 0] + rng.uniform(-0.999, 0.999, len(a))
        rec["epl"][b, 1] = rec["spl"][b, 1] + rng.uniform(-0.999, 0.999, len(b))
        sh = rng.uniform(-200.0, 200.0, (len(c), 2))
        rec["spl"][c] += sh
        rec["epl"][c] += sh
    return rec


def mixtures():
    return [(f"mix-{npts}-{nl}", mixture(7000 + npts, npts, nl)) for npts, nl in MIXTURE_SIZES]


def frame_from_records(rec, seed):
    """A TrackBatch frame (the keys of synth.make_f2f_points_lines) whose f2f match reproduces `rec`: unique random descriptors in the
    previous frame, the same rows permuted in the current one (distance 0 against ~128 for every other row: ratio and mutual checks
    pass), the records carried over unchanged.  The matched records come out in the order of `rec`."""
    rng = np.random.default_rng(seed)

    def unique_desc(n):
        while True:
            dsc = synth.random_desc(rng, n)
            if len(np.unique(dsc, axis=0)) == n:
                return dsc
    n, nl = len(rec["sigma2p"]), len(rec["sigma2l"])
    pd, ld = unique_desc(n), unique_desc(max(nl, 1))[:nl]
    perm, lperm = rng.permutation(n), rng.permutation(nl)   # current row j holds previous row perm[j]
    return dict(prev_desc=pd, prev_P=np.ascontiguousarray(rec["P"]), prev_sigma2=np.ascontiguousarray(rec["sigma2p"]),
                curr_desc=np.ascontiguousarray(pd[perm]), curr_pl=np.ascontiguousarray(rec["pl_obs"][perm]),
                prev_ldesc=ld, prev_sP=np.ascontiguousarray(rec["sP"]), prev_eP=np.ascontiguousarray(rec["eP"]),
                prev_spl=np.ascontiguousarray(rec["spl"]), prev_epl=np.ascontiguousarray(rec["epl"]),
                prev_sigma2l=np.ascontiguousarray(rec["sigma2l"]), curr_le=np.ascontiguousarray(rec["le_obs"][lperm]),
                curr_ldesc=np.ascontiguousarray(ld[lperm]), perm=perm, lperm=lperm, T_true=rec.get("T_true"), cam=rec.get("cam"))


def still_rig_records(seed, n=400, cam=CAM_A):
    """A rig that does not move: every stereo point is observed at its own float (u, v), P = backProjection(u, v, disp)
    (src/stereoFrame.cpp:152-167).  Each residual is the rounding of one back-projection and one projection, far below homog_th."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(19, cam["width"] - 19, n).astype(np.float32).astype(np.float64)
    v = rng.uniform(19, cam["height"] - 19, n).astype(np.float32).astype(np.float64)
    disp = (cam["b"] * cam["fx"] / rng.uniform(4.0, 80.0, n)).astype(np.float32).astype(np.float64)
    rec = _empty()
    rec.update(P=np.ascontiguousarray(synth.back_project(cam, u, v, disp)), pl_obs=np.ascontiguousarray(np.stack([u, v], 1)),
               sigma2p=np.ones(n), inlier_p=np.ones(n, np.int32))
    return rec


# ------------------------------------------------------------------------------------------------
# every case evaluated once by the extended statement and by the oracle; shared by the host and the GPU tests
# ------------------------------------------------------------------------------------------------
FLOOR = {0: 1e-10, 1: 1e-6}   # tests/test_gpu_pose.py::test_normal_eq_vs_oracle; tests/fuzz_entry_points.py (float-truncated MAD)
FACTOR = 16.0
_EVAL = None


def all_cases():
    """[(name, cam, DT, rec)]: the single-feature rows, then every mixture at DT = I and at its T_true."""
    out = list(single_cases())
    for name, rec in mixtures():
        out.append((name + "@I", CAM_A, np.eye(4), rec))
        out.append((name + "@T", CAM_A, rec["T_true"], rec))
    return out


def evaluations(oracle):
    """{(name, robust): dict(cam, DT, rec, ext = (H, g, e, n, s_p, s_l) extended, orc = (H, g, e, n) oracle, dev_orc = the oracle's
    deviation from the extended statement (H, g, e))}, computed once per process and never modified."""
    global _EVAL
    if _EVAL is None:
        import np_pose_terms
        from stvo_amd.ctypes_types import opt_params
        prm = opt_params("kitti")
        assert prm.homog_th == HOMOG_TH
        ev = {}
        for name, cam, DT, rec in all_cases():
            for robust in (0, 1):
                ext = np_pose_terms.evaluate(DT, cam, HOMOG_TH, rec, bool(robust))
                orc = oracle.optimize_functions(DT, cam, prm, rec, robust)
                ev[(name, robust)] = dict(cam=cam, DT=DT, rec=rec, ext=ext, orc=orc,
                                          dev_orc=np_pose_terms.deviation(orc[0], orc[1], orc[2], ext[0], ext[1], ext[2]))
        _EVAL = ev
    return _EVAL


def bound(ev, robust):
    """What a device (or fast-form) evaluation may deviate from the extended statement: the floor, or 16 x the oracle's own deviation
    in the same case where the case itself amplifies rounding (a residual that cancels, a point almost in the camera plane)."""
    return [max(FLOOR[robust], FACTOR * d) for d in ev["dev_orc"]]


def still_rig_sequences(n_streams):
    """One synth.make_stereo_sequence frame (points and key-lines) per stream, repeated three times."""
    out = []
    for b in range(n_streams):
        fr = synth.make_stereo_sequence(4200 + b, n_frames=1, n_pts=400 + 60 * b, n_lines=40 + 5 * b, cam=synth.KITTI_CAM)[0]
        out.append([fr, fr, fr])
    return out
