"""The flow of optimizePose in extended precision, with a trace — TEST INFRASTRUCTURE ONLY.

The judge of the control flow of csrc/pose_block.h: gaussNewtonOptimization, gaussNewtonOptimizationRobust,
levenbergMarquardtOptimization, isGoodSolution and optimizePose, written from src/stereoFrameHandler.cpp:292-547 of the reference
(not from the oracle, not from the kernel) in numpy.longdouble.  Every evaluation is np_pose_terms.evaluate; the 6 x 6 solve, the
inverse and log|det| are one Gauss-Jordan elimination with partial pivoting written here, the eigenvalues a cyclic Jacobi iteration
written here, exp / log of se(3) those of np_trajectory.py.  removeOutliers is outlier_cut_cases.expected (the statement by counting)
on residual norms computed here in extended precision and rounded to double, as the reference's own doubles are.  The pose is held
as the reference holds it, a Matrix4d: every step is computed in extended precision and rounded to double once.

optimize_pose returns the fields of stvo_pose_result and a TRACE:
  trace["stages"]    [dict(stage 0 / 1 / 2 = first optimisation / refinement / robust fallback, alg 0 / 1 / 2 = GN / robust GN / LM,
                     rule = what ended the loop: "max_iters", "min_error", "err_change", "step", "err_up", "lad",
                     evals = [dict(err, err_prev, nt = |inc_t|, nr = |inc_r|, n6 = |inc|_6, lad = log|det H| of the matrix that was
                     solved, lam_before, lam_after, stepped)], H = the matrix the covariance was taken from, DT = the pose left)]
  trace["verdicts"]  [dict(site "stage1" / "commit", err, eig [6], norm_inf, good, regime)] with the regime of the covariance:
                     "A" certified (||cov||_inf <= 1 and positive definite), "B" lambda_max <= 1 < ||cov||_inf, "C" lambda_max > 1
  trace["cmps"]      [(label, a, b, fired, margin)] — EVERY comparison executed, fired or not, with its relative margin
                     |a - b| / max(|a|, |b|); trace["margin"] is the smallest.
Conventions of the margins:
  * isGoodSolution's four comparisons are all recorded, whatever the short-circuit order (the kernel tests err first);
  * log|det H| < 0 is |det H| < 1: its margin is that of (|det H|, 1), since any margin relative to 0 is 1;
  * ||cov||_inf <= 1, the kernel's certificate, is recorded with the verdict although the reference does not compare it;
  * a comparison whose operands are the same number on every deterministic implementation carries no margin (inf): LM's
    err against err_prev after an evaluation without a step (the same pose evaluated twice), the eigenvalues of the identity that
    robust GN leaves after log|det H| < 0;
  * the cut of removeOutliers contributes its closest |r - mean| against inlier_k sigma and its closest r against the 2 sigma gate."""
import numpy as np

import np_pose_terms
import np_trajectory as npt
import outlier_cut_cases as occ

LD = np.longdouble
assert np_pose_terms.BACKEND == "longdouble"
INF = float("inf")
ERR_PREV0 = 999999999.9
RULES = ("max_iters", "min_error", "err_change", "step", "err_up", "lad")


# ---- 6 x 6 algebra in extended precision -------------------------------------------------------------------------------------------
def gauss_jordan(A, B):
    """X with A X = B, log|det A| and sign(det A): elimination with partial pivoting"""
    A = np.array(A, dtype=LD)
    B = np.array(B, dtype=LD).reshape(len(A), -1)
    n = len(A)
    lad, sign = LD(0), 1
    with np.errstate(all="ignore"):
        for k in range(n):
            p = k + int(np.argmax(np.abs(A[k:, k])))
            if p != k:
                A[[k, p]] = A[[p, k]]
                B[[k, p]] = B[[p, k]]
                sign = -sign
            piv = A[k, k]
            lad = lad + np.log(np.abs(piv))
            if piv < 0:
                sign = -sign
            for i in range(n):
                if i != k:
                    f = A[i, k] / piv
                    A[i] = A[i] - f * A[k]
                    B[i] = B[i] - f * B[k]
        X = B / np.diag(A)[:, None]
    return X, lad, sign


def solve(H, g):
    X, lad, _ = gauss_jordan(H, np.asarray(g, dtype=LD).reshape(6, 1))
    return X[:, 0], lad


def inverse(H):
    return gauss_jordan(H, np.eye(6, dtype=LD))[0]


def lower_symmetric(C):
    """the self-adjoint view SelfAdjointEigenSolver takes (:294): the lower triangle"""
    C = np.asarray(C, dtype=LD)
    L = np.tril(C)
    return L + L.T - np.diag(np.diag(C))


def eigenvalues(S):
    """ascending eigenvalues of a symmetric matrix: cyclic Jacobi rotations"""
    A = np.array(S, dtype=LD)
    n = len(A)
    for _ in range(60):
        off = sum(A[i, j] * A[i, j] for i in range(n) for j in range(i))
        if off == 0 or off < LD(1e-70) * sum(A[i, i] * A[i, i] for i in range(n)):
            break
        for p in range(n):
            for q in range(p + 1, n):
                if A[p, q] == 0:
                    continue
                with np.errstate(over="ignore"):   # an entry that is almost gone: theta^2 = inf, t = 0, no rotation
                    theta = (A[q, q] - A[p, p]) / (2 * A[p, q])
                    t = (LD(1) if theta >= 0 else LD(-1)) / (abs(theta) + np.sqrt(theta * theta + 1))
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                R = np.eye(n, dtype=LD)
                R[p, p] = R[q, q] = c
                R[p, q], R[q, p] = s, -s
                A = R.T @ A @ R
    return np.sort(np.diag(A))


def step_pose(DT, inc):
    """DT * inverse_se3(expmap_se3(inc)) (:419), rounded to the Matrix4d the reference keeps"""
    T = np.asarray(DT, np.float64).astype(LD) @ npt.inverse_se3(npt.expmap_se3(inc))
    return T.astype(np.float64)


def _norm(v):
    v = np.asarray(v, dtype=LD)
    return np.sqrt(v @ v)


# ---- the trace --------------------------------------------------------------------------------------------------------------------
class Trace(dict):
    def __init__(self):
        super().__init__(stages=[], verdicts=[], cmps=[], cut=None)

    def cmp(self, label, a, b, op, exact=False, scale=None):
        """a op b, recorded; scale: (a', b') whose relative distance is the margin instead of (a, b)"""
        fired = bool({"<": a < b, ">": a > b, "<=": a <= b}[op])
        ma, mb = (a, b) if scale is None else scale
        den = max(abs(ma), abs(mb))
        if exact:
            m = INF
        elif den > 0 and np.isfinite(float(den)):
            m = float(abs(ma - mb) / den)
        else:   # 0 against 0, or something that is not a number: no margin at all
            m = 0.0
        self["cmps"].append((label, float(a), float(b), fired, m))
        return fired

    @property
    def margin(self):
        return min([c[4] for c in self["cmps"]] + [INF])


# ---- the three optimisers (:394-547) ---------------------------------------------------------------------------------------------
def _with_flags(rec, ip, il):
    r = dict(rec)
    r["inlier_p"], r["inlier_l"] = np.asarray(ip, np.int32), np.asarray(il, np.int32)
    return r


def _evaluate(DT, cam, prm, rec, robust):
    H, g, e, n, _, _ = np_pose_terms.evaluate(DT, cam, prm["homog_th"], rec, robust)
    return np.asarray(H, dtype=LD), np.asarray(g, dtype=LD), LD(e)


def gauss_newton(tr, stage, DT, cam, prm, rec, max_iters):
    """:394-431 -> DT, cov (None where the reference returns without touching it), err"""
    st = dict(stage=stage, alg=0, evals=[], rule="max_iters")
    tr["stages"].append(st)
    err_prev, H, err = LD(ERR_PREV0), None, None
    tag = f"s{stage}.gn"
    for it in range(max_iters):
        H, g, err = _evaluate(DT, cam, prm, rec, False)
        ev = dict(err=err, err_prev=err_prev, nt=None, nr=None, n6=None, lad=None, lam_before=None, lam_after=None, stepped=False)
        st["evals"].append(ev)
        if tr.cmp(f"{tag}[{it}] err > err_prev", err, err_prev, ">"):
            if it > 0:
                st["rule"] = "err_up"
                break
            st.update(rule="err_up_first", H=H, DT=DT)
            return DT, None, LD(-1)
        a = tr.cmp(f"{tag}[{it}] err < min_error", err, LD(prm["min_error"]), "<")
        b = tr.cmp(f"{tag}[{it}] |err - err_prev| < min_error_change", abs(err - err_prev), LD(prm["min_error_change"]), "<")
        if a or b:
            st["rule"] = "min_error" if a else "err_change"
            break
        inc, ev["lad"] = solve(H, g)
        DT = step_pose(DT, inc)
        ev.update(nt=_norm(inc[:3]), nr=_norm(inc[3:]), n6=_norm(inc), stepped=True)
        a = tr.cmp(f"{tag}[{it}] |inc_t| < min_error_change", ev["nt"], LD(prm["min_error_change"]), "<")
        b = tr.cmp(f"{tag}[{it}] |inc_r| < min_error_change", ev["nr"], LD(prm["min_error_change"]), "<")
        if a and b:
            st["rule"] = "step"
            break
        err_prev = err
    st.update(H=H, DT=DT)
    return DT, inverse(H), err


def gauss_newton_robust(tr, stage, DT, cam, prm, rec, max_iters):
    """:433-480"""
    st = dict(stage=stage, alg=1, evals=[], rule="max_iters")
    tr["stages"].append(st)
    DT_in, err_prev, H, err, good = DT, LD(ERR_PREV0), None, None, True
    tag = f"s{stage}.gnr"
    for it in range(max_iters):
        H, g, err = _evaluate(DT, cam, prm, rec, True)
        ev = dict(err=err, err_prev=err_prev, nt=None, nr=None, n6=None, lad=None, lam_before=None, lam_after=None, stepped=False)
        st["evals"].append(ev)
        a = tr.cmp(f"{tag}[{it}] |err - err_prev| < min_error_change", abs(err - err_prev), LD(prm["min_error_change"]), "<")
        b = tr.cmp(f"{tag}[{it}] err < min_error", err, LD(prm["min_error"]), "<")
        if a or b:
            st["rule"] = "err_change" if a else "min_error"
            break
        inc, ev["lad"] = solve(H, g)
        if tr.cmp(f"{tag}[{it}] log|det H| < 0", ev["lad"], LD(0), "<", scale=(np.exp(ev["lad"]), LD(1))):
            good = False
            st["rule"] = "lad"
            break
        DT = step_pose(DT, inc)
        ev.update(nt=_norm(inc[:3]), nr=_norm(inc[3:]), n6=_norm(inc), stepped=True)
        if tr.cmp(f"{tag}[{it}] |inc| < min_error_change", ev["n6"], LD(prm["min_error_change"]), "<"):
            st["rule"] = "step"
            break
        err_prev = err
    if good:
        st.update(H=H, DT=DT)
        return DT, inverse(H), err
    st.update(H=H, DT=DT_in)
    return DT_in, np.eye(6, dtype=LD), LD(-1)


def levenberg_marquardt(tr, stage, DT, cam, prm, rec, max_iters):
    """:482-547"""
    st = dict(stage=stage, alg=2, evals=[], rule="max_iters")
    tr["stages"].append(st)
    tag = f"s{stage}.lm"
    H, g, err = _evaluate(DT, cam, prm, rec, False)
    hmax = LD(0)
    for i in range(6):
        if H[i, i] > hmax or H[i, i] < -hmax:
            hmax = abs(H[i, i])
    lam = LD(0.000000001) * hmax
    st["H_undamped"] = H
    H = H + lam * np.eye(6, dtype=LD)
    inc, lad = solve(H, g)
    DT = step_pose(DT, inc)
    st["evals"].append(dict(err=err, err_prev=LD(ERR_PREV0), nt=_norm(inc[:3]), nr=_norm(inc[3:]), n6=_norm(inc), lad=lad, lam_before=lam,
                            lam_after=lam, stepped=True))
    err_prev, same_pose = err, False
    for it in range(1, max_iters):
        H, g, err = _evaluate(DT, cam, prm, rec, False)
        ev = dict(err=err, err_prev=err_prev, nt=None, nr=None, n6=None, lad=None, lam_before=lam, lam_after=lam, stepped=False)
        st["evals"].append(ev)
        if same_pose:
            assert err == err_prev
        a = tr.cmp(f"{tag}[{it}] |err - err_prev| < min_error_change", abs(err - err_prev), LD(prm["min_error_change"]), "<", exact=same_pose)
        b = tr.cmp(f"{tag}[{it}] err < min_error", err, LD(prm["min_error"]), "<")
        if a or b:
            st["rule"] = "err_change" if a else "min_error"
            break
        st["H_undamped"] = H
        H = H + lam * np.eye(6, dtype=LD)
        inc, ev["lad"] = solve(H, g)
        if tr.cmp(f"{tag}[{it}] err > err_prev", err, err_prev, ">", exact=same_pose):
            lam = lam / 4
            same_pose = True
        else:
            lam = lam * 4
            DT = step_pose(DT, inc)
            ev["stepped"] = True
            same_pose = False
        ev.update(nt=_norm(inc[:3]), nr=_norm(inc[3:]), n6=_norm(inc), lam_after=lam)
        a = tr.cmp(f"{tag}[{it}] |inc_t| < min_error_change", ev["nt"], LD(prm["min_error_change"]), "<")
        b = tr.cmp(f"{tag}[{it}] |inc_r| < min_error_change", ev["nr"], LD(prm["min_error_change"]), "<")
        if a and b:
            st["rule"] = "step"
            break
        err_prev = err
    st.update(H=H, DT=DT)
    return DT, inverse(H), err


RUN = {0: gauss_newton, 1: gauss_newton_robust, 2: levenberg_marquardt}


# ---- isGoodSolution (:292-305) ---------------------------------------------------------------------------------------------------
def is_good_solution(tr, site, DT, cov, err):
    S = lower_symmetric(cov)
    identity = bool(np.array_equal(S, np.eye(6, dtype=LD)))
    eig = eigenvalues(S)
    norm_inf = max(np.sum(np.abs(S), axis=1))
    bad = [tr.cmp(f"{site} eig(0) < 0", eig[0], LD(0), "<", exact=identity),
           tr.cmp(f"{site} eig(5) > 1", eig[5], LD(1), ">", exact=identity),
           tr.cmp(f"{site} err < 0", err, LD(0), "<"),
           tr.cmp(f"{site} err > 1", err, LD(1), ">")]
    certified = (not tr.cmp(f"{site} ||cov||_inf > 1", norm_inf, LD(1), ">", exact=identity)) and eig[0] > 0
    finite = bool(np.all(np.isfinite(np.asarray(DT, np.float64))))
    good = not any(bad) and finite
    regime = "A" if certified else ("C" if eig[5] > 1 else "B")
    tr["verdicts"].append(dict(site=site, err=err, eig=eig, norm_inf=norm_inf, good=good, regime=regime, identity_cov=identity))
    return good


# ---- removeOutliers (:988-1067) ----------------------------------------------------------------------------------------------------
def residual_norms(DT, cam, rec):
    """the weighted residual norms of ALL matches, computed in extended precision and rounded to double"""
    T = np_pose_terms._conv(np.asarray(DT, np.float64).reshape(4, 4))
    c = {k: LD(float(cam[k])) for k in ("fx", "fy", "cx", "cy")}
    rp, rl = [], []
    with np.errstate(all="ignore"):
        for P, o, s2 in zip(rec["P"], rec["pl_obs"], rec["sigma2p"]):
            _, uv = np_pose_terms._project(T, c, [LD(float(v)) for v in P])
            dx, dy = uv[0] - LD(float(o[0])), uv[1] - LD(float(o[1]))
            rp.append(float(np.sqrt(dx * dx + dy * dy) * np.sqrt(LD(float(s2)))))
        for sP, eP, le, s2 in zip(rec["sP"], rec["eP"], rec["le_obs"], rec["sigma2l"]):
            _, s = np_pose_terms._project(T, c, [LD(float(v)) for v in sP])
            _, t = np_pose_terms._project(T, c, [LD(float(v)) for v in eP])
            l = [LD(float(v)) for v in le]
            ds, de = l[0] * s[0] + l[1] * s[1] + l[2], l[0] * t[0] + l[1] * t[1] + l[2]
            rl.append(float(np.sqrt(ds * ds + de * de) * np.sqrt(LD(float(s2)))))
    return np.array(rp, np.float64), np.array(rl, np.float64)


def remove_outliers(tr, DT, cam, prm, rec, ip, il):
    rp, rl = residual_norms(DT, cam, rec)
    info = {}
    for side, r, inl, on in (("p", rp, ip, prm["has_points"]), ("l", rl, il, prm["has_lines"])):
        if not on:
            info[side] = (np.asarray(inl, bool).copy(), None)
            continue
        kept, st = occ.expected(r, np.asarray(inl, bool), prm["inlier_k"])
        info[side] = (kept, st)
        if st.n:
            for i in np.nonzero(np.asarray(inl, bool))[0]:
                tr.cmp(f"cut {side}[{i}] |r - mean| > k sigma", LD(abs(r[i] - st.mean)), LD(st.th), ">")
            for i in range(st.n):
                tr.cmp(f"cut {side}[{i}] r < 2 sigma", LD(r[i]), LD(2.0 * st.sigma), "<")
    tr["cut"] = dict(rp=rp, rl=rl, stats_p=info["p"][1], stats_l=info["l"][1])
    return info["p"][0], info["l"][0]


# ---- optimizePose (:307-392) ---------------------------------------------------------------------------------------------------------
def optimize_pose(init_T, cam, prm, rec):
    """prm: np_model.prm_dict(OptParams).  -> (result: the fields of stvo_pose_result, extended where they are computed; trace)"""
    tr = Trace()
    ip, il = np.asarray(rec["inlier_p"]) > 0, np.asarray(rec["inlier_l"]) > 0
    DT = np.array(init_T, np.float64).reshape(4, 4)
    cov, err = None, LD(-1)
    status, path, iters = 0, 0, [0, 0]
    run = RUN[prm["mode"]]
    if int(ip.sum() + il.sum()) >= prm["min_features"]:
        DT_, cov, err = run(tr, 0, DT.copy(), cam, prm, _with_flags(rec, ip, il), prm["max_iters"])
        iters[0] = len(tr["stages"][-1]["evals"])
        assert cov is not None, "GN returned at its first evaluation: DT_cov is uninitialised in the reference"
        if is_good_solution(tr, "stage1", DT_, cov, err):
            path |= 1
            ip, il = remove_outliers(tr, DT_, cam, prm, rec, ip, il)
            if int(ip.sum() + il.sum()) >= prm["min_features"]:
                path |= 4
                DT, cov2, err = run(tr, 1, DT.copy(), cam, prm, _with_flags(rec, ip, il), prm["max_iters_ref"])
                iters[1] = len(tr["stages"][-1]["evals"])
                assert cov2 is not None
                cov = cov2
            else:
                DT, status = np.eye(4), 2
        else:
            path |= 2
            DT, cov, err = gauss_newton_robust(tr, 2, DT.copy(), cam, prm, _with_flags(rec, ip, il), prm["max_iters_ref"])
            iters[1] = len(tr["stages"][-1]["evals"])
    else:
        DT, status = np.eye(4), 1
    out = dict(T_opt=DT, err_opt=err, path=path, iters=tuple(iters), inlier_p=ip.astype(np.int32), inlier_l=il.astype(np.int32),
               n_inliers_pt=int(ip.sum()), n_inliers_ls=int(il.sum()), n_matched_pt=len(ip), n_matched_ls=len(il))
    if cov is None:   # nothing was optimised: the reference tests its uninitialised DT_cov with err = -1, which decides
        good = False
        tr["verdicts"].append(dict(site="commit", err=err, eig=None, norm_inf=None, good=False, regime=None, identity_cov=False))
    else:
        good = is_good_solution(tr, "commit", DT, cov, err)
    ident = bool(np.array_equal(DT, np.eye(4)))
    tr["identity"] = ident
    if good and not ident:
        out.update(T=npt.expmap_se3(npt.logmap_se3(npt.inverse_se3(DT.astype(LD)))), cov=np.asarray(cov, dtype=LD), err=err, status=status,
                   cov_eig=tr["verdicts"][-1]["eig"])
    else:
        out.update(T=np.eye(4, dtype=LD), cov=np.zeros((6, 6), dtype=LD), err=LD(-1), cov_eig=np.zeros(6, dtype=LD), status=status if status else 3)
    tr["margin"] = tr.margin
    return out, tr
