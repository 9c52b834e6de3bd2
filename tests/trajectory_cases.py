"""Shared inputs and expectations of the trajectory / key-frame tests (tests/test_trajectory_host.py on the CPU,
tests/test_gpu_trajectory.py on the device) — TEST INFRASTRUCTURE ONLY.

Three statements of one update meet here: the product's traj_update.h compiled for the host (traj_host_lib), the extended-precision
statement (np_trajectory) and the oracle's pieces (oracle_lib: orc_expmap / orc_logmap / orc_unccomp / orc_need_new_kf /
orc_curr_frame_is_kf).  The expectations are computed once per process and never changed by a test."""
import functools

import numpy as np

import np_model
import np_trajectory as npt
import oracle_lib
from stvo_amd import capi
from stvo_amd.ctypes_types import POSE_RESULT_DTYPE, TRAJ_RECORD_DTYPE, TRAJ_STATE_DTYPE

SEED = 5          # chosen on the CPU: no frame of the sequence lies within GUARD of a threshold (test_decision_guard)
N_FRAMES = 60
GUARD = 1e-9      # relative distance from a threshold below which a decision would not be compared
INT_FIELDS = ("prev_f_iskf", "N_prevKF_currF", "n_frames", "n_keyframes")
FAR = 1e9         # a threshold out of reach


def prm_dict(p):
    return dict(keyframes=int(p.keyframes), min_entropy_ratio=p.min_entropy_ratio, max_kf_t_dist=p.max_kf_t_dist, max_kf_r_dist=p.max_kf_r_dist)


def result(T=None, cov=None, status=0):
    """One stvo_pose_result as the pose kernel leaves it: a failed frame carries T = I, cov = 0, err = -1 (src/stereoFrameHandler.cpp:382-391)."""
    r = np.zeros((), dtype=POSE_RESULT_DTYPE)
    if status == 0:
        r["T"], r["cov"], r["err"] = np.asarray(T).reshape(-1), np.asarray(cov).reshape(-1), 0.1
    else:
        r["T"], r["err"] = np.eye(4).reshape(-1), -1.0
    r["status"] = status
    return r


def random_cov(rng):
    """inverse(J^T J) of 20 features: determinant near 1e-30, as test_keyframe_decision draws it."""
    J = rng.normal(size=(20, 6)) * np.array([30, 30, 30, 300, 300, 300.0]) * rng.uniform(0.5, 3)
    return np.linalg.inv(J.T @ J)


def sequence(seed=SEED, n=N_FRAMES):
    """n pose results of one stream: forward motion of 0.3 .. 1.2 per frame with small rotations, every 17th frame failed."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=POSE_RESULT_DTYPE)
    for f in range(n):
        inc = np.concatenate([rng.normal(0, 0.02, 2), [-rng.uniform(0.3, 1.2)], rng.normal(0, 0.01, 3)])
        D, Cv = np_model.expmap_se3(inc), random_cov(rng)
        out[f] = result(D, Cv) if f % 17 != 9 else result(status=3)
    return out


# ---- records <-> dicts
def state_to_dict(rec):
    d = {k: (int(rec[k]) if k in INT_FIELDS else np.array(rec[k], dtype=np.float64)) for k in TRAJ_STATE_DTYPE.names}
    d["entropy_first_prevKF"] = float(rec["entropy_first_prevKF"])
    for k, n in (("Tfw", 4), ("T_prevKF", 4), ("Tfw_cov", 6), ("cov_prevKF_currF", 6)):
        d[k] = d[k].reshape(n, n)
    return d


def record_to_dict(rec):
    return dict(Tfw=np.array(rec["Tfw"]).reshape(4, 4), Tfw_cov=np.array(rec["Tfw_cov"]).reshape(6, 6), entropy_ratio=float(rec["entropy_ratio"]),
                t=float(rec["t"]), r=float(rec["r"]), new_kf=int(rec["new_kf"]), frame=int(rec["frame"]))


# ---- the oracle's pieces as one update
def oracle_update(orc, s, res, prm):
    """The update of tests/pipeline_ref.py:run_sequence (Tfw / Tfw_cov through orc_logmap / orc_expmap / orc_unccomp, the decision through
    orc_need_new_kf, the reset through orc_curr_frame_is_kf) from the double state `s`.  t and r are the oracle's logmap of the same
    product; the entropy ratio is formed from the oracle's accumulated covariance and first entropy (it exports no determinant: the
    double LU of np_trajectory.det stands in)."""
    T, cov = np.array(res["T"]).reshape(4, 4), np.array(res["cov"]).reshape(6, 6)
    n = dict(s)
    if int(res["status"]) == 0:
        n["Tfw"] = orc.expmap(orc.logmap(s["Tfw"] @ T))
        n["Tfw_cov"] = orc.unccomp(s["Tfw"], s["Tfw_cov"], cov)
    else:
        T, cov = np.eye(4), np.zeros((6, 6))
    n["n_frames"] = s["n_frames"] + 1
    rec = dict(Tfw=n["Tfw"], Tfw_cov=n["Tfw_cov"], entropy_ratio=0.0, t=0.0, r=0.0, new_kf=0, frame=n["n_frames"])
    if prm["keyframes"]:
        st = np.zeros(55)
        st[0], st[1], st[2] = s["prev_f_iskf"], s["entropy_first_prevKF"], s["N_prevKF_currF"]
        st[3:19], st[19:55] = s["T_prevKF"].reshape(-1), s["cov_prevKF_currF"].reshape(-1)
        need = orc.need_new_kf(st, n["Tfw"], T, cov, prm["min_entropy_ratio"], prm["max_kf_t_dist"], prm["max_kf_r_dist"])
        dX = orc.logmap(orc.inverse_se3(n["Tfw"]) @ s["T_prevKF"])
        c0 = 3.0 * (1.0 + np.log(2.0 * np.arccos(-1.0)))
        with np.errstate(all="ignore"):
            ratio = (c0 + 0.5 * np.log(npt.det(st[19:55].reshape(6, 6), np.float64))) / st[1]
        rec.update(t=float(np.sqrt(dX[:3] @ dX[:3])), r=float(np.sqrt(dX[3:] @ dX[3:]) * np.float32(180.0) / npt.CV_PI),
                   entropy_ratio=float(ratio), new_kf=need)
        n.update(prev_f_iskf=0, entropy_first_prevKF=float(st[1]), cov_prevKF_currF=st[19:55].reshape(6, 6).copy())
        if need:
            orc.curr_frame_is_kf(st)
            n.update(Tfw=np.eye(4), Tfw_cov=np.eye(6), T_prevKF=st[3:19].reshape(4, 4).copy(), cov_prevKF_currF=st[19:55].reshape(6, 6).copy(),
                     prev_f_iskf=int(st[0]), N_prevKF_currF=int(st[2]), n_keyframes=s["n_keyframes"] + 1)
        else:
            n["N_prevKF_currF"] = int(st[2])
    return n, rec


def deviation(got, exp):
    """Largest |got - exp| per field (exp in extended precision); fields that are not finite in the expectation must agree in kind."""
    out = {}
    for k in npt.FIELDS:
        g, e = np.asarray(got[k], dtype=npt.LD).reshape(-1), np.asarray(exp[k], dtype=npt.LD).reshape(-1)
        fin = np.isfinite(e)
        assert np.array_equal(np.isnan(g), np.isnan(e)) and np.array_equal(g[~fin & ~np.isnan(e)], e[~fin & ~np.isnan(e)]), k
        out[k] = float(np.max(np.abs(g[fin] - e[fin]))) if fin.any() else 0.0
    return out


def near_threshold(rec_ld, prm):
    """Frames whose extended-precision entropy ratio, t or r lies within GUARD (relative) of its threshold."""
    pairs = ((rec_ld["entropy_ratio"], prm["min_entropy_ratio"]), (rec_ld["t"], prm["max_kf_t_dist"]), (rec_ld["r"], prm["max_kf_r_dist"]))
    return any(np.isfinite(v) and abs(v - npt.LD(th)) <= GUARD * abs(npt.LD(th)) for v, th in pairs)


@functools.lru_cache(maxsize=None)
def stepwise(keyframes=True, n=N_FRAMES):
    """Case 1: the host function chained over the sequence; at every frame the extended-precision statement and the oracle's pieces
    run one update from the host chain's (double) state.  Returns per-frame decisions of the three, the largest deviation of the host
    function and of the oracle from the extended-precision values per field, the largest magnitude per field, the number of frames
    the guard would leave out, and the host chain's states / records."""
    import traj_host_lib
    orc = oracle_lib.load()
    p = capi.traj_params("kitti", keyframes=keyframes)
    prm = prm_dict(p)
    res = sequence(n=n)
    state = traj_host_lib.init(1)
    dec = {"host": [], "ld": [], "oracle": []}
    dev = {"host": dict.fromkeys(npt.FIELDS, 0.0), "oracle": dict.fromkeys(npt.FIELDS, 0.0)}
    mag = dict.fromkeys(npt.FIELDS, 0.0)
    guarded, states, records, ints = 0, [], [], []
    for f in range(n):
        before = state_to_dict(state[0])
        rec_h = traj_host_lib.update(res[f:f + 1], p, state)
        s_ld, r_ld, _ = npt.update(before, res[f]["T"], res[f]["cov"], int(res[f]["status"]), prm)
        s_o, r_o = oracle_update(orc, before, res[f], prm)
        exp = npt.fields_of(s_ld, r_ld)
        for name, got in (("host", npt.fields_of(state_to_dict(state[0]), record_to_dict(rec_h[0]))), ("oracle", npt.fields_of(s_o, r_o))):
            for k, v in deviation(got, exp).items():
                dev[name][k] = max(dev[name][k], v)
        for k in npt.FIELDS:
            computed = np.isfinite(exp[k]) & (exp[k] != npt.LD(npt.ENTROPY_OF_SINGULAR))   # (the literal is stored, not computed)
            mag[k] = max(mag[k], float(np.max(np.abs(exp[k][computed]), initial=0.0)))
        dec["host"].append(int(rec_h[0]["new_kf"])); dec["ld"].append(r_ld["new_kf"]); dec["oracle"].append(int(r_o["new_kf"]))
        ints.append(dict(host={k: int(state[0][k]) for k in INT_FIELDS}, ld={k: int(s_ld[k]) for k in INT_FIELDS},
                         oracle={k: int(s_o[k]) for k in INT_FIELDS}))
        guarded += bool(keyframes and near_threshold(r_ld, prm))
        states.append(state.copy()); records.append(rec_h.copy())
    return dict(prm=p, results=res, decisions=dec, deviation=dev, magnitude=mag, guarded=guarded, states=states, records=records, ints=ints)


def bounds():
    """Per field: what a device statement may deviate from the extended-precision one — eight times the oracle's own largest deviation
    in case 1 (libm against the device's sin / cos / log / acos, FMA contraction, three chained 6 x 6 products: a factor each), plus
    one ulp of the field's largest magnitude in that case."""
    c = stepwise()
    return {k: 8.0 * c["deviation"]["oracle"][k] + float(np.spacing(c["magnitude"][k])) for k in npt.FIELDS}


# ---- the triggers, each alone
def _steady(n, tz=-0.05, wy=0.0, scale=1.0, seed=11):
    """n good frames of the same increment (tz along the axis, wy about y) with one fixed covariance."""
    cov = random_cov(np.random.default_rng(seed)) * scale
    D = np_model.expmap_se3(np.array([0.0, 0.0, tz, 0.0, wy, 0.0]))
    return [result(D, cov) for _ in range(n)]


def common_params():
    """One parameter set under which every trigger sequence below still fires at its frame by its own operand alone: what one
    launch for all of them (one stream per trigger) needs."""
    return capi.traj_params("kitti", max_kf_t_dist=1.0)


def triggers():
    """[(name, params with the other thresholds out of reach, results, index of the frame that must fire, the one operand of the OR
    that is true there)].  In every case no frame before that index fires and at that index no other operand is true, under the
    case's own parameters and under common_params() (tests/test_trajectory_host.py asserts both on the extended-precision statement).
    Equal covariances k times over give det = k^6 det_1, so the entropy ratio falls as 1 - 3 ln(k) / |entropy_1| (|entropy_1| ~ 26)."""
    P = lambda **kw: capi.traj_params("kitti", **kw)
    out = []
    # a: the accumulated entropy against the first frame's (0.84 at the fourth frame), 0.05 of motion per frame
    out.append(("entropy", P(max_kf_t_dist=FAR, max_kf_r_dist=FAR), _steady(8), 3, "entropy"))
    # b, c: the geometric distances at the third frame (1.2 > 1.0; 18 > 15 degrees), where the entropy ratio is still 0.87
    out.append(("t", P(min_entropy_ratio=-FAR, max_kf_t_dist=1.0, max_kf_r_dist=FAR), _steady(4, tz=-0.4), 2, "t"))
    out.append(("r", P(min_entropy_ratio=-FAR, max_kf_t_dist=FAR, max_kf_r_dist=15.0), _steady(4, tz=-0.01, wy=np.deg2rad(6.0)), 2, "r"))
    # d: 11 frames pass, the 12th fires (covariances 1e-8 of the first frame's: the entropy stays where it was)
    out.append(("count", P(min_entropy_ratio=-FAR, max_kf_t_dist=FAR, max_kf_r_dist=FAR), _steady(1, tz=-0.01) + _steady(12, tz=-0.01, scale=1e-8), 11, "count"))
    # e: a failed frame (second after the key-frame: the first would also meet a zero determinant)
    out.append(("failed", P(min_entropy_ratio=-FAR, max_kf_t_dist=FAR, max_kf_r_dist=FAR), _steady(1) + [result(status=3)] + _steady(1), 1, "failed"))
    # f: det(DT_cov) == 0 exactly on the first frame after a key-frame (a rotation row and column of zeros, pure translation: the
    # accumulated covariance keeps them, its determinant is 0 too, log gives -inf and the ratio +inf)
    cov = random_cov(np.random.default_rng(12)); cov[5, :] = 0.0; cov[:, 5] = 0.0
    out.append(("singular", P(max_kf_t_dist=FAR, max_kf_r_dist=FAR), [result(np_model.expmap_se3(np.array([0.0, 0.0, -0.05, 0, 0, 0])), cov)], 0, "inf"))
    # g: a NaN in DT_cov
    bad = _steady(1)[0].copy(); c = bad["cov"].copy(); c[0] = np.nan; bad["cov"] = c
    out.append(("nan", P(min_entropy_ratio=-FAR, max_kf_t_dist=FAR, max_kf_r_dist=FAR), _steady(1) + [bad], 1, "nan"))
    return [(n, p, np.array(r, dtype=POSE_RESULT_DTYPE), i, t) for n, p, r, i, t in out]


def trigger_batch(n_updates=13):
    """[stream][update]: the trigger sequences side by side, the shorter ones continued with steady frames."""
    rows = []
    for _, _, res, _, _ in triggers():
        pad = np.array(_steady(n_updates), dtype=POSE_RESULT_DTYPE)
        rows.append(np.concatenate([res, pad])[:n_updates])
    return np.stack(rows)


def phased(B, n_updates, n=N_FRAMES):
    """[stream][update]: stream b runs the sequence of case 1 from frame b mod n on."""
    res = sequence(n=n)
    return np.stack([res[(b + np.arange(n_updates)) % n] for b in range(B)])


def run_ld(prm, results):
    """The extended-precision chain (each frame from the rounded state of the one before): [(record, terms)], final state."""
    s, out = npt.initial_state(), []
    for r in results:
        s_ld, rec, terms = npt.update(s, r["T"], r["cov"], int(r["status"]), prm)
        out.append((rec, terms))
        s = npt.rounded(s_ld)
    return out, s


# ---- one checker for every statement that updates a batch (the host function on the CPU, the kernel on the device)
_expect = {}


def _ld_expect(state_rec, res_rec, p):
    key = (state_rec.tobytes(), res_rec["T"].tobytes(), res_rec["cov"].tobytes(), int(res_rec["status"]), bytes(p))
    if key not in _expect:
        prm = prm_dict(p)
        s_ld, r_ld, _ = npt.update(state_to_dict(state_rec), res_rec["T"], res_rec["cov"], int(res_rec["status"]), prm)
        _expect[key] = (s_ld, r_ld, bool(prm["keyframes"] and near_threshold(r_ld, prm)))
    return _expect[key]


def check_batch(update_fn, p, results, state0, bound):
    """results [B][U]: U updates of B streams by update_fn(results [B], p, state [B]) -> (state [B], records [B]) from state0 [B].
    After every update, every stream against one extended-precision update from the state the statement itself held before it:
    decisions, counters and reset values exact, the floating-point fields within `bound` (dict per field).  Returns the largest
    deviation per field, the decisions [B][U] and the number of frames the guard would have left out (asserted 0 by the callers)."""
    B, U = results.shape
    state = state0.copy()
    worst = dict.fromkeys(npt.FIELDS, 0.0)
    decisions = np.zeros((B, U), np.int32)
    guarded = 0
    for u in range(U):
        before = state.copy()
        state, recs = update_fn(np.ascontiguousarray(results[:, u]), p, state)
        for b in range(B):
            s_ld, r_ld, near = _ld_expect(before[b], results[b, u], p)
            guarded += near
            where = (b, u)
            got_s, got_r = state_to_dict(state[b]), record_to_dict(recs[b])
            assert got_r["new_kf"] == r_ld["new_kf"], where
            assert got_r["frame"] == r_ld["frame"] == int(before[b]["n_frames"]) + 1, where
            for k in INT_FIELDS:
                assert got_s[k] == int(s_ld[k]), (where, k)
            assert np.array_equal(got_s["T_prevKF"], np.eye(4)), where
            if r_ld["new_kf"]:   # I, I, 0 exactly
                assert np.array_equal(got_s["Tfw"], np.eye(4)) and np.array_equal(got_s["Tfw_cov"], np.eye(6)), where
                assert not got_s["cov_prevKF_currF"].any() and got_s["prev_f_iskf"] == 1 and got_s["N_prevKF_currF"] == 0, where
            else:                # the state keeps the pose the record shows
                assert np.array_equal(got_s["Tfw"], got_r["Tfw"]) and np.array_equal(got_s["Tfw_cov"], got_r["Tfw_cov"], equal_nan=True), where
            if int(results[b, u]["status"]) != 0:   # carried over, bit for bit
                assert got_r["Tfw"].tobytes() == np.array(before[b]["Tfw"]).tobytes() and got_r["Tfw_cov"].tobytes() == np.array(before[b]["Tfw_cov"]).tobytes(), where
            if not p.keyframes:
                assert got_r["entropy_ratio"] == 0 and got_r["t"] == 0 and got_r["r"] == 0, where
            for k, v in deviation(npt.fields_of(got_s, got_r), npt.fields_of(s_ld, r_ld)).items():
                assert v <= bound[k], (where, k, v, bound[k])
                worst[k] = max(worst[k], v)
            decisions[b, u] = got_r["new_kf"]
    return worst, decisions, guarded


def host_update(results, p, state):
    import traj_host_lib
    state = state.copy()
    return state, traj_host_lib.update(results, p, state)
