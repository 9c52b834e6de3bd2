"""CPU: what tests/outlier_cut_cases.py claims about its cases — the planned residuals are the residuals, bit for bit; three CPU
statements of vector_mean_stdv_mad + the cut agree on every case (a plain one written here, np_model, the C oracle) and equal the
`keep` flags the generator states by counting; optimizePose with min_error = 1e30 is one cut at the initial pose; the robust cases
are sensitive to a rank error of one; every branch the cases are meant to take is taken; the point plans survive the stereo
association and the f2f match of the pipeline as the planned doubles.  tests/test_gpu_outlier_cut.py runs the same cases on every
pose kernel."""
import numpy as np
import pytest

import np_model
import np_pose_terms
import outlier_cut_cases as occ
import pose_edge_cases as pec
from stvo_amd.ctypes_types import STATUS_FEW_AFTER, STATUS_OK

CASES = occ.cases()
NAMES = [c["name"] for c in CASES]
FEW_AFTER = {"gate-count-11", "gate-count-11-swapped", "cut-below-min-features", "cut-below-min-features-swapped"}   # the cases whose cut leaves fewer than min_features inliers


def statement(r):
    """vector_mean_stdv_mad, src/auxiliar.cpp:387-430: (mean, stdv)"""
    n = len(r)
    if n == 0:
        return 0.0, 0.0
    s = sorted(float(x) for x in r)
    median = s[n // 2]
    dev = sorted(float(abs(np.float32(x - median))) for x in s)   # fabsf: the deviations are floats
    stdv = 1.4826 * dev[n // 2]
    below = [x for x in r if x < 2.0 * stdv]
    if len(below) >= int(0.2 * n):
        with np.errstate(invalid="ignore"):
            return float(np.float64(sum(below)) / np.float64(len(below))), stdv
    return sum(float(x) for x in r) / n, stdv


def cut(r, inl, inlier_k):
    """removeOutliers, src/stereoFrameHandler.cpp:988-1067, for one kind of feature"""
    mean, stdv = statement(r)
    return np.array([bool(i) and not abs(x - mean) > inlier_k * stdv for x, i in zip(r, inl)], bool)


def residuals(rec):
    rp = np_model.point_residuals(occ.CAM, occ.DT0, rec) * np.sqrt(rec["sigma2p"]) if len(rec["sigma2p"]) else np.zeros(0)
    rl = np_model.line_residuals(occ.CAM, occ.DT0, rec) * np.sqrt(rec["sigma2l"]) if len(rec["sigma2l"]) else np.zeros(0)
    return rp, rl


@pytest.mark.parametrize("name", NAMES)
def test_planned_residuals_are_the_residuals(name):
    c = occ.by_name(name)
    rec, op, ol, _, _ = occ.built(name)
    rp, rl = residuals(rec)
    for got, plan, order in ((rp, c["plan_p"], op), (rl, c["plan_l"], ol)):
        want = np.array([plan[j].r for j in order], np.float64)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name                               # per feature, bit for bit
        assert np.array_equal(np.sort(got), np.sort(np.array([f.r for f in plan], np.float64))), name     # and as a multiset
        assert np.all(np.isfinite(got))
    assert np.array_equal(rec["inlier_p"], [c["plan_p"][j].inl for j in op]) and np.array_equal(rec["inlier_l"], [c["plan_l"][j].inl for j in ol])
    if c["placement"] == "ascending":
        assert np.all(np.diff(rp) >= 0) and np.all(np.diff(rl) >= 0)
    if c["placement"] == "descending":
        assert np.all(np.diff(rp) <= 0) and np.all(np.diff(rl) <= 0)


@pytest.mark.parametrize("name", NAMES)
def test_three_statements_agree_with_the_stated_outcome(oracle, name):
    c = occ.by_name(name)
    rec, op, ol, ep, el = occ.built(name)
    prm = occ.params(c)
    rp, rl = residuals(rec)
    for r, side in ((rp, "p"), (rl, "l")):   # mean and stdv: the statement, np_model, the oracle, the generator's count
        mean, stdv = statement(r)
        st = c["stats"][side]
        for m2, s2 in (np_model.mean_stdv_mad(r), oracle.mean_stdv_mad(r), (st.mean, st.sigma)):
            assert s2 == stdv and (m2 == mean or (np.isnan(m2) and np.isnan(mean))), (name, side, mean, stdv, m2, s2)
    want_p = cut(rp, rec["inlier_p"], prm.inlier_k) if prm.has_points else rec["inlier_p"].astype(bool)
    want_l = cut(rl, rec["inlier_l"], prm.inlier_k) if prm.has_lines else rec["inlier_l"].astype(bool)
    assert np.array_equal(want_p, ep.astype(bool)) and np.array_equal(want_l, el.astype(bool)), name
    mp, ml = np_model.remove_outliers(occ.DT0, occ.CAM, np_model.prm_dict(prm), rec, rec["inlier_p"], rec["inlier_l"])
    assert np.array_equal(mp, want_p) and np.array_equal(ml, want_l), name
    ip, il, npt, nls = oracle.remove_outliers(occ.DT0, occ.CAM, prm, rec)
    assert np.array_equal(ip, ep) and np.array_equal(il, el) and npt == ep.sum() and nls == el.sum(), name
    # nothing is re-admitted
    assert not np.any(ep > rec["inlier_p"]) and not np.any(el > rec["inlier_l"])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_optimize_pose_is_one_cut_at_the_initial_pose(oracle, name):
    rec, op, ol, ep, el = occ.built(name)
    ref = occ.oracle_pose(oracle, name)
    assert np.array_equal(ref["inlier_p"], ep) and np.array_equal(ref["inlier_l"], el), name
    assert ref["n_inliers_pt"] == ep.sum() and ref["n_inliers_ls"] == el.sum()
    assert ref["n_matched_pt"] == len(ep) and ref["n_matched_ls"] == len(el)
    if name in FEW_AFTER:   # stage 1 good, the cut leaves fewer than min_features: DT = I, no refinement
        assert ep.sum() + el.sum() < occ.params(occ.by_name(name)).min_features
        assert ref["status"] == STATUS_FEW_AFTER and ref["path"] == 1 and ref["iters"] == (1, 0)
        assert np.array_equal(ref["T_opt"], np.eye(4))
    else:
        assert ref["status"] == STATUS_OK and ref["path"] == 5 and ref["iters"] == (1, 1), (name, ref["status"], ref["path"], ref["iters"])
        assert np.array_equal(ref["T_opt"], occ.DT0)                       # bit for bit: no step was taken
        assert np.array_equal(ref["T"], np_model.inverse_se3(occ.DT0))     # the translation (-0.25, 0.5, 0)
        # isGoodSolution is far from both of its edges: cov's eigenvalues in (0, 1) with room, H's spread over fewer than 5 decades
        assert 0 < ref["cov_eig"].max() < 1e-3 and ref["cov_eig"].min() > 1e-5 * ref["cov_eig"].max() and 0 < ref["err"] < 1, name


def order_stat_scale(off_med, off_mad):
    """vector_stdv_mad with the median taken at rank n / 2 + off_med and the MAD at rank n / 2 + off_mad"""
    def f(r):
        r = np.asarray(r, float)
        n = len(r)
        if n == 0:
            return 0.0
        s = np.sort(r)
        dev = np.sort(np.abs((s - s[n // 2 + off_med]).astype(np.float32)).astype(np.float64))
        return 1.4826 * dev[n // 2 + off_mad]
    return f


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["robust"]])
def test_robust_cases_feel_a_rank_error_of_one(oracle, monkeypatch, name):
    """The robust evaluation with the neighbouring order statistic for the median or for the MAD deviates from the right one by more
    than 1000 x what the GPU test allows (pose_edge_cases.bound) in H, g or e: a selection that is off by one rank cannot pass."""
    c = occ.by_name(name)
    rec = occ.built(name)[0]
    prm = occ.params(c)
    ext = np_pose_terms.evaluate(occ.DT0, occ.CAM, prm.homog_th, rec, True)
    orc = oracle.optimize_functions(occ.DT0, occ.CAM, prm, rec, 1)
    dev_orc = np_pose_terms.deviation(orc[0], orc[1], orc[2], ext[0], ext[1], ext[2])
    bound = pec.bound(dict(dev_orc=dev_orc), 1)
    assert all(d <= b for d, b in zip(dev_orc, bound))
    for off_med, off_mad in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        monkeypatch.setattr(np_model, "stdv_mad", order_stat_scale(off_med, off_mad))
        wrong = np_pose_terms.evaluate(occ.DT0, occ.CAM, prm.homog_th, rec, True)
        monkeypatch.undo()
        assert (wrong[4], wrong[5]) != (ext[4], ext[5])
        d = np_pose_terms.deviation(np.asarray(wrong[0], np.float64), np.asarray(wrong[1], np.float64), float(wrong[2]), ext[0], ext[1], ext[2])
        print(f"{name}: rank offsets median {off_med:+d} MAD {off_mad:+d}: scales {wrong[4]:.4f} {wrong[5]:.4f} (right {ext[4]:.4f} {ext[5]:.4f}), "
              f"deviation {d[0]:.2e} {d[1]:.2e} {d[2]:.2e}, bound {bound[0]:.1e}")
        assert max(x / b for x, b in zip(d, bound)) > 1000.0, (name, off_med, off_mad, d, bound)


def test_every_intended_branch_is_taken(oracle):
    kinds = {(side, c["stats"][side].mean_kind) for c in CASES for side in "pl"}
    assert {(s, k) for s in "pl" for k in ("gated", "full", "nan", "none")} <= kinds       # gated mean, full-mean fallback, 0 / 0, empty kind
    for side, plan in (("p", "plan_p"), ("l", "plan_l")):
        has = lambda pred: any(pred(c, c["stats"][side], c[plan]) for c in CASES)   # noqa: E731
        assert has(lambda c, st, p: st.n > 4 and st.mad == 0.0 and all(f.keep for f in p))                                    # MAD 0, all at the mean
        assert has(lambda c, st, p: st.mad == 0.0 and 0 < sum(f.keep for f in p) < st.n and all(f.r == st.mean for f in p if f.keep))   # everything but the mean cut
        assert has(lambda c, st, p: st.mad == 0.0 and st.n > 4 and not any(f.keep for f in p))                               # MAD 0, the mean is nobody's value
        assert has(lambda c, st, p: st.mean_kind == "nan" and all(f.keep for f in p))                                         # NaN mean: nothing cut
        assert has(lambda c, st, p: st.n > 4 and st.mad > 0 and all(f.keep == f.inl for f in p))                              # nothing cut
        assert has(lambda c, st, p: any(not f.inl for f in p) and any(f.inl and not f.keep for f in p))                      # arrive as outliers
        assert has(lambda c, st, p: 1 <= st.n <= 4) and has(lambda c, st, p: st.n == 0)
        assert has(lambda c, st, p: st.ksel == int(0.2 * st.n) and st.mean_kind == "gated")                                   # the count AT the gate
        assert has(lambda c, st, p: st.ksel == int(0.2 * st.n) - 1 and st.mean_kind == "full")                                # and one fewer
        assert has(lambda c, st, p: any(abs(f.r - st.mean) == st.th and f.keep and st.th > 0 for f in p)                      # at the threshold: kept
                   and any(abs(f.r - st.mean) == np.nextafter(st.th, np.inf) and not f.keep for f in p))                      # one ulp beyond: cut
        assert has(lambda c, st, p: any(f.r == 0.0 for f in p) and st.mad > 0)
        assert has(lambda c, st, p: st.sigma > 0 and any(f.r == 2.0 * st.sigma for f in p))                                   # a value AT 2 sigma
    assert any(not c["has_points"] and len(c["plan_p"]) for c in CASES) and any(not c["has_lines"] and len(c["plan_l"]) for c in CASES)
    assert {c["placement"] for c in CASES} == {"ascending", "descending", "shuffle"}
    assert {c["prm"] for c in CASES} == {"kitti", "euroc", "edge"}
    for name in FEW_AFTER:
        assert occ.oracle_pose(oracle, name)["status"] == STATUS_FEW_AFTER
    # sizes: the ordinals of pose_edge_cases, and the line counts on both sides of what the solver wave of pose_kernel holds (128)
    sizes = {(len(c["plan_p"]), len(c["plan_l"])) for c in CASES}
    assert set(pec.MIXTURE_SIZES) <= sizes
    assert any(nl <= 128 for _, nl in sizes) and any(nl > 128 for _, nl in sizes)
    assert max(n for n, _ in sizes) <= 2048 and max(nl for _, nl in sizes) <= 512


def transition(oracle, name):
    """the matched records pipeline_ref.run_sequence hands to optimizePose at the one transition of a pipeline_sequence, and its result"""
    import pipeline_ref
    from stvo_amd.ctypes_types import match_params
    frames, r, keep = occ.pipeline_sequence(name)
    mp, op = match_params("kitti"), occ.opt_params("kitti", min_error=occ.MIN_ERROR)
    prev, curr = (pipeline_ref.stereo_frame(oracle, f, occ.CAM, mp, True, True) for f in frames)
    m12, _ = oracle.match(prev["pdesc"], curr["pdesc"], mp.min_ratio_12_p, mp.best_lr_matches)
    out = pipeline_ref.run_sequence(oracle, frames, occ.CAM, mp, op)
    return prev, curr, m12, out[0], r, keep


@pytest.mark.parametrize("name", occ.PIPELINE_CASES)
def test_pipeline_sequences_carry_the_plan(oracle, name):
    """Through the oracle-driven pipeline (stereo association, back-projection, f2f match): every left key-point becomes a stereo point
    in both frames, pair i is matched to itself, its residual at DT = I is the planned double, and the oracle's optimizePose is one
    cut — status 3 (the committed pose is I, the rejected solution), path 5, iters (1, 1), the stated flags."""
    prev, curr, m12, o, r, keep = transition(oracle, name)
    n = len(r)
    assert len(prev["P"]) == len(curr["P"]) == n and np.array_equal(m12, np.arange(n))
    assert np.all(prev["sigma2p"] == 1.0)
    rec = dict(P=prev["P"], pl_obs=curr["pl"], sigma2p=prev["sigma2p"])
    got = np_model.point_residuals(occ.CAM, np.eye(4), rec)
    assert np.array_equal(got.view(np.uint64), r.view(np.uint64))
    assert (o["status"], o["path"], o["iters"]) == (3, 5, (1, 1)) and o["n_matched_pt"] == n and o["n_matched_ls"] == 0
    assert np.array_equal(o["inlier_p"], keep.astype(np.int32)) and o["n_inliers_pt"] == keep.sum()
    assert np.array_equal(keep, cut(r, np.ones(n, bool), 1.2))
