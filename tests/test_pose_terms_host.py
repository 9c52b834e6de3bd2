"""The per-feature terms at their edges, on the host: shows that the inputs of tests/test_gpu_pose_edges.py are fair before a GPU
is touched.  The extended-precision statement (np_pose_terms.py) judges the oracle, the numpy model and the fast forms the kernels
are built from (pm::point_term_q / pm::line_term_q through tests/cpp/pm_host.cpp::pmh_normal_eq_q)."""
import ctypes as C

import numpy as np
import pytest

import np_model
import np_pose_terms
import oracle_lib
import pm_host_lib
import pose_edge_cases as pec
from stvo_amd import synth
from stvo_amd.ctypes_types import Cam, opt_params

EPS = np.finfo(np.float64).eps


def amplification(cam, DT, rec):
    """How much one case amplifies a rounding of its FP64 evaluation — from the inputs alone: a point at depth gz whose transform sums
    terms of size M carries a relative error eps M / |gz| into its pixel, and a residual |e| that is the difference of pixel-sized
    numbers U carries eps U / |e|.  The largest (1 + M / |gz|) (1 + U / |e|) over the features; 1 for an exactly zero residual."""
    R, t = DT[:3, :3], DT[:3, 3]
    k = 1.0

    def px(P):
        g = R @ P + t
        M = np.abs(R[2] * P).sum() + abs(t[2])
        u = np.array([cam["cx"] + cam["fx"] * g[0] / g[2], cam["cy"] + cam["fy"] * g[1] / g[2]])
        return u, 1.0 + M / abs(g[2]), 1.0 + max(np.abs(R[:2] * P).sum(1).max(), np.abs(t[:2]).max()) / max(np.abs(g[:2]).max(), 1e-300)
    with np.errstate(all="ignore"):
        for P, o in zip(rec["P"], rec["pl_obs"]):
            u, kz, kxy = px(P)
            e = np.linalg.norm(u - o)
            U = max(np.abs(u).max(), np.abs(o).max(), cam["cx"], cam["cy"])
            k = max(k, kz * kxy * (1.0 + (U / e if e > 0 else 0.0)))
        for sP, eP, le in zip(rec["sP"], rec["eP"], rec["le_obs"]):
            for P in (sP, eP):
                u, kz, kxy = px(P)
                d = le[0] * u[0] + le[1] * u[1] + le[2]
                U = abs(le[0] * u[0]) + abs(le[1] * u[1]) + abs(le[2]) + abs(le[0]) * cam["cx"] + abs(le[1]) * cam["cy"]
                k = max(k, kz * kxy * (1.0 + (U / abs(d) if d != 0 else 0.0)))
    return k


def fp64_bound(name, ev, robust):
    """A-priori bound of an FP64 statement's deviation from the extended one.  Single features: 64 eps (a chain of about 60 operations,
    each within one rounding) times the case's amplification.  Mixtures: 1e-11 — up to 2560 features of about 60 operations each add
    their roundings linearly at worst (2560 x 60 x eps = 1.7e-11 if every one had the same sign; they do not), and the features whose
    residual is rounding noise enter H through the 1 / homog_th clamp, six orders below a regular term.  Robust evaluations: the scale
    is a float-truncated MAD of residuals that differ in their last bits, hence the 1e-6 floor of fuzz_entry_points.py."""
    b = 1e-11 if name.startswith("mix-") else 64.0 * EPS * amplification(ev["cam"], ev["DT"], ev["rec"])
    return max(b, 1e-6) if robust else b


@pytest.fixture(scope="module")
def pmh():
    return pm_host_lib.load()


@pytest.fixture(scope="module")
def table(oracle):
    return pec.evaluations(oracle)


def test_extended_precision_is_extended():
    assert np_pose_terms.BACKEND == "mpmath" or np.finfo(np.longdouble).eps < 1e-18


def test_single_cases_reach_what_they_name(table):
    """The generator's claims, checked in extended precision: which side of each homog_th select a row is on, and the overlap value
    of each lambda case."""
    rows = {name.rsplit("@", 1)[0] for name, _ in table}
    for need in ("pt-zero-residual", "pt-e-below-th", "pt-e-above-th", "pt-gz2-below-th", "pt-gz2-above-th", "pt-behind", "pt-far",
                 "pt-residual-1e4", "pt-sigma2-level7", "ln-covers", "ln-inside", "ln-disjoint-low", "ln-disjoint-high", "ln-partial-low",
                 "ln-partial-high", "ln-reversed", "ln-obs-dx-0", "ln-obs-dx-0.999", "ln-obs-dx-1.0", "ln-obs-dy-0.999", "ln-sigma2-level4",
                 "ln-zero-residual", "ln-both-behind", "ln-straddles"):
        assert need in rows, need
    cams = [ev["cam"] is pec.CAM_B for (name, rb), ev in table.items() if rb == 0 and not name.startswith("mix-")]
    assert 0.25 < np.mean(cams) < 0.45
    L = np.longdouble
    for (name, rb), ev in table.items():
        if rb or name.startswith("mix-"):
            continue
        rec, DT, cam = ev["rec"], ev["DT"], ev["cam"]
        if name.startswith("pt-"):
            g = DT[:3, :3].astype(L) @ rec["P"][0].astype(L) + DT[:3, 3].astype(L)
            u = pec._proj_ld(DT, cam, rec["P"][0])
            e = float(np.sqrt(((u - rec["pl_obs"][0].astype(L)) ** 2).sum()))
            gz2 = float(g[2] * g[2])
            if "zero" in name: assert e == 0.0
            if "e-below" in name: assert 0.5e-7 < e < 0.7e-7
            if "e-above" in name: assert 1.5e-7 < e < 1.7e-7
            if "gz2-below" in name: assert 3e-8 < gz2 < 5e-8
            if "gz2-above" in name: assert 1.5e-7 < gz2 < 1.7e-7
            if "behind" in name: assert g[2] < -1
            if "far" in name: assert g[2] > 9e4
            if "1e4" in name: assert e > 1e4
        else:
            s = pec._proj_ld(DT, cam, rec["sP"][0]); t = pec._proj_ld(DT, cam, rec["eP"][0])
            ov = float(np_pose_terms.line_overlap(rec["spl"][0].astype(L), rec["epl"][0].astype(L), s, t))
            want = {"ln-covers": 1.0, "ln-inside": 0.5, "ln-disjoint-low": 0.0, "ln-disjoint-high": 0.0, "ln-partial-low": 0.5,
                    "ln-partial-high": 0.5, "ln-reversed": 0.5}.get(name.rsplit("@", 1)[0])
            if want is not None:
                assert abs(ov - want) < 0.03, (name, ov)
            dx, dy = abs(rec["spl"][0, 0] - rec["epl"][0, 0]), abs(rec["spl"][0, 1] - rec["epl"][0, 1])
            if "dx-0@" in name: assert dx == 0.0
            if "dx-0.999" in name: assert 0.99 < dx < 1.0
            if "dx-1.0" in name: assert dx == 1.0 and dy > 1.0
            if "dy-0.999" in name: assert dx > 1.0 and 0.99 < dy < 1.0
            if "zero" in name: assert float(ev["ext"][2]) == 0.0 and not np.any(ev["ext"][0] != 0)


@pytest.mark.parametrize("robust", [0, 1])
def test_oracle_and_numpy_model_vs_extended(table, robust):
    """Both FP64 statements of the suite against the extended one, on every single-feature row and every mixture; prints the oracle's
    deviation per case (NOTES.md records them)."""
    prm = np_model.prm_dict(opt_params("kitti"))
    worst = {}
    for (name, rb), ev in table.items():
        if rb != robust:
            continue
        xH, xg, xe, xn = ev["ext"][:4]
        oH, og, oe, on = ev["orc"]
        b = fp64_bound(name, ev, robust)
        d = ev["dev_orc"]
        print(f"oracle vs extended  {name:34s} robust={robust}  dH={d[0]:.2e} dg={d[1]:.2e} de={d[2]:.2e}  bound={b:.1e}")
        assert on == xn
        assert max(d) <= b, (name, d, b)
        rec = ev["rec"]
        mH, mg, me = np_model.optimize_functions(ev["DT"], ev["cam"], prm, rec, rec["inlier_p"], rec["inlier_l"], robust=bool(robust))
        dm = np_pose_terms.deviation(mH, mg, me, xH, xg, xe)
        assert max(dm) <= b, (name, dm, b)
        kind = "mixture" if name.startswith("mix-") else ("threshold" if "-e-" in name else "single")
        worst[kind] = max(worst.get(kind, 0.0), max(d))
    print("oracle vs extended, largest deviation by kind:", {k: f"{v:.2e}" for k, v in worst.items()})


def eval_q(pmh, ev, robust):
    rec = ev["rec"]
    m, keep = oracle_lib.Oracle._matched(rec)
    cam = Cam.from_dict(ev["cam"])
    acc = np.empty(28)
    pmh.pmh_normal_eq_q(np.ascontiguousarray(ev["DT"], np.float64).reshape(-1), C.byref(cam), pec.HOMOG_TH, C.addressof(m), robust,
                        ev["ext"][4], ev["ext"][5], acc)
    H, g, e = pm_host_lib.unpack28(acc)
    n = int((rec["inlier_p"] > 0).sum() + (rec["inlier_l"] > 0).sum())
    with np.errstate(all="ignore"):
        return H, g, float(np.float64(e) / np.float64(n)), n


@pytest.mark.parametrize("robust", [0, 1])
def test_fast_forms_vs_extended(pmh, table, robust):
    """pm::point_term_q / pm::line_term_q as the kernels call them (sqrt(sigma2) in the record, 1 / homog_th, reciprocal scales) under
    the bound of the GPU test: max(floor, 16 x the oracle's deviation in the same case)."""
    for (name, rb), ev in table.items():
        if rb != robust:
            continue
        H, g, e, n = eval_q(pmh, ev, robust)
        d = np_pose_terms.deviation(H, g, e, *ev["ext"][:3])
        b = pec.bound(ev, robust)
        assert n == ev["ext"][3]
        assert all(x <= y for x, y in zip(d, b)), (name, d, b)


@pytest.mark.parametrize("robust", [0, 1])
def test_degenerate_segments_fast_forms_vs_oracle(pmh, oracle, robust):
    """Observed segments shorter than a pixel in both directions with dy = 0: lineSegmentOverlap divides by zero.  The fast form and the
    oracle must agree on finiteness and, where finite, within the plain tolerance."""
    prm = opt_params("kitti")
    seen = set()
    for name, cam, DT, rec in pec.degenerate_cases():
        oH, og, oe, on = oracle.optimize_functions(DT, cam, prm, rec, robust)
        ev = dict(rec=rec, cam=cam, DT=DT, ext=(None,) * 4 + (1e-4, 1e-4))   # one feature: MAD = 0, clamped to 1e-4
        H, g, e, n = eval_q(pmh, ev, robust)
        fin = bool(np.all(np.isfinite(oH)) and np.all(np.isfinite(og)) and np.isfinite(oe))
        assert fin == bool(np.all(np.isfinite(H)) and np.all(np.isfinite(g)) and np.isfinite(e)), name
        seen.add(fin)
        if fin:
            assert np.allclose(H, oH, rtol=1e-10, atol=1e-11 * np.abs(oH).max()) and np.allclose(g, og, rtol=1e-10, atol=1e-11 * np.abs(og).max())
            assert np.isclose(e, oe, rtol=1e-10), name
    assert seen == {True, False}   # both outcomes occur


FLOWS = [("kitti", 0), ("euroc", 0), ("euroc", 1), ("euroc", 2)]


@pytest.mark.parametrize("preset,mode", FLOWS)
def test_mixture_flows_oracle_vs_numpy(oracle, preset, mode):
    """The whole optimizePose on the mixtures: the two CPU statements stay inside the tolerances of test_optimize_pose_vs_numpy, with
    the same status, path, iteration counts and masks — so the GPU flow tests need no sensitivity rule."""
    prm = opt_params(preset, mode=mode)
    for name, rec in pec.mixtures():
        out = oracle.optimize_pose(np.eye(4), pec.CAM_A, prm, rec)
        ref = np_model.optimize_pose(np.eye(4), pec.CAM_A, np_model.prm_dict(prm), rec)
        print(name, preset, mode, "status", out["status"], "path", out["path"], "iters", out["iters"])
        assert out["status"] == ref["status"] and out["path"] == ref["path"], name
        assert out["iters"] == ref["iters"], name
        assert np.array_equal(out["inlier_p"], ref["inlier_p"]) and np.array_equal(out["inlier_l"], ref["inlier_l"]), name
        assert np.allclose(out["T"], ref["T"], atol=1e-9), name
        assert np.allclose(out["cov"], ref["cov"], rtol=1e-7, atol=1e-12), name
        assert np.allclose(out["cov_eig"], ref["cov_eig"], rtol=1e-7, atol=1e-13), name
        assert np.isclose(out["err"], ref["err"], rtol=1e-9), name
        # and the comparison is one of solved problems: both stages ran and found the motion the benign features were generated with
        assert out["status"] == 0 and out["path"] == 5, name
        assert np.abs(out["T_opt"] - rec["T_true"]).max() < 0.03, name


def test_still_rig_is_rejected_by_both_statements(oracle):
    """A rig that stands still: every residual is rounding noise below homog_th, both selects fire for every feature, H is ~1e-5 and
    the covariance's eigenvalues exceed isGoodSolution's bound of 1 by orders: status 3 through the robust fallback, T = I, err = -1."""
    prm = opt_params("kitti")
    for seed in range(10):
        rec = pec.still_rig_records(seed)
        res = np_model.point_residuals(pec.CAM_A, np.eye(4), rec)
        assert res.max() < pec.HOMOG_TH
        H, _, _, _ = oracle.optimize_functions(np.eye(4), pec.CAM_A, prm, rec, 0)
        assert np.abs(H).max() < 1e-3
        for out in (oracle.optimize_pose(np.eye(4), pec.CAM_A, prm, rec),
                    np_model.optimize_pose(np.eye(4), pec.CAM_A, np_model.prm_dict(prm), rec)):
            assert out["status"] == 3 and out["path"] == 2 and tuple(out["iters"]) == (1, 1), (seed, out["status"], out["path"], out["iters"])
            assert np.array_equal(out["T"], np.eye(4)) and out["err"] == -1.0 and not np.any(out["cov"])


def test_frame_from_records_matches_back_to_the_records(oracle):
    """frame_from_records: the f2f match of the frame is its permutation and hands optimizePose the records unchanged."""
    name, rec = pec.mixtures()[0]
    fr = pec.frame_from_records(rec, 5)
    m12, n = oracle.match(fr["prev_desc"], fr["curr_desc"], 0.75)
    assert n == len(m12) and np.array_equal(fr["perm"][m12], np.arange(len(m12)))
    assert np.array_equal(fr["curr_pl"][m12], rec["pl_obs"])
    m12l, nl = oracle.match(fr["prev_ldesc"], fr["curr_ldesc"], 0.75)
    assert nl == len(m12l) and np.array_equal(fr["curr_le"][m12l], rec["le_obs"])


def test_still_rig_pipeline_is_rejected_by_the_oracle(oracle):
    """The still rig as the device-resident pipeline sees it (one stereo frame three times): the oracle-driven loop matches most of the
    features and rejects every transition — status 3 through the robust fallback, the held pose."""
    import pipeline_ref
    from stvo_amd.ctypes_types import match_params
    mp, op = match_params("kitti"), opt_params("kitti")
    for seq in pec.still_rig_sequences(4):
        res = pipeline_ref.run_sequence(oracle, seq, synth.KITTI_CAM, mp, op)
        assert len(res) == 2
        for o in res:
            assert o["n_matched_pt"] > 200 and o["n_matched_ls"] > 20
            assert o["status"] == 3 and o["path"] == 2 and np.array_equal(o["T"], np.eye(4)) and o["err"] == -1.0
