"""GPU: the per-feature terms of the pose kernels at their edges (tests/pose_edge_cases.py), judged by the extended-precision
statement (tests/np_pose_terms.py) for single evaluations and by the oracle for whole optimizePose runs — on the latency kernel,
on both wave counts of the batch kernel, through the batched entry and through the device-resident pipeline (pose2c_kernel).
tests/test_pose_terms_host.py shows on the CPU that these inputs are fair: the two CPU statements agree on every one of them."""
import numpy as np
import pytest

import np_pose_terms
import pipeline_ref
import pose_edge_cases as pec
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_pose import check_pose
from test_gpu_seq import run_and_compare
from test_gpu_track_batched import oracle_track_pl

pytestmark = pytest.mark.gpu
POSE_KERNELS = ["default", "1", "4:2", "4:4"]   # the library's choice, pose_kernel.hip, pose_kernel2p.hip with two / four waves per pair
FLOWS = [("kitti", 0), ("euroc", 0), ("euroc", 1), ("euroc", 2)]


def select_kernel(switches, which):
    if which != "default":
        k, _, nw = which.partition(":")
        switches(dict({"STVO_POSE_KERNEL": k}, **({"STVO_POSE2P_NW": nw} if nw else {})))


def finite(H, g, e):
    return bool(np.all(np.isfinite(np.asarray(H, np.float64))) and np.all(np.isfinite(np.asarray(g, np.float64))) and np.isfinite(float(e)))


@pytest.mark.parametrize("robust", [0, 1])
def test_single_evaluations_vs_extended_precision(hip, oracle, robust):
    """stvo_normal_eq on every single-feature row and every mixture against the extended statement: deviation (max|dH| / max|H|,
    max|dg| / max|g|, |de| / |e|) <= max(floor, 16 x the oracle's deviation in the same case), n equal, H exactly symmetric, finite
    exactly where the oracle is.  Every figure is printed before the assertion (run with -s); DESIGN.md section 3 has the measured ones."""
    prm = opt_params("kitti")
    table = pec.evaluations(oracle)
    bad, worst_ratio, worst_abs, worst_mix = [], (0.0, ""), (0.0, ""), 0.0
    for (name, rb), ev in table.items():
        if rb != robust:
            continue
        H, g, e, n = hip.normal_eq(ev["DT"], ev["cam"], prm, ev["rec"], robust)
        xH, xg, xe, xn = ev["ext"][:4]
        oH, og, oe, on = ev["orc"]
        d = np_pose_terms.deviation(H, g, e, xH, xg, xe)
        b = pec.bound(ev, robust)
        print(f"device vs extended  {name:34s} robust={robust}  dH={d[0]:.2e} dg={d[1]:.2e} de={d[2]:.2e}   "
              f"oracle dH={ev['dev_orc'][0]:.2e} dg={ev['dev_orc'][1]:.2e} de={ev['dev_orc'][2]:.2e}")
        if n != xn:
            bad.append((name, "n", n, xn))
        if not np.array_equal(H, H.T):
            bad.append((name, "H is not symmetric"))
        if finite(H, g, e) != finite(oH, og, oe):
            bad.append((name, "finiteness", finite(H, g, e), finite(oH, og, oe)))
        if not all(x <= y for x, y in zip(d, b)):
            bad.append((name, "deviation", d, b))
        for x, o in zip(d, ev["dev_orc"]):
            if np.isfinite(x):
                worst_abs = max(worst_abs, (x, name))
                if name.startswith("mix-"):
                    worst_mix = max(worst_mix, x)
                if x > pec.FLOOR[robust] and o > 0:
                    worst_ratio = max(worst_ratio, (x / o, name))
    print(f"robust={robust}: largest device / oracle deviation ratio above the floor {worst_ratio}, largest deviation {worst_abs}, "
          f"largest on a mixture {worst_mix:.2e}")
    assert not bad, bad


@pytest.mark.parametrize("robust", [0, 1])
def test_degenerate_segments_vs_oracle(hip, oracle, robust):
    """Observed segments shorter than a pixel in both directions with dy = 0 (infinite or NaN lambdas in lineSegmentOverlap): the same
    finiteness as the oracle and, where finite, the plain tolerance of test_normal_eq_vs_oracle.  The extended statement is no judge
    here: one rounding decides 0 / 0."""
    prm = opt_params("kitti")
    seen = set()
    for name, cam, DT, rec in pec.degenerate_cases():
        H, g, e, n = hip.normal_eq(DT, cam, prm, rec, robust)
        oH, og, oe, on = oracle.optimize_functions(DT, cam, prm, rec, robust)
        assert n == on and finite(H, g, e) == finite(oH, og, oe), name
        seen.add(finite(oH, og, oe))
        if finite(oH, og, oe):
            tol = pec.FLOOR[robust]
            assert np.allclose(H, oH, rtol=tol, atol=0.1 * tol * np.abs(oH).max()), name
            assert np.allclose(g, og, rtol=tol, atol=0.1 * tol * np.abs(og).max()), name
            assert np.isclose(e, oe, rtol=tol), name
            assert np.array_equal(H, H.T), name
    assert seen == {True, False}


_REFS = {}


def oracle_pose(oracle, name, rec, preset, mode):
    key = (name, preset, mode)
    if key not in _REFS:
        _REFS[key] = oracle.optimize_pose(np.eye(4), pec.CAM_A, opt_params(preset, mode=mode), rec)
    return _REFS[key]


@pytest.mark.parametrize("preset,mode", FLOWS)
@pytest.mark.parametrize("kernel", POSE_KERNELS)
def test_mixture_flows_vs_oracle(hip, oracle, switches, kernel, preset, mode):
    """The whole optimizePose on the edge mixtures, on every pose kernel: 61 / 7 (a few features per wave), 449 / 65 (one thread of the
    latency kernel owns a pair, every other one runs the weight-0 duplicate) and 2048 / 512 (every ordinal, the arena-resident ones of
    pose2p_kernel included).  No case is skipped or excused: the CPU statements agree on all of them (test_pose_terms_host.py)."""
    select_kernel(switches, kernel)
    prm = opt_params(preset, mode=mode)
    for name, rec in pec.mixtures():
        ref = oracle_pose(oracle, name, rec, preset, mode)
        assert ref["status"] == 0 and ref["path"] == 5, name
        out = hip.optimize_pose(np.eye(4), pec.CAM_A, prm, rec)
        check_pose(out, ref)


@pytest.mark.parametrize("preset,mode", FLOWS)
def test_mixture_frames_through_track_batched(hip, oracle, preset, mode):
    """The same mixtures as TrackBatch frames (frame_from_records: the f2f match is a known permutation), B = 3, on the library's own
    kernel choice: match indices, gathered records, pose — the per-pair assertions of test_track_batched_points_and_lines."""
    import torch
    from stvo_amd.devbatch import TrackBatch
    import np_model
    frames = [pec.frame_from_records(rec, 300 + i) for i, (name, rec) in enumerate(pec.mixtures())]
    batch = TrackBatch(frames, max_pts=2048, max_lines=512)
    prm = opt_params(preset, mode=mode)
    nnr = 0.75
    hip.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        hip.track_batched(batch, pec.CAM_A, prm, nnr, nnr, 1)
        torch.cuda.synchronize()
    finally:
        hip.set_stream(None)
    res = batch.results(); mp_all = batch.m12_pts(); ml_all = batch.m12_lines(); ip_all = batch.inlier_pts(); il_all = batch.inlier_lines()
    for b, fr in enumerate(frames):
        m12, sel, m12l, sl, ref = oracle_track_pl(oracle, fr, prm, nnr, nnr)
        n1, n1l = len(fr["prev_P"]), len(fr["prev_sP"])
        assert len(sel) == n1 and len(sl) == n1l   # every record is matched: optimizePose sees the mixture itself
        assert np.array_equal(mp_all[b, :n1], m12) and np.array_equal(ml_all[b, :n1l], m12l)
        assert res["status"][b] == ref["status"] and res["path"][b] == ref["path"] and tuple(res["iters"][b]) == ref["iters"]
        assert res["n_matched_pt"][b] == len(sel) and res["n_matched_ls"][b] == len(sl)
        assert res["n_inliers_pt"][b] == ref["n_inliers_pt"] and res["n_inliers_ls"][b] == ref["n_inliers_ls"]
        e = -np.ones(n1, np.int32); e[sel] = ref["inlier_p"]
        assert np.array_equal(ip_all[b, :n1], e)
        e = -np.ones(n1l, np.int32); e[sl] = ref["inlier_l"]
        assert np.array_equal(il_all[b, :n1l], e)
        T = res["T"][b].reshape(4, 4)
        assert np_model.rot_angle(T[:3, :3], ref["T"][:3, :3]) < 1e-4 and np.linalg.norm(T[:3, 3] - ref["T"][:3, 3]) < 1e-3
        assert np.allclose(T, ref["T"], atol=1e-8) and np.isclose(res["err"][b], ref["err"], rtol=1e-8)
        assert ref["status"] == 0


@pytest.mark.parametrize("kernel", POSE_KERNELS)
def test_still_rig_records(hip, oracle, switches, kernel):
    """A rig that stands still: every residual is rounding noise below homog_th, so both selects fire for every feature of every
    evaluation; H ~ 1e-5 and the solution is rejected through the robust fallback — the held pose, exactly."""
    select_kernel(switches, kernel)
    prm = opt_params("kitti")
    for seed in (0, 1):
        rec = pec.still_rig_records(seed)
        ref = oracle.optimize_pose(np.eye(4), pec.CAM_A, prm, rec)
        assert ref["status"] == 3 and ref["path"] == 2 and ref["iters"] == (1, 1)
        out = hip.optimize_pose(np.eye(4), pec.CAM_A, prm, rec)
        assert out["status"] == ref["status"] and out["path"] == ref["path"] and out["iters"] == ref["iters"], (out["status"], out["path"], out["iters"])
        assert np.array_equal(out["T"], np.eye(4)) and out["err"] == -1.0 and not np.any(out["cov"])


@pytest.mark.parametrize("n_streams", [1, 4])
@pytest.mark.parametrize("kernel", POSE_KERNELS)
def test_still_rig_pipeline(oracle, switches, kernel, n_streams):
    """The still rig through the device-resident pipeline — the only way to pose2c_kernel (compact records; "4:2" / "4:4" force it for
    these few streams): the same stereo frame three times, as one stream and as four.  Every transition reports the oracle's status,
    path and pose (run_and_compare), and the oracle's are the rejected solution: status 3 through the robust fallback, identity."""
    select_kernel(switches, kernel)
    cam = synth.KITTI_CAM
    seqs = pec.still_rig_sequences(n_streams)
    mp, op = match_params("kitti"), opt_params("kitti")
    for seq in seqs:
        for o in pipeline_ref.run_sequence(oracle, seq, cam, mp, op):
            assert o["n_matched_pt"] > 200 and o["n_matched_ls"] > 20
            assert o["status"] == 3 and o["path"] == 2 and np.array_equal(o["T"], np.eye(4)) and o["err"] == -1.0
    run_and_compare(oracle, seqs, cam, "kitti")
