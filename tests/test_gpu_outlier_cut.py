"""GPU: removeOutliers and the robust scale on planned residual sets (tests/outlier_cut_cases.py) — the selection of pose_block.h
(BlockOps::select2 / mad_sigma2 / outlier_cut) in every pose kernel: ranks, ties, key shapes, the gates, the threshold edges, the
initial masks.  With min_error = 1e30 a whole optimizePose is ONE cut at the initial pose, so the inlier flags that come back are
the verdict on the selection; they must equal what the generator states by counting and what the oracle returns.
tests/test_outlier_cut_host.py shows on the CPU that the planned residuals are exact and that three CPU statements agree.

Which instantiation a size reaches (PPT / LPT keys per thread; the AND / OR prefix exchange needs 64-bit keys and >= 8 per thread):
  "1" (and "default" for a single pair)  pose_kernel, 7 worker waves: PPT 5, LPT 2, no exchange; <= 128 key-lines sit on the
                                          solver wave (own_b = sc), more on the workers
  "4:2"  pose2p_kernel / pose2c_kernel, 2 waves: PPT 16, LPT 4, exchange for the points; a thread's 8th key from 897 points
  "4:4"  pose2p_kernel / pose2c_kernel, 4 waves: PPT 8, LPT 2, exchange for the points; a thread's 8th key from 1793 points"""
import numpy as np
import pytest

import np_pose_terms
import outlier_cut_cases as occ
import pose_edge_cases as pec
from stvo_amd.ctypes_types import STATUS_FEW_AFTER, STATUS_OK, STATUS_REJECTED
from test_gpu_pose import check_pose
from test_gpu_pose_edges import POSE_KERNELS, select_kernel

pytestmark = pytest.mark.gpu
CASES = occ.cases()


def check_case(out, ref, name, ep, el):
    """one optimizePose at min_error = 1e30 against the stated outcome and the oracle"""
    assert np.array_equal(out["inlier_p"], ep) and np.array_equal(out["inlier_l"], el), \
        (name, np.nonzero(out["inlier_p"] != ep)[0][:8], np.nonzero(out["inlier_l"] != el)[0][:8])
    assert out["n_inliers_pt"] == ep.sum() and out["n_inliers_ls"] == el.sum(), name
    assert out["n_matched_pt"] == len(ep) and out["n_matched_ls"] == len(el), name
    assert (out["status"], out["path"], out["iters"]) == (ref["status"], ref["path"], ref["iters"]), (name, out["status"], out["path"], out["iters"])
    if ref["status"] == STATUS_OK:
        assert (ref["path"], ref["iters"]) == (5, (1, 1))
        assert np.array_equal(out["T_opt"], occ.DT0), name   # bit for bit: no step was taken
    else:
        assert ref["status"] == STATUS_FEW_AFTER and np.array_equal(out["T_opt"], np.eye(4)), name
    check_pose(out, ref)


@pytest.mark.parametrize("kernel", POSE_KERNELS)
def test_one_cut_on_every_case(hip, oracle, switches, kernel):
    select_kernel(switches, kernel)
    on_solver = on_workers = 0
    for c in CASES:
        name = c["name"]
        rec, _, _, ep, el = occ.built(name)
        ref = occ.oracle_pose(oracle, name)
        assert np.array_equal(ref["inlier_p"], ep) and np.array_equal(ref["inlier_l"], el)
        out = hip.optimize_pose(occ.DT0, occ.CAM, occ.params(c), rec)
        check_case(out, ref, name, ep, el)
        on_solver += 0 < len(el) <= 128
        on_workers += len(el) > 128
    assert on_solver and on_workers   # pose_kernel: key-lines on the solver wave (<= 64 x LPT = 128) and on the worker waves


def test_key_lines_on_the_worker_waves_at_every_size(hip, oracle, switches):
    """STVO_POSE_LOS=0: the latency kernel keeps its key-lines on the worker waves whatever their number"""
    switches({"STVO_POSE_KERNEL": "1", "STVO_POSE_LOS": "0"})
    for c in CASES:
        rec, _, _, ep, el = occ.built(c["name"])
        check_case(hip.optimize_pose(occ.DT0, occ.CAM, occ.params(c), rec), occ.oracle_pose(oracle, c["name"]), c["name"], ep, el)


_EXT = {}


def extended(oracle, name):
    if name not in _EXT:
        c = occ.by_name(name)
        rec = occ.built(name)[0]
        prm = occ.params(c)
        ext = np_pose_terms.evaluate(occ.DT0, occ.CAM, prm.homog_th, rec, True)
        orc = oracle.optimize_functions(occ.DT0, occ.CAM, prm, rec, 1)
        _EXT[name] = dict(ext=ext, orc=orc, dev_orc=np_pose_terms.deviation(orc[0], orc[1], orc[2], ext[0], ext[1], ext[2]))
    return _EXT[name]


def test_robust_evaluation_on_every_case(hip, oracle):
    """stvo_normal_eq(robust = 1) at the initial pose: mad_sigma2 on the residual norms of the inliers, judged by the extended
    statement under the rule of test_single_evaluations_vs_extended_precision — max(floor, 16 x the oracle's own deviation).  (The
    sensitive-* cases miss that bound by five orders of magnitude with a rank that is off by one: test_outlier_cut_host.py.)"""
    bad = []
    for c in CASES:
        name = c["name"]
        ev = extended(oracle, name)
        prm = occ.params(c)
        H, g, e, n = hip.normal_eq(occ.DT0, occ.CAM, prm, occ.built(name)[0], 1)
        xH, xg, xe, xn = ev["ext"][:4]
        d = np_pose_terms.deviation(H, g, e, xH, xg, xe)
        b = pec.bound(ev, 1)
        print(f"robust evaluation {name:40s} dH={d[0]:.2e} dg={d[1]:.2e} de={d[2]:.2e}   oracle {ev['dev_orc'][0]:.2e} {ev['dev_orc'][1]:.2e} {ev['dev_orc'][2]:.2e}")
        if n != xn or n != ev["orc"][3]:
            bad.append((name, "n", n, xn))
        if not np.array_equal(H, H.T):
            bad.append((name, "H is not symmetric"))
        if not all(x <= y for x, y in zip(d, b)):
            bad.append((name, "deviation", d, b))
    assert not bad, bad


@pytest.mark.parametrize("kernel", POSE_KERNELS)
def test_robust_flow_on_every_case(hip, oracle, switches, kernel):
    """optimizePose in the robust mode: robust evaluation (mad_sigma2 on the inliers), the cut, a robust evaluation on the cut set —
    the inlier masks of the second one are sparser than the matched masks"""
    select_kernel(switches, kernel)
    seen = set()
    for c in CASES:
        rec = occ.built(c["name"])[0]
        ref = occ.oracle_pose(oracle, c["name"], mode=1)
        out = hip.optimize_pose(occ.DT0, occ.CAM, occ.params(c, mode=1), rec)
        check_pose(out, ref)
        seen.add((ref["status"], ref["path"]))
    assert (STATUS_OK, 5) in seen


@pytest.mark.parametrize("kernel", POSE_KERNELS)
def test_results_do_not_depend_on_the_order_of_the_calls(hip, switches, kernel):
    """The three histograms are used in rotation (`rot` is carried from one selection to the next: robust evaluation, cut, robust
    evaluation) and cleaned two rounds ahead.  A selection that left scratch dirty for the next one, or anything kept from one call
    to the next, shows as a result that depends on what ran before: every case in both modes, in two orders, on one context —
    identical, bit for bit."""
    select_kernel(switches, kernel)
    rng = np.random.default_rng(7)

    def run(order):
        out = {}
        for k in order:
            c = CASES[k]
            for mode in (0, 1):
                r = hip.optimize_pose(occ.DT0, occ.CAM, occ.params(c, mode=mode), occ.built(c["name"])[0])
                out[(c["name"], mode)] = (r["inlier_p"].tobytes(), r["inlier_l"].tobytes(), r["T"].tobytes(), r["cov"].tobytes(), np.float64(r["err"]).tobytes(),
                                          r["status"], r["path"], r["iters"], r["T_opt"].tobytes(), np.float64(r["err_opt"]).tobytes())
        return out
    a = run(range(len(CASES)))
    b = run(rng.permutation(len(CASES)))
    diff = [k for k in a if a[k] != b[k]]
    assert not diff, diff


BATCH_CASES = ["sensitive-64-65", "duplicate-blocks", "all-equal", "half-equal", "low-7-bits-points", "one-bin-2048", "spread-2048-512-kitti",
               "exponent-only-lines", "all-equal-3-nan",                                       # kitti
               "at-two-sigma", "float-collisions", "gate-count-12", "spread-449-65-euroc",     # euroc
               "threshold-edge-points", "threshold-edge-lines", "threshold-edge-float-mad"]   # edge


@pytest.mark.parametrize("prm_set", ["kitti", "euroc", "edge"])
def test_cases_through_track_batched(hip, oracle, prm_set):
    """Cases as TrackBatch frames (pose_edge_cases.frame_from_records: the f2f match is a known permutation) on the library's own kernel
    choice, with the per-pair assertions of test_mixture_frames_through_track_batched.  The batched entry starts from DT = I and every
    matched feature arrives as an inlier, so the plans are built for that pose; the committed pose is then I, the rejected solution
    (status 3) — the cut and the flags it leaves are the same."""
    import torch
    from stvo_amd.devbatch import TrackBatch
    names = [n for n in BATCH_CASES if occ.by_name(n)["prm"] == prm_set]
    assert len(names) >= 3
    for n in names:
        c = occ.by_name(n)
        assert c["has_points"] and c["has_lines"] and c["min_features"] is None and all(f.inl for f in c["plan_p"] + c["plan_l"])
    prm = occ.params(occ.by_name(names[0]))
    frames = [pec.frame_from_records(occ.built(n, at_identity=True)[0], 900 + i) for i, n in enumerate(names)]
    batch = TrackBatch(frames, max_pts=2048, max_lines=512)
    nnr = 0.75
    hip.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        hip.track_batched(batch, occ.CAM, prm, nnr, nnr, 1)
        torch.cuda.synchronize()
    finally:
        hip.set_stream(None)
    res = batch.results(); mp_all = batch.m12_pts(); ml_all = batch.m12_lines(); ip_all = batch.inlier_pts(); il_all = batch.inlier_lines()
    for b, (n, fr) in enumerate(zip(names, frames)):
        _, _, _, ep, el = occ.built(n, at_identity=True)
        n1, n1l = len(ep), len(el)
        m12, _ = oracle.match(fr["prev_desc"], fr["curr_desc"], nnr)
        m12l, _ = oracle.match(fr["prev_ldesc"], fr["curr_ldesc"], nnr)
        # every record is matched, to the row that carries its own observation: optimizePose sees the planned sets, in the plan's order
        assert np.array_equal(fr["perm"][m12], np.arange(n1)) and np.array_equal(fr["lperm"][m12l], np.arange(n1l))
        ref = occ.oracle_pose(oracle, n, at_identity=True)
        assert np.array_equal(ref["inlier_p"], ep) and np.array_equal(ref["inlier_l"], el), n
        assert (ref["status"], ref["path"], ref["iters"], ref["err"]) == (STATUS_REJECTED, 5, (1, 1), -1.0), n
        assert np.array_equal(mp_all[b, :n1], m12) and np.array_equal(ml_all[b, :n1l], m12l)
        assert res["status"][b] == ref["status"] and res["path"][b] == ref["path"] and tuple(res["iters"][b]) == ref["iters"], n
        assert res["n_matched_pt"][b] == n1 and res["n_matched_ls"][b] == n1l
        assert res["n_inliers_pt"][b] == ep.sum() and res["n_inliers_ls"][b] == el.sum(), n
        assert np.array_equal(ip_all[b, :n1], ep) and np.array_equal(il_all[b, :n1l], el), n
        assert np.array_equal(res["T"][b].reshape(4, 4), np.eye(4)) and res["err"][b] == -1.0 and not np.any(res["cov"][b])


@pytest.mark.parametrize("n_streams", [1, 4])
@pytest.mark.parametrize("kernel", ["4:2", "4:4"])
def test_point_plans_through_the_device_pipeline(oracle, switches, kernel, n_streams):
    """pose2c_kernel (compact records; only the device-resident pipeline reaches it, and "4:2" / "4:4" force it for these few streams):
    point plans as two-frame stereo sequences (outlier_cut_cases.pipeline_sequence), one stream at a time and four side by side.
    The pipeline starts from DT = I, so the committed pose is the rejected one (status 3) — the cut and the flags it writes are the
    plan's: fetch_inliers, counts, status, path and iters against the oracle-driven pipeline (test_pipeline_sequences_carry_the_plan
    shows that its residuals are the planned doubles) and against the stated flags."""
    import pipeline_ref
    from stvo_amd import capi
    from stvo_amd.ctypes_types import match_params
    select_kernel(switches, kernel)
    mp, op = match_params("kitti"), occ.opt_params("kitti", min_error=occ.MIN_ERROR)
    groups = [[n] for n in ("sensitive-64-65", "eighth-key-897")] if n_streams == 1 else [occ.PIPELINE_CASES[:4], occ.PIPELINE_CASES[4:]]
    for names in groups:
        B = len(names)
        seqs = [occ.pipeline_sequence(n) for n in names]
        ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
        dev = capi.Sequences(ctx, B, 1024, 64, occ.CAM, mp, op)
        try:
            dev.enable_fetch(True)
            _, counts0 = dev.push([s[0][0] for s in seqs])
            res, counts = dev.push([s[0][1] for s in seqs])
            sched = dev.last_schedule()
            assert sched["pose_kernel"] == capi.SCHED_POSE_BATCH and sched["pose_waves"] == int(kernel[-1])
            ip, il = dev.fetch_inliers()
            for b, (name, (frames, r, keep)) in enumerate(zip(names, seqs)):
                n = len(r)
                o = pipeline_ref.run_sequence(oracle, frames, occ.CAM, mp, op)[0]
                assert counts0[b, 0] == counts[b, 0] == n and counts[b, 1] == 0, name
                assert (res[b]["status"], res[b]["path"], tuple(res[b]["iters"])) == (o["status"], o["path"], o["iters"]) == (STATUS_REJECTED, 5, (1, 1)), name
                assert res[b]["n_matched_pt"] == o["n_matched_pt"] == n and res[b]["n_matched_ls"] == 0
                assert res[b]["n_inliers_pt"] == o["n_inliers_pt"] == keep.sum(), name
                assert np.array_equal(ip[b, :n], o["inlier_p"]) and np.array_equal(o["inlier_p"], keep.astype(np.int32)), (name, np.nonzero(ip[b, :n] != keep)[0][:8])
                assert np.all(ip[b, n:] == -1)
                assert np.array_equal(res[b]["T"].reshape(4, 4), np.eye(4)) and res[b]["err"] == -1.0
        finally:
            dev.close()
            ctx.close()
