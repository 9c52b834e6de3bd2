"""GPU: the control flow of csrc/pose_block.h — the three optimisers, their stop rules, isGoodSolution with its certificate shortcut,
the optimizePose state machine and the commit — on the planned cases of tests/pose_flow_cases.py, in every pose kernel and by every
way into them.  Each case states its course (status, path, iters); tests/test_pose_flow_host.py shows on the CPU that the extended
statement (tests/np_pose_flow.py), the oracle and np_model take that course and that every decision on the way has at least 64 x the
room the oracle's own rounding needs.  Here the kernels must take it too, and T_opt, T, cov, cov_eig and err must agree with the
extended statement within max(the floors of test_gpu_pose.check_pose, 16 x the oracle's deviation in the same case).

  direct          stvo_optimize_pose, every case, every entry of POSE_KERNELS; twice in two orders on one context, bit for bit
  track_batched   the cases that start at I with every feature an inlier, as TrackBatch frames (the library's own kernel choice)
  device pipeline the point-only cases as two-frame stereo sequences through capi.Sequences: "4:2" / "4:4" (pose2c_kernel, one stream
                  and four) and one stream on the library's own choice (pose_kernel with the lazy_eig commit: cov_eig of a certified
                  covariance is filled in by stvo_seq_read on the host, of any other one by the kernel)"""
import numpy as np
import pytest

import np_pose_flow as npf
import pose_edge_cases as pec
import pose_flow_cases as pfc
from test_gpu_pose import check_pose
from test_gpu_pose_edges import POSE_KERNELS, select_kernel

pytestmark = pytest.mark.gpu
CASES = pfc.CASES   # built on first use
# |got - statement| <= atol + rtol |statement| elementwise: what check_pose grants against the oracle (np.allclose / np.isclose)
FLOORS = dict(T_opt=(1e-8, 1e-5), T=(1e-8, 1e-5), cov=(1e-12, 1e-6), cov_eig=(1e-13, 1e-6), err=(1e-8, 1e-8))
FACTOR = 16.0


def check_against_statement(got, name, dev):
    """got: dict of the compared fields (doubles); dev: pose_flow_cases.oracle_deviation of the case"""
    want = pfc.by_name(name)["out"]
    for k, (atol, rtol) in FLOORS.items():
        x = np.asarray(want[k], dtype=npf.LD).reshape(-1)
        a = np.asarray(got[k], np.float64).reshape(-1).astype(npf.LD)
        tol = np.maximum(atol + rtol * np.abs(x), FACTOR * dev[k] * np.max(np.abs(x)))
        assert np.all(np.isfinite(a.astype(np.float64))) and np.all(np.abs(a - x) <= tol), (name, k, float(np.max(np.abs(a - x))), float(np.max(tol)))


def check_course(got, name):
    c = pfc.by_name(name)
    assert (got["status"], got["path"], tuple(got["iters"])) == pfc.PLAN[name][0], (name, got["status"], got["path"], got["iters"])
    assert got["n_inliers_pt"] == c["out"]["n_inliers_pt"] and got["n_inliers_ls"] == c["out"]["n_inliers_ls"], name
    assert got["n_matched_pt"] == c["out"]["n_matched_pt"] and got["n_matched_ls"] == c["out"]["n_matched_ls"], name


@pytest.mark.parametrize("kernel", POSE_KERNELS)
def test_every_case_takes_its_course(hip, oracle, switches, kernel):
    select_kernel(switches, kernel)
    for c in CASES:
        name = c["name"]
        out = hip.optimize_pose(c["DT0"], pfc.cam_of(c), pfc.params(c), c["rec"])
        check_course(out, name)
        assert np.array_equal(out["inlier_p"], c["out"]["inlier_p"]) and np.array_equal(out["inlier_l"], c["out"]["inlier_l"]), name
        check_pose(out, pfc.oracle_pose(oracle, name))
        check_against_statement(out, name, pfc.oracle_deviation(oracle, name))
        if "almost-identity" in c["tags"] or "lad-below" in c["tags"]:   # no step taken / the entry pose restored: the pose itself
            assert np.array_equal(out["T_opt"], c["DT0"]), name
        if "lad-below" in c["tags"]:
            assert out["err_opt"] == -1.0 and out["status"] == 3


@pytest.mark.parametrize("kernel", POSE_KERNELS)
def test_results_do_not_depend_on_the_order_of_the_calls(hip, switches, kernel):
    """`good`, `lambda`, `err_prev`, the saved poses and the action word live in LDS from one stage to the next: anything that a
    call inherits from the one before shows as a result that depends on the order.  Every case twice, in two orders, on one
    context: identical bit for bit."""
    select_kernel(switches, kernel)

    def run(order):
        out = {}
        for k in order:
            c = CASES[k]
            r = hip.optimize_pose(c["DT0"], pfc.cam_of(c), pfc.params(c), c["rec"])
            out[c["name"]] = (r["inlier_p"].tobytes(), r["inlier_l"].tobytes(), r["T"].tobytes(), r["cov"].tobytes(), r["cov_eig"].tobytes(),
                              np.float64(r["err"]).tobytes(), r["status"], r["path"], r["iters"], r["T_opt"].tobytes(), np.float64(r["err_opt"]).tobytes())
        return out
    a = run(range(len(CASES)))
    b = run(np.random.default_rng(11).permutation(len(CASES)))
    diff = [k for k in a if a[k] != b[k]]
    assert not diff, diff


def test_cases_through_track_batched(hip, oracle):
    """One TrackBatch frame per case (pose_edge_cases.frame_from_records: the f2f match is a known permutation, so optimizePose sees the
    records of the case in their order), each with its own parameters and camera."""
    import torch
    from stvo_amd.devbatch import TrackBatch
    names = pfc.BATCH_CASES + pfc.pipeline_names()
    nnr = 0.75
    for i, name in enumerate(names):
        c = pfc.by_name(name)
        assert pfc.batchable(c), name
        fr = pec.frame_from_records(c["rec"], 1300 + i)
        batch = TrackBatch([fr], max_pts=2048, max_lines=512)
        hip.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            hip.track_batched(batch, pfc.cam_of(c), pfc.params(c), nnr, nnr, 1)
            torch.cuda.synchronize()
        finally:
            hip.set_stream(None)
        res = batch.results(); mp_all = batch.m12_pts(); ml_all = batch.m12_lines(); ip_all = batch.inlier_pts(); il_all = batch.inlier_lines()
        n1, n1l = len(c["rec"]["sigma2p"]), len(c["rec"]["sigma2l"])
        m12, _ = oracle.match(fr["prev_desc"], fr["curr_desc"], nnr)
        assert np.array_equal(fr["perm"][m12], np.arange(n1)) and np.array_equal(mp_all[0, :n1], m12), name
        if n1l:
            m12l, _ = oracle.match(fr["prev_ldesc"], fr["curr_ldesc"], nnr)
            assert np.array_equal(fr["lperm"][m12l], np.arange(n1l)) and np.array_equal(ml_all[0, :n1l], m12l), name
        got = {k: res[k][0] for k in ("status", "path", "n_matched_pt", "n_matched_ls", "n_inliers_pt", "n_inliers_ls", "err")}
        got.update(iters=tuple(int(v) for v in res["iters"][0]), T=res["T"][0].reshape(4, 4), T_opt=res["T_opt"][0].reshape(4, 4), cov=res["cov"][0].reshape(6, 6), cov_eig=res["cov_eig"][0])
        got.update(inlier_p=ip_all[0, :n1], inlier_l=il_all[0, :n1l])
        check_course(got, name)
        assert np.array_equal(got["inlier_p"], c["out"]["inlier_p"]) and np.array_equal(got["inlier_l"], c["out"]["inlier_l"]), name
        check_pose(got, pfc.oracle_pose(oracle, name))
        check_against_statement(got, name, pfc.oracle_deviation(oracle, name))


def _groups(n_streams):
    """the point-only cases in runs of n_streams that share their optimiser parameters (one Sequences object has one set)"""
    by_prm = {}
    for n in pfc.pipeline_names():
        c = pfc.by_name(n)
        by_prm.setdefault((c["preset"], tuple(sorted(c["prm"].items()))), []).append(n)
    if n_streams == 1:
        return [[n] for n in pfc.pipeline_names()]
    big = [g for g in by_prm.values() if len(g) >= n_streams]
    return [g[:n_streams] for g in big] + [g[-n_streams:] for g in big if len(g) > n_streams]


def run_pipeline(ctx, oracle, names, expect_kernel, expect_waves):
    from stvo_amd import capi
    from stvo_amd.ctypes_types import match_params
    B = len(names)
    cs = [pfc.by_name(n) for n in names]
    seqs = [pfc.pipeline_frames(n) for n in names]
    cams = [pfc.cam_of(c) for c in cs]
    dev = capi.Sequences(ctx, B, 1024, 64, cams[0] if B == 1 else cams, match_params("kitti"), pfc.params(cs[0]))
    try:
        dev.enable_fetch(True)
        dev.push([s[0] for s in seqs])
        res, counts = dev.push([s[1] for s in seqs])
        sched = dev.last_schedule()
        assert sched["pose_kernel"] == expect_kernel and sched["pose_waves"] == expect_waves, sched
        ip, _ = dev.fetch_inliers()
        for b, (name, c) in enumerate(zip(names, cs)):
            n = len(c["rec"]["sigma2p"])
            assert counts[b, 0] == n and counts[b, 1] == 0, name
            got = {k: res[b][k] for k in ("status", "path", "n_matched_pt", "n_matched_ls", "n_inliers_pt", "n_inliers_ls", "err")}
            got.update(iters=tuple(int(v) for v in res[b]["iters"]), inlier_p=ip[b, :n], inlier_l=np.zeros(0, np.int32), T=res[b]["T"].reshape(4, 4), T_opt=res[b]["T_opt"].reshape(4, 4), cov=res[b]["cov"].reshape(6, 6), cov_eig=res[b]["cov_eig"])
            check_course(got, name)   # (path as planned: the library's PATH_EIG_PENDING flag never leaves it)
            assert np.array_equal(ip[b, :n], c["out"]["inlier_p"]) and np.all(ip[b, n:] == -1), name
            check_pose(got, pfc.oracle_pose(oracle, name))
            check_against_statement(got, name, pfc.oracle_deviation(oracle, name))
            regime = c["trace"]["verdicts"][-1]["regime"]
            if regime == "C":
                assert got["status"] == 3 and not np.any(got["cov_eig"]) and np.array_equal(got["T"], np.eye(4)), name
            elif got["status"] == 0:   # regime A: the certificate commits and the host fills cov_eig in; B: the kernel's eigenvalues
                assert np.all(got["cov_eig"] > 0) and np.all(np.diff(got["cov_eig"]) >= 0), (name, regime)
    finally:
        dev.close()


@pytest.fixture
def pipeline_ctx():
    from stvo_amd import capi
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=4)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n_streams", [1, 4])
@pytest.mark.parametrize("kernel", ["4:2", "4:4"])
def test_point_cases_through_the_device_pipeline(pipeline_ctx, oracle, switches, kernel, n_streams):
    """pose2c_kernel (compact records; only the device-resident pipeline reaches it, and "4:2" / "4:4" force it for these few streams)"""
    from stvo_amd import capi
    select_kernel(switches, kernel)
    groups = _groups(n_streams)
    assert groups
    for names in groups:
        run_pipeline(pipeline_ctx, oracle, names, capi.SCHED_POSE_BATCH, int(kernel[-1]))


def test_point_cases_through_the_lazy_eig_commit(pipeline_ctx, oracle):
    """One stream on the library's own choice: pose_kernel, which commits on the certificate alone where it holds (regime A) and leaves
    cov_eig to stvo_seq_read; regimes B and C take the eigen-decomposition in the kernel.
    What this can and cannot show: last_schedule() names the kernel, not the plan's lazy_eig, and PATH_EIG_PENDING never leaves the
    library, so a host-filled cov_eig looks like a device-computed one.  That one stream with fetch on plans lazy_eig is held on the
    host by tests/test_step_plan_host.py; here the verdict (certificate against eigenvalues at 1e-3 .. 1e-2 beside their edges), the
    committed values and cov_eig against the statement are judged whichever side computes them."""
    from stvo_amd import capi
    names = pfc.pipeline_names()
    commits = {(pfc.by_name(n)["trace"]["verdicts"][-1]["regime"], pfc.by_name(n)["out"]["status"]) for n in names}
    assert commits >= {("A", 0), ("B", 0), ("C", 3)}
    for name in names:
        run_pipeline(pipeline_ctx, oracle, [name], capi.SCHED_POSE_LATENCY, 0)
