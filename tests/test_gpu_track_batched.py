"""GPU parity of the batched, device-resident path (f2f match + optimizePose for B frame pairs)
against per-frame oracle runs, at BASELINE config-2 size (2000 ORB rows per frame)."""
import numpy as np
import pytest

import np_model
from stvo_amd import synth
from stvo_amd.ctypes_types import opt_params

pytestmark = pytest.mark.gpu
CAM = synth.KITTI_CAM


def oracle_track(oracle, fr, prm, nnr):
    m12, _ = oracle.match(fr["prev_desc"], fr["curr_desc"], nnr)
    sel = np.nonzero(m12 >= 0)[0]
    z3 = np.zeros((0, 3)); z2 = np.zeros((0, 2))
    rec = dict(P=fr["prev_P"][sel], pl_obs=fr["curr_pl"][m12[sel]], sigma2p=fr["prev_sigma2"][sel],
               inlier_p=np.ones(len(sel), np.int32), sP=z3, eP=z3, le_obs=z3, spl=z2, epl=z2, sigma2l=np.zeros(0),
               inlier_l=np.zeros(0, np.int32))
    out = oracle.optimize_pose(np.eye(4), CAM, prm, rec)
    return m12, sel, out


def test_track_batched_points_config2(hip, oracle):
    import torch
    from stvo_amd.devbatch import TrackBatch
    B = 12
    frames = [synth.make_f2f_points(synth.frame_seed(0, k), n=2000 - 37 * (k % 3)) for k in range(B)]
    batch = TrackBatch(frames, max_pts=2048)
    prm = opt_params("kitti", has_lines=0)
    hip.set_stream(torch.cuda.current_stream().cuda_stream)
    hip.track_batched(batch, CAM, prm, 0.75, 0.75, 1)
    torch.cuda.synchronize()
    res = batch.results(); m12_all = batch.m12_pts(); inl_all = batch.inlier_pts()
    for b, fr in enumerate(frames):
        m12, sel, ref = oracle_track(oracle, fr, prm, 0.75)
        n1 = len(fr["prev_P"])
        assert np.array_equal(m12_all[b, :n1], m12)
        assert res["status"][b] == ref["status"] and res["path"][b] == ref["path"]
        assert tuple(res["iters"][b]) == ref["iters"]
        assert res["n_matched_pt"][b] == len(sel) and res["n_inliers_pt"][b] == ref["n_inliers_pt"]
        exp_inl = -np.ones(n1, np.int32); exp_inl[sel] = ref["inlier_p"]
        assert np.array_equal(inl_all[b, :n1], exp_inl)
        T = res["T"][b].reshape(4, 4)
        assert np_model.rot_angle(T[:3, :3], ref["T"][:3, :3]) < 1e-4
        assert np.linalg.norm(T[:3, 3] - ref["T"][:3, 3]) < 1e-3
        assert np.allclose(T, ref["T"], atol=1e-8)
        assert np.isclose(res["err"][b], ref["err"], rtol=1e-8)
        # and the estimate is the true motion (stored inverted) up to noise
        Tt = np.linalg.inv(fr["T_true"])
        assert np_model.rot_angle(T[:3, :3], Tt[:3, :3]) < 3e-3 and np.linalg.norm(T[:3, 3] - Tt[:3, 3]) < 0.05
    hip.set_stream(None)


def test_overlap_mode_gives_identical_results(oracle):
    """stvo_ctx_set_overlap: pose kernel on the context's second stream, concurrent with the next call's
    matching kernels.  Back-to-back calls on two different batches must reproduce the in-order results."""
    import torch
    from stvo_amd import capi
    from stvo_amd.devbatch import TrackBatch
    prm = opt_params("kitti", has_lines=0)
    fa = [synth.make_f2f_points(synth.frame_seed(3, k), n=900) for k in range(40)]
    fb = [synth.make_f2f_points(synth.frame_seed(4, k), n=1100) for k in range(40)]
    out = {}
    for overlap in (0, 1):
        ctx = capi.Context(device_id=0, max_rows=2048, max_batch=64)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_overlap(overlap)
        ba, bb = TrackBatch(fa, max_pts=2048), TrackBatch(fb, max_pts=2048)
        for _ in range(3):  # a, b, a, b, ... : every hazard class (same buffers two calls apart, scratch reuse)
            ctx.track_batched(ba, CAM, prm, 0.75, 0.75, 1)
            ctx.track_batched(bb, CAM, prm, 0.75, 0.75, 1)
            ctx.track_batched(bb, CAM, prm, 0.75, 0.75, 1)
        ctx.synchronize()
        torch.cuda.synchronize()
        out[overlap] = (ba.results().copy(), bb.results().copy(), ba.m12_pts().copy(), bb.m12_pts().copy(),
                        ba.inlier_pts().copy(), bb.inlier_pts().copy())
        ctx.close()
    for x, y in zip(out[0], out[1]):
        assert x.tobytes() == y.tobytes()
    assert (out[1][0]["status"] == 0).all() and (out[1][1]["status"] == 0).all()


def oracle_track_pl(oracle, fr, prm, nnr_p, nnr_l):
    m12, _ = oracle.match(fr["prev_desc"], fr["curr_desc"], nnr_p)
    sel = np.nonzero(m12 >= 0)[0]
    m12l, _ = oracle.match(fr["prev_ldesc"], fr["curr_ldesc"], nnr_l)
    sl = np.nonzero(m12l >= 0)[0]
    rec = dict(P=fr["prev_P"][sel], pl_obs=fr["curr_pl"][m12[sel]], sigma2p=fr["prev_sigma2"][sel],
               inlier_p=np.ones(len(sel), np.int32), sP=fr["prev_sP"][sl], eP=fr["prev_eP"][sl],
               le_obs=fr["curr_le"][m12l[sl]], spl=fr["prev_spl"][sl], epl=fr["prev_epl"][sl],
               sigma2l=fr["prev_sigma2l"][sl], inlier_l=np.ones(len(sl), np.int32))
    return m12, sel, m12l, sl, oracle.optimize_pose(np.eye(4), CAM, prm, rec)


@pytest.mark.parametrize("preset,mode,nl,nnr", [("kitti", 0, 100, 0.75), ("euroc", 2, 300, 0.9), ("euroc", 1, 300, 0.9)])
def test_track_batched_points_and_lines(hip, oracle, preset, mode, nl, nnr):
    """BASELINE configs[2] / [3] shapes through the batched device path: f2f match of points AND lines,
    on-device gather of both record kinds, GN / LM / robust GN pose."""
    import torch
    from stvo_amd.devbatch import TrackBatch
    B = 6
    npts = 2000 if preset == "kitti" else 800
    frames = [synth.make_f2f_points_lines(synth.frame_seed(2, k), n=npts - 13 * k, n_lines=nl - 3 * k,
                                          octave_probs=None if preset == "kitti" else [.5, .25, .15, .1],
                                          outlier_frac=0.15 if preset == "kitti" else 0.4) for k in range(B)]
    batch = TrackBatch(frames, max_pts=2048, max_lines=320)
    prm = opt_params(preset, mode=mode)
    hip.set_stream(torch.cuda.current_stream().cuda_stream)
    hip.track_batched(batch, CAM, prm, nnr, nnr, 1)
    torch.cuda.synchronize()
    res = batch.results(); mp_all = batch.m12_pts(); ml_all = batch.m12_lines(); ip_all = batch.inlier_pts(); il_all = batch.inlier_lines()
    for b, fr in enumerate(frames):
        m12, sel, m12l, sl, ref = oracle_track_pl(oracle, fr, prm, nnr, nnr)
        n1, n1l = len(fr["prev_P"]), len(fr["prev_sP"])
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
    hip.set_stream(None)


def test_track_batched_ragged_sizes(hip, oracle):
    """Frame pairs of very different sizes in one batch (tail tiles, empty segments, a pair below min_features), run twice
    with the order reversed so that stale scratch of a larger problem (top-2 partials, column claims, verdicts) would show."""
    import torch
    from stvo_amd.devbatch import TrackBatch
    sizes = [2000, 1333, 640, 257, 65, 12, 9, 1999, 300]
    frames = [synth.make_f2f_points(synth.frame_seed(3, k), n=n) for k, n in enumerate(sizes)]
    prm = opt_params("kitti", has_lines=0)
    hip.set_stream(torch.cuda.current_stream().cuda_stream)
    for order in (list(range(len(frames))), list(reversed(range(len(frames))))):
        fs = [frames[i] for i in order]
        batch = TrackBatch(fs, max_pts=2048)
        hip.track_batched(batch, CAM, prm, 0.75, 0.75, 1)
        torch.cuda.synchronize()
        res = batch.results(); m12_all = batch.m12_pts(); inl_all = batch.inlier_pts()
        for b, fr in enumerate(fs):
            m12, sel, ref = oracle_track(oracle, fr, prm, 0.75)
            n1 = len(fr["prev_P"])
            assert np.array_equal(m12_all[b, :n1], m12), (b, n1)
            assert res["status"][b] == ref["status"] and res["path"][b] == ref["path"], (b, n1)
            assert tuple(res["iters"][b]) == ref["iters"]
            assert res["n_matched_pt"][b] == len(sel) and res["n_inliers_pt"][b] == ref["n_inliers_pt"]
            if ref["status"] == 0:
                assert np.allclose(res["T"][b].reshape(4, 4), ref["T"], atol=1e-8)
    hip.set_stream(None)


@pytest.mark.parametrize("preset,mode,nnr", [("kitti", 0, 0.75), ("euroc", 2, 0.9)])
def test_track_batched_more_than_two_pairs_per_cu(oracle, preset, mode, nnr):
    """More than two frame pairs per CU through the batched entry: the batch size at which launch_pose2p takes TWO waves per pair by
    default — here pose2p_kernel<2>, the general-form kernel no other test reaches without a switch — and at which the forward scan
    K1m runs with a batch that is no multiple of the eight XCDs and two query tiles per frame (its "partial tiles last" remap).
    Every pair against the oracle: match indices of points and lines bit for bit, inlier masks, status, path, iterations, pose."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from stvo_amd import capi
    from stvo_amd.devbatch import TrackBatch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * cus + 5
    assert B > 256 and B > 2 * cus and B % 8 != 0   # batch pose kernel, two waves per pair, a partly empty last group of eight
    frames = [synth.make_f2f_points_lines(synth.frame_seed(11, k), n=140 + 40 * (k % 7), n_lines=10 + 6 * (k % 6), outlier_frac=0.15)
              for k in range(B)]
    assert max(max(len(f["prev_P"]), len(f["curr_pl"])) for f in frames) > 256   # two 256-row tiles in some frames
    prm = opt_params(preset, mode=mode)
    with ThreadPoolExecutor(16) as ex:   # the oracle's C functions run outside the GIL
        refs = list(ex.map(lambda fr: oracle_track_pl(oracle, fr, prm, nnr, nnr), frames))
    ctx = capi.Context(device_id=0, max_rows=512, max_batch=B)
    try:
        batch = TrackBatch(frames, max_pts=512, max_lines=64)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.track_batched(batch, CAM, prm, nnr, nnr, 1)
        torch.cuda.synchronize()
        res = batch.results(); mp_all = batch.m12_pts(); ml_all = batch.m12_lines(); ip_all = batch.inlier_pts(); il_all = batch.inlier_lines()
    finally:
        ctx.close()
    for b, (fr, (m12, sel, m12l, sl, ref)) in enumerate(zip(frames, refs)):
        n1, n1l = len(fr["prev_P"]), len(fr["prev_sP"])
        assert np.array_equal(mp_all[b, :n1], m12) and np.array_equal(ml_all[b, :n1l], m12l), b
        assert res["status"][b] == ref["status"] and res["path"][b] == ref["path"] and tuple(res["iters"][b]) == ref["iters"], b
        assert res["n_matched_pt"][b] == len(sel) and res["n_matched_ls"][b] == len(sl), b
        assert res["n_inliers_pt"][b] == ref["n_inliers_pt"] and res["n_inliers_ls"][b] == ref["n_inliers_ls"], b
        e = -np.ones(n1, np.int32); e[sel] = ref["inlier_p"]
        assert np.array_equal(ip_all[b, :n1], e), b
        e = -np.ones(n1l, np.int32); e[sl] = ref["inlier_l"]
        assert np.array_equal(il_all[b, :n1l], e), b
        T = res["T"][b].reshape(4, 4)
        assert np_model.rot_angle(T[:3, :3], ref["T"][:3, :3]) < 1e-4 and np.linalg.norm(T[:3, 3] - ref["T"][:3, 3]) < 1e-3, b
        assert np.allclose(T, ref["T"], atol=1e-8) and np.isclose(res["err"][b], ref["err"], rtol=1e-8), b


@pytest.mark.parametrize("max_pts,max_lines", [(2048, 512), (64, 0)], ids=["full-lds", "64-points"])
def test_latency_kernel_forced_past_256_pairs_equals_single_pair_runs(switches, max_pts, max_lines):
    """STVO_POSE_KERNEL=1 at 257 frame pairs, the first batch size the latency kernel does not take by itself: pose_kernel.hip is
    ONE kernel at every batch size — one workgroup per pair, a fixed summation order, dynamic LDS sized by the capacities alone
    (all 152 KB of it at 2048 points / 512 lines) — so every pair of the batch must come out bit for bit as the same pair run
    alone under the same switch.  A difference means that a launch parameter depends on the batch size."""
    import torch
    from stvo_amd import capi
    from stvo_amd.devbatch import TrackBatch
    switches({"STVO_POSE_KERNEL": "1"})
    B = 257
    if max_lines:   # about 300 points and 40 lines per pair
        frames = [synth.make_f2f_points_lines(synth.frame_seed(12, k), n=300 - 7 * (k % 5), n_lines=40 - k % 4, outlier_frac=0.15)
                  for k in range(B)]
        prm = opt_params("kitti")
    else:           # up to the capacity of 64 points, down to a pair below min_features
        frames = [synth.make_f2f_points(synth.frame_seed(13, k), n=(64, 57, 40, 23, 9)[k % 5]) for k in range(B)]
        prm = opt_params("kitti", has_lines=0)

    def outputs(batch, n):
        res = batch.results()
        out = [res[name][:n].copy() for name in ("status", "path", "iters", "n_matched_pt", "n_matched_ls", "n_inliers_pt", "n_inliers_ls",
                                                  "T", "cov", "err")]
        out.append(batch.inlier_pts()[:n].copy())
        if max_lines:
            out.append(batch.inlier_lines()[:n].copy())
        return out

    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        batch = TrackBatch(frames, max_pts=max_pts, max_lines=max_lines)
        ctx.track_batched(batch, CAM, prm, 0.75, 0.75, 1)
        torch.cuda.synchronize()
        together = outputs(batch, B)
        alone = []
        for fr in frames:
            one = TrackBatch([fr], max_pts=max_pts, max_lines=max_lines)
            ctx.track_batched(one, CAM, prm, 0.75, 0.75, 1)
            torch.cuda.synchronize()
            alone.append(outputs(one, 1))
    finally:
        ctx.close()
    print("status counts", np.bincount(together[0], minlength=4), "paths", sorted(set(together[1].tolist())))
    assert (together[0] == 0).any()   # the comparison is not one of empty results
    for b in range(B):
        for x, y in zip(together, alone[b]):
            assert x[b].tobytes() == y[0].tobytes(), b
