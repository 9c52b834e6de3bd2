"""The record arena of the batch pose kernels belongs to the context that launches them (one grow-only block per stream it launches
on: stvo-pl_amd/csrc/ctx_internal.h, pose_scratch.h).  Batch kernel forced (STVO_POSE_KERNEL=4), two waves per pair
(STVO_POSE2P_NW=2: 128 threads), 1024 points per pair — every thread owns eight record ordinals, the highest of which do not fit
its share of the LDS and live in the arena — and 130 key-lines, which all live there, two threads owning a second one.  The
reference of every run is the same batch run alone in a fresh context: results, inlier rows and iterations bit for bit."""
import numpy as np
import pytest

from stvo_amd import synth
from stvo_amd.ctypes_types import opt_params

pytestmark = pytest.mark.gpu
CAM = synth.KITTI_CAM
N_PTS, N_LINES = 1024, 130
SWITCHES = {"STVO_POSE_KERNEL": "4", "STVO_POSE2P_NW": "2"}


def frame(k):
    """Frame pair k as devbatch.TrackBatch takes it: associated records (prev record i belongs with curr record i) and descriptors
    that the f2f matcher associates the same way — every row its own random 256 bits, equal in both frames."""
    rec = synth.make_matched_records(synth.frame_seed(21, k), n_pts=N_PTS, n_lines=N_LINES)
    rng = np.random.default_rng(1000 + k)
    pd, ld = synth.random_desc(rng, N_PTS), synth.random_desc(rng, N_LINES)
    return dict(prev_P=rec["P"], prev_sigma2=rec["sigma2p"], curr_pl=rec["pl_obs"], prev_desc=pd, curr_desc=pd,
                prev_sP=rec["sP"], prev_eP=rec["eP"], prev_spl=rec["spl"], prev_epl=rec["epl"], prev_sigma2l=rec["sigma2l"],
                curr_le=rec["le_obs"], prev_ldesc=ld, curr_ldesc=ld)


_frames, _alone = {}, {}


def make_batch(B):
    from stvo_amd.devbatch import TrackBatch
    for k in range(B):
        if k not in _frames:
            _frames[k] = frame(k)
    return TrackBatch([_frames[k] for k in range(B)], max_pts=N_PTS, max_lines=N_LINES)


def outputs(batch):
    res = batch.results()
    return res.tobytes(), res["iters"].copy(), batch.inlier_pts().copy(), batch.inlier_lines().copy()


def same(got, want):
    return got[0] == want[0] and all(np.array_equal(x, y) for x, y in zip(got[1:], want[1:]))


def new_context():
    import torch
    from stvo_amd import capi
    ctx = capi.Context(device_id=0, max_rows=N_PTS, max_batch=8)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return ctx


def run(ctx, B):
    import torch
    batch = make_batch(B)
    ctx.optimize_pose_batched(batch, CAM, opt_params("kitti"))
    torch.cuda.synchronize()
    return outputs(batch)


def alone(B):
    """the first B frame pairs in a fresh context that runs nothing else (computed once per B, under the same switches)"""
    if B not in _alone:
        ctx = new_context()
        try:
            _alone[B] = run(ctx, B)
        finally:
            ctx.close()
        res = np.frombuffer(_alone[B][0], dtype=make_batch(B).results().dtype)
        assert (res["status"] == 0).all() and (res["n_matched_pt"] == N_PTS).all() and (res["n_matched_ls"] == N_LINES).all()
        assert (res["n_inliers_pt"] < N_PTS).all() and (_alone[B][1] > 0).any()   # outliers were cut: the records were read back
    return _alone[B]


def test_two_contexts_on_one_stream_each_hold_their_own_arena(switches):
    """X and Y on torch's current stream: X runs 3 pairs, Y runs 5, X is closed, Y runs its 5 again — closing X frees nothing of Y's"""
    switches(SWITCHES)
    want = alone(5)
    x, y = new_context(), new_context()
    try:
        assert same(run(x, 3), alone(3))
        first = run(y, 5)
        x.close()
        second = run(y, 5)
    finally:
        x.close()
        y.close()
    assert same(first, want) and same(second, want)


def test_arena_growth_replaces_the_block(switches):
    """one context: 2 pairs, then 6 (the block is replaced by a larger one), then 2 again in the larger block"""
    switches(SWITCHES)
    ctx = new_context()
    try:
        got = [run(ctx, B) for B in (2, 6, 2)]
    finally:
        ctx.close()
    for g, B in zip(got, (2, 6, 2)):
        assert same(g, alone(B)), B


def test_second_stream_has_its_own_arena(switches):
    """stvo_ctx_set_overlap(1): the pose kernels run on the context's second stream, in that stream's block — two batches of 3 and 5
    pairs tracked back to back come out as with set_overlap(0) (and, the matcher associating row i with row i, as the pose alone)"""
    import torch
    switches(SWITCHES)
    prm = opt_params("kitti")
    out = {}
    for overlap in (0, 1):
        ctx = new_context()
        try:
            ctx.set_overlap(overlap)
            ba, bb = make_batch(3), make_batch(5)
            ctx.track_batched(ba, CAM, prm, 0.75, 0.75, 1)
            ctx.track_batched(bb, CAM, prm, 0.75, 0.75, 1)
            ctx.synchronize()
            torch.cuda.synchronize()
            out[overlap] = (outputs(ba), outputs(bb), ba.m12_pts().copy(), bb.m12_pts().copy(), ba.m12_lines().copy(), bb.m12_lines().copy())
        finally:
            ctx.close()
    for k in (0, 1):
        assert same(out[1][k], out[0][k]), k
    for k in (2, 3, 4, 5):
        assert np.array_equal(out[1][k], out[0][k]) and (out[1][k] == np.arange(out[1][k].shape[1])).all(), k
    assert same(out[1][0], alone(3)) and same(out[1][1], alone(5))
