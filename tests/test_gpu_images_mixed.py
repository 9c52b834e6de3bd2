"""Images -> poses with one camera AND image size per stream (ImagePipeline(cam=[B dicts])), two sets of three streams:
  small  320 x 128, 316 x 124 and 256 x 128 in slots of 320 x 128, then a RESTART of stream 1 into 300 x 120.  At these sizes the CPU chain
         rejects EVERY pose of every stream, the restarted one included (status 3, T = identity: the KITTI calibration leaves the optimiser
         nothing to hold on to), so this set checks counts, verdicts, iteration counts and inliers — no committed pose;
  large  the same pattern at sizes where the chain commits: 640 x 240, 636 x 236 and 512 x 240 in slots of 640 x 240, then a RESTART of
         stream 1 into 600 x 232.  The scene seeds are picked on the CPU, with the oracle, so that the chain commits and every committed
         translation lies in the range tests/test_gpu_images.py asks of this generator; the test asserts both.
Poses and counts are judged against the CPU chain (the ORB oracle on every image at its own size, then the oracle-driven pipeline under the
stream's own camera) exactly as tests/test_gpu_images.py judges them; every stream is byte-equal to a uniform ImagePipeline of its own
size fed three copies of it; the RESTART goes through push_images(control=, cams=) and is judged the same way."""
import numpy as np
import pytest

import np_model
import pipeline_ref
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_images import oracle_frames

pytestmark = pytest.mark.gpu
B, NF = 3, 4
RUN, RESTART = 0, 1
# per set: the three sizes, the size stream 1 restarts into (under another calibration), (seed, shift_per_disp) of the three scenes and of
# the new one, and how many poses the CPU chain must commit (0: it commits none at these sizes)
SETS = {"small": dict(sizes=[(320, 128), (316, 124), (256, 128)], new=(300, 120), scenes=[(70, 0.30), (71, 0.26), (72, 0.22)], new_scene=(77, 0.28),
                      committed=0),
        "large": dict(sizes=[(640, 240), (636, 236), (512, 240)], new=(600, 232), scenes=[(76, 0.30), (71, 0.26), (74, 0.22)], new_scene=(74, 0.28),
                      committed=10)}
SIZES = SETS["small"]["sizes"]
CAMS = [dict(synth.KITTI_CAM, width=w, height=h) for w, h in SIZES]
NEW_CAM = dict(synth.KITTI03_CAM, width=300, height=120)

_seqs = {}


def sequence(scene, cam, n):
    key = (scene, cam["width"], cam["height"], n)
    if key not in _seqs:
        _seqs[key] = synth.make_stereo_image_sequence(scene[0], n, cam, shift_per_disp=scene[1])
    return _seqs[key]


def judge(res, counts, o, where):
    """the per-frame assertions of tests/test_gpu_images.py::test_images_to_poses_two_streams"""
    assert counts[0] == o["n_stereo_pt"] and res["n_matched_pt"] == o["n_matched_pt"], (where, counts, o["n_stereo_pt"])
    assert res["status"] == o["status"] and res["path"] == o["path"] and tuple(res["iters"]) == o["iters"], where
    assert res["n_inliers_pt"] == o["n_inliers_pt"], where
    T = res["T"].reshape(4, 4)
    assert np_model.rot_angle(T[:3, :3], o["T"][:3, :3]) < 1e-4 and np.linalg.norm(T[:3, 3] - o["T"][:3, 3]) < 1e-3, where
    assert np.allclose(T, o["T"], atol=1e-8), where
    if res["status"] == 0:  # the scene: a camera translating a few tenths of the baseline along +x per frame (test_gpu_images.py's range)
        assert 0.05 < abs(T[0, 3]) < 0.3 and abs(T[1, 3]) < 0.05 and abs(T[2, 3]) < 0.1, (where, T[:3, 3])
        return 1
    assert np.array_equal(T, np.eye(4)), where
    return 0


def uniform_run(ctx, cam, seq, mp, op):
    """a pipeline of one camera fed three copies of `seq`: per frame (results, counts, schedule)"""
    from stvo_amd import images
    pipe = images.ImagePipeline(ctx, B, cam, mp, op, max_kp=2048)
    try:
        out = []
        for left, right in seq:
            res, counts = pipe.push_images(np.stack([left] * B), np.stack([right] * B))
            out.append((res.copy(), counts.copy(), pipe.seq.last_schedule()))
        return out
    finally:
        pipe.close()


@pytest.mark.parametrize("name", sorted(SETS))
def test_three_sizes_side_by_side_and_a_restart_into_a_fourth(oracle, name):
    from stvo_amd import capi, images
    S = SETS[name]
    CAMS = [dict(synth.KITTI_CAM, width=w, height=h) for w, h in S["sizes"]]
    NEW_CAM = dict(synth.KITTI03_CAM, width=S["new"][0], height=S["new"][1])   # another calibration and another size
    slot = (max(w for w, _ in S["sizes"]), max(h for _, h in S["sizes"]))
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=0)
    seqs = [sequence(S["scenes"][b], CAMS[b], NF + 2) for b in range(B)]   # (stream 1 leaves its sequence after NF frames)
    new_seq = sequence(S["new_scene"], NEW_CAM, 3)[:2]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=2048)
        try:
            assert (pipe.cols, pipe.rows) == slot and tuple(pipe.img.shape) == (2 * B, slot[1], slot[0])
            pattern = pipe.orb.pattern()
            # hostile slots: whatever lies beyond an image must not matter
            import torch
            pipe.img.copy_(torch.as_tensor(np.random.default_rng(5).integers(0, 256, tuple(pipe.img.shape)).astype(np.uint8)))
            mixed = []
            for k in range(NF):
                res, counts = pipe.push_images([seqs[b][k][0] for b in range(B)], [seqs[b][k][1] for b in range(B)])
                mixed.append((res.copy(), counts.copy(), pipe.seq.last_schedule()))
            # stream 1 begins a sequence of another camera and size; the others run on
            cont = [seqs[0], seqs[2]]
            after = []
            for k in range(2):
                lefts = [cont[0][NF + k][0], new_seq[k][0], cont[1][NF + k][0]]
                rights = [cont[0][NF + k][1], new_seq[k][1], cont[1][NF + k][1]]
                if k == 0:
                    res, counts = pipe.push_images(lefts, rights, control=[RUN, RESTART, RUN], cams=[None, NEW_CAM, None])
                else:
                    res, counts = pipe.push_images(lefts, rights)
                after.append((res.copy(), counts.copy(), pipe.seq.last_schedule()))
            assert pipe.cams[1] == NEW_CAM and pipe.cams[0] == CAMS[0]
        finally:
            pipe.close()
        # 1. against the CPU chain of every stream under its own camera and size
        n_committed = 0
        for b in range(B):
            frames = oracle_frames(oracle, seqs[b] if b != 1 else seqs[b][:NF], pattern)
            ref = pipeline_ref.run_sequence(oracle, frames, CAMS[b], mp, op)
            steps = mixed + (after if b != 1 else [])
            for k in range(1, len(steps)):
                n_committed += judge(steps[k][0][b], steps[k][1][b], ref[k - 1], (b, k))
            print("stream", b, "status", [r["status"] for r in ref], "stereo points", [r["n_stereo_pt"] for r in ref])
        frames = oracle_frames(oracle, new_seq, pattern)
        ref = pipeline_ref.run_sequence(oracle, frames, NEW_CAM, mp, op)
        zero = np.zeros(1, after[0][0].dtype).tobytes()
        assert after[0][0][1].tobytes() == zero and not after[0][1][1, 2:].any()
        first = pipeline_ref.stereo_frame(oracle, frames[0], NEW_CAM, mp, True, False)
        assert after[0][1][1, 0] == len(first["P"])
        n_restart = judge(after[1][0][1], after[1][1][1], ref[0], "restarted")
        print(name, "committed poses", n_committed, "+", n_restart, "of the restarted sequence")
        if S["committed"]:   # the large set: the chain commits, before and behind the restart
            assert n_committed >= S["committed"] and n_restart == 1
        else:                # the small set: it commits nothing (the module's docstring)
            assert n_committed == 0 and n_restart == 0
        # 2. byte for byte a uniform pipeline of the stream's own size, on the same schedule
        for b in range(B):
            uni = uniform_run(ctx, CAMS[b], seqs[b] if b != 1 else seqs[b][:NF], mp, op)
            steps = mixed + (after if b != 1 else [])
            for k, (res, counts, sched) in enumerate(steps):
                assert sched == uni[k][2], (b, k, sched, uni[k][2])
                assert res[b].tobytes() == uni[k][0][b].tobytes() and np.array_equal(counts[b], uni[k][1][b]), (b, k)
        uni = uniform_run(ctx, NEW_CAM, new_seq, mp, op)
        for k in range(2):
            assert after[k][0][1].tobytes() == uni[k][0][1].tobytes() and np.array_equal(after[k][1][1], uni[k][1][1]), k
    finally:
        ctx.close()


def test_a_list_of_cameras_is_key_points_only(oracle):
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=0)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        for name, kw in (("lsd", dict(lsd=capi.lsd_params(nfeatures=50))), ("fld", dict(fld=capi.fld_params(10.0))),
                         ("rectify", dict(rectify=object())), ("channels", dict(channels=3))):
            with pytest.raises(ValueError, match=name):
                images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256, **kw)
        with pytest.raises(ValueError):
            images.ImagePipeline(ctx, B, CAMS[:2], mp, op, max_kp=256)
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256)
        try:
            z = [np.zeros((h, w), np.uint8) for w, h in SIZES]
            with pytest.raises(ValueError):
                pipe.set_images(z[::-1], z)                                              # an image of another stream's size
            with pytest.raises(ValueError):
                pipe.enqueue(cams=[None, NEW_CAM, None])                                 # cameras without a control
            with pytest.raises(ValueError):
                pipe.enqueue(control=[RUN, RESTART, RUN], cams=[None, dict(NEW_CAM, width=321), None])   # larger than the slot
        finally:
            pipe.close()
        one = images.ImagePipeline(ctx, B, CAMS[0], mp, op, max_kp=256)                   # a single dict: as ever, and no cams
        try:
            assert one.cams is None
            with pytest.raises(ValueError):
                one.enqueue(control=[RUN, RESTART, RUN], cams=[None, NEW_CAM, None])
        finally:
            one.close()
    finally:
        ctx.close()
