"""Images -> poses with key-points AND key-lines, one camera and image size per stream: ImagePipeline(cam=[B dicts], lsd=...,
lines_per_stream=True, lsd_min_length_ratio=0.025).  The "large" pattern of tests/test_gpu_images_mixed.py with op.has_lines = 1: three
streams of 640 x 240, 636 x 236 and 512 x 240 in slots of 640 x 240, then a RESTART of stream 1 into 600 x 232 under KITTI03_CAM; every
stream's minimum line length is 0.025 x min(width, height) of its own camera (6.0, 5.9, 6.0, then 5.8 pixels).

Every stream, the restarted one included, is judged against the CPU chain (the ORB, LSD and LBD oracles on every image at its own size
and minimum length, then pipeline_ref.run_sequence under that stream's camera) with the assertions and tolerances of
tests/test_gpu_images.py::test_images_to_poses_points_and_lines, and byte for byte against a uniform ImagePipeline of its own size and
minimum length on the same schedule.  The CPU chain itself must match key-lines on every stream and commit poses before and behind the
restart: asserted on the CPU, before anything runs on the GPU.  A second pass feeds RAW grey slots through a rectifier bank (two dist 0
calibrations, two KITTI-form ones with distortion) and is judged byte for byte against the pipeline without a bank fed the crops
rectified in numpy."""
import numpy as np
import pytest

import np_model
import np_rectify as nr
import pipeline_ref
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_images import oracle_frames
from test_gpu_images_mixed import SETS, sequence

pytestmark = pytest.mark.gpu
B, NF, NLINES, MAX_KL, RATIO = 3, 4, 100, 128, 0.025
RUN, RESTART = 0, 1
S = SETS["large"]
CAMS = [dict(synth.KITTI_CAM, width=w, height=h) for w, h in S["sizes"]]
NEW_CAM = dict(synth.KITTI03_CAM, width=S["new"][0], height=S["new"][1])
SLOT = (max(w for w, _ in S["sizes"]), max(h for _, h in S["sizes"]))

_chain = {}


def min_length(cam):
    return RATIO * min(cam["width"], cam["height"])


def sequences():
    seqs = [sequence(S["scenes"][b], CAMS[b], NF + 2) for b in range(B)]   # (stream 1 leaves its sequence after NF frames)
    return seqs, sequence(S["new_scene"], NEW_CAM, 3)[:2]


def line_frames(oracle, pairs, pattern, cam):
    """the CPU front-end of one stream: ORB, LSD at the camera's own minimum length, LBD — on every image at its own size"""
    from stvo_amd import capi
    frames = oracle_frames(oracle, pairs, pattern)
    lopts = oracle.lsd_opts(min_length=min_length(cam), nfeatures=NLINES)
    for fr, (left, right) in zip(frames, pairs):
        for side, img in (("l", left), ("r", right)):
            assert img.shape == (cam["height"], cam["width"])
            kl = oracle.lsd_detect(img, lopts)
            rec = np.stack([kl["sx"], kl["sy"], kl["ex"], kl["ey"], kl["angle"]], axis=1).astype(np.float32)
            fr["kl_" + side] = np.ascontiguousarray(rec[:, :4])
            fr["ldesc_" + side] = oracle.lbd_compute(img, rec, kl["num_pixels"])
            if side == "l":
                fr["ang_l"] = np.ascontiguousarray(rec[:, 4]); fr["oct_ll"] = np.zeros(len(rec), np.int32)
    return frames


def cpu_chain(oracle, pattern, mp, op):
    """-> (per stream: the chain's results of its sequence, the restarted sequence's frames and results); the conditions the test rests
    on are asserted here, on the CPU"""
    key = pattern.tobytes()
    if key not in _chain:
        seqs, new_seq = sequences()
        refs = []
        for b in range(B):
            frames = line_frames(oracle, seqs[b] if b != 1 else seqs[b][:NF], pattern, CAMS[b])
            refs.append(pipeline_ref.run_sequence(oracle, frames, CAMS[b], mp, op))
        new_frames = line_frames(oracle, new_seq, pattern, NEW_CAM)
        new_ref = pipeline_ref.run_sequence(oracle, new_frames, NEW_CAM, mp, op)
        for b in range(B):
            assert sum(r["n_matched_ls"] for r in refs[b]) > 0, b                       # key-lines are matched on every stream
            assert sum(r["status"] == 0 for r in refs[b][:NF - 1]) > 0, b               # and poses committed before the restart
        assert all(sum(r["status"] == 0 for r in refs[b][NF - 1:]) > 0 for b in (0, 2))   # and behind it, on the streams that run on
        assert new_ref[0]["n_matched_ls"] > 0 and new_ref[0]["status"] == 0             # and on the restarted one
        _chain[key] = (refs, new_frames, new_ref)
    return _chain[key]


def judge(res, counts, o, where):
    """the per-frame assertions of tests/test_gpu_images.py::test_images_to_poses_points_and_lines"""
    assert counts[0] == o["n_stereo_pt"] and counts[1] == o["n_stereo_ls"], (where, counts, o["n_stereo_pt"], o["n_stereo_ls"])
    assert res["n_matched_pt"] == o["n_matched_pt"] and res["n_matched_ls"] == o["n_matched_ls"], where
    assert res["status"] == o["status"] and res["path"] == o["path"] and tuple(res["iters"]) == o["iters"], where
    assert res["n_inliers_pt"] == o["n_inliers_pt"] and res["n_inliers_ls"] == o["n_inliers_ls"], where
    T = res["T"].reshape(4, 4)
    assert np_model.rot_angle(T[:3, :3], o["T"][:3, :3]) < 1e-4 and np.linalg.norm(T[:3, 3] - o["T"][:3, 3]) < 1e-3, where
    assert np.allclose(T, o["T"], atol=1e-8), where


def lsd_for(cam=None):
    from stvo_amd import capi
    return capi.lsd_params(min_length=min_length(cam) if cam is not None else 1.0, nfeatures=NLINES)


def uniform_run(ctx, cam, seq, mp, op):
    """a pipeline of one camera, its own size and minimum length, fed three copies of `seq`: per frame (results, counts, schedule)"""
    from stvo_amd import images
    pipe = images.ImagePipeline(ctx, B, cam, mp, op, max_kp=2048, lsd=lsd_for(cam), max_kl=MAX_KL)
    try:
        out = []
        for left, right in seq:
            res, counts = pipe.push_images(np.stack([left] * B), np.stack([right] * B))
            out.append((res.copy(), counts.copy(), pipe.seq.last_schedule()))
        return out
    finally:
        pipe.close()


def schedule(push, seqs, new_seq, restart_kw):
    """the run of the module's docstring through push(lefts, rights, **kw): NF steps side by side, the RESTART of stream 1, one more step"""
    steps = []
    for k in range(NF):
        steps.append(push([seqs[b][k][0] for b in range(B)], [seqs[b][k][1] for b in range(B)]))
    cont = [seqs[0], seqs[2]]
    for k in range(2):
        lefts = [cont[0][NF + k][0], new_seq[k][0], cont[1][NF + k][0]]
        rights = [cont[0][NF + k][1], new_seq[k][1], cont[1][NF + k][1]]
        steps.append(push(lefts, rights, **(restart_kw if k == 0 else {})))
    return steps[:NF], steps[NF:]


def hostile(pipe):
    """whatever lies beyond an image in its slot must not matter"""
    import torch
    rng = np.random.default_rng(5)
    for buf in (pipe.img, pipe.rect_img):
        if buf is not None:
            buf.copy_(torch.as_tensor(rng.integers(0, 256, tuple(buf.shape)).astype(np.uint8)))


def test_three_sizes_with_lines_and_a_restart_into_a_fourth(oracle):
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    seqs, new_seq = sequences()
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=2048, lsd=lsd_for(), max_kl=MAX_KL, lines_per_stream=True,
                                    lsd_min_length_ratio=RATIO)
        try:
            assert (pipe.cols, pipe.rows) == SLOT and tuple(pipe.img.shape) == (2 * B, SLOT[1], SLOT[0])
            refs, new_frames, new_ref = cpu_chain(oracle, pipe.orb.pattern(), mp, op)   # (its conditions: before the GPU run)
            hostile(pipe)

            def push(lefts, rights, **kw):
                res, counts = pipe.push_images(lefts, rights, **kw)
                return res.copy(), counts.copy(), pipe.seq.last_schedule()
            mixed, after = schedule(push, seqs, new_seq, dict(control=[RUN, RESTART, RUN], cams=[None, NEW_CAM, None]))
            assert pipe.cams[1] == NEW_CAM and pipe.cams[0] == CAMS[0]
        finally:
            pipe.close()
        # 1. against the CPU chain of every stream under its own camera, size and minimum length
        lines_used = np.zeros(B, np.int64)
        for b in range(B):
            steps = mixed + (after if b != 1 else [])
            for k in range(1, len(steps)):
                judge(steps[k][0][b], steps[k][1][b], refs[b][k - 1], (b, k))
                lines_used[b] += steps[k][0][b]["n_matched_ls"]
        assert (lines_used > 0).all(), lines_used
        zero = np.zeros(1, after[0][0].dtype).tobytes()
        assert after[0][0][1].tobytes() == zero and not after[0][1][1, 2:].any()     # the restarted stream's first frame: no pose
        first = pipeline_ref.stereo_frame(oracle, new_frames[0], NEW_CAM, mp, True, True)
        assert after[0][1][1, 0] == len(first["P"]) and after[0][1][1, 1] == len(first["sP"])
        judge(after[1][0][1], after[1][1][1], new_ref[0], "restarted")
        assert after[1][0][1]["n_matched_ls"] > 0 and after[1][0][1]["status"] == 0
        # 2. byte for byte a uniform pipeline of the stream's own size and minimum length, on the same schedule
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


def calibrations():
    """four calibrations of the four sizes: dist 0 (a copy) for streams 0 and 1, KITTI form with distortion for stream 2 and for the
    sequence stream 1 restarts into -> [(RectCalib, (map1, map2) or None)]"""
    from stvo_amd import capi
    out = []
    for (w, h), d in zip(S["sizes"] + [S["new"]], ([0.0] * 4, [0.0] * 4, [-0.10, 0.02, 0.0004, -0.0003], [-0.12, 0.03, 0.0005, -0.0004])):
        c = capi.RectCalib()
        c.form, c.width, c.height, c.b = capi.RECT_FORM_KITTI, w, h, synth.KITTI_CAM["b"]
        c.fx, c.fy, c.cx, c.cy = 0.58 * w, 0.58 * w, 0.5 * w - 1.0, 0.5 * h + 0.5
        c.d[:] = d
        if any(d):
            cam, m1, m2 = capi.rectify_compute(c)
            assert cam["dist"] == 1
            out.append((c, (m1, m2)))
        else:
            out.append((c, None))
    return out


def test_raw_grey_slots_through_the_bank(oracle):
    """the same run on RAW frames, rectified per stream by the bank in front of ORB, LSD and LBD — against the pipeline without a bank fed
    the crops rectified in numpy"""
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    seqs, new_seq = sequences()
    cal = calibrations()
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    rects = bank = pipe = ref = None
    try:
        rects = [capi.Rectifier(ctx, B, calib=c) for c, _ in cal]
        assert [r.dist for r in rects] == [0, 0, 1, 1]
        bank = capi.RectifierBank(ctx, B, SLOT[0], SLOT[1], rects)
        kw = dict(max_kp=2048, lsd=lsd_for(), max_kl=MAX_KL, lines_per_stream=True, lsd_min_length_ratio=RATIO)
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, rectify=bank, calibs=[0, 1, 2], **kw)
        ref = images.ImagePipeline(ctx, B, CAMS, mp, op, **kw)
        hostile(pipe); hostile(ref)
        calibs_now = [0, 1, 2]

        def rectified(img, k, side):
            maps = cal[k][1]
            return img.copy() if maps is None else nr.remap(img, maps[0][side], maps[1][side])

        def push(lefts, rights, **kw):
            if kw:
                calibs_now[1] = 3
            got = pipe.push_images(lefts, rights, calibs=[None, 3, None], **kw) if kw else pipe.push_images(lefts, rights)
            want = ref.push_images([rectified(im, calibs_now[b], 0) for b, im in enumerate(lefts)],
                                   [rectified(im, calibs_now[b], 1) for b, im in enumerate(rights)], **kw)
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), (calibs_now, kw)
            assert pipe.seq.last_schedule() == ref.seq.last_schedule()
            return got[0].copy(), got[1].copy()
        mixed, after = schedule(push, seqs, new_seq, dict(control=[RUN, RESTART, RUN], cams=[None, NEW_CAM, None]))
        assert pipe.calibs == [0, 3, 2] and pipe.cams[1] == NEW_CAM
        # the run is a real one: key-lines matched on every stream, the restarted one included, and the copied streams are the CPU chain's
        assert all(sum(int(r[0][b]["n_matched_ls"]) for r in mixed + after) > 0 for b in range(B))
        assert after[1][0][1]["n_matched_ls"] > 0
        refs, _, _ = cpu_chain(oracle, pipe.orb.pattern(), mp, op)
        for k in range(1, NF):
            judge(mixed[k][0][0], mixed[k][1][0], refs[0][k - 1], ("copied", 0, k))
            judge(mixed[k][0][1], mixed[k][1][1], refs[1][k - 1], ("copied", 1, k))
    finally:
        for o in (pipe, ref, bank):
            if o is not None:
                o.close()
        for r in rects or []:
            r.close()
        ctx.close()


def test_refusals():
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        with pytest.raises(ValueError, match="lsd"):            # the refusal without the opt-in stays
            images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256, lsd=lsd_for())
        with pytest.raises(ValueError, match="fld"):            # the FLD walk holds one size: refused with and without the opt-in
            images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256, fld=capi.fld_params(10.0))
        with pytest.raises(ValueError, match="fld"):
            images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256, fld=capi.fld_params(10.0), lsd=lsd_for(), lines_per_stream=True)
        with pytest.raises(ValueError, match="lines_per_stream"):   # without a list
            images.ImagePipeline(ctx, B, CAMS[0], mp, op, max_kp=256, lsd=lsd_for(), lines_per_stream=True)
        with pytest.raises(ValueError, match="lines_per_stream"):   # without lsd
            images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256, lines_per_stream=True)
        with pytest.raises(ValueError, match="lines_per_stream"):
            images.ImagePipeline(ctx, B, CAMS[0], mp, op, max_kp=256, lines_per_stream=True)
        # a camera larger than the slot on a RESTART: refused before anything is staged, the detectors keep their tables
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256, lsd=lsd_for(), max_kl=MAX_KL, lines_per_stream=True, lsd_min_length_ratio=RATIO)
        try:
            with pytest.raises(ValueError):
                pipe.enqueue(control=[RUN, RESTART, RUN], cams=[None, dict(NEW_CAM, width=SLOT[0] + 1), None])
            with pytest.raises(ValueError):
                pipe.enqueue(cams=[None, NEW_CAM, None])
            assert pipe.cams == CAMS
        finally:
            pipe.close()
    finally:
        ctx.close()
