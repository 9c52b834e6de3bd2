"""Images -> poses with key-points AND FLD key-lines (use_fld_lines), one camera and image size per stream: ImagePipeline(cam=[B dicts],
fld=..., lines_per_stream=True, fld_min_length_ratio=0.025).  The pattern of tests/test_gpu_images_mixed_lines.py on the same "large"
set: three streams of 640 x 240, 636 x 236 and 512 x 240 in slots of 640 x 240, then a RESTART of stream 1 into 600 x 232 under
KITTI03_CAM; every stream's length threshold is int(0.025 x min(width, height)) of its own camera — 6, 5, 6, then 5 — so the threshold
per image and the detector's minimum (5, under a caller's 6) are both exercised.

Every stream, the restarted one included, is judged against the CPU chain (the ORB oracle, the FLD statement tests/cpp/fld_ref.c and the
LBD oracle on every image at its own size and threshold, then pipeline_ref.run_sequence under that stream's camera) with the assertions
and tolerances of tests/test_gpu_fld.py::test_images_to_poses_fld_lines, and byte for byte against a uniform ImagePipeline of its own
size and threshold on the same schedule, with noise beyond every image in its slot.  What the run rests on is asserted on the CPU
chain before anything runs on the GPU.  A second pass feeds RAW B, G, R slots through a rectifier bank: ORB reads the grey plane, FLD
and LBD the swapped-weight one, both in the slot layout; the planes are held against np_color.gray of the crops rectified in numpy, and
the results byte for byte against one-camera colour pipelines (no bank) fed those rectified crops."""
import numpy as np
import pytest

import fld_statement
import np_color
import pipeline_ref
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_fld import fld_lines
from test_gpu_images import oracle_frames
from test_gpu_images_bank import colour_of, rectified
from test_gpu_images_mixed_lines import B, CAMS, MAX_KL, NEW_CAM, NF, NLINES, RESTART, RUN, S, SLOT, calibrations, judge, schedule, sequences

pytestmark = pytest.mark.gpu
RATIO = 0.025

_chain = {}


@pytest.fixture(scope="module")
def stmt():
    return fld_statement.load()


def threshold(cam):
    return int(RATIO * min(cam["width"], cam["height"]))


def fld_for(cam=None):
    from stvo_amd import capi
    return capi.fld_params(threshold(cam) if cam is not None else 6, nfeatures=NLINES)


def line_frames(oracle, stmt, pairs, pattern, cam):
    """the CPU front-end of one stream: ORB, FLD at the camera's own threshold, LBD — on every image at its own size"""
    frames = oracle_frames(oracle, pairs, pattern)
    for fr, (left, right) in zip(frames, pairs):
        assert left.shape == right.shape == (cam["height"], cam["width"])
        fr["kl_l"], fr["ang_l"], fr["ldesc_l"] = fld_lines(oracle, stmt, left, threshold(cam), NLINES)
        fr["kl_r"], _, fr["ldesc_r"] = fld_lines(oracle, stmt, right, threshold(cam), NLINES)
        fr["oct_ll"] = np.zeros(len(fr["kl_l"]), np.int32)
    return frames


def cpu_chain(oracle, stmt, pattern, mp, op):
    """-> (per stream: the chain's results of its sequence, the restarted sequence's frames and results); the conditions the test rests
    on are asserted here, on the CPU"""
    key = pattern.tobytes()
    if key not in _chain:
        assert [threshold(c) for c in CAMS + [NEW_CAM]] == [6, 5, 6, 5]
        seqs, new_seq = sequences()
        refs = []
        for b in range(B):
            frames = line_frames(oracle, stmt, seqs[b] if b != 1 else seqs[b][:NF], pattern, CAMS[b])
            refs.append(pipeline_ref.run_sequence(oracle, frames, CAMS[b], mp, op))
        new_frames = line_frames(oracle, stmt, new_seq, pattern, NEW_CAM)
        new_ref = pipeline_ref.run_sequence(oracle, new_frames, NEW_CAM, mp, op)
        for where, ref in [(b, refs[b]) for b in range(B)] + [("restarted", new_ref)]:
            stereo, matched = [r["n_stereo_ls"] for r in ref], [r["n_matched_ls"] for r in ref]
            print("stream", where, "stereo key-lines", stereo, "matched", matched, "status", [r["status"] for r in ref])
            assert all(35 <= n <= 56 for n in stereo), (where, stereo)               # every stream gets stereo key-lines in every frame,
            assert all(25 <= n <= 49 for n in matched), (where, matched)             # matches them frame to frame,
            assert all(r["status"] == 0 for r in ref), where                         # and every tracked frame commits, the restarted one included
        _chain[key] = (refs, new_frames, new_ref)
    return _chain[key]


def uniform_run(ctx, cam, seq, mp, op, **kw):
    """a pipeline of one camera, its own size and threshold, fed three copies of `seq`: per frame (results, counts, schedule)"""
    from stvo_amd import images
    pipe = images.ImagePipeline(ctx, B, cam, mp, op, max_kp=2048, fld=fld_for(cam), max_kl=MAX_KL, **kw)
    try:
        out = []
        for left, right in seq:
            res, counts = pipe.push_images(np.stack([left] * B), np.stack([right] * B))
            out.append((res.copy(), counts.copy(), pipe.seq.last_schedule()))
        return out
    finally:
        pipe.close()


def hostile(pipe):
    """whatever lies beyond an image in its slot must not matter"""
    import torch
    rng = np.random.default_rng(5)
    for buf in (pipe.img, pipe.rect_img, pipe.color, pipe.gray_b):
        if buf is not None:
            buf.copy_(torch.as_tensor(rng.integers(0, 256, tuple(buf.shape)).astype(np.uint8)))


def same_as_uniform(ctx, mixed, after, seqs, new_seq, mp, op, prep=None, **kw):
    """byte for byte a uniform pipeline of the stream's own size and threshold, on the same schedule"""
    prep = prep or (lambda pairs, k: pairs)
    for b in range(B):
        uni = uniform_run(ctx, CAMS[b], prep(seqs[b] if b != 1 else seqs[b][:NF], b), mp, op, **kw)
        steps = mixed + (after if b != 1 else [])
        for k, (res, counts, sched) in enumerate(steps):
            assert sched == uni[k][2], (b, k, sched, uni[k][2])
            assert res[b].tobytes() == uni[k][0][b].tobytes() and np.array_equal(counts[b], uni[k][1][b]), (b, k)
    uni = uniform_run(ctx, NEW_CAM, prep(new_seq, 3), mp, op, **kw)
    for k in range(2):
        assert after[k][0][1].tobytes() == uni[k][0][1].tobytes() and np.array_equal(after[k][1][1], uni[k][1][1]), k


def test_three_sizes_with_fld_lines_and_a_restart_into_a_fourth(oracle, stmt):
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    seqs, new_seq = sequences()
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=2048, fld=fld_for(), max_kl=MAX_KL, lines_per_stream=True,
                                    fld_min_length_ratio=RATIO)
        try:
            assert (pipe.cols, pipe.rows) == SLOT and tuple(pipe.img.shape) == (2 * B, SLOT[1], SLOT[0])
            assert pipe.fld_store_threshold == 5 and pipe.fld_length_threshold == 6     # created at the smallest it is given
            refs, new_frames, new_ref = cpu_chain(oracle, stmt, pipe.orb.pattern(), mp, op)   # (its conditions: before the GPU run)
            hostile(pipe)

            def push(lefts, rights, **kw):
                res, counts = pipe.push_images(lefts, rights, **kw)
                return res.copy(), counts.copy(), pipe.seq.last_schedule()
            mixed, after = schedule(push, seqs, new_seq, dict(control=[RUN, RESTART, RUN], cams=[None, NEW_CAM, None]))
            assert pipe.cams[1] == NEW_CAM and pipe.cams[0] == CAMS[0]
        finally:
            pipe.close()
        # 1. against the CPU chain of every stream under its own camera, size and threshold
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
        # 2. byte for byte the uniform pipelines
        same_as_uniform(ctx, mixed, after, seqs, new_seq, mp, op)
    finally:
        ctx.close()


def test_raw_colour_slots_through_the_bank():
    """the same run on RAW B, G, R frames, rectified and converted per stream by the bank's one launch in front of ORB (the grey plane) and
    of FLD and LBD (the swapped-weight plane)"""
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    seqs, new_seq = sequences()
    cal = calibrations()
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    rects = bank = pipe = None
    try:
        rects = [capi.Rectifier(ctx, B, calib=c) for c, _ in cal]
        bank = capi.RectifierBank(ctx, B, SLOT[0], SLOT[1], rects)
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, rectify=bank, calibs=[0, 1, 2], channels=3, max_kp=2048, fld=fld_for(),
                                    max_kl=MAX_KL, lines_per_stream=True, fld_min_length_ratio=RATIO)
        assert pipe.gray_b is not None and tuple(pipe.gray_b.shape) == (2 * B, SLOT[1], SLOT[0])
        hostile(pipe)
        calibs_now = [0, 1, 2]

        def push(lefts, rights, **kw):
            if kw:
                calibs_now[1] = 3
            lefts, rights = [colour_of(im) for im in lefts], [colour_of(im) for im in rights]
            got = pipe.push_images(lefts, rights, calibs=[None, 3, None], **kw) if kw else pipe.push_images(lefts, rights)
            sched = pipe.seq.last_schedule()
            # the two planes the detectors read, in the slot layout: the crops rectified and converted in numpy
            ga, gb = pipe.img.cpu().numpy(), pipe.gray_b.cpu().numpy()
            for side, imgs in ((0, lefts), (1, rights)):
                for b, im in enumerate(imgs):
                    r = rectified(im, cal[calibs_now[b]][1], side)
                    h, w = r.shape[:2]
                    assert np.array_equal(ga[side * B + b, :h, :w], np_color.gray(r, "bgr", "q14")), (side, b)
                    assert np.array_equal(gb[side * B + b, :h, :w], np_color.gray(r, "rgb", "q14")), (side, b)
                    assert not np.array_equal(ga[side * B + b, :h, :w], gb[side * B + b, :h, :w])
            return got[0].copy(), got[1].copy(), sched
        mixed, after = schedule(push, seqs, new_seq, dict(control=[RUN, RESTART, RUN], cams=[None, NEW_CAM, None]))
        assert pipe.calibs == [0, 3, 2] and pipe.cams[1] == NEW_CAM
        assert all(sum(int(r[0][b]["n_matched_ls"]) for r in mixed + after) > 0 for b in range(B))   # a real run: key-lines matched everywhere
        assert after[1][0][1]["n_matched_ls"] > 0
        pipe.close(); pipe = None

        def prep(pairs, k):   # stream k's (k = 3: the restarted sequence's) colour frames under its calibration, rectified in numpy
            return [(rectified(colour_of(l), cal[k][1], 0), rectified(colour_of(r), cal[k][1], 1)) for l, r in pairs]
        same_as_uniform(ctx, mixed, after, seqs, new_seq, mp, op, prep=prep, channels=3)
    finally:
        for o in (pipe, bank):
            if o is not None:
                o.close()
        for r in rects or []:
            r.close()
        ctx.close()


def test_a_restart_camera_the_stores_cannot_hold():
    """three streams of threshold 6: the detector's stores hold 640 x 240 / 7 + 1 = 21943 segments; 600 x 232 at its own threshold 5
    needs 23201 — ValueError before anything is staged, and the pipeline runs on as it was"""
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    cams = [CAMS[0], CAMS[2], CAMS[0]]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        pipe = images.ImagePipeline(ctx, B, cams, mp, op, max_kp=256, fld=fld_for(), max_kl=MAX_KL, lines_per_stream=True, fld_min_length_ratio=RATIO)
        try:
            assert pipe.fld_store_threshold == 6
            with pytest.raises(ValueError, match="23201.*21943"):
                pipe.enqueue(control=[RUN, RESTART, RUN], cams=[None, NEW_CAM, None])
            assert pipe.cams == cams
            # the detector's own refusal, had the pipeline not looked first: the same rule, and the table stays
            with pytest.raises(capi.StvoError, match="23201"):
                pipe.fld.set_image_sizes([(600, 232)], [5])
            seqs, _ = sequences()
            res, counts = pipe.push_images([seqs[0][0][0], seqs[2][0][0], seqs[0][0][0]], [seqs[0][0][1], seqs[2][0][1], seqs[0][0][1]])
            assert counts[:, 1].min() > 0 and np.array_equal(counts[0], counts[2])
        finally:
            pipe.close()
        with pytest.raises(ValueError, match="lines_per_stream"):   # the opt-in still goes with a detector
            images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256, lines_per_stream=True)
    finally:
        ctx.close()
