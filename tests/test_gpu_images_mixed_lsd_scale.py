"""Images -> poses with key-lines at lsd_scale 0.5, one camera and image size per stream: ImagePipeline(cam=[B dicts],
lsd=capi.lsd_params(scale=0.5, ...), lines_per_stream=True, lsd_min_length_ratio=0.025) — the blur radius is 5, so the scaled image comes
from the MIXED instance of the fused blur + resize (csrc/lsd_scale_kernels.hip) under the slot's tile plan.  The "large" pattern of
tests/test_gpu_images_mixed_lines.py: three streams of 640 x 240, 636 x 236 and 512 x 240 in slots of 640 x 240, then a RESTART of
stream 1 into 600 x 232 under KITTI03_CAM.

Every stream, the restarted one included, is judged byte for byte — results and counts — against a uniform ImagePipeline of its own
size and minimum length at the same lsd_scale on the same schedule.  Those uniform pipelines are code that existed, and the conditions
the test rests on are asserted on THEM before the mixed result is looked at: key-lines are matched on every stream, and poses committed
before and behind the restart.  A second pass feeds RAW grey slots through a rectifier bank and is judged against the pipeline without a
bank fed the crops rectified in numpy."""
import numpy as np
import pytest

import np_rectify as nr
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_images_mixed_lines import (B, CAMS, MAX_KL, NEW_CAM, NF, NLINES, RATIO, RESTART, RUN, SLOT, calibrations, hostile, min_length,
                                         schedule, sequences)

pytestmark = pytest.mark.gpu
SCALE = 0.5


def lsd_for(cam=None):
    from stvo_amd import capi
    return capi.lsd_params(min_length=min_length(cam) if cam is not None else 1.0, nfeatures=NLINES, scale=SCALE)


def uniform_run(ctx, cam, seq, mp, op):
    """a pipeline of one camera, its own size and minimum length, fed three copies of `seq`: per frame (results, counts, schedule)"""
    from stvo_amd import images
    pipe = images.ImagePipeline(ctx, B, cam, mp, op, max_kp=2048, lsd=lsd_for(cam), max_kl=MAX_KL)
    try:
        assert pipe.lsd.geometry["radius"] == 5
        out = []
        for left, right in seq:
            res, counts = pipe.push_images(np.stack([left] * B), np.stack([right] * B))
            out.append((res.copy(), counts.copy(), pipe.seq.last_schedule()))
        return out
    finally:
        pipe.close()


def test_three_sizes_at_half_scale_and_a_restart_into_a_fourth():
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    seqs, new_seq = sequences()
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        # the uniform pipelines first, and on them what the test rests on
        unis = [uniform_run(ctx, CAMS[b], seqs[b] if b != 1 else seqs[b][:NF], mp, op) for b in range(B)]
        uni_new = uniform_run(ctx, NEW_CAM, new_seq, mp, op)
        for b in range(B):
            assert sum(int(u[0][b]["n_matched_ls"]) for u in unis[b]) > 0, b                        # key-lines are matched on every stream
            assert sum(int(u[0][b]["status"]) == 0 for u in unis[b][1:NF]) > 0, b                   # and poses committed before the restart
        assert all(sum(int(u[0][b]["status"]) == 0 for u in unis[b][NF:]) > 0 for b in (0, 2))      # and behind it, on the streams that run on
        assert uni_new[1][0][1]["n_matched_ls"] > 0 and uni_new[1][0][1]["status"] == 0             # and on the restarted one
        lsd = lsd_for()
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=2048, lsd=lsd, max_kl=MAX_KL, lines_per_stream=True,
                                    lsd_min_length_ratio=RATIO)
        try:
            assert lsd.flags == 0                                     # the caller's parameters are not touched: the pipeline flags a copy
            assert (pipe.cols, pipe.rows) == SLOT and pipe.lsd.geometry["radius"] == 5
            hostile(pipe)

            def push(lefts, rights, **kw):
                res, counts = pipe.push_images(lefts, rights, **kw)
                return res.copy(), counts.copy(), pipe.seq.last_schedule()
            mixed, after = schedule(push, seqs, new_seq, dict(control=[RUN, RESTART, RUN], cams=[None, NEW_CAM, None]))
            assert pipe.cams[1] == NEW_CAM and pipe.cams[0] == CAMS[0]
        finally:
            pipe.close()
        for b in range(B):
            steps = mixed + (after if b != 1 else [])
            for k, (res, counts, sched) in enumerate(steps):
                assert sched == unis[b][k][2], (b, k, sched, unis[b][k][2])
                assert res[b].tobytes() == unis[b][k][0][b].tobytes() and np.array_equal(counts[b], unis[b][k][1][b]), (b, k)
        zero = np.zeros(1, after[0][0].dtype).tobytes()
        assert after[0][0][1].tobytes() == zero and not after[0][1][1, 2:].any()     # the restarted stream's first frame: no pose
        for k in range(2):
            assert after[k][0][1].tobytes() == uni_new[k][0][1].tobytes() and np.array_equal(after[k][1][1], uni_new[k][1][1]), k
        # the scale is not ignored on the mixed route: at the shipped 1.2 the same streams give other key-line counts
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=2048, lsd=capi.lsd_params(min_length=1.0, nfeatures=NLINES), max_kl=MAX_KL,
                                    lines_per_stream=True, lsd_min_length_ratio=RATIO)
        try:
            hostile(pipe)
            _, counts = pipe.push_images([seqs[b][0][0] for b in range(B)], [seqs[b][0][1] for b in range(B)])
            assert not np.array_equal(counts[:, 1], mixed[0][1][:, 1])
        finally:
            pipe.close()
    finally:
        ctx.close()


def test_raw_grey_slots_through_the_bank_at_half_scale():
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
        bank = capi.RectifierBank(ctx, B, SLOT[0], SLOT[1], rects)
        kw = dict(max_kp=2048, lsd=lsd_for(), max_kl=MAX_KL, lines_per_stream=True, lsd_min_length_ratio=RATIO)
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, rectify=bank, calibs=[0, 1, 2], **kw)
        ref = images.ImagePipeline(ctx, B, CAMS, mp, op, **kw)
        assert pipe.lsd.geometry["radius"] == 5
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
        # the run is a real one: key-lines matched on every stream, the restarted one included
        assert all(sum(int(r[0][b]["n_matched_ls"]) for r in mixed + after) > 0 for b in range(B))
        assert after[1][0][1]["n_matched_ls"] > 0
    finally:
        for o in (pipe, ref, bank):
            if o is not None:
                o.close()
        for r in rects or []:
            r.close()
        ctx.close()


def test_without_the_opt_in_nothing_changes():
    """a list of cameras with lsd and no lines_per_stream is refused at every scale, as before"""
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        with pytest.raises(ValueError, match="lsd"):
            images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256, lsd=lsd_for())
    finally:
        ctx.close()
