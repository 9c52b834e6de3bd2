"""ImagePipeline(cam=[B dicts], lsd=..., lines_per_stream=True, lsd_many_waves=True): the pipeline sets STVO_LSD_TABLE_BY_BATCH on its LSD
detector, so the 2 B images of a step run the many-wave search under their size table (csrc/lsd_route.h).  Four streams over the three
cameras of tests/test_gpu_images_mixed_lines.py (640 x 240, 636 x 236, 512 x 240, and 640 x 240 again on another scene: 8 images per LSD
launch), four steps side by side, then a RESTART of stream 1 into 600 x 232 under KITTI03_CAM and one more step: key-lines, their
descriptors, counts, schedules and pose results must match, byte for byte, a second pipeline built with lsd_many_waves=False on the same
frames.  That pipeline's results are judged against the CPU chain by tests/test_gpu_images_mixed_lines.py."""
import numpy as np
import pytest

import test_gpu_images_mixed_lines as ml
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_images_mixed import sequence

pytestmark = pytest.mark.gpu
B = 4
CAMS = ml.CAMS + [ml.CAMS[0]]
RUN, RESTART, NF = ml.RUN, ml.RESTART, ml.NF


def frames():
    """per step: (lefts, rights, keywords) for the four streams"""
    seqs, new_seq = ml.sequences()
    seqs = seqs + [sequence(ml.S["new_scene"], ml.CAMS[0], NF + 2)]
    steps = [([seqs[b][k][0] for b in range(B)], [seqs[b][k][1] for b in range(B)], {}) for k in range(NF)]
    for k in range(2):
        own = [seqs[b][NF + k] for b in range(B)]
        own[1] = new_seq[k]
        kw = dict(control=[RUN, RESTART, RUN, RUN], cams=[None, ml.NEW_CAM, None, None]) if k == 0 else {}
        steps.append(([p[0] for p in own], [p[1] for p in own], kw))
    return steps


def lines_of(pipe):
    """what the line front-end left for the 2 B images of the last step: (counts, records, descriptors) of the kept key-lines"""
    nl = pipe.nl.cpu().numpy()
    kl, ld = pipe.kl.cpu().numpy(), pipe.ldesc.cpu().numpy()
    return nl, [kl[i, :nl[i]].tobytes() for i in range(2 * B)], [ld[i, :nl[i]].tobytes() for i in range(2 * B)]


def test_four_streams_three_cameras_on_many_waves():
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    pipes = []
    try:
        for many in (True, False):
            pipes.append(images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=2048, lsd=ml.lsd_for(), max_kl=ml.MAX_KL, lines_per_stream=True,
                                              lsd_min_length_ratio=ml.RATIO, lsd_many_waves=many))
            ml.hostile(pipes[-1])
        fast, slow = pipes
        assert fast.lsd.search_route() == capi.LSD_SEARCH_MANY_WAVES and slow.lsd.search_route() == capi.LSD_SEARCH_ONE_WAVE
        lines_matched = np.zeros(B, np.int64)
        for k, (lefts, rights, kw) in enumerate(frames()):
            got = fast.push_images(lefts, rights, **kw)
            want = slow.push_images(lefts, rights, **kw)
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), k
            assert fast.seq.last_schedule() == slow.seq.last_schedule(), k
            (n_f, kl_f, ld_f), (n_s, kl_s, ld_s) = lines_of(fast), lines_of(slow)
            assert np.array_equal(n_f, n_s) and kl_f == kl_s and ld_f == ld_s, k
            assert (n_f > 0).all(), (k, n_f)
            assert fast.lsd.search_route() == capi.LSD_SEARCH_MANY_WAVES, k     # the RESTART's new table keeps the route
            lines_matched += np.array([int(r["n_matched_ls"]) for r in got[0]])
        assert fast.cams[1] == ml.NEW_CAM and (lines_matched > 0).all(), lines_matched
    finally:
        for p in pipes:
            p.close()
        ctx.close()


def test_where_lsd_many_waves_is_refused():
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        kw = dict(max_kp=256, max_kl=ml.MAX_KL, lsd_many_waves=True)
        with pytest.raises(ValueError, match="lsd_many_waves"):       # one camera for all streams
            images.ImagePipeline(ctx, B, CAMS[0], mp, op, lsd=ml.lsd_for(CAMS[0]), **kw)
        with pytest.raises(ValueError, match="lsd_many_waves"):       # no line detector
            images.ImagePipeline(ctx, B, CAMS, mp, op, **kw)
        with pytest.raises(ValueError, match="lsd_many_waves"):       # the FLD detector
            images.ImagePipeline(ctx, B, CAMS, mp, op, fld=capi.fld_params(10.0), lines_per_stream=True, **kw)
        with pytest.raises(ValueError):                               # lsd without the opt-in for key-lines per stream
            images.ImagePipeline(ctx, B, CAMS, mp, op, lsd=ml.lsd_for(), **kw)
        with pytest.raises(ValueError):                               # no list and no detector
            images.ImagePipeline(ctx, B, CAMS[0], mp, op, **kw)
    finally:
        ctx.close()
