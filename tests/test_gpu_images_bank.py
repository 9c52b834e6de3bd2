"""Raw frames -> poses with one camera, image size AND rectification per stream: ImagePipeline(cam=[B dicts], rectify=RectifierBank,
calibs=[...]).  Three streams on three calibrations in slots of 320 x 128 — a dist 0 calibration (the reference copies), a rad-tan
one from stvo_rectify_compute with EuRoC's coefficients at a scaled focal length, one from seeded caller maps — fed raw grey frames and raw
B, G, R frames over a few steps; stream 1 then RESTARTs into a fourth calibration of another size (300 x 120, KITTI form with
distortion).  The judge is an ImagePipeline(cam=[...]) WITHOUT rectifier fed the crops rectified (and greyed) in numpy — np_rectify.remap,
np_color.remap_color, np_color.gray with each calibration's own maps: results and counts of every stream and step are equal byte for
byte.  Sizes and scenes are those of tests/test_gpu_images_mixed.py."""
import os

import numpy as np
import pytest

import np_color
import np_rectify as nr
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_images_mixed import CAMS, NEW_CAM, SETS, SIZES, sequence

pytestmark = pytest.mark.gpu
B = 3
RUN, RESTART = 0, 1
SLOT = (320, 128)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def calibrations():
    """-> [(Rectifier keyword arguments, (map1, map2) or None for the copy)] of the four calibrations, sizes SIZES + the new one"""
    from stvo_amd import capi
    out = []
    # 0: KITTI form, d0 = 0: dist 0, a copy
    c = capi.RectCalib()
    c.form, c.width, c.height, c.b = capi.RECT_FORM_KITTI, SIZES[0][0], SIZES[0][1], synth.KITTI_CAM["b"]
    c.fx, c.fy, c.cx, c.cy = 185.0, 185.0, 160.0, 64.0
    c.d[:] = [0.0, 0.0, 0.0, 0.0]
    out.append((dict(calib=c), None))
    # 1: rad-tan, EuRoC's distortion, rotation and baseline with the intrinsics scaled to 316 x 124
    e = capi.read_dataset_params(os.path.join(ROOT, "tests", "golden", "dataset_params", "euroc_params.yaml"))
    s, (w, h) = SIZES[1][0] / e.width, SIZES[1]   # one scale for both axes, the principal points kept where they were from the centre
    e.Kl[:] = [e.Kl[0] * s, e.Kl[1] * s, w / 2 + (e.Kl[2] - e.width / 2) * s, h / 2 + (e.Kl[3] - e.height / 2) * s]
    e.Kr[:] = [e.Kr[0] * s, e.Kr[1] * s, w / 2 + (e.Kr[2] - e.width / 2) * s, h / 2 + (e.Kr[3] - e.height / 2) * s]
    e.width, e.height = w, h
    cam, m1, m2 = capi.rectify_compute(e)
    assert cam["dist"] == 1
    out.append((dict(calib=e), (m1, m2)))
    # 2: seeded caller maps at 256 x 128: a gentle warp, another one per side
    cols, rows = SIZES[2]
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    sides = []
    for side in range(2):
        a, p = rng.uniform(0.8, 1.6, 2), rng.uniform(0, 6, 2)
        sides.append(nr.encode(xx + a[0] * np.sin(yy / 19.0 + p[0]) - 0.7, yy + a[1] * np.sin(xx / 31.0 + p[1]) + 0.4))
    m1, m2 = np.stack([s[0] for s in sides]), np.stack([s[1] for s in sides])
    out.append((dict(maps=(m1, m2)), (m1, m2)))
    # 3: KITTI form with distortion at 300 x 120
    k = capi.RectCalib()
    k.form, k.width, k.height, k.b = capi.RECT_FORM_KITTI, NEW_CAM["width"], NEW_CAM["height"], NEW_CAM["b"]
    k.fx, k.fy, k.cx, k.cy = 175.0, 175.0, 149.0, 61.0
    k.d[:] = [-0.12, 0.03, 0.0005, -0.0004]
    cam, m1, m2 = capi.rectify_compute(k)
    assert cam["dist"] == 1
    out.append((dict(calib=k), (m1, m2)))
    return out


def colour_of(img):
    """a B, G, R frame made from a grey one: three different channels, every one with the scene's texture"""
    return np.stack([img, 255 - img, np.roll(img, 3, axis=1) // 2 + 60], -1).astype(np.uint8)


def rectified(img, maps, side):
    if maps is None:
        return img.copy()
    if img.ndim == 2:
        return nr.remap(img, maps[0][side], maps[1][side])
    return np_color.remap_color(img, maps[0][side], maps[1][side])


def same(got, want, where):
    assert got[0].tobytes() == want[0].tobytes(), where
    assert np.array_equal(got[1], want[1]), where


@pytest.mark.parametrize("channels", [1, 3])
def test_raw_frames_of_three_calibrations_and_a_restart_into_a_fourth(channels):
    import torch
    from stvo_amd import capi, images
    S = SETS["small"]
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=0)
    nf = 3 if channels == 1 else 2
    seqs = [sequence(S["scenes"][b], CAMS[b], nf + 3) for b in range(B)]
    new_seq = sequence(S["new_scene"], NEW_CAM, 3)[:2]
    cal = calibrations()
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    rects = bank = pipe = ref = None
    try:
        rects = [capi.Rectifier(ctx, B, **kw) for kw, _ in cal]
        assert [(r.cols, r.rows) for r in rects] == SIZES + [(NEW_CAM["width"], NEW_CAM["height"])] and [r.dist for r in rects] == [0, 1, 1, 1]
        bank = capi.RectifierBank(ctx, B, SLOT[0], SLOT[1], rects)
        pipe = images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=2048, rectify=bank, calibs=[0, 1, 2], channels=channels)
        ref = images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=2048)
        assert (pipe.cols, pipe.rows) == SLOT and pipe.calibs == [0, 1, 2]
        # hostile slots: whatever lies beyond an image must not matter, in the raw buffer and in the rectified one
        noise = np.random.default_rng(5)
        for buf in (pipe.img, pipe.rect_img, pipe.color):
            if buf is not None:
                buf.copy_(torch.as_tensor(noise.integers(0, 256, tuple(buf.shape)).astype(np.uint8)))

        def raw(frame):
            return frame if channels == 1 else colour_of(frame)

        def judged(frame, k, side):
            r = rectified(raw(frame), cal[k][1], side)
            return r if channels == 1 else np_color.gray(r, "bgr", "q14")

        def step(frames, calibs_now, **kw):
            """frames: B (left, right); -> what the bank pipeline and the judge return"""
            got = pipe.push_images([raw(f[0]) for f in frames], [raw(f[1]) for f in frames], **kw)
            kw.pop("calibs", None)
            want = ref.push_images([judged(f[0], calibs_now[b], 0) for b, f in enumerate(frames)],
                                   [judged(f[1], calibs_now[b], 1) for b, f in enumerate(frames)], **kw)
            return (got[0].copy(), got[1].copy()), (want[0].copy(), want[1].copy())

        stereo = np.zeros(B, np.int64)
        for k in range(nf):
            got, want = step([seqs[b][k] for b in range(B)], [0, 1, 2])
            same(got, want, ("step", k))
            stereo += got[1][:, 0]
        print("stereo points per stream over", nf, "steps:", stereo.tolist())
        assert stereo[0] > 0, stereo                 # (the copied stream: the scene as tests/test_gpu_images_mixed.py sees it)
        # a calibration whose size disagrees with the camera of its stream: refused, and nothing is staged — the next step runs
        # every stream on, as the judge's does
        frames = [seqs[0][nf], new_seq[0], seqs[2][nf]]
        with pytest.raises(ValueError):
            pipe.push_images([raw(f[0]) for f in frames], [raw(f[1]) for f in frames], control=[RUN, RESTART, RUN],
                             cams=[None, NEW_CAM, None], calibs=[None, 0, None])
        with pytest.raises(ValueError):
            pipe.enqueue(control=[RUN, RESTART, RUN], cams=[None, NEW_CAM, None])             # a camera of another size without its calibration
        with pytest.raises(ValueError):
            pipe.enqueue(control=[RUN, RESTART, RUN], calibs=[None, 3, None])                  # a calibration of another size without its camera
        with pytest.raises(ValueError):
            pipe.enqueue(calibs=[None, 1, None])                                               # calibrations without a control
        with pytest.raises(ValueError):
            pipe.enqueue(control=[RUN, RESTART, RUN], cams=[None, CAMS[1], None], calibs=[None, 4, None])   # not a calibration of the bank
        assert pipe.calibs == [0, 1, 2] and pipe.cams == CAMS and bank.calibs == [0, 1, 2]
        got, want = step([seqs[b][nf] for b in range(B)], [0, 1, 2])
        same(got, want, "the step behind the refusals")
        zero = np.zeros(1, got[0].dtype).tobytes()
        assert all(got[0][b].tobytes() != zero for b in range(B))           # nobody restarted: no first-frame record
        # stream 1 begins a sequence of another camera, size and calibration; the others run on
        for k in range(2):
            frames = [seqs[0][nf + 1 + k], new_seq[k], seqs[2][nf + 1 + k]]
            kw = dict(control=[RUN, RESTART, RUN], cams=[None, NEW_CAM, None], calibs=[None, 3, None]) if k == 0 else {}
            got, want = step(frames, [0, 3, 2], **kw)
            same(got, want, ("behind the restart", k))
            if k == 0:
                assert got[0][1].tobytes() == np.zeros(1, got[0].dtype).tobytes() and not got[1][1, 2:].any()   # a first frame
        assert pipe.calibs == [0, 3, 2] and bank.calibs == [0, 3, 2] and pipe.cams[1] == NEW_CAM
    finally:
        for o in (pipe, ref, bank):
            if o is not None:
                o.close()
        for r in rects or []:
            r.close()
        ctx.close()


def test_the_refusals_with_a_list_of_cameras_stay():
    from stvo_amd import capi, images
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=0)
    cal = calibrations()
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    rects = bank = None
    try:
        rects = [capi.Rectifier(ctx, B, **kw) for kw, _ in cal]
        bank = capi.RectifierBank(ctx, B, SLOT[0], SLOT[1], rects)
        for name, kw in (("rectify", dict(rectify=object())), ("rectify", dict(rectify=rects[0])), ("channels", dict(channels=3)),
                         ("lsd", dict(lsd=capi.lsd_params(nfeatures=50))), ("fld", dict(fld=capi.fld_params(10.0))),
                         ("lsd", dict(lsd=capi.lsd_params(nfeatures=50), rectify=bank, calibs=[0, 1, 2])),
                         ("fld", dict(fld=capi.fld_params(10.0), rectify=bank, calibs=[0, 1, 2]))):
            with pytest.raises(ValueError, match=name):
                images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256, **kw)
        for kw in (dict(rectify=bank), dict(rectify=bank, calibs=[0, 1]), dict(rectify=bank, calibs=[0, 1, 4]), dict(rectify=bank, calibs=[1, 1, 2]),
                   dict(calibs=[0, 1, 2])):
            with pytest.raises(ValueError):                                   # no calibs, too few, out of range, a size that disagrees, no bank
                images.ImagePipeline(ctx, B, CAMS, mp, op, max_kp=256, **kw)
        with pytest.raises(ValueError):
            images.ImagePipeline(ctx, B, CAMS[0], mp, op, max_kp=256, rectify=bank, calibs=[0, 0, 0])   # one dict: nothing changes, no bank
    finally:
        if bank is not None:
            bank.close()
        for r in rects or []:
            r.close()
        ctx.close()
