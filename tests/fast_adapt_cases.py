"""The four stereo image streams of the adaptive FAST tests and their CPU chain: per frame the ORB oracle at the threshold the
previous frame left behind, then the oracle-driven per-frame pipeline (pipeline_ref.run_sequence with fast=), as tests/test_gpu_handler.py
chains them for one stream.  Computed once per process and shared, never modified."""
import functools

import numpy as np

import pipeline_ref
from stvo_amd import capi, synth
from stvo_amd.ctypes_types import match_params, opt_params

CAM = dict(synth.KITTI_CAM, width=640, height=240)   # the KITTI camera on small images: the CPU chain takes ~1 s per stream
N_FRAMES = 6
NFEATURES = 2000
MAX_KP = 2048     # the per-image capacity of the device pipeline (STVO_POSE_MAX_POINTS): at low thresholds more key-points than that qualify
                  # (retainBest keeps the ties at its cut) and both sides keep the first MAX_KP of the row-major order
TH0 = 20
STREAMS = ((50, {}), (51, dict(shift_per_disp=0.25)), (54, dict(shift_per_disp=0.1)), (77, {}))


def params():
    """config_kitti.yaml's rule as shipped.  (Stream 54 reaches max_th = 30 by two rises and then rises again — 244 inliers > 3 x 50 —
    which min(30, 35) cuts: the clip at max_th of the chain.)"""
    return capi.fast_adapt_params("kitti")


def ref_fast(prm, th0=TH0):
    return dict(adaptive=True, th0=th0, mn=prm.min_th, mx=prm.max_th, inc=prm.inc_th, feat=prm.feat_th, err=prm.err_th)


@functools.lru_cache(maxsize=None)
def images():
    """[stream][frame] = (left, right) uint8 [240, 640]"""
    return tuple(tuple(synth.make_stereo_image_sequence(seed, N_FRAMES, CAM, **kw)) for seed, kw in STREAMS)


_chain = {}


def cpu_chain(oracle):
    """[stream] = dict(th = the threshold every frame was DETECTED with [N_FRAMES], after = the threshold left behind by frame k >= 1
    (index k - 1), ref = run_sequence's per-frame outputs for frames 1 .., uncut = the key-points (left, right) of every frame that the
    ORB oracle emits when MAX_KP does not cut them)."""
    if "v" in _chain:
        return _chain["v"]
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=0)
    fast = ref_fast(params())
    pattern = oracle.orb_default_pattern()
    z4 = np.zeros((0, 4), np.float32); zd = np.zeros((0, 32), np.uint8)
    out = []
    for pairs in images():
        frames, th, ths, ref, uncut = [], fast["th0"], [], [], []
        for k, (left, right) in enumerate(pairs):
            ths.append(th)
            l = oracle.orb_detect_levels(left, nfeatures=NFEATURES, nlevels=1, fast_th=th, pattern=pattern, cap=MAX_KP)
            r = oracle.orb_detect_levels(right, nfeatures=NFEATURES, nlevels=1, fast_th=th, pattern=pattern, cap=MAX_KP)
            uncut.append(tuple(len(oracle.orb_detect_levels(im, nfeatures=NFEATURES, nlevels=1, fast_th=th, pattern=pattern, cap=1 << 16)["kp"])
                               for im in (left, right)))
            frames.append(dict(kp_l=l["kp"], oct_l=l["octave"], desc_l=l["desc"], kp_r=r["kp"], desc_r=r["desc"], kl_l=z4,
                               oct_ll=np.zeros(0, np.int32), ldesc_l=zd, kl_r=z4, ldesc_r=zd))
            if k:
                ref = pipeline_ref.run_sequence(oracle, frames, CAM, mp, op, fast=fast)
                th = ref[-1]["fast"]   # updateFrame's threshold for the NEXT detection
        out.append(dict(th=ths, after=[r["fast"] for r in ref], ref=ref, uncut=uncut))
    _chain["v"] = out
    return out
