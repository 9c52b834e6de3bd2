#!/usr/bin/env python3
"""The cost of orb_score 0 (HARRIS_SCORE ranking) next to orb_score 1 (FAST_SCORE) in the ORB point front-end: images per second of
stvo_orb_detect_levels_dev on the same images resident in HBM, ONE detector switched between the two rankings (stvo_orb_set_score_type)
in interleaved rounds of one process, at the shapes and the batch size of bench.py's ORB leg (KITTI size, one level, 2000 features;
EuRoC size, four levels at 1.2, 600 features; 256 images per launch).  Reports median and range per ranking.
    python tools/bench_orb_harris.py [--batch 256] [--rounds 7] [--iters 5] [--out profiles/orb_harris_bench.json]
    rocprofv3 --kernel-trace --stats -- python tools/bench_orb_harris.py --profile-only      (the per-kernel split of the Harris mode)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--profile-only", action="store_true", help="a few Harris-mode launches of both shapes and nothing else")
a = ap.parse_args()
import torch  # noqa: E402
from stvo_amd import capi, synth  # noqa: E402

B, K = a.batch, 2048
out = {"images_per_launch": B, "rounds": a.rounds, "launches_per_round": a.iters, "shapes": {}}
for name, cols, rows, nlev, nfeat in (("kitti_1_level", 1241, 376, 1, 2000), ("euroc_4_levels", 752, 480, 4, 600)):
    base = [synth.make_image(500 + k, cols=cols, rows=rows) for k in range(8)]
    imgs = np.stack([np.roll(base[b % 8], 7 * (b // 8), axis=1) for b in range(B)])
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    orb = capi.Orb(ctx, B, cols, rows, max_keypoints=K, nfeatures=nfeat, nlevels=nlev)
    d = dict(img=torch.from_numpy(imgs).cuda(), kp=torch.zeros(B, K, 2, device="cuda"), resp=torch.zeros(B, K, device="cuda"),
             ang=torch.zeros(B, K, device="cuda"), desc=torch.zeros(B, K, 32, dtype=torch.uint8, device="cuda"),
             n=torch.zeros(B, dtype=torch.int32, device="cuda"), oct=torch.zeros(B, K, dtype=torch.int32, device="cuda"),
             nt=torch.zeros(B, dtype=torch.int32, device="cuda"))

    def run():
        orb.detect_dev(d["img"].data_ptr(), d["kp"].data_ptr(), d["resp"].data_ptr(), d["ang"].data_ptr(), d["desc"].data_ptr(), d["n"].data_ptr(),
                       octave=d["oct"].data_ptr(), n_total=d["nt"].data_ptr())

    def timed(score, iters):
        orb.set_score_type(score)
        run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    try:
        if a.profile_only:
            timed(0, 3)
            continue
        ms = {0: [], 1: []}
        nk = {}
        for r in range(a.rounds):
            for score in ((1, 0) if r % 2 == 0 else (0, 1)):
                ms[score].append(timed(score, a.iters) * 1e3)
                nk[score] = float(d["n"].float().mean())
        rec = {"workload": f"{B} synthetic {cols} x {rows} images, orb_nfeatures {nfeat}, FAST threshold 20, {nlev} pyramid level(s)"}
        for score, label in ((1, "orb_score_1_fast"), (0, "orb_score_0_harris")):
            v = ms[score]
            rec[label] = {"ms_per_launch_median": statistics.median(v), "ms_per_launch_min": min(v), "ms_per_launch_max": max(v),
                          "images_per_s_median": B / statistics.median(v) * 1e3, "images_per_s_range": [B / max(v) * 1e3, B / min(v) * 1e3],
                          "mean_keypoints": nk[score]}
        rec["harris_over_fast_time"] = statistics.median(ms[0]) / statistics.median(ms[1])
        out["shapes"][name] = rec
    finally:
        orb.close(); ctx.close()
if not a.profile_only:
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
