#!/usr/bin/env python3
"""Images in, poses out (bench.py's `images_to_poses` leg on its own): the ORB point front-end feeding the device-resident
per-frame pipeline for B stereo streams of KITTI-size images.
    python tools/bench_images.py [--streams 128] [--steps 8] [--adaptive-fast {kitti,euroc}]
--adaptive-fast runs the same leg twice — one fixed FAST threshold, then the reference's adaptative_fast per stream on the device
(ImagePipeline(adaptive_fast=...)) — and prints stereo pairs/s of both, the thresholds the streams ended on and the time of the
rule's kernel (events around back-to-back launches).  The thresholds change the number of key-points, so the two figures differ
by content as well as by the cost of the feature."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))

import bench  # noqa: E402


def leg(B, steps, adaptive):
    """bench.images_leg's workload and timed region (key-points only), with ImagePipeline's adaptive_fast.  A copy, because bench.py's
    leg takes no such argument: KEEP IT IN STEP with bench.images_leg — __main__ runs both at the fixed threshold and stops if they
    disagree on what they computed."""
    import numpy as np
    import torch
    from stvo_amd import capi, images, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    cam = synth.KITTI_CAM
    nf = 4
    base = [synth.make_stereo_image_sequence(900 + j, nf, cam) for j in range(2)]
    frames = torch.empty((nf, 2 * B, cam["height"], cam["width"]), dtype=torch.uint8, device="cuda:0")
    for k in range(nf):
        for side in (0, 1):
            for b in range(B):
                frames[k, side * B + b] = torch.from_numpy(np.roll(base[b % 2][k][side], 11 * (b // 2), axis=1))
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    pipe = images.ImagePipeline(ctx, B, cam, match_params("kitti"), opt_params("kitti", has_lines=0), max_kp=2048, adaptive_fast=adaptive)
    order = [0, 1, 2, 3, 2, 1]
    try:
        for k in (0, 1):
            pipe.enqueue(frames[k].data_ptr())
        pipe.seq.read()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            pipe.enqueue(frames[order[(i + 2) % len(order)]].data_ptr())
        res, counts = pipe.seq.read()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        out = {"streams": B, "stereo_pairs_per_s": B / dt, "ms_per_step": dt * 1e3, "mean_keypoints_per_image": float(pipe.n.float().mean()),
               "committed_pose_fraction_last_step": float((res["status"] == 0).mean()), "mean_matched_points_last_step": float(counts[:, 2].mean())}
        if adaptive is not None:
            th = pipe.fast_thresholds()
            out["fast_thresholds_min_mean_max"] = [int(th.min()), float(th.mean()), int(th.max())]
            keep = pipe.fast_th.clone()
            n = 200
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            pipe.seq.adapt_fast_dev(adaptive, pipe.fast_th)
            e0.record()
            for _ in range(n):
                pipe.seq.adapt_fast_dev(adaptive, pipe.fast_th)
            e1.record()
            torch.cuda.synchronize()
            pipe.fast_th.copy_(keep)
            out["adapt_kernel_us_per_launch_back_to_back"] = e0.elapsed_time(e1) / n * 1e3
    finally:
        pipe.close(); ctx.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--adaptive-fast", choices=("kitti", "euroc"), default=None)
    a = ap.parse_args()
    if a.adaptive_fast is None:
        print(json.dumps(bench.images_leg(0, B=a.streams, steps=a.steps)))
    else:
        from stvo_amd import capi
        fixed = bench.images_leg(0, B=a.streams, steps=a.steps)
        off = leg(a.streams, a.steps, None)
        for k in ("mean_keypoints_per_image", "committed_pose_fraction_last_step", "mean_matched_points_last_step"):
            if off[k] != fixed[k]:
                sys.exit(f"tools/bench_images.py: leg() no longer runs bench.images_leg's workload ({k}: {off[k]} against {fixed[k]})")
        on = leg(a.streams, a.steps, capi.fast_adapt_params(a.adaptive_fast))
        print(json.dumps({"adaptive_fast": a.adaptive_fast, "fixed_threshold": fixed, "fixed_threshold_this_tools_leg": off, "adaptive": on,
                          "pairs_per_s_fixed": fixed["stereo_pairs_per_s"], "pairs_per_s_adaptive": on["stereo_pairs_per_s"]}))
