"""LSD key-lines at lsd_scale 0.5 next to the shipped 1.2 (lsd_sigma_scale 0.6) on KITTI-size images: what the smaller scaled image
buys and what it costs in key-lines.  Per scale: LSD of one image, one stereo pair from images to pose with key-lines, images ->
poses with key-lines at the stream count of tools/bench_images.py, each with the key-line counts beside the time; and the blur +
resize stage alone at 256 images, which comes from a kernel trace (a run of its own: tracing slows the host).

    python tools/bench_lsd_scale.py --out lsd_scale_bench.json [--kernel-stats <rocprofv3 kernel_stats.csv>] [--ab-dir DIR]
    rocprofv3 --kernel-trace --stats -d lsd_scale_prof -- python tools/bench_lsd_scale.py --profile-only
    python tools/bench_lsd_scale.py --ab            # the figures at 1.2 only, one JSON line (runs unchanged on the parent commit)

--profile-only runs the detector once per scale on 256 images after a warm-up, nothing else; --kernel-stats adds the traced times of
the kernels that make the scaled image (orb_blur_kernel + orb_resize_kernel at 1.2, lsd_blur_resize_kernel at 0.5).  --ab-dir reads
parent_*.json / this_*.json, the --ab lines of alternating runs of the parent commit and this one, and records both spreads."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))

from stvo_amd import capi, images, synth  # noqa: E402
from stvo_amd.ctypes_types import match_params, opt_params  # noqa: E402

COLS, ROWS = 1241, 376
MIN_LENGTH = 0.025 * ROWS
SCALES = (1.2, 0.5)


def kitti_images(n):
    base = [synth.make_image(s, COLS, ROWS) for s in range(min(n, 8))]
    return np.stack([base[i % len(base)] for i in range(n)])


def lsd_batch(ctx, B, scale, iters, nfeatures=300):
    """stvo_lsd_detect_dev on B resident images: host clock around back-to-back calls that end in a synchronise."""
    import torch
    imgs = torch.as_tensor(kitti_images(B)).cuda()
    kl = torch.zeros((B, 300, 6), dtype=torch.float32, device="cuda")
    resp = torch.zeros((B, 300), dtype=torch.float32, device="cuda")
    nl = torch.zeros((B,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det = capi.Lsd(ctx, B, COLS, ROWS, capi.lsd_params(min_length=MIN_LENGTH, nfeatures=nfeatures, scale=scale), max_keylines=300)
    try:
        for _ in range(2):
            det.detect_dev(imgs.data_ptr(), kl.data_ptr(), resp.data_ptr(), nl.data_ptr())
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            det.detect_dev(imgs.data_ptr(), kl.data_ptr(), resp.data_ptr(), nl.data_ptr())
        ctx.synchronize()
        s = (time.perf_counter() - t0) / iters
        n_seg, n_pass = det.counts()
        return dict(ms_per_call=1e3 * s, images_per_s=B / s, mean_segments=float(n_seg.mean()), mean_longer_than_min_length=float(n_pass.mean()),
                    mean_keylines=float(nl.float().mean()))
    finally:
        det.close()


def pair_to_pose(scale, iters):
    """One stereo pair per step through ImagePipeline: ORB + LSD + LBD + stereo + f2f + pose, host-timed with a device synchronise
    after every step."""
    import torch
    cam = dict(synth.KITTI_CAM)
    pairs = synth.make_stereo_image_sequence(7, 4, cam)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=1)
    pipe = images.ImagePipeline(ctx, 1, cam, match_params("kitti"), opt_params("kitti", has_lines=1), max_kp=2048, max_kl=128,
                                lsd=capi.lsd_params(min_length=MIN_LENGTH, nfeatures=100, scale=scale))
    try:
        for k in range(4):
            pipe.push_images(pairs[k % 4][0][None], pairs[k % 4][1][None])
        ts, lines, matched, ok = [], [], [], []
        for k in range(iters):
            left, right = pairs[k % 4]
            t0 = time.perf_counter()
            res, counts = pipe.push_images(left[None], right[None])
            torch.cuda.synchronize(); ctx.synchronize()
            ts.append(time.perf_counter() - t0)
            lines.append(float(pipe.nl.float().mean())); matched.append(int(counts[0, 3])); ok.append(int(res["status"][0] == 0))
        return dict(ms_median=1e3 * float(np.median(ts)), ms_min=1e3 * float(np.min(ts)), mean_keylines_per_image=float(np.mean(lines)),
                    mean_matched_lines=float(np.mean(matched)), committed_pose_fraction=float(np.mean(ok)))
    finally:
        pipe.close()
        ctx.close()


def leg(B, steps, scale):
    """bench.images_leg(lines=True)'s workload and timed region with lsd_scale as an argument.  A copy, because bench.py's leg takes
    no such argument: KEEP IT IN STEP with bench.images_leg — main() runs both at 1.2 and stops if they disagree on what they computed."""
    import torch
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
    pipe = images.ImagePipeline(ctx, B, cam, match_params("kitti"), opt_params("kitti", has_lines=1), max_kp=2048,
                                lsd=capi.lsd_params(min_length=0.025 * cam["height"], nfeatures=100, scale=scale), max_kl=128)
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
        return {"streams": B, "stereo_pairs_per_s": B / dt, "ms_per_step": dt * 1e3, "mean_keypoints_per_image": float(pipe.n.float().mean()),
                "mean_keylines_per_image": float(pipe.nl.float().mean()), "committed_pose_fraction_last_step": float((res["status"] == 0).mean()),
                "mean_stereo_lines_last_step": float(counts[:, 1].mean()), "mean_matched_points_last_step": float(counts[:, 2].mean()),
                "mean_matched_lines_last_step": float(counts[:, 3].mean())}
    finally:
        pipe.close(); ctx.close()


def kernel_stats(path):
    """Average time per launch of the kernels that make the scaled image, from rocprofv3's kernel_stats.csv of a --profile-only run."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for key in ("orb_blur_kernel", "orb_resize_kernel", "lsd_blur_resize_kernel"):
                if key in name:
                    out[key] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3)
    return out


def ab_figures(iters, streams, steps):
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=4)
    try:
        one = lsd_batch(ctx, 1, 1.2, iters)
    finally:
        ctx.close()
    pair = pair_to_pose(1.2, iters)
    many = leg(streams, steps, 1.2)
    return dict(lsd_one_image_ms=one["ms_per_call"], pair_to_pose_ms_median=pair["ms_median"], pairs_per_s=many["stereo_pairs_per_s"])


def ab_spread(d):
    out = {}
    for side in ("parent", "this"):
        runs = [json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, side + "_*.json")))]
        out[side] = {k: [r[k] for r in runs] for k in (runs[0] if runs else {})}
    out["this_inside_parent_spread"] = {k: bool(min(out["parent"][k]) <= float(np.median(out["this"][k])) <= max(out["parent"][k]))
                                        for k in out["parent"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--ab-dir", default=None)
    a = ap.parse_args()
    if a.ab:
        print(json.dumps(ab_figures(a.iters, a.streams, a.steps)))
        return
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=4)
    try:
        if a.profile_only:
            for scale in SCALES:
                lsd_batch(ctx, 256, scale, 1)
            return
        res = dict(image=f"{COLS}x{ROWS} synth.make_image scenes", sigma_scale=0.6, min_length=MIN_LENGTH,
                   geometry={str(s): {k: (v.tolist() if hasattr(v, "tolist") else v)
                                      for k, v in capi.lsd_geometry(capi.lsd_params(scale=s), COLS, ROWS).items()} for s in SCALES})
        res["lsd_one_image_nfeatures_300"] = {str(s): lsd_batch(ctx, 1, s, a.iters) for s in SCALES}
        res["lsd_256_images_nfeatures_300"] = {str(s): lsd_batch(ctx, 256, s, 3) for s in SCALES}
    finally:
        ctx.close()
    res["stereo_pair_to_pose_nfeatures_100"] = {str(s): pair_to_pose(s, a.iters) for s in SCALES}
    import bench
    fixed = bench.images_leg(0, B=a.streams, steps=a.steps, lines=True)
    legs = {str(s): leg(a.streams, a.steps, s) for s in SCALES}
    for k in ("mean_keypoints_per_image", "committed_pose_fraction_last_step", "mean_matched_points_last_step", "mean_matched_lines_last_step"):
        if legs["1.2"][k] != fixed[k]:
            sys.exit(f"tools/bench_lsd_scale.py: leg() no longer runs bench.images_leg's workload ({k}: {legs['1.2'][k]} against {fixed[k]})")
    res["images_to_poses_with_keylines"] = legs
    if a.kernel_stats:
        res["blur_resize_stage_256_images_kernel_trace"] = kernel_stats(a.kernel_stats)
    if a.ab_dir:
        res["parent_and_this_commit_alternating_at_1.2"] = ab_spread(a.ab_dir)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
