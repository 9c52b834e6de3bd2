#!/usr/bin/env python3
"""Colour frames in: what the grey conversion, the fused colour rectification and colour input to images -> poses cost on one MI355X.

    python tools/bench_color_input.py [--parent-tree /path/to/built/parent/checkout] --out profiles/color_input_bench.json

  conversion      stvo_color_to_gray_dev on KITTI-size images (1241 x 376), 256 and 6144 images per launch, 3 and 4 channels, one
                  plane and two: time per launch and achieved bytes/s (source read once, every plane written once), next to a
                  device-to-device copy of the same byte count timed in the same process (the yardstick: a copy moves every byte it
                  counts twice, so its figure is bytes copied x 2 / time).
  fused           raw colour pairs at EuRoC size (752 x 480, the shipped calibration): stvo_rectify_color_to_gray_dev against
                  stvo_rectify_color_images_dev followed by stvo_color_to_gray_dev, alternating in one process.
  images          ImagePipeline (key-points only, KITTI size, bench.py's images leg scenes) at 128 and 3072 streams: colour frames in
                  against the grey planes of the same frames in; one process per leg, the added time per step.
  vs_parent       with --parent-tree: the headline step (tools/bench_trajectory.py's step leg) and the images leg with grey input on the
                  parent commit's built checkout against this tree, alternating runs, one process each; this tree's median must lie
                  inside the parent's spread (not above its slowest run).

Timing: host clock around `iters` back-to-back launches ended by a stream synchronisation, after a warm-up; medians of `repeats`
groups."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KITTI = (376, 1241)


def use_tree(tree):
    sys.path.insert(0, os.path.join(tree, "stvo-pl_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(ctx, fn, iters, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    groups = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        ctx.synchronize()
        groups.append((time.perf_counter() - t0) / iters)
    return float(np.median(groups)), [float(g) for g in groups]


def conversion_leg(a):
    import torch
    from stvo_amd import capi
    ctx = capi.Context(device_id=0, max_rows=256, max_batch=1)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)  # the copies below ride torch's stream: one stream for both
    rows, cols = KITTI
    out = []
    for n in (256, 6144):
        for ch in (3, 4):
            src = torch.randint(0, 256, (n, rows, cols, ch), dtype=torch.uint8, device="cuda")
            pa, pb = (torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda") for _ in range(2))
            iters = max(3, a.iters * 256 // n)
            for planes in (1, 2):
                moved = n * rows * cols * (ch + planes)
                t, groups = timed(ctx, lambda: capi.color_to_gray_dev(ctx, n, rows, cols, ch, src.data_ptr(), pa.data_ptr(),
                                                                      pb.data_ptr() if planes == 2 else None), iters, a.repeats)
                half = moved // 2
                flat = src.view(-1)
                dst = torch.empty(half, dtype=torch.uint8, device="cuda")
                tc, _ = timed(ctx, lambda: dst.copy_(flat[:half]), iters, a.repeats)
                out.append(dict(images_per_launch=n, channels=ch, planes=planes, ms_per_launch=t * 1e3, ms_groups=[g * 1e3 for g in groups],
                                bytes_moved=moved, achieved_GBps=moved / t / 1e9, images_per_s=n / t,
                                copy_same_bytes=dict(bytes_read_plus_written=2 * half, ms=tc * 1e3, achieved_GBps=2 * half / tc / 1e9),
                                share_of_copy_rate=(moved / t) / (2 * half / tc)))
                del dst
            del src, pa, pb
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(out))


def fused_leg(a):
    import torch
    from stvo_amd import capi
    c = capi.read_dataset_params(os.path.join(ROOT, "tests", "golden", "dataset_params", "euroc_params.yaml"))
    ctx = capi.Context(device_id=0, max_rows=256, max_batch=1)
    px = c.width * c.height
    out = []
    for n in (1, 64, 1024):
        for ch in (3, 4):
            rect = capi.Rectifier(ctx, n, calib=c)
            src = torch.randint(0, 256, (2 * n, c.height, c.width, ch), dtype=torch.uint8, device="cuda")
            col = torch.empty_like(src)
            gray = torch.empty((2, 2 * n, c.height, c.width), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            s, d, ga, gb = src.data_ptr(), col.data_ptr(), gray[0].data_ptr(), gray[1].data_ptr()
            iters = max(3, a.iters * 16 // max(16, n))
            row = dict(pairs=n, channels=ch)
            for planes in (1, 2):
                b_l, b_r = (gb, gb + n * px) if planes == 2 else (None, None)

                def fused():
                    rect.rectify_color_to_gray_dev(n, ch, s, s + n * px * ch, ga, ga + n * px, b_l, b_r)

                def two_step():
                    rect.rectify_color_dev(n, ch, s, s + n * px * ch, d, d + n * px * ch)
                    capi.color_to_gray_dev(ctx, 2 * n, c.height, c.width, ch, d, ga, gb if planes == 2 else None)

                tf, tt = [], []
                for _ in range(a.repeats):  # alternating groups
                    tf.append(timed(ctx, fused, iters, 1)[0])
                    tt.append(timed(ctx, two_step, iters, 1)[0])
                row[f"planes_{planes}"] = dict(fused_ms=float(np.median(tf)) * 1e3, two_step_ms=float(np.median(tt)) * 1e3,
                                               fused_over_two_step=float(np.median(tf) / np.median(tt)),
                                               fused_pairs_per_s=n / float(np.median(tf)))
            out.append(row)
            rect.close()
            del src, col, gray
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(out))


def images_leg(a):
    """bench.py's images leg scenes (two base sequences rolled over the streams), two frames resident, steps alternating between them.
    channels 3 / 4: the scenes through three tone curves (tests/test_gpu_color.py's colorize); channels 1: the BGR-weighted grey of
    those colour frames, so both legs detect on the same planes."""
    import torch
    import np_color as nc
    from stvo_amd import capi, images, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    cam, B, ch = synth.KITTI_CAM, a.streams, a.channels

    def colorize(img):
        x = img.astype(np.float64) / 255.0
        planes = [img, np.rint(255.0 * x ** 0.7).astype(np.uint8), np.rint(255.0 * x ** 1.6).astype(np.uint8)]
        return np.stack(planes + [img] * (a.color_channels - 3), -1)

    nf = 2
    base = [synth.make_stereo_image_sequence(900 + j, nf, cam) for j in range(2)]
    shape = (nf, 2 * B, cam["height"], cam["width"]) + ((ch,) if ch != 1 else ())
    frames = torch.empty(shape, dtype=torch.uint8, device="cuda:0")
    for k in range(nf):
        for side in (0, 1):
            for j in range(2):
                col = colorize(base[j][k][side])
                one = torch.from_numpy(col if ch != 1 else nc.gray(col)).cuda()
                for b in range(j, B, 2):
                    frames[k, side * B + b] = torch.roll(one, 11 * (b // 2), dims=1)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    kw = dict(channels=ch) if ch != 1 else {}  # (the parent commit's ImagePipeline has no such argument)
    pipe = images.ImagePipeline(ctx, B, cam, match_params("kitti"), opt_params("kitti", has_lines=0), max_kp=2048, **kw)
    try:
        k = 0
        for _ in range(a.warmup):
            pipe.enqueue(frames[k & 1].data_ptr()); k += 1
        pipe.seq.read()
        torch.cuda.synchronize()
        groups = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                pipe.enqueue(frames[k & 1].data_ptr()); k += 1
            torch.cuda.synchronize()
            groups.append((time.perf_counter() - t0) / a.steps * 1e3)
        res, counts = pipe.seq.read()
        out = dict(streams=B, channels=ch, ms_per_step_groups=groups, ms_per_step_median=float(np.median(groups)),
                   stereo_pairs_per_s=B / float(np.median(groups)) * 1e3, mean_keypoints_per_image=float(pipe.n.float().mean()),
                   committed_pose_fraction_last_step=float((res["status"] == 0).mean()), mean_matched_points_last_step=float(counts[:, 2].mean()))
    finally:
        pipe.close(); ctx.close()
    print(json.dumps(out))


def spawn(tree, leg, a, streams=0, channels=1):
    env = dict(os.environ)
    env.pop("STVO_LIB", None)
    if leg == "step":  # the headline step: tools/bench_trajectory.py's leg, the loop of the earlier feature rows
        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_trajectory.py"), "--leg", "step", "--streams", str(streams), "--trajectory", "off",
               "--tree", tree]
    else:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", tree, "--streams", str(streams), "--channels", str(channels),
               "--color-channels", str(a.color_channels), "--iters", str(a.iters), "--repeats", str(a.repeats), "--steps", str(a.steps),
               "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def against_parent(a, leg, streams, rounds):
    runs = {"parent": [], "this": []}
    for _ in range(rounds):  # parent, this, parent, this, ...
        for side, tree in (("parent", a.parent_tree), ("this", ROOT)):
            runs[side].append(spawn(tree, leg, a, streams)["ms_per_step_median"])
        print(leg, streams, "parent", runs["parent"][-1], "this", runs["this"][-1], flush=True)
    med = float(np.median(runs["this"]))
    return dict(streams=streams, ms_per_step_runs=runs, parent_median_min_max=[float(np.median(runs["parent"])), min(runs["parent"]), max(runs["parent"])],
                this_median_min_max=[med, min(runs["this"]), max(runs["this"])],
                gate=dict(statement="this tree's median ms per step is not above the parent's slowest run", this_median=med,
                          parent_slowest_run=max(runs["parent"]), holds=bool(med <= max(runs["parent"]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["conversion", "fused", "images"], default=None)
    ap.add_argument("--tree", default=ROOT, help="checkout whose python package and library a leg uses")
    ap.add_argument("--parent-tree", default=None, help="built checkout of the parent commit, for vs_parent")
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--shapes", default="128,3072")
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--color-channels", type=int, default=3, help="channels of the colour frames of the images legs")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-step-streams", type=int, default=3072)
    ap.add_argument("--parent-images-streams", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        use_tree(a.tree)
        {"conversion": conversion_leg, "fused": fused_leg, "images": images_leg}[a.leg](a)
        return
    doc = dict(what="colour frames in on one MI355X: the grey conversion against a device copy of the same bytes, the fused colour "
                    "rectification against remap-then-convert, images -> poses with colour frames against the same frames as grey planes, "
                    "and grey input against the parent commit",
               timing=f"host clock around back-to-back launches ended by a stream synchronisation, after a warm-up; medians of {a.repeats} groups; "
                      "every leg a process of its own")
    doc["conversion"] = spawn(ROOT, "conversion", a)
    print("conversion", json.dumps(doc["conversion"]), flush=True)
    doc["fused_vs_two_step"] = spawn(ROOT, "fused", a)
    print("fused", json.dumps(doc["fused_vs_two_step"]), flush=True)
    doc["images_to_poses"] = []
    for B in [int(s) for s in a.shapes.split(",")]:
        legs = {"gray": spawn(ROOT, "images", a, B, 1), "color": spawn(ROOT, "images", a, B, a.color_channels)}
        g, c = legs["gray"]["ms_per_step_median"], legs["color"]["ms_per_step_median"]
        same = all(legs["gray"][k] == legs["color"][k] for k in ("mean_keypoints_per_image", "committed_pose_fraction_last_step",
                                                                 "mean_matched_points_last_step"))
        doc["images_to_poses"].append(dict(streams=B, legs=legs, added_ms_per_step=c - g, added_percent=100.0 * (c - g) / g,
                                           added_us_per_stereo_pair=1e3 * (c - g) / B, same_features_and_poses=same))
        print("images", B, g, c, same, flush=True)
    if a.parent_tree:
        doc["vs_parent"] = dict(headline_step=against_parent(a, "step", a.parent_step_streams, a.rounds),
                                image_pipeline_gray=against_parent(a, "images", a.parent_images_streams, a.rounds))
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
