#!/usr/bin/env python3
"""Mixed image sizes and cameras per stream: what the unchanged paths cost beside the parent commit, and what the new paths cost.
One JSON line per run.  python tools/bench_mixed_sizes.py --mode MODE [--tree DIR] [--iters N]

  orb-uniform     the ORB front-end, 256 KITTI-size images per launch, no size table (the path every existing caller takes)
  images-uniform  ImagePipeline with one camera dict at 128 streams: ms per enqueued step
  orb-mixed       256 images of the three KITTI sizes (1241 x 376, 1242 x 375, 1226 x 370) in 1242 x 376 slots with a size table, next to the
                  same images through three uniform detectors (86 + 85 + 85 images), one launch each
  ragged          eleven sequences of the KITTI odometry lengths (x --ragged-scale) with their three cameras on B = 4 streams through
                  ragged.run(cams=...), next to the same plan without cameras (every sequence generated under stream 0's camera)

  ab              the unchanged paths beside the parent commit: --runs (4) alternating child processes each of --parent-tree (a built
                  checkout of the parent commit) and of this tree, for orb-uniform, images-uniform and the default `python bench.py` line;
                  prints the "unchanged_paths" block of profiles/mixed_sizes_bench.json — per path the runs of both, the parent's min and
                  max, this tree's median and whether it lies inside (machines differ by a few per cent, so only alternation compares)

--tree DIR runs the first two modes against another checkout of the repository (its package and its built library); `ab` uses it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["orb-uniform", "images-uniform", "orb-mixed", "ragged", "ab"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--ragged-scale", type=float, default=1.0)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--runs", type=int, default=4)
a = ap.parse_args()
ROOT = os.path.abspath(a.tree)
if a.mode == "ab":
    import statistics
    import subprocess
    if not a.parent_tree:
        ap.error("--mode ab needs --parent-tree")
    here, parent = ROOT, os.path.abspath(a.parent_tree)

    def child(cmd):
        run = subprocess.run([sys.executable] + cmd, capture_output=True, text=True)
        if run.returncode != 0:
            sys.exit("bench_mixed_sizes: %s failed (%d)\n%s" % (" ".join(cmd), run.returncode, run.stderr[-2000:]))
        return json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    block = {}
    for name, key, cmd in (("orb", "ms_per_launch", lambda t: [os.path.abspath(__file__), "--mode", "orb-uniform", "--tree", t, "--iters", str(a.iters)]),
                           ("images", "ms_per_step", lambda t: [os.path.abspath(__file__), "--mode", "images-uniform", "--tree", t, "--iters", str(a.iters)]),
                           ("bench", "value", lambda t: [os.path.join(t, "bench.py"), "--gpus", "1"])):
        p, t = [], []
        for _ in range(a.runs):
            p.append(child(cmd(parent))[key])
            t.append(child(cmd(here))[key])
        block[name] = {"metric": key, "parent_runs": p, "this_runs": t, "parent_min": min(p), "parent_max": max(p),
                       "this_median": statistics.median(t), "inside_parent_min_max": min(p) <= statistics.median(t) <= max(p)}
    print(json.dumps({"unchanged_paths": block}))
    sys.exit(0)
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))
import torch  # noqa: E402
from stvo_amd import capi, synth  # noqa: E402
from stvo_amd.ctypes_types import match_params, opt_params  # noqa: E402

KITTI_SIZES = [(1241, 376), (1242, 375), (1226, 370)]
KITTI_LENGTHS = [4541, 1101, 4661, 801, 271, 2761, 1101, 1101, 4071, 1591, 1201]   # sequences 00 .. 10
KITTI_CAMS = [synth.KITTI_CAM] * 3 + [synth.KITTI03_CAM] + [synth.KITTI04_CAM] * 7
K = 2048


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


class OrbRun:
    def __init__(self, ctx, imgs, cols, rows, sizes=None):
        B = len(imgs)
        self.ctx, self.orb = ctx, capi.Orb(ctx, B, cols, rows, max_keypoints=K)
        if sizes is not None:
            self.orb.set_image_sizes(sizes)
        self.d = dict(img=torch.from_numpy(imgs).cuda(), kp=torch.zeros(B, K, 2, device="cuda"), resp=torch.zeros(B, K, device="cuda"),
                      ang=torch.zeros(B, K, device="cuda"), desc=torch.zeros(B, K, 32, dtype=torch.uint8, device="cuda"),
                      n=torch.zeros(B, dtype=torch.int32, device="cuda"))

    def __call__(self):
        d = self.d
        self.ctx._chk(self.ctx.lib.stvo_orb_detect_dev(self.orb.h, d["img"].data_ptr(), d["kp"].data_ptr(), d["resp"].data_ptr(),
                                                       d["ang"].data_ptr(), d["desc"].data_ptr(), d["n"].data_ptr()))


def scenes(n, cols=1242, rows=376):
    base = [synth.make_image(500 + k, cols=cols, rows=rows) for k in range(8)]
    return [np.roll(base[b % 8], 7 * (b // 8), axis=1) for b in range(n)]


out = dict(mode=a.mode, library=os.path.relpath(capi.LIB_PATH, ROOT))
if a.mode == "orb-uniform":
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    run = OrbRun(ctx, np.stack(scenes(256, 1241, 376)), 1241, 376)
    out.update(images_per_launch=256, ms_per_launch=timed(run, a.iters), mean_keypoints=float(run.d["n"].float().mean()))
elif a.mode == "images-uniform":
    from stvo_amd import images
    B = 128
    cam = synth.KITTI_CAM
    ctx = capi.Context(0, 2048, B)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    pipe = images.ImagePipeline(ctx, B, cam, match_params("kitti"), opt_params("kitti", has_lines=0), max_kp=K)
    pairs = [synth.make_stereo_image_sequence(50 + b, 2, cam) for b in range(4)]
    frames = [(torch.from_numpy(np.stack([pairs[b % 4][k][0] for b in range(B)])).cuda(),
               torch.from_numpy(np.stack([pairs[b % 4][k][1] for b in range(B)])).cuda()) for k in range(2)]
    state = dict(k=0)

    def step():
        left, right = frames[state["k"] & 1]
        pipe.set_images(left, right)
        pipe.enqueue()
        state["k"] += 1
    out.update(streams=B, ms_per_step=timed(step, a.iters, warm=4))
    res, counts = pipe.seq.read()
    out.update(mean_stereo_points=float(counts[:, 0].mean()), poses_ok=int((res["status"] == 0).sum()))
elif a.mode == "orb-mixed":
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    B = 256
    sc = scenes(B)
    # two entries per stereo pair would do; here every image names its own size, in the order 00-02, 03, 04-10 round robin
    sizes = [KITTI_SIZES[b % 3] for b in range(B)]
    slots = np.zeros((B, 376, 1242), np.uint8)
    for b, (c, r) in enumerate(sizes):
        slots[b, :r, :c] = sc[b][:r, :c]
    mixed = OrbRun(ctx, slots, 1242, 376, sizes)
    ms_mixed = timed(mixed, a.iters)
    n_mixed = mixed.d["n"].cpu().numpy()
    uni, n_uni = [], np.zeros(B, np.int32)
    for e, (c, r) in enumerate(KITTI_SIZES):
        members = [b for b in range(B) if b % 3 == e]
        uni.append((members, OrbRun(ctx, np.stack([np.ascontiguousarray(sc[b][:r, :c]) for b in members]), c, r)))

    def three():
        for _, u in uni:
            u()
    ms_uni = timed(three, a.iters)
    for members, u in uni:
        n_uni[members] = u.d["n"].cpu().numpy()
    out.update(images_per_launch=B, slot=[1242, 376], ms_mixed_one_launch=ms_mixed, ms_three_uniform_detectors=ms_uni,
               same_keypoint_counts=bool(np.array_equal(n_mixed, n_uni)), mean_keypoints=float(n_mixed.mean()))
else:
    from stvo_amd import ragged
    B = 4
    lengths = [max(1, int(round(n * a.ragged_scale))) for n in KITTI_LENGTHS]
    mp, op = match_params("kitti"), opt_params("kitti", has_lines=1)

    class Cycle:
        """a sequence of n frames that walks back and forth over a few generated ones"""

        def __init__(self, frames, n):
            self.f, self.n = frames, n

        def __len__(self):
            return self.n

        def __getitem__(self, k):
            p = 2 * (len(self.f) - 1)
            j = k % p
            return self.f[j if j < len(self.f) else p - j]

    def make(cams):
        return [Cycle(synth.make_stereo_sequence(synth.frame_seed(60 + i, 0), n_frames=6, n_pts=300, n_lines=40, cam=cams[i]), n)
                for i, n in enumerate(lengths)]

    def run(cams, with_cams):
        seqs = make(cams)
        ctx = capi.Context(0, 2048, B)
        dev = capi.Sequences(ctx, B, 512, 64, ragged.initial_cameras(lengths, B, cams), mp, op)
        try:
            t0 = time.perf_counter()
            res, _, _ = ragged.run(dev, seqs, cams=cams if with_cams else None)
            dt = time.perf_counter() - t0
        finally:
            dev.close(); ctx.close()
        return dt, sum(int((r["status"] == 0).sum()) for r in res)
    steps = ragged.plan(lengths, B)
    restarts = sum(int((st.control == ragged.STREAM_RESTART).sum()) for st in steps)
    dt_c, ok_c = run(KITTI_CAMS, True)
    dt_p, ok_p = run([KITTI_CAMS[0]] * len(lengths), False)
    out.update(streams=B, sequences=len(lengths), frames=sum(lengths), steps=len(steps), restarts=restarts,
               s_with_cameras=dt_c, ms_per_step_with_cameras=dt_c / len(steps) * 1e3, poses_ok_with_cameras=ok_c,
               s_one_camera=dt_p, ms_per_step_one_camera=dt_p / len(steps) * 1e3, poses_ok_one_camera=ok_p)
print(json.dumps(out))
