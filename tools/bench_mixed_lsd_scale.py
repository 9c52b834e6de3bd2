#!/usr/bin/env python3
"""Key-lines on mixed image sizes at lsd_scale 0.5 (blur radius 5: the fused blur + resize under a size table): what the unchanged paths
cost beside the parent commit, and what the new paths cost.  One JSON line per run.
python tools/bench_mixed_lsd_scale.py --mode MODE [--tree DIR] [--iters N] [--scale S]

  lsd-uniform     the LSD detector, 256 KITTI-size images per launch, no size table, at --scale (1.2: the two ORB kernels; 0.5: the uniform
                  instance of the fused kernel)
  images-uniform  ImagePipeline with lsd (1.2) and one camera dict at 128 streams: ms per enqueued step
  lsd-mixed       256 images of the three KITTI sizes (1241 x 376, 1242 x 375, 1226 x 370) in 1242 x 376 slots at lsd_scale 0.5 with a size
                  table and each size's own minimum length, next to the same images through three uniform detectors at 0.5 (86 + 85 + 85
                  images), one launch each
  images-mixed    ImagePipeline(cam=[128 dicts], lsd, lines_per_stream) over the three KITTI cameras at lsd_scale 0.5, next to the same at 1.2:
                  ms per enqueued step
  kernel-profile  for a run under  rocprofv3 --kernel-trace --stats : 256 full 1242 x 376 slots at 0.5 through a detector with a table of
                  the slot's own size (the MIXED instance of the fused kernel) and through one without (the uniform instance)

  ab              the unchanged paths beside the parent commit: --runs (4) alternating child processes each of --parent-tree (a built
                  checkout of the parent commit) and of this tree, for the legs of --legs (lsd12, lsd05, images, bench)
  new             the two new-path modes, one JSON document
  assemble        --parts FILE... (the documents of ab and new runs, and --kernel-stats, rocprofv3's kernel_stats.csv of a kernel-profile
                  run) into --out, as profiles/mixed_lsd_scale_bench.json is laid out

--tree DIR runs the first two modes against another checkout of the repository (its package and its built library); `ab` uses it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["lsd-uniform", "images-uniform", "lsd-mixed", "images-mixed", "kernel-profile", "ab", "new", "assemble"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.2)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--child-timeout", type=int, default=300, help="seconds a child process of ab / new may take")
ap.add_argument("--legs", default="lsd12,lsd05,images,bench")
ap.add_argument("--parts", nargs="*", default=[])
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
ROOT = os.path.abspath(a.tree)


def emit(doc):
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))
    sys.exit(0)


if a.mode in ("ab", "new"):
    import statistics
    import subprocess
    me = os.path.abspath(__file__)

    def child(cmd):
        try:   # (a child that hangs must not hang the alternation)
            run = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=a.child_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("bench_mixed_lsd_scale: %s ran longer than %d s" % (" ".join(cmd), a.child_timeout))
        if run.returncode != 0:
            sys.exit("bench_mixed_lsd_scale: %s failed (%d)\n%s" % (" ".join(cmd), run.returncode, run.stderr[-2000:]))
        return json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    if a.mode == "new":
        emit({"new_paths": {"lsd_256_images_three_kitti_sizes_at_0.5": child([me, "--mode", "lsd-mixed", "--iters", str(a.iters)]),
                            "images_128_streams_lines_per_stream_0.5_against_1.2": child([me, "--mode", "images-mixed", "--iters", str(a.iters)])}})
    if not a.parent_tree:
        ap.error("--mode ab needs --parent-tree")
    here, parent = ROOT, os.path.abspath(a.parent_tree)
    legs = {"lsd12": ("lsd_256_images_no_table_1.2", "ms_per_launch", lambda t: [me, "--mode", "lsd-uniform", "--scale", "1.2", "--tree", t, "--iters", str(a.iters)]),
            "lsd05": ("lsd_256_images_no_table_0.5", "ms_per_launch", lambda t: [me, "--mode", "lsd-uniform", "--scale", "0.5", "--tree", t, "--iters", str(a.iters)]),
            "images": ("images_128_streams_one_camera", "ms_per_step", lambda t: [me, "--mode", "images-uniform", "--tree", t, "--iters", str(a.iters)]),
            "bench": ("bench", "value", lambda t: [os.path.join(t, "bench.py"), "--gpus", "1"])}
    block = {}
    for leg in a.legs.split(","):
        name, key, cmd = legs[leg]
        p, t = [], []
        for _ in range(a.runs):
            p.append(child(cmd(parent))[key])
            t.append(child(cmd(here))[key])
            print(name, "run", len(t), p[-1], t[-1], file=sys.stderr, flush=True)
        block[name] = {"metric": key, "parent_runs": p, "this_runs": t, "parent_min": min(p), "parent_max": max(p),
                       "this_median": statistics.median(t), "inside_parent_min_max": min(p) <= statistics.median(t) <= max(p)}
    emit({"unchanged_paths": block})
if a.mode == "assemble":
    import csv
    doc = {"what": "key-lines on mixed image sizes at lsd_scale 0.5 on one MI355X: tools/bench_mixed_lsd_scale.py (unchanged_paths: --mode ab, "
                   "alternating child processes of the parent commit and this one; new_paths: --mode new" +
                   ("; the fused kernel alone: a rocprofv3 kernel trace of --mode kernel-profile)" if a.kernel_stats else ")"),
           "unchanged_paths": {}, "new_paths": {}}
    for path in a.parts:
        with open(path) as f:
            part = json.load(f)
        for k in ("unchanged_paths", "new_paths"):
            doc[k].update(part.get(k, {}))
    if a.kernel_stats:
        rows = {}
        with open(a.kernel_stats, newline="") as f:
            for row in csv.DictReader(f):
                if "lsd_blur_resize_kernel" in row.get("Name", ""):
                    rows[row["Name"]] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3)
        doc["new_paths"]["fused_kernel_alone_256_full_slots_at_0.5_kernel_trace"] = rows
    emit(doc)

sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))
import torch  # noqa: E402
from stvo_amd import capi, synth  # noqa: E402
from stvo_amd.ctypes_types import match_params, opt_params  # noqa: E402

KITTI_SIZES = [(1241, 376), (1242, 375), (1226, 370)]
KITTI_CAMS = [dict(synth.KITTI_CAM, width=1241, height=376), dict(synth.KITTI03_CAM, width=1242, height=375),
              dict(synth.KITTI04_CAM, width=1226, height=370)]
M, NLINES, RATIO = 128, 100, 0.025


def timed(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


class LsdRun:
    def __init__(self, ctx, imgs, cols, rows, scale, sizes=None, min_lengths=None):
        B = len(imgs)
        kw = dict(sizes_any_radius=True) if sizes is not None else {}   # (the keyword does not exist in the parent tree, which sets no table)
        self.lsd = capi.Lsd(ctx, B, cols, rows, capi.lsd_params(min_length=RATIO * min(cols, rows), nfeatures=NLINES, scale=scale, **kw), max_keylines=M)
        if sizes is not None:
            self.lsd.set_image_sizes(sizes, min_lengths)
        self.d = dict(img=torch.from_numpy(imgs).cuda(), rec=torch.zeros(B, M, 6, device="cuda"), n=torch.zeros(B, dtype=torch.int32, device="cuda"))

    def __call__(self):
        self.lsd.detect_dev(self.d["img"].data_ptr(), self.d["rec"].data_ptr(), None, self.d["n"].data_ptr())


def scenes(n, cols=1242, rows=376):
    base = [synth.make_image(500 + k, cols=cols, rows=rows) for k in range(8)]
    return [np.roll(base[b % 8], 7 * (b // 8), axis=1) for b in range(n)]


def pipeline_ms(cams, iters, scale, **kw):
    """ImagePipeline with lsd at len(cams) streams (one dict: 128 streams of it): ms per enqueued step, and what the last step gave"""
    from stvo_amd import images
    one = isinstance(cams, dict)
    B = 128 if one else len(cams)
    ctx = capi.Context(0, 2048, B)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    cam0 = cams if one else cams[0]
    lsd = capi.lsd_params(min_length=RATIO * min(cam0["width"], cam0["height"]), nfeatures=NLINES, scale=scale)
    pipe = images.ImagePipeline(ctx, B, cams, match_params("kitti"), opt_params("kitti", has_lines=1), max_kp=2048, lsd=lsd, max_kl=M, **kw)
    kinds = [cams] if one else KITTI_CAMS
    pairs = {(e, s): synth.make_stereo_image_sequence(50 + s, 2, c) for e, c in enumerate(kinds) for s in range(2)}
    frames = []
    for k in range(2):
        for side in range(2):
            buf = np.zeros((B, pipe.rows, pipe.cols), np.uint8)
            for b in range(B):
                im = pairs[(0 if one else b % 3, (b // 3) % 2)][k][side]
                buf[b, :im.shape[0], :im.shape[1]] = im
            frames.append(torch.from_numpy(buf).cuda())
    state = dict(k=0)

    def step():
        k = state["k"] & 1
        pipe.img[:B].copy_(frames[2 * k]); pipe.img[B:].copy_(frames[2 * k + 1])
        pipe.enqueue()
        state["k"] += 1
    ms = timed(step, iters, warm=3)
    res, counts = pipe.seq.read()
    out = dict(ms_per_step=ms, pairs_per_s=B / ms * 1e3, mean_stereo_points=float(counts[:, 0].mean()), mean_stereo_lines=float(counts[:, 1].mean()),
               mean_keylines_per_image=float(pipe.nl.float().mean()), poses_ok=int((res["status"] == 0).sum()))
    pipe.close(); ctx.close()
    return B, out


out = dict(mode=a.mode, library=os.path.relpath(capi.LIB_PATH, ROOT))
if a.mode == "lsd-uniform":
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    run = LsdRun(ctx, np.stack(scenes(256, 1241, 376)), 1241, 376, a.scale)
    out.update(images_per_launch=256, scale=a.scale, ms_per_launch=timed(run, a.iters), mean_keylines=float(run.d["n"].float().mean()))
elif a.mode == "images-uniform":
    B, rest = pipeline_ms(dict(synth.KITTI_CAM), a.iters, 1.2)
    out.update(streams=B, **rest)
elif a.mode == "images-mixed":
    cams = [KITTI_CAMS[b % 3] for b in range(128)]
    for scale in (0.5, 1.2):
        B, rest = pipeline_ms(cams, a.iters, scale, lines_per_stream=True, lsd_min_length_ratio=RATIO)
        out["lsd_scale_%g" % scale] = rest
    out.update(streams=B, slot=[1242, 376], speedup=out["lsd_scale_1.2"]["ms_per_step"] / out["lsd_scale_0.5"]["ms_per_step"])
elif a.mode == "lsd-mixed":
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    B = 256
    sc = scenes(B)
    sizes = [KITTI_SIZES[b % 3] for b in range(B)]
    slots = np.zeros((B, 376, 1242), np.uint8)
    for b, (c, r) in enumerate(sizes):
        slots[b, :r, :c] = sc[b][:r, :c]
    mixed = LsdRun(ctx, slots, 1242, 376, 0.5, sizes, [RATIO * min(c, r) for c, r in sizes])
    ms_mixed = timed(mixed, a.iters)
    n_mixed = mixed.d["n"].cpu().numpy()
    uni, n_uni = [], np.zeros(B, np.int32)
    for e, (c, r) in enumerate(KITTI_SIZES):
        members = [b for b in range(B) if b % 3 == e]
        uni.append((members, LsdRun(ctx, np.stack([np.ascontiguousarray(sc[b][:r, :c]) for b in members]), c, r, 0.5)))

    def three():
        for _, u in uni:
            u()
    ms_uni = timed(three, a.iters)
    for members, u in uni:
        n_uni[members] = u.d["n"].cpu().numpy()
    out.update(images_per_launch=B, slot=[1242, 376], scale=0.5, min_lengths=[RATIO * min(c, r) for c, r in KITTI_SIZES], ms_mixed_one_launch=ms_mixed,
               ms_three_uniform_detectors=ms_uni, same_keyline_counts=bool(np.array_equal(n_mixed, n_uni)), mean_keylines=float(n_mixed.mean()))
else:  # kernel-profile
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    imgs = np.stack(scenes(256))
    for sizes in (None, [(1242, 376)]):
        run = LsdRun(ctx, imgs, 1242, 376, 0.5, sizes)
        timed(run, a.iters)
    out.update(images_per_launch=256, scale=0.5)
print(json.dumps(out))
