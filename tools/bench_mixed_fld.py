#!/usr/bin/env python3
"""FLD key-lines on mixed image sizes: what the unchanged paths cost beside the parent commit, and what the new paths cost.
One JSON line per run.  python tools/bench_mixed_fld.py --mode MODE [--tree DIR] [--iters N]

  fld-uniform     the FLD detector, 256 KITTI-size images per launch, no size table (the path every existing caller takes)
  images-uniform  ImagePipeline with fld and one camera dict at 128 streams: ms per enqueued step
  fld-mixed       256 images of the three KITTI sizes (1241 x 376, 1242 x 375, 1226 x 370) in 1242 x 376 slots with a size table and each
                  size's own length threshold (int(0.025 x min(width, height))), next to the same images through three uniform detectors
                  (86 + 85 + 85 images), one launch each; the key-line counts of both must agree
  images-mixed    ImagePipeline(cam=[128 dicts], fld, lines_per_stream) over the three KITTI cameras, next to the same streams under one
                  camera: ms per enqueued step

  ab              the unchanged paths beside the parent commit: --runs (4) alternating child processes each of --parent-tree (a built
                  checkout of the parent commit) and of this tree, for fld-uniform, images-uniform and the default `python bench.py` line
  all             ab + the two new-path modes, assembled as profiles/mixed_fld_bench.json is laid out, written to --out

--tree DIR runs the first two modes against another checkout of the repository (its package and its built library); `ab` uses it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["fld-uniform", "images-uniform", "fld-mixed", "images-mixed", "ab", "all"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--out", default=None)
a = ap.parse_args()
ROOT = os.path.abspath(a.tree)
if a.mode in ("ab", "all"):
    import statistics
    import subprocess
    if not a.parent_tree:
        ap.error("--mode %s needs --parent-tree" % a.mode)
    here, parent, me = ROOT, os.path.abspath(a.parent_tree), os.path.abspath(__file__)

    def child(cmd):
        run = subprocess.run([sys.executable] + cmd, capture_output=True, text=True)
        if run.returncode != 0:   # (a failed child ends the whole run: nothing more is started on the device)
            sys.exit("bench_mixed_fld: %s failed (%d)\n%s" % (" ".join(cmd), run.returncode, run.stderr[-2000:]))
        return json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    block = {}
    for name, key, cmd in (("fld", "ms_per_launch", lambda t: [me, "--mode", "fld-uniform", "--tree", t, "--iters", str(a.iters)]),
                           ("images", "ms_per_step", lambda t: [me, "--mode", "images-uniform", "--tree", t, "--iters", str(a.iters)]),
                           ("bench", "value", lambda t: [os.path.join(t, "bench.py"), "--gpus", "1"])):
        p, t = [], []
        for _ in range(a.runs):
            p.append(child(cmd(parent))[key])
            t.append(child(cmd(here))[key])
            print(name, "run", len(t), p[-1], t[-1], file=sys.stderr, flush=True)
        block[name] = {"metric": key, "parent_runs": p, "this_runs": t, "parent_min": min(p), "parent_max": max(p),
                       "this_median": statistics.median(t), "inside_parent_min_max": min(p) <= statistics.median(t) <= max(p)}
        print(name, json.dumps(block[name]), file=sys.stderr, flush=True)
    doc = {"unchanged_paths": block}
    if a.mode == "all":
        doc = {"what": "FLD key-lines on mixed image sizes on one MI355X: tools/bench_mixed_fld.py --mode all --parent-tree <built checkout of the "
                       "parent commit> (unchanged_paths: alternating child processes of the parent commit and this one; new_paths: --mode "
                       "fld-mixed, images-mixed)",
               "unchanged_paths": block,
               "new_paths": {"fld_256_images_three_kitti_sizes": child([me, "--mode", "fld-mixed", "--iters", str(a.iters)]),
                             "images_128_streams_lines_per_stream": child([me, "--mode", "images-mixed", "--iters", str(a.iters)])}}
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))
    sys.exit(0)
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))
import torch  # noqa: E402
from stvo_amd import capi, synth  # noqa: E402
from stvo_amd.ctypes_types import match_params, opt_params  # noqa: E402

KITTI_SIZES = [(1241, 376), (1242, 375), (1226, 370)]
KITTI_CAMS = [dict(synth.KITTI_CAM, width=1241, height=376), dict(synth.KITTI03_CAM, width=1242, height=375),
              dict(synth.KITTI04_CAM, width=1226, height=370)]
M, NLINES, RATIO = 128, 100, 0.025


def threshold(cols, rows):
    return int(RATIO * min(cols, rows))


def timed(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


class FldRun:
    def __init__(self, ctx, imgs, cols, rows, L, sizes=None, thresholds=None):
        B = len(imgs)
        self.fld = capi.Fld(ctx, B, cols, rows, capi.fld_params(L, nfeatures=NLINES), max_keylines=M)
        if sizes is not None:
            self.fld.set_image_sizes(sizes, thresholds)
        self.d = dict(img=torch.from_numpy(imgs).cuda(), rec=torch.zeros(B, M, 6, device="cuda"), n=torch.zeros(B, dtype=torch.int32, device="cuda"))

    def __call__(self):
        self.fld.detect_dev(self.d["img"].data_ptr(), self.d["rec"].data_ptr(), None, self.d["n"].data_ptr())


def scenes(n, cols=1242, rows=376):
    base = [synth.make_image(500 + k, cols=cols, rows=rows) for k in range(8)]
    return [np.roll(base[b % 8], 7 * (b // 8), axis=1) for b in range(n)]


def pipeline_ms(cams, iters, **kw):
    """ImagePipeline with fld at len(cams) streams (one dict: 128 streams of it): ms per enqueued step, and what the last step gave"""
    from stvo_amd import images
    one = isinstance(cams, dict)
    B = 128 if one else len(cams)
    ctx = capi.Context(0, 2048, B)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    cam0 = cams if one else cams[0]
    fld = capi.fld_params(threshold(cam0["width"], cam0["height"]), nfeatures=NLINES)
    pipe = images.ImagePipeline(ctx, B, cams, match_params("kitti"), opt_params("kitti", has_lines=1), max_kp=2048, fld=fld, max_kl=M, **kw)
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
    return B, ms, dict(mean_stereo_points=float(counts[:, 0].mean()), mean_stereo_lines=float(counts[:, 1].mean()),
                       poses_ok=int((res["status"] == 0).sum()))


out = dict(mode=a.mode, library=os.path.relpath(capi.LIB_PATH, ROOT))
if a.mode == "fld-uniform":
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    run = FldRun(ctx, np.stack(scenes(256, 1241, 376)), 1241, 376, threshold(1241, 376))
    out.update(images_per_launch=256, ms_per_launch=timed(run, a.iters), mean_keylines=float(run.d["n"].float().mean()))
elif a.mode == "images-uniform":
    B, ms, rest = pipeline_ms(dict(synth.KITTI_CAM), a.iters)
    out.update(streams=B, ms_per_step=ms, **rest)
elif a.mode == "images-mixed":
    cams = [KITTI_CAMS[b % 3] for b in range(128)]
    B, ms, rest = pipeline_ms(cams, a.iters, lines_per_stream=True, fld_min_length_ratio=RATIO)
    out.update(streams=B, slot=[1242, 376], ms_per_step_lines_per_stream=ms, lines_per_stream=rest)
    B, ms, rest = pipeline_ms(dict(KITTI_CAMS[0]), a.iters)
    out.update(ms_per_step_one_camera=ms, one_camera=rest)
else:
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    B = 256
    sc = scenes(B)
    sizes = [KITTI_SIZES[b % 3] for b in range(B)]
    slots = np.zeros((B, 376, 1242), np.uint8)
    for b, (c, r) in enumerate(sizes):
        slots[b, :r, :c] = sc[b][:r, :c]
    ths = [threshold(c, r) for c, r in sizes]
    mixed = FldRun(ctx, slots, 1242, 376, min(ths), sizes, ths)
    ms_mixed = timed(mixed, a.iters)
    n_mixed = mixed.d["n"].cpu().numpy()
    uni, n_uni = [], np.zeros(B, np.int32)
    for e, (c, r) in enumerate(KITTI_SIZES):
        members = [b for b in range(B) if b % 3 == e]
        uni.append((members, FldRun(ctx, np.stack([np.ascontiguousarray(sc[b][:r, :c]) for b in members]), c, r, threshold(c, r))))

    def three():
        for _, u in uni:
            u()
    ms_uni = timed(three, a.iters)
    for members, u in uni:
        n_uni[members] = u.d["n"].cpu().numpy()
    out.update(images_per_launch=B, slot=[1242, 376], length_thresholds=[threshold(c, r) for c, r in KITTI_SIZES], ms_mixed_one_launch=ms_mixed,
               ms_three_uniform_detectors=ms_uni, same_keyline_counts=bool(np.array_equal(n_mixed, n_uni)), mean_keylines=float(n_mixed.mean()))
print(json.dumps(out))
