#!/usr/bin/env python3
"""The many-wave LSD search under a size table (stvo_lsd_set_table_route): what the new route costs beside the one-wave route, and what
the unchanged paths cost beside the parent commit.  One JSON line per run.
python tools/bench_lsd_table_route.py --mode MODE [--tree DIR] [--iters N]

  lsd-one         the LSD detector on one KITTI-size image, no size table
  lsd-256         256 KITTI-size images per launch, no size table
  lsd-256-table   256 images of the three KITTI sizes in 1242 x 376 slots under a size table with the default table route
  new-path        2, 8, 32 and 128 images of the three KITTI sizes (1241 x 376, 1242 x 375, 1226 x 370) in 1242 x 376 slots, each at its
                  own minimum length (0.025 x min(width, height)), at lsd_scale 1.2 and 0.5: under the table on the one-wave and on the
                  many-wave route, in --rounds alternating rounds of --iters launches within this one process (medians of the rounds),
                  beside the same images through three uniform detectors (one per size, one launch each) and the same batch of
                  1241 x 376 images with no table
  images          ImagePipeline(cam=[B dicts], lsd, lines_per_stream) at 4 and 64 streams over the three KITTI cameras with
                  lsd_many_waves on and off, alternating rounds: ms per enqueued step

  ab              the unchanged paths beside the parent commit: --runs (4) alternating child processes each of --parent-tree (a built
                  checkout of the parent commit) and of this tree, for lsd-one, lsd-256, lsd-256-table and the default `python bench.py`
  all             ab + new-path + images, assembled as profiles/lsd_table_route_bench.json is laid out, written to --out

--tree DIR runs the three lsd-* modes against another checkout of the repository (its package and its built library); `ab` uses it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["lsd-one", "lsd-256", "lsd-256-table", "new-path", "images", "ab", "all"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--out", default=None)
a = ap.parse_args()
ROOT = os.path.abspath(a.tree)
if a.mode in ("ab", "all"):
    import subprocess
    if not a.parent_tree:
        ap.error("--mode %s needs --parent-tree" % a.mode)
    here, parent, me = ROOT, os.path.abspath(a.parent_tree), os.path.abspath(__file__)

    def child(cmd):
        run = subprocess.run([sys.executable] + cmd, capture_output=True, text=True)
        if run.returncode != 0:
            sys.exit("bench_lsd_table_route: %s failed (%d)\n%s" % (" ".join(cmd), run.returncode, run.stderr[-2000:]))
        return json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])

    def lsd_mode(mode):
        return lambda t: [me, "--mode", mode, "--tree", t, "--iters", str(a.iters)]
    new_paths = None
    if a.mode == "all":   # (first: the longer a process has run, the more the numbers of the unchanged paths are worth keeping)
        new_paths = {"lsd_under_a_table_by_route": child([me, "--mode", "new-path", "--iters", str(a.iters), "--rounds", str(a.rounds)]),
                     "images_lines_per_stream": child([me, "--mode", "images", "--iters", str(a.iters), "--rounds", str(a.rounds)])}
        print("new_paths", json.dumps(new_paths), file=sys.stderr, flush=True)
    block = {}
    for name, key, cmd in (("lsd_one_image_no_table", "ms_per_launch", lsd_mode("lsd-one")),
                           ("lsd_256_images_no_table", "ms_per_launch", lsd_mode("lsd-256")),
                           ("lsd_256_mixed_images_default_table_route", "ms_per_launch", lsd_mode("lsd-256-table")),
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
        doc = {"what": "the many-wave LSD search under a size table on one MI355X: tools/bench_lsd_table_route.py --mode all --parent-tree <built "
                       "checkout of the parent commit> (unchanged_paths: alternating child processes of the parent commit and this one; "
                       "new_paths: --mode new-path and images, alternating rounds of the two routes within one process)",
               "unchanged_paths": block,
               "new_paths": new_paths}
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
    def __init__(self, ctx, imgs, cols, rows, sizes=None, min_lengths=None, scale=1.2):
        B = len(imgs)
        prm = capi.lsd_params(min_length=RATIO * min(cols, rows), nfeatures=NLINES, scale=scale)
        if sizes is not None and scale != 1.2:
            prm.flags |= capi.LSD_SIZES_ANY_RADIUS
        self.lsd = capi.Lsd(ctx, B, cols, rows, prm, max_keylines=M)
        if sizes is not None:
            self.lsd.set_image_sizes(sizes, min_lengths)
        self.d = dict(img=torch.from_numpy(imgs).cuda(), rec=torch.zeros(B, M, 6, device="cuda"), n=torch.zeros(B, dtype=torch.int32, device="cuda"))

    def __call__(self):
        self.lsd.detect_dev(self.d["img"].data_ptr(), self.d["rec"].data_ptr(), None, self.d["n"].data_ptr())

    def counts(self):
        torch.cuda.synchronize()
        return self.d["n"].cpu().numpy().copy()

    def close(self):
        torch.cuda.synchronize()
        self.lsd.close()
        self.d = None


def scenes(n, cols=1242, rows=376):
    base = [synth.make_image(500 + k, cols=cols, rows=rows) for k in range(8)]
    return [np.roll(base[b % 8], 7 * (b // 8), axis=1) for b in range(n)]


def mixed_slots(B):
    sc = scenes(B)
    sizes = [KITTI_SIZES[b % 3] for b in range(B)]
    slots = np.zeros((B, 376, 1242), np.uint8)
    for b, (c, r) in enumerate(sizes):
        slots[b, :r, :c] = sc[b][:r, :c]
    return sc, sizes, slots


def alternate(runs, iters, rounds):
    """runs: name -> callable.  `rounds` rounds, each timing every run once in turn -> name -> (median of the rounds, the rounds)"""
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            ms[k].append(timed(fn, iters, warm=1))
    return {k: dict(ms_median=statistics.median(v), ms_rounds=v) for k, v in ms.items()}


out = dict(mode=a.mode, library=os.path.relpath(capi.LIB_PATH, ROOT))
if a.mode in ("lsd-one", "lsd-256"):
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    B = 1 if a.mode == "lsd-one" else 256
    run = LsdRun(ctx, np.stack(scenes(B, 1241, 376)), 1241, 376)
    out.update(images_per_launch=B, ms_per_launch=timed(run, a.iters * (8 if B == 1 else 1)), mean_keylines=float(run.counts().mean()))
elif a.mode == "lsd-256-table":
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    sc, sizes, slots = mixed_slots(256)
    run = LsdRun(ctx, slots, 1242, 376, sizes, [RATIO * min(c, r) for c, r in sizes])
    out.update(images_per_launch=256, ms_per_launch=timed(run, a.iters), mean_keylines=float(run.counts().mean()))
elif a.mode == "new-path":
    ctx = capi.Context(0, 2048, 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for scale in (1.2, 0.5):
        for B in (2, 8, 32, 128):
            sc, sizes, slots = mixed_slots(B)
            mls = [RATIO * min(c, r) for c, r in sizes]
            one = LsdRun(ctx, slots, 1242, 376, sizes, mls, scale)
            many = LsdRun(ctx, slots, 1242, 376, sizes, mls, scale)
            many.lsd.set_table_route(capi.LSD_TABLE_BY_BATCH)
            assert one.lsd.search_route() == capi.LSD_SEARCH_ONE_WAVE and many.lsd.search_route() == capi.LSD_SEARCH_MANY_WAVES
            plain = LsdRun(ctx, np.stack(scenes(B, 1241, 376)), 1241, 376, scale=scale)
            uni = []
            for e, (c, r) in enumerate(KITTI_SIZES):
                members = [b for b in range(B) if b % 3 == e]
                if members:
                    uni.append((members, LsdRun(ctx, np.stack([np.ascontiguousarray(sc[b][:r, :c]) for b in members]), c, r, scale=scale)))

            def three():
                for _, u in uni:
                    u()
            res = alternate({"table_one_wave": one, "table_many_waves": many, "three_uniform_detectors": three, "no_table_one_size": plain},
                            a.iters, a.rounds)
            n_one, n_many, n_uni = one.counts(), many.counts(), np.zeros(B, np.int32)
            for members, u in uni:
                n_uni[members] = u.counts()
            res.update(same_keyline_counts=bool(np.array_equal(n_one, n_many) and np.array_equal(n_one, n_uni)), mean_keylines=float(n_one.mean()),
                       many_waves_faster_than_one_wave=bool(res["table_many_waves"]["ms_median"] < res["table_one_wave"]["ms_median"]))
            out["scale_%g_batch_%d" % (scale, B)] = res
            print("scale", scale, "batch", B, json.dumps({k: v["ms_median"] for k, v in res.items() if isinstance(v, dict)}), file=sys.stderr, flush=True)
            for r in [one, many, plain] + [u for _, u in uni]:
                r.close()
else:
    from stvo_amd import images
    for B in (4, 64):
        cams = [KITTI_CAMS[b % 3] for b in range(B)]
        ctx = capi.Context(0, 2048, B)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        lsd = capi.lsd_params(min_length=RATIO * 376, nfeatures=NLINES)
        pairs = {(e, s): synth.make_stereo_image_sequence(50 + s, 2, c) for e, c in enumerate(KITTI_CAMS) for s in range(2)}
        pipes, steps = {}, {}
        for name, many in (("one_wave", False), ("many_waves", True)):
            pipe = images.ImagePipeline(ctx, B, cams, match_params("kitti"), opt_params("kitti", has_lines=1), max_kp=2048, lsd=lsd, max_kl=M,
                                        lines_per_stream=True, lsd_min_length_ratio=RATIO, lsd_many_waves=many)
            frames = []
            for k in range(2):
                for side in range(2):
                    buf = np.zeros((B, pipe.rows, pipe.cols), np.uint8)
                    for b in range(B):
                        im = pairs[(b % 3, (b // 3) % 2)][k][side]
                        buf[b, :im.shape[0], :im.shape[1]] = im
                    frames.append(torch.from_numpy(buf).cuda())
            state = dict(k=0)

            def step(pipe=pipe, frames=frames, state=state):
                k = state["k"] & 1
                pipe.img[:B].copy_(frames[2 * k]); pipe.img[B:].copy_(frames[2 * k + 1])
                pipe.enqueue()
                state["k"] += 1
            pipes[name], steps[name] = pipe, step
        res = alternate(steps, a.iters, a.rounds)
        torch.cuda.synchronize()
        reads = {k: p.seq.read() for k, p in pipes.items()}
        res.update(streams=B, lsd_images_per_launch=2 * B, slot=[1242, 376],
                   same_results=bool(reads["one_wave"][0].tobytes() == reads["many_waves"][0].tobytes() and
                                     np.array_equal(reads["one_wave"][1], reads["many_waves"][1])),
                   mean_stereo_lines=float(reads["many_waves"][1][:, 1].mean()), poses_ok=int((reads["many_waves"][0]["status"] == 0).sum()))
        out["streams_%d" % B] = res
        print("streams", B, json.dumps({k: v["ms_median"] for k, v in res.items() if isinstance(v, dict)}), file=sys.stderr, flush=True)
        for p in pipes.values():
            p.close()
        ctx.close()
print(json.dumps(out))
