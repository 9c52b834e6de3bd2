"""FLD key-line detector (stvo_fld_*) on the GPU: KITTI-size images per second at several batch sizes, the latency of one image,
one stereo pair from images to pose with FLD key-lines next to the same with LSD (ImagePipeline(fld=...) / (lsd=...)), and the edge /
component statistics of the images (the walk of the largest component is the one sequential part).  Writes one JSON document.

    python tools/bench_fld.py --out fld_bench.json
    rocprofv3 --kernel-trace --stats -d fld_prof -- python tools/bench_fld.py --profile-only

The per-kernel split comes from the second command (a run of its own: tracing slows the host); --profile-only runs the timed
shapes once each, nothing else.  profiles/fld_bench.json is the first command's document with that split added as "kernel_split"."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))

from stvo_amd import capi, images, synth  # noqa: E402
from stvo_amd.ctypes_types import match_params, opt_params  # noqa: E402

COLS, ROWS = 1241, 376
L = int(0.025 * min(COLS, ROWS))  # 9


def kitti_images(n):
    base = [synth.make_image(s, COLS, ROWS) for s in range(min(n, 8))]
    return np.stack([base[i % len(base)] for i in range(n)])


def time_detect(ctx, det, img_dev, kl, resp, nl, iters):
    for _ in range(2):
        det.detect_dev(img_dev.data_ptr(), kl.data_ptr(), resp.data_ptr(), nl.data_ptr())
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        det.detect_dev(img_dev.data_ptr(), kl.data_ptr(), resp.data_ptr(), nl.data_ptr())
    ctx.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_batches(ctx, batches, iters, lsd_too=True):
    import torch
    out = {}
    for B in batches:
        imgs = torch.as_tensor(kitti_images(B)).cuda()
        kl = torch.zeros((B, 300, 6), dtype=torch.float32, device="cuda")
        resp = torch.zeros((B, 300), dtype=torch.float32, device="cuda")
        nl = torch.zeros((B,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        row = {}
        for name, det in (("fld", capi.Fld(ctx, B, COLS, ROWS, capi.fld_params(L, nfeatures=300), max_keylines=300)),
                          ("lsd", capi.Lsd(ctx, B, COLS, ROWS, capi.lsd_params(min_length=0.025 * ROWS, nfeatures=300), max_keylines=300)
                           if lsd_too else None)):
            if det is None:
                continue
            try:
                s = time_detect(ctx, det, imgs, kl, resp, nl, iters if B <= 16 else max(2, iters // 4))
                row[name] = dict(ms_per_call=1e3 * s, images_per_s=B / s)
            finally:
                det.close()
        out[str(B)] = row
        print(B, row, flush=True)
    return out


def component_stats(n=4):
    """Edge pixels, 8-connected components and the largest component of the KITTI-size scenes (host side, from the statement's
    numpy edge map)."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import np_fld
    rows = []
    for img in kitti_images(n):
        e = np_fld.canny_edges(img) > 0
        lab, k = ndimage.label(e, structure=np.ones((3, 3)))
        sz = np.bincount(lab.ravel())[1:]
        rows.append(dict(edge_px=int(e.sum()), components=int(k), largest=int(sz.max()) if k else 0))
    return rows


def pair_to_pose(iters):
    """One stereo pair per step through ImagePipeline: ORB + key-lines (FLD or LSD) + LBD + stereo + f2f + pose, host-timed with a
    device synchronise after every step."""
    import torch
    cam = dict(synth.KITTI_CAM)
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    pairs = synth.make_stereo_image_sequence(7, 4, cam)
    out = {}
    for name in ("fld", "lsd"):
        ctx = capi.Context(device_id=0, max_rows=2048, max_batch=1)
        kw = dict(fld=capi.fld_params(L, nfeatures=100)) if name == "fld" else dict(lsd=capi.lsd_params(min_length=0.025 * ROWS, nfeatures=100))
        pipe = images.ImagePipeline(ctx, 1, cam, mp, op, max_kp=2048, max_kl=128, **kw)
        try:
            for k in range(4):
                pipe.push_images(pairs[k % 4][0][None], pairs[k % 4][1][None])
            ts = []
            for k in range(iters):
                left, right = pairs[k % 4]
                t0 = time.perf_counter()
                pipe.push_images(left[None], right[None])
                torch.cuda.synchronize(); ctx.synchronize()
                ts.append(time.perf_counter() - t0)
            out[name] = dict(ms_median=1e3 * float(np.median(ts)), ms_min=1e3 * float(np.min(ts)))
        finally:
            pipe.close()
            ctx.close()
        print(name, out[name], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="1,2,16,128,1024")
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=4)
    try:
        if a.profile_only:
            bench_batches(ctx, [1, 128], 3, lsd_too=False)
            return
        res = dict(image=f"{COLS}x{ROWS} synth.make_image scenes", length_threshold=L, nfeatures=300)
        res["batches"] = bench_batches(ctx, [int(b) for b in a.batches.split(",")], a.iters)
        res["one_image_latency_ms"] = {k: v["ms_per_call"] for k, v in res["batches"]["1"].items()}
    finally:
        ctx.close()
    res["stereo_pair_to_pose"] = pair_to_pose(a.iters)
    res["components"] = component_stats()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
