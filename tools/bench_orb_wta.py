#!/usr/bin/env python3
"""The cost of the ORB descriptor settings (stvo_orb_set_descriptor) next to the default (WTA_K 2, patch 31), and the default itself on
two builds of the library: images per second of stvo_orb_detect_levels_dev on KITTI-size images resident in HBM, 256 per launch,
2000 features, one level.
    python tools/bench_orb_wta.py [--parent-tree DIR] [--rounds 4] [--iters 5] [--out profiles/orb_wta_bench.json]
Every measurement runs in a child process of its own that talks to the library through ctypes alone (so that a build without the new
symbols can be measured): the default setting alternately on the library of --parent-tree (a built checkout of the parent commit) and
on this tree's library, `rounds` times each; then (3, 31), (4, 31), (2, 21), (2, 27) at edge 19 and (4, 63) at edge 44 on this tree's library.
--headline adds each tree's own bench.py step at 3072 streams, alternating.
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_orb_wta.py --child-profile
    python tools/bench_orb_wta.py --kernel-trace DIR/.../kernel_trace.csv --out ...        (adds the describe kernel's time per setting)"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIS_LIB = os.path.join(ROOT, "stvo-pl_amd", "libstvo_hip.so")
COLS, ROWS, K, NFEAT = 1241, 376, 2048, 2000
SETTINGS = [(2, 31, 19), (3, 31, 19), (4, 31, 19), (2, 21, 19), (2, 27, 19), (4, 63, 44)]   # wta_k, patch_size, edge_threshold
PROFILE_LAUNCHES = 4   # per setting under --child-profile: one warm-up and three that count


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("fast_threshold", C.c_int32), ("edge_threshold", C.c_int32), ("nlevels", C.c_int32),
                ("scale_factor", C.c_double)]


def child(lib_path, wta_k, patch, edge, batch, iters, launches_only=0):
    """One detector, one setting: ms per launch (median of `iters` timed launches), or `launches_only` launches and no timing."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))
    from stvo_amd import synth
    L = C.CDLL(lib_path)
    ctx, orb = C.c_void_p(), C.c_void_p()

    def chk(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {rc}")
    L.stvo_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    chk(L.stvo_ctx_create(0, 2048, 4, C.byref(ctx)), "stvo_ctx_create")
    L.stvo_orb_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OrbParams), C.POINTER(C.c_void_p)]
    prm = OrbParams(NFEAT, 20, edge, 1, 1.2)
    chk(L.stvo_orb_create(ctx, batch, COLS, ROWS, K, C.byref(prm), C.byref(orb)), "stvo_orb_create")
    if (wta_k, patch) != (2, 31):
        L.stvo_orb_set_descriptor.argtypes = [C.c_void_p, C.c_int, C.c_int]
        chk(L.stvo_orb_set_descriptor(orb, wta_k, patch), "stvo_orb_set_descriptor")
    base = [synth.make_image(500 + k, cols=COLS, rows=ROWS) for k in range(8)]
    imgs = np.stack([np.roll(base[b % 8], 7 * (b // 8), axis=1) for b in range(batch)])
    d = [torch.from_numpy(imgs).cuda(), torch.zeros(batch, K, 2, device="cuda"), torch.zeros(batch, K, device="cuda"), torch.zeros(batch, K, device="cuda"),
         torch.zeros(batch, K, dtype=torch.int32, device="cuda"), torch.zeros(batch, K, 32, dtype=torch.uint8, device="cuda"),
         torch.zeros(batch, dtype=torch.int32, device="cuda"), torch.zeros(batch, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()   # (the detector runs on the context's own stream)
    L.stvo_orb_detect_levels_dev.argtypes = [C.c_void_p] * 9
    L.stvo_ctx_synchronize.argtypes = [C.c_void_p]

    def run():
        chk(L.stvo_orb_detect_levels_dev(orb, *[t.data_ptr() for t in d]), "stvo_orb_detect_levels_dev")

    def sync():
        chk(L.stvo_ctx_synchronize(ctx), "stvo_ctx_synchronize")
    if launches_only:
        for _ in range(launches_only):
            run()
            sync()
        ms = []
    else:
        for _ in range(2):
            run()
        sync()
        ms = []
        for _ in range(iters):
            t0 = time.perf_counter()
            run()
            sync()
            ms.append((time.perf_counter() - t0) * 1e3)
    mean_kp = float(d[6].float().mean())
    L.stvo_orb_destroy.argtypes = [C.c_void_p]
    L.stvo_ctx_destroy.argtypes = [C.c_void_p]
    L.stvo_orb_destroy(orb)
    L.stvo_ctx_destroy(ctx)
    return dict(ms=ms, mean_keypoints=mean_kp)


def spawn(args, lib, *setting):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", lib, *[str(v) for v in setting], "--batch", str(args.batch), "--iters", str(args.iters)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def summary(ms, batch):
    med = statistics.median(ms)
    return {"ms_per_launch_median": med, "ms_per_launch_min": min(ms), "ms_per_launch_max": max(ms), "images_per_s_median": batch / med * 1e3,
            "images_per_s_range": [batch / max(ms) * 1e3, batch / min(ms) * 1e3]}


def headline(tree, streams, steps, warmup):
    env = {k: v for k, v in os.environ.items() if k != "STVO_LIB"}
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--batch", str(streams)],
                         capture_output=True, text=True, timeout=900, env=env, cwd=tree)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def describe_times(path):
    """Per setting, the median duration (us) of the describe kernel's counted dispatches in a kernel trace of --child-profile."""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "orb_describe" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == PROFILE_LAUNCHES * len(SETTINGS), len(rows)
    out = {}
    for i, (k, P, e) in enumerate(SETTINGS):
        grp = rows[i * PROFILE_LAUNCHES + 1:(i + 1) * PROFILE_LAUNCHES]
        out[f"wta_k_{k}_patch_{P}"] = {"kernel": re.search(r"orb_describe\w*(<[^>]*>)?", grp[0]["Kernel_Name"]).group(0),
                                       "us_median": statistics.median((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in grp)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4, metavar=("LIB", "WTA_K", "PATCH", "EDGE"))
    ap.add_argument("--child-profile", action="store_true")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--headline-only", action="store_true", help="bench.py on both trees and nothing else (merged into --out)")
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.parent_tree:
        a.parent_tree = os.path.abspath(a.parent_tree)
    if a.child:
        print(json.dumps(child(a.child[0], int(a.child[1]), int(a.child[2]), int(a.child[3]), a.batch, a.iters)))
        return 0
    if a.child_profile:
        for k, P, e in SETTINGS:
            child(THIS_LIB, k, P, e, a.batch, 0, launches_only=PROFILE_LAUNCHES)
        return 0
    out = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out.update({"images_per_launch": a.batch, "workload": f"{a.batch} synthetic {COLS} x {ROWS} images, orb_nfeatures {NFEAT}, FAST threshold 20, 1 level",
                "timed_launches_per_run": a.iters})
    if a.kernel_trace:
        out["describe_kernel"] = describe_times(a.kernel_trace)
    elif not a.headline_only:
        runs = {"parent": [], "this": []}
        parent_lib = os.path.join(a.parent_tree, "stvo-pl_amd", "libstvo_hip.so") if a.parent_tree else None
        if parent_lib:
            for r in range(a.rounds):
                for which in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
                    runs[which].append(statistics.median(spawn(a, parent_lib if which == "parent" else THIS_LIB, 2, 31, 19)["ms"]))
            out["default_2_31"] = {"parent": dict(summary(runs["parent"], a.batch), runs_ms=runs["parent"]),
                                   "this": dict(summary(runs["this"], a.batch), runs_ms=runs["this"])}
            out["default_2_31"]["this_over_parent_time"] = statistics.median(runs["this"]) / statistics.median(runs["parent"])
        ref = None
        out["settings"] = {}
        for k, P, e in SETTINGS:
            r = spawn(a, THIS_LIB, k, P, e)
            rec = dict(summary(r["ms"], a.batch), edge_threshold=e, mean_keypoints=r["mean_keypoints"])
            if (k, P) == (2, 31):
                ref = rec["ms_per_launch_median"]
            rec["time_over_default"] = rec["ms_per_launch_median"] / ref
            out["settings"][f"wta_k_{k}_patch_{P}"] = rec
    if (a.headline or a.headline_only) and a.parent_tree:
        h = {"parent": [], "this": []}
        for r in range(a.rounds):
            for which in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
                h[which].append(headline(a.parent_tree if which == "parent" else ROOT, a.streams, 24, 6))
        out["headline_bench_py"] = {"streams": a.streams, "parent": h["parent"], "this": h["this"]}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
