"""Feature tracks and key-frame sets per stream on the device pipeline (stvo_seq_set_tracks): what the feature costs and what it
replaces, on one MI355X.  Writes one JSON document:

  off_vs_parent   the whole step (stvo_seq_step_dev) with the feature off on this tree against another tree (the parent commit's
                  checkout, built): alternating runs, one process each; this tree's median must lie inside the parent's own spread
  on_vs_off       the same shapes with the tracks on, without and with key-frame sets, without key-frames (no trajectory: only the first
                  frame is one) and with the trajectory's key-frame decision on (the fraction of stream-steps that took one is reported)
  host            the alternative a caller of the batched path has without the feature: by-product fetch on, the f2f match rows and
                  inlier rows of all streams read on the host after every step, and the host build of csrc/track_update.h on one core
  resources       registers / scratch / LDS of the kernel, from the compiler's remarks (--resources-json, or compiled here)

    python tools/bench_tracks.py --parent-tree /path/to/parent/checkout --out profiles/feature_tracks_bench.json
    python tools/bench_tracks.py --leg step --streams 3072 --tracks sets --trajectory on      (one run, one JSON line; what the above spawns)

The kernel alone is taken from a kernel trace of one such leg (a run of its own; --kernel-us-json merges the figures into the document).
Every leg is a process of its own; a step leg times `--repeats` groups of `--steps` steps by the host clock around a stream
synchronisation, after `--warmup` steps, and reports each group."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIQUE = 64   # distinct synthetic sequences; stream b runs sequence b mod UNIQUE


def use_tree(tree):
    sys.path.insert(0, os.path.join(tree, "stvo-pl_amd", "python"))


def open_pipeline(a, fetch=False):
    import torch  # noqa: F401  (one HIP runtime per process, see capi.load)
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    cam, B = synth.KITTI_CAM, a.streams
    uniq = [synth.make_stereo_sequence(synth.frame_seed(b, 0), n_frames=2, n_pts=a.points, n_lines=a.lines, cam=cam) for b in range(min(B, UNIQUE))]
    seqs = [uniq[b % len(uniq)] for b in range(B)]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    dev = capi.Sequences(ctx, B, 2048, 512, cam, match_params("kitti"), opt_params("kitti", has_lines=1 if a.lines > 0 else 0))
    if fetch:
        dev.enable_fetch(True)
    if a.trajectory == "on":
        dev.set_trajectory(capi.traj_params("kitti"), 1)
    if a.tracks != "off":
        dev.set_tracks(log_steps=1, keyframe_sets=a.tracks == "sets")
    dev.upload(0, [s[0] for s in seqs])
    dev.upload(1, [s[1] for s in seqs])
    return ctx, dev


def step_leg(a):
    """B streams, two frames per stream resident in HBM, steps alternating between them (tools/bench_pipeline.py's loop)."""
    ctx, dev = open_pipeline(a)
    B = a.streams
    try:
        k = 0
        for _ in range(a.warmup):
            dev.step_dev(k & 1); k += 1
        ctx.synchronize()
        groups = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                dev.step_dev(k & 1); k += 1
            ctx.synchronize()
            groups.append((time.perf_counter() - t0) / a.steps * 1e3)
        res, _ = dev.read()
        out = dict(streams=B, tracks=a.tracks, trajectory=a.trajectory, ms_per_step_groups=groups, ms_per_step_median=float(np.median(groups)),
                   frame_pairs_per_s=B / float(np.median(groups)) * 1e3, committed_pose_fraction=float((res["status"] == 0).mean()),
                   steps=a.steps, repeats=a.repeats, warmup=a.warmup)
        if a.trajectory == "on":
            st = dev.trajectory_state()
            out.update(keyframe_fraction_of_stream_steps=float(st["n_keyframes"].mean() / max(1, int(st["n_frames"][0]))))
        if a.tracks != "off":
            pts, lines, cnt = dev.read_tracks(1)
            n = cnt[0][:, 0]
            out.update(points_per_stream_mean=float(n.mean()), lines_per_stream_mean=float(cnt[0][:, 1].mean()),
                       followed_fraction_points=float(np.mean([(pts[0, b, :n[b]]["age"] > 0).mean() for b in range(min(B, UNIQUE))])))
        if a.tracks == "sets":
            out.update(keyframe_serial_mean=float(dev.keyframe_headers()["serial"].mean()))
    finally:
        dev.close()
        ctx.close()
    print(json.dumps(out))


def host_leg(a):
    """Without the feature: fetch on, and after every step the f2f match rows and inlier rows of all streams on the host (pinned copies
    the step makes: a copy kernel behind the f2f stage and one behind the pose kernel), then track_update.h per stream on one core."""
    import ctypes as C
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import track_host_lib
    from np_tracks import TRACK
    a.tracks, a.trajectory = "off", "off"
    ctx, dev = open_pipeline(a, fetch=True)
    B = a.streams
    lib = track_host_lib.load()
    K, M = dev.strides()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    state = [[np.zeros((B, K), TRACK), np.zeros((B, K), TRACK)], [np.zeros((B, M), TRACK), np.zeros((B, M), TRACK)]]
    rec = [np.zeros((B, K), TRACK), np.zeros((B, M), TRACK)]
    n_prev = None
    try:
        for k in range(4):
            dev.step_dev(k & 1)
        dev.read()
        t_step, t_read, t_host = [], [], []
        for k in range(a.steps):
            t0 = time.perf_counter()
            dev.step_dev(k & 1)
            ctx.synchronize()
            t1 = time.perf_counter()
            _, counts = dev.read()
            _, _, m12p, m12l = dev.fetch_matches()
            inlp, inll = dev.fetch_inliers()
            t2 = time.perf_counter()
            n_cur = [np.ascontiguousarray(counts[:, 0]), np.ascontiguousarray(counts[:, 1])]
            if n_prev is not None:
                for j, (m12, inl, cap) in enumerate(((m12p, inlp, K), (m12l, inll, M))):
                    lib.tkh_step_batch(B, cap, p(n_prev[j]), p(m12), p(inl), p(state[j][k & 1]), p(n_cur[j]), p(rec[j]), p(state[j][(k & 1) ^ 1]))
            t3 = time.perf_counter()
            n_prev = n_cur
            t_step.append((t1 - t0) * 1e3); t_read.append((t2 - t1) * 1e3); t_host.append((t3 - t2) * 1e3)
        med = lambda v: [float(np.median(v)), float(np.min(v)), float(np.max(v))]
        out = dict(streams=B, cores=1, step_with_fetch_ms_median_min_max=med(t_step), read_matches_inliers_ms_median_min_max=med(t_read),
                   host_update_ms_median_min_max=med(t_host[1:]), bytes_read_per_step=B * (2 * K + 2 * M) * 4 * 2,
                   round_trip_ms_median=float(np.median(t_read)) + float(np.median(t_host[1:])))
    finally:
        dev.close()
        ctx.close()
    print(json.dumps(out))


def resources():
    """Registers, scratch and LDS of csrc/track_kernel.hip's kernel, from -Rpass-analysis=kernel-resource-usage."""
    src = os.path.join(ROOT, "stvo-pl_amd", "csrc", "track_kernel.hip")
    p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = "track_update_kernel" if "track_update_kernel" in m.group(1) else m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\S+)", line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


def spawn(tree, leg, streams, a, tracks="off", trajectory="off"):
    env = dict(os.environ)
    env.pop("STVO_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__) if tree == ROOT else os.path.join(ROOT, "tools", "bench_trajectory.py"), "--leg", leg,
           "--streams", str(streams), "--trajectory", trajectory, "--tree", tree, "--steps", str(a.steps), "--repeats", str(a.repeats),
           "--warmup", str(a.warmup), "--points", str(a.points), "--lines", str(a.lines)]
    if tree == ROOT:
        cmd += ["--tracks", tracks]   # (the parent tree has no such feature: its step leg is tools/bench_trajectory.py's, the same loop)
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["step", "host"], default=None)
    ap.add_argument("--tree", default=ROOT, help="checkout whose python package and library a leg uses")
    ap.add_argument("--parent-tree", default=None, help="built checkout of the parent commit, for off_vs_parent")
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--shapes", default="3072,128")
    ap.add_argument("--tracks", choices=["off", "on", "sets"], default="off")
    ap.add_argument("--trajectory", choices=["off", "on"], default="off")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--points", type=int, default=1650)
    ap.add_argument("--lines", type=int, default=85)
    ap.add_argument("--resources-json", default=None)
    ap.add_argument("--kernel-us-json", default=None, help="kernel-trace figures of track_update_kernel, merged as `kernel_alone`")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        use_tree(a.tree)
        {"step": step_leg, "host": host_leg}[a.leg](a)
        return
    doc = dict(what="feature tracks and key-frame sets per stream on one MI355X: the step with the feature off against the parent commit "
                    "(alternating runs, one process each), the step with the feature on against off, and the host alternative (fetch of the "
                    "match and inlier rows + the host build of the same functions on one core)",
               workload=f"KITTI-shaped stereo, {a.points} points + {a.lines} lines per image (+ 20 % distractors), {UNIQUE} distinct synthetic "
                        f"sequences tiled over the streams, two frames per stream resident in HBM; a run = {a.repeats} groups of {a.steps} steps "
                        f"after {a.warmup}, host clock around a stream synchronisation")
    for B in [int(s) for s in a.shapes.split(",")]:
        row = {}
        if a.parent_tree:
            runs = {"parent": [], "this": []}
            for _ in range(a.rounds):   # parent, this, parent, this, ...
                runs["parent"].append(spawn(a.parent_tree, "step", B, a)["ms_per_step_median"])
                runs["this"].append(spawn(ROOT, "step", B, a)["ms_per_step_median"])
                print(B, "parent", runs["parent"][-1], "this", runs["this"][-1], flush=True)
            med = float(np.median(runs["this"]))
            row["off_vs_parent"] = dict(ms_per_step_runs=runs, parent_median_min_max=[float(np.median(runs["parent"])), min(runs["parent"]), max(runs["parent"])],
                                        this_median_min_max=[med, min(runs["this"]), max(runs["this"])],
                                        gate=dict(statement="this tree's median ms per step with the feature off is not above the parent's slowest run",
                                                  this_median=med, parent_slowest_run=max(runs["parent"]), holds=bool(med <= max(runs["parent"]))))
        legs = {}
        for traj in ("off", "on"):
            for tracks in ("off", "on", "sets"):
                r = [spawn(ROOT, "step", B, a, tracks, traj) for _ in range(2)]
                legs[f"trajectory_{traj}_tracks_{tracks}"] = dict(runs=r, ms_per_step=float(np.median([x["ms_per_step_median"] for x in r])))
                print(B, traj, tracks, legs[f"trajectory_{traj}_tracks_{tracks}"]["ms_per_step"], flush=True)
        added = {}
        for traj in ("off", "on"):
            base = legs[f"trajectory_{traj}_tracks_off"]["ms_per_step"]
            for tracks in ("on", "sets"):
                ms = legs[f"trajectory_{traj}_tracks_{tracks}"]["ms_per_step"]
                added[f"trajectory_{traj}_tracks_{tracks}"] = dict(us_added_per_step=1e3 * (ms - base), percent_of_step=100.0 * (ms - base) / base)
        row["on_vs_off"] = dict(legs=legs, added=added)
        row["host"] = spawn(ROOT, "host", B, a)
        doc[f"streams_{B}"] = row
        print(B, json.dumps(added), row["host"], flush=True)
    if a.resources_json:
        with open(a.resources_json) as f:
            doc["resources"] = json.load(f)
    else:
        doc["resources"] = resources()
    if a.kernel_us_json:
        with open(a.kernel_us_json) as f:
            doc["kernel_alone"] = json.load(f)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
