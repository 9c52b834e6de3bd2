"""Trajectory and key-frame decision per stream on the device pipeline (stvo_seq_set_trajectory): what the feature costs and what it
replaces, on one MI355X.  Writes one JSON document with four measurements:

  off_vs_parent   the whole step (stvo_seq_step_dev) with the feature off on this tree against another tree (the parent commit's
                  checkout, built): alternating runs, one process each; this tree's median must lie inside the parent's own spread
  on_vs_off       the same shapes with the feature on (key-frames on, log_steps 1), and the update kernel alone between an event pair
  host            the same updates through the host build of csrc/traj_update.h on one core, results read back included: the round
                  trip a caller of the batched path had to make
  resources       VGPRs / scratch bytes of the kernel, from the compiler's remarks (--resources-json, or compiled here)

    python tools/bench_trajectory.py --parent-tree /path/to/parent/checkout --out profiles/trajectory_bench.json
    python tools/bench_trajectory.py --leg step --streams 3072 --trajectory off        (one run, one JSON line; what the above spawns)

Every step leg is a process of its own (fresh context, its own code-object load); a leg times `--repeats` groups of `--steps` steps
by the host clock around a stream synchronisation, after `--warmup` steps, and reports each group."""
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


def step_leg(a):
    """B streams, two frames per stream resident in HBM, steps alternating between them (tools/bench_pipeline.py's loop)."""
    import torch  # noqa: F401  (one HIP runtime per process, see capi.load)
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    cam, B = synth.KITTI_CAM, a.streams
    uniq = [synth.make_stereo_sequence(synth.frame_seed(b, 0), n_frames=2, n_pts=a.points, n_lines=a.lines, cam=cam) for b in range(min(B, UNIQUE))]
    seqs = [uniq[b % len(uniq)] for b in range(B)]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    dev = capi.Sequences(ctx, B, 2048, 512, cam, match_params("kitti"), opt_params("kitti", has_lines=1 if a.lines > 0 else 0))
    try:
        if a.trajectory == "on":
            dev.set_trajectory(capi.traj_params("kitti"), 1)
        dev.upload(0, [s[0] for s in seqs])
        dev.upload(1, [s[1] for s in seqs])
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
        out = dict(streams=B, trajectory=a.trajectory, ms_per_step_groups=groups, ms_per_step_median=float(np.median(groups)),
                   frame_pairs_per_s=B / float(np.median(groups)) * 1e3, committed_pose_fraction=float((res["status"] == 0).mean()),
                   steps=a.steps, repeats=a.repeats, warmup=a.warmup)
        if a.trajectory == "on":
            rec = dev.read_trajectory(1)[0]
            st = dev.trajectory_state()
            out.update(keyframes_per_stream_mean=float(st["n_keyframes"].mean()), frames_per_stream=int(st["n_frames"][0]),
                       new_kf_fraction_last_step=float(rec["new_kf"].mean()))
    finally:
        dev.close()
        ctx.close()
    print(json.dumps(out))


def pose_results(B):
    """B pose results of the kind the step leaves: the sequence of tests/trajectory_cases.py, stream b at frame b mod 60."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import trajectory_cases as tc
    res = tc.sequence()
    return res[np.arange(B) % len(res)], tc


def kernel_leg(a):
    """The update kernel alone: one launch between an event pair, `--steps` times; and the same number back to back in one pair."""
    import torch
    from stvo_amd import capi
    from stvo_amd.ctypes_types import TRAJ_RECORD_DTYPE, TRAJ_STATE_DTYPE
    B = a.streams
    res, _ = pose_results(B)
    stream = torch.cuda.Stream()
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=4)
    try:
        ctx.set_stream(stream.cuda_stream)
        d_res = torch.from_numpy(res.view(np.uint8).reshape(-1).copy()).cuda()
        d_state = torch.zeros(B * TRAJ_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_rec = torch.zeros(B * TRAJ_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        prm = capi.traj_params("kitti")
        capi.traj_init_dev(ctx, d_state)
        for _ in range(5):
            capi.traj_update_dev(ctx, d_res, prm, d_state, d_rec)
        stream.synchronize()
        single = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            capi.traj_update_dev(ctx, d_res, prm, d_state, d_rec)
            e1.record(stream)
            e1.synchronize()
            single.append(e0.elapsed_time(e1) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            capi.traj_update_dev(ctx, d_res, prm, d_state, d_rec)
        e1.record(stream)
        e1.synchronize()
        out = dict(streams=B, launches=a.steps, us_one_launch_between_events_median_min_max=[float(np.median(single)), float(np.min(single)), float(np.max(single))],
                   us_per_launch_back_to_back=e0.elapsed_time(e1) * 1e3 / a.steps)
    finally:
        ctx.close()
    print(json.dumps(out))


def host_leg(a):
    """What a caller of the batched path did without the feature: read the B results back (stvo_seq_read: one synchronisation, 700 bytes
    per stream) and run the update per stream on the host — the host build of the same function, one core."""
    import ctypes as C
    import torch  # noqa: F401
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    res, _ = pose_results(a.streams)
    import traj_host_lib
    prm = capi.traj_params("kitti")
    B = a.streams
    state = traj_host_lib.init(B)
    traj_host_lib.update(res, prm, state)
    t = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        traj_host_lib.load().trh_update(B, res.ctypes.data_as(C.c_void_p), C.byref(prm), state.ctypes.data_as(C.c_void_p), None)
        t.append((time.perf_counter() - t0) * 1e3)
    out = dict(streams=B, cores=1, host_update_ms_median_min_max=[float(np.median(t)), float(np.min(t)), float(np.max(t))],
               us_per_stream=float(np.median(t)) / B * 1e3)
    # the read-back the host update needs: the pipeline's own read of B results behind a finished step
    cam = synth.KITTI_CAM
    uniq = [synth.make_stereo_sequence(synth.frame_seed(b, 0), n_frames=2, n_pts=a.points, n_lines=a.lines, cam=cam) for b in range(min(B, UNIQUE))]
    seqs = [uniq[b % len(uniq)] for b in range(B)]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    dev = capi.Sequences(ctx, B, 2048, 512, cam, match_params("kitti"), opt_params("kitti", has_lines=1 if a.lines > 0 else 0))
    try:
        dev.upload(0, [s[0] for s in seqs]); dev.upload(1, [s[1] for s in seqs])
        for k in range(4):
            dev.step_dev(k & 1)
        rd = []
        for k in range(a.steps):
            dev.step_dev(k & 1)
            ctx.synchronize()
            t0 = time.perf_counter()
            dev.read()
            rd.append((time.perf_counter() - t0) * 1e3)
        out.update(read_back_ms_median_min_max=[float(np.median(rd)), float(np.min(rd)), float(np.max(rd))],
                   read_back_bytes=B * 700, round_trip_ms_median=float(np.median(rd)) + float(np.median(t)))
    finally:
        dev.close()
        ctx.close()
    print(json.dumps(out))


def resources():
    """VGPRs, AGPRs, scratch of the two kernels of csrc/traj_kernel.hip, from -Rpass-analysis=kernel-resource-usage."""
    src = os.path.join(ROOT, "stvo-pl_amd", "csrc", "traj_kernel.hip")
    p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = "traj_update_kernel" if "traj_update_kernel" in m.group(1) else "traj_init_kernel" if "traj_init_kernel" in m.group(1) else m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\S+)", line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


def spawn(tree, leg, streams, a, trajectory="off"):
    env = dict(os.environ)
    env.pop("STVO_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--streams", str(streams), "--trajectory", trajectory, "--tree", tree,
           "--steps", str(a.steps), "--repeats", str(a.repeats), "--warmup", str(a.warmup), "--points", str(a.points), "--lines", str(a.lines)]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["step", "kernel", "host"], default=None)
    ap.add_argument("--tree", default=ROOT, help="checkout whose python package and library a leg uses")
    ap.add_argument("--parent-tree", default=None, help="built checkout of the parent commit, for off_vs_parent")
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--shapes", default="3072,128")
    ap.add_argument("--trajectory", choices=["off", "on"], default="off")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--points", type=int, default=1650)
    ap.add_argument("--lines", type=int, default=85)
    ap.add_argument("--resources-json", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        use_tree(a.tree)
        {"step": step_leg, "kernel": kernel_leg, "host": host_leg}[a.leg](a)
        return
    doc = dict(what="trajectory and key-frame decision per stream on one MI355X: the step with the feature off against the parent commit "
                    "(alternating runs, one process each), the step with the feature on against off, the update kernel alone, and the host "
                    "alternative (read-back + the host build of the same function on one core)",
               workload=f"KITTI-shaped stereo, {a.points} points + {a.lines} lines per image (+ 20 % distractors), {UNIQUE} distinct synthetic "
                        f"sequences tiled over the streams, two frames per stream resident in HBM; a run = {a.repeats} groups of {a.steps} steps "
                        f"after {a.warmup}, host clock around a stream synchronisation")
    shapes = [int(s) for s in a.shapes.split(",")]
    for B in shapes:
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
        on = [spawn(ROOT, "step", B, a, "on") for _ in range(2)]
        off = [spawn(ROOT, "step", B, a, "off") for _ in range(2)]
        row["on_vs_off"] = dict(on=on, off=off, ms_per_step_on=float(np.median([r["ms_per_step_median"] for r in on])),
                                ms_per_step_off=float(np.median([r["ms_per_step_median"] for r in off])))
        row["on_vs_off"]["us_added_per_step"] = 1e3 * (row["on_vs_off"]["ms_per_step_on"] - row["on_vs_off"]["ms_per_step_off"])
        row["kernel_alone"] = spawn(ROOT, "kernel", B, a)
        row["host"] = spawn(ROOT, "host", B, a)
        doc[f"streams_{B}"] = row
        print(B, json.dumps(row["on_vs_off"]["us_added_per_step"]), row["kernel_alone"], row["host"], flush=True)
    if a.resources_json:
        with open(a.resources_json) as f:
            doc["resources"] = json.load(f)
    else:
        doc["resources"] = resources()
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
