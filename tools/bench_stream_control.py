"""Restart and park of single streams between steps (stvo_seq_control_next_step): what the feature costs on one MI355X.  Writes one
JSON document with two measurements per batch size:

  unused_vs_parent   the whole step (stvo_seq_step_dev) with no control ever staged, on this tree against another tree (the parent
                     commit's checkout, built): alternating runs, one process each; this tree's median must lie inside the parent's
                     own spread — an unused control adds no launch, no allocation and no stream operation
  control_vs_plain   in ONE process of this tree, groups of plain steps alternating with groups in which every `--control-every`-th
                     step carries a control (RESTART of 1 stream, and of 10 % of the streams, spread over the batch): the time a
                     control step adds — the host call with its staged copy, two small launches, and at large batches the grid and
                     key-line stage that this step does not run ahead.  A recorded number, no threshold.

    python tools/bench_stream_control.py --parent-tree /path/to/parent/checkout --out profiles/stream_control_bench.json
    python tools/bench_stream_control.py --leg step --streams 3072                     (one run, one JSON line; what the above spawns)

Every leg is a process of its own (fresh context, its own code-object load); it times `--repeats` groups of `--steps` steps by the
host clock around a stream synchronisation, after `--warmup` steps, and reports each group."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIQUE = 64   # distinct synthetic sequences; stream b runs sequence b mod UNIQUE


def use_tree(tree):
    sys.path.insert(0, os.path.join(tree, "stvo-pl_amd", "python"))


def make_pipeline(a):
    import torch  # noqa: F401  (one HIP runtime per process, see capi.load)
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    cam, B = synth.KITTI_CAM, a.streams
    uniq = [synth.make_stereo_sequence(synth.frame_seed(b, 0), n_frames=2, n_pts=a.points, n_lines=a.lines, cam=cam) for b in range(min(B, UNIQUE))]
    seqs = [uniq[b % len(uniq)] for b in range(B)]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    dev = capi.Sequences(ctx, B, 2048, 512, cam, match_params("kitti"), opt_params("kitti", has_lines=1 if a.lines > 0 else 0))
    dev.upload(0, [s[0] for s in seqs])
    dev.upload(1, [s[1] for s in seqs])
    return ctx, dev


def step_leg(a):
    """B streams, two frames per stream resident in HBM, steps alternating between them; no control is ever staged."""
    ctx, dev = make_pipeline(a)
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
        out = dict(streams=a.streams, ms_per_step_groups=groups, ms_per_step_median=float(np.median(groups)),
                   frame_pairs_per_s=a.streams / float(np.median(groups)) * 1e3, committed_pose_fraction=float((res["status"] == 0).mean()),
                   schedule_last_step=dev.last_schedule(), steps=a.steps, repeats=a.repeats, warmup=a.warmup)
    finally:
        dev.close()
        ctx.close()
    print(json.dumps(out))


def control_leg(a):
    """Plain groups and groups with a control in every `control_every`-th step, alternating in one process."""
    from stvo_amd import capi
    ctx, dev = make_pipeline(a)
    try:
        B = a.streams
        n_ctl = max(1, int(round(B * a.control_fraction))) if a.control_fraction > 0 else 1
        ctl = np.zeros(B, np.int32)
        ctl[np.linspace(0, B - 1, n_ctl).astype(int)] = capi.STREAM_RESTART
        k = 0
        for _ in range(a.warmup):
            dev.step_dev(k & 1); k += 1
        ctx.synchronize()
        plain, with_ctl, sched = [], [], None
        n_control_steps = len(range(0, a.steps, a.control_every))
        for _ in range(a.repeats):
            for groups, use in ((plain, False), (with_ctl, True)):
                t0 = time.perf_counter()
                for i in range(a.steps):
                    if use and i % a.control_every == 0:
                        dev.control_next_step(ctl)
                        dev.step_dev(k & 1); k += 1
                        sched = dev.last_schedule()
                    else:
                        dev.step_dev(k & 1); k += 1
                ctx.synchronize()
                groups.append((time.perf_counter() - t0) * 1e3)   # ms per group
        res, _ = dev.read()
        added = (float(np.median(with_ctl)) - float(np.median(plain))) / n_control_steps * 1e3
        out = dict(streams=B, controlled_streams=int(n_ctl), control_every=a.control_every, control_steps_per_group=n_control_steps,
                   ms_per_group_plain=plain, ms_per_group_with_control=with_ctl,
                   ms_per_step_plain=float(np.median(plain)) / a.steps, us_added_per_control_step=added,
                   schedule_of_a_control_step=sched, schedule_of_the_last_plain_step=dev.last_schedule(),
                   committed_pose_fraction=float((res["status"] == 0).mean()), steps=a.steps, repeats=a.repeats, warmup=a.warmup)
    finally:
        dev.close()
        ctx.close()
    print(json.dumps(out))


def spawn(tree, leg, streams, a, extra=()):
    env = dict(os.environ)
    env.pop("STVO_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--streams", str(streams), "--tree", tree, "--steps", str(a.steps),
           "--repeats", str(a.repeats), "--warmup", str(a.warmup), "--points", str(a.points), "--lines", str(a.lines), *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["step", "control"], default=None)
    ap.add_argument("--tree", default=ROOT, help="checkout whose python package and library a leg uses")
    ap.add_argument("--parent-tree", default=None, help="built checkout of the parent commit, for unused_vs_parent")
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--shapes", default="3072,128")
    ap.add_argument("--control-fraction", type=float, default=0.0, help="streams a control restarts, as a fraction of B (0: one stream)")
    ap.add_argument("--control-every", type=int, default=8)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--points", type=int, default=1650)
    ap.add_argument("--lines", type=int, default=85)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        use_tree(a.tree)
        {"step": step_leg, "control": control_leg}[a.leg](a)
        return
    doc = dict(what="restart and park of single streams between steps on one MI355X: the step with no control ever staged against the parent "
                    "commit (alternating runs, one process each), and what a step that carries a control adds over a plain step of the same "
                    "build (groups alternating in one process)",
               workload=f"KITTI-shaped stereo, {a.points} points + {a.lines} lines per image (+ 20 % distractors), {UNIQUE} distinct synthetic "
                        f"sequences tiled over the streams, two frames per stream resident in HBM; a run = {a.repeats} groups of {a.steps} steps "
                        f"after {a.warmup}, host clock around a stream synchronisation; control groups: a RESTART in every {a.control_every}th step")
    for B in [int(s) for s in a.shapes.split(",")]:
        row = {}
        if a.parent_tree:
            runs = {"parent": [], "this": []}
            for _ in range(a.rounds):   # parent, this, parent, this, ...
                runs["parent"].append(spawn(a.parent_tree, "step", B, a)["ms_per_step_median"])
                runs["this"].append(spawn(ROOT, "step", B, a)["ms_per_step_median"])
                print(B, "parent", runs["parent"][-1], "this", runs["this"][-1], flush=True)
            med = float(np.median(runs["this"]))
            row["unused_vs_parent"] = dict(ms_per_step_runs=runs, parent_median_min_max=[float(np.median(runs["parent"])), min(runs["parent"]), max(runs["parent"])],
                                           this_median_min_max=[med, min(runs["this"]), max(runs["this"])],
                                           gate=dict(statement="this tree's median ms per step with no control staged is not above the parent's slowest run",
                                                     this_median=med, parent_slowest_run=max(runs["parent"]), holds=bool(med <= max(runs["parent"]))))
        ctl = ["--control-every", str(a.control_every)]
        row["control_vs_plain"] = dict(one_stream=spawn(ROOT, "control", B, a, ctl + ["--control-fraction", "0"]),
                                       ten_percent=spawn(ROOT, "control", B, a, ctl + ["--control-fraction", "0.1"]))
        doc[f"streams_{B}"] = row
        print(B, {k: v["us_added_per_control_step"] for k, v in row["control_vs_plain"].items()}, flush=True)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
