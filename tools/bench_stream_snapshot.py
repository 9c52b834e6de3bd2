"""Export and import of single streams (stvo_seq_export_streams_dev / stvo_seq_import_streams_dev): what they cost on one MI355X.
Writes one JSON document, per batch size:

  snapshot           export and import of ALL streams of the pipeline, everything on (motion model, trajectory with key-frames, tracks,
                     key-frame sets) and everything off: ms per call, event-timed around `--calls` back-to-back calls after a warm-up,
                     the blob bytes and the live bytes among them, and a plain device-to-device copy of the blob bytes timed the same way
                     in the same run.  Expectation to confirm or refute: within 2 x the time of that copy.
  host_alternative   (at the small batch) the same state fetched with the existing read calls, one hipMemcpy per piece
  import_then_step   in one process, groups of plain steps alternating with groups in which every `--every`-th step follows an import of
                     one stream: what the import call and the step behind it (which gives up the stages ahead) add over a plain step
  unused_vs_parent   the whole step with no export or import ever called, on this tree against another tree (the parent commit's
                     checkout, built): alternating runs, one process each (the step leg of tools/bench_stream_control.py)

    python tools/bench_stream_snapshot.py --parent-tree /path/to/parent/checkout --out profiles/stream_snapshot_bench.json
    python tools/bench_stream_snapshot.py --leg snapshot --streams 3072 --features on      (one run, one JSON line)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

import bench_stream_control as bsc

ROOT = bsc.ROOT


def make_pipeline(a, features):
    import torch
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    cam, B = synth.KITTI_CAM, a.streams
    uniq = [synth.make_stereo_sequence(synth.frame_seed(b, 0), n_frames=2, n_pts=a.points, n_lines=a.lines, cam=cam) for b in range(min(B, bsc.UNIQUE))]
    seqs = [uniq[b % len(uniq)] for b in range(B)]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    ts = torch.cuda.Stream()
    ctx.set_stream(ts.cuda_stream)   # the library's work on a stream torch can put events on
    dev = capi.Sequences(ctx, B, 2048, 512, cam, match_params("kitti"), opt_params("kitti", has_lines=1 if a.lines > 0 else 0))
    if features:
        dev.set_motion_model(True)
        dev.set_trajectory(capi.traj_params("kitti"), log_steps=1)
        dev.set_tracks(log_steps=1, keyframe_sets=True)
    dev.upload(0, [s[0] for s in seqs])
    dev.upload(1, [s[1] for s in seqs])
    for k in range(4):
        dev.step_dev(k & 1)
    ctx.synchronize()
    return ctx, dev, ts


def timed(ts, fn, calls, warmup, groups=5):
    """Median over groups of the event time of `calls` back-to-back calls of fn, in ms per call."""
    import torch
    out = []
    with torch.cuda.stream(ts):
        for _ in range(warmup):
            fn()
        ts.synchronize()
        for _ in range(groups):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            for _ in range(calls):
                fn()
            e1.record(ts)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / calls)
    return float(np.median(out)), out


def snapshot_leg(a):
    import torch
    from stvo_amd import capi
    features = a.features == "on"
    ctx, dev, ts = make_pipeline(a, features)
    try:
        B, info = a.streams, dev.snapshot_info()
        streams = np.arange(B, dtype=np.int32)
        total = B * info["bytes"]
        with torch.cuda.stream(ts):
            blobs = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
            other = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
        ts.synchronize()
        exp_ms, exp_groups = timed(ts, lambda: dev.export_streams_dev(streams, blobs.data_ptr()), a.calls, a.warmup)
        imp_ms, imp_groups = timed(ts, lambda: dev.import_streams_dev(streams, blobs.data_ptr(), info["bytes"]), a.calls, a.warmup)
        copy_ms, copy_groups = timed(ts, lambda: other.copy_(blobs), a.calls, a.warmup)
        host = blobs.cpu().numpy().reshape(B, -1)
        live = int(sum(int(capi.snapshot_views(host[b])["live"].sum()) for b in range(0, B, max(1, B // 64)))) * max(1, B // 64)
        out = dict(streams=B, features=a.features, flags=info["flags"], bytes_per_stream=info["bytes"], blob_bytes=total, live_bytes_estimate=live,
                   export_ms=exp_ms, export_ms_groups=exp_groups, import_ms=imp_ms, import_ms_groups=imp_groups,
                   import_note="an import call fetches the headers first (one small copy, one synchronisation) and checks them on the host",
                   copy_same_bytes_ms=copy_ms, copy_ms_groups=copy_groups, copy_GBps_read_plus_written=2 * total / copy_ms / 1e6,
                   export_GBps_blob_written=total / exp_ms / 1e6, export_over_copy=exp_ms / copy_ms, import_over_copy=imp_ms / copy_ms,
                   within_2x_of_the_copy=dict(export=bool(exp_ms <= 2 * copy_ms), import_=bool(imp_ms <= 2 * copy_ms)), calls=a.calls)
        if a.host_alternative and features:
            t0 = time.perf_counter()
            for b in range(B):
                dev.debug_stereo(b)
                dev.read_keyframe(b)
            dev.trajectory_state(); dev.keyframe_headers(); dev.read_tracks(1)
            out["host_alternative_ms"] = (time.perf_counter() - t0) * 1e3
            out["host_alternative_note"] = ("debug_stereo + read_keyframe per stream (one hipMemcpy per array: 20 per stream) + trajectory_state, "
                                            "keyframe_headers and read_tracks once; the motion seed and the propagating track copy have no read call")
            t0 = time.perf_counter()
            dev.export_streams(streams)
            out["export_to_host_ms"] = (time.perf_counter() - t0) * 1e3
    finally:
        dev.close()
        ctx.close()
    print(json.dumps(out))


def import_step_leg(a):
    import torch
    ctx, dev, ts = make_pipeline(a, True)
    try:
        info = dev.snapshot_info()
        one = np.zeros(1, np.int32)
        with torch.cuda.stream(ts):
            blob = torch.zeros(info["bytes"], dtype=torch.uint8, device="cuda:0")
        dev.export_streams_dev(one, blob.data_ptr())
        ctx.synchronize()
        k, plain, with_imp, sched = 0, [], [], None
        n_imp = len(range(0, a.steps, a.every))
        for _ in range(a.repeats):
            for groups, use in ((plain, False), (with_imp, True)):
                t0 = time.perf_counter()
                for i in range(a.steps):
                    if use and i % a.every == 0:
                        dev.import_streams_dev(one, blob.data_ptr(), info["bytes"])
                        dev.step_dev(k & 1); k += 1
                        sched = dev.last_schedule()
                    else:
                        dev.step_dev(k & 1); k += 1
                ctx.synchronize()
                groups.append((time.perf_counter() - t0) * 1e3)
        out = dict(streams=a.streams, import_every=a.every, imports_per_group=n_imp, ms_per_group_plain=plain, ms_per_group_with_import=with_imp,
                   ms_per_step_plain=float(np.median(plain)) / a.steps,
                   us_added_per_import_and_step=(float(np.median(with_imp)) - float(np.median(plain))) / n_imp * 1e3,
                   schedule_of_a_step_after_an_import=sched, schedule_of_the_last_plain_step=dev.last_schedule(), steps=a.steps, repeats=a.repeats)
    finally:
        dev.close()
        ctx.close()
    print(json.dumps(out))


def spawn(tree, leg, streams, a, extra=()):
    env = dict(os.environ)
    env.pop("STVO_LIB", None)
    script = os.path.abspath(__file__) if leg != "step" else os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_stream_control.py")
    cmd = [sys.executable, script, "--leg", leg, "--streams", str(streams), "--tree", tree, "--steps", str(a.steps),
           "--repeats", str(a.repeats), "--warmup", str(a.warmup), "--points", str(a.points), "--lines", str(a.lines), *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["snapshot", "import_step"], default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent-tree", default=None, help="built checkout of the parent commit, for unused_vs_parent")
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--shapes", default="3072,128")
    ap.add_argument("--features", choices=["on", "off"], default="on")
    ap.add_argument("--host-alternative", action="store_true")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--points", type=int, default=1650)
    ap.add_argument("--lines", type=int, default=85)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        bsc.use_tree(a.tree)
        {"snapshot": snapshot_leg, "import_step": import_step_leg}[a.leg](a)
        return
    doc = dict(what="export and import of single streams of the device pipeline on one MI355X: all streams per call against a plain device copy of "
                    "the blob bytes, the host alternative, the step behind an import, and the step of a pipeline that never exports or imports "
                    "against the parent commit",
               workload=f"KITTI-shaped stereo, {a.points} points + {a.lines} lines per image (+ 20 % distractors), {bsc.UNIQUE} distinct synthetic "
                        f"sequences tiled over the streams, capacities 2048 / 512, four steps taken before anything is exported")
    shapes = [int(s) for s in a.shapes.split(",")]
    for B in shapes:
        row = dict(snapshot_everything_on=spawn(ROOT, "snapshot", B, a, ["--features", "on", "--calls", str(a.calls)] + (["--host-alternative"] if B == min(shapes) else [])),
                   snapshot_everything_off=spawn(ROOT, "snapshot", B, a, ["--features", "off", "--calls", str(a.calls)]),
                   import_then_step=spawn(ROOT, "import_step", B, a, ["--every", str(a.every)]))
        print(B, {k: (v.get("export_ms"), v.get("import_ms"), v.get("copy_same_bytes_ms")) for k, v in row.items()}, flush=True)
        if a.parent_tree:
            runs = {"parent": [], "this": []}
            for _ in range(a.rounds):   # parent, this, parent, this, ...
                runs["parent"].append(spawn(a.parent_tree, "step", B, a)["ms_per_step_median"])
                runs["this"].append(spawn(ROOT, "step", B, a)["ms_per_step_median"])
                print(B, "parent", runs["parent"][-1], "this", runs["this"][-1], flush=True)
            med = float(np.median(runs["this"]))
            row["unused_vs_parent"] = dict(ms_per_step_runs=runs, parent_median_min_max=[float(np.median(runs["parent"])), min(runs["parent"]), max(runs["parent"])],
                                           this_median_min_max=[med, min(runs["this"]), max(runs["this"])],
                                           gate=dict(statement="this tree's median ms per step lies inside the parent's range (not above its slowest run)",
                                                     this_median=med, parent_slowest_run=max(runs["parent"]), holds=bool(med <= max(runs["parent"]))))
        doc[f"streams_{B}"] = row
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
