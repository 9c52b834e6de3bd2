#!/usr/bin/env python3
"""A/B of the batch pose kernel's launch time and the bench headline between two builds of the library, inside ONE call on one MI355X:
child processes of --parent-lib (libstvo_hip.so of a built checkout of the parent commit, through STVO_LIB) and of this tree's library
alternate run by run.  Boxes of a pool differ by a few per cent, so only runs of one call compare.

    python tools/ab_pose_prologue.py --parent-lib /path/to/parent/stvo-pl_amd/libstvo_hip.so --out-dir DIR [--runs 4] [--no-trace]

Per library:  once `STVO_POSE_PROF=1 python bench.py --gpus 1 --steps 4 --warmup 2` (the PROF instantiation: mean prologue / total ticks per
pair, recorded, not gated); --runs times `python bench.py --gpus 1 --steps 24 --warmup 6` (value); --runs times the same under
`rocprofv3 --kernel-trace --stats -- ... --streams-cache FILE` (average launch time of pose2c_kernel's dominant launch shape,
tools/rocprof_summary.py split).  Every child runs under its own `timeout -k 10`; the first one that fails ends the call — nothing more is
started on the GPU.  DIR/ab.json is rewritten after every run; its `acceptance` block applies the rule of profiles/k1m_ragged_ab.json:
new median launch time below the parent's minimum AND new median value above the parent's maximum."""
import argparse
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--out-dir", required=True)
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--no-trace", action="store_true")
a = ap.parse_args()
OUT = os.path.abspath(a.out_dir)
os.makedirs(OUT, exist_ok=True)
PARENT = os.path.abspath(a.parent_lib)
BENCH = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"]
HEADLINE = BENCH + ["--steps", "24", "--warmup", "6"]
doc = {"headline_frame_pairs_per_s": {"parent": {"runs": []}, "this": {"runs": []}},
       "pose2c_avg_launch_us": {"parent": {"runs": []}, "this": {"runs": []}}, "prof_ticks_per_pair": {}, "children": []}
T0 = time.time()


def save():
    with open(os.path.join(OUT, "ab.json"), "w") as f:
        json.dump(doc, f, indent=1)


def child(cmd, which, limit, tag, extra_env=None):
    env = dict(os.environ, **(extra_env or {}))
    if which == "parent":
        env["STVO_LIB"] = PARENT
    t = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    doc["children"].append({"tag": tag, "library": which, "rc": r.returncode, "seconds": round(time.time() - t, 1)})
    with open(os.path.join(OUT, "%s_%s.log" % (tag, which)), "w") as f:
        f.write(r.stdout[-20000:] + "\n---- stderr ----\n" + r.stderr[-20000:])
    save()
    if r.returncode != 0:
        sys.exit("ab_pose_prologue: %s (%s) failed with %d\n%s" % (tag, which, r.returncode, r.stderr[-1500:]))
    return r


def summary(block):
    for which in ("parent", "this"):
        v = block[which]["runs"]
        if v:
            block[which].update(median=statistics.median(v), min=min(v), max=max(v))


for which in ("parent", "this"):
    r = child(BENCH + ["--steps", "4", "--warmup", "2"], which, 400, "prof", {"STVO_POSE_PROF": "1"})
    line = [l for l in r.stderr.splitlines() if "[pose prof]" in l][-1]
    doc["prof_ticks_per_pair"][which] = {"prologue": int(re.search(r"prologue (\d+)", line).group(1)),
                                         "total": int(re.search(r"total (\d+)", line).group(1)), "line": line}
    save()
for i in range(a.runs):
    for which in ("parent", "this"):
        r = child(HEADLINE, which, 400, "headline%d" % i)
        v = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"]
        doc["headline_frame_pairs_per_s"][which]["runs"].append(v)
        print("headline", i, which, v, flush=True)
        summary(doc["headline_frame_pairs_per_s"])
        save()
if not a.no_trace:
    cache = os.path.join(OUT, "streams.pkl")
    for i in range(a.runs):
        for which in ("parent", "this"):
            d = os.path.join(OUT, "trace_%s_%d" % (which, i))
            child(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--"] + HEADLINE + ["--streams-cache", cache], which, 500, "trace%d" % i)
            db = sorted(glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True), key=os.path.getsize)[-1]
            s = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rocprof_summary.py"), "split", db, "pose2c_kernel"],
                               capture_output=True, text=True)
            with open(os.path.join(OUT, "split_%s_%d.txt" % (which, i)), "w") as f:
                f.write(s.stdout + s.stderr)
            avg = float([l.split() for l in s.stdout.splitlines()[1:] if l.strip()][0][4])   # rows come largest total first: the step's launch
            doc["pose2c_avg_launch_us"][which]["runs"].append(avg)
            print("pose2c", i, which, avg, flush=True)
            for p in glob.glob(os.path.join(d, "**", "*"), recursive=True):   # the summaries are kept, the traces are not
                if os.path.isfile(p):
                    os.remove(p)
            summary(doc["pose2c_avg_launch_us"])
            save()
    if os.path.exists(cache):
        os.remove(cache)
h, k = doc["headline_frame_pairs_per_s"], doc["pose2c_avg_launch_us"]
if h["this"]["runs"] and k["this"]["runs"]:
    doc["acceptance"] = {"pose2c_new_median_below_parent_min": k["this"]["median"] < k["parent"]["min"],
                         "pose2c_us": [k["this"]["median"], k["parent"]["min"]],
                         "headline_new_median_above_parent_max": h["this"]["median"] > h["parent"]["max"],
                         "headline": [h["this"]["median"], h["parent"]["max"]]}
save()
print(json.dumps({x: doc[x] for x in doc if x != "children"}))
