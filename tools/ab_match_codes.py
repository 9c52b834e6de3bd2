#!/usr/bin/env python3
"""A/B of the forward matcher's launch time and the bench headline between an ORDERED list of builds of the library, inside ONE call on
one MI355X (the protocol of tools/ab_pose_prologue.py, for any number of libraries): every library is a libstvo_hip.so selected through
STVO_LIB, child processes of the libraries alternate run by run, and an item is judged against the library BEFORE it in the list.

    python tools/ab_match_codes.py --lib parent=/path/parent.so --lib A=/path/a.so --lib AB=stvo-pl_amd/libstvo_hip.so --out-dir DIR
                                   [--runs 4] [--parts headline,kernel,identity]

headline:  --runs times `python bench.py --gpus 1 --steps 24 --warmup 6` per library (value).  An item counts if its MEDIAN lies above
           the HIGHEST run of the library before it.
kernel:    --runs times the same under `rocprofv3 --kernel-trace --stats` (no counters in the run): average launch time of the dominant
           launch shape of hamming_knn2_mfma_kernel<2, 0> (tools/rocprof_summary.py split).  MEDIAN below the LOWEST run of the one before.
identity:  `bench.py --batch 512 --steps 4 --warmup 2 --dump-outputs` once per library; every array byte for byte against the FIRST library's.
Every child runs under its own `timeout -k 10`; the first one that fails ends the call — nothing more is started on the GPU.
DIR/ab.json is rewritten after every run."""
import argparse
import glob
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "hamming_knn2_mfma_kernel<2, 0>"
ap = argparse.ArgumentParser()
ap.add_argument("--lib", action="append", required=True, metavar="NAME=PATH")
ap.add_argument("--out-dir", required=True)
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--parts", default="headline,kernel,identity")
a = ap.parse_args()
OUT = os.path.abspath(a.out_dir)
os.makedirs(OUT, exist_ok=True)
LIBS = [(s.split("=", 1)[0], os.path.abspath(s.split("=", 1)[1])) for s in a.lib]
for name, path in LIBS:
    if not os.path.exists(path):
        sys.exit("ab_match_codes: no library %s" % path)
PARTS = a.parts.split(",")
BENCH = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"]
CACHE = os.path.join(OUT, "streams.pkl")
HEADLINE = BENCH + ["--steps", "24", "--warmup", "6", "--streams-cache", CACHE]
doc = {"libraries": [n for n, _ in LIBS], "headline_frame_pairs_per_s": {n: {"runs": []} for n, _ in LIBS},
       "k1m_avg_launch_us": {n: {"runs": []} for n, _ in LIBS}, "identity_512_streams": {}, "children": []}


def save():
    with open(os.path.join(OUT, "ab.json"), "w") as f:
        json.dump(doc, f, indent=1)


def child(cmd, name, path, limit, tag):
    import time
    t = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=dict(os.environ, STVO_LIB=path), cwd=ROOT)
    doc["children"].append({"tag": tag, "library": name, "rc": r.returncode, "seconds": round(time.time() - t, 1)})
    with open(os.path.join(OUT, "%s_%s.log" % (tag, name)), "w") as f:
        f.write(r.stdout[-20000:] + "\n---- stderr ----\n" + r.stderr[-20000:])
    save()
    if r.returncode != 0:
        sys.exit("ab_match_codes: %s (%s) failed with %d\n%s" % (tag, name, r.returncode, r.stderr[-1500:]))
    return r


def summary(block):
    for n, _ in LIBS:
        v = block[n]["runs"]
        if v:
            block[n].update(median=statistics.median(v), min=min(v), max=max(v))


if "headline" in PARTS:
    for i in range(a.runs):
        for name, path in LIBS:
            r = child(HEADLINE, name, path, 400, "headline%d" % i)
            v = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"]
            doc["headline_frame_pairs_per_s"][name]["runs"].append(v)
            print("headline", i, name, v, flush=True)
            summary(doc["headline_frame_pairs_per_s"])
            save()
if "kernel" in PARTS:
    for i in range(a.runs):
        for name, path in LIBS:
            d = os.path.join(OUT, "trace_%s_%d" % (name, i))
            child(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--"] + HEADLINE, name, path, 500, "trace%d" % i)
            db = sorted(glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True), key=os.path.getsize)[-1]
            s = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rocprof_summary.py"), "split", db, "hamming_knn2_mfma_kernel<2"],
                               capture_output=True, text=True)
            with open(os.path.join(OUT, "split_%s_%d.txt" % (name, i)), "w") as f:
                f.write(s.stdout + s.stderr)
            avg = float([l.split() for l in s.stdout.splitlines()[1:] if l.strip()][0][4])   # rows come largest total first: the key-point launch
            doc["k1m_avg_launch_us"][name]["runs"].append(avg)
            print("k1m", i, name, avg, flush=True)
            for p in glob.glob(os.path.join(d, "**", "*"), recursive=True):   # the summaries are kept, the traces are not
                if os.path.isfile(p):
                    os.remove(p)
            summary(doc["k1m_avg_launch_us"])
            save()
if "identity" in PARTS:
    sums = {}
    for name, path in LIBS:
        d = os.path.join(OUT, "dump_" + name)
        child(BENCH + ["--batch", "512", "--steps", "4", "--warmup", "2", "--dump-outputs", d], name, path, 400, "identity")
        sums[name] = {os.path.basename(p): hashlib.sha256(open(p, "rb").read()).hexdigest() for p in sorted(glob.glob(os.path.join(d, "*.npy")))}
        for p in glob.glob(os.path.join(d, "*.npy")):
            os.remove(p)
    first = LIBS[0][0]
    doc["identity_512_streams"] = {"arrays": len(sums[first]), "sha256_of_first": sums[first],
                                   "identical_to_first": {n: bool(sums[first]) and sums[n] == sums[first] for n, _ in LIBS[1:]}}
    save()
if os.path.exists(CACHE):
    os.remove(CACHE)
h, k = doc["headline_frame_pairs_per_s"], doc["k1m_avg_launch_us"]
doc["acceptance"] = {}
for (prev, _), (name, _) in zip(LIBS, LIBS[1:]):
    acc = {"against": prev}
    if h[name]["runs"]:
        acc.update(headline_median_above_max_before=h[name]["median"] > h[prev]["max"], headline=[h[name]["median"], h[prev]["max"]])
    if k[name]["runs"]:
        acc.update(k1m_median_below_min_before=k[name]["median"] < k[prev]["min"], k1m_us=[k[name]["median"], k[prev]["min"]])
    doc["acceptance"][name] = acc
save()
print(json.dumps({x: doc[x] for x in doc if x != "children"}))
