#!/usr/bin/env python3
"""bench.py — stereo frame pairs/s through the per-frame hot path of PL-StVO on MI355X.

One "step" = one pass of the WHOLE hot path over one batch: B independent stereo sequences advance by one frame each
through the device-resident pipeline (stvo_seq_step_dev): stereo association of points and lines on the 64x48 grid
(matchGrid), f2f brute-force mutual-NNR matching of points and lines (match), optimizePose — BASELINE.json configs[2]
(KITTI-00-shaped stereo with points + lines, ~2000 ORB key-points and ~100 key-lines per image, config_kitti.yaml).
The B streams of a rank cycle through the eight sequence ids of configs[4] with the calibration of their KITTI dataset
(kitti00-02 / kitti03 / kitti04-10); stream g = rank + world * b is sequence g mod 8, i.e. sequence s lives on rank
s mod G.  Every stream keeps `--slots` consecutive frames resident in HBM and the steps ping-pong through them, so the
per-step working set (>= 4 x ~110 MB of raw features + the stereo sets and scratch) does not fit the 256 MB Infinity Cache.
Prints ONE JSON line (rank 0).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--slots S] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times exactly K steps once and prints the line.  `--full` adds everything else the benchmark
measures or checks, after the timed region: the region repeated (`--repeats`, median), rocm-smi clocks, per-stage and roofline
passes, the oracle parity sample, the extra legs, the CPU baselines and the full record in bench_extras.json.  `--dump-outputs DIR`
writes the results of the last timed step as DIR/<name>.npy (the inputs are seeded: the same arguments give the same streams).

`--gpus N` without a torch.distributed environment re-executes itself under torch.distributed.run with N ranks (one
process per GPU, RCCL).  Multi-GPU: the path has no exchange step — the only collectives are the timing barrier and the
max / sum reductions of the report (weak scaling: B streams per GPU).
"""
import argparse
import json
import os
import re
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))

HBM_PEAK_GBS = 8000.0        # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s
# K1m takes the 256-bit distances from the matrix cores: 2 x 256 multiply-accumulate ops per (query, train) pair.  Rounds 1-3 ran
# them on i8 operands and priced the kernel against the dense int8 peak (2x the bf16 dense peak, MI355X_MICROARCH.md: bf16 ~2.5 PF
# dense, "i8 ~2x bf16 rate (2xK)"; micro-benchmark floor 4404 TOP/s); round 4 runs them on FP4 (e2m1) operands of the block-scaled
# instruction, whose dense peak is ~10 PF (measured floor 9099 TF, same guide).  `roofline.peak` is the peak of the instruction the
# kernel uses (FP4: 10000); `roofline.int8_equivalent` prices the same launch against the 5000 the earlier rounds (and the round-3
# verdict's target for this kernel) were quoted on.
I8_MFMA_PEAK_TOPS = 5000.0
I8_MFMA_MEASURED_FLOOR_TOPS = 4404.0
FP4_MFMA_PEAK_TOPS = 10000.0
K1M_OPS_PER_PAIR = 2 * 256
PREV_PROFILE_TAG = "r05"
PROFILE_TAG = "r06"          # committed rocprofv3 PMC passes the `traffic` figures are read from
FP64_PEAK_TFLOPS = 78.6      # MI355X_MICROARCH.md: vector FP64 (the matrix FP64 rate is the same on gfx950)
TOL_RAD, TOL_M = 1e-4, 1e-3  # BASELINE.json north_star: pose within 1e-4 rad / 1e-3 m of the reference CPU path per frame


def counter_calibration(path):
    """(FETCH_SIZE factor, WRITE_SIZE factor) a committed counter file states in its line '# calibration: FETCH_SIZE x <f> WRITE_SIZE x <w>'
    (measured by tools/hbm_calib on known byte counts: on gfx950 FETCH_SIZE tallies its 128-byte requests at 64 bytes).  (1, 1) if absent."""
    try:
        for line in open(path):
            if line.startswith("# calibration:"):
                f = line.replace(",", " ").split()
                return float(f[f.index("FETCH_SIZE") + 2]), float(f[f.index("WRITE_SIZE") + 2])
    except (OSError, ValueError, IndexError):
        pass
    return 1.0, 1.0


def committed_traffic(kernel, col=1):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes (FETCH_SIZE + WRITE_SIZE, separate
    `--pmc` runs summarised by tools/rocprof_summary.py; values there are KB per dispatch: n, avg, min, max), each counter times the
    calibration factor its file states.  `col`: 1 = the average over the launches, 3 = the largest launch (a kernel that also runs on
    the small key-line problems).  The newest committed pass that lists the kernel is used (this round's, else the previous
    round's).  None if unavailable."""
    for tag in (PROFILE_TAG, PREV_PROFILE_TAG):
        path = os.path.join(ROOT, "profiles", f"{tag}_hbm_counters.txt")
        try:
            cal_f, cal_w = counter_calibration(os.path.join(ROOT, "profiles", f"{PROFILE_TAG}_hbm_counters.txt"))  # (a property of the counters)
            tot = {}
            for line in open(path):
                f = line.split()
                if len(f) >= 6 and f[4] in ("FETCH_SIZE", "WRITE_SIZE") and kernel in line and f[4] not in tot:
                    tot[f[4]] = float(f[col]) * 1024.0
            if len(tot) == 2:
                return tot["FETCH_SIZE"] * cal_f + tot["WRITE_SIZE"] * cal_w
        except (OSError, ValueError, KeyError):
            pass
    return None


_CAL = counter_calibration(os.path.join(ROOT, "profiles", f"{PROFILE_TAG}_hbm_counters.txt"))
TRAFFIC_SRC = (f"bytes per launch = {_CAL[0]:g} x FETCH_SIZE + {_CAL[1]:g} x WRITE_SIZE of separate rocprofv3 --pmc passes over this command, read "
               f"from the committed profiles/{PROFILE_TAG}_hbm_counters.txt (profiles/{PREV_PROFILE_TAG}_hbm_counters.txt for kernels that file "
               f"does not list; not re-measured by this run); the factors are the calibration that file states (tools/hbm_calib: 2 GiB streamed "
               f"with 4- and 16-byte loads / stores and a 16-of-64-byte gather — FETCH_SIZE reports half the bytes read, WRITE_SIZE the bytes "
               f"written); null when neither file lists the kernel")


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def stream_ids(rank, world, B):
    """(sequence id 0..7, replica) of the B streams of this rank: global stream g = rank + world * b."""
    from stvo_amd import synth
    g = rank + world * np.arange(B)
    return g % synth.CONFIG5_N_SEQUENCES, g // synth.CONFIG5_N_SEQUENCES


def _gen_stream(args):
    from stvo_amd import synth
    s, rep, n_frames, n_pts, n_lines = args[:5]
    return synth.make_config5_sequence(int(s), n_frames=n_frames, n_pts=n_pts, n_lines=n_lines, replica=int(rep),
                                       cluster_kw=args[5] if len(args) > 5 else None)


def generate_streams(seq_ids, replicas, n_frames, n_pts, n_lines, cluster_kw=None):
    jobs = [(s, r, n_frames, n_pts, n_lines, cluster_kw) for s, r in zip(seq_ids, replicas)]
    nproc = min(16, os.cpu_count() or 1, max(1, len(jobs) // 8))   # (at most 16 workers, as for the configs[3] sequences)
    if nproc <= 1:
        return [_gen_stream(j) for j in jobs]
    import multiprocessing as mp
    with mp.get_context("fork").Pool(nproc) as pool:
        return pool.map(_gen_stream, jobs, chunksize=max(1, len(jobs) // (4 * nproc)))


def ping_pong(n_slots):
    """0, 1, .., S-1, S-2, .., 1, 0, 1, ...: every transition is between temporally adjacent frames."""
    period = list(range(n_slots)) + list(range(n_slots - 2, 0, -1))
    k = 0
    while True:
        yield period[k % len(period)]
        k += 1


# ---------------------------------------------------------------------------------------------------------------------
# CPU legs (checker code used ONLY as the timed CPU baseline, after the timed GPU region)
# ---------------------------------------------------------------------------------------------------------------------
def gpu_clocks_under_load(run_some_work, card=0):
    """sclk / mclk / power / power cap of the GPU WHILE it runs the bench workload (rocm-smi, one sample): `rocm-smi` is started,
    run_some_work() keeps enqueueing steps until it has answered.  Lets a slow box be told from a regression (boxes of this pool
    differed by 10 % on identical code in round 3).  Never raises: a missing tool yields {"error": ...}."""
    try:
        p = subprocess.Popen(["rocm-smi", "-d", str(card), "-c", "-P", "--showmaxpower", "--showperflevel", "--json"],
                             stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    except OSError as e:
        return {"error": f"rocm-smi: {e}"}
    t0 = time.perf_counter()
    while p.poll() is None and time.perf_counter() - t0 < 20.0:
        run_some_work()
    try:
        txt = p.communicate(timeout=5)[0]
    except subprocess.SubprocessError:
        p.kill()
        return {"error": "rocm-smi timed out"}
    try:
        d = json.loads(txt[txt.index("{"):])   # (a low-power warning line may precede the JSON)
        c = d.get(f"card{card}", next(iter(d.values())))
    except (ValueError, StopIteration, AttributeError):
        return {"error": "rocm-smi output not parsed", "raw": txt[:300]}
    out = {"source": "rocm-smi -c -P --showmaxpower --showperflevel --json, one sample while bench steps were running"}
    def mhz(v):
        m = re.search(r"([0-9.]+)\s*mhz", str(v), re.I)
        return float(m.group(1)) if m else v
    for k, v in c.items():
        kl = k.lower()
        if "clock speed" in kl:
            for name in ("sclk", "mclk", "fclk", "socclk"):
                if kl.startswith(name): out[name + "_mhz"] = mhz(v)
        elif "max graphics package power" in kl: out["power_cap_w"] = float(v)
        elif "graphics package power" in kl: out["power_w"] = float(v)
        elif "performance level" in kl: out["perf_level"] = v
    return out


def cpu_baseline(n_pts, n_lines, budget_s=12.0):
    """The oracle (scalar C port of the reference path, oracle/stvo_oracle.c) on the same per-frame pipeline — stereo
    association + f2f + optimizePose per frame — on this box's host cores, 1 thread, bounded sample."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    import pipeline_ref
    from stvo_amd import synth
    from stvo_amd.ctypes_types import match_params, opt_params
    orc = oracle_lib.load()
    mp, op = match_params("kitti"), opt_params("kitti")
    nf = 6
    warm = synth.make_config5_sequence(0, n_frames=3, n_pts=n_pts, n_lines=n_lines, replica=900)
    pipeline_ref.run_sequence(orc, warm, synth.config5_cam(0), mp, op)   # untimed: library load, page faults
    done, t_used, k = 0, 0.0, 0
    while t_used < budget_s:
        s = k % synth.CONFIG5_N_SEQUENCES
        sq = synth.make_config5_sequence(s, n_frames=nf, n_pts=n_pts, n_lines=n_lines, replica=901 + k // 8)
        t0 = time.perf_counter()
        pipeline_ref.run_sequence(orc, sq, synth.config5_cam(s), mp, op)
        t_used += time.perf_counter() - t0
        done += nf   # nf stereo associations, nf - 1 x (f2f + optimizePose): counted as nf frames, as the GPU steps are
        k += 1
    return {"value": done / t_used, "unit": "frame-pairs/s", "cores": 1, "kind": "port",
            "sample": f"{k} sequences x {nf} frames of the same workload (stereo association + f2f + optimizePose per frame), "
                      f"oracle/stvo_oracle.c (-O3), {t_used:.1f} s of CPU work, host has {os.cpu_count()} cores",
            "ms_per_frame": t_used / done * 1e3}


def cpu_baseline_fanout(n_pts, n_lines, budget_s=5.0):
    """One stream at the reference's OWN thread structure: points || lines in the stereo association and in f2fTracking
    (stereoFrame.cpp:64-72, stereoFrameHandler.cpp:115-118) and 12 || 21 inside every StVO::match (matching.cpp:69-74) — up to four
    busy threads.  Same results as the sequential loop (tests/test_oracle_matching.py); this is the CPU latency the reference's
    design would show on this box, next to the 1-core figure."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from concurrent.futures import ThreadPoolExecutor
    import oracle_lib
    import pipeline_ref
    from stvo_amd import synth
    from stvo_amd.ctypes_types import match_params, opt_params
    orc = oracle_lib.load()
    mp, op = match_params("kitti"), opt_params("kitti")
    nf = 6
    with ThreadPoolExecutor(6) as ex:
        warm = synth.make_config5_sequence(0, n_frames=3, n_pts=n_pts, n_lines=n_lines, replica=980)
        pipeline_ref.run_sequence(orc, warm, synth.config5_cam(0), mp, op, fanout=ex)
        done, t_used, k = 0, 0.0, 0
        while t_used < budget_s:
            s = k % synth.CONFIG5_N_SEQUENCES
            sq = synth.make_config5_sequence(s, n_frames=nf, n_pts=n_pts, n_lines=n_lines, replica=981 + k // 8)
            t0 = time.perf_counter()
            pipeline_ref.run_sequence(orc, sq, synth.config5_cam(s), mp, op, fanout=ex)
            t_used += time.perf_counter() - t0
            done += nf
            k += 1
    return {"value": done / t_used, "unit": "frame-pairs/s", "cores": 4, "kind": "port", "ms_per_frame": t_used / done * 1e3,
            "sample": f"{k} sequences x {nf} frames, one stream, the reference's thread fan-out (points || lines, 12 || 21: up to 4 busy threads), "
                      f"{t_used:.1f} s"}


def cpu_baseline_threads(n_pts, n_lines, budget_s=6.0):
    """Independent sequences on many host threads (the oracle's C functions run outside the GIL): the all-cores figure
    SURVEY.md §8(d) asks for next to the 1-thread one.  Reported beside `cpu_baseline`, never instead of it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from concurrent.futures import ThreadPoolExecutor
    import oracle_lib
    import pipeline_ref
    from stvo_amd import synth
    from stvo_amd.ctypes_types import match_params, opt_params
    orc = oracle_lib.load()
    mp, op = match_params("kitti"), opt_params("kitti")
    nthr = min(32, os.cpu_count() or 1)
    nf = 4
    n_jobs = max(nthr, int(budget_s * nthr / (nf * 0.009)) // 2)
    seqs = [synth.make_config5_sequence(k % 8, n_frames=nf, n_pts=n_pts, n_lines=n_lines, replica=950 + k // 8) for k in range(min(n_jobs, 2 * nthr))]

    def one(k):
        pipeline_ref.run_sequence(orc, seqs[k % len(seqs)], synth.config5_cam(k % len(seqs) % 8), mp, op)

    with ThreadPoolExecutor(nthr) as ex:
        t0 = time.perf_counter()
        list(ex.map(one, range(n_jobs)))
        dt = time.perf_counter() - t0
    return {"value": n_jobs * nf / dt, "unit": "frame-pairs/s", "cores": nthr, "kind": "port",
            "sample": f"{n_jobs} independent sequences x {nf} frames on {nthr} host threads, {dt:.1f} s"}


def single_stream_latency(local_rank, n_pts, n_lines, n_frames=61):
    """Single-stream latency incl. every H2D / D2H copy and synchronisation (host feature buffers in, pose out) —
    PCIe-inclusive, never `value`: (a) stvo_seq_push through the C-ABI in this process, (b) the imagesStVO loop through
    the StereoFrameHandler mirror (stvo-pl_amd/bin/imagesStVO_synth, "Proc. time"), when the binary exists."""
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    cam = synth.KITTI_CAM
    seq = synth.make_stereo_sequence(synth.frame_seed(77, 0), n_frames=n_frames, n_pts=n_pts, n_lines=n_lines, cam=cam)
    out = {"workload": f"one KITTI-00-shaped sequence, {len(seq[0]['kp_l'])} key-points + {len(seq[0]['kl_l'])} key-lines per image, "
                       f"{n_frames - 1} frame pairs after 10 warm-up frames; host buffers in, pose out (PCIe and synchronisation included)"}
    ctx = capi.Context(device_id=local_rank, max_rows=2048, max_batch=1)
    dev = capi.Sequences(ctx, 1, 2048, 512, cam, match_params("kitti"), opt_params("kitti"))
    try:
        packed = [dev._pack([fr]) for fr in seq]   # the caller's own buffers: packing them is not part of the path
        import ctypes as C
        from stvo_amd.ctypes_types import POSE_RESULT_DTYPE
        res = np.zeros(1, dtype=POSE_RESULT_DTYPE); counts = np.zeros(4, np.int32)
        ts = []
        for k, (ff, keep) in enumerate(packed):
            t0 = time.perf_counter()
            ctx._chk(ctx.lib.stvo_seq_push(dev.h, C.byref(ff), res.ctypes.data_as(C.c_void_p), counts))
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts[10:]) * 1e3
        out["seq_push_ms"] = {"median": float(np.median(ts)), "mean": float(ts.mean()), "p90": float(np.percentile(ts, 90))}
    finally:
        dev.close()
        ctx.close()
    exe = os.path.join(ROOT, "stvo-pl_amd", "bin", "imagesStVO_synth")
    if os.path.exists(exe):
        try:
            import tempfile
            with tempfile.TemporaryDirectory() as td:
                sp = os.path.join(td, "seq.bin")
                synth.write_sequence(sp, seq, cam)
                env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", str(local_rank)))
                txt = subprocess.run([exe, sp, os.path.join(td, "res.bin"), "--preset", "kitti"], capture_output=True, text=True,
                                     timeout=120, env=env).stdout
                m = re.search(r"mean Proc\. time ([0-9.]+) ms, median ([0-9.]+) ms", txt)
                if m:
                    out["handler_ms"] = {"mean": float(m.group(1)), "median": float(m.group(2)),
                                         "what": "StereoFrameHandler mirror (insertStereoPair + optimizePose), app/imagesStVO.cpp:95-98 timed region"}
        except (OSError, subprocess.SubprocessError):
            pass
    return out


# ---------------------------------------------------------------------------------------------------------------------
def configs1_leg(ctx_dev, rank, B=512, n=2000, steps=10):
    """The round-1 headline, kept as an extra key: BASELINE configs[1] — f2f brute-force mutual-NNR match of 2000 x 2000
    ORB rows + optimizePose for B frame pairs resident in HBM (stvo_track_batched_dev)."""
    import torch
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import opt_params
    from stvo_amd.devbatch import TrackBatch
    frames = [synth.make_f2f_points(synth.frame_seed(rank, k), n=n) for k in range(B)]
    batch = TrackBatch(frames, max_pts=2048, max_lines=0, device=ctx_dev)
    prm = opt_params("kitti", has_lines=0)
    ctx = capi.Context(device_id=int(ctx_dev.split(":")[1]), max_rows=2048, max_batch=B)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for _ in range(3):
            ctx.track_batched(batch, synth.KITTI_CAM, prm, 0.75, 0.75, 1)
        ctx.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.track_batched(batch, synth.KITTI_CAM, prm, 0.75, 0.75, 1)
        ctx.synchronize(); torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ok = float((batch.results()["status"] == 0).mean())
        ctx.set_kernel_timing(True)
        for _ in range(steps):
            ctx.track_batched(batch, synth.KITTI_CAM, prm, 0.75, 0.75, 1)
        k1_ms, rev_ms, _ = ctx.get_kernel_timing()
        ctx.set_kernel_timing(False)
        pose_ms = ctx.time_stage(batch, synth.KITTI_CAM, prm, 0.75, 1, 5)
    finally:
        ctx.close()
    ops = float((batch.host["n_prev_pts"].astype(np.int64) * batch.host["n_curr_pts"].astype(np.int64)).sum()) * K1M_OPS_PER_PAIR
    tops = ops / (k1_ms * 1e-3) / 1e12
    return {"workload": "BASELINE configs[1]: f2f brute-force mutual-NNR point match (2000 x 2000 ORB rows) + optimizePose, "
                        f"{B} frame pairs per step resident in HBM (the same batch every step: fits the Infinity Cache)",
            "value": B * steps / dt, "unit": "frame-pairs/s", "ms_per_step": dt / steps * 1e3, "steps": steps,
            "committed_pose_fraction": ok,
            "stage_ms": {"hamming_knn2": k1_ms, "reverse_check": rev_ms, "pose_solo": pose_ms},
            "roofline": {"kernel": "hamming_knn2_mfma_kernel<2, 0>", "bound": "mfma", "achieved": tops, "peak": FP4_MFMA_PEAK_TOPS,
                         "unit": "TFLOP/s", "frac": tops / FP4_MFMA_PEAK_TOPS, "frac_int8_equivalent": tops / I8_MFMA_PEAK_TOPS, "avg_launch_ms": k1_ms,
                         "note": "the same kernel on full 2000 x 2000 problems (8 query tiles of 256 rows, all full): the headline workload's "
                                 "~1650-row sets leave the 7th tile 43 % full"}}


def orb_leg(local_rank, B=256):
    """SURVEY 8(f) rank 3, measured beside the hot path: the ORB point front-end (stvo_orb_detect_levels_dev) on B synthetic
    images resident in HBM — per level FAST-9 + NMS + retainBest + orientation + blur + rBRIEF; KITTI size with one pyramid
    level (config_kitti.yaml) and EuRoC size with four levels at 1.2 (config_euroc.yaml:60-61)."""
    import torch
    from stvo_amd import capi, synth
    K = 2048
    dev = f"cuda:{local_rank}"
    out = {}
    for name, cols, rows, nlev, nfeat in (("kitti_1_level", 1241, 376, 1, 2000), ("euroc_4_levels", 752, 480, 4, 600)):
        base = [synth.make_image(500 + k, cols=cols, rows=rows) for k in range(8)]
        imgs = np.stack([np.roll(base[b % 8], 7 * (b // 8), axis=1) for b in range(B)])
        ctx = capi.Context(device_id=local_rank, max_rows=2048, max_batch=4)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        orb = capi.Orb(ctx, B, cols, rows, max_keypoints=K, nfeatures=nfeat, nlevels=nlev)
        d = dict(img=torch.from_numpy(imgs).to(dev), kp=torch.zeros(B, K, 2, device=dev), resp=torch.zeros(B, K, device=dev),
                 ang=torch.zeros(B, K, device=dev), desc=torch.zeros(B, K, 32, dtype=torch.uint8, device=dev),
                 n=torch.zeros(B, dtype=torch.int32, device=dev), oct=torch.zeros(B, K, dtype=torch.int32, device=dev),
                 nt=torch.zeros(B, dtype=torch.int32, device=dev))

        def run():
            orb.detect_dev(d["img"].data_ptr(), d["kp"].data_ptr(), d["resp"].data_ptr(), d["ang"].data_ptr(), d["desc"].data_ptr(), d["n"].data_ptr(),
                           octave=d["oct"].data_ptr(), n_total=d["nt"].data_ptr())
        try:
            for _ in range(2):
                run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                run()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 5
            nk = float(d["n"].float().mean())
            truncated = int((d["nt"] > d["n"]).sum())
            per_level = [float((d["oct"][:, :int(nk)] == l).float().sum(dim=1).mean()) for l in range(nlev)]
        finally:
            orb.close(); ctx.close()
        px = float(sum((round(cols / 1.2 ** l) * round(rows / 1.2 ** l)) for l in range(nlev)))
        alg = B * (2.0 * px + nk * (8 + 4 + 4 + 4 + 32))   # level images in once, blurred images out once, key-point records out
        out[name] = {"workload": f"{B} synthetic {cols} x {rows} images, orb_nfeatures {nfeat}, FAST threshold 20, {nlev} pyramid level(s)",
                     "levels": nlev, "images_per_s": B / dt, "ms_per_launch": dt * 1e3, "mean_keypoints": nk, "mean_keypoints_per_level": per_level,
                     "images_truncated_at_capacity": truncated,
                     "roofline": {"bound": "hbm", "achieved": alg / dt / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg / dt / 1e9 / HBM_PEAK_GBS,
                                  "algorithmic_bytes_per_launch": alg, "traffic": committed_traffic("orb_fast_nms_kernel") if nlev == 1 else None,
                                  "note": "all kernels of the front-end together; algorithmic bytes = level images read once + blurred images "
                                          "written once + key-point records (score / keep maps are intermediate); traffic = the FAST + NMS kernel's "
                                          "counted bytes (the largest kernel), when a committed PMC pass lists it"}}
    return out


def lsd_leg(local_rank, B=8192, B2=4096):
    """SURVEY 8(f) rank 4, measured beside the hot path: the LSD key-line detector (stvo_lsd_detect_dev) on B synthetic KITTI-size
    images resident in HBM — blur + 1.2x resize, level-line angles, pseudo-ordering (the library's counting sort), region growing +
    rectangles (one wavefront per image), wrapper + top-N cut — and the LBD descriptors of its key-lines (stvo_lbd_compute_dev).
    B = 8192 images per launch (165 GB of the 288 GB: eight images per SIMD hide the search's memory round trips better than four:
    28 k against 24 k images/s); the figure of B2 = 4096 per launch, the batch of rounds 4 - 5, rides along."""
    r = _lsd_leg(local_rank, B)
    if B2 and "images_per_s" in r:
        r2 = _lsd_leg(local_rank, B2, one_image=False)
        r["images_per_s_at_4096_per_launch"] = r2.get("images_per_s")
        r["with_lbd_images_per_s_at_4096_per_launch"] = r2.get("with_lbd_images_per_s")
    return r


def _lsd_leg(local_rank, B, one_image=True):
    import torch
    from stvo_amd import capi, synth
    import oracle_lib
    cols, rows, M = 1241, 376, 128
    dev = f"cuda:{local_rank}"
    base = [synth.make_image(500 + k, cols=cols, rows=rows) for k in range(8)]
    imgs = np.stack([np.roll(base[b % 8], 7 * (b // 8), axis=1) for b in range(B)])
    min_len = 0.025 * rows
    ctx = capi.Context(device_id=local_rank, max_rows=2048, max_batch=4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lsd = capi.Lsd(ctx, B, cols, rows, capi.lsd_params(min_length=min_len, nfeatures=100), max_keylines=M)
    lbd = capi.Lbd(ctx, B, cols, rows, max_keylines=M)
    d = dict(img=torch.from_numpy(imgs).to(dev), kl=torch.zeros(B, M, 6, device=dev), resp=torch.zeros(B, M, device=dev),
             n=torch.zeros(B, dtype=torch.int32, device=dev), desc=torch.zeros(B, M, 32, dtype=torch.uint8, device=dev))
    try:
        def run(with_lbd):
            lsd.detect_dev(d["img"].data_ptr(), d["kl"].data_ptr(), d["resp"].data_ptr(), d["n"].data_ptr())
            if with_lbd:
                lbd.compute_dev(d["img"].data_ptr(), d["kl"].data_ptr(), d["n"].data_ptr(), d["desc"].data_ptr())
        out = {}
        for name, with_lbd in (("lsd", False), ("lsd_lbd", True)):
            run(with_lbd)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                run(with_lbd)
            torch.cuda.synchronize()
            out[name] = (time.perf_counter() - t0) / 3
        nl = d["n"].cpu().numpy()
        kl = d["kl"].cpu().numpy().view(np.float32)
        # parity of the run's own output, after the timed region: the first two images against the oracle
        o = oracle_lib.load()
        ok = True
        t0 = time.perf_counter()
        for b in (0, 1):
            ref = o.lsd_detect(imgs[b], o.lsd_opts(min_length=min_len, nfeatures=100))
            got = kl[b, :nl[b], :4]
            ok = ok and len(ref) == nl[b] and np.array_equal(got, np.stack([ref["sx"], ref["sy"], ref["ex"], ref["ey"]], axis=1))
        cpu_ms = (time.perf_counter() - t0) / 2 * 1e3
    finally:
        lsd.close(); lbd.close(); ctx.close()
    del d
    torch.cuda.empty_cache()
    batch = {"workload": f"{B} synthetic {cols} x {rows} images, lsd_scale 1.2, lsd_refine 0, min_line_length 0.025, lsd_nfeatures 100 (config_kitti.yaml)",
             "images_per_s": B / out["lsd"], "ms_per_launch": out["lsd"] * 1e3, "with_lbd_images_per_s": B / out["lsd_lbd"],
             "mean_keylines": float(nl.mean()), "parity_first_two_images": bool(ok), "oracle_ms_per_image_1_core": cpu_ms}
    if not one_image:
        return batch
    # ONE image (device-resident, host synchronisation included): batches of <= 128 images take the many-waves region growing (one XCD per image up to 8)
    ctx1 = capi.Context(device_id=local_rank, max_rows=2048, max_batch=4)
    ctx1.set_stream(torch.cuda.current_stream().cuda_stream)
    lsd1 = capi.Lsd(ctx1, 1, cols, rows, capi.lsd_params(min_length=min_len, nfeatures=100), max_keylines=M)
    try:
        d1 = dict(img=torch.from_numpy(imgs[:1]).to(dev), kl=torch.zeros(1, M, 6, device=dev), resp=torch.zeros(1, M, device=dev),
                  n=torch.zeros(1, dtype=torch.int32, device=dev))
        ts = []
        for k in range(6):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            lsd1.detect_dev(d1["img"].data_ptr(), d1["kl"].data_ptr(), d1["resp"].data_ptr(), d1["n"].data_ptr())
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t1)
        one_ms = float(np.median(ts[1:]) * 1e3)
        one_ok = int(d1["n"].cpu().numpy()[0]) == int(nl[0]) and np.array_equal(d1["kl"].cpu().numpy().view(np.float32)[0, :nl[0], :4], kl[0, :nl[0], :4])
    finally:
        lsd1.close(); ctx1.close()
    return {**batch, "one_image_ms": one_ms, "one_image_equals_batch_result": bool(one_ok),
            "one_image_vs_oracle_1_core": cpu_ms / one_ms if one_ms > 0 else None,
            "note": "region growing is sequential per image by definition.  Batches: one wavefront per image (~65 ms alone: ~44 k rounds of ~3.4 "
                    "region points, one L2 round trip + ~1500 cycles of dependent instructions each) — the batch is the parallelism, throughput "
                    "still grows from 4096 to 8192 images in flight.  one_image_ms: the many-waves form of batches <= 8 (lsd_grow_xcd_kernel, round 6: one XCD "
                    "per image — a committing wave on an LDS bitmap, a dispatcher and a feeder wave beside it, 64 speculating waves on sixteen "
                    "other CUs, exact), device-resident image, host synchronisation included"}


def images_leg(local_rank, B=128, steps=8, lines=False):
    """SURVEY 8(f) ranks 3 / 4 joined to the hot path: stereo IMAGES in, poses out, nothing through the host — the ORB point
    front-end on 2 B KITTI-size images (lines = True: also the LSD detector + LBD descriptors), the features ingested on the device
    (stvo_seq_upload_dev), then the per-frame pipeline (grid stereo association, f2f, optimizePose) for B streams."""
    import torch
    from stvo_amd import capi, images, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    cam = synth.KITTI_CAM
    nf = 4
    base = [synth.make_stereo_image_sequence(900 + j, nf, cam) for j in range(2)]
    dev = f"cuda:{local_rank}"
    frames = torch.empty((nf, 2 * B, cam["height"], cam["width"]), dtype=torch.uint8, device=dev)
    for k in range(nf):
        for side in (0, 1):
            for b in range(B):  # streams = the two scenes, rolled horizontally (the seam is a vertical edge like any other)
                frames[k, side * B + b] = torch.from_numpy(np.roll(base[b % 2][k][side], 11 * (b // 2), axis=1))
    ctx = capi.Context(device_id=local_rank, max_rows=2048, max_batch=B)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lsd_prm = capi.lsd_params(min_length=0.025 * cam["height"], nfeatures=100) if lines else None
    pipe = images.ImagePipeline(ctx, B, cam, match_params("kitti"), opt_params("kitti", has_lines=1 if lines else 0), max_kp=2048, device=dev,
                                lsd=lsd_prm, max_kl=128)
    order = [0, 1, 2, 3, 2, 1]  # consecutive views are always neighbours of the same scene
    try:
        for k in (0, 1):
            pipe.enqueue(frames[k].data_ptr())
        pipe.seq.read()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ok = 0
        for i in range(steps):
            pipe.enqueue(frames[order[(i + 2) % len(order)]].data_ptr())
        res, counts = pipe.seq.read()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        ok = float((res["status"] == 0).mean())
        nk = float(pipe.n.float().mean())
    finally:
        pipe.close(); ctx.close()
    return {"workload": f"{B} stereo streams of 1241 x 376 image pairs resident in HBM (two synthetic layered scenes, rolled per stream), "
                        "orb_nfeatures 2000, one pyramid level" + (", LSD key-lines (lsd_nfeatures 100) with LBD descriptors" if lines else ", key-points only") +
                        "; per step: ORB" + (" + LSD + LBD" if lines else "") + " on 2 B images -> device ingest -> grid stereo "
                        "association -> f2f -> optimizePose", "stereo_pairs_per_s": B / dt, "ms_per_step": dt * 1e3, "streams": B,
            "mean_keypoints_per_image": nk, "committed_pose_fraction_last_step": ok, "mean_stereo_points_last_step": float(counts[:, 0].mean()),
            "mean_matched_points_last_step": float(counts[:, 2].mean()), "mean_stereo_lines_last_step": float(counts[:, 1].mean()),
            "mean_matched_lines_last_step": float(counts[:, 3].mean())}


CORRELATED_MODELS = {
    "clustered": dict(cluster_frac=0.6, cluster_size=8, spread_p=0.06),
    "heavily_clustered": dict(cluster_frac=0.9, cluster_size=16, spread_p=0.04),
}


def correlated_leg(ctx_dev, rank, B=512, n=2000, steps=8):
    """What the mutual (reverse) check of StVO::match costs when descriptors do NOT discriminate like i.i.d. bits: the
    configs[1] batch (f2f brute-force mutual-NNR match + optimizePose) with clustered descriptor rows (synth.clustered_desc:
    groups of near-duplicates, so that second-best distances overlap the blocking thresholds).  The i.i.d. workload needs
    ZERO reverse distance evaluations; these need the sparse reverse scans.  Live hipEvent timing of the forward scan and of
    plan + reverse scans, and the plan statistics of the last step."""
    import torch
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import opt_params
    from stvo_amd.devbatch import TrackBatch
    prm = opt_params("kitti", has_lines=0)
    out = {}
    for name, kw in [("iid", None)] + list(CORRELATED_MODELS.items()):
        frames = [synth.make_f2f_points(synth.frame_seed(rank + 40, k), n=n, desc_model="iid" if kw is None else "clustered", cluster_kw=kw)
                  for k in range(B)]
        batch = TrackBatch(frames, max_pts=2048, max_lines=0, device=ctx_dev)
        ctx = capi.Context(device_id=int(ctx_dev.split(":")[1]), max_rows=2048, max_batch=B)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            for _ in range(2):
                ctx.track_batched(batch, synth.KITTI_CAM, prm, 0.75, 0.75, 1)
            ctx.synchronize(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ctx.track_batched(batch, synth.KITTI_CAM, prm, 0.75, 0.75, 1)
            ctx.synchronize(); torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ctx.set_kernel_timing(True)
            for _ in range(steps):
                ctx.track_batched(batch, synth.KITTI_CAM, prm, 0.75, 0.75, 1)
            fwd_ms, rev_ms, _ = ctx.get_kernel_timing()
            ctx.set_kernel_timing(False)
            plan = ctx.last_reverse_plan(B).astype(np.int64)
            n1v = batch.host["n_prev_pts"].astype(np.int64)
            res = batch.results()
            out[name] = {"descriptor_model": "i.i.d. bits (SURVEY 8d)" if kw is None else kw, "ms_per_step": dt / steps * 1e3,
                         "forward_scan_ms": fwd_ms, "reverse_check_ms": rev_ms,
                         "claimed_columns": float(plan[0].mean()), "light_columns": float(plan[1].mean()), "heavy_columns": float(plan[2].mean()),
                         "rows_in_S": float(plan[3].mean()), "rows_in_S_fraction": float((plan[3] / np.maximum(n1v, 1)).mean()), "tau": float(plan[4].mean()),
                         "reverse_distance_evaluations_per_frame": float((plan[1] * plan[3] + plan[2] * n1v).mean()),
                         "accepted_matches": float(res["n_matched_pt"].mean()), "committed_pose_fraction": float((res["status"] == 0).mean())}
        finally:
            ctx.close()
    out["note"] = ("reverse check = forward_plan kernel + ONE launch of the sparse reverse scans (hamming_knn2_mfma_reverse_kernel: light columns against "
                   "the rows of S, heavy columns against all rows, the train side of an item resident in LDS; the plan writes m12 as far as the forward top-2 decides it, the scans clear the "
                   "claimants they find blocked; DESIGN.md section 5); the plan of a frame of near-duplicates degrades towards the full reverse scan")
    return out


def clustered_headline_leg(local_rank, streams, cams, S, steps, warmup, repeats, max_keylines, model="clustered"):
    """The HEADLINE workload — same pipeline, same stream count, same slot rotation — on streams whose landmark descriptors are
    clustered (CORRELATED_MODELS["clustered"]: 60 % of the rows in groups of ~8 near-duplicates) instead of i.i.d. bits: the mutual
    check of StVO::match then needs its reverse scans (the i.i.d. rows need none), and the grid matcher sees close second bests.
    value_clustered = frame pairs / s exactly as `value` is formed (median of `repeats` timed regions of `steps` steps)."""
    from stvo_amd import capi
    from stvo_amd.ctypes_types import match_params, opt_params
    B = len(streams)
    mp, op = match_params("kitti"), opt_params("kitti")
    ctx = capi.Context(device_id=local_rank, max_rows=2048, max_batch=B)
    pipe = capi.Sequences(ctx, B, 2048, max_keylines, cams, mp, op)
    try:
        pipe.set_slots(S)
        for k in range(S):
            pipe.upload(k, [st[k] for st in streams])
        ctx.synchronize()
        order = ping_pong(S)
        for _ in range(warmup):
            pipe.step_dev(next(order))
        ctx.synchronize()
        rep = []
        for _ in range(max(1, repeats)):
            t0 = time.perf_counter()
            for _ in range(steps):
                pipe.step_dev(next(order))
            ctx.synchronize()
            rep.append(time.perf_counter() - t0)
        dt = float(np.median(rep))
        pipe.set_stage_timing(True)
        for _ in range(steps):
            pipe.step_dev(next(order))
        stage_ms, n_timed = pipe.get_stage_timing()
        pipe.set_stage_timing(False)
        res, counts = pipe.read()
        return {"descriptor_model": CORRELATED_MODELS.get(model, model), "value": B * steps / dt, "unit": "frame-pairs/s", "ms_per_step": dt / steps * 1e3,
                "streams": B, "steps": steps, "repeats": len(rep), "stage_ms": stage_ms,
                "committed_pose_fraction": float((res["status"] == 0).mean()), "mean_stereo_points": float(counts[:, 0].mean()),
                "mean_matched_points": float(counts[:, 2].mean())}
    finally:
        pipe.close()
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# Parity at the headline shape (checker code, AFTER the timed region): a sample of the bench's own streams against the
# oracle-driven per-frame loop (tests/pipeline_ref.py over oracle/stvo_oracle.c)
# ---------------------------------------------------------------------------------------------------------------------
def rot_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.arccos(min(1.0, max(-1.0, c))))


def parity_sample(pipe, streams, cams, mp, op, order, last_slot, sample):
    """Advance the pipeline by further steps of the bench's own slot order until a forward AND a backward (ping-pong)
    transition have been seen, and compare the streams in `sample` with the oracle on exactly those frame pairs: set sizes,
    match counts, status, path, iteration counts and inlier counts exactly, pose within the north star's tolerance."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    import pipeline_ref
    orc = oracle_lib.load()
    seen, checked, worst_rad, worst_m, bad = set(), 0, 0.0, 0.0, []
    prev = last_slot
    for _ in range(8):
        cur = next(order)
        pipe.step_dev(cur)
        res, counts = pipe.read()
        kind = "forward" if cur > prev else "backward"
        if kind not in seen:
            seen.add(kind)
            for b in sample:
                o = pipeline_ref.run_sequence(orc, [streams[b][prev], streams[b][cur]], cams[b], mp, op)[0]
                r = res[b]
                T = r["T"].reshape(4, 4)
                d_rad, d_m = rot_angle(T[:3, :3], o["T"][:3, :3]), float(np.linalg.norm(T[:3, 3] - o["T"][:3, 3]))
                worst_rad, worst_m = max(worst_rad, d_rad), max(worst_m, d_m)
                same = (int(counts[b, 0]) == o["n_stereo_pt"] and int(counts[b, 1]) == o["n_stereo_ls"]
                        and int(r["n_matched_pt"]) == o["n_matched_pt"] and int(r["n_matched_ls"]) == o["n_matched_ls"]
                        and int(r["status"]) == o["status"] and int(r["path"]) == o["path"] and tuple(int(v) for v in r["iters"]) == tuple(o["iters"])
                        and int(r["n_inliers_pt"]) == o["n_inliers_pt"] and int(r["n_inliers_ls"]) == o["n_inliers_ls"]
                        and d_rad < TOL_RAD and d_m < TOL_M)
                checked += 1
                if not same:
                    bad.append({"stream": int(b), "slots": [int(prev), int(cur)]})
        prev = cur
        if len(seen) == 2:
            break
    return {"streams": len(sample), "frame_pairs_checked": checked, "transitions": sorted(seen), "ok": not bad and len(seen) == 2,
            "max_rot_err_rad": worst_rad, "max_trans_err_m": worst_m, "tolerance": {"rad": TOL_RAD, "m": TOL_M}, "mismatches": bad,
            "what": "streams of THIS run (one per sequence id 0-7, i.e. all three KITTI calibrations) after the timed region, HIP pipeline vs "
                    "oracle/stvo_oracle.c on the same frame pairs: stereo-set sizes, f2f match counts, status, path, iteration counts and inlier "
                    "counts exact; pose within the tolerance"}, prev


CONFIGS3_SHAPE = dict(n_pts=660, n_lines=250, depth=(0.5, 8.0), octave_probs=[.5, .25, .15, .1], outlier_frac=0.4)


def _gen_configs3(args):
    from stvo_amd import synth
    seed, nf = args
    return synth.make_stereo_sequence(synth.frame_seed(3000 + seed, 0), n_frames=nf, cam=synth.EUROC_CAM, **CONFIGS3_SHAPE)


def configs3_leg(local_rank, seqs, B=512, steps=10):
    """BASELINE configs[3] on this round's code: EuRoC-MH_01-shaped 752 x 480 stereo (synthetic rectified intrinsics), ~800
    key-points over 4 octaves, 300 key-lines, depth 0.5-8 m, 40 % point outliers, config_euroc.yaml values; optimiser modes
    0 (GN) / 1 (robust GN) / 2 (LM).  Per mode: batched throughput (B streams, two resident frames), single-stream latency
    (stvo_seq_push, host buffers in / pose out) and the oracle on one host core on the same shape."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C
    import oracle_lib
    import pipeline_ref
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import POSE_RESULT_DTYPE, match_params, opt_params
    cam = synth.EUROC_CAM
    mp = match_params("euroc")
    orc = oracle_lib.load()
    n_dist = len(seqs)
    out = {"workload": f"BASELINE configs[3]: EuRoC-shaped 752 x 480, {len(seqs[0][0]['kp_l'])} key-points over 4 octaves + "
                       f"{len(seqs[0][0]['kl_l'])} key-lines per image, 40 % point outliers, config_euroc.yaml (nnr 0.9, inlier_k 4); "
                       f"{B} streams = {n_dist} distinct synthetic sequences replicated, two resident frames"}
    for mode, name in ((0, "gn"), (1, "robust_gn"), (2, "lm")):
        op = opt_params("euroc", mode=mode)
        ctx = capi.Context(device_id=local_rank, max_rows=2048, max_batch=B)
        dev = capi.Sequences(ctx, B, 1024, 512, cam, mp, op)
        try:
            for k in (0, 1):
                dev.upload(k, [seqs[b % n_dist][k] for b in range(B)])
            for k in range(4):
                dev.step_dev(k & 1)
            ctx.synchronize()
            t0 = time.perf_counter()
            for k in range(steps):
                dev.step_dev(k & 1)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            res, counts = dev.read()
        finally:
            dev.close(); ctx.close()
        # parity of the sample against the oracle on the same frame pair (last step: slot 0 -> slot 1 for even `steps`)
        a, b_ = ((steps - 2) & 1, (steps - 1) & 1)
        ok = True
        for s in range(min(4, n_dist)):
            o = pipeline_ref.run_sequence(orc, [seqs[s][a], seqs[s][b_]], cam, mp, op)[0]
            r = res[s]
            T = r["T"].reshape(4, 4)
            ok = ok and (int(r["status"]) == o["status"] and int(r["path"]) == o["path"] and tuple(int(v) for v in r["iters"]) == tuple(o["iters"])
                         and int(r["n_inliers_pt"]) == o["n_inliers_pt"] and int(r["n_inliers_ls"]) == o["n_inliers_ls"]
                         and rot_angle(T[:3, :3], o["T"][:3, :3]) < TOL_RAD and float(np.linalg.norm(T[:3, 3] - o["T"][:3, 3])) < TOL_M)
        # single stream
        ctx = capi.Context(device_id=local_rank, max_rows=2048, max_batch=1)
        one = capi.Sequences(ctx, 1, 1024, 512, cam, mp, op)
        try:
            pp = ping_pong(len(seqs[0]))             # there and back again: consecutive frames stay neighbours
            packed = [one._pack([seqs[0][next(pp)]]) for _ in range(46)]
            r1 = np.zeros(1, dtype=POSE_RESULT_DTYPE); c1 = np.zeros(4, np.int32)
            ts = []
            for ff, keep in packed:
                t1 = time.perf_counter()
                ctx._chk(ctx.lib.stvo_seq_push(one.h, C.byref(ff), r1.ctypes.data_as(C.c_void_p), c1))
                ts.append(time.perf_counter() - t1)
            lat = float(np.median(np.array(ts[6:]) * 1e3))
        finally:
            one.close(); ctx.close()
        # the oracle on one host core, same shape (bounded: ~1 s per mode)
        pipeline_ref.run_sequence(orc, seqs[1 % n_dist], cam, mp, op)
        t2 = time.perf_counter(); nfr = 0
        for s in range(min(6, n_dist)):
            pipeline_ref.run_sequence(orc, seqs[s], cam, mp, op); nfr += len(seqs[s])
        cpu_ms = (time.perf_counter() - t2) / nfr * 1e3
        out[name] = {"mode": mode, "value": B * steps / dt, "unit": "frame-pairs/s", "ms_per_step": dt / steps * 1e3, "steps": steps,
                     "committed_pose_fraction": float((res["status"] == 0).mean()), "mean_stereo_points": float(counts[:, 0].mean()),
                     "mean_stereo_lines": float(counts[:, 1].mean()), "mean_matched_points": float(counts[:, 2].mean()),
                     "mean_matched_lines": float(counts[:, 3].mean()), "single_stream_push_ms_median": lat,
                     "parity_sampled_ok": bool(ok),
                     "cpu_baseline": {"value": 1e3 / cpu_ms, "unit": "frame-pairs/s", "ms_per_frame": cpu_ms, "cores": 1, "kind": "port",
                                      "sample": f"{min(6, n_dist)} sequences x {len(seqs[0])} frames of this shape, oracle/stvo_oracle.c"},
                     "single_stream_speedup_vs_oracle_1_core": cpu_ms / lat}
    out["note"] = ("mode 1: optimizeFunctionsRobust leaves the residual unscaled (stereoFrameHandler.cpp:813,923), err ~ 6 > 1, so isGoodSolution "
                   "rejects every frame on the GPU exactly as in the oracle (committed_pose_fraction 0); the reference reaches that optimiser "
                   "only as the fallback of :359")
    return out


def headline_record(args, world, backend, frames_total, dt, rep_dt, per_rank, streams, ok_frac):
    """The record of the timed region: the contract's keys and the workload — all a run without --full reports."""
    B, S = len(streams), len(streams[0])
    n_kp = np.array([[len(st[k]["kp_l"]) + len(st[k]["kp_r"]) for k in range(S)] for st in streams], np.float64)  # [B][S]
    resident_mb = S * B * (2 * 2048 * (8 + 32) + 2048 * 4 + 2 * 512 * (16 + 32) + 512 * 4) / 1e6
    return {
        "metric": "stereo frames/s (match+optimizePose)", "value": frames_total / dt, "unit": "frame-pairs/s",
        "n_gpus": world, "rccl_ranks": world, "collective_backend": ("rccl" if backend == "nccl" else backend), "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
        "repeats": {"n": len(rep_dt), "statistic": "median", "value_min": frames_total / max(rep_dt), "value_max": frames_total / min(rep_dt),
                    "ms_per_step_all": [d / args.steps * 1e3 for d in rep_dt]},
        "parity_sampled": None,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8/fp4+f64", "data": "synthetic",
        "config": {"workload": "BASELINE configs[2]: KITTI-00-shaped stereo with points + lines (ORB + LBD rows), grid-windowed stereo "
                               "match (points and lines) + f2f brute-force mutual-NNR match (points and lines) + full GN optimizePose "
                               "(config_kitti.yaml), device-resident per-frame pipeline; the streams cycle through the 8 sequence ids / 3 "
                               "KITTI calibrations of configs[4] (sequence s on rank s mod G)",
                   "streams_per_gpu": B, "resident_frames_per_stream": S, "slot_order": "ping-pong",
                   "resident_raw_features_MB_per_gpu": resident_mb,
                   "keypoints_per_image": float(n_kp.mean() / 2), "keylines_per_image": float(np.mean([len(st[0]["kl_l"]) for st in streams])),
                   "cameras": "kitti00-02 (seq 0-2), kitti03 (seq 3), kitti04-10 (seq 4-7)",
                   "parallelism": f"seq-shard x{world}", "committed_pose_fraction": ok_frac},
        "per_rank_frame_pairs_per_s": per_rank if world > 1 else None,
        # (the driver computes scaling efficiency itself; this is a convenience when the N = 1 value of the same box is handed in)
        "scaling_efficiency_vs_n1": (frames_total / dt / (world * float(os.environ["STVO_N1_VALUE"]))
                                     if world > 1 and os.environ.get("STVO_N1_VALUE") else None),
    }


SHORT_LINE_MAX = 6000   # bytes: the driver keeps a bounded tail of stdout — round 5's 20 KB line was recorded as "parsed": null


def _num(v, nd=6):
    """Numbers of the short line to `nd` significant digits (every digit beyond is noise of the run)."""
    if isinstance(v, bool) or v is None or isinstance(v, (int, str)):
        return v
    if isinstance(v, float):
        return float(f"{v:.{nd}g}")
    if isinstance(v, dict):
        return {k: _num(x, nd) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_num(x, nd) for x in v]
    return v


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def short_line(full):
    """The ONE stdout line of the driver contract, <= SHORT_LINE_MAX bytes: the contract's keys, the three roofline objects (numbers only),
    cpu_baseline and a number per extra leg.  Every note, every `what` and every extra leg in full goes to bench_extras.json."""
    roof_keys = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_ops_per_launch", "algorithmic_bytes_per_launch",
                 "avg_launch_ms", "launches_timed", "pairs_per_s", "hbm_view_frac")
    out = _pick(full, ("metric", "value", "unit", "n_gpus", "rccl_ranks", "collective_backend", "steps", "warmup", "ms_per_step", "higher_is_better",
                       "scaling", "vs_baseline", "dtype", "data"))
    rep = full.get("repeats") or {}
    out["repeats"] = _pick(rep, ("n", "value_min", "value_max"))
    cfg = full.get("config") or {}
    out["config"] = _pick(cfg, ("workload", "streams_per_gpu", "resident_frames_per_stream", "keypoints_per_image", "keylines_per_image",
                                "mean_stereo_points", "mean_matched_points", "mean_matched_lines", "parallelism", "committed_pose_fraction",
                                "value_clustered", "value_clustered_over_value", "value_1024_streams"))
    par = full.get("parity_sampled")
    out["parity_sampled"] = _pick(par, ("ok", "skipped", "frame_pairs_checked", "max_rot_err_rad", "max_trans_err_m")) if isinstance(par, dict) else par
    for k in ("roofline", "roofline_pose", "roofline_grid_scan"):
        if isinstance(full.get(k), dict):
            out[k] = _pick(full[k], roof_keys)
            if isinstance(full[k].get("fp64_view"), dict):
                out[k]["fp64_frac"] = full[k]["fp64_view"].get("frac")
    if "roofline" in out:
        out["roofline"]["timing"] = "hipEvent pairs, light pass (see bench_extras.json)"
    for k in ("per_rank_frame_pairs_per_s", "scaling_efficiency_vs_n1"):
        if full.get(k) is not None:
            out[k] = full[k]
    cb = full.get("cpu_baseline")
    if isinstance(cb, dict):
        out["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "sample", "ms_per_frame", "ms_per_frame_reference_fanout_4_threads",
                                         "speedup_vs_1_core", "speedup_vs_reference_fanout"))
        ss = cb.get("single_stream_ms")
        if isinstance(ss, dict):
            out["cpu_baseline"]["single_stream_ms"] = _pick(ss, ("seq_push", "handler"))
    # one number per extra leg (the legs in full: bench_extras.json)
    legs = {}

    def leg(name, *path):
        v = full.get(path[0])
        for k in path[1:]:
            v = v.get(k) if isinstance(v, dict) else None
        if isinstance(full.get(path[0]), dict) and "error" in full[path[0]]:
            legs[name] = "error"
        elif v is not None:
            legs[name] = v
    leg("configs1_frame_pairs_per_s", "configs1", "value")
    for m in ("gn", "robust_gn", "lm"):
        leg(f"configs3_{m}_frame_pairs_per_s", "configs3", m, "value")
    leg("configs3_single_stream_ms", "configs3", "gn", "single_stream_push_ms_median")
    leg("configs3_single_stream_vs_oracle_1_core", "configs3", "gn", "single_stream_speedup_vs_oracle_1_core")
    leg("orb_images_per_s", "orb_front_end", "kitti_1_level", "images_per_s")
    leg("images_to_poses_pairs_per_s", "images_to_poses", "stereo_pairs_per_s")
    leg("lsd_images_per_s", "lsd_front_end", "images_per_s")
    leg("lsd_one_image_ms", "lsd_front_end", "one_image_ms")
    leg("lsd_one_image_vs_oracle_1_core", "lsd_front_end", "one_image_vs_oracle_1_core")
    leg("images_to_poses_with_lines_pairs_per_s", "images_to_poses_with_lines", "stereo_pairs_per_s")
    leg("one_stereo_pair_with_lines_ms", "one_stereo_pair_with_lines", "ms_per_step")
    leg("clustered_reverse_check_ms", "reverse_check_correlated", "clustered", "reverse_check_ms")
    if legs:
        out["legs"] = legs
    out["extras_file"] = full.get("extras_file")
    out = _num(out)
    line = json.dumps(out, separators=(",", ":"))
    if len(line) > SHORT_LINE_MAX:   # never again: drop the optional parts in order until it fits
        for k in ("legs", "roofline_grid_scan", "roofline_pose"):
            out.pop(k, None)
            line = json.dumps(out, separators=(",", ":"))
            if len(line) <= SHORT_LINE_MAX:
                break
    return line


def write_extras(full, path=None):
    """Everything the run measured, with every note: bench_extras.json beside bench.py (and in gpurun_out/ when that exists)."""
    paths = [path or os.path.join(ROOT, "bench_extras.json")]
    if os.path.isdir(os.path.join(ROOT, "gpurun_out")):
        paths.append(os.path.join(ROOT, "gpurun_out", "bench_extras.json"))
    written = None
    for q in paths:
        try:
            with open(q, "w") as f:
                json.dump(full, f, indent=1)
            written = written or os.path.relpath(q, ROOT)
        except OSError:
            pass
    return written


DUMP_MAX_BYTES = 63 * 10**6   # (--dump-outputs writes at most 64 MB, the .npy headers included)


def dump_outputs(out_dir, res, counts, suffix=""):
    """--dump-outputs: the last timed step's stvo_seq_read results — every field of the pose record of every stream and the
    per-stream set sizes (stereo points, stereo lines, matched points, matched lines) — as float64 arrays, one DIR/<name>.npy each.
    Past DUMP_MAX_BYTES in all, a fixed seeded sample of the streams is written, with their indices in stream_index.npy."""
    arrays = {name: res[name].astype(np.float64) for name in res.dtype.names}
    arrays["counts"] = counts.astype(np.float64)
    n = len(counts)
    row_bytes = sum(a[:1].nbytes for a in arrays.values())
    if n * row_bytes > DUMP_MAX_BYTES:
        rows = np.sort(np.random.default_rng(0).choice(n, DUMP_MAX_BYTES // (row_bytes + 8), replace=False))
        arrays = {k: a[rows] for k, a in arrays.items()}
        arrays["stream_index"] = rows.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=3072, help="independent stereo sequences (streams) per GPU: three residency rounds of the pose kernel (round 6: 1.29 M frame pairs/s "
                         "at 1024, 1.33 M at 2048, 1.37 M at 3072, 1.37 M at 4096 — the event gaps of a step and the pose kernel's tail are paid once per step); the committed PMC passes "
                         "(roofline traffic) are of this default; config.value_1024_streams keeps the figure of rounds 2 - 5's batch")
    ap.add_argument("--slots", type=int, default=4, help="consecutive frames of every stream kept resident in HBM")
    ap.add_argument("--points", type=int, default=1650, help="landmarks per stream; + 20 %% distractors ~ 2000 key-points per image")
    ap.add_argument("--lines", type=int, default=85, help="3-D segments per stream; + 20 %% distractors ~ 100 key-lines per image")
    ap.add_argument("--max-keylines", type=int, default=128,
                    help="key-line capacity per image of the pipeline (config_kitti.yaml: lsd_nfeatures 100; the library allows up to 512)")
    ap.add_argument("--repeats", type=int, default=None, help="the timed region (exactly --steps steps between barriers) is repeated this often; value = median "
                    "(default: 1, with --full 5)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: repeated timed regions, the rocm-smi clock sample, the per-stage "
                    "and roofline passes, the oracle parity sample, the extra legs, the CPU baselines and bench_extras.json.  Without it a run sets up, "
                    "warms up, times --steps steps once and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed (the pose results and set sizes a "
                    "caller of stvo_seq_read receives, one float64 .npy per field) into DIR")
    ap.add_argument("--no-parity", action="store_true", help="(--full) skip the oracle parity sample after the timed region (counter passes: every dispatch costs seconds)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baselines")
    ap.add_argument("--no-clocks", action="store_true", help="(--full) skip the rocm-smi clock sample (it keeps enqueueing steps until rocm-smi answers: counter passes, where every dispatch costs seconds)")
    ap.add_argument("--no-extras", action="store_true", help="(--full) skip the latency / configs[1] / correlated-descriptor legs")
    ap.add_argument("--print-extras", action="store_true", help="(--full) also print the full record (bench_extras.json) on stderr")
    ap.add_argument("--streams-cache", default=None, help="pickle file for the synthetic streams of rank 0: written when absent, read when present — counter passes "
                    "(rocprofv3 --pmc) then start without forking generator processes under the profiler, which is where they tend to hang on this pool")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    extras = args.full and not args.no_extras

    # ---- `--gpus N` from a plain `python bench.py`: spawn N ranks (one process per GPU) under torch.distributed.run
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import torch
        n_vis = torch.cuda.device_count()
        # STVO_BENCH_BACKEND=gloo (tests on a 1-GPU box): the ranks share the visible GPU(s), the barrier and the two scalar
        # all-reduces run over gloo with CPU tensors — everything else of the N > 1 branch is the code an 8-GPU node executes
        if n_vis < args.gpus and os.environ.get("STVO_BENCH_BACKEND", "nccl") != "gloo":
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {n_vis} GPU(s) visible")
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd, env=env))

    from stvo_amd import shard, synth
    world, rank, local_rank = shard.env_world()
    # synthetic streams first: the generator forks worker processes, which must happen before this process touches the GPU
    B, S = args.batch, max(2, min(args.slots, 16))
    seq_ids, replicas = stream_ids(rank, world, B)
    cache = args.streams_cache if (args.streams_cache and world == 1) else None
    if cache and os.path.exists(cache):
        import pickle
        with open(cache, "rb") as f:
            streams = pickle.load(f)
        if len(streams) != B or len(streams[0]) != S:
            raise SystemExit(f"--streams-cache {cache}: holds {len(streams)} streams x {len(streams[0])} frames, this run wants {B} x {S}")
    else:
        streams = generate_streams(seq_ids, replicas, S, args.points, args.lines)
        if cache:
            import pickle
            with open(cache, "wb") as f:
                pickle.dump(streams, f, protocol=4)
    streams_cl = None
    if rank == 0 and world == 1 and extras:   # the same streams with clustered landmark descriptors (value_clustered)
        streams_cl = generate_streams(seq_ids, replicas, S, args.points, args.lines, cluster_kw=CORRELATED_MODELS["clustered"])
    c3_seqs = None
    if rank == 0 and world == 1 and extras:   # configs[3] sequences, also before the GPU is touched (fork)
        import multiprocessing as mp_
        with mp_.get_context("fork").Pool(min(16, os.cpu_count() or 1)) as pool:
            c3_seqs = pool.map(_gen_configs3, [(k, 5) for k in range(64)])

    import torch
    from stvo_amd import capi
    from stvo_amd.ctypes_types import match_params, opt_params
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a MI355X: the product path has no CPU fallback")
    backend = os.environ.get("STVO_BENCH_BACKEND", "nccl") if world > 1 else None
    if backend == "gloo":      # ranks may outnumber the GPUs: rank r runs on GPU r mod (visible GPUs)
        local_rank = local_rank % torch.cuda.device_count()
        dist.init_process_group("gloo")
    elif world > 1:            # "nccl" IS RCCL on ROCm
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
    if args.gpus != world and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but the torch.distributed world has {world} rank(s); reporting n_gpus = {world}", file=sys.stderr)
    torch.cuda.set_device(local_rank)
    dev_name = f"cuda:{local_rank}"
    agg_dev = "cpu" if backend == "gloo" else dev_name   # where the two scalars of shard.aggregate live

    cams = [synth.config5_cam(int(s)) for s in seq_ids]
    mp, op = match_params("kitti"), opt_params("kitti")
    ctx = capi.Context(device_id=local_rank, max_rows=2048, max_batch=B)
    pipe = capi.Sequences(ctx, B, 2048, args.max_keylines, cams, mp, op)
    pipe.set_slots(S)
    for k in range(S):
        pipe.upload(k, [st[k] for st in streams])
    ctx.synchronize()
    order = ping_pong(S)

    last_slot = None
    for _ in range(args.warmup):
        last_slot = next(order); pipe.step_dev(last_slot)
    ctx.synchronize()
    # ---- the timed region: EXACTLY --steps steps between barrier + synchronize on both sides, max over ranks; repeated
    # --repeats times back to back, `value` = the median repeat (min / max beside it)
    rep_dt, rep_dt_local = [], []
    frames_total = B * args.steps * world
    for _ in range(max(1, args.repeats)):
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last_slot = next(order); pipe.step_dev(last_slot)
        ctx.synchronize()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        dt_r = time.perf_counter() - t0
        rep_dt_local.append(dt_r)
        frames_total, dt_r = shard.aggregate(dist, B * args.steps, dt_r, device=agg_dev)   # sum of frame pairs, max of seconds
        rep_dt.append(dt_r)
    dt = float(np.median(rep_dt))
    # reporting only: every rank's own rate (its frame pairs / its own median time), gathered to rank 0
    per_rank = shard.gather_scalars(dist, B * args.steps / float(np.median(rep_dt_local)), device=agg_dev)

    res, counts = pipe.read()   # the results of the last timed step, as a caller of the path receives them
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, res, counts, suffix=f".rank{rank}" if world > 1 else "")

    clocks = None
    if rank == 0 and args.full and not args.no_clocks:   # outside the timed region: a few hundred more steps while rocm-smi takes its sample
        def _work():
            nonlocal last_slot
            for _ in range(8):
                last_slot = next(order); pipe.step_dev(last_slot)
            ctx.synchronize()
        clocks = gpu_clocks_under_load(_work, card=local_rank)
        res, counts = pipe.read()
    ok_frac = float((res["status"] == 0).mean())   # sanity: the timed work produced real poses

    out = None
    if rank == 0 and not args.full:   # the headline alone
        out = headline_record(args, world, backend, frames_total, dt, rep_dt, per_rank, streams, ok_frac)
    elif rank == 0:
        # ---- per-kernel figures, measured LIVE behind the timed region, same streams, same slot order, hipEvent pairs on the stream the
        # kernels run on.  Two passes.  (B) counting pass: an event pair around EVERY stage and a read after every step -> `stage_ms`
        # (bench_extras.json only: the markers change what runs beside what) and the set sizes / match counts / evaluations of every slot
        # transition, which depend on the transition alone.  (A) light pass: the steps back to back exactly as in the timed region —
        # key-line stream unmarked, next frame's grid built ahead on it — with pairs around the three big kernels of the point stream
        # only (stvo_seq_set_stage_timing(.., 2)) -> `roofline*`: each kernel keeps the neighbours it has in the region that produced
        # `value` (profiles/<tag>_kernel_stats.txt is the rocprofv3 view of the same command).
        pipe.set_stage_timing(True)
        per_tr = {}   # (prev slot, slot) -> (pairs, n1, n2, matched points, matched lines, evaluations)
        n_by_slot = {}
        prev_counts, prev_slot = counts, last_slot
        for _ in range(args.steps):
            last_slot = next(order); pipe.step_dev(last_slot)
            r_k, c_k = pipe.read()
            n_prev, n_curr = prev_counts[:, 0].astype(np.int64), c_k[:, 0].astype(np.int64)
            per_tr[(prev_slot, last_slot)] = (float((n_prev * n_curr).sum()), float(n_prev.sum()), float(n_curr.sum()),
                                              float(c_k[:, 2].sum()), float(c_k[:, 3].sum()), float(r_k["iters"].sum()))
            n_by_slot[last_slot] = float(n_curr.sum())
            prev_counts, prev_slot = c_k, last_slot
        stage_ms_full, n_timed_full = pipe.get_stage_timing()
        pipe.set_stage_timing(2)
        tr_seq = []
        for _ in range(args.steps):
            prev_slot, last_slot = last_slot, next(order)
            pipe.step_dev(last_slot)
            tr_seq.append((prev_slot, last_slot))
        ctx.synchronize()
        stage_ms, n_timed = pipe.get_stage_timing()
        pipe.set_stage_timing(False)
        missing = [t for t in tr_seq if t not in per_tr]
        if missing:   # (fewer steps than the slot period: count the transitions the counting pass did not see)
            for t in dict.fromkeys(missing):
                pipe.step_dev(t[0]); _, c_a = pipe.read()
                pipe.step_dev(t[1]); r_k, c_k = pipe.read()
                n_prev, n_curr = c_a[:, 0].astype(np.int64), c_k[:, 0].astype(np.int64)
                per_tr[t] = (float((n_prev * n_curr).sum()), float(n_prev.sum()), float(n_curr.sum()),
                             float(c_k[:, 2].sum()), float(c_k[:, 3].sum()), float(r_k["iters"].sum()))
            last_slot = missing[-1][1]
        pairs, n1s, n2s, nps, nls, evals = (list(v) for v in zip(*[per_tr[t] for t in tr_seq]))
        # parity at the headline shape: 8 streams of this run (sequence ids 0-7 = all three calibrations) vs the oracle
        if args.no_parity:
            parity = {"skipped": True}
        else:
            parity, last_slot = parity_sample(pipe, streams, cams, mp, op, order, last_slot, list(range(min(8, B))))
        n_kp = np.array([[len(st[k]["kp_l"]) + len(st[k]["kp_r"]) for k in range(S)] for st in streams], np.float64)  # [B][S]
        pairs_l, n1_l, n2_l, np_l, nl_l = (float(np.mean(v)) for v in (pairs, n1s, n2s, nps, nls))

        # K1m forward scan: every prev stereo point against every curr stereo point, one launch per step
        k1_ms = stage_ms["hamming_knn2"]
        ops = pairs_l * K1M_OPS_PER_PAIR
        k1_bytes = 32.0 * (n1_l + n2_l) + 8.0 * n1_l      # descriptors in once, one packed top-2 per prev row out
        k1_tops = ops / (k1_ms * 1e-3) / 1e12 if k1_ms > 0 else 0.0
        timing = ("hipEvent pairs around the launch on its stream, over K more steps enqueued back to back as in the timed region "
                  "(markers on these three kernels only; key-line stream unmarked)")
        k1_name = "hamming_knn2_mfma_kernel<2, 0>"
        roofline = {"kernel": k1_name, "bound": "mfma", "achieved": k1_tops, "peak": FP4_MFMA_PEAK_TOPS, "unit": "TFLOP/s",
                    "unit_note": "multiply-accumulate ops (TOP/s), 2 x 256 per 256-bit Hamming distance, on FP4 (e2m1) operands: peak = the dense "
                                 "FP4 / FP6 figure of MI355X_MICROARCH.md",
                    "frac": k1_tops / FP4_MFMA_PEAK_TOPS,
                    "int8_equivalent": {"peak": I8_MFMA_PEAK_TOPS, "frac": k1_tops / I8_MFMA_PEAK_TOPS,
                                        "note": "the same launch against the dense int8 peak the kernel was priced on while it used i8 operands "
                                                "(rounds 1-3: 0.57 - 0.60)"}, "traffic": committed_traffic(k1_name, col=3),  # the key-point launch (the key-line launch of the same kernel is ~20x smaller)
                    "traffic_source": TRAFFIC_SRC,
                    "algorithmic_ops_per_launch": ops, "algorithmic_bytes_per_launch": k1_bytes, "avg_launch_ms": k1_ms, "launches_timed": n_timed,
                    "timing": timing, "frac_of_measured_mfma_floor": k1_tops / 9099.0,  # register-only FP4 floor of the guide
                    "hbm_view_frac": k1_bytes / (k1_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if k1_ms > 0 else 0.0,
                    # SURVEY.md section 8(d)'s own units for match_bf: unique (query, train) distances per second, and the integer-VALU
                    # work the reference formulation would need for them (8 x (v_xor + v_bcnt) = 16 lane-ops per pair) against the
                    # 39.3 T lane-ops/s VALU roof the survey prices the path on — above 1 because the distances come from the matrix
                    # cores (the bit-exact parity tests are the evidence that they are all computed)
                    "pairs_per_s": pairs_l / (k1_ms * 1e-3) if k1_ms > 0 else 0.0,
                    "valu_roof_equivalent": {"lane_ops_per_pair": 16, "peak_lane_ops_per_s": 3.93e13,
                                             "frac": 16.0 * pairs_l / (k1_ms * 1e-3) / 3.93e13 if k1_ms > 0 else 0.0},
                    "note": "dominant kernel: all-pairs Hamming distances of the f2f point match as a Gram matrix of +-4 FP4 elements on the "
                            "matrix cores (v_mfma_scale_f32_32x32x64_f8f6f4), top-2 fold in the shadow of the matrix instructions; ~56 k "
                            "bit-operations per compulsory byte, so HBM is idle by construction (hbm_view_frac)"}
        # pose kernel: priced against HBM (SURVEY.md §8d gn_accumulate + remove_outliers: records once, m12 + inlier masks, result)
        pose_ms = stage_ms["pose"]
        # round 4: the stereo points are compact records ({u, v, disparity, level} = 16 B): a matched point costs its own record
        # and its observation's (32 B), an unmatched prev point its record (16 B, read to find out nothing matches it)
        pose_bytes = 32.0 * np_l + 16.0 * (n1_l - np_l) + 116.0 * nl_l + 8.0 * n1_l + 8.0 * (B * 64.0) + B * 840.0
        pose_gbs = pose_bytes / (pose_ms * 1e-3) / 1e9 if pose_ms > 0 else 0.0
        # kernel the library picks for this batch size (csrc/pose_kernel.hip: launch_pose), as rocprofv3 names it
        forced = os.environ.get("STVO_POSE_KERNEL", "")
        pose_name = {"1": "pose_kernel<", "4": "pose2c_kernel<"}.get(forced, "pose_kernel<" if B <= 256 else "pose2c_kernel<")
        # FP64 view (SURVEY.md §8d gn_accumulate): 150 flop per point and 400 per line and evaluation; evaluations = the iteration
        # counts the kernel reports (stage 1 + refinement), all matched features priced at every evaluation
        evals_l = float(np.mean(evals)) / B
        pose_flops = (150.0 * np_l + 400.0 * nl_l) * evals_l
        pose_tf = pose_flops / (pose_ms * 1e-3) / 1e12 if pose_ms > 0 else 0.0
        roofline_pose = {"kernel": pose_name, "bound": "hbm", "achieved": pose_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": pose_gbs / HBM_PEAK_GBS, "traffic": committed_traffic(pose_name), "traffic_source": TRAFFIC_SRC,
                         "algorithmic_bytes_per_launch": pose_bytes, "avg_launch_ms": pose_ms, "launches_timed": n_timed, "timing": timing,
                         "fp64_view": {"achieved": pose_tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": pose_tf / FP64_PEAK_TFLOPS,
                                       "algorithmic_flops_per_launch": pose_flops, "mean_evaluations_per_pair": evals_l,
                                       "note": "(150 Np + 400 Nl) flop per evaluation x evaluations per frame pair (SURVEY.md 8d)"},
                         "note": "optimizePose for B frame pairs in one launch; algorithmic bytes = 32 B per matched point (two compact "
                                 "16-byte records; 52 B of doubles until round 3) + 16 B per unmatched prev point + 116 B per matched line "
                                 "(read once) + m12 and inlier masks (4 + 4 B per prev stereo feature) + 840 B result"}
        # point grid matcher (one workgroup per frame; STVO_GRID_FUSED=0: the scan formulation): SURVEY.md §8d match_grid bytes
        scan_ms = stage_ms["grid_scan"]
        n_kp_step = float(n_kp.mean(axis=1).sum())   # left + right key-points of one step, all streams
        scan_bytes = 32.0 * n_kp_step + 12.0 * n_kp_step / 2 + 4.0 * (3073.0 * B + n_kp_step / 2)
        fused_tail = os.environ.get("STVO_GRID_FUSED", "1") != "0" and os.environ.get("STVO_GRID_TAIL", "1") != "0"
        if fused_tail:  # the matcher launch also runs the tail of the association: key-point coordinates and octaves in, stereo set out
            scan_bytes += 8.0 * n_kp_step + 4.0 * n_kp_step / 2 + (16.0 + 32.0) * n2_l
        scan_gbs = scan_bytes / (scan_ms * 1e-3) / 1e9 if scan_ms > 0 else 0.0
        fused = os.environ.get("STVO_GRID_FUSED", "1") != "0"
        scan_name = "grid_points_fused_kernel" if fused else "grid_scan_kernel<false"
        roofline_grid = {"kernel": scan_name if fused else "grid_scan_kernel<false, 1> + <false, 2>", "bound": "hbm", "achieved": scan_gbs, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": scan_gbs / HBM_PEAK_GBS, "traffic": committed_traffic(scan_name), "traffic_source": TRAFFIC_SRC,
                         "algorithmic_bytes_per_launch": scan_bytes, "avg_launch_ms": scan_ms, "launches_timed": n_timed, "timing": timing,
                         "note": "matchGrid (points), all frames in one launch: 32 (N1 + N2) + 8 N1 + 4 (3073 + N2) + 4 N1 bytes per frame"
                                 + (", and as its last phase the tail of the stereo association (filters, back-projection, ordered compaction: "
                                    "8 (N1 + N2) + 4 N1 bytes in, 48 bytes per stereo point out: a 16-byte compact record + the descriptor row)" if fused_tail else "") +
                                 "; ~16 k candidate pairs per frame — bound by LDS gathers and the issue of the per-thread sort / chain code "
                                 "at 4 waves per SIMD (one workgroup per CU), not by HBM"}
        out = headline_record(args, world, backend, frames_total, dt, rep_dt, per_rank, streams, ok_frac)
        out["parity_sampled"] = parity
        out["config"].update({"mean_stereo_points": n2_l / B, "mean_matched_points": np_l / B, "mean_matched_lines": nl_l / B})
        out.update({
            "roofline": roofline, "roofline_pose": roofline_pose, "roofline_grid_scan": roofline_grid, "gpu_clocks": clocks,
            "stage_ms": dict(stage_ms_full, steps_timed=n_timed_full,
                             note="stereo_points_stage = cells + grid matcher (with the tail of the association as its last phase) of the "
                                  "key-points (contains grid_scan = the matcher launch); the key-line stage (line_stereo_fused_kernel, "
                                  "match_small_kernel) runs on a second stream.  These figures come from the COUNTING pass (an event pair around every "
                                  "stage, a read after every step; the roofline objects come from the light pass instead); the markers change what runs beside what (the key-line kernels then share the GPU "
                                  "with the point matcher: 0.14 ms alone, while in the timed region — fork behind the cells kernel, no markers — "
                                  "they run beside the forward scan and stretch IT), so the stages do not add up to ms_per_step: "
                                  "profiles/<tag>_step_timeline.txt has the dispatches of the timed region itself"),
        })
    pipe.close()
    ctx.close()
    if rank == 0 and world == 1 and extras:
        def extra(name, leg, *a, **kw):
            """The extra legs run after the timed region of the headline: one that fails is reported in its own key and must not
            cost the line (the headline, roofline and cpu_baseline objects above / below do not depend on them)."""
            try:
                out[name] = leg(*a, **kw)
            except Exception as e:  # noqa: BLE001 — whatever a leg raises (HIP error codes arrive as StvoError, allocation as RuntimeError)
                out[name] = {"error": f"{type(e).__name__}: {e}"}
        extra("headline_clustered", clustered_headline_leg, local_rank, streams_cl, cams, S, args.steps, args.warmup, args.repeats, args.max_keylines)
        hc = out["headline_clustered"]
        if "error" not in hc:   # beside `value`, inside the object the driver keeps whole
            out["config"]["value_clustered"] = hc["value"]
            out["config"]["value_clustered_over_value"] = hc["value"] / out["value"]
            out["config"]["value_clustered_note"] = ("the same pipeline and stream count on streams whose landmark descriptors are clustered "
                                                     "(60 % of the rows in groups of ~8 near-duplicates, spread 6 % of the bits): the i.i.d. "
                                                     "rows of `value` need no reverse distance evaluation in the mutual check, these do")
        if B > 1024:   # the batch of rounds 2 - 5, on the first 1024 of the same streams
            extra("headline_1024_streams", clustered_headline_leg, local_rank, streams[:1024], cams[:1024], S, args.steps, args.warmup, args.repeats,
                  args.max_keylines, model="i.i.d. descriptor bits (the streams of `value`)")
            h1 = out["headline_1024_streams"]
            if "error" not in h1:
                out["config"]["value_1024_streams"] = h1["value"]
        extra("latency", single_stream_latency, local_rank, args.points, args.lines)
        extra("configs1", configs1_leg, dev_name, rank)
        extra("configs3", configs3_leg, local_rank, c3_seqs)
        extra("reverse_check_correlated", correlated_leg, dev_name, rank)
        extra("orb_front_end", orb_leg, local_rank)
        extra("images_to_poses", images_leg, local_rank, B=512)
        extra("lsd_front_end", lsd_leg, local_rank)
        extra("images_to_poses_with_lines", images_leg, local_rank, B=3072, steps=3, lines=True)  # (the headline's stream count: 6144 images per step — 7.9 k pairs/s at 2048 streams, 9.2 k here, 9.0 k at 4096)
        # the reference application's own case (app/imagesStVO.cpp: ONE stereo pair per step, key-points + key-lines): latency, not throughput
        extra("one_stereo_pair_with_lines", images_leg, local_rank, B=1, steps=12, lines=True)
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args.points, args.lines)
        out["cpu_baseline_fanout"] = cpu_baseline_fanout(args.points, args.lines)
        out["cpu_baseline_threads"] = cpu_baseline_threads(args.points, args.lines)
        if "latency" in out and "error" not in out["latency"]:
            # the north star's latency target (>= 30x the CPU per-frame latency at 1 GPU) is worded on the StereoFrameHandler API:
            # both routes, against the 1-core oracle and against the oracle at the reference's own 4-thread fan-out, inside the
            # object the driver keeps whole
            lat, cb = out["latency"], out["cpu_baseline"]
            ss = {"seq_push": lat["seq_push_ms"]["median"], "handler": lat.get("handler_ms", {}).get("median"),
                  "what": "median ms per frame of ONE KITTI-00-shaped stream, host feature buffers in -> pose out (PCIe + synchronisation "
                          "included): stvo_seq_push through the C-ABI / the StereoFrameHandler mirror (imagesStVO_synth, the timed region "
                          "of app/imagesStVO.cpp:95-98)"}
            cb["single_stream_ms"] = ss
            cb["speedup_vs_1_core"] = {k: (cb["ms_per_frame"] / ss[k] if ss[k] else None) for k in ("seq_push", "handler")}
            fo = out["cpu_baseline_fanout"]["ms_per_frame"]
            cb["speedup_vs_reference_fanout"] = {k: (fo / ss[k] if ss[k] else None) for k in ("seq_push", "handler")}
            cb["ms_per_frame_reference_fanout_4_threads"] = fo
            out["latency"]["oracle_ms_1_core"] = out["cpu_baseline"]["ms_per_frame"]
            out["latency"]["speedup_vs_oracle_1_core"] = out["cpu_baseline"]["ms_per_frame"] / out["latency"]["seq_push_ms"]["median"]
            # the same against the reference's own thread structure (what its CPU latency would be on this box)
            out["latency"]["oracle_ms_reference_fanout_4_threads"] = out["cpu_baseline_fanout"]["ms_per_frame"]
            out["latency"]["speedup_vs_oracle_reference_fanout"] = out["cpu_baseline_fanout"]["ms_per_frame"] / out["latency"]["seq_push_ms"]["median"]
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and args.full:
        out["extras_file"] = write_extras(out)
        if args.print_extras:   # the full record on an EARLIER line of stderr; stdout carries the one short line only
            print("bench_extras: " + json.dumps(out), file=sys.stderr)
    if rank == 0:
        print(short_line(out), flush=True)


if __name__ == "__main__":
    main()
