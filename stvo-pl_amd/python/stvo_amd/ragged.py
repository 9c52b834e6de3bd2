"""Sequences of different lengths on the B lock-step streams of the device-resident pipeline: a stream whose sequence has ended takes
the next one with a RESTART (StereoFrameHandler::initialize for that stream alone) and is PARKED when nothing is left, while the other
streams go on — no junk frames through a finished stream's state, no rebuild of the pipeline.

plan() is a pure host function (no GPU, no library); run() drives a capi.Sequences object through it.  Plumbing for tests and tools."""
from collections import namedtuple

import numpy as np

STREAM_RUN, STREAM_RESTART, STREAM_PARK = 0, 1, 2   # capi.STREAM_* (include/stvo_hip.h: STVO_STREAM_*)

# control: int32 [B] for Sequences.control_next_step; consume: B entries, (sequence, frame) or None for a parked stream
Step = namedtuple("Step", ["control", "consume"])


def plan(lengths, B):
    """Packs N sequences of lengths[i] >= 1 frames onto B streams: longest first, each onto the stream that frees up earliest (the
    lowest-numbered of several; sequences of equal length in their given order).  Returns one Step per pipeline step: the control
    words (RESTART exactly on frame 0 of a sequence that does not start in step 0, PARK on a stream with nothing left, RUN otherwise)
    and, per stream, the (sequence, frame) it consumes.  The number of steps is the makespan of that packing; no sequence: no step."""
    lengths = [int(n) for n in lengths]
    if B < 1:
        raise ValueError("ragged.plan: at least one stream")
    if any(n < 1 for n in lengths):
        raise ValueError("ragged.plan: every sequence holds at least one frame")
    free = [0] * B                       # the step from which stream b is free
    starts = [[] for _ in range(B)]      # per stream: (first step, sequence), ascending
    for i in sorted(range(len(lengths)), key=lambda i: (-lengths[i], i)):
        b = min(range(B), key=lambda b: (free[b], b))
        starts[b].append((free[b], i))
        free[b] += lengths[i]
    steps = []
    for t in range(max(free) if lengths else 0):
        control = np.full(B, STREAM_PARK, np.int32)
        consume = [None] * B
        for b in range(B):
            for t0, i in starts[b]:
                if t0 <= t < t0 + lengths[i]:
                    consume[b] = (i, t - t0)
                    control[b] = STREAM_RESTART if (t == t0 and t > 0) else STREAM_RUN
        steps.append(Step(control, consume))
    return steps


def empty_frame():
    """What a parked stream is fed: a frame without features."""
    z2, z4, zd, zi = np.zeros((0, 2), np.float32), np.zeros((0, 4), np.float32), np.zeros((0, 32), np.uint8), np.zeros(0, np.int32)
    return dict(kp_l=z2, oct_l=zi, desc_l=zd, kp_r=z2, desc_r=zd, kl_l=z4, oct_ll=zi, ldesc_l=zd, kl_r=z4, ldesc_r=zd)


def initial_cameras(lengths, B, cams):
    """The B camera dicts to create the pipeline of run(dev, sequences, cams=cams) with: cams[i] of the sequence the plan starts on each
    stream in step 0, and — a stream that starts parked reads no camera before its first RESTART brings one — cams[0] for the others."""
    steps = plan(lengths, B)
    if not steps:
        raise ValueError("ragged.initial_cameras: no sequence")
    return [cams[c[0]] if c is not None else cams[0] for c in steps[0].consume]


def run(dev, sequences, tracks=0, keyframe_sets=False, cams=None):
    """Drives dev (a fresh capi.Sequences of B streams) through plan([len(s) for s in sequences], dev.B), one push per step.
    cams: None (every sequence has the camera its stream was created with), or one camera dict per sequence — dev is then created with
    initial_cameras(lengths, B, cams), and every RESTART of the plan is followed by Sequences.restart_cameras with the camera of the
    sequence that begins (a stream's sequences need not share a calibration or an image size).
    Returns (results, counts, records): per sequence a POSE_RESULT_DTYPE array [frames] (entry 0, the sequence's first frame, all-zero),
    an int32 array [frames, 4], and — with the trajectory on (Sequences.set_trajectory), else records is None — a TRAJ_RECORD_DTYPE
    array [frames - 1] of the tracked frames (its `frame` counts from 1 in every sequence).
    tracks >= 1 (the ring's rows; keyframe_sets as for Sequences.set_tracks): the feature tracks are turned on before the first step and a
    fourth value is returned — per sequence and frame a dict of pts / lines (TRACK_DTYPE rows [0, count)) and, with keyframe_sets,
    kf_header (the stream's KF_HEADER_DTYPE record behind that step)."""
    if tracks:
        dev.set_tracks(log_steps=tracks, keyframe_sets=keyframe_sets)
    feats = [[] for _ in sequences] if tracks else None
    steps = plan([len(s) for s in sequences], dev.B)
    traj = getattr(dev, "_traj_log_steps", 0) > 0
    results = [[] for _ in sequences]
    counts = [[] for _ in sequences]
    records = [[] for _ in sequences] if traj else None
    idle = empty_frame()
    for st in steps:
        if st.control.any():
            dev.control_next_step(st.control)
            if cams is not None and (st.control == STREAM_RESTART).any():
                dev.restart_cameras([cams[c[0]] if st.control[b] == STREAM_RESTART else None for b, c in enumerate(st.consume)])
        res, cnt = dev.push([sequences[c[0]][c[1]] if c is not None else idle for c in st.consume])
        rec = dev.read_trajectory(1) if traj else None
        if tracks:
            tp, tl, tc = dev.read_tracks(1)
            hdr = dev.keyframe_headers() if keyframe_sets else None
        for b, c in enumerate(st.consume):
            if c is None:
                continue
            results[c[0]].append(res[b].copy())
            counts[c[0]].append(cnt[b].copy())
            if traj and c[1] > 0:
                records[c[0]].append(rec[-1][b].copy())
            if tracks:
                f = dict(pts=tp[-1][b][:tc[-1][b][0]].copy(), lines=tl[-1][b][:tc[-1][b][1]].copy())
                if keyframe_sets:
                    f["kf_header"] = hdr[b].copy()
                feats[c[0]].append(f)
    results = [np.array(r, dtype=r[0].dtype) for r in results]
    counts = [np.array(c, np.int32).reshape(-1, 4) for c in counts]
    if traj:
        from .ctypes_types import TRAJ_RECORD_DTYPE
        records = [np.array(r, dtype=TRAJ_RECORD_DTYPE) for r in records]
    if tracks:
        return results, counts, records, feats
    return results, counts, records
