"""A RESTART stream takes the camera of the sequence it begins (stvo_seq_restart_cameras, Sequences.restart_cameras, ragged.run(cams=)).
Five sequences of 4, 3, 2, 2 and 1 frames with the three KITTI calibrations (kitti00-02 / 03 / 04-10: focal length, principal point,
baseline AND image size differ) and one camera with fx != fy at another size, on B = 3 streams: ragged.plan puts sequence 3 behind
sequence 2 on stream 2 and sequence 4 behind sequence 1 on stream 1, neither pair sharing a camera.

Every tracked frame is judged against its own oracle chain under its own camera exactly as tests/test_gpu_stream_control.py judges
(check_tracked / compare_record, imported), every first frame by its stereo counts under its own camera (the grid scale 64 / cols,
48 / rows decides them); every restarted sequence is byte-equal to the same sequence on a fresh pipeline created with its camera; the
stream that never restarts is byte-equal to a run without any camera call; and a snapshot taken after a swap carries the new camera."""
import ctypes as C

import numpy as np
import pytest

import pipeline_ref
import test_gpu_stream_control as sc
from stvo_amd import ragged, synth

gpu = pytest.mark.gpu   # (the plan test needs none)
B = 3
LENGTHS = (4, 3, 2, 2, 1)
ODD_CAM = dict(fx=612.4, fy=598.7, cx=498.3, cy=241.9, b=0.4125, width=1000, height=480)
CAMS = [synth.config5_cam(0), synth.config5_cam(3), synth.config5_cam(4), ODD_CAM, synth.config5_cam(0)]

_seqs, _chains = {}, {}


def sequences():
    if not _seqs:
        for i, n in enumerate(LENGTHS):
            _seqs[i] = synth.make_stereo_sequence(synth.frame_seed(40 + i, 0), n_frames=n, n_pts=300, n_lines=40, cam=CAMS[i])
    return [_seqs[i] for i in range(len(LENGTHS))]


def chain(oracle, cfg, i):
    """the oracle chain of sequence i under ITS camera, and the stereo counts of its first frame; computed once per configuration"""
    if (i, cfg.key) not in _chains:
        fr = sequences()[i]
        ref = pipeline_ref.run_sequence(oracle, list(fr), CAMS[i], cfg.mp, cfg.op, motion_model=cfg.motion_model,
                                        keyframes=sc.KF if cfg.keyframes else None) if len(fr) > 1 else []
        first = pipeline_ref.stereo_frame(oracle, fr[0], CAMS[i], cfg.mp, True, bool(cfg.has_lines))
        _chains[i, cfg.key] = (ref, (len(first["P"]), len(first["sP"])))
    return _chains[i, cfg.key]


def open_dev(cfg, cams, traj):
    from stvo_amd import capi
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        dev = capi.Sequences(ctx, B, 512, 64, cams, cfg.mp, cfg.op)
    except Exception:
        ctx.close()
        raise
    if cfg.motion_model:
        dev.set_motion_model(True)
    if traj:
        dev.set_trajectory(capi.traj_params("kitti", **sc.KF), log_steps=1)
    return ctx, dev


def close(ctx, dev):
    dev.close()
    ctx.close()


def test_plan_puts_other_cameras_behind_each_other():
    steps = ragged.plan(LENGTHS, B)
    assert len(steps) == 4
    assert [c for c in steps[0].consume] == [(0, 0), (1, 0), (2, 0)]
    assert steps[2].control.tolist() == [sc.RUN, sc.RUN, sc.RESTART] and steps[2].consume[2] == (3, 0)
    assert steps[3].control.tolist() == [sc.RUN, sc.RESTART, sc.RUN] and steps[3].consume[1] == (4, 0)
    assert ragged.initial_cameras(LENGTHS, B, CAMS) == CAMS[:3]
    assert CAMS[3] != CAMS[2] and CAMS[4] != CAMS[1] and ODD_CAM["fx"] != ODD_CAM["fy"]
    # a stream that starts parked is created with any camera: its first RESTART brings its own
    assert len(ragged.initial_cameras((2,), 3, [ODD_CAM])) == 3


@gpu
@pytest.mark.parametrize("pose,traj", [(None, True), ("4", False)], ids=["latency-kernel-trajectory", "batch-kernel"])
def test_ragged_run_with_a_camera_per_sequence(oracle, switches, pose, traj):
    from stvo_amd import capi
    if pose:
        switches({"STVO_POSE_KERNEL": pose})
    cfg = sc.Cfg(1, True, keyframes=traj)
    seqs = sequences()
    ctx, dev = open_dev(cfg, ragged.initial_cameras(LENGTHS, B, CAMS), traj)
    try:
        results, counts, records = ragged.run(dev, seqs, cams=CAMS)
        want = capi.SCHED_POSE_BATCH if pose else capi.SCHED_POSE_LATENCY
        assert dev.last_schedule()["pose_kernel"] == want
    finally:
        close(ctx, dev)
    # 1. every sequence against its own chain under its own camera
    for i, n in enumerate(LENGTHS):
        ref, first = chain(oracle, cfg, i)
        assert results[i].shape == (n,) and counts[i].shape == (n, 4)
        assert results[i][0].tobytes() == sc.ZERO_RESULT and not counts[i][0, 2:].any()
        print("sequence", i, "first frame counts", tuple(counts[i][0, :2]), "oracle", first)
        assert tuple(counts[i][0, :2]) == first, (i, counts[i][0], first)
        for k in range(1, n):
            sc.check_tracked(results[i][k], counts[i][k], ref[k - 1], (i, k))
            if traj:
                sc.compare_record(records[i][k - 1], ref[k - 1])
                assert records[i][k - 1]["frame"] == k
    # the cameras matter: the first frame of sequence 3 counts otherwise under the camera its stream had before (another grid scale)
    stale = pipeline_ref.stereo_frame(oracle, seqs[3][0], CAMS[2], cfg.mp, True, True)
    assert (len(stale["P"]), len(stale["sP"])) != chain(oracle, cfg, 3)[1]
    # 2. every restarted sequence is, byte for byte, the same sequence on a fresh pipeline created with its camera (on its stream)
    for i, b in ((3, 2), (4, 1)):
        ctx, dev = open_dev(cfg, [CAMS[i]] * B, traj)
        try:
            for k, fr in enumerate(seqs[i]):
                res, cnt = dev.push([fr] * B)
                assert res[b].tobytes() == results[i][k].tobytes() and np.array_equal(cnt[b], counts[i][k]), (i, k)
                if traj and k > 0:
                    assert dev.read_trajectory(1)[-1][b].tobytes() == records[i][k - 1].tobytes(), (i, k)
        finally:
            close(ctx, dev)
    # 3. the stream that never restarts (sequence 0), and sequences 1 and 2, which end before their streams restart, are, byte for byte,
    #    what they are in a run of the same plan without any camera call
    ctx, dev = open_dev(cfg, ragged.initial_cameras(LENGTHS, B, CAMS), traj)
    try:
        plain = ragged.run(dev, seqs)
    finally:
        close(ctx, dev)
    for i in (0, 1, 2):
        assert plain[0][i].tobytes() == results[i].tobytes() and np.array_equal(plain[1][i], counts[i]), i
        if traj:
            assert plain[2][i].tobytes() == records[i].tobytes(), i
    # ... in which the restarted sequences kept their stream's camera, as before this call existed
    assert tuple(plain[1][3][0, :2]) != tuple(counts[3][0, :2]) or plain[0][3][1].tobytes() != results[3][1].tobytes()


@gpu
def test_snapshot_carries_the_new_camera(oracle):
    from stvo_amd import capi
    cfg = sc.Cfg(1, False)
    seqs = sequences()
    ctx, dev = open_dev(cfg, CAMS[:3], False)
    try:
        dev.push([seqs[0][0], seqs[1][0], seqs[2][0]])
        dev.control_next_step([sc.RUN, sc.RUN, sc.RESTART])
        dev.restart_cameras([None, None, CAMS[3]])
        dev.push([seqs[0][1], seqs[1][1], seqs[3][0]])
        blob = dev.export_streams([2])
        hdr = capi.snapshot_views(blob[0])["header"]
        assert (int(hdr["cols"]), int(hdr["rows"])) == (ODD_CAM["width"], ODD_CAM["height"])
        assert [float(hdr["cam"][k]) for k in ("fx", "fy", "cx", "cy", "b")] == [ODD_CAM[k] for k in ("fx", "fy", "cx", "cy", "b")]
        kept = capi.snapshot_views(dev.export_streams([1])[0])["header"]     # a stream that did not restart keeps its camera
        assert (int(kept["cols"]), int(kept["rows"])) == (CAMS[1]["width"], CAMS[1]["height"])
        # the pipeline itself now takes this blob back, and no longer one of the camera the stream had
        dev.import_streams([2], blob)
    finally:
        close(ctx, dev)
    ref = chain(oracle, cfg, 3)[0]
    for cams, ok in (([CAMS[0], CAMS[1], CAMS[3]], True), (CAMS[:3], False)):
        ctx, dev = open_dev(cfg, cams, False)
        try:
            dev.push([seqs[0][0], seqs[1][0], seqs[2][0]])
            if ok:
                dev.import_streams([2], blob)
                res, cnt = dev.push([seqs[0][1], seqs[1][1], seqs[3][1]])
                sc.check_tracked(res[2], cnt[2], ref[0], "continued under the new camera")
            else:
                with pytest.raises(capi.StvoError):
                    dev.import_streams([2], blob)
        finally:
            close(ctx, dev)


@gpu
def test_argument_checks(oracle):
    from stvo_amd import capi
    from stvo_amd.ctypes_types import Cam
    cfg = sc.Cfg(1, False)
    seqs = sequences()
    INVALID = -1
    ctx, dev = open_dev(cfg, CAMS[:3], False)
    try:
        L = ctx.lib
        cams = (Cam * B)(*[Cam.from_dict(CAMS[3])] * B)
        cols, rows = np.full(B, 1000, np.int32), np.full(B, 480, np.int32)
        args = (C.cast(cams, C.c_void_p), cols.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p))
        dev.push([seqs[0][0], seqs[1][0], seqs[2][0]])
        assert L.stvo_seq_restart_cameras(dev.h, *args) == INVALID                       # nothing staged
        dev.control_next_step([sc.RUN, sc.PARK, sc.RUN])
        assert L.stvo_seq_restart_cameras(dev.h, *args) == INVALID                       # a control, but no RESTART in it
        dev.control_next_step([sc.RUN, sc.RUN, sc.RESTART])
        assert L.stvo_seq_restart_cameras(None, *args) == INVALID
        for k in range(3):
            assert L.stvo_seq_restart_cameras(dev.h, *[None if j == k else a for j, a in enumerate(args)]) == INVALID
        for bad in (0, -5):
            c2 = cols.copy(); c2[2] = bad
            assert L.stvo_seq_restart_cameras(dev.h, args[0], c2.ctypes.data_as(C.c_void_p), args[2]) == INVALID
            r2 = rows.copy(); r2[2] = bad
            assert L.stvo_seq_restart_cameras(dev.h, args[0], args[1], r2.ctypes.data_as(C.c_void_p)) == INVALID
        with pytest.raises(ValueError):
            dev.restart_cameras([CAMS[3]])                                                # one entry per stream
        # every refusal left the stream's camera alone: the restart runs under the camera of creation (sequence 2's), as without the call
        res, cnt = dev.push([seqs[0][1], seqs[1][1], seqs[2][0]])
        assert tuple(cnt[2, :2]) == chain(oracle, cfg, 2)[1]
        # sizes of streams that do not restart are not read
        dev.control_next_step([sc.RUN, sc.RUN, sc.RESTART])
        c2 = cols.copy(); c2[:2] = 0
        assert L.stvo_seq_restart_cameras(dev.h, args[0], c2.ctypes.data_as(C.c_void_p), args[2]) == 0
        res, cnt = dev.push([seqs[0][2], seqs[1][2], seqs[3][0]])
        assert tuple(cnt[2, :2]) == chain(oracle, cfg, 3)[1]
        sc.check_tracked(res[0], cnt[0], chain(oracle, cfg, 0)[0][1], "neighbour")
    finally:
        close(ctx, dev)
