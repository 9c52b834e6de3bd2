"""Feature tracks and key-frame sets per stream on the device pipeline (stvo_seq_set_tracks / read_tracks / keyframe_headers /
read_keyframe).  The yardstick for every step and every stream is tests/np_tracks.py fed with what the pipeline's existing interfaces
report for that step — fetch_matches (f2f rows), fetch_inliers, the counts, the trajectory ring's new_kf, the control words — and every
field of rows [0, n) is compared exactly.  Where a route exists only with the by-product fetch off (the key-line stage ahead) the run is
compared, byte for byte, with a run of the same input that was checked that way."""
import functools

import numpy as np
import pytest

import np_tracks
from np_tracks import PARK, RESTART, RUN
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params

pytestmark = pytest.mark.gpu
CAM = synth.KITTI_CAM
KF = dict(min_entropy_ratio=0.85, max_kf_t_dist=1.4, max_kf_r_dist=15.0)   # tests/test_gpu_trajectory.py: a reset within three frames
N_STEPS = 6
# key-points / key-lines per frame and stream.  Without distractors every left key-point has its partner in the right image on the same
# row, so the stereo point counts are these numbers in nearly every frame (the set is asserted): empty, one, around a wave, beyond a workgroup
SHAPES = [(0, 40), (1, 0), (63, 12), (64, 40), (65, 1), (300, 70)]


@functools.lru_cache(maxsize=None)
def shaped(seed, n_pts, n_lines, n_frames=N_STEPS):
    return tuple(synth.make_stereo_sequence(seed, n_frames=n_frames, n_pts=n_pts, n_lines=n_lines, cam=CAM, distract=0.0))


@functools.lru_cache(maxsize=None)
def plain(seed, n_frames=N_STEPS):
    return tuple(synth.make_stereo_sequence(seed, n_frames=n_frames, n_pts=300, n_lines=40, cam=CAM))


def open_dev(B, mp=None, op=None, max_kp=512, max_kl=128, fetch=True, tracks=2, keyframe_sets=False, trajectory=None, traj_log=2):
    from stvo_amd import capi
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=max(B, 1))
    try:
        dev = capi.Sequences(ctx, B, max_kp, max_kl, CAM, mp or match_params("kitti"), op or opt_params("kitti"))
    except Exception:
        ctx.close()
        raise
    if fetch:
        dev.enable_fetch(True)
    if trajectory is not None:
        dev.set_trajectory(trajectory, log_steps=traj_log)
    if tracks:
        dev.set_tracks(log_steps=tracks, keyframe_sets=keyframe_sets)
    return ctx, dev


def close(ctx, dev):
    dev.close()
    ctx.close()


def drive(dev, streams, controls=None, trajectory=False, log_steps=2, after_step=None):
    """Pushes streams[b][t] step by step and checks EVERY stream of EVERY step against np_tracks.  controls: {step: [B] words}.
    Returns per step a dict of what was read."""
    B, steps = len(streams), len(streams[0])
    chains = [np_tracks.Stream() for _ in range(B)]
    out, last_rows = [], None
    for t in range(steps):
        ctl = np.asarray((controls or {}).get(t, [RUN] * B), np.int32)
        if ctl.any():
            dev.control_next_step(ctl)
        res, counts = dev.push([streams[b][t] for b in range(B)])
        sched = dev.last_schedule()
        m12p = m12l = inlp = inll = None
        if t > 0:
            _, _, m12p, m12l = dev.fetch_matches()
            inlp, inll = dev.fetch_inliers()
        new_kf = np.zeros(B, np.int32)
        if trajectory and t > 0:
            new_kf = dev.read_trajectory(1)[0]["new_kf"].astype(np.int32)
        pts, lines, cnt = dev.read_tracks(1)
        assert pts.shape[:2] == (1, B) and np.array_equal(cnt[0], counts[:, :2]), (t, cnt[0], counts)
        want = []
        for b in range(B):
            first = t == 0
            c = RUN if first else int(ctl[b])     # a control staged for the pipeline's first step is consumed without effect
            w = chains[b].step(counts[b, :2], m12=(m12p[b], m12l[b]) if t else (None, None), inl=(inlp[b], inll[b]) if t else (None, None),
                               ctl=c, first=first, new_kf=int(new_kf[b]))
            n, nl = int(counts[b, 0]), int(counts[b, 1])
            assert pts[0, b, :n].tobytes() == w[0].tobytes(), (t, b, "points", pts[0, b, :n][:8], w[0][:8])
            assert lines[0, b, :nl].tobytes() == w[1].tobytes(), (t, b, "lines", lines[0, b, :nl][:8], w[1][:8])
            want.append(w)
        # the ring: asked for more than it holds, oldest first
        rows = dev.read_tracks(log_steps + 3)
        assert rows[0].shape[0] == min(t + 1, log_steps)
        assert rows[0][-1].tobytes() == pts[0].tobytes() and rows[1][-1].tobytes() == lines[0].tobytes()
        if last_rows is not None and log_steps >= 2:
            assert rows[0][-2].tobytes() == last_rows[0].tobytes() and rows[1][-2].tobytes() == last_rows[1].tobytes()
            assert np.array_equal(rows[2][-2], last_rows[2])
        last_rows = (pts[0].copy(), lines[0].copy(), cnt[0].copy())
        rec = dict(res=res.copy(), counts=counts.copy(), sched=sched, ctl=ctl, pts=pts[0].copy(), lines=lines[0].copy(), m12p=m12p, m12l=m12l,
                   new_kf=new_kf, want=want, serial=[c_.serial for c_ in chains])
        out.append(rec)
        if after_step is not None:
            after_step(t, rec)
    return out


def propagated(out):
    """How many records of a run came through an f2f match."""
    return sum(int((r["pts"]["age"] > 0).sum()) + int((r["lines"]["age"] > 0).sum()) for r in out)


# ---- 1. small batch: every count shape, points and lines, the ring wraps, both pose kernels

@pytest.mark.parametrize("pose", [None, "4"], ids=["latency-kernel", "batch-kernel"])
def test_small_batch_every_count_shape(switches, pose):
    from stvo_amd import capi
    if pose:
        switches({"STVO_POSE_KERNEL": pose})
    streams = [shaped(8100 + b, n_pts, n_lines) for b, (n_pts, n_lines) in enumerate(SHAPES)]
    ctx, dev = open_dev(len(streams))
    try:
        out = drive(dev, streams)
        want = capi.SCHED_POSE_BATCH if pose else capi.SCHED_POSE_LATENCY
        assert all(o["sched"]["pose_kernel"] == want for o in out[1:])
        point_counts = {int(c) for o in out for c in o["counts"][:, 0]}
        assert {0, 1, 63, 64, 65} <= point_counts and max(point_counts) > 256, point_counts
        line_counts = {int(c) for o in out for c in o["counts"][:, 1]}
        assert 0 in line_counts and max(line_counts) > 16, line_counts
        assert propagated(out) > 1000                       # the chains are not all "unmatched"
        ages = out[-1]["pts"][-1]["age"][:300]
        assert ages.max() == N_STEPS - 1                    # a feature followed through every frame
        assert {0, 1} <= set(np.unique(out[-1]["pts"][-1]["inlier"][:300]).tolist())
        with pytest.raises(capi.StvoError):
            dev.keyframe_headers()                          # tracks on, key-frame sets off
    finally:
        close(ctx, dev)


# ---- 2. the one-way route: several previous features name one current feature, the largest wins

def with_twins(fr, n_twins):
    """The frame with n_twins of its left key-points (and their right partners) repeated 16 rows lower — another grid row, so the stereo
    association of either is undisturbed — under the same descriptors: two features of this frame that the next frame's one answers."""
    rows_r = {float(v): j for j, v in enumerate(fr["kp_r"][:, 1])}
    pick = [i for i in range(len(fr["kp_l"])) if float(fr["kp_l"][i, 1]) in rows_r and fr["kp_l"][i, 1] < CAM["height"] - 40][:n_twins]
    assert len(pick) == n_twins
    js = [rows_r[float(fr["kp_l"][i, 1])] for i in pick]
    down = np.array([0, 16], np.float32)
    out = dict(fr)
    out["kp_l"] = np.concatenate([fr["kp_l"], fr["kp_l"][pick] + down])
    out["oct_l"] = np.concatenate([fr["oct_l"], fr["oct_l"][pick]])
    out["desc_l"] = np.concatenate([fr["desc_l"], fr["desc_l"][pick]])
    out["kp_r"] = np.concatenate([fr["kp_r"], fr["kp_r"][js] + down])
    out["desc_r"] = np.concatenate([fr["desc_r"], fr["desc_r"][js]])
    return out


def test_one_way_route_duplicates():
    base = [shaped(8200 + b, 120, 20) for b in range(3)]
    streams = [[with_twins(fr, 24) if k % 2 == 0 else fr for k, fr in enumerate(s)] for s in base]
    ctx, dev = open_dev(3, mp=match_params("kitti", best_lr_matches=0))
    try:
        out = drive(dev, streams)
        dups = 0
        for o in out[1:]:
            for b in range(3):
                hit = o["m12p"][b][o["m12p"][b] >= 0]
                dups += len(hit) - len(np.unique(hit))
        assert dups >= 10, dups                              # the fetched m12 names current features twice
        assert propagated(out) > 500
    finally:
        close(ctx, dev)


# ---- 3. key-frames: the reset, and the key-frame sets byte for byte

def test_keyframes_and_keyframe_sets():
    from stvo_amd import capi
    B = 5
    streams = [plain(7100 + b) for b in range(B)]
    ctx, dev = open_dev(B, keyframe_sets=True, trajectory=capi.traj_params("kitti", **KF))
    captured = [None] * B   # (step, debug_stereo) at the stream's last key-frame

    def after_step(t, rec):
        st = dev.trajectory_state()
        hdr = dev.keyframe_headers()
        for b in range(B):
            if t == 0 or rec["new_kf"][b] == 1:
                captured[b] = (t, dev.debug_stereo(b))
            step, cap = captured[b]
            assert (hdr[b]["n_pts"], hdr[b]["n_lines"], hdr[b]["frame"]) == (cap["n"], cap["nl"], step), (t, b, hdr[b])
            assert hdr[b]["serial"] == st[b]["n_keyframes"] + 1 == rec["serial"][b], (t, b, hdr[b], st[b]["n_keyframes"])
            got = dev.read_keyframe(b)
            assert (got["frame"], got["serial"]) == (step, hdr[b]["serial"])
            for k, v in cap.items():
                assert np.asarray(got[k]).tobytes() == np.asarray(v).tobytes(), (t, b, k)

    try:
        out = drive(dev, streams, trajectory=True, after_step=after_step)
        kf = np.array([o["new_kf"] for o in out[1:]])
        assert any(0 < row.sum() < B for row in kf), kf       # a step with streams both with and without a key-frame
        # behind a key-frame the features that were followed observe THAT frame: kf 1, age 1, idx = their position in it
        seen = 0
        for t in range(1, N_STEPS - 1):
            for b in range(B):
                if kf[t - 1][b] == 1:
                    nxt, n = out[t + 1]["pts"][b], out[t + 1]["counts"][b, 0]
                    hit = nxt[:n][nxt[:n]["age"] > 0]
                    assert len(hit) and (hit["kf"] == 1).all() and (hit["age"] == 1).all()
                    m12 = out[t + 1]["m12p"][b]
                    assert all(m12[r["idx"]] >= 0 for r in hit)
                    seen += 1
        assert seen >= 1
    finally:
        close(ctx, dev)


# ---- 4. controls: RESTART and PARK mixed with RUN in one step, PARK followed by RUN; the neighbours do not notice

@pytest.mark.parametrize("B", [4, 20], ids=["B4-pinned-masks", "B20-device-masks"])
def test_controls(B):
    from stvo_amd import capi
    streams = [plain(8300 + b % 4) for b in range(B)]
    controls = {2: [RUN, RESTART, PARK, RUN] * (B // 4), 4: [RUN, PARK, RUN, RUN] * (B // 4)}   # step 3: PARK then RUN, RESTART then RUN
    runs = []
    for ctl in (controls, None):
        ctx, dev = open_dev(B, keyframe_sets=True, trajectory=capi.traj_params("kitti", **KF))
        try:
            runs.append(drive(dev, streams, controls=ctl, trajectory=True))
            if ctl:
                hdr = dev.keyframe_headers()
                assert (hdr["serial"] == [o for o in runs[0][-1]["serial"]]).all()
        finally:
            close(ctx, dev)
    with_ctl, without = runs
    o = with_ctl[2]
    for b in range(B):
        n = o["counts"][b, 0]
        if b % 4 == 1:
            assert (o["pts"][b][:n]["kf"] == 1).all() and (o["pts"][b][:n]["age"] == 0).all() and (o["pts"][b][:n]["inlier"] == -1).all()
        if b % 4 == 2:
            assert (o["pts"][b][:n]["kf"] == 0).all() and (o["pts"][b][:n]["age"] == 0).all()
    # PARK then RUN tracks against the parked frame: features followed once, none of them an observation of a key-frame
    o = with_ctl[3]
    for b in range(2, B, 4):
        rows = o["pts"][b][:o["counts"][b, 0]]
        assert (rows["age"] > 0).sum() > 50 and (rows["age"] <= 1).all() and (rows["kf"] == 0).all()
    for t in range(N_STEPS):
        for b in list(range(0, B, 4)) + list(range(3, B, 4)):   # never under a control
            n, nl = with_ctl[t]["counts"][b, :2]
            assert with_ctl[t]["pts"][b][:n].tobytes() == without[t]["pts"][b][:n].tobytes(), (t, b)
            assert with_ctl[t]["lines"][b][:nl].tobytes() == without[t]["lines"][b][:nl].tobytes(), (t, b)


# ---- 5. the key-line stage ahead recycles the set and the match copy this kernel reads

def test_line_stage_ahead():
    """The smallest batch the planner lets run ahead (more than two streams per CU, by-product fetch off), five steps enqueued back to
    back — both copies of the key-line match indices — against the same input run with the fetch on (no stage ahead), every stream of
    which is checked against np_tracks."""
    import torch
    B = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    steps = 5
    seqs = [plain(8400 + k, steps) for k in range(8)]
    streams = [seqs[b % 8] for b in range(B)]
    ctx, dev = open_dev(B, tracks=steps)
    try:
        ref = drive(dev, streams, log_steps=steps)
        assert all(o["sched"]["lines_ahead"] == 0 for o in ref)
        assert propagated(ref) > 100 * B
    finally:
        close(ctx, dev)
    ctx, dev = open_dev(B, fetch=False, tracks=steps)
    try:
        dev.set_slots(steps)
        for k in range(steps):
            dev.upload(k, [s[k] for s in streams])
        sched = []
        for k in range(steps):
            dev.step_dev(k)
            sched.append(dev.last_schedule())
        assert [s["lines_ahead"] for s in sched] == [0, 0, 1, 1, 1], sched
        pts, lines, cnt = dev.read_tracks(steps)
        assert pts.shape[0] == steps
        for t in range(steps):
            assert np.array_equal(cnt[t], ref[t]["counts"][:, :2]), t
            for b in range(B):
                n, nl = cnt[t][b]
                assert pts[t, b, :n].tobytes() == ref[t]["pts"][b][:n].tobytes(), (t, b)
                assert lines[t, b, :nl].tobytes() == ref[t]["lines"][b][:nl].tobytes(), (t, b)
    finally:
        close(ctx, dev)


# ---- 6. no side effect; 7. feature off

def test_no_side_effect_and_feature_off():
    from stvo_amd import capi
    B = 3
    streams = [plain(8500 + b) for b in range(B)]
    runs = []
    for tracks in (2, 0):
        ctx, dev = open_dev(B, fetch=False, tracks=tracks, keyframe_sets=bool(tracks), trajectory=capi.traj_params("kitti", **KF), traj_log=N_STEPS)
        try:
            steps = [dev.push([s[t] for s in streams]) for t in range(N_STEPS)]
            runs.append((steps, dev.read_trajectory(N_STEPS), dev.trajectory_state()))
            if not tracks:
                K, M = dev.strides()
                for call in (lambda: dev.read_tracks(1), dev.keyframe_headers, lambda: dev.read_keyframe(0), dev.tracks_dev):
                    with pytest.raises(capi.StvoError):
                        call()
                n = capi.C.c_int32()
                assert ctx.lib.stvo_seq_read_tracks(dev.h, 1, None, None, None, capi.C.byref(n)) == -1
                assert ctx.lib.stvo_seq_keyframe_headers(dev.h, np.zeros(B * 4, np.int32).ctypes.data_as(capi.C.c_void_p)) == -1
            else:
                p, l, c = dev.tracks_dev()
                assert p and l and c
        finally:
            close(ctx, dev)
    (on, traj_on, st_on), (off, traj_off, st_off) = runs
    for (ra, ca), (rb, cb) in zip(on, off):
        assert ra.tobytes() == rb.tobytes() and np.array_equal(ca, cb)
    assert traj_on.tobytes() == traj_off.tobytes() and st_on.tobytes() == st_off.tobytes()
    assert traj_on["new_kf"].sum() >= 1


# ---- 8. the app: the --tracks lines of the two routes

def test_app_routes_print_the_same_tracks(tmp_path):
    import os
    import subprocess
    app = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stvo-pl_amd", "bin", "imagesStVO_synth")
    seq = str(tmp_path / "seq.bin")
    synth.write_sequence(seq, list(plain(7100)), CAM)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"max_kf_t_dist : {KF['max_kf_t_dist']}\n")
    lines = {}
    for name, extra in (("device", ("--device-pipeline",)), ("handler", ())):
        p = subprocess.run([app, seq, str(tmp_path / f"{name}.bin"), "--preset", "kitti", "-c", str(cfg), "--keyframes", "--tracks", *extra],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr + p.stdout
        lines[name] = [ln for ln in p.stdout.splitlines() if ln.startswith("Tracks:")]
        res = synth.read_results(str(tmp_path / f"{name}.bin"))
        assert 1 <= sum(int(r["pad"]) for r in res) < len(res)          # key-frames, and frames between them
    assert len(lines["device"]) == N_STEPS - 1 and lines["device"] == lines["handler"], lines
    fields = [ln.split() for ln in lines["device"]]
    assert all(int(f[4]) > 50 and int(f[6]) > 20 for f in fields), lines["device"]   # features of a key-frame are followed, most are inliers
    no_flag = subprocess.run([app, seq, str(tmp_path / "plain.bin"), "--preset", "kitti", "--device-pipeline"], capture_output=True, text=True, timeout=120)
    assert no_flag.returncode == 0 and "Tracks:" not in no_flag.stdout
