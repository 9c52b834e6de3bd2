"""Restart and park single streams of the device pipeline between steps (stvo_seq_control_next_step / stvo_seq_restart_fast_dev,
Sequences.control_next_step, ImagePipeline(control=), stvo_amd.ragged): a RESTART stream must compute exactly what a fresh sequence
computes (StereoFrameHandler::initialize, the reference's src/stereoFrameHandler.cpp:35-52), a PARKed stream must report and advance
nothing, and the streams without a control must not notice.  Reference: the oracle chain (pipeline_ref.run_sequence) of every sequence
from ITS frame 0, with the tolerances tests/test_gpu_seq.py::run_and_compare and tests/test_gpu_trajectory.py::compare_record apply to
the same quantities."""
import ctypes as C

import numpy as np
import pytest

import np_fast_adapt
import np_model
import pipeline_ref
from stvo_amd import ragged, synth
from stvo_amd.ctypes_types import POSE_RESULT_DTYPE, TRAJ_RECORD_DTYPE, TRAJ_STATE_DTYPE, match_params, opt_params

pytestmark = pytest.mark.gpu
RUN, RESTART, PARK = 0, 1, 2
CAM = synth.KITTI_CAM
KF = dict(min_entropy_ratio=0.85, max_kf_t_dist=1.4, max_kf_r_dist=15.0)   # the thresholds of tests/test_gpu_trajectory.py
ZERO_RESULT = np.zeros(1, POSE_RESULT_DTYPE).tobytes()

_seqs, _chains, _stereo = {}, {}, {}


def sequence(seed, n_frames=6):
    if (seed, n_frames) not in _seqs:
        _seqs[seed, n_frames] = synth.make_stereo_sequence(seed, n_frames=n_frames, n_pts=300, n_lines=40, cam=CAM)
    return _seqs[seed, n_frames]


class Cfg:
    """What the oracle chains of a test are computed under."""

    def __init__(self, has_lines=1, motion_model=False, keyframes=False):
        self.has_lines, self.motion_model, self.keyframes = has_lines, motion_model, keyframes
        self.mp, self.op = match_params("kitti"), opt_params("kitti", has_lines=has_lines)
        self.key = (has_lines, motion_model, keyframes)


def chain(oracle, cfg, frames, tag):
    """run_sequence on `frames` (tag names them), computed once per configuration and shared."""
    key = (tag, cfg.key)
    if key not in _chains:
        _chains[key] = pipeline_ref.run_sequence(oracle, list(frames), CAM, cfg.mp, cfg.op, motion_model=cfg.motion_model,
                                                 keyframes=KF if cfg.keyframes else None)
    return _chains[key]


def stereo_counts(oracle, cfg, fr, tag):
    key = (tag, cfg.has_lines)
    if key not in _stereo:
        ref = pipeline_ref.stereo_frame(oracle, fr, CAM, cfg.mp, True, bool(cfg.has_lines))
        _stereo[key] = (len(ref["P"]), len(ref["sP"]))
    return _stereo[key]


# ---- a stream's script: one entry per step = (control word, frame, oracle output of that frame or None, (tag, frame number in its sequence))

def start(oracle, cfg, seed, n, first=RUN):
    """Frames 0 .. n - 1 of sequence `seed` from its frame 0: `first` = RUN in a pipeline's first step, RESTART anywhere."""
    fr = sequence(seed)[:n]
    ref = chain(oracle, cfg, fr, (seed, 0, n))
    return [(first if k == 0 else RUN, fr[k], ref[k - 1] if k else None, ((seed, k), k)) for k in range(n)]


def park(seed, ks):
    return [(PARK, sequence(seed)[k], None, ((seed, k), 0)) for k in ks]


def resume(oracle, cfg, seed, k0, n):
    """RUN on frames k0 + 1 .. k0 + n of `seed` behind a step that was fed frame k0 (parked): the chain of the sequence that starts at k0."""
    fr = sequence(seed)[k0:k0 + n + 1]
    ref = chain(oracle, cfg, fr, (seed, k0, n + 1))
    return [(RUN, fr[k], ref[k - 1], ((seed, k0 + k), k)) for k in range(1, n + 1)]


def check_tracked(r, c, o, where):
    """The per-frame assertions of tests/test_gpu_seq.py::run_and_compare."""
    assert c[0] == o["n_stereo_pt"] and c[1] == o["n_stereo_ls"], (where, c, o["n_stereo_pt"], o["n_stereo_ls"])
    assert r["n_matched_pt"] == o["n_matched_pt"] and r["n_matched_ls"] == o["n_matched_ls"], where
    assert c[2] == o["n_matched_pt"] and c[3] == o["n_matched_ls"], where
    assert r["status"] == o["status"] and r["path"] == o["path"] and tuple(r["iters"]) == o["iters"], where
    assert r["n_inliers_pt"] == o["n_inliers_pt"] and r["n_inliers_ls"] == o["n_inliers_ls"], where
    T = r["T"].reshape(4, 4)
    assert np_model.rot_angle(T[:3, :3], o["T"][:3, :3]) < 1e-4 and np.linalg.norm(T[:3, 3] - o["T"][:3, 3]) < 1e-3, where
    assert np.allclose(T, o["T"], atol=1e-8) and np.isclose(r["err"], o["err"], rtol=1e-8), where
    assert np.allclose(r["cov"].reshape(6, 6), o["cov"], rtol=1e-6, atol=1e-12), where


def compare_record(rec, o, keyframes=True):
    """tests/test_gpu_trajectory.py::compare_record"""
    assert np.allclose(rec["Tfw"].reshape(4, 4), o["Tfw"], atol=1e-7)
    assert np.allclose(rec["Tfw_cov"].reshape(6, 6), o["Tfw_cov"], rtol=1e-6, atol=1e-10)
    assert int(rec["new_kf"]) == (o["new_kf"] if keyframes else 0)


def make_dev(B, cfg, max_rows=2048):
    from stvo_amd import capi
    ctx = capi.Context(device_id=0, max_rows=max_rows, max_batch=max(B, 1))
    try:
        dev = capi.Sequences(ctx, B, 512, 64, CAM, cfg.mp, cfg.op)
    except Exception:
        ctx.close()
        raise
    if cfg.motion_model:
        dev.set_motion_model(True)
    return ctx, dev


def drive(oracle, cfg, dev, scripts, control=True, check=True, after_step=None):
    """Pushes the scripts of the B streams step by step (a control is staged only for a step that has a word other than RUN) and checks
    every stream-step: a tracked frame against its oracle output, any other as "no pose in this step".  Returns per step
    (results, counts, last_schedule, control words)."""
    B, steps = len(scripts), len(scripts[0])
    assert all(len(s) == steps for s in scripts)
    out = []
    for t in range(steps):
        ctl = np.array([scripts[b][t][0] for b in range(B)], np.int32)
        if control and ctl.any():
            dev.control_next_step(ctl)
        res, counts = dev.push([scripts[b][t][1] for b in range(B)])
        sched = dev.last_schedule()
        if check:
            for b in range(B):
                _, fr, o, (tag, _) = scripts[b][t]
                if o is None:
                    assert res[b].tobytes() == ZERO_RESULT, (t, b)
                    assert counts[b, 2] == 0 and counts[b, 3] == 0, (t, b, counts[b])
                    assert tuple(counts[b, :2]) == stereo_counts(oracle, cfg, fr, tag), (t, b, counts[b])   # the new frame's association ran
                else:
                    check_tracked(res[b], counts[b], o, (t, b))
        out.append((res.copy(), counts.copy(), sched, ctl))
        if after_step is not None:
            after_step(t, res, counts)
    return out


# ---- 1. restart equals a fresh sequence; 2. neighbours are untouched

def restart_scripts(oracle, cfg, B, restarted):
    """Every stream runs its own six frames; the streams of `restarted` get three frames and then RESTART onto another sequence."""
    scripts = []
    for b in range(B):
        a = 3100 + b % 8
        if b in restarted:
            scripts.append(start(oracle, cfg, a, 3) + start(oracle, cfg, 3200 + b % 5, 3, first=RESTART))
        else:
            scripts.append(start(oracle, cfg, a, 6))
    return scripts


@pytest.mark.parametrize("B,pose,has_lines,motion_model", [(3, None, 1, False), (3, None, 0, False), (3, None, 1, True), (3, None, 0, True),
                                                           (40, "4", 1, True), (40, "4", 1, False)],
                         ids=["lines", "points", "lines-motion", "points-motion", "batch-kernel-B40-motion", "batch-kernel-B40"])
def test_restart_equals_a_fresh_sequence(oracle, switches, B, pose, has_lines, motion_model):
    """Stream 1 of 3 (at B = 40: streams 0, 7, 13, 26 and 39, on the batch pose kernel selected as test_seq_pipeline_motion_model selects
    it) tracks sequence A for three frames and is then restarted onto sequence C while the others run on: every tracked frame of every
    stream equals its own oracle chain — A's, then C's from C's frame 0 — and the restart step reads as all-zero result bytes with
    counts[2..3] = 0 and the stereo counts of C's first frame."""
    if pose:
        switches({"STVO_POSE_KERNEL": pose})
    cfg = Cfg(has_lines, motion_model)
    restarted = {1} if B == 3 else {0, 7, 13, 26, B - 1}
    scripts = restart_scripts(oracle, cfg, B, restarted)
    ctx, dev = make_dev(B, cfg)
    try:
        out = drive(oracle, cfg, dev, scripts)
        from stvo_amd import capi
        want = capi.SCHED_POSE_BATCH if pose else capi.SCHED_POSE_LATENCY
        assert all(o[2]["pose_kernel"] == want for o in out[1:])
        # the restart is no accident of equal inputs: the restarted streams' tracked frames after it differ from what they would have
        # computed on the old sequence
        b = min(restarted)
        a_on = chain(oracle, cfg, sequence(3100 + b % 8), (3100 + b % 8, 0, 6))
        assert not np.allclose(out[4][0][b]["T"].reshape(4, 4), a_on[3]["T"], atol=1e-6)
    finally:
        dev.close()
        ctx.close()


@pytest.mark.parametrize("B,pose", [(3, None), (40, "4")], ids=["B3", "batch-kernel-B40"])
def test_neighbours_are_untouched(oracle, switches, B, pose):
    """The run above against the same inputs with no control at all: the result bytes and counts of the streams that never had a control
    are identical in every step, and so is stvo_seq_last_schedule of the control-free steps."""
    if pose:
        switches({"STVO_POSE_KERNEL": pose})
    cfg = Cfg(1, True)
    restarted = {1} if B == 3 else {0, 7, 13, 26, B - 1}
    scripts = restart_scripts(oracle, cfg, B, restarted)
    runs = []
    for control in (True, False):
        ctx, dev = make_dev(B, cfg)
        try:
            runs.append(drive(oracle, cfg, dev, scripts, control=control, check=control))
        finally:
            dev.close()
            ctx.close()
    others = [b for b in range(B) if b not in restarted]
    for t, ((ra, ca, sa, ctl), (rb, cb, sb, _)) in enumerate(zip(*runs)):
        for b in others:
            assert ra[b].tobytes() == rb[b].tobytes() and np.array_equal(ca[b], cb[b]), (t, b)
        if not ctl.any():
            assert sa == sb, (t, sa, sb)
    r = min(restarted)
    assert runs[0][3][0][r].tobytes() == ZERO_RESULT and runs[1][3][0][r].tobytes() != ZERO_RESULT   # the control-free run tracked across the cut


# ---- 3. sequencing edges

def test_sequencing_edges(oracle):
    """RESTART in the pipeline's first step (a no-op), in two consecutive steps of one stream, PARK -> RESTART, and
    RESTART -> RUN -> PARK -> RUN where the last RUN tracks against the frame pushed during the PARK."""
    cfg = Cfg(1, True)
    s0 = start(oracle, cfg, 3300, 3, first=RESTART) + start(oracle, cfg, 3301, 1, first=RESTART) + start(oracle, cfg, 3302, 3, first=RESTART)
    s1 = start(oracle, cfg, 3303, 2) + park(3304, [0]) + start(oracle, cfg, 3305, 4, first=RESTART)
    s2 = start(oracle, cfg, 3306, 1) + start(oracle, cfg, 3307, 2, first=RESTART) + park(3308, [0]) + resume(oracle, cfg, 3308, 0, 3)
    assert [e[0] for e in s0] == [RESTART, RUN, RUN, RESTART, RESTART, RUN, RUN]
    assert [e[0] for e in s1] == [RUN, RUN, PARK, RESTART, RUN, RUN, RUN]
    assert [e[0] for e in s2] == [RUN, RESTART, RUN, PARK, RUN, RUN, RUN]
    ctx, dev = make_dev(3, cfg)
    try:
        out = drive(oracle, cfg, dev, [s0, s1, s2])
        assert sum(r["status"] == 0 for o in out for r in o[0]) >= 8   # poses were accepted along the way
    finally:
        dev.close()
        ctx.close()


@pytest.mark.parametrize("B", [2, 20], ids=["B2-zero-copy", "B20-device-results"])
def test_restart_all_streams_at_once_and_one_shot(oracle, B):
    """Every stream restarted in the same step; the step after it runs all-RUN without a new call (its frames track), and a PARK of every
    stream behind that.  B = 20: results in device memory instead of the pinned block."""
    cfg = Cfg(1, False)
    scripts = [start(oracle, cfg, 3400 + b % 4, 2) + start(oracle, cfg, 3410 + b % 3, 3, first=RESTART) + park(3420, [0]) for b in range(B)]
    ctx, dev = make_dev(B, cfg)
    try:
        drive(oracle, cfg, dev, scripts)
    finally:
        dev.close()
        ctx.close()


def test_rotating_slots_with_a_control(oracle):
    """stvo_seq_set_slots + upload / step_dev: the control belongs to the step, whatever slot it runs on."""
    cfg = Cfg(1, False)
    a, c = sequence(3500)[:3], sequence(3501)[:3]
    ref_a, ref_c = chain(oracle, cfg, a, (3500, 0, 3)), chain(oracle, cfg, c, (3501, 0, 3))
    ctx, dev = make_dev(2, cfg)
    try:
        dev.set_slots(6)
        for k in range(3):
            dev.upload(k, [a[k], a[k]])
            dev.upload(3 + k, [a[k], c[k]])
        for t, slot in enumerate([0, 1, 2, 3, 4, 5]):
            if slot == 3:
                dev.control_next_step([RESTART, RESTART])
            dev.step_dev(slot)
            res, counts = dev.read()
            if slot in (0, 3):
                assert res.tobytes() == ZERO_RESULT * 2 and not counts[:, 2:].any()
                continue
            check_tracked(res[0], counts[0], ref_a[slot % 3 - 1], (t, 0))
            check_tracked(res[1], counts[1], (ref_a if slot < 3 else ref_c)[slot % 3 - 1], (t, 1))
    finally:
        dev.close()
        ctx.close()


def test_control_between_steps_enqueued_back_to_back(switches):
    """The schedule the control has to live with at large batches: the key-line stage one step AHEAD on its own stream (forced here for
    320 streams, as tests/test_gpu_seq.py::test_seq_steps_back_to_back_schedules_agree forces it), seven steps enqueued back to back with a
    control in the fourth and the sixth.  A step with a control gives up the grid and the key-line stage ahead, the step behind it runs
    ahead again, and the last step's results equal, bit for bit, those of the plain schedule with a read after every step."""
    from stvo_amd import capi
    B, S = 320, 3
    base = [synth.make_config5_sequence(s, n_frames=S, n_pts=300, n_lines=40, replica=3000) for s in range(8)]
    streams = [base[b % 8] for b in range(B)]
    cams = [synth.config5_cam(b % 8) for b in range(B)]
    mp = match_params("kitti"); op = opt_params("kitti")
    order = [0, 1, 2, 1, 0, 1, 2]
    ctl = {3: np.array([(RESTART if b % 10 == 0 else PARK if b % 10 == 5 else RUN) for b in range(B)], np.int32),
           5: np.array([(PARK if b % 7 == 0 else RESTART if b % 7 == 3 else RUN) for b in range(B)], np.int32)}

    def run(env, read_every_step):
        switches(env)
        ctx = capi.Context(device_id=0, max_rows=512, max_batch=B)
        dev = capi.Sequences(ctx, B, 512, 64, cams, mp, op)
        try:
            dev.set_motion_model(True)
            dev.set_trajectory(capi.traj_params("kitti", **KF), log_steps=1)
            dev.set_slots(S)
            for k in range(S):
                dev.upload(k, [st[k] for st in streams])
            sched = []
            for t, cur in enumerate(order):
                if t in ctl:
                    dev.control_next_step(ctl[t])
                dev.step_dev(cur)
                sched.append(dev.last_schedule())
                if read_every_step:
                    dev.read()
            res, counts = dev.read()
            return res.copy(), counts.copy(), dev.trajectory_state().copy(), sched
        finally:
            dev.close()
            ctx.close()

    ref_res, ref_counts, ref_state, _ = run({"STVO_LINES_AHEAD": "0"}, True)
    assert (ref_res["status"] == 0).mean() > 0.8
    res, counts, state, sched = run({"STVO_LINES_AHEAD": "1"}, False)
    print("[stream control] schedules:", [(s["cells_ahead"], s["lines_ahead"], s["gate"]) for s in sched])
    for t, s in enumerate(sched):
        if t in ctl:
            assert s["cells_ahead"] == 0 and s["lines_ahead"] == 0 and s["gate"] == 0 and s["mid_fork"] == 1, (t, s)
    assert sched[2]["lines_ahead"] == 1 and sched[4]["lines_ahead"] == 1 and sched[6]["lines_ahead"] == 1   # ahead again behind a control step
    assert np.array_equal(counts, ref_counts)
    assert res.tobytes() == ref_res.tobytes()
    assert state.tobytes() == ref_state.tobytes()


# ---- 4. trajectory

def test_trajectory_restart_and_park(oracle):
    import traj_host_lib
    from stvo_amd import capi
    cfg = Cfg(1, False, keyframes=True)
    s0 = start(oracle, cfg, 3600, 6)
    s1 = start(oracle, cfg, 3601, 3) + start(oracle, cfg, 3602, 3, first=RESTART)
    s2 = start(oracle, cfg, 3603, 3) + park(3604, [0, 1, 2])
    scripts = [s0, s1, s2]
    init = traj_host_lib.init(1).tobytes()
    ctx, dev = make_dev(3, cfg)
    try:
        dev.set_trajectory(capi.traj_params("kitti", **KF), log_steps=2)
        seen = {}

        def after_step(t, res, counts):
            got = dev.read_trajectory(5)
            st = dev.trajectory_state()
            if t == 0:
                assert got.shape == (0, 3) and st.tobytes() == init * 3
                seen["state"] = st.copy()
                return
            assert got.shape == (min(t, 2), 3)
            for b in range(3):
                ctl, _, o, (_, k) = scripts[b][t]
                rec = got[-1][b]
                if o is None:
                    assert rec.tobytes() == bytes(TRAJ_RECORD_DTYPE.itemsize), (t, b)   # frame == 0: no pose in this step
                    if ctl == RESTART:
                        assert st[b].tobytes() == init, (t, b)
                    else:   # PARK: bit for bit what it was
                        assert st[b].tobytes() == seen["state"][b].tobytes(), (t, b)
                else:
                    compare_record(rec, o)
                    assert rec["frame"] == k, (t, b, rec["frame"], k)   # counts from 1 in every sequence
            if t >= 3:
                assert st[0].tobytes() != seen["state"][0].tobytes()   # the others' states move while stream 2 is parked
            seen["state"] = st.copy()

        drive(oracle, cfg, dev, scripts, after_step=after_step)
        st = dev.trajectory_state()
        for b, (seed, n) in enumerate(((3600, 6), (3602, 3), (3603, 3))):
            ref = chain(oracle, cfg, sequence(seed)[:n], (seed, 0, n))
            assert st[b]["n_frames"] == n - 1 and st[b]["n_keyframes"] == sum(o["new_kf"] for o in ref), (b, st[b]["n_frames"], st[b]["n_keyframes"])
    finally:
        dev.close()
        ctx.close()


# ---- 5. FAST thresholds, rule level, no images

@pytest.mark.parametrize("B", [3, 70], ids=["B3-pinned-results", "B70-device-results"])
def test_fast_thresholds_rule_level(oracle, B):
    """stvo_seq_restart_fast_dev writes th0 to the staged RESTART streams and to nothing else (and launches nothing when nothing is
    staged); stvo_seq_adapt_fast_dev behind a step with a control moves the RUN streams only, by np_fast_adapt.update on that step's
    results, and behind the next step every stream again.  B = 70: more than one workgroup of the rule, no multiple of its 64 lanes."""
    import torch
    from stvo_amd import capi
    cfg = Cfg(0, False)
    prm = capi.fast_adapt_params("kitti")
    ctl = np.array([(RUN, RESTART, PARK)[b % 3] for b in range(B)], np.int32)
    if B > 3:
        ctl[[0, B - 1]] = RESTART, PARK
    fr = [sequence(3700 + b % 4, 4) for b in range(B)]
    th_start = np.array([(20, 7, 27, 30, 12, 45)[b % 6] for b in range(B)], np.int32)
    ctx, dev = make_dev(B, cfg, max_rows=512)
    try:
        th = torch.cat([torch.from_numpy(th_start.copy()), torch.full((3,), -77, dtype=torch.int32)]).to("cuda:0")
        torch.cuda.synchronize()
        tail = lambda: th.cpu().numpy()[B:].tolist() == [-77] * 3   # nothing beyond B is touched
        now = lambda: (ctx.synchronize(), th.cpu().numpy()[:B].copy())[1]
        dev.restart_fast_dev(th[:B], 20)                       # nothing staged: nothing changes
        assert now().tolist() == th_start.tolist()
        dev.push([f[0] for f in fr])
        dev.push([f[1] for f in fr])
        dev.control_next_step(np.zeros(B, np.int32))           # all-RUN stages nothing
        dev.restart_fast_dev(th[:B], 20)
        assert now().tolist() == th_start.tolist()
        dev.control_next_step(ctl)
        dev.restart_fast_dev(th[:B], 19)
        exp = np.where(ctl == RESTART, 19, th_start).astype(np.int32)
        assert now().tolist() == exp.tolist() and tail()
        res, _ = dev.push([f[2] for f in fr])
        assert all(res[b].tobytes() == ZERO_RESULT for b in range(B) if ctl[b] != RUN)
        dev.adapt_fast_dev(prm, th[:B])
        moved = np_fast_adapt.update_batch(exp, res, prm)
        exp2 = np.where(ctl == RUN, moved, exp).astype(np.int32)
        got = now()
        assert got.tolist() == exp2.tolist() and tail(), (got.tolist(), exp2.tolist())
        assert np.any(exp2 != exp)                             # the rule moved something
        assert np.any(np_fast_adapt.update_batch(exp, res, prm)[ctl != RUN] != exp[ctl != RUN])   # ... and would have moved the others
        dev.restart_fast_dev(th[:B], 20)                       # the control was one-shot: nothing staged any more
        assert now().tolist() == exp2.tolist()
        res, _ = dev.push([f[3] for f in fr])
        dev.adapt_fast_dev(prm, th[:B])                        # behind a step without a control: every stream
        exp3 = np_fast_adapt.update_batch(exp2, res, prm)
        assert now().tolist() == exp3.tolist() and tail()
        assert np.any(exp3[ctl == PARK] != exp2[ctl == PARK])
    finally:
        dev.close()
        ctx.close()


# ---- 6. images -> poses, thresholds and trajectory with a restart mid-way

def check_image_record(rec, o, where):
    """The record of a tracked frame of the image test (an addition to what the poses and thresholds show; the records of tests 4 and 8
    are held to compare_record as it stands).  Tfw as compare_record holds it.  Tfw_cov is a sum of products Ad * cov * Ad^T over the
    frames so far (unccomp_se3), with the entries of Ad of order one on these scenes, and every element of a pose kernel's cov is accepted
    within rtol = 1e-6 of its own size (tests/test_gpu_seq.py::run_and_compare) — an ABSOLUTE error of 1e-6 x the large entries, which
    the composition carries into the small off-diagonal entries of Tfw_cov unchanged.  So the bound is absolute, 1e-6 x the largest
    entry of the reference Tfw_cov; compare_record's element-wise rtol asks of the small entries more than the inputs hold (measured
    here, on the stream that never has a control: up to 1.0e-9, e.g. 4e-10 on an entry of 5.6e-5 beside a diagonal of 1.2; every other
    record within 7e-13)."""
    assert np.allclose(rec["Tfw"].reshape(4, 4), o["Tfw"], atol=1e-7), where
    dev = np.abs(rec["Tfw_cov"].reshape(6, 6) - o["Tfw_cov"]).max()
    print(f"[stream control] image record {where}: max |Tfw_cov - ref| = {dev:.3e}, largest entry {np.abs(o['Tfw_cov']).max():.3e}")
    assert dev <= 1e-6 * np.abs(o["Tfw_cov"]).max(), (where, dev)


def test_image_pipeline_restart(oracle):
    """ImagePipeline(adaptive_fast, trajectory), B = 2, the image size and scenes of tests/test_gpu_adaptive_fast.py: stream 0 runs scene 0
    for six frames, stream 1 runs scene 1 for three and is restarted onto scene 2.  Poses, trajectory records and thresholds frame by
    frame against the CPU chain of each scene (a chain is causal: its first frames are the chain of the shorter sequence); the restart
    frame is detected at fast_threshold although the stream's threshold had moved."""
    import fast_adapt_cases as fc
    from stvo_amd import capi, images
    chains, imgs = fc.cpu_chain(oracle), fc.images()
    plan = [[(0, k) for k in range(6)], [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]]
    assert chains[1]["after"][1] != fc.TH0     # stream 1's threshold has left fast_threshold when the restart comes
    B = 2
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        pipe = images.ImagePipeline(ctx, B, fc.CAM, match_params("kitti"), opt_params("kitti", has_lines=0), max_kp=fc.MAX_KP, nfeatures=fc.NFEATURES,
                                    fast_threshold=fc.TH0, adaptive_fast=fc.params(), trajectory=capi.traj_params("kitti", keyframes=False),
                                    trajectory_log=1)
        try:
            for t in range(6):
                left = np.stack([imgs[s][k][0] for s, k in (plan[0][t], plan[1][t])])
                right = np.stack([imgs[s][k][1] for s, k in (plan[0][t], plan[1][t])])
                res, counts = pipe.push_images(left, right, control=[RUN, RESTART] if t == 3 else None)
                th = pipe.fast_thresholds()
                rec = pipe.read_trajectory()
                for b in range(B):
                    s, k = plan[b][t]
                    if k == 0:
                        assert res[b].tobytes() == ZERO_RESULT and not counts[b, 2:].any()
                        assert th[b] == fc.TH0, (t, b, th)            # reset before the detection, and no rule behind an initialize
                        if t:
                            assert rec[0][b].tobytes() == bytes(TRAJ_RECORD_DTYPE.itemsize)
                            # detected at fast_threshold: the stereo set of the restart frame is the one the chain's first frame has
                            pattern = oracle.orb_default_pattern()
                            det = [oracle.orb_detect_levels(im, nfeatures=fc.NFEATURES, nlevels=1, fast_th=fc.TH0, pattern=pattern, cap=fc.MAX_KP)
                                   for im in imgs[s][0]]
                            z4 = np.zeros((0, 4), np.float32); zd = np.zeros((0, 32), np.uint8)
                            fr = dict(kp_l=det[0]["kp"], oct_l=det[0]["octave"], desc_l=det[0]["desc"], kp_r=det[1]["kp"], desc_r=det[1]["desc"],
                                      kl_l=z4, oct_ll=np.zeros(0, np.int32), ldesc_l=zd, kl_r=z4, ldesc_r=zd)
                            n_ref = len(pipeline_ref.stereo_frame(oracle, fr, fc.CAM, match_params("kitti"), True, False)["P"])
                            assert counts[b, 0] == n_ref, (counts[b], n_ref)
                        continue
                    o = chains[s]["ref"][k - 1]
                    r = res[b]
                    assert counts[b, 0] == o["n_stereo_pt"] and r["n_matched_pt"] == o["n_matched_pt"], (t, b, counts[b], o["n_stereo_pt"], o["n_matched_pt"])
                    assert r["status"] == o["status"] and r["path"] == o["path"] and tuple(r["iters"]) == o["iters"], (t, b)
                    assert r["n_inliers_pt"] == o["n_inliers_pt"], (t, b)
                    assert np.allclose(r["T"].reshape(4, 4), o["T"], atol=1e-8), (t, b)
                    assert th[b] == chains[s]["after"][k - 1], (t, b, th)
                    check_image_record(rec[0][b], o, (t, b))
                    assert rec[0][b]["frame"] == k and rec[0][b]["new_kf"] == 0
        finally:
            pipe.close()
    finally:
        ctx.close()


# ---- 7. fetch by-products

@pytest.mark.parametrize("B", [1, 2, 20], ids=["B1-by-the-pose-kernel", "B2-pinned-inliers", "B20-copies"])
def test_fetch_by_products(oracle, B):
    """With stvo_seq_enable_fetch the f2f match rows and the inlier rows of a RESTART stream are all -1 in that step and its stereo match
    rows those of the new frame; every other row of every step equals the control-free run on the same frames."""
    cfg = Cfg(1, False)
    frames = [sequence(3800 + b % 4, 4) for b in range(B)]
    r = B - 1
    runs = []
    for control in (True, False):
        ctx, dev = make_dev(B, cfg)
        try:
            dev.enable_fetch(True)
            steps = []
            for k in range(4):
                if control and k == 2:
                    dev.control_next_step([RESTART if b == r else RUN for b in range(B)])
                res, counts = dev.push([f[k] for f in frames])
                m = dev.fetch_matches()
                inl = dev.fetch_inliers() if k else None
                steps.append((res.copy(), counts.copy(), m, inl))
            runs.append(steps)
        finally:
            dev.close()
            ctx.close()
    for k, ((ra, ca, ma, ia), (rb, cb, mb, ib)) in enumerate(zip(*runs)):
        assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1]), k     # stereo rows: those of the frame, control or not
        others = [b for b in range(B) if not (b == r and k == 2)]
        for b in others:
            assert np.array_equal(ma[2][b], mb[2][b]) and np.array_equal(ma[3][b], mb[3][b]), (k, b)
            if k:
                assert np.array_equal(ia[0][b], ib[0][b]) and np.array_equal(ia[1][b], ib[1][b]), (k, b)
            assert ra[b].tobytes() == rb[b].tobytes(), (k, b)
        if k == 2:
            assert (ma[2][r] == -1).all() and (ma[3][r] == -1).all()
            assert (ia[0][r] == -1).all() and (ia[1][r] == -1).all()
            assert ra[r].tobytes() == ZERO_RESULT
            assert (mb[2][r] >= 0).sum() > 50 and (ib[0][r] == 1).sum() > 50   # the control-free run matched across the cut
    assert (runs[0][3][2][2][r] >= 0).sum() > 50   # the frame after the restart tracks again


# ---- 8. ragged.run

def test_ragged_run(oracle):
    """Five sequences of 2, 3, 4, 6 and 3 frames on two streams: every sequence's results, counts and trajectory records equal its own
    oracle chain, and every stream-step of the plan is accounted for."""
    from stvo_amd import capi
    cfg = Cfg(1, True, keyframes=True)
    lengths = (2, 3, 4, 6, 3)
    seqs = [sequence(3900 + i)[:n] for i, n in enumerate(lengths)]
    steps = ragged.plan(lengths, 2)
    assert sum(c is not None for st in steps for c in st.consume) == sum(lengths)
    assert sum(c is not None for st in steps for c in st.consume) + sum(int((st.control == PARK).sum()) for st in steps) == 2 * len(steps)
    ctx, dev = make_dev(2, cfg)
    try:
        dev.set_trajectory(capi.traj_params("kitti", **KF), log_steps=1)
        results, counts, records = ragged.run(dev, seqs)
    finally:
        dev.close()
        ctx.close()
    for i, n in enumerate(lengths):
        ref = chain(oracle, cfg, seqs[i], (3900 + i, 0, n))
        assert results[i].shape == (n,) and counts[i].shape == (n, 4) and records[i].shape == (n - 1,)
        assert results[i][0].tobytes() == ZERO_RESULT and not counts[i][0, 2:].any()
        assert tuple(counts[i][0, :2]) == stereo_counts(oracle, cfg, seqs[i][0], (3900 + i, 0))
        for k in range(1, n):
            check_tracked(results[i][k], counts[i][k], ref[k - 1], (i, k))
            compare_record(records[i][k - 1], ref[k - 1])
            assert records[i][k - 1]["frame"] == k


def test_ragged_run_parks_streams_without_a_sequence(oracle):
    """More streams than sequences, and a stream that runs out: parked streams are fed empty frames and report nothing."""
    cfg = Cfg(1, False)
    lengths = (4, 2)
    seqs = [sequence(3950 + i)[:n] for i, n in enumerate(lengths)]
    ctx, dev = make_dev(3, cfg)
    try:
        results, counts, records = ragged.run(dev, seqs)
        res, cnt = dev.read()
        assert res[1].tobytes() == ZERO_RESULT and res[2].tobytes() == ZERO_RESULT and not cnt[1:].any()   # the last step parked streams 1 and 2
    finally:
        dev.close()
        ctx.close()
    assert records is None
    for i, n in enumerate(lengths):
        ref = chain(oracle, cfg, seqs[i], (3950 + i, 0, n))
        for k in range(1, n):
            check_tracked(results[i][k], counts[i][k], ref[k - 1], (i, k))


# ---- 9. argument checks: each refused, each refusal changes nothing

def test_argument_checks(oracle):
    import torch
    from stvo_amd import capi
    cfg = Cfg(1, False)
    fr = sequence(3990, 3)
    ref = chain(oracle, cfg, fr, (3990, 0, 3))
    INVALID = -1
    ctx, dev = make_dev(2, cfg)
    try:
        L = ctx.lib
        ok = np.array([RESTART, PARK], np.int32)
        assert L.stvo_seq_control_next_step(None, ok.ctypes.data_as(C.c_void_p)) == INVALID
        assert L.stvo_seq_control_next_step(dev.h, None) == INVALID
        th = torch.full((2,), 11, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        assert L.stvo_seq_restart_fast_dev(None, th.data_ptr(), 20) == INVALID
        assert L.stvo_seq_restart_fast_dev(dev.h, None, 20) == INVALID
        dev.push([fr[0], fr[0]])
        for bad in ([3, 0], [0, -1], [RESTART, 3]):
            with pytest.raises(capi.StvoError):
                dev.control_next_step(bad)
        with pytest.raises(ValueError):
            dev.control_next_step([RESTART])          # one word per stream
        for th0 in (0, 255, -4):
            assert L.stvo_seq_restart_fast_dev(dev.h, th.data_ptr(), th0) == INVALID
        dev.restart_fast_dev(th, 20)                  # nothing was staged by the refused calls
        ctx.synchronize()
        assert th.cpu().numpy().tolist() == [11, 11]
        res, counts = dev.push([fr[1], fr[1]])        # ... and the next step is all-RUN
        for b in range(2):
            check_tracked(res[b], counts[b], ref[0], b)
        # a refused call leaves a control staged before it in place
        dev.control_next_step([RUN, RESTART])
        with pytest.raises(capi.StvoError):
            dev.control_next_step([RUN, 7])
        res, counts = dev.push([fr[2], fr[2]])
        check_tracked(res[0], counts[0], ref[1], 0)
        assert res[1].tobytes() == ZERO_RESULT
        with pytest.raises(ValueError):
            dev.restart_fast_dev(torch.zeros(3, dtype=torch.int32, device="cuda:0"), 20)
    finally:
        dev.close()
        ctx.close()
