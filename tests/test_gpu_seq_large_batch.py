"""GPU parity of the device-resident per-frame pipeline (stvo_seq_*) at the batch sizes bench.py's `value` is quoted on: more than
two streams per CU, where the host takes other routes than for the few hundred streams the rest of the suite runs — the batch pose
kernel with TWO waves per frame pair, the key-line stage one step AHEAD behind the stream gate with the second copy of the key-line
match indices in use, K1m's "partial tiles last" remap over a batch that is no multiple of eight, and beyond four streams per CU a
second residency round of the pose kernel.  Every stream is compared with the oracle-driven per-frame loop (tests/pipeline_ref.py), on
default switches, read after every step and with the steps enqueued back to back (only then do the overlaps happen), and every test
asserts through Sequences.last_schedule() that the step took the route it is about.

The gap these tests close is one of batch COUNT, so the frames are small (a few hundred key-points, at most 58 key-lines) and the
batch sizes are the smallest that cross each threshold, derived from the CU count of the device; one test uses the headline's frame
shape.  Streams and oracle results are built once per process and shared by the tests."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import np_model
import pipeline_ref
from fuzz_pipeline import oracle_sensitivity
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params

pytestmark = pytest.mark.gpu

PTS = [300, 6, 340, 120, 260, 40, 400, 200, 12, 380, 160]
LNS = [40, 0, 48, 12, 30]
ORDER = [0, 1, 2, 1, 0, 1, 2]   # 0->1, 1->2 forward; 2->1, 1->0 backward; then forward again
SENSITIVITY_SHARE = 0.01        # at most this share of the compared cases may be judged by the oracle's own sensitivity

_MIX = dict(streams=[], cams=[], refs={})        # the small mix: stream b, and (b, from, to) -> oracle result
_HEADLINE = dict(streams=[], cams=[], refs={})   # the headline frame shape


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _params():
    return match_params("kitti"), opt_params("kitti")


def _mix_stream(b):
    seq = synth.make_config5_sequence(b % 8, n_frames=3, n_pts=PTS[b % 11], n_lines=LNS[b % 5], replica=2000 + b // 8)
    if b % 53 == 7:   # the right camera dropped out in frame 1 (as in test_seq_pipeline_empty_and_tiny_frames)
        z2 = np.zeros((0, 2), np.float32); zd = np.zeros((0, 32), np.uint8); z4 = np.zeros((0, 4), np.float32)
        seq[1] = dict(seq[1], kp_r=z2, desc_r=zd, kl_r=z4, ldesc_r=zd)
    return seq


def _headline_stream(b):
    return synth.make_config5_sequence(b % 8, n_frames=3, n_pts=1650, n_lines=85, replica=400 + b // 8)


def _prepare(cache, make, oracle, B, transitions):
    """Streams 0 .. B - 1 of `cache` and the oracle's results of `transitions` for each of them: built once, never changed."""
    mp, op = _params()
    with ThreadPoolExecutor(16) as ex:   # numpy's generators and the oracle's C functions run outside the GIL
        n0 = len(cache["streams"])
        if B > n0:
            cache["streams"] += list(ex.map(make, range(n0, B)))
            cache["cams"] += [synth.config5_cam(b % 8) for b in range(n0, B)]
        todo = [(b, a, c) for (a, c) in transitions for b in range(B) if (b, a, c) not in cache["refs"]]

        def ref_pair(key):
            b, a, c = key
            return pipeline_ref.run_sequence(oracle, [cache["streams"][b][a], cache["streams"][b][c]], cache["cams"][b], mp, op)[0]
        for key, o in zip(todo, ex.map(ref_pair, todo)):
            cache["refs"][key] = o
    return cache["streams"][:B], cache["cams"][:B]


def _transitions(n_steps):
    return [(ORDER[k - 1], ORDER[k]) for k in range(1, n_steps)]


def _open(B, streams, cams, max_kp, max_kl, max_rows):
    from stvo_amd import capi
    mp, op = _params()
    ctx = capi.Context(device_id=0, max_rows=max_rows, max_batch=B)
    try:
        dev = capi.Sequences(ctx, B, max_kp, max_kl, cams, mp, op)
    except Exception:
        ctx.close()
        raise
    try:
        dev.set_slots(3)
        for k in range(3):
            dev.upload(k, [st[k] for st in streams])
    except Exception:
        dev.close()
        ctx.close()
        raise
    return ctx, dev


class Judge:
    """The comparison of tests/test_gpu_seq.py (run_and_compare and the headline-shape test) for one (stream, transition) at a time.
    A case that misses the plain numeric tolerances, or takes another course through the optimiser, is judged as tests/fuzz_pipeline.py
    judges it — by how far the ORACLE's own answer moves under a few roundings of its inputs (oracle_sensitivity, its bounds unchanged);
    discrete fields are excused only where that sensitivity is not finite — and is counted: finish() allows SENSITIVITY_SHARE of them."""

    def __init__(self, oracle, cache, tag):
        self.oracle, self.cache, self.tag = oracle, cache, tag
        self.n = 0
        self.bad, self.sens = [], []

    def compare(self, res, counts, a, c):
        mp, op = _params()
        for b in range(len(res)):
            o, r = self.cache["refs"][(b, a, c)], res[b]
            self.n += 1
            where = (b, f"{a}->{c}")
            if not (counts[b, 0] == o["n_stereo_pt"] and counts[b, 1] == o["n_stereo_ls"]):
                self.bad.append(where + ("stereo counts", tuple(counts[b, :2]), (o["n_stereo_pt"], o["n_stereo_ls"])))
                continue
            if not (r["n_matched_pt"] == o["n_matched_pt"] and r["n_matched_ls"] == o["n_matched_ls"]):
                self.bad.append(where + ("n_matched_pt / n_matched_ls", (int(r["n_matched_pt"]), int(r["n_matched_ls"])), (o["n_matched_pt"], o["n_matched_ls"])))
                continue
            frames = [self.cache["streams"][b][a], self.cache["streams"][b][c]]
            got = (int(r["status"]), int(r["path"]), tuple(int(i) for i in r["iters"]), int(r["n_inliers_pt"]), int(r["n_inliers_ls"]))
            exp = (o["status"], o["path"], tuple(o["iters"]), o["n_inliers_pt"], o["n_inliers_ls"])
            if got != exp:
                sT = oracle_sensitivity(self.oracle, frames, self.cache["cams"][b], mp, op, False, 0, trials=24)[0]
                (self.sens if not np.isfinite(sT) else self.bad).append(where + ("status / path / iters / inliers", got, exp))
                continue
            T, cov = r["T"].reshape(4, 4), r["cov"].reshape(6, 6)
            if (np_model.rot_angle(T[:3, :3], o["T"][:3, :3]) < 1e-4 and np.linalg.norm(T[:3, 3] - o["T"][:3, 3]) < 1e-3
                    and np.allclose(T, o["T"], atol=1e-8) and np.isclose(r["err"], o["err"], rtol=1e-8)
                    and np.allclose(cov, o["cov"], rtol=1e-6, atol=1e-12)):
                continue
            cscale = float(np.max(np.abs(o["cov"])))
            dT = float(np.max(np.abs(T - o["T"])))
            derr = abs(r["err"] - o["err"]) / max(abs(o["err"]), 1e-300)
            dcov = float(np.max(np.abs(cov - o["cov"]))) / cscale if cscale > 0 else float(np.max(np.abs(cov)))
            sT, serr, scov = oracle_sensitivity(self.oracle, frames, self.cache["cams"][b], mp, op, False, 0)
            fig = where + ("pose / err / cov", (dT, derr, dcov), "oracle's own sensitivity", (sT, serr, scov), "key-points", len(frames[0]["kp_l"]))
            ok = dT <= max(1e-8, 100 * sT) and derr <= max(1e-8, 100 * serr) and dcov <= max(1e-6, 100 * scov)
            (self.sens if ok else self.bad).append(fig)

    def finish(self):
        print(f"[large batch] {self.tag}: {self.n} cases compared, {len(self.sens)} judged by the oracle's sensitivity "
              f"({100.0 * len(self.sens) / max(self.n, 1):.2f} %), {len(self.bad)} wrong")
        assert self.n > 0
        assert not self.bad, (self.tag, len(self.bad), "of", self.n, "cases differ from the oracle; the first:", self.bad[:12])
        assert len(self.sens) <= SENSITIVITY_SHARE * self.n, (self.tag, len(self.sens), "of", self.n, "cases needed the sensitivity route:", self.sens)


def _assert_mix_is_mixed(cache, B, transitions):
    seen = {cache["refs"][(b, a, c)]["status"] for (a, c) in transitions for b in range(B)}
    assert {0, 1, 2, 3} <= seen, ("the stream mix no longer reaches every status", sorted(seen))


def _assert_two_waves_lines_ahead(sch, step):
    """The default route of a tracked step beyond two streams per CU; `step` counts the steps of the Sequences from 0."""
    from stvo_amd import capi
    assert sch["pose_kernel"] == capi.SCHED_POSE_BATCH and sch["pose_waves"] == 2, (step, sch)
    assert sch["fused_cells"] == 0 and sch["mid_fork"] == 1, (step, sch)
    # the key-line stage runs ahead from the first step whose predecessor launched a pose kernel that publishes its start: the first
    # step builds the first stereo sets only, the second launches the first pose kernel, the third is the first that can wait for it
    ahead = 1 if step >= 2 else 0
    assert sch["lines_ahead"] == ahead and sch["gate"] == ahead and sch["cells_ahead"] >= ahead, (step, sch)


def _read_after_every_step(oracle, B, tag, check_schedule):
    streams, cams = _prepare(_MIX, _mix_stream, oracle, B, _transitions(5))
    _assert_mix_is_mixed(_MIX, B, _transitions(5))
    judge = Judge(oracle, _MIX, tag)
    ctx, dev = _open(B, streams, cams, 512, 64, 512)
    try:
        for k, cur in enumerate(ORDER[:5]):
            dev.step_dev(cur)
            sch = dev.last_schedule()
            res, counts = dev.read()
            if k > 0:
                check_schedule(sch, k)
                judge.compare(res, counts, ORDER[k - 1], cur)
    finally:
        dev.close()
        ctx.close()
    judge.finish()


def test_at_the_threshold_four_waves_no_lines_ahead(oracle):
    """B = 2 x CUs exactly: the conditions are `B > 2 x CUs`, so the batch pose kernel still takes FOUR waves per pair and the key-line
    stage stays in its own step.  Every stream against the oracle on the four transitions, read after every step."""
    from stvo_amd import capi
    B = 2 * _cus()

    def check(sch, step):
        assert sch["pose_kernel"] == capi.SCHED_POSE_BATCH and sch["pose_waves"] == 4, (step, sch)
        assert sch["lines_ahead"] == 0 and sch["gate"] == 0 and sch["fused_cells"] == 0, (step, sch)
    _read_after_every_step(oracle, B, f"B {B} (2 x CUs), read after every step", check)


def test_just_over_the_threshold_two_waves_lines_ahead(oracle):
    """B = 2 x CUs + 11 — not a multiple of 8, so the last group of eight frames K1m deals to the XCDs is partly empty —: two waves per
    pair from the first transition on, the key-line stage ahead and behind the gate from the first step that can be.  Every stream
    against the oracle on the four transitions, read after every step."""
    B = 2 * _cus() + 11
    _read_after_every_step(oracle, B, f"B {B} (2 x CUs + 11), read after every step", _assert_two_waves_lines_ahead)


def test_beyond_one_residency_round(oracle):
    """B = 4 x CUs + 76 (1100 on 256 CUs; neither a multiple of 8 nor of 1024): the two-wave pose kernel needs a second residency
    round and K1m's remap spans more than one dispatch round.  The checks of the test above on every stream, and the raw stereo
    matches of the last step of streams at both ends of the batch and on both sides of the first round's edge."""
    cus = _cus()
    B = 4 * cus + 76
    _read_after_every_step(oracle, B, f"B {B} (4 x CUs + 76), read after every step", _assert_two_waves_lines_ahead)
    # the by-product fetch needs a pipeline of its own: with it on, the copies read the first copy of the key-line match indices, so the
    # key-line stage cannot run ahead (the record says so) — the point matcher it reads is the same
    streams, cams = _MIX["streams"][:B], _MIX["cams"][:B]
    mp, _ = _params()
    ctx, dev = _open(B, streams, cams, 512, 64, 512)
    try:
        dev.enable_fetch(True)
        for cur in ORDER[:5]:
            dev.step_dev(cur)
        assert dev.last_schedule()["lines_ahead"] == 0 and dev.last_schedule()["pose_waves"] == 2
        dev.read()
        ms_p = dev.fetch_matches()[0].copy()
    finally:
        dev.close()
        ctx.close()
    last = ORDER[4]
    for b in (0, 7, 4 * cus - 1, 4 * cus, B - 1):
        ref = pipeline_ref.stereo_frame(oracle, streams[b][last], cams[b], mp, True, False)
        assert np.array_equal(ms_p[b, :len(streams[b][last]["kp_l"])], ref["m12_raw_p"]), b


@pytest.mark.parametrize("L", [3, 5, 7])
@pytest.mark.parametrize("size", ["2xCUs+11", "4xCUs+76"])
def test_steps_back_to_back(oracle, size, L):
    """The first L steps of 0, 1, 2, 1, 0, 1, 2 enqueued with NO read in between — only then do the step overlaps of the default
    schedule happen: the key-line kernels of step k + 1 beside the pose kernel of step k, writing the other copy of the key-line match
    indices — then one read: every stream of that last step against the oracle's pair of its transition (1 -> 2, 1 -> 0, 1 -> 2).
    Key-line counts and n_matched_ls are part of the comparison: a stale copy of the line match indices shows there."""
    cus = _cus()
    B = 2 * cus + 11 if size == "2xCUs+11" else 4 * cus + 76
    a, c = ORDER[L - 2], ORDER[L - 1]
    streams, cams = _prepare(_MIX, _mix_stream, oracle, B, [(a, c)])
    judge = Judge(oracle, _MIX, f"B {B} ({size}), {L} steps back to back")
    ctx, dev = _open(B, streams, cams, 512, 64, 512)
    try:
        for cur in ORDER[:L]:
            dev.step_dev(cur)
        sch = dev.last_schedule()
        res, counts = dev.read()
    finally:
        dev.close()
        ctx.close()
    _assert_two_waves_lines_ahead(sch, L - 1)
    assert counts[:, 1].max() > 0 and res["n_matched_ls"].max() > 0   # key-lines take part
    judge.compare(res, counts, a, c)
    judge.finish()


@pytest.mark.parametrize("L", [3, 4])
def test_headline_frame_shape_over_the_threshold(oracle, L):
    """The frame shape bench.py's `value` is quoted on (1650 landmarks ~ 2000 key-points, 85 segments ~ 100 key-lines, the eight
    sequence ids of configs[4]) at B = 2 x CUs + 8, the first L steps of 0, 1, 2, 1 back to back on default switches, then one read:
    EVERY stream against the oracle (1 -> 2 forward, 2 -> 1 backward) on the default large-batch schedule."""
    B = 2 * _cus() + 8
    a, c = ORDER[L - 2], ORDER[L - 1]
    streams, cams = _prepare(_HEADLINE, _headline_stream, oracle, B, [(a, c)])
    judge = Judge(oracle, _HEADLINE, f"B {B} (2 x CUs + 8), headline frame shape, {L} steps back to back")
    ctx, dev = _open(B, streams, cams, 2048, 128, 2048)
    try:
        for cur in ORDER[:L]:
            dev.step_dev(cur)
        sch = dev.last_schedule()
        res, counts = dev.read()
    finally:
        dev.close()
        ctx.close()
    _assert_two_waves_lines_ahead(sch, L - 1)
    judge.compare(res, counts, a, c)
    judge.finish()
    assert (res["status"] == 0).mean() > 0.95 and res["n_matched_pt"].mean() > 1300
