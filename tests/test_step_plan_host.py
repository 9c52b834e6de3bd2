"""The step planner (stvo-pl_amd/csrc/step_plan.h: plan_step + commit) on the CPU: the header is built for the host with g++ (no GPU, no
HIP) and every expectation below is written by hand from the rules, never produced by calling the planner.

`caps` states what the launch helpers answer for a batch (kernels.h / their definitions): the one-workgroup point matcher fits,
match_small_ok(stride) = 0 < stride <= 512, pose_inline_sync_ok = 1 <= B <= 16 unless STVO_POSE_KERNEL=4, the batch pose kernel beyond 256
frame pairs or with STVO_POSE_KERNEL=4 (never with 1) — it publishes its start —, on two waves per pair beyond two pairs per CU and four
otherwise; and what stvo_seq_create gives a batch: results written straight to the host up to 16 streams, the second copy of the
key-line match indices and of the grid buffers from 64 streams on."""
import itertools

import pytest

import step_plan_host_lib as sp
from step_plan_host_lib import BOTH_DIRS, LAZY, ONE_WAY, SMALL

CUS = [256, 40]   # 40: the smallest round count whose "two streams per CU" still lies beyond the 64 streams the mid fork starts at


def caps(B, cus, K=512, M=320, pose_kernel=sp.UNSET):
    batch = pose_kernel == 4 or (pose_kernel != 1 and B > 256)
    return dict(B=B, K=K, M=M, cus=cus, zero_copy=B <= 16, has_alt_m12l=B >= 64, cells_differ=B >= 64, grid_points_fused_ok=1,
                match_small_ok_K=0 < K <= 512, match_small_ok_M=0 < M <= 512, pose_inline_sync_ok=1 <= B <= 16 and pose_kernel != 4,
                pose_batch_kernel_selected=batch, pose_start_flag_ok=batch, pose2p_waves_per_pair=(2 if B > 2 * cus else 4) if batch else 0)


def facts(B, cus, frame_idx=3, sw=None, **kw):
    """A tracked step of a sequence with key-points and ~40 key-lines per image, behind steps that did the same."""
    K, M = kw.pop("K", 512), kw.pop("M", 320)
    f = dict(has_points=1, has_lines=1, best_lr_matches=1, lines_now=1, lines_prev=1, track=1, frame_idx=frame_idx, raw_split=0,
             raw_max_lines=40, set_lines_cap_prev=64, set_lines_cap_cur=64, st_dirty=1, fetch=0, timing=0, timing_events=0)
    f.update(caps(B, cus, K, M, (sw or {}).get("pose_kernel", sp.UNSET)))
    f.update(kw)
    return f


def plan(B, cus, sw=None, history=None, lds_fits=True, frame_idx=3, **kw):
    h = (frame_idx - 1,) * 3 if history is None else history
    return sp.plan(facts(B, cus, frame_idx, sw, **kw), sw, h, lds_fits)[0]


# ---- each side of every threshold ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cus", CUS)
def test_mid_fork_from_64_streams(cus):
    a, b = plan(63, cus), plan(64, cus)
    assert (a["par"], a["mid_fork"], a["fork_at_start"], a["line_forked"]) == (1, 0, 1, 1)
    assert (b["par"], b["mid_fork"], b["fork_at_start"], b["line_forked"]) == (1, 1, 0, 1)
    # single-stream operation: the upload split the slot and the point stream is clean — no event at all
    c = plan(1, cus, raw_split=1, st_dirty=0)
    assert (c["par"], c["mid_fork"], c["fork_at_start"], c["line_forked"]) == (1, 0, 0, 0)
    assert plan(1, cus, raw_split=1, st_dirty=1)["fork_at_start"] == 1 and plan(1, cus, raw_split=0, st_dirty=0)["fork_at_start"] == 1
    # no key-lines in the frame, or no key-points at all: nothing runs on the line stream
    d = plan(64, cus, lines_now=0)
    assert (d["par"], d["mid_fork"], d["line_forked"], d["zero_nl"], d["line_stage"], d["clear_nl"]) == (0, 0, 0, 1, 0, 0)
    e = plan(64, cus, has_points=0, grid_points_fused_ok=0)
    assert (e["par"], e["mid_fork"], e["point_stage"], e["line_stage"], e["lean_cells"], e["cells_ahead"]) == (0, 0, 0, 1, 0, 0)
    assert plan(64, cus, has_points=0, grid_points_fused_ok=0, lines_now=0)["clear_nl"] == 1


@pytest.mark.parametrize("cus", CUS)
def test_fused_cells_up_to_one_frame_per_cu(cus):
    a, b = plan(cus, cus), plan(cus + 1, cus)
    assert (a["lean_cells"], a["has_tail"], a["fused_cells"]) == (1, 1, 1)
    assert (b["lean_cells"], b["has_tail"], b["fused_cells"]) == (1, 1, 0)
    c = plan(1, cus, grid_points_fused_ok=0)   # the scan formulation: nothing fused
    assert (c["lean_cells"], c["has_tail"], c["fused_cells"], c["cells_ahead"]) == (0, 0, 0, 0)


@pytest.mark.parametrize("cus", CUS)
def test_lines_ahead_beyond_two_streams_per_cu_and_up_to_128_key_lines(cus):
    for B, la in ((2 * cus, 0), (2 * cus + 1, 1)):
        p = plan(B, cus)
        assert (p["mid_fork"], p["cells_ahead"], p["lines_ahead"], p["gate"]) == (1, 1, la, la), B
    B = 2 * cus + 1
    assert plan(B, cus, raw_max_lines=128)["lines_ahead"] == 1 and plan(B, cus, raw_max_lines=129)["lines_ahead"] == 0
    assert plan(B, cus, set_lines_cap_prev=128)["lines_ahead"] == 1 and plan(B, cus, set_lines_cap_prev=129)["lines_ahead"] == 0
    p = plan(B, cus, {"lines_ahead": 1}, raw_max_lines=129)   # forced wherever it is safe
    assert (p["lines_ahead"], p["gate"]) == (1, 1)


def test_lines_ahead_needs_the_mid_fork_too():
    """Eight CUs: 17 streams are more than two per CU but fewer than the 64 the mid fork (and the second copies) start at."""
    p = plan(17, 8)
    assert (p["mid_fork"], p["cells_ahead"], p["lines_ahead"], p["gate"]) == (0, 0, 0, 0)
    assert plan(65, 8)["lines_ahead"] == 1


@pytest.mark.parametrize("cus", CUS)
def test_line_fused_by_batch_size_and_line_count(cus):
    exp = {(15, 128): 1, (15, 129): 0, (16, 128): 1, (16, 129): 1}   # 129 lines: LDS for 192
    for (B, n), lf in exp.items():
        p = plan(B, cus, raw_max_lines=n)
        assert p["Mk"] == (128 if n == 128 else 192) and p["line_fused"] == lf and p["sched_line_fused"] == lf, (B, n)
    assert sp.load().sph_lsf_max_lines() == 512
    assert plan(16, cus, M=512)["line_fused"] == 1 and plan(16, cus, M=576)["line_fused"] == 0
    assert plan(16, cus, {"line_fused": 1}, M=576)["line_fused"] == 0
    assert plan(16, cus, lines_now=0)["line_fused"] == 0 and plan(16, cus, lines_now=0)["Mk"] == 0


def test_line_fused_lds_opt_in_is_lazy():
    """LDS per launch: Mk x 169 + 4 + Mk x (Mk / 32) x 4 bytes; the opt-in is asked above 48 KB only, and only when all else holds."""
    p = plan(16, 256, raw_max_lines=192)
    assert (p["Mk"], p["line_lds"], p["lds_asked"], p["line_fused"]) == (192, 192 * 169 + 4 + 192 * 6 * 4, 0, 1)   # 37060 bytes
    for fits in (True, False):
        p = plan(16, 256, raw_max_lines=256, lds_fits=fits)
        assert (p["Mk"], p["line_lds"], p["lds_asked"], p["lds_asked_bytes"]) == (256, 51460, 1, 51460)   # > 49152
        assert p["line_fused"] == (1 if fits else 0)
    p = plan(16, 256, M=512, raw_max_lines=300, lds_fits=False)
    assert (p["Mk"], p["line_lds"], p["lds_asked"], p["line_fused"]) == (320, 320 * 169 + 4 + 320 * 10 * 4, 1, 0)
    # not asked where the route is already decided against
    assert plan(16, 256, {"line_fused": 0}, raw_max_lines=256)["lds_asked"] == 0
    assert plan(15, 256, raw_max_lines=256)["lds_asked"] == 0
    assert plan(16, 256, M=576, raw_max_lines=256)["lds_asked"] == 0
    assert plan(16, 256, raw_max_lines=256, lines_now=0)["lds_asked"] == 0


@pytest.mark.parametrize("n,Mk", [(0, 64), (1, 64), (64, 64), (65, 128), (320, 320), (300, 320), (319, 320)])
def test_mk_rounds_the_slots_line_count_to_64_within_the_capacity(n, Mk):
    assert plan(16, 256, raw_max_lines=n)["Mk"] == Mk
    assert plan(16, 256, M=64, raw_max_lines=n)["Mk"] == 64


@pytest.mark.parametrize("cus", CUS)
def test_small_set_route_up_to_128_key_lines(cus):
    p = plan(16, cus, raw_max_lines=128)
    assert (p["points_route"], p["points_small_cap"], p["lines_route"], p["lines_small_cap"], p["match_lines_run"]) == (SMALL, 0, SMALL, 128, 1)
    p = plan(16, cus, raw_max_lines=129)
    assert (p["points_route"], p["lines_route"]) == (LAZY, LAZY)
    p = plan(16, cus, set_lines_cap_prev=192)   # the previous set was the bigger one
    assert (p["points_route"], p["lines_route"]) == (LAZY, LAZY)
    assert plan(16, cus, set_lines_cap_prev=128)["lines_small_cap"] == 128
    # the line stage skipped: the set of this step still holds the capacity of its last use
    p = plan(16, cus, lines_now=0, set_lines_cap_cur=192)
    assert (p["points_route"], p["match_lines_run"], p["clear_m12l"]) == (LAZY, 0, 1)
    p = plan(16, cus, lines_now=0, set_lines_cap_cur=64)
    assert (p["points_route"], p["match_lines_run"], p["clear_m12l"]) == (SMALL, 0, 1)
    assert plan(16, cus, lines_prev=0)["match_lines_run"] == 0 and plan(16, cus, lines_prev=0)["clear_m12l"] == 0
    # more rows than the small-set kernel takes
    p = plan(16, cus, K=576)
    assert (p["points_route"], p["lines_route"]) == (LAZY, SMALL)
    p = plan(16, cus, M=576)
    assert (p["points_route"], p["lines_route"]) == (SMALL, LAZY)
    # the first step tracks nothing
    p = plan(16, cus, track=0, frame_idx=0)
    assert (p["track"], p["match_lines_run"], p["inline_sync"], p["pose_flagged"], p["sched_pose_kernel"]) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("cus", CUS)
def test_both_directions_up_to_four_pairs_lazy_beyond_one_way_without_mutual(cus):
    kw = dict(raw_max_lines=200, K=2048)   # neither set takes the small-set route
    p = plan(4, cus, **kw)
    assert (p["points_route"], p["points_nseg_cap"], p["lines_route"], p["lines_nseg_cap"]) == (BOTH_DIRS, 4, BOTH_DIRS, 4)
    p = plan(5, cus, **kw)
    assert (p["points_route"], p["points_nseg_cap"], p["lines_route"], p["lines_nseg_cap"]) == (LAZY, 0, LAZY, 0)
    for B in (4, 5):
        p = plan(B, cus, best_lr_matches=0, **kw)
        assert (p["points_route"], p["lines_route"], p["points_nseg_cap"]) == (ONE_WAY, ONE_WAY, 0)
    p = plan(4, cus, best_lr_matches=0)   # the small-set kernel takes either
    assert (p["points_route"], p["lines_route"]) == (SMALL, SMALL)


@pytest.mark.parametrize("cus", CUS)
def test_inline_sync_up_to_16_streams(cus):
    a, b = plan(16, cus), plan(17, cus)
    assert (a["inline_sync"], a["join_signal"], a["lazy_eig"], a["fetch_by_pose"], a["fetch_copy"], a["inl_copy"]) == (1, 1, 1, 0, 0, 0)
    assert (b["inline_sync"], b["join_signal"], b["lazy_eig"], b["fetch_by_pose"], b["fetch_copy"], b["inl_copy"]) == (0, 0, 0, 0, 0, 0)
    c = plan(16, cus, lines_now=0)   # nothing to join
    assert (c["inline_sync"], c["join_signal"]) == (1, 0)


@pytest.mark.parametrize("cus", CUS)
def test_fetch_one_zero_copy_stream_against_two(cus):
    a = plan(1, cus, fetch=1)
    assert (a["inline_sync"], a["fetch_by_pose"], a["inl_zero_copy"], a["fetch_copy"], a["inl_copy"]) == (1, 1, 1, 0, 0)
    b = plan(2, cus, fetch=1)
    assert (b["inline_sync"], b["fetch_by_pose"], b["inl_zero_copy"], b["fetch_copy"], b["inl_copy"], b["join_signal"]) == (0, 0, 1, 1, 0, 0)
    c = plan(17, cus, fetch=1)
    assert (c["inline_sync"], c["fetch_by_pose"], c["inl_zero_copy"], c["fetch_copy"], c["inl_copy"]) == (0, 0, 0, 1, 1)
    d = plan(1, cus, fetch=1, zero_copy=0)
    assert (d["inline_sync"], d["fetch_by_pose"], d["inl_zero_copy"], d["fetch_copy"], d["inl_copy"], d["lazy_eig"]) == (0, 0, 0, 1, 1, 0)
    e = plan(1, cus, fetch=1, track=0, frame_idx=0)   # first step: the stereo match indices still leave, by the copy
    assert (e["fetch_by_pose"], e["fetch_copy"], e["inl_copy"]) == (0, 1, 0)


@pytest.mark.parametrize("cus", CUS)
def test_stage_timing_modes(cus):
    B = max(cus + 1, 64)
    exp = {(0, 0): (0, 1), (1, 1): (0, 0), (2, 1): (1, 1), (1, 0): (0, 1), (2, 0): (0, 1)}   # (mode, events obtained) -> light, cells_ahead
    for (mode, ev), (light, ca) in exp.items():
        p = plan(B, cus, timing=mode, timing_events=ev)
        assert (p["light"], p["cells_ahead"], p["sched_cells_ahead"]) == (light, ca, ca), (mode, ev)
    for (mode, ev), timed in {(0, 0): 0, (1, 1): 1, (2, 1): 1, (1, 0): 0}.items():
        p = plan(1, cus, timing=mode, timing_events=ev)
        # a timed point set takes the general launches (here, four pairs at most and no lazy switch... but timed: the lazy formulation)
        assert (p["inline_sync"], p["points_route"], p["lines_route"]) == ((0, LAZY, SMALL) if timed else (1, SMALL, SMALL)), (mode, ev)


# ---- every switch the step reads --------------------------------------------------------------------------------------------------

def test_switch_grid_tail():
    assert [plan(1, 256, sw)["has_tail"] for sw in ({}, {"grid_tail": 0}, {"grid_tail": 1})] == [1, 0, 1]
    assert plan(1, 256, {"grid_tail": 0})["lean_cells"] == 1


def test_switch_grid_cells():
    assert [plan(1, 256, sw)["fused_cells"] for sw in ({}, {"grid_cells": 0}, {"grid_cells": 1})] == [1, 0, 1]
    assert plan(257, 256, {"grid_cells": 1})["fused_cells"] == 0   # one frame per workgroup is what fits
    p = plan(64, 256, {"grid_cells": 0})   # its own launch for a batch: it may then be built ahead
    assert (p["fused_cells"], p["cells_ahead"]) == (0, 1)


def test_switch_cells_ahead():
    B = 2 * 256 + 11
    for sw, exp in (({}, (1, 1, 1)), ({"cells_ahead": 0}, (0, 0, 0)), ({"cells_ahead": 1}, (1, 1, 1))):
        p = plan(B, 256, sw)
        assert (p["cells_ahead"], p["lines_ahead"], p["gate"]) == exp, sw


def test_switch_lines_ahead():
    big, mid = 2 * 256 + 11, 257
    assert [plan(big, 256, sw)["lines_ahead"] for sw in ({}, {"lines_ahead": 0}, {"lines_ahead": 1})] == [1, 0, 1]
    assert plan(big, 256, {"lines_ahead": 0})["gate"] == 0
    assert [plan(mid, 256, sw)["lines_ahead"] for sw in ({}, {"lines_ahead": 0}, {"lines_ahead": 1})] == [0, 0, 1]
    # forced at a batch whose pose kernel publishes no start: ahead, but no gate to wait at
    p = plan(mid, 256, {"lines_ahead": 1}, history=(2, -2, 2))
    assert (p["lines_ahead"], p["gate"]) == (1, 0)
    # ... and never where it is not safe: no fork event recorded in the last step / the by-product fetch reads the first copy
    assert plan(big, 256, {"lines_ahead": 1}, history=(1, 2, 2))["lines_ahead"] == 0
    assert plan(big, 256, {"lines_ahead": 1}, fetch=1)["lines_ahead"] == 0
    assert plan(big, 256, {"lines_ahead": 1}, has_alt_m12l=0, pose_start_flag_ok=0)["lines_ahead"] == 0


def test_switch_line_fused():
    assert [plan(16, 256, sw)["line_fused"] for sw in ({}, {"line_fused": 0}, {"line_fused": 1})] == [1, 0, 1]
    assert [plan(1, 256, sw, raw_max_lines=192)["line_fused"] for sw in ({}, {"line_fused": 0}, {"line_fused": 1})] == [0, 0, 1]


def test_switch_match_small():
    assert [plan(16, 256, sw)["lines_route"] for sw in ({}, {"match_small": 0}, {"match_small": 1})] == [SMALL, LAZY, SMALL]
    assert [plan(16, 256, sw, raw_max_lines=192)["lines_route"] for sw in ({}, {"match_small": 0}, {"match_small": 1})] == [LAZY, LAZY, SMALL]
    assert plan(16, 256, {"match_small": 1}, raw_max_lines=192)["lines_small_cap"] == 192
    assert plan(16, 256, {"match_small": 0})["points_route"] == LAZY


def test_switch_match_lazy():
    kw = dict(raw_max_lines=200, K=2048)
    assert [plan(4, 256, sw, **kw)["points_route"] for sw in ({}, {"match_lazy": 1}, {"match_lazy": 0})] == [BOTH_DIRS, LAZY, BOTH_DIRS]
    assert [plan(4, 256, sw, **kw)["lines_route"] for sw in ({}, {"match_lazy": 1})] == [BOTH_DIRS, LAZY]


def test_switch_seq_inline():
    for sw, exp in (({}, (1, 1, 1)), ({"seq_inline": 0}, (0, 0, 0)), ({"seq_inline": 1}, (1, 1, 1))):
        p = plan(1, 256, sw)
        assert (p["inline_sync"], p["join_signal"], p["lazy_eig"]) == exp, sw
    p = plan(1, 256, {"seq_inline": 0}, fetch=1)
    assert (p["fetch_by_pose"], p["fetch_copy"], p["inl_zero_copy"]) == (0, 1, 1)


def test_switch_pose_kernel_through_the_capability_answers():
    a = plan(1, 256)
    assert (a["inline_sync"], a["lazy_eig"], a["pose_flagged"], a["sched_pose_kernel"], a["sched_pose_waves"]) == (1, 1, 0, 1, 0)
    b = plan(1, 256, {"pose_kernel": 4})
    assert (b["inline_sync"], b["lazy_eig"], b["pose_flagged"], b["sched_pose_kernel"], b["sched_pose_waves"]) == (0, 0, 0, 2, 4)
    c = plan(64, 256, {"pose_kernel": 4})   # a batch with the second copy: the batch kernel publishes its start
    assert (c["pose_flagged"], c["sched_pose_kernel"], c["sched_pose_waves"]) == (1, 2, 4)
    d = plan(600, 256, {"pose_kernel": 1})
    assert (d["pose_flagged"], d["sched_pose_kernel"], d["sched_pose_waves"]) == (0, 1, 0)
    assert [plan(B, 256)["sched_pose_kernel"] for B in (256, 257)] == [1, 2]
    assert [plan(B, 256)["sched_pose_waves"] for B in (512, 513)] == [4, 2]
    # the planner's own read of the switch: no lazy eigenvalues beside the batch kernel, whatever the helpers answered
    assert plan(1, 256, {"pose_kernel": 4}, pose_inline_sync_ok=1)["lazy_eig"] == 0


# ---- a sequence through plan_step + commit ---------------------------------------------------------------------------------------

SEQ_CUS = [256, 160]   # 2 x CUs + 11 streams must be more than the 256 frame pairs the latency pose kernel takes: only the batch kernel publishes its start


def run_sequence(cus, steps=5, fetch=0, skip_lines_in=()):
    B = 2 * cus + 11
    hist, plans = (-2, -2, -2), []
    cap = [0, 0, 0]   # set_lines_cap of the three sets, kept as the enqueue side keeps it
    for k in range(steps):
        lines_now = 0 if k in skip_lines_in else 1
        cur, prev = k % 3, (k + 2) % 3
        f = facts(B, cus, frame_idx=k, track=k > 0, lines_now=lines_now, lines_prev=1 if (k > 0 and k - 1 not in skip_lines_in) else 0,
                  raw_max_lines=60, set_lines_cap_prev=cap[prev], set_lines_cap_cur=cap[cur], fetch=fetch)
        p, hist = sp.plan(f, None, hist, True, commit=True)
        if lines_now:
            cap[cur] = p["Mk"]
        plans.append(p)
    return plans, hist


@pytest.mark.parametrize("cus", SEQ_CUS)
def test_sequence_runs_ahead_from_the_third_step(cus):
    plans, hist = run_sequence(cus)
    assert [p["lines_ahead"] for p in plans] == [0, 0, 1, 1, 1]
    assert [p["gate"] for p in plans] == [0, 0, 1, 1, 1]
    assert [p["cells_ahead"] for p in plans] == [0, 1, 1, 1, 1]
    assert [p["use_alt_m12l"] for p in plans] == [0, 1, 0, 1, 0]   # the copy of the match indices alternates with the step
    assert [p["pose_flagged"] for p in plans] == [0, 1, 1, 1, 1]
    assert [p["sched_pose_waves"] for p in plans] == [0, 2, 2, 2, 2]
    assert [p["mid_fork"] for p in plans] == [1] * 5 and [p["line_fused"] for p in plans] == [1] * 5
    assert hist == (4, 4, 4)


def test_sequence_behind_the_latency_pose_kernel_stays_in_its_step():
    """40 CUs: 91 streams are more than two per CU, but their pose kernel is the latency kernel, which publishes no start."""
    plans, hist = run_sequence(40)
    assert [p["pose_flagged"] for p in plans] == [0] * 5 and [p["sched_pose_kernel"] for p in plans] == [0, 1, 1, 1, 1]
    assert [p["lines_ahead"] for p in plans] == [0] * 5 and [p["gate"] for p in plans] == [0] * 5
    assert [p["cells_ahead"] for p in plans] == [0, 1, 1, 1, 1]
    assert hist == (4, -2, 4)


@pytest.mark.parametrize("cus", SEQ_CUS)
def test_sequence_with_fetch_never_runs_ahead(cus):
    plans, _ = run_sequence(cus, fetch=1)
    assert [p["lines_ahead"] for p in plans] == [0] * 5 and [p["gate"] for p in plans] == [0] * 5
    assert [p["use_alt_m12l"] for p in plans] == [0] * 5
    assert [p["cells_ahead"] for p in plans] == [0, 1, 1, 1, 1]
    assert [p["pose_flagged"] for p in plans] == [0, 1, 1, 1, 1]


@pytest.mark.parametrize("cus", SEQ_CUS)
def test_sequence_line_stage_skipped_once(cus):
    """No key-lines in step 3: nothing forks there, so step 4 neither builds its grid ahead nor runs its key-line stage ahead; step 5 may
    build the grid ahead again, step 6 is the first to run ahead again."""
    plans, _ = run_sequence(cus, steps=7, skip_lines_in=(3,))
    assert [p["mid_fork"] for p in plans] == [1, 1, 1, 0, 1, 1, 1]
    assert [p["cells_ahead"] for p in plans] == [0, 1, 1, 0, 0, 1, 1]
    assert [p["lines_ahead"] for p in plans] == [0, 0, 1, 0, 0, 1, 1]
    assert [p["gate"] for p in plans] == [0, 0, 1, 0, 0, 1, 1]
    assert [p["clear_m12l"] for p in plans] == [0, 0, 0, 1, 0, 0, 0]
    assert [p["match_lines_run"] for p in plans] == [0, 1, 1, 0, 0, 1, 1]


# ---- invariants over the whole product of a coarse grid of facts ---------------------------------------------------------------

def test_invariants_over_a_grid_of_facts():
    """The conditions the comments of step_plan.h give as the reason each overlap is safe, on every plan of the grid."""
    F = 3   # frame_idx
    histories = [(-2, -2, -2), (F - 1, F - 1, F - 1), (F - 2, F - 2, F - 2), (F - 1, -2, F - 1), (F - 1, F - 1, -2), (-2, F - 1, F - 1)]
    buffers = [None, (1, 0), (0, 1)]   # as stvo_seq_create gives them, or (second copy of the match indices, of the grid buffers)
    switches = [{}, {"lines_ahead": 1}, {"lines_ahead": 1, "grid_cells": 0}, {"pose_kernel": 4, "lines_ahead": 1}]
    seen = dict.fromkeys(("gate", "lines_ahead", "cells_ahead", "mid_fork", "has_tail", "fused_cells", "inline_sync", "fetch_by_pose", "pose_flagged"), 0)
    n = 0
    for cus in (256, 8):
        Bs = sorted({1, 16, 17, 64, cus, cus + 1, 2 * cus + 1, 2 * cus + 64})
        for B, (lines_now, nl), fetch, (mode, ev), hist, buf, sw in itertools.product(
                Bs, ((0, 40), (1, 40), (1, 200)), (0, 1), ((0, 0), (1, 1), (2, 1)), histories, buffers, switches):
            kw = dict(lines_now=lines_now, raw_max_lines=nl, fetch=fetch, timing=mode, timing_events=ev)
            if buf is not None:
                kw.update(has_alt_m12l=buf[0], cells_differ=buf[1])
            f = facts(B, cus, F, sw, **kw)
            p = sp.plan(f, sw, hist)[0]
            n += 1
            for a, b in (("gate", "lines_ahead"), ("lines_ahead", "cells_ahead"), ("cells_ahead", "mid_fork"), ("mid_fork", "par"),
                         ("has_tail", "lean_cells"), ("fused_cells", "lean_cells"), ("fetch_by_pose", "inline_sync")):
                assert not p[a] or p[b], (a, b, f, sw, hist)
            if p["lines_ahead"]:
                assert f["has_alt_m12l"] and not f["fetch"] and hist[0] == F - 1, (f, sw, hist)
            if p["gate"]:
                assert hist[1] == F - 1, (f, sw, hist)
            if p["cells_ahead"]:
                assert f["cells_differ"] and hist[2] == F - 1 and not p["fused_cells"], (f, sw, hist)
            if p["fused_cells"]:
                assert B <= cus, (f, sw)
            if p["inline_sync"]:
                assert B <= 16 and not (mode and ev), (f, sw)
            if p["pose_flagged"]:
                assert f["has_alt_m12l"], (f, sw)
            batch = f["pose_batch_kernel_selected"]
            sched = dict(pose_kernel=2 if batch else 1, pose_waves=f["pose2p_waves_per_pair"] if batch else 0, fused_cells=p["fused_cells"],
                         cells_ahead=p["cells_ahead"], lines_ahead=p["lines_ahead"], gate=p["gate"], mid_fork=p["mid_fork"], line_fused=p["line_fused"])
            assert {k: p["sched_" + k] for k in sp.SCHEDULE} == sched, (f, sw, hist)
            for k in seen:
                seen[k] += p[k]
    assert n > 3000 and all(seen.values()), (n, seen)   # every antecedent occurs: none of the implications holds vacuously
