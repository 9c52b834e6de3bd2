"""The two key-line matchers of the device pipeline at their edges: line_stereo_fused_kernel (stereo_assoc_kernels.hip; the stereo association
of the key-lines in one workgroup per frame) and match_small_kernel (match_kernels.hip; the frame-to-frame match of one pair in
one workgroup), and the general kernels that take their place on the other routes.  The case frames are those of
tests/line_match_cases.py, which tests/test_line_match_host.py has shown to be fair and to hit their edges on the CPU.  Every
comparison is exact integer equality of raw match indices with the oracle AND with the numpy model; there is no tolerance here.

Stereo cases are judged on fetch_matches()[1] of the first step.  Frame-to-frame cases on fetch_matches()[3] of the tracked step,
the expectation computed on the rows that debug_stereo read back from the device after either step, so the matcher is judged on
what it received.  last_schedule has no slot for the f2f route: the expected one is computed by the planner itself, built for the
host (tests/step_plan_host_lib.py), from the facts the test sets up, and must be the route the case is after."""
import numpy as np
import pytest

import line_match_cases as cases
import np_model
import step_plan_host_lib as sp
from stvo_amd.ctypes_types import opt_params

pytestmark = pytest.mark.gpu

STEREO = [cs["name"] for cs in cases.stereo_sets()]
F2F = [cs["name"] for cs in cases.f2f_sets()]


def lines_cap(M, frames):
    """StepPlan::Mk: the LDS of the fused kernel is sized for the most key-lines of one image in the slot, in steps of 64"""
    n = max(max(len(f["kl_l"]), len(f["kl_r"])) for f in frames)
    return min(M, max(64, (n + 63) & ~63))


def run_stereo(oracle, cs, switches, env, fused):
    from stvo_amd import capi
    switches(env)
    res = cases.stereo_results(oracle, cs)
    frames = [cf["frame"] for cf in cs["frames"]]
    B, M = len(frames), cs["M"]
    ctx = capi.Context(device_id=0, max_rows=512, max_batch=B)
    dev = capi.Sequences(ctx, B, cs["K"], M, cs["cam"], cs["mp"], opt_params("kitti"))
    try:
        dev.enable_fetch(True)
        _, counts = dev.push(frames)
        assert dev.last_schedule()["line_fused"] == fused, (cs["name"], env, "Mk", lines_cap(M, frames), "B", B)
        ms_l = dev.fetch_matches()[1]
        for b, (cf, (ref, mdl, t)) in enumerate(zip(cs["frames"], res)):
            where = (cs["name"], cf["name"], "stream", b, env)
            nl = len(cf["frame"]["kl_l"])
            got = ms_l[b, :nl]
            bad = np.nonzero(got != ref)[0]
            assert len(bad) == 0, (where, "left rows", bad[:8], "device", got[bad[:8]], "oracle", ref[bad[:8]],
                                   "(best, second)", [(int(t["best"][i]), int(t["second"][i])) for i in bad[:8]])
            assert np.array_equal(got, mdl), where
            assert (ms_l[b, nl:] == -1).all(), (where, "rows beyond nl")
            assert counts[b, 1] == len(t["kept_ldesc"]), (where, "stereo lines", counts[b, 1], len(t["kept_ldesc"]))
            assert np.array_equal(dev.debug_stereo(b)["ldesc"], t["kept_ldesc"]), (where, "kept rows")
    finally:
        dev.close()
        ctx.close()


def default_fused(cs):
    """the rule of the route table: the fused kernel up to 128 key-lines per image, and for 16 streams or more"""
    return int(lines_cap(cs["M"], [cf["frame"] for cf in cs["frames"]]) <= 128 or len(cs["frames"]) >= 16)


@pytest.mark.parametrize("name", STEREO)
def test_stereo_lines_default_route(oracle, switches, name):
    cs = [s for s in cases.stereo_sets() if s["name"] == name][0]
    run_stereo(oracle, cs, switches, {}, default_fused(cs))


def test_stereo_default_routes_cover_the_table():
    d = {cs["name"]: default_fused(cs) for cs in cases.stereo_sets()}
    assert d["S1 windows"] == 1 and d["S6 counts M=64"] == 1 and d["S6 counts M=128"] == 1          # Mk <= 128
    assert d["S6 counts M=320"] == 0 and d["S6 counts M=512"] == 0                                  # the general matcher
    big = [cs for cs in cases.stereo_sets() if cs["name"] == "S6 counts M=320, 16 streams"][0]
    assert len(big["frames"]) >= 16 and lines_cap(320, [cf["frame"] for cf in big["frames"]]) > 128 and d[big["name"]] == 1


@pytest.mark.parametrize("name", STEREO)
def test_stereo_lines_general_matcher(oracle, switches, name):
    cs = [s for s in cases.stereo_sets() if s["name"] == name][0]
    run_stereo(oracle, cs, switches, {"STVO_LINE_FUSED": "0"}, 0)


@pytest.mark.parametrize("name", [n for n in STEREO if "M=320" in n or "M=512" in n])
def test_stereo_lines_fused_at_320_and_512(oracle, switches, name):
    cs = [s for s in cases.stereo_sets() if s["name"] == name][0]
    run_stereo(oracle, cs, switches, {"STVO_LINE_FUSED": "1"}, 1)


@pytest.mark.parametrize("M", [320, 512])
def test_stereo_edges_in_a_larger_capacity(oracle, switches, M):
    """the planned edges with max_keylines above what the frames hold: the LDS arrays (Mk = 64 or 128) are narrower than the stride"""
    for name in ("S1 windows", "S3+S4 kitti"):
        cs = dict([s for s in cases.stereo_sets() if s["name"] == name][0], M=M)
        run_stereo(oracle, cs, switches, {}, 1)


# ---- frame to frame ------------------------------------------------------------------------------------------------------------------
def expected_route(cs, B, env):
    import torch
    M, K = cs["M"], cs["K"]
    sw = {k: int(env[e]) for k, e in (("match_small", "STVO_MATCH_SMALL"), ("match_lazy", "STVO_MATCH_LAZY")) if e in env}
    facts = dict(B=B, K=K, M=M, cus=torch.cuda.get_device_properties(0).multi_processor_count, has_points=1, has_lines=1,
                 best_lr_matches=int(cs["mp"].best_lr_matches), lines_now=1, lines_prev=1, track=1, frame_idx=1, raw_split=0,
                 raw_max_lines=max(max(len(f["kl_l"]), len(f["kl_r"])) for f in cs["steps"][1]),
                 set_lines_cap_prev=lines_cap(M, cs["steps"][0]), set_lines_cap_cur=0, st_dirty=1, fetch=1, zero_copy=B <= 16, timing=0,
                 timing_events=0, has_alt_m12l=B >= 64, cells_differ=B >= 64, grid_points_fused_ok=1, match_small_ok_K=0 < K <= 512,
                 match_small_ok_M=0 < M <= 512, pose_inline_sync_ok=1 <= B <= 16, pose_batch_kernel_selected=B > 256,
                 pose_start_flag_ok=B > 256, pose2p_waves_per_pair=0)
    p = sp.plan(facts, sw)[0]
    return p["lines_route"], p["lines_small_cap"]


def run_f2f(oracle, cs, switches, env, route, cap_below_stride=None):
    from stvo_amd import capi
    switches(env)
    op = opt_params("kitti")
    res = cases.f2f_results(oracle, cs, op)
    B, M, mp = len(cs["streams"]), cs["M"], cs["mp"]
    nnr, lr = float(mp.min_ratio_12_l), bool(mp.best_lr_matches)
    got_route, cap = expected_route(cs, B, env)
    assert got_route == route, (cs["name"], env, "B", B, "the planner's route", got_route, "the case is after", route)
    if cap_below_stride is not None:
        assert (cap < M) == cap_below_stride, (cs["name"], cap, M)
    ctx = capi.Context(device_id=0, max_rows=512, max_batch=B)
    dev = capi.Sequences(ctx, B, cs["K"], M, cs["cam"], mp, op)
    try:
        dev.enable_fetch(True)
        sets = []
        for step in (0, 1):
            out, counts = dev.push(cs["steps"][step])
            ms_l = dev.fetch_matches()[1]
            rows = []
            for b, r in enumerate(res):
                where = (cs["name"], cs["streams"][b].name, "stream", b, "step", step, env)
                nl = len(cs["steps"][step][b]["kl_l"])
                assert np.array_equal(ms_l[b, :nl], r["raw"][step]) and (ms_l[b, nl:] == -1).all(), (where, "stereo matches")
                assert counts[b, 1] == len(r["sets"][step]) and counts[b, 0] == r["n_pts"][step], (where, counts[b])
                rows.append(dev.debug_stereo(b)["ldesc"])
                assert np.array_equal(rows[-1], r["sets"][step]), (where, "the stereo set is not the planned one")
            sets.append(rows)
        m_l = dev.fetch_matches()[3]
        for b, r in enumerate(res):
            where = (cs["name"], cs["streams"][b].name, "stream", b, env)
            A, Bd = sets[0][b], sets[1][b]
            exp, n = oracle.match(A, Bd, nnr, int(lr))
            got = m_l[b, :len(A)]
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, (where, "query rows", bad[:8], "device", got[bad[:8]], "oracle", exp[bad[:8]])
            assert np.array_equal(got, np_model.match(A, Bd, nnr, lr)), where
            if len(A) and len(Bd):
                assert out[b]["n_matched_ls"] == n == int((exp >= 0).sum()), (where, out[b]["n_matched_ls"], n)
            else:
                assert out[b]["n_matched_ls"] == 0, where
            assert out[b]["status"] == r["ref"]["status"], (where, "status", out[b]["status"], r["ref"]["status"])
    finally:
        dev.close()
        ctx.close()


def fset(name):
    return [s for s in cases.f2f_sets() if s["name"] == name][0]


@pytest.mark.parametrize("name", [n for n in F2F if "M=" not in n])
def test_f2f_lines_small_default(oracle, switches, name):
    """max_keylines <= 128: match_small_kernel"""
    cs = fset(name)
    run_f2f(oracle, cs, switches, {}, sp.SMALL, cap_below_stride=lines_cap(128, cs["steps"][0] + cs["steps"][1]) < 128)


@pytest.mark.parametrize("name,below", [("F4 sizes M=320", True), ("F4 sizes M=512", False)])
def test_f2f_lines_small_with_a_cap(oracle, switches, name, below):
    """STVO_MATCH_SMALL=1 beyond 128 key-lines: the kernel's LDS is sized by a cap, below the stride (256 of 320) and at it (512)"""
    run_f2f(oracle, fset(name), switches, {"STVO_MATCH_SMALL": "1"}, sp.SMALL, cap_below_stride=below)


@pytest.mark.parametrize("name", [n for n in F2F if "off" not in n])
def test_f2f_lines_lazy_batches(oracle, switches, name):
    """STVO_MATCH_SMALL=0 with more than four streams: forward scan, plan, selective reverse scans"""
    cs = fset(name)
    assert len(cs["streams"]) > 4
    run_f2f(oracle, cs, switches, {"STVO_MATCH_SMALL": "0"}, sp.LAZY)


@pytest.mark.parametrize("name", ["F1-F3 edges, ratio 0.75", "F2 ratio 0.9", "F1 ratio 1.0", "F4 sizes",
                                  "F4 sizes M=320", "F4 sizes M=512"])
@pytest.mark.parametrize("env,route", [({"STVO_MATCH_SMALL": "0"}, sp.BOTH_DIRS), ({"STVO_MATCH_SMALL": "0", "STVO_MATCH_LAZY": "1"}, sp.LAZY)],
                         ids=["both-directions", "lazy"])
def test_f2f_lines_few_streams(oracle, switches, name, env, route):
    """up to four streams without the one-workgroup kernel: both directions in one launch, or the lazy formulation by its switch"""
    cs = fset(name)
    for a in range(0, len(cs["streams"]), 4):
        run_f2f(oracle, cases.f2f_chunk(cs, a, min(a + 4, len(cs["streams"]))), switches, env, route)


@pytest.mark.parametrize("name", [n for n in F2F if "off" in n])
def test_f2f_lines_one_way(oracle, switches, name):
    """best_lr_matches off on the general machinery: forward scan and ratio test only"""
    run_f2f(oracle, fset(name), switches, {"STVO_MATCH_SMALL": "0"}, sp.ONE_WAY)
