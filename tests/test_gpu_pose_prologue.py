"""The prologue of the batch pose kernels (pose_kernel2p.hip) at the ownership edges of a workgroup: counts, match indices and records
are fetched in three round trips, from addresses clamped to the pair's slot, and validity is applied where a value is consumed — so
what must be shown is that a slot past the count, an index of -1, an absent array and an empty pair never reach a result.

pose2c_kernel (compact records) is reached through the device-resident pipeline only (capi.Sequences, as tests/test_gpu_pose_edges.py
and test_gpu_seq.py reach it), forced for these few streams with STVO_POSE_KERNEL=4 on both wave counts.  The frames are built so that
the stereo association keeps EXACTLY the wanted number of points and lines (`trimmed`), in the order of the left rows:
  * counts: n_prev_pts 0, 1, 2, 127, 128, 129, 2047, 2048 (a 128-thread block with 16 slots per thread; 2048 = max_pts) beside
    n_prev_lines 0, 1, 127, 128, 129, 192 (= max_lines: the pipeline rounds its key-line capacity up to 64, never to 0), 8 pairs per launch;
  * match patterns, 6 pairs per launch: every index -1; exactly one point match, in the last owned slot (row 2047); exactly one line
    match, in the last owned line slot (row 191); one match each in the first and the last row; natural matches that point at row 0
    and at the last current row; a full pair whose current frame has no key-lines.
What the pipeline cannot reach for pose2c: it always hands over match arrays and never initial-inlier flags, and max_lines is never 0.
Those forms run on pose2p_kernel (the same prologue rule) through Context.optimize_pose — no match arrays, initial-inlier flags with
zeros on matched rows in the first and last owned slots — and with no key-line arrays at all.

Expected values are the oracle's (pipeline_ref's plumbing, oracle/stvo_oracle.c's numbers) with the tolerances of run_and_compare /
check_pose on the pose; status, path, iteration counts, match indices, inlier counts and masks are exact.  Pairs with fewer features
than the optimiser accepts must report the oracle's refusal.  test_cases_are_what_they_claim checks on the CPU that every case is
what its name says and that the oracle returns a defined result for it.

As a script (`python tests/test_gpu_pose_prologue.py DIR`) it writes every output array of the pose2c launches into DIR, one .npy each:
run once per build (STVO_LIB) to compare two builds bit for bit."""
import os
import sys

if __name__ == "__main__":   # (under pytest tests/conftest.py has done this)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stvo-pl_amd", "python"))

import numpy as np
import pytest

import np_model
import pipeline_ref
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_pose import check_pose

CAM = synth.KITTI_CAM
MAX_KP, MAX_KL = 2048, 192
PT_COUNTS = [0, 1, 2, 127, 128, 129, 2047, 2048]
LN_COUNTS = [0, 1, 127, 128, 129, 192, 128, 0]
P_KEYS = ("kp_l", "oct_l", "desc_l")
L_KEYS = ("kl_l", "ang_l", "oct_ll", "ldesc_l")


def trimmed(oracle, fr, mp, n_pts, n_lines):
    """fr with exactly n_pts stereo points and n_lines stereo lines: the first of those the oracle's association keeps, left row i
    beside its right partner in row i"""
    cols, rows = CAM["width"], CAM["height"]
    out = dict(fr)
    sp = oracle.stereo_points(fr["kp_l"], fr["oct_l"], fr["desc_l"], fr["kp_r"], fr["desc_r"], cols, rows, CAM, mp)
    L = np.asarray(sp["src_idx"][:n_pts], np.int64)
    assert len(L) == n_pts
    R = np.asarray(sp["m12_raw"], np.int64)[L]
    out.update({k: np.ascontiguousarray(fr[k][L]) for k in P_KEYS})
    out.update(kp_r=np.ascontiguousarray(fr["kp_r"][R]), desc_r=np.ascontiguousarray(fr["desc_r"][R]))
    sl = oracle.stereo_lines(fr["kl_l"], fr["ang_l"], fr["oct_ll"], fr["ldesc_l"], fr["kl_r"], fr["ldesc_r"], cols, rows, CAM, mp)
    L = np.asarray(sl["src_idx"][:n_lines], np.int64)
    assert len(L) == n_lines
    R = np.asarray(sl["m12_raw"], np.int64)[L]
    out.update({k: np.ascontiguousarray(fr[k][L]) for k in L_KEYS})
    out.update(kl_r=np.ascontiguousarray(fr["kl_r"][R]), ldesc_r=np.ascontiguousarray(fr["ldesc_r"][R]))
    return out


def redescribed(fr, rng, points=None, lines=None):
    """fr with fresh descriptors (nothing of the previous frame matches them), except rows {row: descriptor}"""
    out = dict(fr)
    if points is not None:
        d = synth.random_desc(rng, len(fr["desc_l"]))
        for row, desc in points.items():
            d[row] = desc
        out.update(desc_l=d, desc_r=d.copy())
    if lines is not None:
        d = synth.random_desc(rng, len(fr["ldesc_l"]))
        for row, desc in lines.items():
            d[row] = desc
        out.update(ldesc_l=d, ldesc_r=d.copy())
    return out


def ends_matched(oracle, f0, f1, mp, op):
    """f1 with its rows reordered (left and right alike) so that row 0 and the last row of points and of lines are match targets of f0"""
    ref = reference(oracle, f0, f1, mp, op)
    out = dict(f1)
    for m12, keys in ((ref["m12p"], P_KEYS + ("kp_r", "desc_r")), (ref["m12l"], L_KEYS + ("kl_r", "ldesc_r"))):
        hit = np.unique(m12[m12 >= 0])
        rest = [i for i in range(len(f1[keys[0]])) if i not in (hit[0], hit[-1])]
        perm = np.array([hit[0]] + rest + [hit[-1]], np.int64)
        out.update({k: np.ascontiguousarray(f1[k][perm]) for k in keys})
    return out


def reference(oracle, f0, f1, mp, op):
    """one tracked pair as pipeline_ref.run_sequence states it, keeping what that loop drops: the match indices and the rows behind the records"""
    prev, curr = (pipeline_ref.stereo_frame(oracle, f, CAM, mp, True, True) for f in (f0, f1))
    z3, z2 = np.zeros((0, 3)), np.zeros((0, 2))
    rec = dict(P=z3, pl_obs=z2, sigma2p=np.zeros(0), inlier_p=np.zeros(0, np.int32), sP=z3, eP=z3, le_obs=z3, spl=z2, epl=z2,
               sigma2l=np.zeros(0), inlier_l=np.zeros(0, np.int32))
    m12p, m12l = -np.ones(len(prev["P"]), np.int32), -np.ones(len(prev["sP"]), np.int32)
    if len(prev["P"]) and len(curr["P"]):
        m12p, _ = oracle.match(prev["pdesc"], curr["pdesc"], mp.min_ratio_12_p, mp.best_lr_matches)
        sel = np.nonzero(m12p >= 0)[0]
        rec.update(P=prev["P"][sel], pl_obs=curr["pl"][m12p[sel]], sigma2p=prev["sigma2p"][sel], inlier_p=np.ones(len(sel), np.int32))
    if len(prev["sP"]) and len(curr["sP"]):
        m12l, _ = oracle.match(prev["ldesc"], curr["ldesc"], mp.min_ratio_12_l, mp.best_lr_matches)
        sel = np.nonzero(m12l >= 0)[0]
        rec.update(sP=prev["sP"][sel], eP=prev["eP"][sel], le_obs=curr["le"][m12l[sel]], spl=prev["spl"][sel], epl=prev["epl"][sel],
                   sigma2l=pipeline_ref.matched_line_sigma2(prev["sigma2l"][sel], prev["llevel"][sel], mp.lsd_scale),
                   inlier_l=np.ones(len(sel), np.int32))
    out = oracle.optimize_pose(np.eye(4), CAM, op, rec)
    return dict(n_prev=(len(prev["P"]), len(prev["sP"])), n_curr=(len(curr["P"]), len(curr["sP"])), m12p=np.asarray(m12p), m12l=np.asarray(m12l),
                out=out, rows_in_order=np.array_equal(prev["pdesc"], f0["desc_l"]) and np.array_equal(prev["ldesc"], f0["ldesc_l"]))


_LAUNCHES = {}


def launches(oracle):
    """{name: [stream, ...]}, stream = dict(name, frames=[f0, f1], ref=reference(...)); built once"""
    if _LAUNCHES:
        return _LAUNCHES
    mp, op = match_params("kitti"), opt_params("kitti")

    def base(seed):
        f0, f1 = synth.make_stereo_sequence(seed, n_frames=2, n_pts=2300, n_lines=250, cam=CAM, distract=0.0)
        return f0, trimmed(oracle, f1, mp, MAX_KP, MAX_KL)

    def stream(name, f0, f1):
        return dict(name=name, frames=[f0, f1], ref=reference(oracle, f0, f1, mp, op))

    counts = []
    for b, (n_p, n_l) in enumerate(zip(PT_COUNTS, LN_COUNTS)):
        f0, f1 = base(4100 + b)
        counts.append(stream("counts-%d-%d" % (n_p, n_l), trimmed(oracle, f0, mp, n_p, n_l), f1))
    rng = np.random.default_rng(4200)
    f0, f1 = base(4201)
    full = trimmed(oracle, f0, mp, MAX_KP, MAX_KL)
    odd = trimmed(oracle, f0, mp, MAX_KP - 1, 129)
    z4, zd = np.zeros((0, 4), np.float32), np.zeros((0, 32), np.uint8)
    patterns = [
        stream("none", full, redescribed(f1, rng, points={}, lines={})),
        stream("one-point-last-slot", full, redescribed(f1, rng, points={5: full["desc_l"][MAX_KP - 1]}, lines={})),
        stream("one-line-last-slot", full, redescribed(f1, rng, lines={7: full["ldesc_l"][MAX_KL - 1]})),
        stream("first-and-last-rows", odd, redescribed(f1, rng, points={MAX_KP - 1: odd["desc_l"][0], 0: odd["desc_l"][MAX_KP - 2]},
                                                       lines={MAX_KL - 1: odd["ldesc_l"][0], 0: odd["ldesc_l"][128]})),
        stream("natural", full, ends_matched(oracle, full, f1, mp, op)),
        stream("no-current-lines", full, dict(f1, kl_r=z4, ldesc_r=zd)),
    ]
    _LAUNCHES.update(counts=counts, patterns=patterns)
    return _LAUNCHES


def test_cases_are_what_they_claim(oracle):
    """CPU: the oracle's association keeps exactly the wanted rows in the order of the left rows, the match patterns are the named ones,
    and optimizePose returns a defined result (a pose or a refusal, finite either way) for every pair."""
    L = launches(oracle)
    for s, n_p, n_l in zip(L["counts"], PT_COUNTS, LN_COUNTS):
        r = s["ref"]
        assert r["n_prev"] == (n_p, n_l) and r["n_curr"] == (MAX_KP, MAX_KL) and r["rows_in_order"], s["name"]
        assert (r["out"]["status"] == 0) == (n_p + n_l > 2), (s["name"], r["out"]["status"])   # 0 + 0 and 1 + 1 features are refused
        assert 2 * (r["m12p"] >= 0).sum() > n_p - 2 and 2 * (r["m12l"] >= 0).sum() > n_l - 2, s["name"]   # most rows are matched
    p = {s["name"]: s["ref"] for s in L["patterns"]}
    for name, r in p.items():
        assert r["rows_in_order"] and np.all(np.isfinite(r["out"]["T"])), name
    hits = lambda m: {int(i): int(m[i]) for i in np.nonzero(m >= 0)[0]}
    assert not hits(p["none"]["m12p"]) and not hits(p["none"]["m12l"]) and p["none"]["out"]["status"] != 0
    assert hits(p["one-point-last-slot"]["m12p"]) == {MAX_KP - 1: 5} and not hits(p["one-point-last-slot"]["m12l"])
    assert hits(p["one-line-last-slot"]["m12l"]) == {MAX_KL - 1: 7} and p["one-line-last-slot"]["out"]["status"] == 0
    assert hits(p["first-and-last-rows"]["m12p"]) == {0: MAX_KP - 1, MAX_KP - 2: 0}
    assert hits(p["first-and-last-rows"]["m12l"]) == {0: MAX_KL - 1, 128: 0}
    nat = p["natural"]
    assert nat["out"]["status"] == 0 and {0, MAX_KP - 1} <= set(nat["m12p"].tolist()) and {0, MAX_KL - 1} <= set(nat["m12l"].tolist())
    assert nat["out"]["n_inliers_pt"] < (nat["m12p"] >= 0).sum()   # outliers are cut: the records are read back
    assert p["no-current-lines"]["n_curr"] == (MAX_KP, 0) and p["no-current-lines"]["out"]["status"] == 0


def run_launch(streams, nw, set_switches):
    """both frames of every stream through one pipeline: what stvo_seq_read and the fetch calls return for the tracked pair"""
    from stvo_amd import capi
    set_switches({"STVO_POSE_KERNEL": "4", "STVO_POSE2P_NW": nw})
    B = len(streams)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    dev = capi.Sequences(ctx, B, MAX_KP, MAX_KL, CAM, match_params("kitti"), opt_params("kitti"))
    try:
        dev.enable_fetch(True)
        _, counts0 = dev.push([s["frames"][0] for s in streams])
        res, counts1 = dev.push([s["frames"][1] for s in streams])
        _, _, m_p, m_l = dev.fetch_matches()
        ip, il = dev.fetch_inliers()
        return dict(res=res.copy(), counts0=counts0.copy(), counts1=counts1.copy(), m_p=m_p.copy(), m_l=m_l.copy(), ip=ip.copy(), il=il.copy())
    finally:
        dev.close()
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nw", ["2", "4"])
@pytest.mark.parametrize("launch", ["counts", "patterns"])
def test_pose2c_prologue_edges_vs_oracle(oracle, switches, launch, nw):
    streams = launches(oracle)[launch]
    assert 3 <= len(streams) <= 9
    got = run_launch(streams, nw, switches)
    for b, s in enumerate(streams):
        ref, o, r, name = s["ref"], s["ref"]["out"], got["res"][b], s["name"]
        n_p, n_l = ref["n_prev"]
        assert tuple(got["counts0"][b, :2]) == ref["n_prev"] and tuple(got["counts1"][b, :2]) == ref["n_curr"], name   # stereo points, stereo lines
        assert np.array_equal(got["m_p"][b, :n_p], ref["m12p"]) and np.array_equal(got["m_l"][b, :n_l], ref["m12l"]), name
        sel_p, sel_l = np.nonzero(ref["m12p"] >= 0)[0], np.nonzero(ref["m12l"] >= 0)[0]
        assert r["n_matched_pt"] == len(sel_p) and r["n_matched_ls"] == len(sel_l), name
        assert r["status"] == o["status"] and r["path"] == o["path"] and tuple(r["iters"]) == o["iters"], (name, r["status"], o["status"])
        assert r["n_inliers_pt"] == o["n_inliers_pt"] and r["n_inliers_ls"] == o["n_inliers_ls"], name
        e = -np.ones(n_p, np.int32); e[sel_p] = o["inlier_p"]
        assert np.array_equal(got["ip"][b, :n_p], e) and np.all(got["ip"][b, n_p:] == -1), name
        e = -np.ones(n_l, np.int32); e[sel_l] = o["inlier_l"]
        assert np.array_equal(got["il"][b, :n_l], e) and np.all(got["il"][b, n_l:] == -1), name
        T = r["T"].reshape(4, 4)
        assert np_model.rot_angle(T[:3, :3], o["T"][:3, :3]) < 1e-4 and np.linalg.norm(T[:3, 3] - o["T"][:3, 3]) < 1e-3, name
        assert np.allclose(T, o["T"], atol=1e-8) and np.isclose(r["err"], o["err"], rtol=1e-8), name
        assert np.allclose(r["cov"].reshape(6, 6), o["cov"], rtol=1e-6, atol=1e-12), name


_FLAG_REFS = {}


def flagged_records(oracle, with_lines):
    """129 points (+ 129 key-lines): the last row is the one a second slot of a thread holds; zero initial-inlier flags on matched rows
    in the first and last owned slots.  (Context.optimize_pose hands over records in order: no match arrays.)"""
    if with_lines not in _FLAG_REFS:
        rec = synth.make_matched_records(4300 + with_lines, n_pts=129, n_lines=129 if with_lines else 0)
        rec["inlier_p"] = rec["inlier_p"].copy(); rec["inlier_p"][[0, 127, 128]] = 0
        if with_lines:
            rec["inlier_l"] = rec["inlier_l"].copy(); rec["inlier_l"][[0, 127, 128]] = 0
        _FLAG_REFS[with_lines] = (rec, oracle.optimize_pose(np.eye(4), CAM, opt_params("kitti"), rec))
    return _FLAG_REFS[with_lines]


def test_flagged_records_are_defined_for_the_oracle(oracle):
    for with_lines in (0, 1):
        rec, ref = flagged_records(oracle, with_lines)
        assert ref["status"] == 0 and ref["n_inliers_pt"] < 126


@pytest.mark.gpu
@pytest.mark.parametrize("with_lines", [0, 1])
@pytest.mark.parametrize("nw", ["2", "4"])
def test_pose2p_initial_inlier_flags_and_absent_arrays(hip, oracle, switches, nw, with_lines):
    switches({"STVO_POSE_KERNEL": "4", "STVO_POSE2P_NW": nw})
    rec, ref = flagged_records(oracle, with_lines)
    check_pose(hip.optimize_pose(np.eye(4), CAM, opt_params("kitti"), rec), ref)


if __name__ == "__main__":
    import oracle_lib
    from stvo_amd import capi

    def reparse(env):
        os.environ.update(env)
        capi.load().stvo_debug_reparse_env()
    os.makedirs(sys.argv[1], exist_ok=True)
    for launch, streams in launches(oracle_lib.load()).items():
        for nw in ("2", "4"):
            for k, v in run_launch(streams, nw, reparse).items():
                np.save(os.path.join(sys.argv[1], "%s_nw%s_%s.npy" % (launch, nw, k)), np.frombuffer(np.ascontiguousarray(v).tobytes(), np.uint8))
