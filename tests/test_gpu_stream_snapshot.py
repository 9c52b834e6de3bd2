"""Export and import of single streams of the device pipeline (stvo_seq_export_streams / stvo_seq_import_streams, Sequences.export_streams /
import_streams, capi.snapshot_views).  Nothing in the reference corresponds to this; a continued frame is judged twice:
  (a) against the oracle chain of its sequence from frame 0 (pipeline_ref.run_sequence), with exactly the assertions and tolerances of
      tests/test_gpu_stream_control.py::check_tracked / compare_record, and its track records by tests/np_tracks.py where the by-product
      fetch that feeds it can be on;
  (b) byte for byte against an uninterrupted device run of the same sequence — results, counts, trajectory records and state, track
      records, key-frame headers and sets — when the continuing step took the same route (last_schedule equal).  Every such test first
      asserts that two uninterrupted runs agree byte for byte with each other.
The scenes, the capacities (512 / 64) and the cached oracle chains are those of tests/test_gpu_stream_control.py."""
import ctypes as C

import numpy as np
import pytest

import np_tracks
import test_gpu_stream_control as sc
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params

pytestmark = pytest.mark.gpu
RUN, RESTART, PARK = 0, 1, 2
CAM = sc.CAM
KF = sc.KF
INVALID, CAPACITY = -1, -4   # include/stvo_types.h: STVO_ERR_INVALID_ARG, STVO_ERR_CAPACITY
SET_KEYS = ("rc", "desc", "spl", "epl", "sP", "eP", "le", "s2l", "s2lm", "ldesc")
BATCH = {"STVO_POSE_KERNEL": "4"}


def open_dev(B, cfg, K=512, M=64, features=True, fetch=False, cam=CAM, max_rows=2048):
    """features: trajectory (key-frames as cfg says, the KF thresholds), tracks and key-frame sets; the motion model as cfg says."""
    from stvo_amd import capi
    ctx = capi.Context(device_id=0, max_rows=max_rows, max_batch=max(B, 1))
    try:
        dev = capi.Sequences(ctx, B, K, M, cam, cfg.mp, cfg.op)
    except Exception:
        ctx.close()
        raise
    if cfg.motion_model:
        dev.set_motion_model(True)
    if features:
        dev.set_trajectory(capi.traj_params("kitti", keyframes=cfg.keyframes, **KF), log_steps=2)
        dev.set_tracks(log_steps=2, keyframe_sets=True)
    if fetch:
        dev.enable_fetch(True)
    return ctx, dev


def close(ctx, dev):
    dev.close()
    ctx.close()


def observe(dev, res, counts, features=True, kf_streams=()):
    """Everything a step leaves that a caller can read, as bytes-comparable numpy values."""
    o = dict(res=res.copy(), counts=counts.copy(), sched=dev.last_schedule())
    if features:
        o["traj"] = dev.read_trajectory(1)
        o["state"] = dev.trajectory_state()
        o["pts"], o["lines"], o["cnt"] = (a[0] for a in dev.read_tracks(1))
        o["hdr"] = dev.keyframe_headers()
        o["kf"] = {b: dev.read_keyframe(b) for b in kf_streams}
    return o


def same_stream(got, b, ref, rb, where, frame_offset=0, first_own_step=None):
    """(b): stream b of observation `got` equals stream rb of observation `ref`, byte for byte.  A key-frame header's `frame` names a step
    of the pipeline that took the key-frame: verbatim when it was imported, shifted by frame_offset when the continuing pipeline took it
    (reference step >= first_own_step)."""
    assert got["res"][b].tobytes() == ref["res"][rb].tobytes(), where
    assert np.array_equal(got["counts"][b], ref["counts"][rb]), (where, got["counts"][b], ref["counts"][rb])
    if "state" not in got:
        return
    assert got["traj"].shape[0] == ref["traj"].shape[0] == 1 and got["traj"][0][b].tobytes() == ref["traj"][0][rb].tobytes(), where
    assert got["state"][b].tobytes() == ref["state"][rb].tobytes(), where
    n, nl = (int(v) for v in ref["cnt"][rb])
    assert tuple(got["cnt"][b]) == (n, nl), where
    assert got["pts"][b][:n].tobytes() == ref["pts"][rb][:n].tobytes() and got["lines"][b][:nl].tobytes() == ref["lines"][rb][:nl].tobytes(), where
    hg, hr = got["hdr"][b], ref["hdr"][rb]
    assert (hg["n_pts"], hg["n_lines"], hg["serial"]) == (hr["n_pts"], hr["n_lines"], hr["serial"]), (where, hg, hr)
    own = first_own_step is not None and hr["frame"] >= first_own_step
    assert hg["frame"] == hr["frame"] - (frame_offset if own else 0), (where, hg, hr, frame_offset)
    if b in got["kf"] and rb in ref["kf"]:
        for k in SET_KEYS:
            assert np.asarray(got["kf"][b][k]).tobytes() == np.asarray(ref["kf"][rb][k]).tobytes(), (where, k)


def judge_a(o, b, ref_out, where, keyframes):
    """(a): the frame against the oracle output of its sequence's chain."""
    sc.check_tracked(o["res"][b], o["counts"][b], ref_out, where)
    if "traj" in o:
        sc.compare_record(o["traj"][0][b], ref_out, keyframes=keyframes)


def run_plain(cfg, B, seqs, steps, features=True, K=512, M=64, kf_streams=(), fetch=False):
    """An uninterrupted run: seqs[b][t] pushed for t in `steps`; one observation per step."""
    ctx, dev = open_dev(B, cfg, K, M, features, fetch)
    try:
        out = []
        for t in steps:
            res, counts = dev.push([seqs[b][t] for b in range(B)])
            out.append(observe(dev, res, counts, features, kf_streams))
        return out
    finally:
        close(ctx, dev)


def assert_runs_agree(r1, r2, B, kf_streams=()):
    """The precondition of (b): two uninterrupted runs of the same input agree byte for byte."""
    for t, (x, y) in enumerate(zip(r1, r2)):
        assert x["sched"] == y["sched"], t
        for b in range(B):
            if t == 0 and "traj" in x:   # no trajectory record yet
                assert x["res"][b].tobytes() == y["res"][b].tobytes() and x["state"][b].tobytes() == y["state"][b].tobytes()
                continue
            same_stream(x, b, y, b, ("two plain runs", t, b))


def seeds_for(B, base):
    return [base + b % 8 for b in range(B)]


# ---- 1. blob content

def check_blob(capi, dev, blob, b, features):
    """The views of stream b's blob equal what the existing read calls report, and every other byte is zero."""
    v = capi.snapshot_views(blob)
    h, info = v["header"], dev.snapshot_info()
    assert (h["magic"], h["version"], h["bytes"], h["K"], h["M"], h["flags"]) == (capi.SNAP_MAGIC, capi.SNAP_VERSION, blob.size, info["K"], info["M"], info["flags"])
    assert (h["cols"], h["rows"]) == (CAM["width"], CAM["height"]) and h["cam"]["fx"] == CAM["fx"] and h["cam"]["b"] == CAM["b"]
    assert not blob[~v["live"]].any(), "a byte that is no valid row and no header field is not zero"
    return v


def test_blob_content(oracle):
    from stvo_amd import capi
    import torch
    cfg = sc.Cfg(1, True, True)
    B = 3
    seqs = [sc.sequence(s) for s in seeds_for(B, 4000)]
    ctx, dev = open_dev(B, cfg)
    try:
        info = dev.snapshot_info()
        assert info["flags"] == 31 and info["bytes"] == capi.snapshot_layout(512, 64, 31)["bytes"]
        # before the first step: an empty set and initial states
        early = dev.export_streams([0, 1, 2])
        init = dev.trajectory_state()
        for b in range(B):
            v = check_blob(capi, dev, early[b], b, True)
            assert v["header"]["n"] == 0 and v["header"]["nl"] == 0 and v["header"]["kf"].tobytes() == bytes(16)
            assert v["motion"][0].tolist() == np.eye(4).reshape(-1).tolist() and v["traj"][0].tobytes() == init[b].tobytes()
        for t in range(4):
            dev.push([seqs[b][t] for b in range(B)])
        st, hdr = dev.trajectory_state(), dev.keyframe_headers()
        pts, lines, cnt = (a[0] for a in dev.read_tracks(1))
        new_kf = dev.read_trajectory(1)[0]["new_kf"]
        blobs = dev.export_streams([0, 1, 2])
        assert blobs.shape == (3, info["bytes"])
        for b in range(B):
            v = check_blob(capi, dev, blobs[b], b, True)
            ds = dev.debug_stereo(b)
            assert (v["header"]["n"], v["header"]["nl"]) == (ds["n"], ds["nl"]) and ds["n"] > 100 and ds["nl"] > 5
            for k in SET_KEYS:
                assert v[k].tobytes() == np.asarray(ds[k]).tobytes(), (b, k)
            assert v["traj"][0].tobytes() == st[b].tobytes()
            assert v["header"]["kf"].tobytes() == hdr[b].tobytes()
            kf = dev.read_keyframe(b)
            for k in SET_KEYS:
                assert v["kf_" + k].tobytes() == np.asarray(kf[k]).tobytes(), (b, "kf", k)
            if not new_kf[b]:   # no key-frame in the last step: its record is also the state the next step propagates from
                assert v["tracks_p"].tobytes() == pts[b][:ds["n"]].tobytes() and v["tracks_l"].tobytes() == lines[b][:ds["nl"]].tobytes()
            else:
                want = np_tracks.fresh(ds["n"], 1)
                want["inlier"] = pts[b][:ds["n"]]["inlier"]
                assert v["tracks_p"].tobytes() == want.tobytes()
        assert any(hdr[b]["n_pts"] != dev.debug_stereo(b)["n"] for b in range(B))   # a key-frame set that is not the current set
        assert dev.export_streams([0, 1, 2]).tobytes() == blobs.tobytes()               # a function of the state
        assert dev.export_streams([2, 2, 0]).tobytes() == blobs[[2, 2, 0]].tobytes()    # any order, duplicates
        # the _dev form
        buf = torch.full((3 * info["bytes"] + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        dev.export_streams_dev([0, 1, 2], buf.data_ptr())
        ctx.synchronize()
        host = buf.cpu().numpy()
        assert host[:3 * info["bytes"]].tobytes() == blobs.tobytes() and (host[3 * info["bytes"]:] == 0x5A).all()
    finally:
        close(ctx, dev)
    # everything off: only the header and the stereo set exist
    cfg0 = sc.Cfg(1, False, False)
    ctx, dev = open_dev(B, cfg0, features=False)
    try:
        info = dev.snapshot_info()
        assert info["flags"] == 0 and info["bytes"] == 256 + 48 * 512 + 152 * 64
        for t in range(2):
            dev.push([seqs[b][t] for b in range(B)])
        blobs = dev.export_streams([0, 1, 2])
        for b in range(B):
            v = check_blob(capi, dev, blobs[b], b, False)
            ds = dev.debug_stereo(b)
            for k in SET_KEYS:
                assert v[k].tobytes() == np.asarray(ds[k]).tobytes(), (b, k)
            assert "motion" not in v and "traj" not in v and "tracks_p" not in v and "kf_rc" not in v
    finally:
        close(ctx, dev)


# ---- 2. restore into a fresh context and pipeline

@pytest.mark.parametrize("B,pose,has_lines", [(4, None, 1), (4, None, 0), (66, "4", 1)], ids=["latency-lines", "latency-points", "batch-B66-lines"])
def test_restore(oracle, switches, B, pose, has_lines):
    from stvo_amd import capi
    if pose:
        switches(BATCH)
    cfg = sc.Cfg(has_lines, True, True)
    seeds = seeds_for(B, 4100)
    seqs = [sc.sequence(s) for s in seeds]
    refs = [sc.chain(oracle, cfg, seqs[b], (seeds[b], 0, 6)) for b in range(B)]
    kfs = (0, B - 1)
    full = run_plain(cfg, B, seqs, range(6), kf_streams=kfs)
    assert_runs_agree(full, run_plain(cfg, B, seqs, range(6), kf_streams=kfs), B)
    want = capi.SCHED_POSE_BATCH if pose else capi.SCHED_POSE_LATENCY
    assert all(o["sched"]["pose_kernel"] == want for o in full[1:])
    ctx, dev = open_dev(B, cfg)
    try:
        for t in range(3):
            dev.push([seqs[b][t] for b in range(B)])
        blobs = dev.export_streams(range(B))
    finally:
        close(ctx, dev)      # the exporting pipeline and its context are gone
    ctx, dev = open_dev(B, cfg)
    try:
        dev.import_streams(range(B), blobs)
        with pytest.raises(capi.StvoError):
            dev.set_tracks(log_steps=2, keyframe_sets=True)   # refused after an import as after a step
        with pytest.raises(capi.StvoError):
            dev.set_trajectory(capi.traj_params("kitti", **KF), log_steps=2)
        assert dev.export_streams(range(B)).tobytes() == blobs.tobytes()   # the restored state is the exported state
        same_route = 0
        for t in range(3, 6):
            res, counts = dev.push([seqs[b][t] for b in range(B)])
            o = observe(dev, res, counts, kf_streams=kfs)
            assert o["sched"]["pose_kernel"] == want
            for b in range(B):
                judge_a(o, b, refs[b][t - 1], (t, b), True)
            if o["sched"] == full[t]["sched"]:
                same_route += 1
                for b in range(B):
                    same_stream(o, b, full[t], b, (t, b), frame_offset=2, first_own_step=3)
            else:
                print(f"[snapshot] restore B={B} step {t}: route differs from the uninterrupted run: {o['sched']} vs {full[t]['sched']}")
        assert same_route >= 2
    finally:
        close(ctx, dev)


def test_restore_track_records_follow_the_reference_rule(oracle):
    """(a) for the track records: tests/np_tracks.py, fed across the cut with what the two pipelines' by-product fetch reports, as
    tests/test_gpu_tracks.py::drive feeds it within one pipeline."""
    cfg = sc.Cfg(1, True, True)
    B = 3
    seqs = [sc.sequence(s) for s in seeds_for(B, 4100)]
    chains = [np_tracks.Stream() for _ in range(B)]

    def step(dev, t, first):
        res, counts = dev.push([seqs[b][t] for b in range(B)])
        m12p = m12l = inlp = inll = None
        if not first:
            _, _, m12p, m12l = dev.fetch_matches()
            inlp, inll = dev.fetch_inliers()
        new_kf = dev.read_trajectory(1)[0]["new_kf"] if not first else np.zeros(B, np.int32)
        pts, lines, cnt = (a[0] for a in dev.read_tracks(1))
        for b in range(B):
            w = chains[b].step(counts[b, :2], m12=(m12p[b], m12l[b]) if not first else (None, None),
                               inl=(inlp[b], inll[b]) if not first else (None, None), first=first, new_kf=int(new_kf[b]))
            n, nl = int(counts[b, 0]), int(counts[b, 1])
            assert pts[b, :n].tobytes() == w[0].tobytes() and lines[b, :nl].tobytes() == w[1].tobytes(), (t, b)
        return pts

    ctx, dev = open_dev(B, cfg, fetch=True)
    try:
        for t in range(3):
            step(dev, t, t == 0)
        blobs = dev.export_streams(range(B))
    finally:
        close(ctx, dev)
    ctx, dev = open_dev(B, cfg, fetch=True)
    try:
        dev.import_streams([2, 0, 1], blobs[[2, 0, 1]])
        for t in range(3, 6):
            pts = step(dev, t, False)
        assert pts["age"].max() >= 3     # features followed across the cut
    finally:
        close(ctx, dev)


# ---- 3. migration into a running pipeline: other index, other B, both parities of the target's step counter

def long_sequence(seed):
    return sc.sequence(seed, 7)


def migration(oracle, cfg, Bs, Bt, src_streams, dst_streams, t_imp, src_seeds, dst_seeds, env_ok=None):
    """Streams src_streams of a Bs pipeline, exported after its step 2, go into dst_streams of a Bt pipeline in front of its step t_imp.
    Returns nothing; asserts (a) for every tracked frame of the migrated streams, (b) where the route is the same, and that the other
    streams of the target are byte-identical to a run without the import."""
    src = [sc.sequence(s) for s in src_seeds]
    src_ref = [sc.chain(oracle, cfg, src[b], (src_seeds[b], 0, 6)) for b in range(Bs)]
    dst = [long_sequence(s) for s in dst_seeds]
    n_steps = 7
    kf_src, kf_dst = tuple(src_streams), tuple(dst_streams)
    src_full = run_plain(cfg, Bs, src, range(6), kf_streams=kf_src)
    assert_runs_agree(src_full, run_plain(cfg, Bs, src, range(6), kf_streams=kf_src), Bs)
    plain = run_plain(cfg, Bt, dst, range(n_steps))
    ctx, dev = open_dev(Bs, cfg)
    try:
        for t in range(3):
            dev.push([src[b][t] for b in range(Bs)])
        blobs = dev.export_streams(src_streams)
    finally:
        close(ctx, dev)
    ctx, dev = open_dev(Bt, cfg)
    try:
        others = [b for b in range(Bt) if b not in dst_streams]
        for t in range(n_steps):
            if t == t_imp:
                before = dev.export_streams(others)
                dev.import_streams(dst_streams, blobs)
                assert dev.export_streams(others).tobytes() == before.tobytes()        # streams not named keep their state bit for bit
                assert dev.export_streams(dst_streams).tobytes() == blobs.tobytes()
            k = 3 + t - t_imp       # the source frame a migrated stream is fed
            frames = [dst[b][t] for b in range(Bt)]
            if t >= t_imp:
                for i, b in enumerate(dst_streams):
                    frames[b] = src[src_streams[i]][min(k, 5)]
            res, counts = dev.push(frames)
            o = observe(dev, res, counts, kf_streams=kf_dst if t >= t_imp else ())
            for b in others:
                if t:
                    same_stream(o, b, plain[t], b, ("neighbour", t, b))
                else:
                    assert o["res"][b].tobytes() == plain[t]["res"][b].tobytes() and np.array_equal(o["counts"][b], plain[t]["counts"][b])
            if t >= t_imp and k <= 5:
                for i, b in enumerate(dst_streams):
                    sb = src_streams[i]
                    judge_a(o, b, src_ref[sb][k - 1], ("migrated", t, b), True)
                    if o["sched"] == src_full[k]["sched"]:
                        same_stream(o, b, src_full[k], sb, ("migrated", t, b), frame_offset=k - t, first_own_step=3)
                    else:
                        print(f"[snapshot] migration step {t}: route differs: {o['sched']} vs {src_full[k]['sched']}")
    finally:
        close(ctx, dev)


@pytest.mark.parametrize("t_imp", [4, 5], ids=["before-step-4", "before-step-5"])
def test_migration_other_index_other_batch(oracle, t_imp):
    cfg = sc.Cfg(1, True, True)
    migration(oracle, cfg, 4, 8, [3, 0], [1, 5], t_imp, seeds_for(4, 4200), [4300 + b for b in range(8)])


# ---- 4. batch schedule: behind a step with the key-line stage ahead, into a pipeline that runs ahead

def test_batch_schedule_key_line_stage_ahead(oracle, switches):
    from stvo_amd import capi
    switches({"STVO_POSE_KERNEL": "4", "STVO_GRID_CELLS": "0", "STVO_LINES_AHEAD": "1"})
    cfg = sc.Cfg(1, True, True)
    B = 66
    src_streams, dst_streams = [0, 63, 64, 65], [65, 1, 0, 64]
    src_seeds, dst_seeds = seeds_for(B, 4100), seeds_for(B, 4400)
    src = [sc.sequence(s) for s in src_seeds]
    src_ref = {b: sc.chain(oracle, cfg, src[b], (src_seeds[b], 0, 6)) for b in src_streams}
    dst = [sc.sequence(s) for s in dst_seeds]
    src_full = run_plain(cfg, B, src, range(6), kf_streams=tuple(src_streams))
    assert_runs_agree(src_full, run_plain(cfg, B, src, range(6), kf_streams=tuple(src_streams)), B)
    plain = run_plain(cfg, B, dst, range(6))
    assert all(o["sched"]["lines_ahead"] == 1 and o["sched"]["pose_kernel"] == capi.SCHED_POSE_BATCH for o in plain[2:]), [o["sched"] for o in plain]
    ctx, dev = open_dev(B, cfg)
    try:
        for t in range(3):
            dev.push([src[b][t] for b in range(B)])
        assert dev.last_schedule()["lines_ahead"] == 1          # the export is behind a step that ran ahead
        blobs = dev.export_streams(src_streams)
    finally:
        close(ctx, dev)
    ctx, dev = open_dev(B, cfg)
    try:
        others = [b for b in range(B) if b not in dst_streams]
        for t in range(6):
            if t == 3:
                dev.import_streams(dst_streams, blobs)
            frames = [dst[b][t] for b in range(B)]
            if t >= 3:
                for i, b in enumerate(dst_streams):
                    frames[b] = src[src_streams[i]][t]
            res, counts = dev.push(frames)
            o = observe(dev, res, counts, kf_streams=tuple(dst_streams) if t >= 3 else ())
            if t == 3:      # the step after an import gives up the stages ahead, the one behind it runs ahead again
                assert o["sched"]["lines_ahead"] == 0 and o["sched"]["cells_ahead"] == 0 and o["sched"]["gate"] == 0 and o["sched"]["mid_fork"] == 1
            elif t >= 2:
                assert o["sched"] == plain[t]["sched"] and o["sched"]["lines_ahead"] == 1, (t, o["sched"])
            for b in others:
                if t:
                    same_stream(o, b, plain[t], b, ("neighbour", t, b))
            if t >= 3:
                for i, b in enumerate(dst_streams):
                    sb = src_streams[i]
                    judge_a(o, b, src_ref[sb][t - 1], ("migrated", t, b), True)
                    if o["sched"] == src_full[t]["sched"]:
                        same_stream(o, b, src_full[t], sb, ("migrated", t, b), frame_offset=0, first_own_step=3)
    finally:
        close(ctx, dev)


# ---- 5. key-lines arriving by import

def without_lines(fr):
    z4 = np.zeros((0, 4), np.float32); zd = np.zeros((0, 32), np.uint8)
    out = dict(fr)
    out.update(kl_l=z4, kl_r=z4.copy(), oct_ll=np.zeros(0, np.int32), ldesc_l=zd, ldesc_r=zd.copy(), ang_l=fr["ang_l"][:0])
    return out


def test_key_lines_arrive_by_import(oracle):
    """The target was fed points-only frames, so the set its next step tracks against is flagged as having no key-lines; a stream with
    nl > 0 is imported and the next frame has key-lines: its matched lines and pose follow its oracle chain."""
    cfg = sc.Cfg(1, True, True)
    seed = 4500
    seq = sc.sequence(seed)
    ref = sc.chain(oracle, cfg, seq, (seed, 0, 6))
    assert ref[2]["n_matched_ls"] > 3
    ctx, dev = open_dev(1, cfg)
    try:
        for t in range(3):
            dev.push([seq[t]])
        blob = dev.export_streams([0])
    finally:
        close(ctx, dev)
    from stvo_amd import capi
    assert capi.snapshot_views(blob[0])["header"]["nl"] > 5
    other = sc.sequence(4501)
    ctx, dev = open_dev(2, cfg)
    try:
        for t in range(3):
            res, counts = dev.push([without_lines(other[t]), without_lines(other[t])])
            assert not counts[:, 1].any()
        dev.import_streams([1], blob)
        for t in range(3, 6):
            res, counts = dev.push([without_lines(other[t]) if t > 3 else other[t], seq[t]])
            o = observe(dev, res, counts)
            judge_a(o, 1, ref[t - 1], (t, 1), True)
            assert res[1]["n_matched_ls"] == ref[t - 1]["n_matched_ls"]
            assert res[0]["n_matched_ls"] == 0 and res[0]["status"] == 0
    finally:
        close(ctx, dev)


# ---- 6. capacities

def test_other_capacities(oracle):
    from stvo_amd import capi
    cfg = sc.Cfg(1, True, True)
    B = 2
    seeds = seeds_for(B, 4100)
    seqs = [sc.sequence(s) for s in seeds]
    refs = [sc.chain(oracle, cfg, seqs[b], (seeds[b], 0, 6)) for b in range(B)]
    full = run_plain(cfg, B, seqs, range(6), kf_streams=(0, 1))
    assert_runs_agree(full, run_plain(cfg, B, seqs, range(6), kf_streams=(0, 1)), B)
    ctx, dev = open_dev(B, cfg)
    try:
        for t in range(3):
            dev.push([seqs[b][t] for b in range(B)])
        blobs = dev.export_streams(range(B))
    finally:
        close(ctx, dev)
    heads = [capi.snapshot_views(b)["header"] for b in blobs]
    assert all(128 < max(h["n"], h["kf"]["n_pts"]) <= 384 and h["K"] == 512 for h in heads), heads
    assert all(max(r["n_stereo_pt"] for r in refs[b]) <= 384 for b in range(B))
    # (384, 64): every count fits, the continuation is exact
    ctx, dev = open_dev(B, cfg, K=384)
    try:
        assert dev.snapshot_info()["K"] == 384
        dev.import_streams(range(B), blobs)
        again = dev.export_streams(range(B))
        for b in range(B):     # the same state, cut at other capacities
            va, vb = capi.snapshot_views(again[b]), capi.snapshot_views(blobs[b])
            assert va["header"]["K"] == 384 and va["header"]["bytes"] < vb["header"]["bytes"]
            for k in vb:
                if k not in ("header", "layout", "live"):
                    assert va[k].tobytes() == vb[k].tobytes(), (b, k)
        for t in range(3, 6):
            res, counts = dev.push([seqs[b][t] for b in range(B)])
            o = observe(dev, res, counts, kf_streams=(0, 1))
            for b in range(B):
                judge_a(o, b, refs[b][t - 1], (t, b), True)
                if o["sched"] == full[t]["sched"]:
                    same_stream(o, b, full[t], b, (t, b), frame_offset=2, first_own_step=3)
    finally:
        close(ctx, dev)
    # (128, 64): refused, and the target's next step is what it is without the attempt
    outs = []
    for attempt in (True, False):
        ctx, dev = open_dev(B, cfg, K=128)
        try:
            small = [[dict(f, kp_l=f["kp_l"][:100], oct_l=f["oct_l"][:100], desc_l=f["desc_l"][:100], kp_r=f["kp_r"][:100], desc_r=f["desc_r"][:100])
                      for f in s] for s in seqs]
            dev.push([small[b][0] for b in range(B)])
            if attempt:
                before = dev.export_streams(range(B))
                rc = ctx.lib.stvo_seq_import_streams(dev.h, B, np.arange(B, dtype=np.int32).ctypes.data_as(C.c_void_p),
                                                     blobs.ctypes.data_as(C.c_void_p), blobs.shape[1])
                assert rc == CAPACITY
                assert dev.export_streams(range(B)).tobytes() == before.tobytes()
            res, counts = dev.push([small[b][1] for b in range(B)])
            outs.append(observe(dev, res, counts))
        finally:
            close(ctx, dev)
    assert outs[0]["sched"] == outs[1]["sched"]
    for b in range(B):
        same_stream(outs[0], b, outs[1], b, ("after a refused import", b))


# ---- 7. counts at the edges of the copy

def cut_points(fr, n):
    return dict(fr, kp_l=fr["kp_l"][:n], oct_l=fr["oct_l"][:n], desc_l=fr["desc_l"][:n], kp_r=fr["kp_r"][:n], desc_r=fr["desc_r"][:n])


def empty_frame(fr):
    return without_lines(cut_points(fr, 0))


def edge_sequence(case):
    """Five planned frames whose frame 2 leaves the set under test; (frames, K)."""
    normal = sc.sequence(4610)
    if case == "full-capacity":   # 64 key-points that all associate, at capacity 64 (the count is asserted where it is relied on)
        return synth.make_stereo_sequence(4600, n_frames=5, n_pts=64, n_lines=12, cam=CAM, distract=0.0), 64
    n_pts = {"empty": 0, "one-point": 1}[case]
    edge = synth.make_stereo_sequence(4620, n_frames=3, n_pts=n_pts, n_lines=0, cam=CAM, distract=0.0)[2]
    return [normal[0], normal[1], edge, normal[3], normal[4]], 512


@pytest.mark.parametrize("case", ["empty", "one-point", "full-capacity"])
def test_counts_at_the_edges(oracle, case):
    """A stream whose set is empty (n = nl = 0) / holds one point / holds exactly K = 64 points, its key-frame set holding another
    number of rows where the scene gives one: export -> import into ANOTHER stream of the same pipeline -> export gives the identical
    blob, and from then on the copy, fed the same frames in the same steps, equals the original byte for byte and both follow the
    oracle chain."""
    from stvo_amd import capi
    cfg = sc.Cfg(1, True, True)
    frames, K = edge_sequence(case)
    ref = sc.chain(oracle, cfg, frames, ("edge", case))
    other = synth.make_stereo_sequence(4602, n_frames=5, n_pts=64, n_lines=12, cam=CAM, distract=0.0)
    want_n = {"empty": 0, "one-point": 1, "full-capacity": 64}[case]
    ctx, dev = open_dev(2, cfg, K=K)
    try:
        assert dev.snapshot_info()["K"] == K
        for t in range(3):
            dev.push([frames[t], other[t]])
        blob = dev.export_streams([0])
        h = capi.snapshot_views(blob[0])["header"]
        assert h["n"] == want_n and (case == "full-capacity" or h["nl"] == 0), h
        if case != "full-capacity":
            assert h["kf"]["n_pts"] != h["n"] or ref[1]["new_kf"], h     # the key-frame set is not the current set
        dev.import_streams([1], blob)
        assert dev.export_streams([1]).tobytes() == blob.tobytes() == dev.export_streams([0]).tobytes()
        for t in range(3, 5):
            res, counts = dev.push([frames[t], frames[t]])
            o = observe(dev, res, counts, kf_streams=(0, 1))
            for b in range(2):
                judge_a(o, b, ref[t - 1], (case, t, b), True)
            same_stream(o, 1, o, 0, (case, t))
    finally:
        close(ctx, dev)


# ---- 8. refusals: every row of the table through the C ABI, and each leaves the pipeline as it was

def test_refusals(oracle):
    from stvo_amd import capi
    cfg = sc.Cfg(1, True, True)
    B = 2
    seeds = seeds_for(B, 4100)
    seqs = [sc.sequence(s) for s in seeds]
    refs = [sc.chain(oracle, cfg, seqs[b], (seeds[b], 0, 6)) for b in range(B)]

    def exported(cfg_, cam=CAM, features=True):
        ctx_, dev_ = open_dev(B, cfg_, features=features, cam=cam)
        try:
            for t in range(2):
                dev_.push([seqs[b][t] for b in range(B)])
            return dev_.export_streams(range(B))
        finally:
            close(ctx_, dev_)

    good = exported(cfg)
    ctx, dev = open_dev(B, cfg)
    try:
        L = ctx.lib
        for t in range(2):
            dev.push([seqs[b][t] for b in range(B)])
        state = dev.export_streams(range(B))
        assert state.tobytes() == good.tobytes()
        idx = np.arange(B, dtype=np.int32)

        def rc_of(blobs, streams=idx, n=B, stride=None):
            blobs = np.ascontiguousarray(blobs)
            st = np.ascontiguousarray(streams, dtype=np.int32)
            return L.stvo_seq_import_streams(dev.h, n, st.ctypes.data_as(C.c_void_p), blobs.ctypes.data_as(C.c_void_p),
                                             blobs.shape[1] if stride is None else stride)

        def broken(field, value):
            bad = good.copy()
            bad[1, :256].view(capi.SNAP_HEADER_DTYPE)[0][field] = value
            return bad

        cases = {
            "magic": (broken("magic", capi.SNAP_MAGIC ^ 1), INVALID),
            "version": (broken("version", capi.SNAP_VERSION + 1), INVALID),
            "bytes": (broken("bytes", good.shape[1] - 256), INVALID),
            "flags": (exported(sc.Cfg(1, False, True)), INVALID),                        # no motion model there
            "flags, trajectory without key-frames": (exported(sc.Cfg(1, True, False)), INVALID),
            "flags, nothing on": (exported(cfg, features=False), INVALID),
            "camera": (exported(cfg, cam=dict(CAM, b=CAM["b"] * 1.01)), INVALID),
            "image size": (exported(cfg, cam=dict(CAM, height=CAM["height"] + 8)), INVALID),
            "mp": (exported(_cfg_with(mp=match_params("kitti", min_disp=1.5))), INVALID),
            "op": (exported(_cfg_with(op=opt_params("kitti", max_iters=4))), INVALID),
        }
        for name, (blobs, want) in cases.items():
            assert rc_of(blobs) == want, name
            assert dev.export_streams(range(B)).tobytes() == state.tobytes(), name
        assert rc_of(good, streams=[0, 2]) == INVALID and rc_of(good, streams=[-1, 1]) == INVALID      # out of range
        assert rc_of(good, streams=[1, 1]) == INVALID                                                    # named twice
        assert rc_of(good, stride=good.shape[1] - 16) == INVALID                                         # blobs would overlap
        assert L.stvo_seq_import_streams(dev.h, B, None, good.ctypes.data_as(C.c_void_p), good.shape[1]) == INVALID
        assert L.stvo_seq_import_streams(dev.h, B, idx.ctypes.data_as(C.c_void_p), None, good.shape[1]) == INVALID
        assert L.stvo_seq_import_streams(None, B, idx.ctypes.data_as(C.c_void_p), good.ctypes.data_as(C.c_void_p), good.shape[1]) == INVALID
        assert L.stvo_seq_export_streams(dev.h, B, np.array([0, B], np.int32).ctypes.data_as(C.c_void_p), state.ctypes.data_as(C.c_void_p)) == INVALID
        assert L.stvo_seq_export_streams(dev.h, B, None, state.ctypes.data_as(C.c_void_p)) == INVALID
        assert L.stvo_seq_export_streams(dev.h, B, idx.ctypes.data_as(C.c_void_p), None) == INVALID
        lay = capi.SnapshotLayout()
        assert L.stvo_seq_snapshot_layout(512, 64, 4, C.byref(lay)) == INVALID and L.stvo_seq_snapshot_layout(512, 64, 16, C.byref(lay)) == INVALID
        assert L.stvo_seq_snapshot_layout(512, 64, 31, None) == INVALID
        # (counts that do not fit, STVO_ERR_CAPACITY: test_other_capacities)
        assert dev.export_streams(range(B)).tobytes() == state.tobytes()
        # after all of it the next step is the undisturbed one: the oracle chain, and the schedule of a pipeline that never imported
        res, counts = dev.push([seqs[b][2] for b in range(B)])
        o = observe(dev, res, counts)
        for b in range(B):
            judge_a(o, b, refs[b][1], ("after the refusals", b), True)
        plain = run_plain(cfg, B, seqs, range(3))
        assert o["sched"] == plain[2]["sched"]
        for b in range(B):
            same_stream(o, b, plain[2], b, ("after the refusals", b))
    finally:
        close(ctx, dev)


def _cfg_with(mp=None, op=None):
    cfg = sc.Cfg(1, True, True)
    if mp is not None:
        cfg.mp = mp
    if op is not None:
        cfg.op = op
    return cfg


# ---- 9. ImagePipeline: images -> poses with the thresholds travelling beside the blobs

def test_image_pipeline_export_import():
    """adaptive_fast and trajectory at B = 2 on the images of tests/test_gpu_adaptive_fast.py: three pairs, export, a NEW context and
    pipeline, import with the thresholds, two more pairs — poses, counts, trajectory records and fast_thresholds() equal the
    uninterrupted run byte for byte."""
    import fast_adapt_cases as fc
    from stvo_amd import capi, images
    imgs = fc.images()
    B = 2

    def open_pipe():
        ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
        try:
            pipe = images.ImagePipeline(ctx, B, fc.CAM, match_params("kitti"), opt_params("kitti", has_lines=0), max_kp=fc.MAX_KP,
                                        nfeatures=fc.NFEATURES, fast_threshold=fc.TH0, adaptive_fast=fc.params(),
                                        trajectory=capi.traj_params("kitti", keyframes=False), trajectory_log=1)
        except Exception:
            ctx.close()
            raise
        return ctx, pipe

    def push(pipe, t):
        left = np.stack([imgs[s][t][0] for s in range(B)])
        right = np.stack([imgs[s][t][1] for s in range(B)])
        res, counts = pipe.push_images(left, right)
        rec = pipe.read_trajectory() if t else None
        return res.tobytes(), counts.tobytes(), rec.tobytes() if t else b"", pipe.fast_thresholds().tobytes()

    ctx, pipe = open_pipe()
    try:
        full = [push(pipe, t) for t in range(5)]
    finally:
        pipe.close()
        ctx.close()
    assert len({f[3] for f in full}) > 1     # the thresholds moved along the way
    ctx, pipe = open_pipe()
    try:
        for t in range(3):
            assert push(pipe, t) == full[t]   # two uninterrupted runs agree
        blobs, th = pipe.export_streams([0, 1])
        assert th.tobytes() == full[2][3]
    finally:
        pipe.close()
        ctx.close()
    ctx, pipe = open_pipe()
    try:
        pipe.import_streams([0, 1], blobs, th)
        assert pipe.fast_thresholds().tobytes() == full[2][3]
        for t in range(3, 5):
            assert push(pipe, t) == full[t], t
    finally:
        pipe.close()
        ctx.close()


# ---- 10. the app: --save-state / --load-state on the --device-pipeline route

def test_app_save_and_load_state(tmp_path):
    import os
    import subprocess
    from stvo_amd import capi
    app = os.path.join(capi.PKG_DIR, "bin", "imagesStVO_synth")
    seq = str(tmp_path / "seq.bin")
    synth.write_sequence(seq, list(sc.sequence(4700)), CAM)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"max_kf_t_dist : {KF['max_kf_t_dist']}\n")
    common = ["--preset", "kitti", "-c", str(cfg), "--device-pipeline", "--keyframes", "--tracks"]

    def run(name, extra, preset_args=None, ok=True):
        res = str(tmp_path / f"{name}.bin")
        args = [app, seq, res] + (preset_args or common) + list(extra)
        p = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert (p.returncode == 0) == ok, (args, p.returncode, p.stderr[-800:], p.stdout[-400:])
        tracks = [ln for ln in p.stdout.splitlines() if "Proc. time" not in ln and "frame pairs" not in ln]
        return (open(res, "rb").read() if ok else b""), tracks, p

    state = str(tmp_path / "state.bin")
    whole, whole_tracks, _ = run("whole", ["-n", "6"])
    head, head_tracks, _ = run("head", ["-n", "3", "--save-state", state])
    tail, tail_tracks, _ = run("tail", ["-o", "3", "-n", "3", "--load-state", state])
    assert len(synth.read_results(str(tmp_path / "whole.bin"))) == 5 and len(synth.read_results(str(tmp_path / "tail.bin"))) == 3
    assert head + tail == whole                       # the output records, byte for byte
    assert head_tracks + tail_tracks == whole_tracks and len(whole_tracks) >= 5   # and what --tracks prints of every frame
    assert os.path.getsize(state) == capi.snapshot_layout(2048, 512, capi.SNAP_TRAJ | capi.SNAP_TRAJ_KF | capi.SNAP_TRACKS)["bytes"]
    # a state saved under another preset is refused
    other = str(tmp_path / "state_euroc.bin")
    run("euroc", ["-n", "3", "--save-state", other], preset_args=["--preset", "euroc", "--device-pipeline", "--keyframes", "--tracks"])
    _, _, p = run("refused", ["-o", "3", "-n", "3", "--load-state", other], ok=False)
    assert "--load-state" in p.stderr and "does not fit" in p.stderr
    # ... and so is one saved with other options (no tracks), and a file that is no state
    _, _, p = run("refused2", ["-o", "3", "-n", "3", "--load-state", seq], ok=False)
    assert "--load-state" in p.stderr
    _, _, p = run("refused3", ["-n", "3", "--save-state", state], preset_args=["--preset", "kitti"], ok=False)
    assert "--device-pipeline" in p.stderr


# ---- the _dev forms end to end, blobs further apart than their size

def test_device_forms_round_trip(oracle):
    import torch
    cfg = sc.Cfg(1, True, True)
    B = 3
    seeds = seeds_for(B, 4100)
    seqs = [sc.sequence(s) for s in seeds]
    refs = [sc.chain(oracle, cfg, seqs[b], (seeds[b], 0, 6)) for b in range(B)]
    ctx, dev = open_dev(B, cfg)
    try:
        for t in range(3):
            dev.push([seqs[b][t] for b in range(B)])
        size = dev.snapshot_info()["bytes"]
        stride = size + 512
        packed = torch.zeros(B * size, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        dev.export_streams_dev([2, 0, 1], packed.data_ptr())
        ctx.synchronize()
        blobs = packed.cpu().numpy().reshape(B, size)
        assert blobs.tobytes() == dev.export_streams([2, 0, 1]).tobytes()
        spaced = torch.full((B * stride,), 0x5A, dtype=torch.uint8, device="cuda:0")
        spaced.view(B, stride)[:, :size] = packed.view(B, size)
        torch.cuda.synchronize()
    finally:
        close(ctx, dev)
    ctx, dev = open_dev(4, cfg)
    try:
        dev.import_streams_dev([3, 1, 0], spaced.data_ptr(), stride)     # source streams 2, 0, 1 -> 3, 1, 0
        assert ctx.lib.stvo_seq_import_streams_dev(dev.h, 3, np.array([3, 1, 0], np.int32).ctypes.data_as(C.c_void_p),
                                                   C.c_void_p(spaced.data_ptr()), stride - 8) == INVALID    # not a multiple of 16
        assert ctx.lib.stvo_seq_import_streams_dev(dev.h, 3, np.array([3, 1, 0], np.int32).ctypes.data_as(C.c_void_p),
                                                   C.c_void_p(spaced.data_ptr() + 8), stride) == INVALID    # blobs not 16-byte aligned
        assert dev.export_streams([3, 1, 0]).tobytes() == blobs.tobytes()
        from stvo_amd import capi
        h = capi.snapshot_views(dev.export_streams([2])[0])["header"]     # the stream not named: an empty set, no key-frame set
        assert h["n"] == 0 and h["nl"] == 0 and h["kf"].tobytes() == bytes(16)
        src_of = {3: 2, 1: 0, 0: 1}
        for t in range(3, 5):
            frames = [seqs[src_of[b]][t] if b in src_of else sc.sequence(4108)[t] for b in range(4)]
            res, counts = dev.push(frames)
            o = observe(dev, res, counts)
            for b, sb in src_of.items():
                judge_a(o, b, refs[sb][t - 1], (t, b), True)
    finally:
        close(ctx, dev)
