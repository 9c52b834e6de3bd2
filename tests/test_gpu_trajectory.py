"""Trajectory and key-frame decision per stream on the device: the stand-alone kernel (stvo_traj_init_dev / stvo_traj_update_dev)
against the extended-precision statement on the shared inputs of tests/trajectory_cases.py, then the same behind the pipeline's steps
(stvo_seq_set_trajectory / stvo_seq_read_trajectory), behind ImagePipeline and in the app, against the oracle-driven CPU chain
(tests/pipeline_ref.py)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import np_trajectory as npt
import pipeline_ref
import trajectory_cases as tc
from stvo_amd import synth
from stvo_amd.ctypes_types import POSE_RESULT_DTYPE, TRAJ_RECORD_DTYPE, TRAJ_STATE_DTYPE, match_params, opt_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "stvo-pl_amd", "bin", "imagesStVO_synth")
PAD = 2   # records behind the B a launch is given: it must not touch them


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def device_update(hip):
    """update_fn of trajectory_cases.check_batch on the kernel: state and records carry PAD records of a byte pattern behind B."""
    import torch
    from stvo_amd import capi

    def fn(results, p, state):
        B = len(state)
        d_state = torch.cat([to_dev(state), torch.full((PAD * TRAJ_STATE_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")])
        d_rec = torch.full(((B + PAD) * TRAJ_RECORD_DTYPE.itemsize,), 0x5A, dtype=torch.uint8, device="cuda:0")
        d_res = to_dev(results)
        torch.cuda.synchronize()
        capi.traj_update_dev(hip, d_res, p, d_state[:B * TRAJ_STATE_DTYPE.itemsize], d_rec[:B * TRAJ_RECORD_DTYPE.itemsize])
        hip.synchronize()
        hs, hr = d_state.cpu().numpy(), d_rec.cpu().numpy()
        assert (hs[B * TRAJ_STATE_DTYPE.itemsize:] == 0xA5).all() and (hr[B * TRAJ_RECORD_DTYPE.itemsize:] == 0x5A).all()
        return hs[:B * TRAJ_STATE_DTYPE.itemsize].view(TRAJ_STATE_DTYPE).copy(), hr[:B * TRAJ_RECORD_DTYPE.itemsize].view(TRAJ_RECORD_DTYPE).copy()
    return fn


def device_init(hip, B):
    import torch
    from stvo_amd import capi
    d = torch.full(((B + PAD) * TRAJ_STATE_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    capi.traj_init_dev(hip, d[:B * TRAJ_STATE_DTYPE.itemsize])
    hip.synchronize()
    h = d.cpu().numpy()
    assert (h[B * TRAJ_STATE_DTYPE.itemsize:] == 0xA5).all()
    return h[:B * TRAJ_STATE_DTYPE.itemsize].view(TRAJ_STATE_DTYPE).copy()


def report(title, worst):
    """The measured deviation per field as a multiple of the oracle's own (the bound is 8 of them plus one ulp)."""
    c = tc.stepwise()
    print(f"\n{title}: deviation from the extended-precision statement, device / oracle")
    for k in npt.FIELDS:
        o = c["deviation"]["oracle"][k]
        print(f"  {k:22s} {worst[k]:10.3e} / {o:10.3e} = {worst[k] / o if o else 0.0:6.2f}")


# ---- 4. the stand-alone kernel, every stream at another phase of case 1

@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_kernel_against_the_statement(hip, B):
    """13 consecutive updates of B streams, stream b starting at frame b mod 60 of case 1: in one launch some lanes reset, some fail
    and some count on, and the 12-frame rule passes through every stream.  State and records after every update: decisions, counters,
    new_kf and the reset values exact; floating-point fields within 8 x the oracle's own deviation from the extended-precision
    statement (+ one ulp of the field's largest magnitude)."""
    import traj_host_lib
    state0 = device_init(hip, B)
    assert state0.tobytes() == traj_host_lib.init(B).tobytes()
    worst, dec, guarded = tc.check_batch(device_update(hip), tc.stepwise()["prm"], tc.phased(B, 13), state0, tc.bounds())
    assert guarded == 0
    assert dec.any(axis=1).all() and not dec.all()
    if B > 1:
        assert len({tuple(d) for d in dec}) > 1   # the lanes of one launch diverge
    report(f"B = {B}", worst)


# ---- 5. every trigger in one launch, then keyframes off

def test_triggers_in_one_batch_and_keyframes_off(hip):
    import traj_host_lib
    trig = tc.triggers()
    worst, dec, guarded = tc.check_batch(device_update(hip), tc.common_params(), tc.trigger_batch(), device_init(hip, len(trig)), tc.bounds())
    assert guarded == 0 and len(trig) == 7
    assert [int(np.argmax(d)) for d in dec] == [c[3] for c in trig] and dec.any(axis=1).all()   # each at its frame, none before
    report("triggers", worst)
    # 2h on a second state array: 40 updates, never a reset
    from stvo_amd import capi
    off = capi.traj_params("kitti", keyframes=False)
    worst, dec, guarded = tc.check_batch(device_update(hip), off, tc.phased(3, 40), traj_host_lib.init(3), tc.bounds())
    assert not dec.any() and guarded == 0
    report("keyframes off", worst)


# ---- 6. behind the pipeline's steps

KF = dict(min_entropy_ratio=0.85, max_kf_t_dist=1.4, max_kf_r_dist=15.0)   # the scenes move 0.5 .. 1.5 per frame: a reset within three frames
SEQ_SEEDS = (7100, 7101, 7102)


@functools.lru_cache(maxsize=None)
def seq_frames():
    return tuple(tuple(synth.make_stereo_sequence(s, n_frames=6, n_pts=300, n_lines=40, cam=synth.KITTI_CAM)) for s in SEQ_SEEDS)


_seq_ref = {}


def seq_reference(oracle, motion_model=False, keyframes=True):
    key = (motion_model, keyframes)
    if key not in _seq_ref:
        _seq_ref[key] = [pipeline_ref.run_sequence(oracle, list(fr), synth.KITTI_CAM, match_params("kitti"), opt_params("kitti"),
                                                   keyframes=KF if keyframes else None, motion_model=motion_model) for fr in seq_frames()]
        if keyframes:
            assert all(1 <= sum(o["new_kf"] for o in r) < len(r) for r in _seq_ref[key])   # a reset falls inside the 6 frames of every stream
    return _seq_ref[key]


def compare_record(rec, o, keyframes=True):
    """The tolerances tests/test_gpu_handler.py::compare applies to the same quantities (they include the pose kernel's own deviation)."""
    assert np.allclose(rec["Tfw"].reshape(4, 4), o["Tfw"], atol=1e-7)
    assert np.allclose(rec["Tfw_cov"].reshape(6, 6), o["Tfw_cov"], rtol=1e-6, atol=1e-10)
    assert int(rec["new_kf"]) == (o["new_kf"] if keyframes else 0)


@pytest.mark.parametrize("streams,reps,motion_model", [(3, 1, False), (3, 1, True), (1, 1, False), (3, 6, False)],
                         ids=["B3", "B3-motion-model", "B1", "B18-results-in-device-memory"])
def test_behind_the_pipeline_steps(oracle, streams, reps, motion_model):
    """B <= 16: the step writes its results into the pinned block and the update reads them there; B = 18: device memory."""
    from stvo_amd import capi
    B = streams * reps
    frames, ref = seq_frames(), seq_reference(oracle, motion_model)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    dev = capi.Sequences(ctx, B, 512, 64, synth.KITTI_CAM, match_params("kitti"), opt_params("kitti"))
    try:
        if motion_model:
            dev.set_motion_model(True)
        dev.set_trajectory(capi.traj_params("kitti", **KF), log_steps=2)
        seen = []
        for k in range(6):
            res, _ = dev.push([frames[b % streams][k] for b in range(B)])
            got = dev.read_trajectory(5)
            if k == 0:
                assert got.shape == (0, B)   # the first frame alone: no update, the state initial
                assert dev.trajectory_state().tobytes() == np.tile(np.frombuffer(npt_initial_bytes(), np.uint8), B).tobytes()
                continue
            assert got.shape == (min(k, 2), B)   # asked for 5, the ring holds 2
            last = dev.read_trajectory(1)
            assert last.shape == (1, B) and last.tobytes() == got[-1:].tobytes()
            if seen:
                assert got[0].tobytes() == seen[-1].tobytes()   # oldest first
            seen.append(got[-1].copy())
            for b in range(B):
                o = ref[b % streams][k - 1]
                assert res[b]["status"] == o["status"]
                compare_record(got[-1][b], o)
                assert got[-1][b]["frame"] == k
        st = dev.trajectory_state()
        for b in range(B):
            n_kf = sum(o["new_kf"] for o in ref[b % streams])
            assert st[b]["n_frames"] == 5 and st[b]["n_keyframes"] == n_kf
    finally:
        dev.close()
        ctx.close()


def npt_initial_bytes():
    import traj_host_lib
    return traj_host_lib.init(1).tobytes()


# ---- 7. images -> trajectory

IMG_CAM = dict(synth.KITTI_CAM, width=320, height=200)
IMG_SEEDS = (54, 55)   # 54: every pose accepted, a key-frame by the rule; 55: a rejected pose, an accepted one, too few inliers
IMG_FRAMES = 4


@functools.lru_cache(maxsize=None)
def image_pairs():
    return tuple(tuple(synth.make_stereo_image_sequence(s, IMG_FRAMES, IMG_CAM)) for s in IMG_SEEDS)


_img_ref = {}


def image_reference(oracle, kf):
    """The CPU chain of tests/fast_adapt_cases.py without the adaptive threshold: the ORB oracle on every image, its key-points
    through the oracle-driven per-frame loop with the key-frame decision."""
    key = tuple(sorted(kf.items()))
    if key not in _img_ref:
        pattern = oracle.orb_default_pattern()
        z4 = np.zeros((0, 4), np.float32); zd = np.zeros((0, 32), np.uint8)
        out = []
        for pairs in image_pairs():
            frames = []
            for left, right in pairs:
                l = oracle.orb_detect_levels(left, nfeatures=2000, nlevels=1, fast_th=20, pattern=pattern, cap=2048)
                r = oracle.orb_detect_levels(right, nfeatures=2000, nlevels=1, fast_th=20, pattern=pattern, cap=2048)
                frames.append(dict(kp_l=l["kp"], oct_l=l["octave"], desc_l=l["desc"], kp_r=r["kp"], desc_r=r["desc"], kl_l=z4,
                                   oct_ll=np.zeros(0, np.int32), ldesc_l=zd, kl_r=z4, ldesc_r=zd))
            out.append(pipeline_ref.run_sequence(oracle, frames, IMG_CAM, match_params("kitti"), opt_params("kitti", has_lines=0),
                                                 fast=dict(adaptive=False, th0=20), keyframes=kf))
        _img_ref[key] = out
    return _img_ref[key]


def test_image_pipeline_trajectory(oracle):
    from stvo_amd import capi, images
    kf = dict(min_entropy_ratio=0.85, max_kf_t_dist=5.0, max_kf_r_dist=15.0)
    ref = image_reference(oracle, kf)
    assert any(o["status"] == 0 for r in ref for o in r)
    B = len(IMG_SEEDS)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        pipe = images.ImagePipeline(ctx, B, IMG_CAM, match_params("kitti"), opt_params("kitti", has_lines=0), max_kp=2048, nfeatures=2000,
                                    fast_threshold=20, trajectory=capi.traj_params("kitti", **kf), trajectory_log=1)
        try:
            pairs = image_pairs()
            for k in range(IMG_FRAMES):
                res, _ = pipe.push_images(np.stack([pairs[b][k][0] for b in range(B)]), np.stack([pairs[b][k][1] for b in range(B)]))
                got = pipe.read_trajectory()
                if k == 0:
                    assert got.shape == (0, B)
                    continue
                assert got.shape == (1, B)
                for b in range(B):
                    assert res[b]["status"] == ref[b][k - 1]["status"]
                    compare_record(got[0][b], ref[b][k - 1])
        finally:
            pipe.close()
        plain = images.ImagePipeline(ctx, B, IMG_CAM, match_params("kitti"), opt_params("kitti", has_lines=0), max_kp=2048, nfeatures=2000)
        try:
            with pytest.raises(ValueError):
                plain.read_trajectory()
        finally:
            plain.close()
    finally:
        ctx.close()


# ---- 8. the app

def run_app(tmp_path, name, extra):
    seq = str(tmp_path / "seq.bin"); res = str(tmp_path / f"{name}.bin")
    if not os.path.exists(seq):
        synth.write_sequence(seq, list(seq_frames()[0]), synth.KITTI_CAM)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"max_kf_t_dist : {KF['max_kf_t_dist']}\n")
    p = subprocess.run([APP, seq, res, "--preset", "kitti", "-c", str(cfg), *extra], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr + p.stdout
    return synth.read_results(res)


@pytest.mark.parametrize("keyframes", [True, False])
def test_app_device_pipeline_writes_the_trajectory(tmp_path, oracle, keyframes):
    flags = ("--keyframes",) if keyframes else ()
    dev = run_app(tmp_path, "dev", ("--device-pipeline",) + flags)
    handler = run_app(tmp_path, "handler", flags)
    ref = seq_reference(oracle, keyframes=keyframes)[0]
    assert len(dev) == len(handler) == 5
    for r, h, o in zip(dev, handler, ref):
        assert r["ints"][1] == h["ints"][1] == o["status"]
        assert r["Tfw"].any()   # no longer the 52 zeros
        assert np.allclose(r["Tfw"].reshape(4, 4), h["Tfw"].reshape(4, 4), atol=1e-7)
        assert np.allclose(r["Tfw_cov"].reshape(6, 6), h["Tfw_cov"].reshape(6, 6), rtol=1e-6, atol=1e-10)
        assert int(r["pad"]) == int(h["pad"]) == (o["new_kf"] if keyframes else 0)
        assert np.allclose(r["Tfw"].reshape(4, 4), o["Tfw"], atol=1e-7)
    if keyframes:
        assert 1 <= sum(int(r["pad"]) for r in dev) < 5
        return
    # -o / -s stay refused on the device path
    seq = str(tmp_path / "seq.bin")
    p = subprocess.run([APP, seq, str(tmp_path / "x.bin"), "--device-pipeline", "-o", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "-o / -s" in p.stderr


# ---- 9. off is off

def test_off_is_off(hip):
    from stvo_amd import capi
    frames = seq_frames()
    B = len(frames)
    mk = lambda: capi.Sequences(hip, B, 512, 64, synth.KITTI_CAM, match_params("kitti"), opt_params("kitti"))
    off, on = mk(), mk()
    try:
        on.set_trajectory(capi.traj_params("kitti", **KF), log_steps=1)
        for k in range(4):
            ra, ca = off.push([frames[b][k] for b in range(B)])
            sa = off.last_schedule()
            rb, cb = on.push([frames[b][k] for b in range(B)])
            assert sa == on.last_schedule()
            assert ra.tobytes() == rb.tobytes() and np.array_equal(ca, cb)   # the feature only reads the results
        assert any(r["status"] == 0 for r in ra)
        rec = np.zeros((1, B), dtype=TRAJ_RECORD_DTYPE)
        n = C.c_int32(-7)
        assert hip.lib.stvo_seq_read_trajectory(off.h, 1, rec.ctypes.data_as(C.c_void_p), C.byref(n)) == -1   # STVO_ERR_INVALID_ARG
        assert n.value == -7 and not rec.view(np.uint8).any()
        p = C.c_void_p(5)
        assert hip.lib.stvo_seq_trajectory_state_dev(off.h, C.byref(p)) == -1 and p.value == 5
        st = np.full(B, 7, dtype=np.uint8).repeat(TRAJ_STATE_DTYPE.itemsize)
        assert hip.lib.stvo_seq_read_trajectory_state(off.h, st.ctypes.data_as(C.c_void_p)) == -1 and (st == 7).all()
        with pytest.raises(capi.StvoError):
            off.read_trajectory()
        assert on.read_trajectory().shape == (1, B)
    finally:
        off.close()
        on.close()


# ---- 10. argument checks: each refused, each refusal changes nothing

def test_argument_checks(hip):
    import torch
    from stvo_amd import capi
    L, INVALID = hip.lib, -1
    prm = capi.traj_params("kitti")
    B = 4
    state = to_dev(np.zeros(B, dtype=TRAJ_STATE_DTYPE))
    res = to_dev(np.zeros(B, dtype=POSE_RESULT_DTYPE))
    torch.cuda.synchronize()
    capi.traj_init_dev(hip, state)
    hip.synchronize()
    before = state.cpu().numpy().tobytes()
    assert L.stvo_traj_init_dev(None, B, state.data_ptr()) == INVALID
    assert L.stvo_traj_init_dev(hip.h, B, None) == INVALID
    assert L.stvo_traj_init_dev(hip.h, 0, state.data_ptr()) == INVALID
    for args in ((None, B, res.data_ptr(), C.byref(prm), state.data_ptr(), None), (hip.h, 0, res.data_ptr(), C.byref(prm), state.data_ptr(), None),
                 (hip.h, B, None, C.byref(prm), state.data_ptr(), None), (hip.h, B, res.data_ptr(), None, state.data_ptr(), None),
                 (hip.h, B, res.data_ptr(), C.byref(prm), None, None)):
        assert L.stvo_traj_update_dev(*args) == INVALID
    hip.synchronize()
    assert state.cpu().numpy().tobytes() == before
    frames = seq_frames()
    seq = capi.Sequences(hip, 1, 512, 64, synth.KITTI_CAM, match_params("kitti"), opt_params("kitti"))
    try:
        assert L.stvo_seq_set_trajectory(None, C.byref(prm), 1) == INVALID
        assert L.stvo_seq_set_trajectory(seq.h, C.byref(prm), 0) == INVALID
        assert L.stvo_seq_set_trajectory(seq.h, C.byref(prm), -3) == INVALID
        too_many = (1 << 30) // TRAJ_RECORD_DTYPE.itemsize + 1        # one record more than 1 GiB at B = 1
        assert L.stvo_seq_set_trajectory(seq.h, C.byref(prm), too_many) == INVALID
        with pytest.raises(capi.StvoError):   # every refusal left the feature off
            seq.read_trajectory()
        seq.set_trajectory(prm, log_steps=3)
        assert L.stvo_seq_set_trajectory(seq.h, C.byref(prm), 0) == INVALID   # ... or on, as it was
        assert seq.read_trajectory(3).shape == (0, 1)
        rec = np.zeros((1, 1), dtype=TRAJ_RECORD_DTYPE); n = C.c_int32(-7)
        assert L.stvo_seq_read_trajectory(seq.h, 0, rec.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID
        assert L.stvo_seq_read_trajectory(seq.h, 1, None, C.byref(n)) == INVALID
        assert L.stvo_seq_read_trajectory(seq.h, 1, rec.ctypes.data_as(C.c_void_p), None) == INVALID
        assert L.stvo_seq_read_trajectory(None, 1, rec.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID and n.value == -7
        assert L.stvo_seq_trajectory_state_dev(seq.h, None) == INVALID
        assert L.stvo_seq_read_trajectory_state(seq.h, None) == INVALID and L.stvo_seq_read_trajectory_state(None, rec.ctypes.data_as(C.c_void_p)) == INVALID
        assert seq.read_trajectory(1 << 30).shape == (0, 1)   # asked for far more than the ring holds: no more is allocated
        seq.push([frames[0][0]])
        seq.push([frames[0][1]])
        one = seq.read_trajectory(3)
        assert one.shape == (1, 1)
        # after a step: refused, on or off, and the trajectory goes on as it was
        assert L.stvo_seq_set_trajectory(seq.h, C.byref(prm), 1) == INVALID
        assert L.stvo_seq_set_trajectory(seq.h, None, 1) == INVALID
        assert seq.read_trajectory(3).tobytes() == one.tobytes()
        seq.push([frames[0][2]])
        two = seq.read_trajectory(3)
        assert two.shape == (2, 1) and two[0].tobytes() == one[0].tobytes() and two[1][0]["frame"] == 2
    finally:
        seq.close()
