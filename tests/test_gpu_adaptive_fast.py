"""The reference's adaptative_fast on the batched device path: a FAST threshold per image inside the ORB kernels
(stvo_orb_set_fast_thresholds[_dev]), updateFrame's rule as a kernel (stvo_fast_adapt_dev / stvo_seq_adapt_fast_dev), and
ImagePipeline(adaptive_fast=...) — images in, poses out, the threshold of every stream moving on the device — against the CPU chain of
tests/fast_adapt_cases.py (ORB oracle at the threshold the previous frame left, oracle-driven pipeline, the rule of pipeline_ref)."""
import numpy as np
import pytest

import fast_adapt_cases as fc
import np_fast_adapt
import np_harris
from stvo_amd import synth
from stvo_amd.ctypes_types import POSE_RESULT_DTYPE, match_params, opt_params

pytestmark = pytest.mark.gpu
KEYS = ("kp", "response", "angle", "desc", "octave")


def same(got, ref):
    for k in KEYS:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), k   # bitwise, floats included
    assert got["n_total"] == ref["n_total"]


# ---- 1. the detector alone ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nlevels,score", [(1, 1), (4, 1), (1, 0), (4, 0)])
def test_detector_threshold_per_image(hip, oracle, nlevels, score):
    import torch
    from stvo_amd import capi
    # a budget the corners of these images do not fill at most thresholds, so that every threshold gives another set of key-points
    # (at 1 the output capacity cuts; under the Harris ranking both of its cuts apply at 1 and 7)
    cols, rows, B, nf, K = 320, 200, 6, (600 if (score, nlevels) == (0, 1) else 2000), 2048
    imgs = np.stack([synth.make_image(900 + i, cols=cols, rows=rows, n_rects=90, n_discs=25, noise=4.0) for i in range(B)])
    cache = {}

    def ref(i, th):
        if (i, th) not in cache:
            cache[i, th] = np_harris.detect_levels(oracle, imgs[i], nf, nlevels, 1.2, th, cap=K, score=0) if score == 0 else \
                oracle.orb_detect_levels(imgs[i], nfeatures=nf, nlevels=nlevels, scale_factor=1.2, fast_th=th, cap=K)
            if "n_total" not in cache[i, th]:   # the ORB oracle reports no count: what it emits when nothing cuts its output
                cache[i, th]["n_total"] = len(oracle.orb_detect_levels(imgs[i], nfeatures=nf, nlevels=nlevels, scale_factor=1.2, fast_th=th,
                                                                       cap=1 << 16)["kp"])
        return cache[i, th]

    def check(out, ths):
        for i in range(B):
            r = ref(i, ths[i % len(ths)])
            for k in KEYS:
                assert out[i][k].shape == r[k].shape, (i, ths, k, out[i][k].shape, r[k].shape)
                assert np.array_equal(out[i][k].view(np.uint8), r[k].view(np.uint8)), (i, ths, k)
            assert out[i]["n_total"] == r["n_total"], (i, ths, out[i]["n_total"], r["n_total"])   # the uncapped count

    orb = capi.Orb(hip, B, cols, rows, max_keypoints=K, nfeatures=nf, fast_threshold=20, nlevels=nlevels, scale_factor=1.2, score=score)
    plain = capi.Orb(hip, B, cols, rows, max_keypoints=K, nfeatures=nf, fast_threshold=20, nlevels=nlevels, scale_factor=1.2, score=score)
    try:
        scalar = plain.detect(imgs)   # a detector that never had the array
        check(scalar, [20])
        full = [1, 7, 20, 21, 50, 254]
        orb.set_fast_thresholds(np.array(full, np.int32))
        out = orb.detect(imgs)
        check(out, full)
        print("nlevels", nlevels, "score", score, "key-points at", full, [len(o["kp"]) for o in out])
        for i in range(B):   # the thresholds bite on every image: a kernel that took another entry, or the scalar, would not pass
            assert len({len(ref(i, t)["kp"]) for t in full}) >= 5, (i, [len(ref(i, t)["kp"]) for t in full])
        orb.set_fast_thresholds(np.array([7, 20, 35], np.int32))       # images 3 .. 5 reuse entries 0 .. 2
        check(orb.detect(imgs), [7, 20, 35])
        orb.set_fast_thresholds(np.array([13], np.int32))
        check(orb.detect(imgs), [13])
        for bad in ([20] * 4, [20] * 12, [], [20, 0, 20], [20, 255]):    # n_th must divide B; host values are validated
            with pytest.raises(capi.StvoError):
                orb.set_fast_thresholds(np.array(bad, np.int32))
        check(orb.detect(imgs), [13])                                      # a refused call changes nothing
        # the device form: read when the detection runs, and clamped there (another kernel writes it: nothing validates it on the host)
        t = torch.tensor([0, 300, -5, 20, 255, 1], dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        orb.set_fast_thresholds(t)
        check(orb.detect(imgs), [1, 254, 1, 20, 254, 1])
        t.copy_(torch.tensor(full, dtype=torch.int32))                     # same pointer, new contents: no second call
        torch.cuda.synchronize()
        check(orb.detect(imgs), full)
        with pytest.raises(capi.StvoError):
            hip._chk(hip.lib.stvo_orb_set_fast_thresholds_dev(orb.h, t.data_ptr(), 4))
        orb.set_fast_threshold(20)
        orb.set_fast_thresholds(None)                                      # back to the scalar
        back = orb.detect(imgs)
        for i in range(B):
            for k in KEYS:
                assert np.array_equal(back[i][k].view(np.uint8), scalar[i][k].view(np.uint8)), (i, k)
            assert back[i]["n_total"] == scalar[i]["n_total"]
    finally:
        orb.close()
        plain.close()


# ---- 2. the rule alone -------------------------------------------------------------------------------------------------------

def rule_records():
    """32 pose results and start thresholds at the edges of the rule (kitti values: min 7, max 30, inc 5, feat 50)."""
    moved = np.eye(4); moved[0, 3] = 0.1
    rec = []

    def add(th=20, n=120, T=moved, err=0.1):
        rec.append((th, n, np.array(T, np.float64).reshape(16), err))

    for n in (49, 50, 99, 100, 150, 151, 200, 201, 1000):      # the rows of the rule
        add(n=n)
    add(T=np.eye(4))                                           # lost: DT == I, whatever err says
    for (i, j), v in (((0, 0), np.nextafter(1.0, 2.0)), ((0, 0), np.nextafter(1.0, 0.0)), ((2, 3), np.nextafter(0.0, 1.0))):
        T = np.eye(4); T[i, j] = v                             # one element off by one ulp: not the identity
        add(T=T)
    T = np.eye(4); T[1, 2] = -0.0                              # Eigen's == compares values: -0.0 is 0
    add(T=T)
    for err in (-1.0, 0.5, np.nextafter(0.5, 1.0)):            # err > 0.5f, strictly
        add(err=err)
    for err in (0.3, 0.30000001, 0.3000001):                   # 0.3f = 0.300000011920929 (the second parameter set)
        add(err=err)
    for th in (16, 17, 18):                                    # two steps down: cut at 7, exactly 7, 8
        add(th=th, n=49)
    for th in (11, 12, 13):                                    # one step down
        add(th=th, n=99)
    for th in (24, 25, 26):                                    # one step up: 29, exactly 30, cut at 30
        add(th=th, n=151)
    add(th=1, n=151)                                           # below min_th moving up: 6, not pulled up to 7
    add(th=50, n=99)                                           # above max_th moving down: 45, not pulled down to 30
    add(th=26, T=np.eye(4), n=1000)                            # lost beats the inlier count
    assert len(rec) == 32
    res = np.zeros(len(rec), POSE_RESULT_DTYPE)
    res["cov"] = np.nan; res["T_opt"] = np.nan                 # fields the rule must not read
    for b, (th, n, T, err) in enumerate(rec):
        res["T"][b] = T; res["err"][b] = err; res["n_inliers_pt"][b] = n
        res["status"][b] = 3 if err < 0 else 0
    return np.array([r[0] for r in rec], np.int32), res


@pytest.mark.parametrize("err_th", [0.5, 0.3])
def test_rule_alone_at_its_edges(hip, err_th):
    import torch
    from stvo_amd import capi
    th0, res = rule_records()
    prm = capi.fast_adapt_params("kitti", err_th=err_th)
    exp = np_fast_adapt.update_batch(th0, res, prm)
    assert len(set((exp - th0).tolist())) >= 5 and np.any(exp == 7) and np.any(exp == 30)
    if err_th == 0.3:
        assert np_fast_adapt.update_batch(th0, res, capi.fast_adapt_params("kitti")).tolist() != exp.tolist()
    d_res = torch.from_numpy(res.view(np.uint8).copy()).to("cuda:0")
    d_th = torch.from_numpy(th0.copy()).to("cuda:0")
    torch.cuda.synchronize()
    capi.fast_adapt_dev(hip, d_res, prm, d_th)
    hip.synchronize()
    got = d_th.cpu().numpy()
    assert got.tolist() == exp.tolist(), [(b, int(th0[b]), int(got[b]), int(exp[b])) for b in np.nonzero(got != exp)[0]]
    # B that is no multiple of the 64 lanes of its one workgroup, and more than one workgroup
    for B in (1, 70):
        idx = np.arange(B) % len(th0)
        d_res = torch.from_numpy(res[idx].view(np.uint8).copy()).to("cuda:0")
        d_th = torch.cat([torch.from_numpy(th0[idx].copy()), torch.full((3,), -77, dtype=torch.int32)]).to("cuda:0")
        torch.cuda.synchronize()
        capi.fast_adapt_dev(hip, d_res, prm, d_th[:B])
        hip.synchronize()
        got = d_th.cpu().numpy()
        assert got[:B].tolist() == exp[idx].tolist() and got[B:].tolist() == [-77] * 3   # nothing beyond B is touched


# ---- 3 - 5. the pipeline -----------------------------------------------------------------------------------------------------

def stacked(k, reps):
    imgs = fc.images()
    return (np.stack([imgs[s][k][0] for s in range(len(imgs))] * reps), np.stack([imgs[s][k][1] for s in range(len(imgs))] * reps))


def make_pipe(B, adaptive, fast_threshold=fc.TH0):
    from stvo_amd import capi, images
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        pipe = images.ImagePipeline(ctx, B, fc.CAM, match_params("kitti"), opt_params("kitti", has_lines=0), max_kp=fc.MAX_KP,
                                    nfeatures=fc.NFEATURES, fast_threshold=fast_threshold, adaptive_fast=adaptive)
    except Exception:
        ctx.close()
        raise
    return ctx, pipe


def check_frame(chain, k, res, counts, reps):
    S = len(chain)
    for b in range(S * reps):
        o, r = chain[b % S]["ref"][k - 1], res[b]
        assert counts[b, 0] == o["n_stereo_pt"] and r["n_matched_pt"] == o["n_matched_pt"], (b, k, counts[b], o["n_stereo_pt"], o["n_matched_pt"])
        assert r["status"] == o["status"] and r["path"] == o["path"] and tuple(r["iters"]) == o["iters"], (b, k)
        assert r["n_inliers_pt"] == o["n_inliers_pt"], (b, k)
        assert np.allclose(r["T"].reshape(4, 4), o["T"], atol=1e-8), (b, k)


@pytest.fixture(scope="module")
def stepwise(oracle):
    """Test 3 with B = 4 leaves the last frame's results and thresholds for test 4."""
    return {}


@pytest.mark.parametrize("reps", [1, 5])
def test_pipeline_frame_by_frame(oracle, stepwise, reps):
    """B = 4: the step writes its results into the pinned block (the pipeline's zero-copy form, chosen by the library for B <= 16 — a
    caller cannot choose it) and the rule reads them there; B = 20 (every stream five times): results in device memory."""
    chain = fc.cpu_chain(oracle)
    S = len(chain)
    B = S * reps
    ctx, pipe = make_pipe(B, fc.params())
    try:
        assert np.array_equal(pipe.orb.pattern().reshape(-1), oracle.orb_default_pattern().reshape(-1))
        assert pipe.fast_thresholds().tolist() == [fc.TH0] * B
        for k in range(fc.N_FRAMES):
            left, right = stacked(k, reps)
            res, counts = pipe.push_images(left, right)
            th = pipe.fast_thresholds()
            if k == 0:
                assert th.tolist() == [fc.TH0] * B   # initialize() has no updateFrame()
                continue
            check_frame(chain, k, res, counts, reps)
            assert th.tolist() == [chain[b % S]["after"][k - 1] for b in range(B)], (k, th.tolist())
        if reps == 1:
            stepwise["res"], stepwise["counts"], stepwise["th"] = res.copy(), counts.copy(), th.copy()
    finally:
        pipe.close()
        ctx.close()


def test_pipeline_no_host_in_the_loop(oracle, stepwise):
    """Six frames resident on the device, six enqueues back to back, ONE read: the last frame's results and the final thresholds depend
    on the whole threshold history, i.e. on every adapt kernel having run between its pose kernel and the next detection."""
    import torch
    chain = fc.cpu_chain(oracle)
    B = len(chain)
    ctx, pipe = make_pipe(B, fc.params())
    try:
        buf = torch.from_numpy(np.stack([np.concatenate(stacked(k, 1)) for k in range(fc.N_FRAMES)])).to("cuda:0")   # [6][2 B][rows][cols]
        torch.cuda.synchronize()
        frame_bytes = 2 * B * pipe.rows * pipe.cols
        for k in range(fc.N_FRAMES):
            pipe.enqueue(img_ptr=buf.data_ptr() + k * frame_bytes)
        res, counts = pipe.seq.read()
        th = pipe.fast_thresholds()
        check_frame(chain, fc.N_FRAMES - 1, res, counts, 1)
        assert th.tolist() == [c["after"][-1] for c in chain]
        if stepwise:   # (test 3 ran in this process) the same bits as frame by frame
            assert th.tolist() == stepwise["th"].tolist() and np.array_equal(counts, stepwise["counts"])
            for f in ("T", "err", "status", "path", "iters", "n_matched_pt", "n_inliers_pt"):
                assert np.array_equal(res[f], stepwise["res"][f]), f
    finally:
        pipe.close()
        ctx.close()


def test_nothing_changes_when_off(oracle):
    """adaptive_fast=None against a rule that can never move the threshold (min_th = max_th = 20): the same poses, bit for bit."""
    from stvo_amd import capi
    B = len(fc.STREAMS)
    outs = []
    for adaptive in (None, capi.fast_adapt_params("kitti", min_th=20, max_th=20)):
        ctx, pipe = make_pipe(B, adaptive)
        try:
            assert (pipe.fast_th is None) == (adaptive is None)
            frames = []
            for k in range(3):
                res, counts = pipe.push_images(*stacked(k, 1))
                frames.append((res.copy(), counts.copy()))
            if adaptive is not None:
                assert pipe.fast_thresholds().tolist() == [20] * B
            else:
                with pytest.raises(ValueError):
                    pipe.fast_thresholds()
            outs.append(frames)
        finally:
            pipe.close()
            ctx.close()
    for (ra, ca), (rb, cb) in zip(*outs):
        assert np.array_equal(ca, cb) and ra.tobytes() == rb.tobytes()
    assert any(r["status"] == 0 for r in outs[0][1][0])


def test_adapt_before_the_first_step_is_refused(hip):
    import torch
    from stvo_amd import capi
    seq = capi.Sequences(hip, 2, 256, 64, fc.CAM, match_params("kitti"), opt_params("kitti", has_lines=0))
    try:
        th = torch.full((2,), 20, dtype=torch.int32, device="cuda:0")
        with pytest.raises(capi.StvoError):
            seq.adapt_fast_dev(capi.fast_adapt_params("kitti"), th)
    finally:
        seq.close()
