"""The FLD key-line detector on the GPU (csrc/fld_kernels.hip, stvo_fld_*) against the CPU statement tests/cpp/fld_ref.c, bit for bit:
the edge map, the raw segments in detection order, the key-lines (end points, angle, numOfPixels) and their responses; then images
to poses with FLD key-lines through ImagePipeline(fld=...) and through the handler mirror's app (use_fld_lines : true)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fld_statement
import np_model
import pipeline_ref
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_handler import APP, compare
from test_gpu_images import oracle_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stmt():
    return fld_statement.load()


def same_f32(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_batch(ctx, stmt, imgs, L, nfeatures=300, K=512):
    """Every image of the batch against the statement; returns the segments found per image."""
    from stvo_amd import capi
    imgs = np.ascontiguousarray(imgs, np.uint8)
    B, rows, cols = imgs.shape
    fld = capi.Fld(ctx, B, cols, rows, capi.fld_params(L, nfeatures=nfeatures), max_keylines=K)
    try:
        kls = fld.detect(imgs)  # the first call of a new detector
        counts = fld.counts()
        edges = fld.edges(imgs)
        segs, nseg = fld.segments(imgs)
    finally:
        fld.close()
    found = []
    for b in range(B):
        assert np.array_equal(edges[b], stmt.edges(imgs[b])), b
        ref = stmt.segments(imgs[b], L)
        assert nseg[b] == len(ref) and counts[b] == len(ref), (b, nseg[b], counts[b], len(ref))
        assert same_f32(segs[b], ref[:8192]), b
        rec, resp, nfound = stmt.keylines(imgs[b], L, nfeatures, K)
        got, gresp = kls[b]
        assert len(got) == len(rec), (b, len(got), len(rec))
        assert got.tobytes() == rec.tobytes(), b
        assert same_f32(gresp, resp), b
        found.append(len(ref))
    return found


def scene(seed, cols, rows):
    return synth.make_image(seed, cols, rows, n_rects=max(20, cols * rows // 500), n_discs=max(5, cols * rows // 2000))


@pytest.mark.parametrize("cols,rows", [(1241, 376), (752, 480), (640, 240), (333, 217), (1024, 1024)])
def test_fld_bit_exact_by_size(hip, stmt, cols, rows):
    L = int(0.025 * min(cols, rows))
    assert check_batch(hip, stmt, scene(cols + rows, cols, rows)[None], L)[0] > 20


@pytest.mark.parametrize("B", [1, 2, 16, 130])
def test_fld_bit_exact_by_batch(hip, stmt, B):
    imgs = np.stack([scene(100 + b, 320, 200) for b in range(B)])
    assert min(check_batch(hip, stmt, imgs, 5)) > 5


def test_fld_walk_edge_cases(hip, stmt):
    """A serpentine band (its boundary one component of ~129 k edge pixels, walked by one lane), thousands of dots (tiny
    components, far more than the walk's 1024 lanes), a blank image (no edge, no line)."""
    board = np.full((1024, 1024), 40, np.uint8)
    for k in range(64):
        board[16 * k:16 * k + 8, 8:1016] = 210
        x0 = 8 if k % 2 == 0 else 1008
        if k < 63:
            board[16 * k + 8:16 * k + 16, x0:x0 + 8] = 210
    dots = np.full((1024, 1024), 30, np.uint8)
    dots[3::5, 3::5] = 220
    blank = np.full((1024, 1024), 128, np.uint8)
    n = check_batch(hip, stmt, np.stack([board, dots, blank]), 9)
    assert n[0] > 100 and n[2] == 0
    assert np.count_nonzero(stmt.edges(dots)) > 100000


def test_fld_cuts(hip, stmt):
    """The top-N cut by length (nfeatures) and the capacity cut (nfeatures 0 against max_keylines 16: the 16 longest), with the
    count of what was found before."""
    from stvo_amd import capi
    img = scene(5, 640, 480)
    n = check_batch(hip, stmt, img[None], 12, nfeatures=10)[0]
    assert n > 40
    fld = capi.Fld(hip, 1, 640, 480, capi.fld_params(12, nfeatures=0), max_keylines=16)
    try:
        got = fld.detect(img[None])[0][0]
        assert len(got) == 16 and fld.counts()[0] == n
        want = stmt.keylines(img, 12, nfeatures=16)[0]
        assert got.tobytes() == want.tobytes()
    finally:
        fld.close()


def test_fld_refusals(hip):
    from stvo_amd import capi
    h = C.c_void_p()

    def rc(cols=640, rows=480, L=12, **kw):
        r = hip.lib.stvo_fld_create(hip.h, 1, cols, rows, 64, C.byref(capi.fld_params(L, **kw)), C.byref(h))
        if r == 0:
            hip.lib.stvo_fld_destroy(h)
        return r
    assert rc() == 0
    assert rc(do_merge=1) == -5
    assert rc(canny_aperture_size=5) == -5
    assert rc(canny_th2=100.0) == -5
    assert rc(cols=1025, rows=1024) == -5
    assert rc(L=0) == -1


def test_fld_two_detectors_at_once(hip, stmt):
    from stvo_amd import capi
    a, b = scene(21, 640, 240), scene(22, 752, 480)
    fa = capi.Fld(hip, 1, 640, 240, capi.fld_params(6, nfeatures=100))
    fb = capi.Fld(hip, 1, 752, 480, capi.fld_params(12, nfeatures=300))
    try:
        for _ in range(2):
            ga, gb = fa.detect(a[None])[0][0], fb.detect(b[None])[0][0]
            assert ga.tobytes() == stmt.keylines(a, 6, 100)[0].tobytes()
            assert gb.tobytes() == stmt.keylines(b, 12, 300)[0].tobytes()
    finally:
        fa.close()
        fb.close()


def fld_lines(oracle, stmt, img, L, nlines):
    rec, _, _ = stmt.keylines(img, L, nlines, 512)
    r5 = np.stack([rec["sx"], rec["sy"], rec["ex"], rec["ey"], rec["angle"]], axis=1).astype(np.float32)
    return np.ascontiguousarray(r5[:, :4]), np.ascontiguousarray(r5[:, 4]), oracle.lbd_compute(img, r5, rec["num_pixels"])


def test_images_to_poses_fld_lines(oracle, stmt):
    """ORB + FLD (+ top-N cut by length) + LBD on the device, the end points handed to stvo_seq_upload_dev, the per-frame pipeline
    with has_lines — against the CPU chain (ORB oracle, FLD statement -> oracle.lbd_compute -> oracle pipeline), pose for pose."""
    from stvo_amd import capi, images
    cam = dict(synth.KITTI_CAM, width=640, height=240)
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    B, nf, nlines = 2, 3, 100
    L = int(0.025 * min(cam["width"], cam["height"]))
    seqs = [synth.make_stereo_image_sequence(60 + b, nf, cam, shift_per_disp=0.3 - 0.05 * b) for b in range(B)]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    pipe = images.ImagePipeline(ctx, B, cam, mp, op, max_kp=2048, fld=capi.fld_params(L, nfeatures=nlines), max_kl=128)
    try:
        frames = [oracle_frames(oracle, seqs[b], pipe.orb.pattern()) for b in range(B)]
        for b in range(B):
            for fr, (left, right) in zip(frames[b], seqs[b]):
                fr["kl_l"], fr["ang_l"], fr["ldesc_l"] = fld_lines(oracle, stmt, left, L, nlines)
                fr["kl_r"], _, fr["ldesc_r"] = fld_lines(oracle, stmt, right, L, nlines)
                fr["oct_ll"] = np.zeros(len(fr["kl_l"]), np.int32)
        refs = [pipeline_ref.run_sequence(oracle, frames[b], cam, mp, op) for b in range(B)]
        n_lines_used = 0
        for k in range(nf):
            res, counts = pipe.push_images(np.stack([seqs[b][k][0] for b in range(B)]), np.stack([seqs[b][k][1] for b in range(B)]))
            if k == 0:
                continue
            for b in range(B):
                o, r = refs[b][k - 1], res[b]
                assert counts[b, 0] == o["n_stereo_pt"] and counts[b, 1] == o["n_stereo_ls"], (b, k, counts[b])
                assert r["n_matched_pt"] == o["n_matched_pt"] and r["n_matched_ls"] == o["n_matched_ls"]
                assert r["status"] == o["status"] and r["path"] == o["path"] and tuple(r["iters"]) == o["iters"]
                assert r["n_inliers_pt"] == o["n_inliers_pt"] and r["n_inliers_ls"] == o["n_inliers_ls"]
                T = r["T"].reshape(4, 4)
                assert np_model.rot_angle(T[:3, :3], o["T"][:3, :3]) < 1e-4 and np.linalg.norm(T[:3, 3] - o["T"][:3, 3]) < 1e-3
                assert np.allclose(T, o["T"], atol=1e-8)
                n_lines_used += r["n_matched_ls"]
        assert n_lines_used > 0
    finally:
        pipe.close()
        ctx.close()


def test_image_entry_points_fld_lines(tmp_path, oracle, stmt):
    """imagesStVO_synth -c cfg.yaml with use_fld_lines : true: the handler mirror's detectStereoLines takes the FLD branch
    (length_threshold = (int)(min_line_length x min(cols, rows)), nfeatures = lsd_nfeatures) — against the CPU chain."""
    cam = dict(synth.KITTI_CAM, width=640, height=240)
    pairs = synth.make_stereo_image_sequence(91, 4, cam)
    seq = str(tmp_path / "img.bin"); res_path = str(tmp_path / "res.bin")
    synth.write_image_sequence(seq, pairs, cam)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("use_fld_lines : true\n")
    p = subprocess.run([APP, seq, res_path, "--preset", "kitti", "-c", str(cfg)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr + p.stdout
    res = synth.read_results(res_path)
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    fast = dict(adaptive=True, th0=20, mn=7, mx=30, inc=5, feat=50, err=0.5)
    pattern = oracle.orb_default_pattern()
    L, nlines = int(0.025 * min(cam["width"], cam["height"])), 100
    frames, th, ref = [], fast["th0"], []
    for k, (left, right) in enumerate(pairs):
        l = oracle.orb_detect_levels(left, nfeatures=2000, nlevels=1, fast_th=th, pattern=pattern)
        r = oracle.orb_detect_levels(right, nfeatures=2000, nlevels=1, fast_th=th, pattern=pattern)
        kl_l, ang_l, ld_l = fld_lines(oracle, stmt, left, L, nlines)
        kl_r, _, ld_r = fld_lines(oracle, stmt, right, L, nlines)
        assert len(kl_l) > 20 and len(kl_r) > 20
        frames.append(dict(kp_l=l["kp"], oct_l=l["octave"], desc_l=l["desc"], kp_r=r["kp"], desc_r=r["desc"], kl_l=kl_l,
                           oct_ll=np.zeros(len(kl_l), np.int32), ldesc_l=ld_l, kl_r=kl_r, ldesc_r=ld_r, ang_l=ang_l))
        if k:
            ref = pipeline_ref.run_sequence(oracle, frames, cam, mp, op, fast=fast)
            th = ref[-1]["fast"]
    compare(res, ref)
    assert any(r["ints"][7] > 0 for r in res[1:])  # matched key-lines took part


def test_fld_fuzz_short(hip, stmt):
    """Random sizes, contents, length thresholds, budgets and capacities, seeded and short."""
    rng = np.random.default_rng(2024)
    for case in range(12):
        cols, rows, B = int(rng.integers(16, 700)), int(rng.integers(16, 500)), int(rng.integers(1, 4))
        imgs = []
        for b in range(B):
            kind = (case + b) % 3
            if kind == 0:
                imgs.append(scene(int(rng.integers(1 << 30)), cols, rows))
            elif kind == 1:
                imgs.append(rng.integers(0, 256, (rows, cols)).astype(np.uint8))
            else:
                blocks = rng.integers(0, 256, (rows // 8 + 1, cols // 8 + 1))
                imgs.append(np.kron(blocks, np.ones((8, 8)))[:rows, :cols].astype(np.uint8))
        check_batch(hip, stmt, np.stack(imgs), int(rng.integers(1, 40)), nfeatures=int(rng.choice([0, 5, 50, 300])),
                    K=int(rng.choice([8, 64, 512])))
