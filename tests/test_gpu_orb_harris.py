"""orb_score 0 on the GPU (stvo_orb_set_score_type, csrc/orb_kernels.hip: orb_harris_kernel + the float cut of orb_order_kernel) against
the expectation composed from the unchanged ORB oracle and the numpy statement of HarrisResponses (tests/np_harris.py): coordinates,
response bits, angle, octave and descriptor BIT-EXACT; the switch between the two rankings on one detector; the mode through the
handler mirror (orb_score in a config file) and through ImagePipeline(orb_score=0)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import harris_cases
import np_harris
import np_model
import pipeline_ref
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "stvo-pl_amd", "bin", "imagesStVO_synth")
GOLD = os.path.join(os.path.dirname(__file__), "golden", "orb_goldens.npz")
KEYS = ("kp", "response", "angle", "desc", "octave")


def same(got, ref, keys=KEYS):
    for k in keys:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), k   # bitwise, floats included


@pytest.mark.parametrize("name", sorted(harris_cases.CASES))
def test_orb_harris_bit_exact(hip, oracle, name):
    from stvo_amd import capi
    cols, rows, nf, nlev, sf, th, seeds, _ = harris_cases.CASES[name]
    imgs = harris_cases.images(name)
    B = len(imgs)
    orb = capi.Orb(hip, B, cols, rows, max_keypoints=4096, nfeatures=nf, fast_threshold=th, nlevels=nlev, scale_factor=sf, score=0)
    try:
        out = orb.detect(imgs)
        for b in range(B):
            info = []
            ref = np_harris.detect_levels(oracle, imgs[b], nf, nlev, sf, th, cap=4096, info=info)
            assert all(lv["n_cand"] > lv["n"] and lv["differs"] for lv in info) and len(info) == nlev
            print(name, b, "key-points", len(ref["kp"]), [(lv["n"], lv["n_cand"], lv["n_keep"]) for lv in info])
            same(out[b], ref)
            assert out[b]["n_total"] == ref["n_total"]
            assert np.all(np.diff(ref["octave"]) >= 0) and len(np.unique(ref["octave"])) == nlev
        again = orb.detect(imgs[::-1].copy())   # the scratch (histograms, candidate counts, response words) is reused
        for b in range(B):
            same(again[b], out[B - 1 - b])
    finally:
        orb.close()


def test_orb_harris_capacity_and_few_corners(hip, oracle):
    """The output capacity cuts the row-major order (n_total reports what passed the Harris cut); a budget beyond the corners there are
    keeps them all, with their Harris responses."""
    from stvo_amd import capi
    img = synth.make_image(307, cols=640, rows=200, n_rects=120, n_discs=30, noise=4.0)
    for nf, th, cap in ((300, 12, 128), (5000, 35, 1024), (50, 60, 64)):
        orb = capi.Orb(hip, 1, 640, 200, max_keypoints=cap, nfeatures=nf, fast_threshold=th, score=0)
        try:
            got = orb.detect(img[None])[0]
            ref = np_harris.detect_levels(oracle, img, nf, 1, 1.2, th, cap=cap)
            same(got, ref)
            assert got["n_total"] == ref["n_total"]
        finally:
            orb.close()


def test_orb_harris_masses_of_equal_responses(hip, oracle):
    """A dot lattice: thousands of key-points with one FAST score and one Harris response.  Both cuts keep all their ties — far more than
    the ordering kernel sorts in LDS — and the output is the first max_keypoints of the row-major order, n_total the uncapped count."""
    from stvo_amd import capi
    cols, rows = 1024, 512
    yy, xx = np.mgrid[0:rows, 0:cols]
    img = np.where((yy % 7 == 0) & (xx % 7 == 0), 200, 40).astype(np.uint8)
    full = np_harris.detect_levels(oracle, img, 200, 1, 1.2, 20, cap=1 << 16)
    assert full["n_total"] > 4096 and len(np.unique(full["response"])) <= 4
    for cap in (4096, 1000):
        orb = capi.Orb(hip, 2, cols, rows, max_keypoints=cap, nfeatures=200, fast_threshold=20, score=0)
        try:
            out = orb.detect(np.stack([img, img[::-1].copy()]))
            same(out[0], {k: full[k][:cap] for k in KEYS})
            assert out[0]["n_total"] == full["n_total"] and len(out[0]["kp"]) == cap
            same(out[1], np_harris.detect_levels(oracle, img[::-1].copy(), 200, 1, 1.2, 20, cap=cap))
        finally:
            orb.close()


def test_orb_score_switching_and_fast_goldens(hip, oracle):
    """One detector FAST -> Harris -> FAST: the third run is the first again, bit for bit, and score type 1 still gives the committed
    goldens (the parent's FAST output) on their inputs; a value that is neither 0 nor 1 is refused and changes nothing."""
    from stvo_amd import capi
    g = np.load(GOLD)
    for c, (seed, cols, rows, nf, th) in enumerate(g["cases"]):
        img = g[f"img_{c}"]
        orb = capi.Orb(hip, 1, int(cols), int(rows), max_keypoints=4096, nfeatures=int(nf), fast_threshold=int(th))
        try:
            first = orb.detect(img[None])[0]
            for k in ("kp", "response", "angle", "desc"):
                assert np.array_equal(first[k], g[f"{k}_{c}"]), (c, k)
            orb.set_score_type(0)
            harris = orb.detect(img[None])[0]
            same(harris, np_harris.detect_levels(oracle, img, int(nf), 1, 1.2, int(th), cap=4096))
            for bad in (2, -1, 7):
                with pytest.raises(capi.StvoError):
                    orb.set_score_type(bad)
            same(orb.detect(img[None])[0], harris)   # still Harris
            orb.set_score_type(1)
            third = orb.detect(img[None])[0]
            same(third, first)
            assert third["n_total"] == first["n_total"]
            for k in ("kp", "response", "angle", "desc"):
                assert np.array_equal(third[k], g[f"{k}_{c}"]), (c, k)
        finally:
            orb.close()
    with pytest.raises(capi.StvoError):
        capi.Orb(hip, 1, 640, 200, score=3)


def test_orb_harris_plain_entry_point_and_levels_switch(hip, oracle):
    """stvo_orb_detect (no octave, no n_total) in Harris mode, and the switch on a four-level detector with a batch."""
    from stvo_amd import capi
    cols, rows, nf, nlev, sf, th, seeds, _ = harris_cases.CASES["euroc_4levels_batch"]
    imgs = harris_cases.images("euroc_4levels_batch")
    B, K = len(imgs), 2048
    orb = capi.Orb(hip, B, cols, rows, max_keypoints=K, nfeatures=nf, fast_threshold=th, nlevels=nlev, scale_factor=sf)
    try:
        fast = orb.detect(imgs)
        for b in range(B):
            same(fast[b], oracle.orb_detect_levels(imgs[b], nfeatures=nf, nlevels=nlev, scale_factor=sf, fast_th=th, cap=K))
        orb.set_score_type(0)
        kp = np.zeros((B, K, 2), np.float32); resp = np.zeros((B, K), np.float32); ang = np.zeros((B, K), np.float32)
        desc = np.zeros((B, K, 32), np.uint8); n = np.zeros(B, np.int32)
        hip._chk(hip.lib.stvo_orb_detect(orb.h, imgs.reshape(-1), kp.reshape(-1), resp.reshape(-1), ang.reshape(-1), desc.reshape(-1), n))
        for b in range(B):
            ref = np_harris.detect_levels(oracle, imgs[b], nf, nlev, sf, th, cap=K)
            got = dict(kp=kp[b, :n[b]], response=resp[b, :n[b]], angle=ang[b, :n[b]], desc=desc[b, :n[b]])
            same(got, ref, ("kp", "response", "angle", "desc"))
        orb.set_score_type(1)
        back = orb.detect(imgs)
        for b in range(B):
            same(back[b], fast[b])
    finally:
        orb.close()


def harris_frames(oracle, pairs, pattern, nfeatures, nlevels, th=20, lines_of=None):
    frames = []
    z4 = np.zeros((0, 4), np.float32); zd = np.zeros((0, 32), np.uint8)
    for left, right in pairs:
        l = np_harris.detect_levels(oracle, left, nfeatures, nlevels, 1.2, th, pattern=pattern)
        r = np_harris.detect_levels(oracle, right, nfeatures, nlevels, 1.2, th, pattern=pattern)
        fr = dict(kp_l=l["kp"], oct_l=l["octave"], desc_l=l["desc"], kp_r=r["kp"], desc_r=r["desc"], kl_l=z4, oct_ll=np.zeros(0, np.int32),
                  ldesc_l=zd, kl_r=z4, ldesc_r=zd, ang_l=np.zeros(0, np.float32))
        if lines_of is not None:
            kl_l, ang_l, ld_l = lines_of(left)
            kl_r, _, ld_r = lines_of(right)
            fr.update(kl_l=kl_l, oct_ll=np.zeros(len(kl_l), np.int32), ldesc_l=ld_l, kl_r=kl_r, ldesc_r=ld_r, ang_l=ang_l)
        frames.append(fr)
    return frames


@pytest.mark.parametrize("preset,nlevels,nfeat", [("kitti", 1, 500), ("euroc", 4, 800)])
def test_handler_reads_orb_score_from_the_config_file(tmp_path, oracle, preset, nlevels, nfeat):
    """`orb_score : 0` in the file given with -c reaches the handler's detector (Config::orbScore -> stvo_orb_set_score_type): images in,
    key-points (Harris-ranked) and key-lines on the GPU, the usual path — against the CPU chain with the composed Harris expectation,
    with the adaptive FAST threshold the previous frame left behind."""
    import test_gpu_handler as tgh
    cam = dict(synth.KITTI_CAM if preset == "kitti" else synth.EUROC_CAM, width=640, height=240)
    pairs = synth.make_stereo_image_sequence(91, 4, cam)
    seq = str(tmp_path / "img.bin"); res_path = str(tmp_path / "res.bin")
    synth.write_image_sequence(seq, pairs, cam)
    cfg = tmp_path / "cfg.yaml"
    # (a budget below the corners of these small images, so that the Harris cut has something to drop)
    cfg.write_text(f"orb_nfeatures : {nfeat}\norb_score : 0   # 0 - HARRIS | 1 - FAST\n")
    p = subprocess.run([APP, seq, res_path, "--preset", preset, "-c", str(cfg)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr + p.stdout
    res = synth.read_results(res_path)
    mp = match_params(preset); op = opt_params(preset, has_lines=1)
    nlines = {"kitti": 100, "euroc": 300}[preset]
    fast = dict(adaptive=True, th0=20, mn=7, mx=30, inc=5, feat=50, err=0.5) if preset == "kitti" else \
        dict(adaptive=True, th0=20, mn=5, mx=50, inc=5, feat=50, err=0.5)
    pattern = oracle.orb_default_pattern()
    lopts = oracle.lsd_opts(min_length=0.025 * min(cam["width"], cam["height"]), nfeatures=nlines)

    def lines_of(img):
        kl = oracle.lsd_detect(img, lopts)
        rec = np.stack([kl["sx"], kl["sy"], kl["ex"], kl["ey"], kl["angle"]], axis=1).astype(np.float32)
        return np.ascontiguousarray(rec[:, :4]), np.ascontiguousarray(rec[:, 4]), oracle.lbd_compute(img, rec, kl["num_pixels"])

    frames, th, ref, differs = [], fast["th0"], [], False
    for k, pair in enumerate(pairs):
        frames += harris_frames(oracle, [pair], pattern, nfeat, nlevels, th, lines_of)
        plain = oracle.orb_detect_levels(pair[0], nfeatures=nfeat, nlevels=nlevels, fast_th=th, pattern=pattern)
        differs = differs or not (plain["kp"].shape == frames[-1]["kp_l"].shape and np.array_equal(plain["kp"], frames[-1]["kp_l"]))
        if k:
            ref = pipeline_ref.run_sequence(oracle, frames, cam, mp, op, fast=fast)
            th = ref[-1]["fast"]
    assert differs   # the key changes the key-points of these images: it was not ignored on either side
    tgh.compare(res, ref)
    assert sum(r["ints"][1] == 0 for r in res) >= 2


def test_image_pipeline_with_harris_ranking(oracle):
    """ImagePipeline(orb_score=0): images in, poses out on the device (stvo_orb_detect_levels_dev in Harris mode feeding the resident
    pipeline) against the CPU chain composed from the oracle and the numpy Harris statement, pose for pose."""
    from stvo_amd import capi, images
    cam = dict(synth.KITTI_CAM, width=640, height=240)
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=0)
    B, nf, nfeat = 2, 4, 700
    seqs = [synth.make_stereo_image_sequence(50 + b, nf, cam, shift_per_disp=0.3 - 0.05 * b) for b in range(B)]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    pipe = images.ImagePipeline(ctx, B, cam, mp, op, max_kp=2048, nfeatures=nfeat, orb_score=0)
    n_committed = 0
    try:
        pattern = pipe.orb.pattern()
        frames = [harris_frames(oracle, seqs[b], pattern, nfeat, 1) for b in range(B)]
        plain = oracle.orb_detect_levels(seqs[0][0][0], nfeatures=nfeat, nlevels=1, pattern=pattern)
        assert not (plain["kp"].shape == frames[0][0]["kp_l"].shape and np.array_equal(plain["kp"], frames[0][0]["kp_l"]))
        refs = [pipeline_ref.run_sequence(oracle, frames[b], cam, mp, op) for b in range(B)]
        for k in range(nf):
            res, counts = pipe.push_images(np.stack([seqs[b][k][0] for b in range(B)]), np.stack([seqs[b][k][1] for b in range(B)]))
            if k == 0:
                continue
            for b in range(B):
                o, r = refs[b][k - 1], res[b]
                assert counts[b, 0] == o["n_stereo_pt"] and r["n_matched_pt"] == o["n_matched_pt"], (b, k, counts[b], o["n_stereo_pt"])
                assert r["status"] == o["status"] and r["path"] == o["path"] and tuple(r["iters"]) == o["iters"]
                assert r["n_inliers_pt"] == o["n_inliers_pt"]
                T = r["T"].reshape(4, 4)
                assert np_model.rot_angle(T[:3, :3], o["T"][:3, :3]) < 1e-4 and np.linalg.norm(T[:3, 3] - o["T"][:3, 3]) < 1e-3
                assert np.allclose(T, o["T"], atol=1e-8)
                n_committed += r["status"] == 0
        assert n_committed >= 3
    finally:
        pipe.close()
        ctx.close()


def test_randomised_harris_parity_short_run():
    import fuzz_orb_harris
    assert fuzz_orb_harris.main(["--seconds", "120", "--cases", "40", "--seed", "7"]) == 0
