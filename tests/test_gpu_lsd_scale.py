"""LSD key-lines at any lsd_scale on the GPU: the scaled image for every blur radius 0 .. 15 (lsd_scale_kernels.hip; radius 3 keeps
the kernels of tests/test_gpu_lsd.py) bit for bit against the numpy statement of tests/lsd_scale_statement.py, the segments against
the detector composed from that statement and the oracle at scale 1, the wrapper's key-lines, and the way the scale travels through
ImagePipeline and the handler mirror's yaml."""
import subprocess

import numpy as np
import pytest

import lsd_scale_statement as st
import pipeline_ref
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_handler import APP, compare

pytestmark = pytest.mark.gpu

SIZES = [(97, 61),    # odd, no multiple of 4 or of the tile
         (36, 33),    # radius 15 is nearly the image: repeated reflection
         (260, 37)]   # wide: crosses tile seams of the source and of the scaled image


def scene(cols, rows, seed=8):
    return synth.make_image(seed, cols, rows, n_rects=30, n_discs=0)


def three_images(cols, rows, seed):
    rng = np.random.default_rng(seed)
    return np.stack([scene(cols, rows, seed), rng.integers(0, 256, (rows, cols), dtype=np.uint8),
                     np.kron(rng.integers(0, 256, (rows // 4 + 1, cols // 4 + 1)), np.ones((4, 4)))[:rows, :cols].astype(np.uint8)])


@pytest.mark.parametrize("scale,sigma_scale,radius", st.PAIRS)
def test_scaled_image_bit_exact(hip, oracle, scale, sigma_scale, radius):
    """Three different images per batch (batch strides), three sizes, every radius but 3: blur -> bytes -> resize, bit for bit."""
    from stvo_amd import capi
    for cols, rows in SIZES:
        imgs = three_images(cols, rows, 11 + radius)
        lsd = capi.Lsd(hip, 3, cols, rows, capi.lsd_params(scale=scale, sigma_scale=sigma_scale), max_keylines=64)
        try:
            assert lsd.geometry["radius"] == radius
            got = lsd.scaled_image(imgs)
            for b in range(3):
                want = st.scaled_image(oracle, imgs[b], scale, sigma_scale)
                assert got[b].shape == want.shape and want.size > 0
                assert np.array_equal(got[b], want), (cols, rows, b, int(np.sum(got[b] != want)))
        finally:
            lsd.close()


@pytest.mark.parametrize("scale,sigma_scale,white", [(0.65, 0.6, 255), (0.22, 0.8, 247)])
def test_scaled_image_clamp_and_low_sum(hip, oracle, scale, sigma_scale, white):
    """Weights adding up to 259: an all-255 image gives 261 before the clamp, 255 after it; to 252: it comes out as 247."""
    from stvo_amd import capi
    cols, rows = 97, 61
    imgs = np.stack([np.full((rows, cols), 255, np.uint8), np.zeros((rows, cols), np.uint8)])
    lsd = capi.Lsd(hip, 2, cols, rows, capi.lsd_params(scale=scale, sigma_scale=sigma_scale), max_keylines=64)
    try:
        got = lsd.scaled_image(imgs)
        assert np.array_equal(got[0], st.scaled_image(oracle, imgs[0], scale, sigma_scale))
        assert np.all(got[0] == white) and np.all(got[1] == 0)
    finally:
        lsd.close()


def test_scaled_image_radius_3_and_scale_1_are_what_they_were(hip, oracle):
    """The test hook on the routes that existed: radius 3 (the 7 x 7 kernel + the resize kernel) and scale 1 (the input itself)."""
    from stvo_amd import capi
    cols, rows = 97, 61
    imgs = three_images(cols, rows, 5)
    for scale in (1.2, 0.8, 1.0):
        lsd = capi.Lsd(hip, 3, cols, rows, capi.lsd_params(scale=scale), max_keylines=64)
        try:
            got = lsd.scaled_image(imgs)
            for b in range(3):
                assert np.array_equal(got[b], st.scaled_image(oracle, imgs[b], scale, 0.6))
        finally:
            lsd.close()


# what the statement finds in scene(cols, rows) at the coarsest pairs is 5 (97 x 61) and 42 (320 x 200) segments: every comparison
# below is between lists at least this long
MIN_SEGMENTS = {(97, 61): 5, (320, 200): 40}


@pytest.mark.parametrize("scale,sigma_scale", [(s, ss) for s, ss, _ in st.PAIRS] + [(2.0, 1.0), (0.6, 0.6)])
def test_segments_against_the_composed_statement(hip, oracle, scale, sigma_scale):
    """Count and order for every pair; coordinates bit for bit at 0.5, 0.25 and 2.0, within 2^-23 relative elsewhere.  B = 1 and
    B = 3: many waves per image."""
    from stvo_amd import capi
    for cols, rows in MIN_SEGMENTS:
        imgs = np.stack([scene(cols, rows), scene(cols, rows, 9), scene(cols, rows, 7)])
        want = [st.segments(oracle, im, scale, sigma_scale) for im in imgs]
        assert len(want[0]) >= MIN_SEGMENTS[(cols, rows)]
        for B in (1, 3):
            lsd = capi.Lsd(hip, B, cols, rows, capi.lsd_params(min_length=4.0, nfeatures=0, scale=scale, sigma_scale=sigma_scale), max_keylines=512)
            try:
                segs, n = lsd.segments(imgs[:B])
                for b in range(B):
                    assert n[b] == len(want[b])
                    st.same_segments(segs[b], want[b], scale)
            finally:
                lsd.close()


def test_segments_one_wave_per_image(hip, oracle):
    """B = 130: beyond the many-waves form, every image on one wavefront."""
    from stvo_amd import capi
    cols, rows, B = 97, 61, 130
    base = [scene(cols, rows, 7 + i) for i in range(5)]
    want = [st.segments(oracle, im, 0.5, 0.6) for im in base]
    assert min(len(w) for w in want) >= 5
    lsd = capi.Lsd(hip, B, cols, rows, capi.lsd_params(min_length=4.0, nfeatures=0, scale=0.5), max_keylines=128)
    try:
        segs, n = lsd.segments(np.stack([base[b % 5] for b in range(B)]))
        for b in range(B):
            assert n[b] == len(want[b % 5]) and np.array_equal(segs[b], want[b % 5]), b
    finally:
        lsd.close()


def test_segments_refine_std_at_half_scale(hip, oracle):
    from stvo_amd import capi
    cols, rows = 320, 200
    imgs = np.stack([scene(cols, rows), scene(cols, rows, 9)])
    lsd = capi.Lsd(hip, 2, cols, rows, capi.lsd_params(min_length=4.0, nfeatures=0, scale=0.5, refine=1), max_keylines=512)
    try:
        segs, n = lsd.segments(imgs)
        for b in range(2):
            want = st.segments(oracle, imgs[b], 0.5, 0.6, refine=1)
            assert len(want) >= 40 and n[b] == len(want) and np.array_equal(segs[b], want)
    finally:
        lsd.close()


@pytest.mark.parametrize("nfeatures", [0, 10])
def test_keylines_are_the_wrapper_of_the_devices_segments(hip, oracle, nfeatures):
    """Lsd.detect at 0.5 against the wrapper stated in numpy (checkLineExtremes, length, min_length, numOfPixels, response, a stable
    top-N) applied to the device's own segments."""
    from stvo_amd import capi
    cols, rows = 320, 200
    imgs = np.stack([scene(cols, rows), scene(cols, rows, 9)])
    lsd = capi.Lsd(hip, 2, cols, rows, capi.lsd_params(min_length=4.0, nfeatures=nfeatures, scale=0.5), max_keylines=512)
    try:
        segs, n = lsd.segments(imgs)
        dets = lsd.detect(imgs)
        for b in range(2):
            ref = st.keylines(oracle, segs[b], cols, rows, 4.0, nfeatures)
            assert len(ref) == (10 if nfeatures else len(ref)) and len(ref) >= 10
            st.check_keylines(dets[b], ref)
    finally:
        lsd.close()


def test_image_pipeline_at_half_scale(oracle):
    """ImagePipeline(lsd = scale 0.5), B = 2, two steps: pose results and counts byte for byte what Sequences gives when it is fed
    what Orb, Lsd and Lbd return one by one for the same parameters (end points as stvo_keylines_xy_dev lays them out: sx, sy, ex, ey)."""
    from stvo_amd import capi, images
    cam = dict(synth.KITTI_CAM, width=640, height=240)
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    B, nf, M = 2, 3, 128
    prm = capi.lsd_params(min_length=0.025 * 240, nfeatures=100, scale=0.5)
    seqs = [synth.make_stereo_image_sequence(60 + b, nf, cam, shift_per_disp=0.3 - 0.05 * b) for b in range(B)]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    pipe = images.ImagePipeline(ctx, B, cam, mp, op, max_kp=2048, lsd=prm, max_kl=M)
    orb = capi.Orb(ctx, 2 * B, 640, 240, 2048)
    lsd = capi.Lsd(ctx, 2 * B, 640, 240, prm, max_keylines=M)
    lbd = capi.Lbd(ctx, 2 * B, 640, 240, max_keylines=M)
    seq = capi.Sequences(ctx, B, 2048, M, cam, mp, op)
    try:
        assert pipe.lsd.geometry["radius"] == 5
        n_lines = 0
        for k in range(nf):
            left, right = np.stack([seqs[b][k][0] for b in range(B)]), np.stack([seqs[b][k][1] for b in range(B)])
            res, counts = pipe.push_images(left, right)
            both = np.concatenate([left, right])
            pts, lines = orb.detect(both), lsd.detect(both)
            r5 = [np.stack([kl[f] for f in ("sx", "sy", "ex", "ey", "angle")], axis=1).astype(np.float32) for kl, _ in lines]
            ld = lbd.compute(both, r5, [kl["num_pixels"] for kl, _ in lines])
            frames = [dict(kp_l=pts[b]["kp"], oct_l=pts[b]["octave"], desc_l=pts[b]["desc"], kp_r=pts[B + b]["kp"], desc_r=pts[B + b]["desc"],
                           kl_l=r5[b][:, :4], oct_ll=np.zeros(len(r5[b]), np.int32), ldesc_l=ld[b], kl_r=r5[B + b][:, :4], ldesc_r=ld[B + b])
                      for b in range(B)]
            res2, counts2 = seq.push(frames)
            n_lines += sum(len(r) for r in r5)
            assert np.array_equal(counts, counts2), k
            assert res.tobytes() == res2.tobytes(), k
        assert n_lines >= 2 * B * 20 * nf and int(np.sum(res["n_matched_ls"])) > 0
    finally:
        seq.close(); lbd.close(); lsd.close(); orb.close(); pipe.close(); ctx.close()


def test_image_entry_points_at_half_scale(tmp_path, hip, oracle):
    """lsd_scale : 0.5 in the yaml (src/config.cpp:106) travels through Config and the handler mirror to the detector: the app's
    results against the CPU chain fed with the key-lines of capi.Lsd at that scale (ORB and LBD from their oracles)."""
    from stvo_amd import capi
    cam = dict(synth.KITTI_CAM, width=640, height=240)
    pairs = synth.make_stereo_image_sequence(91, 4, cam)
    seq = str(tmp_path / "img.bin"); res_path = str(tmp_path / "res.bin")
    synth.write_image_sequence(seq, pairs, cam)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("lsd_scale : 0.5\n")
    p = subprocess.run([APP, seq, res_path, "--preset", "kitti", "-c", str(cfg)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr + p.stdout
    res = synth.read_results(res_path)
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=1)
    fast = dict(adaptive=True, th0=20, mn=7, mx=30, inc=5, feat=50, err=0.5)
    pattern = oracle.orb_default_pattern()
    lsd = capi.Lsd(hip, 2, 640, 240, capi.lsd_params(min_length=0.025 * 240, nfeatures=100, scale=0.5), max_keylines=512)
    try:
        frames, th, ref = [], fast["th0"], []
        for k, (left, right) in enumerate(pairs):
            l = oracle.orb_detect_levels(left, nfeatures=2000, nlevels=1, fast_th=th, pattern=pattern)
            r = oracle.orb_detect_levels(right, nfeatures=2000, nlevels=1, fast_th=th, pattern=pattern)
            kls = [d[0] for d in lsd.detect(np.stack([left, right]))]
            r5 = [np.stack([kl[f] for f in ("sx", "sy", "ex", "ey", "angle")], axis=1).astype(np.float32) for kl in kls]
            ld = [oracle.lbd_compute(img, rec, kl["num_pixels"]) for img, rec, kl in zip((left, right), r5, kls)]
            assert len(r5[0]) > 20 and len(r5[1]) > 20
            frames.append(dict(kp_l=l["kp"], oct_l=l["octave"], desc_l=l["desc"], kp_r=r["kp"], desc_r=r["desc"],
                               kl_l=np.ascontiguousarray(r5[0][:, :4]), oct_ll=np.zeros(len(r5[0]), np.int32), ldesc_l=ld[0],
                               kl_r=np.ascontiguousarray(r5[1][:, :4]), ldesc_r=ld[1], ang_l=np.ascontiguousarray(r5[0][:, 4])))
            if k:
                ref = pipeline_ref.run_sequence(oracle, frames, cam, mp, op, fast=fast)
                th = ref[-1]["fast"]
    finally:
        lsd.close()
    compare(res, ref)
    assert any(r["ints"][7] > 0 for r in res[1:])  # matched key-lines took part
    # ... and the scale changes the key-lines of these images (the yaml key was not ignored)
    plain = oracle.lsd_detect(pairs[0][0], oracle.lsd_opts(min_length=0.025 * 240, nfeatures=100))
    assert len(plain) != len(frames[0]["kl_l"]) or not np.array_equal(plain["sx"], frames[0]["kl_l"][:, 0])


def test_radius_16_is_refused(hip):
    from stvo_amd import capi
    from stvo_amd.capi import StvoError
    assert st.sigma_radius(0.2, 0.85)[1] == 16
    with pytest.raises(StvoError, match=r"\(-5\)"):   # STVO_ERR_UNSUPPORTED
        capi.Lsd(hip, 1, 320, 200, capi.lsd_params(scale=0.2, sigma_scale=0.85))
    lsd = capi.Lsd(hip, 1, 320, 200, capi.lsd_params(scale=0.25, sigma_scale=1.0))   # radius 15 is built
    lsd.close()
