"""orb_wta_k 2 / 3 / 4 and orb_patch_size 2 .. 63 on the GPU (stvo_orb_set_descriptor, csrc/orb_kernels.hip: orb_describe_wta_kernel)
against the plain statement tests/np_orb_wta.py on the planned images of tests/orb_wta_cases.py: key-points, order, responses, angles,
octaves, descriptors and counts BIT FOR BIT through every entry point; the default setting untouched by a round trip through another;
the effective pattern read back; refusals that change nothing; the keys through the handler mirror and ImagePipeline; a short
randomised pass.  tests/test_orb_wta_host.py checks on the CPU that every case sits on the edge it was planned for."""
import os
import subprocess

import numpy as np
import pytest

import np_model
import np_orb_wta as nw
import orb_wta_cases as wc
import pipeline_ref
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "stvo-pl_amd", "bin", "imagesStVO_synth")
CASES = {c["name"]: c for c in wc.all_cases()}
KEYS = ("kp", "response", "angle", "desc", "octave")


def same(got, ref, what, keys=KEYS):
    for k in keys:
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), (what, k)   # bitwise, floats included


def make_orb(hip, c, **kw):
    from stvo_amd import capi
    p = c["prm"]
    B, rows, cols = c["images"].shape
    orb = capi.Orb(hip, B, cols, rows, max_keypoints=p["max_keypoints"], nfeatures=p["nfeatures"], fast_threshold=p["fast_th"],
                   edge_threshold=p["edge_th"], nlevels=p["nlevels"], scale_factor=p["scale_factor"], score=p["score"], **kw)
    orb.set_pattern(c["pool"])
    return orb


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_equal_the_statement(hip, name):
    """stvo_orb_detect_levels and stvo_orb_detect_levels_dev, twice each on one detector (the scratch is reused)."""
    import torch
    c = CASES[name]
    p = c["prm"]
    B, rows, cols = c["images"].shape
    K = p["max_keypoints"]
    exp = wc.expected(c)
    orb = make_orb(hip, c)
    try:
        orb.set_descriptor(p["wta_k"], p["patch_size"])            # (after the pool: derived from it at patch size 31)
        assert np.array_equal(orb.pattern().reshape(512, 2)[:len(exp[0]["trace"]["points"])], exp[0]["trace"]["points"])
        for run in range(2):
            out = orb.detect(c["images"])
            for b in range(B):
                same(out[b], exp[b], (name, run, b))
                assert out[b]["n_total"] == exp[b]["n_total"], (name, run, b)
        dev = "cuda:0"
        img = torch.from_numpy(c["images"]).to(dev)
        kp = torch.zeros((B, K, 2), dtype=torch.float32, device=dev); resp = torch.zeros((B, K), dtype=torch.float32, device=dev)
        ang = torch.zeros((B, K), dtype=torch.float32, device=dev); desc = torch.zeros((B, K, 32), dtype=torch.uint8, device=dev)
        n = torch.zeros(B, dtype=torch.int32, device=dev); octv = torch.full((B, K), -1, dtype=torch.int32, device=dev)
        ntot = torch.zeros(B, dtype=torch.int32, device=dev)
        for run in range(2):
            orb.detect_dev(img.data_ptr(), kp.data_ptr(), resp.data_ptr(), ang.data_ptr(), desc.data_ptr(), n.data_ptr(), octv.data_ptr(), ntot.data_ptr())
            hip.synchronize()
            nn = n.cpu().numpy()
            for b in range(B):
                got = dict(kp=kp[b, :nn[b]].cpu().numpy(), response=resp[b, :nn[b]].cpu().numpy(), angle=ang[b, :nn[b]].cpu().numpy(),
                           desc=desc[b, :nn[b]].cpu().numpy(), octave=octv[b, :nn[b]].cpu().numpy())
                same(got, exp[b], (name, "dev", run, b))
                assert int(ntot[b]) == exp[b]["n_total"]
    finally:
        orb.close()


@pytest.mark.parametrize("name", wc.ENTRY_SUBSET)
def test_plain_entry_points(hip, name):
    """stvo_orb_detect and stvo_orb_detect_dev (no octave, no n_total), the setting given to the constructor."""
    import torch
    c = CASES[name]
    p = c["prm"]
    B, rows, cols = c["images"].shape
    K = p["max_keypoints"]
    exp = wc.expected(c)
    orb = make_orb(hip, c, wta_k=p["wta_k"], patch_size=p["patch_size"])     # (set_pattern after the setting: the pattern is derived again)
    try:
        kp = np.zeros((B, K, 2), np.float32); resp = np.zeros((B, K), np.float32); ang = np.zeros((B, K), np.float32)
        desc = np.zeros((B, K, 32), np.uint8); n = np.zeros(B, np.int32)
        hip._chk(hip.lib.stvo_orb_detect(orb.h, c["images"].reshape(-1), kp.reshape(-1), resp.reshape(-1), ang.reshape(-1), desc.reshape(-1), n))
        for b in range(B):
            same(dict(kp=kp[b, :n[b]], response=resp[b, :n[b]], angle=ang[b, :n[b]], desc=desc[b, :n[b]]), exp[b], (name, b), KEYS[:4])
        dev = "cuda:0"
        img = torch.from_numpy(c["images"]).to(dev)
        t = [torch.zeros(s, dtype=d, device=dev) for s, d in (((B, K, 2), torch.float32), ((B, K), torch.float32), ((B, K), torch.float32),
                                                              ((B, K, 32), torch.uint8), ((B,), torch.int32))]
        hip._chk(hip.lib.stvo_orb_detect_dev(orb.h, img.data_ptr(), *[x.data_ptr() for x in t]))
        hip.synchronize()
        nn = t[4].cpu().numpy()
        for b in range(B):
            got = dict(kp=t[0][b, :nn[b]].cpu().numpy(), response=t[1][b, :nn[b]].cpu().numpy(), angle=t[2][b, :nn[b]].cpu().numpy(),
                       desc=t[3][b, :nn[b]].cpu().numpy())
            same(got, exp[b], (name, "dev", b), KEYS[:4])
    finally:
        orb.close()


def test_default_setting_survives_a_round_trip(hip, oracle):
    """A detector set to (4, 21) and back to (2, 31) gives byte-identical output to one never set — the committed goldens, i.e. the
    parent's output — and get_pattern follows every setting."""
    from stvo_amd import capi
    g = np.load(os.path.join(ROOT, "tests", "golden", "orb_goldens.npz"))
    for c, (seed, cols, rows, nf, th) in enumerate(g["cases"]):
        img = g[f"img_{c}"]
        orb = capi.Orb(hip, 1, int(cols), int(rows), max_keypoints=4096, nfeatures=int(nf), fast_threshold=int(th))
        try:
            pool = orb.pattern().copy()
            assert np.array_equal(pool.reshape(512, 2), capi.orb_pattern(2, 31))
            first = orb.detect(img[None])[0]
            orb.set_descriptor(4, 21)
            assert np.array_equal(orb.pattern().reshape(512, 2), nw.effective_pattern(4, 21))
            other = orb.detect(img[None])[0]
            same(other, nw.detect_levels(img, int(nf), 1, 1.2, int(th), 19, pool, 4096, 4, 21), c)
            assert not np.array_equal(other["desc"], first["desc"]) and np.array_equal(other["kp"], first["kp"])
            orb.set_descriptor(3, 31)
            eff = nw.effective_pattern(3, 31, pool)
            got = orb.pattern().reshape(512, 2)
            assert np.array_equal(got[:384], eff) and not got[384:].any()
            orb.set_descriptor(2, 31)
            assert np.array_equal(orb.pattern(), pool)
            third = orb.detect(img[None])[0]
            same(third, first, c)
            for k in ("kp", "response", "angle", "desc"):
                assert np.array_equal(third[k], g[f"{k}_{c}"]), (c, k)
        finally:
            orb.close()


def test_refusals_leave_the_setting_in_force(hip):
    from stvo_amd import capi
    c = CASES["patch_P27_k4_e19"]
    exp = wc.expected(c)
    for edge in sorted({e for _, _, e, _ in wc.REFUSED}):
        orb = capi.Orb(hip, 1, 192, 144, edge_threshold=edge) if edge != 19 else make_orb(hip, c)
        try:
            if edge == 19:
                orb.set_descriptor(4, 27)
            before = orb.pattern().copy()
            for k, P, e, code in wc.REFUSED:
                if e != edge:
                    continue
                with pytest.raises(capi.StvoError, match=rf"\({code}\)"):
                    orb.set_descriptor(k, P)
                assert np.array_equal(orb.pattern(), before), (k, P)
            if edge == 19:
                # a pool a tuple of four cannot be drawn from is refused under WTA_K 4 and changes nothing
                three = np.zeros((512, 2), np.int8)
                three[1::3] = (2, 2)
                three[2::3] = (-5, 7)
                orb.set_descriptor(4, 31)
                kept = orb.pattern().copy()
                with pytest.raises(capi.StvoError, match=r"\(-1\)"):
                    orb.set_pattern(three)
                assert np.array_equal(orb.pattern(), kept)
                orb.set_descriptor(4, 27)
                same(orb.detect(c["images"])[0], exp[0], "after the refusals")
        finally:
            orb.close()
    with pytest.raises(capi.StvoError):
        capi.Orb(hip, 1, 192, 144, patch_size=28)
    with pytest.raises(capi.StvoError):
        capi.Orb(hip, 1, 192, 144, wta_k=5)


def wta_frames(pairs, pool, nfeatures, nlevels, wta_k, patch_size, th=20):
    frames = []
    z4 = np.zeros((0, 4), np.float32); zd = np.zeros((0, 32), np.uint8)
    for left, right in pairs:
        l = nw.detect_levels(left, nfeatures, nlevels, 1.2, th, 19, pool, 4096, wta_k, patch_size)
        r = nw.detect_levels(right, nfeatures, nlevels, 1.2, th, 19, pool, 4096, wta_k, patch_size)
        frames.append(dict(kp_l=l["kp"], oct_l=l["octave"], desc_l=l["desc"], kp_r=r["kp"], desc_r=r["desc"], kl_l=z4, oct_ll=np.zeros(0, np.int32),
                           ldesc_l=zd, kl_r=z4, ldesc_r=zd, ang_l=np.zeros(0, np.float32)))
    return frames


def test_handler_reads_the_descriptor_keys_from_the_config_file(tmp_path, oracle):
    """`orb_wta_k : 4` and `orb_patch_size : 27` in the file given with -c reach the handler's detector: images in, poses out, against the
    CPU chain fed with the statement's key-points, with the adaptive FAST threshold the previous frame left behind.  A setting the
    border rule refuses ends the program with the handler's error."""
    import test_gpu_handler as tgh
    cam = dict(synth.KITTI_CAM, width=640, height=240)
    pairs = synth.make_stereo_image_sequence(93, 3, cam)
    seq = str(tmp_path / "img.bin"); res_path = str(tmp_path / "res.bin")
    synth.write_image_sequence(seq, pairs, cam)
    cfg = tmp_path / "cfg.yaml"
    nfeat = 600
    cfg.write_text(f"orb_nfeatures : {nfeat}\norb_wta_k : 4   # was set to 2\norb_patch_size : 27\n")
    p = subprocess.run([APP, seq, res_path, "--preset", "kitti", "--no-lines", "-c", str(cfg)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr + p.stdout
    res = synth.read_results(res_path)
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=0)
    fast = dict(adaptive=True, th0=20, mn=7, mx=30, inc=5, feat=50, err=0.5)
    pool = oracle.orb_default_pattern()
    frames, th, ref = [], fast["th0"], []
    for k, pair in enumerate(pairs):
        frames += wta_frames([pair], pool, nfeat, 1, 4, 27, th)
        if k == 0:
            plain = oracle.orb_detect_levels(pair[0], nfeatures=nfeat, nlevels=1, fast_th=th, pattern=pool)
            assert np.array_equal(plain["kp"], frames[0]["kp_l"]) and not np.array_equal(plain["desc"], frames[0]["desc_l"])
        else:
            ref = pipeline_ref.run_sequence(oracle, frames, cam, mp, op, fast=fast)
            th = ref[-1]["fast"]
    tgh.compare(res, ref)
    assert sum(r["ints"][1] == 0 for r in res) >= 1
    cfg.write_text("orb_patch_size : 28\n")
    p = subprocess.run([APP, seq, res_path, "--preset", "kitti", "--no-lines", "-c", str(cfg)], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "stvo_orb_set_descriptor" in p.stderr + p.stdout


def test_image_pipeline_with_a_descriptor_setting(oracle):
    """ImagePipeline(orb_wta_k=3, orb_patch_size=21): images in, one step's poses out on the device against the CPU chain."""
    from stvo_amd import capi, images
    cam = dict(synth.KITTI_CAM, width=640, height=240)
    mp = match_params("kitti"); op = opt_params("kitti", has_lines=0)
    B, nfeat = 2, 600
    seqs = [synth.make_stereo_image_sequence(60 + b, 2, cam, shift_per_disp=0.3 - 0.05 * b) for b in range(B)]
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        with pytest.raises(capi.StvoError):
            images.ImagePipeline(ctx, B, cam, mp, op, orb_patch_size=28)       # the border rule at edge 19
    except BaseException:
        ctx.close()
        raise
    pipe = images.ImagePipeline(ctx, B, cam, mp, op, max_kp=2048, nfeatures=nfeat, orb_wta_k=3, orb_patch_size=21)
    try:
        assert np.array_equal(pipe.orb.pattern().reshape(512, 2)[:384], nw.effective_pattern(3, 21))
        refs = [pipeline_ref.run_sequence(oracle, wta_frames(seqs[b], None, nfeat, 1, 3, 21), cam, mp, op) for b in range(B)]
        for k in range(2):
            res, counts = pipe.push_images(np.stack([seqs[b][k][0] for b in range(B)]), np.stack([seqs[b][k][1] for b in range(B)]))
            if k == 0:
                continue
            for b in range(B):
                o, r = refs[b][0], res[b]
                assert counts[b, 0] == o["n_stereo_pt"] and r["n_matched_pt"] == o["n_matched_pt"], (b, counts[b], o["n_stereo_pt"])
                assert r["status"] == o["status"] and r["path"] == o["path"] and tuple(r["iters"]) == o["iters"]
                assert r["n_inliers_pt"] == o["n_inliers_pt"]
                T = r["T"].reshape(4, 4)
                assert np_model.rot_angle(T[:3, :3], o["T"][:3, :3]) < 1e-4 and np.linalg.norm(T[:3, 3] - o["T"][:3, 3]) < 1e-3
                assert np.allclose(T, o["T"], atol=1e-8)
    finally:
        pipe.close()
        ctx.close()


def test_randomised_parity_short_run():
    import fuzz_orb_wta
    assert fuzz_orb_wta.main(["--seconds", "60", "--cases", "40", "--seed", "11", "--max-size", "300"]) == 0
