"""Stereo rectification on the GPU (stvo_rectify_*): the remap kernel bit for bit against numpy (tests/np_rectify.py) for the
shipped calibrations, caller maps over every border, batches smaller than the rectifier; the copy when dist is false; and raw
distorted EuRoC-size pairs through images.ImagePipeline(rectify=...) and the app's --dataset-params, against the same images
rectified in numpy and fed to the existing paths."""
import os
import subprocess

import numpy as np
import pytest
import torch

import np_rectify as nr
from stvo_amd import capi, images, synth
from stvo_amd.ctypes_types import match_params, opt_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "tests", "golden", "dataset_params")
APP = os.path.join(ROOT, "stvo-pl_amd", "bin", "imagesStVO_synth")


def calib_of(name):
    return capi.read_dataset_params(os.path.join(PARAMS, name))


def kitti_distorted():
    c = calib_of("kitti00-02.yaml")
    c.d[:] = [-0.17, 0.021, 0.0004, -0.0003]
    return c


def odd_calib():
    c = capi.RectCalib()
    c.form, c.width, c.height, c.b = capi.RECT_FORM_KITTI, 37, 19, 0.1
    c.fx, c.fy, c.cx, c.cy = 30.0, 30.0, 18.2, 9.4
    c.d[:] = [-0.25, 0.05, 0.001, 0.0]
    return c


def make_images(seed, n, rows, cols):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k % 2 == 0:
            out.append(rng.integers(0, 256, (rows, cols), dtype=np.uint8))
        else:  # structured: ramps, a checkerboard and the extremes
            yy, xx = np.mgrid[0:rows, 0:cols]
            im = ((xx * 7 + yy * 3 + k) % 256).astype(np.uint8)
            im[(xx // 5 + yy // 5) % 2 == 0] = 255
            im[:, :2] = 0
            out.append(im)
    return np.stack(out)



def expect(imgs, m1, m2):
    return np.stack([nr.remap(im, m1, m2) for im in imgs])


@pytest.mark.parametrize("name,ns", [("euroc_params.yaml", (1, 3, 64)), ("perceptin_params.yaml", (1, 3)), ("kitti_distorted", (1, 3)),
                                     ("odd", (1, 3, 64)), ("odd", (64, 2))])  # (64, 2): fewer pairs than B after a full staging block
def test_remap_parity(hip, name, ns):
    c = kitti_distorted() if name == "kitti_distorted" else odd_calib() if name == "odd" else calib_of(name)
    cam, m1, m2 = capi.rectify_compute(c)
    assert cam["dist"] == 1
    rect = capi.Rectifier(hip, 64, calib=c)
    try:
        for n in ns:
            L = make_images(n, n, c.height, c.width)
            R = make_images(1000 + n, n, c.height, c.width)
            ol, orr = rect.rectify(L, R)
            assert np.array_equal(ol, expect(L, m1[0], m2[0])), (name, n)
            assert np.array_equal(orr, expect(R, m1[1], m2[1])), (name, n)
    finally:
        rect.close()


def test_remap_device_entry_point_subsets(hip):
    """stvo_rectify_images_dev on torch buffers: n < B pairs out of the middle of an ImagePipeline-shaped buffer (B left, B right)."""
    c = calib_of("euroc_params.yaml")
    _, m1, m2 = capi.rectify_compute(c)
    B, n, off = 8, 3, 2
    imgs = make_images(5, 2 * B, c.height, c.width)
    rect = capi.Rectifier(hip, B, calib=c)
    try:
        src = torch.from_numpy(imgs).cuda()
        dst = torch.zeros_like(src)
        torch.cuda.synchronize()
        px = c.height * c.width
        s, d = src.data_ptr(), dst.data_ptr()
        rect.rectify_dev(n, s + off * px, s + (B + off) * px, d + off * px, d + (B + off) * px)
        hip.synchronize()
        out = dst.cpu().numpy()
        assert np.array_equal(out[off:off + n], expect(imgs[off:off + n], m1[0], m2[0]))
        assert np.array_equal(out[B + off:B + off + n], expect(imgs[B + off:B + off + n], m1[1], m2[1]))
        untouched = np.ones(2 * B, bool)
        untouched[off:off + n] = untouched[B + off:B + off + n] = False
        assert not out[untouched].any()
        with pytest.raises(capi.StvoError):  # a destination over a source
            rect.rectify_dev(n, s, s + B * px, s + px, d)
        with pytest.raises(capi.StvoError):  # more pairs than the rectifier holds
            rect.rectify_dev(B + 1, s, s + B * px, d, d + B * px)
    finally:
        rect.close()


def test_identity_maps_return_the_image(hip):
    rows, cols = 61, 203
    yy, xx = np.mgrid[0:rows, 0:cols]
    m1 = np.stack([np.stack([xx, yy], -1)] * 2).astype(np.int16)
    m2 = np.zeros((2, rows, cols), np.uint16)
    rect = capi.Rectifier(hip, 4, maps=(m1, m2))
    try:
        L, R = make_images(3, 4, rows, cols), make_images(4, 4, rows, cols)
        ol, orr = rect.rectify(L, R)
        assert np.array_equal(ol, L) and np.array_equal(orr, R)
    finally:
        rect.close()


@pytest.mark.parametrize("rows,cols", [(19, 37), (480, 752), (64, 96)])
def test_random_caller_maps_every_border(hip, rows, cols):
    """Random source positions over [-2, cols + 1] x [-2, rows + 1] with every fraction: taps outside the source on all four sides,
    the last column and the last row."""
    rng = np.random.default_rng(rows * cols)
    u = rng.uniform(-2, cols + 1, (2, rows, cols))
    v = rng.uniform(-2, rows + 1, (2, rows, cols))
    iu, iv = np.floor(u * 32).astype(np.int64), np.floor(v * 32).astype(np.int64)
    m1 = np.stack([iu >> 5, iv >> 5], -1).astype(np.int16)
    m2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    m2.reshape(-1)[:1024] = np.arange(1024)  # every fraction at least once
    rect = capi.Rectifier(hip, 5, maps=(m1, m2))
    try:
        for n in (1, 5):
            L, R = make_images(7 + n, n, rows, cols), make_images(17 + n, n, rows, cols)
            ol, orr = rect.rectify(L, R)
            assert np.array_equal(ol, expect(L, m1[0], m2[0])) and np.array_equal(orr, expect(R, m1[1], m2[1]))
    finally:
        rect.close()


def test_dist_false_is_a_copy(hip):
    c = calib_of("kitti00-02.yaml")
    rect = capi.Rectifier(hip, 3, calib=c)
    try:
        assert rect.dist == 0
        L, R = make_images(1, 3, c.height, c.width), make_images(2, 3, c.height, c.width)
        ol, orr = rect.rectify(L, R)
        assert np.array_equal(ol, L) and np.array_equal(orr, R)
    finally:
        rect.close()


# ---- end to end: raw distorted images -> poses ----------------------------------------------------------------------------------

def distort_view(img, K, D, R, P, iters=20):
    """Render the raw (distorted, unrectified) view of a rectified image: each raw pixel is undistorted, rotated and projected with
    R / P into the rectified image, which is sampled bilinearly (0 outside)."""
    rows, cols = img.shape
    k = nr.dist12(D)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    x0, y0 = (xx - K[2]) / K[0], (yy - K[3]) / K[1]
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icd = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        x, y = (x0 - 2 * k[2] * x * y - k[3] * (r2 + 2 * x * x)) * icd, (y0 - k[2] * (r2 + 2 * y * y) - 2 * k[3] * x * y) * icd
    M = P[:, :3] @ R
    q = np.stack([x, y, np.ones_like(x)], -1) @ M.T
    u, v = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
    u0, v0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = u - u0, v - v0
    src = img.astype(np.float64)

    def at(a, b):
        ok = (a >= 0) & (a < cols) & (b >= 0) & (b < rows)
        return np.where(ok, src[np.clip(b, 0, rows - 1), np.clip(a, 0, cols - 1)], 0.0)

    out = (at(u0, v0) * (1 - fu) * (1 - fv) + at(u0 + 1, v0) * fu * (1 - fv) + at(u0, v0 + 1) * (1 - fu) * fv +
           at(u0 + 1, v0 + 1) * fu * fv)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def raw_sequences(c, cam, B, nf):
    rc = dict(cam["cam"], width=c.width, height=c.height)
    K1, K2 = [nr.f32(v) for v in c.Kl[:4]], [nr.f32(v) for v in c.Kr[:4]]
    seqs = []
    for b in range(B):
        pairs = synth.make_stereo_image_sequence(300 + b, nf, rc, shift_per_disp=0.3 - 0.05 * b)
        seqs.append([(distort_view(l, K1, c.Dl[:c.n_dist], cam["R1"], cam["P1"]), distort_view(r, K2, c.Dr[:c.n_dist], cam["R2"], cam["P2"]))
                     for l, r in pairs])
    return rc, seqs


def test_raw_images_to_poses_match_numpy_rectified():
    c = calib_of("euroc_params.yaml")
    cam, m1, m2 = capi.rectify_compute(c)
    B, nf = 2, 4
    rc, seqs = raw_sequences(c, cam, B, nf)
    mp, op = match_params("euroc"), opt_params("euroc", has_lines=0)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        rect = capi.Rectifier(ctx, B, calib=c)
        assert rect.camera == rc
        pipe_r = images.ImagePipeline(ctx, B, rc, mp, op, max_kp=2048, nlevels=4, rectify=rect)
        pipe_n = images.ImagePipeline(ctx, B, rc, mp, op, max_kp=2048, nlevels=4)
        n_ok = 0
        for k in range(nf):
            L = np.stack([seqs[b][k][0] for b in range(B)])
            R = np.stack([seqs[b][k][1] for b in range(B)])
            res_r, cnt_r = pipe_r.push_images(L, R)
            res_n, cnt_n = pipe_n.push_images(expect(L, m1[0], m2[0]), expect(R, m1[1], m2[1]))
            assert np.array_equal(cnt_r, cnt_n), k
            for f in res_r.dtype.names:
                assert np.array_equal(res_r[f], res_n[f]), (k, f)
            if k:
                n_ok += int((res_r["status"] == 0).sum())
                assert cnt_r[:, 0].min() > 20, cnt_r  # stereo association works on the rectified images
        assert n_ok >= 1
        pipe_r.close()
        pipe_n.close()
        rect.close()
    finally:
        ctx.close()


def test_app_dataset_params_on_raw_images(tmp_path):
    c = calib_of("euroc_params.yaml")
    cam, m1, m2 = capi.rectify_compute(c)
    rc, seqs = raw_sequences(c, cam, 1, 4)
    raw, rectified = str(tmp_path / "raw.bin"), str(tmp_path / "rect.bin")
    synth.write_image_sequence(raw, seqs[0], dict(rc, fx=1.0, fy=1.0, cx=0.0, cy=0.0, b=1.0))  # a header camera the flag must not use
    synth.write_image_sequence(rectified, [(nr.remap(l, m1[0], m2[0]), nr.remap(r, m1[1], m2[1])) for l, r in seqs[0]], rc)
    outs = []
    for seq, extra in ((raw, ["--dataset-params", os.path.join(PARAMS, "euroc_params.yaml")]), (rectified, [])):
        res = str(tmp_path / (os.path.basename(seq) + ".res"))
        p = subprocess.run([APP, seq, res, "--preset", "euroc", "--no-lines", *extra], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr + p.stdout
        outs.append(open(res, "rb").read())
    assert len(outs[0]) == 3 * synth.RESULT_DTYPE.itemsize
    assert outs[0] == outs[1]
