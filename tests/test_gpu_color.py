"""Colour frames in (stvo_color_to_gray*, stvo_rectify_color_*, ImagePipeline(channels=...), the handler mirror's Image overloads
and the app's STVOIMG2 files) against the statement tests/np_color.py, bit for bit: the grey conversion on every (B, G, R) triple
in both weight sets and both channel orders, the shapes and alignments where the indexing of the stream kernel can go wrong, the
colour remap over every border, the fused remap -> grey against remap-then-grey (and told apart from grey-then-remap), and colour
frames to poses against the same pipeline fed the grey planes the statement gives."""
import os
import subprocess

import numpy as np
import pytest
import torch

import np_color as nc
import np_rectify as nr
from stvo_amd import capi, images, synth
from stvo_amd.ctypes_types import match_params, opt_params
from test_gpu_rectify import APP, PARAMS, calib_of, distort_view

pytestmark = pytest.mark.gpu

OTHER = {"bgr": "rgb", "rgb": "bgr"}


# ---- the conversion --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def all_triples():
    """4096 x 4096 x 3: every (B, G, R) value once."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.parametrize("weights", ["q14", "q15"])
@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_every_triple(hip, all_triples, order, weights):
    a, b = capi.color_to_gray(hip, all_triples, order, weights, swapped=True)
    assert np.array_equal(a, nc.gray(all_triples, order, weights))
    assert np.array_equal(b, nc.gray(all_triples, OTHER[order], weights))
    rng = np.random.default_rng(11)
    bgra = np.concatenate([all_triples[:, 1024:1280], rng.integers(0, 256, (4096, 256, 1), dtype=np.uint8)], -1)
    a4, b4 = capi.color_to_gray(hip, bgra, order, weights, swapped=True)
    assert np.array_equal(a4, nc.gray(bgra, order, weights)) and np.array_equal(a4, a[:, 1024:1280])
    assert np.array_equal(b4, nc.gray(bgra, OTHER[order], weights))


GUARD = 0xA5


def convert_dev(ctx, img, src_off, dst_off, two, order="bgr", weights="q14"):
    """stvo_color_to_gray_dev on slices of larger device tensors that start src_off / dst_off bytes past a 256-byte boundary; returns
    the plane(s) and checks that the bytes around each destination kept their guard value."""
    n, rows, cols, ch = img.shape
    npix = n * rows * cols
    src = torch.full((npix * ch + 512,), GUARD, dtype=torch.uint8, device="cuda")
    src[256 + src_off:256 + src_off + npix * ch] = torch.from_numpy(img.reshape(-1)).cuda()
    dst = [torch.full((npix + 512,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(2 if two else 1)]
    torch.cuda.synchronize()
    ptrs = [d.data_ptr() + 256 + dst_off for d in dst]
    assert src.data_ptr() % 256 == 0 and all(d.data_ptr() % 256 == 0 for d in dst)
    capi.color_to_gray_dev(ctx, n, rows, cols, ch, src.data_ptr() + 256 + src_off, ptrs[0], ptrs[1] if two else None, order, weights)
    ctx.synchronize()
    out = []
    for d in dst:
        h = d.cpu().numpy()
        assert (h[:256 + dst_off] == GUARD).all() and (h[256 + dst_off + npix:] == GUARD).all()
        out.append(h[256 + dst_off:256 + dst_off + npix].reshape(n, rows, cols))
    return out


@pytest.mark.parametrize("rows,cols", [(19, 37), (61, 203), (64, 96)])
def test_shapes_alignments_and_guards(hip, rows, cols):
    """(19, 37) and (61, 203): pixel counts that are no multiple of the 16 pixels of a thread (a tail); n = 5 of (61, 203): more than
    one block; offsets 0: the 16-byte path, 1 and 3: the byte path."""
    rng = np.random.default_rng(rows * cols)
    for n in (1, 5):
        for ch in (3, 4):
            img = rng.integers(0, 256, (n, rows, cols, ch), dtype=np.uint8)
            want_a, want_b = nc.gray(img, "bgr"), nc.gray(img, "rgb")
            for src_off, dst_off in ((0, 0), (1, 1), (3, 3), (1, 0), (0, 3), (16, 32)):
                for two in (False, True):
                    got = convert_dev(hip, img, src_off, dst_off, two)
                    assert np.array_equal(got[0], want_a), (n, ch, src_off, dst_off, two)
                    if two:
                        assert np.array_equal(got[1], want_b), (n, ch, src_off, dst_off)
    assert (1 * 19 * 37) % 16 and (5 * 61 * 203) % 16  # the tails these shapes are here for


def test_conversion_refusals(hip):
    img = torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 2, 8, 8), dtype=torch.uint8, device="cuda")
    s, a, b = img.data_ptr(), out[0].data_ptr(), out[1].data_ptr()
    capi.color_to_gray_dev(hip, 2, 8, 8, 4, s, a, b)
    for ch in (2, 5, 1, 0):
        with pytest.raises(capi.StvoError):
            capi.color_to_gray_dev(hip, 2, 8, 8, ch, s, a, b)
    with pytest.raises(capi.StvoError):  # a plane inside the source
        capi.color_to_gray_dev(hip, 2, 8, 8, 4, s, s + 64, None)
    with pytest.raises(capi.StvoError):  # the planes overlap each other
        capi.color_to_gray_dev(hip, 2, 8, 8, 4, s, a, a + 64)
    with pytest.raises(capi.StvoError):  # NULL source / plane
        capi.color_to_gray_dev(hip, 2, 8, 8, 4, None, a, b)
    with pytest.raises(capi.StvoError):
        capi.color_to_gray_dev(hip, 2, 8, 8, 4, s, None, b)
    with pytest.raises(capi.StvoError):  # an unknown weight set
        hip._chk(hip.lib.stvo_color_to_gray_dev(hip.h, 2, 8, 8, 4, 0, 2, s, a, b))
    hip.synchronize()


# ---- colour rectification ----------------------------------------------------------------------------------------------------------

def random_maps(rows, cols):
    """The maps of test_gpu_rectify.test_random_caller_maps_every_border."""
    rng = np.random.default_rng(rows * cols)
    u = rng.uniform(-2, cols + 1, (2, rows, cols))
    v = rng.uniform(-2, rows + 1, (2, rows, cols))
    iu, iv = np.floor(u * 32).astype(np.int64), np.floor(v * 32).astype(np.int64)
    m1 = np.stack([iu >> 5, iv >> 5], -1).astype(np.int16)
    m2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    m2.reshape(-1)[:1024] = np.arange(1024)
    return m1, m2


def fused_dev(ctx, rect, L, R, two, order="bgr", weights="q14"):
    """stvo_rectify_color_to_gray_dev: (plane A left, right[, plane B left, right])."""
    n, rows, cols, ch = L.shape
    src = torch.from_numpy(np.stack([L, R])).cuda()
    out = torch.full((4, n, rows, cols), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = [out[k].data_ptr() for k in range(4)]
    rect.rectify_color_to_gray_dev(n, ch, src[0].data_ptr(), src[1].data_ptr(), p[0], p[1], p[2] if two else None, p[3] if two else None,
                                   order, weights)
    ctx.synchronize()
    h = out.cpu().numpy()
    if not two:
        assert (h[2:] == GUARD).all()
    return h


@pytest.mark.parametrize("rows,cols", [(19, 37), (64, 96), (480, 752)])
def test_color_remap_every_border(hip, rows, cols):
    m1, m2 = random_maps(rows, cols)
    rect = capi.Rectifier(hip, 5, maps=(m1, m2))
    rng = np.random.default_rng(rows + cols)
    try:
        for ch, n in ((3, 1), (4, 5), (3, 5), (4, 1)) if rows < 480 else ((3, 1), (4, 5)):
            L, R = (rng.integers(0, 256, (n, rows, cols, ch), dtype=np.uint8) for _ in range(2))
            want_l, want_r = nc.remap_color(L, m1[0], m2[0]), nc.remap_color(R, m1[1], m2[1])
            ol, orr = rect.rectify_color(L, R)
            assert np.array_equal(ol, want_l) and np.array_equal(orr, want_r), (ch, n)
            for two in (False, True):
                order, weights = ("bgr", "q14") if two else ("rgb", "q15")
                h = fused_dev(hip, rect, L, R, two, order, weights)
                assert np.array_equal(h[0], nc.gray(want_l, order, weights)) and np.array_equal(h[1], nc.gray(want_r, order, weights)), (ch, n)
                if two:
                    assert np.array_equal(h[2], nc.gray(want_l, "rgb")) and np.array_equal(h[3], nc.gray(want_r, "rgb")), (ch, n)
            # the test can tell the reference's order (remap, then grey) from the other one
            other = nr.remap(nc.gray(L, "bgr"), m1[0], m2[0])
            assert (other != nc.gray(want_l, "bgr")).mean() >= 0.05
    finally:
        rect.close()


def test_identity_maps_and_dist_false_are_the_plain_conversion(hip):
    rows, cols = 61, 203
    yy, xx = np.mgrid[0:rows, 0:cols]
    m1 = np.stack([np.stack([xx, yy], -1)] * 2).astype(np.int16)
    m2 = np.zeros((2, rows, cols), np.uint16)
    rng = np.random.default_rng(4)
    rect = capi.Rectifier(hip, 4, maps=(m1, m2))
    try:
        for ch in (3, 4):
            L, R = (rng.integers(0, 256, (4, rows, cols, ch), dtype=np.uint8) for _ in range(2))
            ol, orr = rect.rectify_color(L, R)
            assert np.array_equal(ol, L) and np.array_equal(orr, R)
            h = fused_dev(hip, rect, L, R, True)
            assert np.array_equal(h[0], nc.gray(L)) and np.array_equal(h[1], nc.gray(R))
            assert np.array_equal(h[2], nc.gray(L, "rgb")) and np.array_equal(h[3], nc.gray(R, "rgb"))
    finally:
        rect.close()
    c = calib_of("kitti00-02.yaml")
    rect = capi.Rectifier(hip, 3, calib=c)
    try:
        assert rect.dist == 0
        for ch, n in ((3, 3), (4, 2)):
            L, R = (rng.integers(0, 256, (n, c.height, c.width, ch), dtype=np.uint8) for _ in range(2))
            ol, orr = rect.rectify_color(L, R)
            assert np.array_equal(ol, L) and np.array_equal(orr, R)  # the reference's copy
            for two in (False, True):
                h = fused_dev(hip, rect, L, R, two, "bgr", "q15")
                assert np.array_equal(h[0], nc.gray(L, "bgr", "q15")) and np.array_equal(h[1], nc.gray(R, "bgr", "q15"))
                if two:
                    assert np.array_equal(h[2], nc.gray(L, "rgb", "q15")) and np.array_equal(h[3], nc.gray(R, "rgb", "q15"))
    finally:
        rect.close()


def test_color_rectify_refusals(hip):
    m1, m2 = random_maps(19, 37)
    B, px = 3, 19 * 37
    rect = capi.Rectifier(hip, B, maps=(m1, m2))
    try:
        src = torch.zeros((2, B + 1, 19, 37, 4), dtype=torch.uint8, device="cuda")
        dst = torch.zeros((2, B + 1, 19, 37, 4), dtype=torch.uint8, device="cuda")
        sl, sr, dl, dr = src[0].data_ptr(), src[1].data_ptr(), dst[0].data_ptr(), dst[1].data_ptr()
        rect.rectify_color_dev(B, 4, sl, sr, dl, dr)
        rect.rectify_color_to_gray_dev(B, 4, sl, sr, dl, dr)
        for ch in (2, 5, 1):
            with pytest.raises(capi.StvoError):
                rect.rectify_color_dev(B, ch, sl, sr, dl, dr)
            with pytest.raises(capi.StvoError):
                rect.rectify_color_to_gray_dev(B, ch, sl, sr, dl, dr)
        with pytest.raises(capi.StvoError):  # more pairs than the rectifier holds
            rect.rectify_color_dev(B + 1, 4, sl, sr, dl, dr)
        with pytest.raises(capi.StvoError):
            rect.rectify_color_to_gray_dev(B + 1, 4, sl, sr, dl, dr)
        with pytest.raises(capi.StvoError):  # a destination over a source
            rect.rectify_color_dev(B, 4, sl, sr, sl + 4 * px, dr)
        with pytest.raises(capi.StvoError):  # overlapping destinations
            rect.rectify_color_dev(B, 4, sl, sr, dl, dl + 4 * px)
        with pytest.raises(capi.StvoError):  # a plane over a source; planes over each other; one swapped plane without the other
            rect.rectify_color_to_gray_dev(B, 4, sl, sr, sr + px, dr)
        with pytest.raises(capi.StvoError):
            rect.rectify_color_to_gray_dev(B, 4, sl, sr, dl, dl + px)
        with pytest.raises(capi.StvoError):
            rect.rectify_color_to_gray_dev(B, 4, sl, sr, dl, dr, dl + 8 * B * px, None)
        with pytest.raises(capi.StvoError):  # NULL
            rect.rectify_color_dev(B, 4, sl, None, dl, dr)
        hip.synchronize()
    finally:
        rect.close()


# ---- colour frames to poses --------------------------------------------------------------------------------------------------------

def colorize(img, same_red_blue=False):
    """A grey scene -> B, G, R with three different tone curves (the same edges in every channel, so the grey images track like the
    scene does, but the BGR-weighted and the RGB-weighted grey differ by up to ~10 levels); same_red_blue: R = B, both greys equal."""
    x = img.astype(np.float64) / 255.0
    g = np.rint(255.0 * x ** 0.7).astype(np.uint8)
    r = img if same_red_blue else np.rint(255.0 * x ** 1.6).astype(np.uint8)
    return np.stack([img, g, r], -1)


class Scenes:
    pass


@pytest.fixture(scope="module")
def euroc():
    """B = 2 streams, 4 frames at EuRoC size: rectified colour pairs, the raw colour pairs the calibration distorts them into
    (distort_view per channel), and the grey planes the statement gives for both."""
    s = Scenes()
    s.c = calib_of("euroc_params.yaml")
    cam, m1, m2 = capi.rectify_compute(s.c)
    s.m1, s.m2 = m1, m2
    s.rc = dict(cam["cam"], width=s.c.width, height=s.c.height)
    s.B, s.nf = 2, 4
    K = [[nr.f32(v) for v in s.c.Kl[:4]], [nr.f32(v) for v in s.c.Kr[:4]]]
    D = [s.c.Dl[:s.c.n_dist], s.c.Dr[:s.c.n_dist]]
    RP = [(cam["R1"], cam["P1"]), (cam["R2"], cam["P2"])]
    s.color, s.raw = [], []  # [frame][side] -> uint8 [B, rows, cols, 3]
    seqs = [synth.make_stereo_image_sequence(300 + b, s.nf, s.rc, shift_per_disp=0.3 - 0.05 * b) for b in range(s.B)]
    for k in range(s.nf):
        col = [np.stack([colorize(seqs[b][k][side]) for b in range(s.B)]) for side in range(2)]
        raw = [np.stack([np.stack([distort_view(np.ascontiguousarray(col[side][b][..., ch]), K[side], D[side], *RP[side], iters=6)
                                   for ch in range(3)], -1) for b in range(s.B)]) for side in range(2)]
        s.color.append(col)
        s.raw.append(raw)
    return s


def same_results(a, b, k):
    (res_a, cnt_a), (res_b, cnt_b) = a, b
    assert np.array_equal(cnt_a, cnt_b), k
    for f in res_a.dtype.names:
        assert res_a[f].tobytes() == res_b[f].tobytes(), (k, f)


def lsd_for(rc):
    return capi.lsd_params(min_length=0.025 * min(rc["width"], rc["height"]), nfeatures=100)


def test_color_frames_to_poses_lsd(euroc):
    s = euroc
    mp, op = match_params("euroc"), opt_params("euroc", has_lines=1)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=s.B)
    try:
        pipe_c = images.ImagePipeline(ctx, s.B, s.rc, mp, op, max_kp=2048, nlevels=4, lsd=lsd_for(s.rc), max_kl=128, channels=3)
        pipe_g = images.ImagePipeline(ctx, s.B, s.rc, mp, op, max_kp=2048, nlevels=4, lsd=lsd_for(s.rc), max_kl=128)
        assert pipe_c.gray_b is None and pipe_c.color is not None
        n_ok = n_lines = 0
        for k in range(s.nf):
            L, R = s.color[k]
            assert (nc.gray(L, "bgr") != nc.gray(L, "rgb")).mean() > 0.2
            got = pipe_c.push_images(L, R)
            same_results(got, pipe_g.push_images(nc.gray(L, "bgr"), nc.gray(R, "bgr")), k)
            if k:
                n_ok += int((got[0]["status"] == 0).sum())
                n_lines += int(got[0]["n_matched_ls"].sum())
        assert n_ok >= 1 and n_lines > 0
        pipe_c.close()
        pipe_g.close()
    finally:
        ctx.close()


def test_raw_color_frames_to_poses_lsd(euroc):
    s = euroc
    mp, op = match_params("euroc"), opt_params("euroc", has_lines=1)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=s.B)
    try:
        rect = capi.Rectifier(ctx, s.B, calib=s.c)
        pipe_c = images.ImagePipeline(ctx, s.B, s.rc, mp, op, max_kp=2048, nlevels=4, lsd=lsd_for(s.rc), max_kl=128, channels=3, rectify=rect)
        pipe_g = images.ImagePipeline(ctx, s.B, s.rc, mp, op, max_kp=2048, nlevels=4, lsd=lsd_for(s.rc), max_kl=128)
        assert pipe_c.rect_img is None  # the rectified colour image is never written
        n_ok = 0
        for k in range(s.nf):
            L, R = s.raw[k]
            gl, gr = nc.gray(nc.remap_color(L, s.m1[0], s.m2[0])), nc.gray(nc.remap_color(R, s.m1[1], s.m2[1]))
            got = pipe_c.push_images(L, R)
            same_results(got, pipe_g.push_images(gl, gr), k)
            if k:
                n_ok += int((got[0]["status"] == 0).sum())
                assert got[1][:, 0].min() > 20, got[1]
        assert n_ok >= 1
        pipe_c.close()
        pipe_g.close()
        rect.close()
    finally:
        ctx.close()


def test_one_channel_is_untouched(euroc):
    s = euroc
    mp, op = match_params("euroc"), opt_params("euroc", has_lines=1)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=s.B)
    try:
        pipe_1 = images.ImagePipeline(ctx, s.B, s.rc, mp, op, max_kp=2048, nlevels=4, lsd=lsd_for(s.rc), max_kl=128, channels=1)
        pipe_0 = images.ImagePipeline(ctx, s.B, s.rc, mp, op, max_kp=2048, nlevels=4, lsd=lsd_for(s.rc), max_kl=128)
        assert pipe_1.color is None and pipe_1.gray_b is None and pipe_1.rect_img is None
        for k in range(2):
            gl, gr = nc.gray(s.color[k][0]), nc.gray(s.color[k][1])
            same_results(pipe_1.push_images(gl, gr), pipe_0.push_images(gl, gr), k)
        pipe_1.close()
        pipe_0.close()
        for bad in (0, 2, 5):
            with pytest.raises(ValueError):
                images.ImagePipeline(ctx, s.B, s.rc, mp, op, channels=bad)
        with pytest.raises(ValueError):
            images.ImagePipeline(ctx, s.B, s.rc, mp, op, channels=3, gray_weights="q16")
    finally:
        ctx.close()


def test_pipeline_fld_reads_the_swapped_plane():
    """use_fld_lines on colour frames: ORB on the BGR-weighted grey, FLD and LBD on the RGB-weighted one (src/stereoFrame.cpp:249-258,303)."""
    cam = dict(synth.KITTI_CAM, width=640, height=240)
    B, K, M = 2, 2048, 128
    Lth = int(0.025 * 240)
    pair = [synth.make_stereo_image_sequence(60 + b, 1, cam)[0] for b in range(B)]
    L, R = np.stack([colorize(pair[b][0]) for b in range(B)]), np.stack([colorize(pair[b][1]) for b in range(B)])
    both = np.concatenate([L, R])
    bgr, rgb = nc.gray(both, "bgr"), nc.gray(both, "rgb")
    mp, op = match_params("kitti"), opt_params("kitti", has_lines=1)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    try:
        pipe = images.ImagePipeline(ctx, B, cam, mp, op, max_kp=K, fld=capi.fld_params(Lth, nfeatures=100), max_kl=M, channels=3)
        assert pipe.gray_b is not None
        pipe.set_images(L, R)
        torch.cuda.current_stream().synchronize()
        pipe.enqueue()
        ctx.synchronize()
        assert np.array_equal(pipe.img.cpu().numpy(), bgr) and np.array_equal(pipe.gray_b.cpu().numpy(), rgb)
        n, nl = pipe.n.cpu().numpy(), pipe.nl.cpu().numpy()
        kp, desc = pipe.kp.cpu().numpy(), pipe.desc.cpu().numpy()
        kl = pipe.kl.cpu().numpy().view(capi.KEYLINE_DTYPE).reshape(2 * B, M)
        ldesc = pipe.ldesc.cpu().numpy()
        orb = capi.Orb(ctx, 2 * B, 640, 240, K, 2000, 20, 19, 1, 1.2)
        fld = capi.Fld(ctx, 2 * B, 640, 240, capi.fld_params(Lth, nfeatures=100), max_keylines=M)
        lbd = capi.Lbd(ctx, 2 * B, 640, 240, max_keylines=M)

        def points_equal(plane):
            return all(len(d["kp"]) == n[i] and np.array_equal(d["kp"], kp[i, :n[i]]) and np.array_equal(d["desc"], desc[i, :n[i]])
                       for i, d in enumerate(orb.detect(plane)))

        def lines_equal(plane):
            recs = [r for r, _ in fld.detect(plane)]
            ld = lbd.compute(plane, [np.stack([r["sx"], r["sy"], r["ex"], r["ey"], r["angle"]], 1) for r in recs], [r["num_pixels"] for r in recs])
            return all(len(r) == nl[i] and r.tobytes() == kl[i, :nl[i]].tobytes() and np.array_equal(ld[i], ldesc[i, :nl[i]])
                       for i, r in enumerate(recs))

        assert n.min() > 100 and nl.min() > 20
        assert points_equal(bgr) and lines_equal(rgb)
        assert not points_equal(rgb) and not lines_equal(bgr)
        orb.close(); fld.close(); lbd.close()
        pipe.close()
    finally:
        ctx.close()


# ---- the handler mirror and the app ------------------------------------------------------------------------------------------------

def run_app(tmp_path, name, pairs, cam, *args):
    seq, res = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".res"))
    if isinstance(pairs, list) and isinstance(pairs[0], dict):
        synth.write_sequence(seq, pairs, cam)
    else:
        synth.write_image_sequence(seq, pairs, cam)
    p = subprocess.run([APP, seq, res, *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr + p.stdout
    return open(res, "rb").read()


def test_app_color_file_against_gray_file(tmp_path):
    cam = dict(synth.EUROC_CAM, width=640, height=240)
    pairs = synth.make_stereo_image_sequence(91, 4, cam)
    color = [(colorize(l), colorize(r)) for l, r in pairs]
    bgra = [(np.concatenate([l, l[..., :1] ^ 0x5A], -1), np.concatenate([r, r[..., 1:2]], -1)) for l, r in color]
    gray = [(nc.gray(l), nc.gray(r)) for l, r in color]
    want = run_app(tmp_path, "gray", gray, cam, "--preset", "euroc")  # points and LSD key-lines
    assert len(want) == 3 * synth.RESULT_DTYPE.itemsize
    assert run_app(tmp_path, "color", color, cam, "--preset", "euroc") == want
    assert run_app(tmp_path, "bgra", bgra, cam, "--preset", "euroc") == want
    res = synth.read_results(str(tmp_path / "color.res"))
    assert any(r["ints"][1] == 0 for r in res) and any(r["ints"][7] > 0 for r in res)
    gray15 = [(nc.gray(l, "bgr", "q15"), nc.gray(r, "bgr", "q15")) for l, r in color]
    assert run_app(tmp_path, "color15", color, cam, "--preset", "euroc", "--gray-weights", "q15") == \
        run_app(tmp_path, "gray15", gray15, cam, "--preset", "euroc")


def test_app_raw_color_with_dataset_params(tmp_path, euroc):
    s = euroc
    raw = [(s.raw[k][0][0], s.raw[k][1][0]) for k in range(s.nf)]
    rect = [(nc.gray(nc.remap_color(l, s.m1[0], s.m2[0])), nc.gray(nc.remap_color(r, s.m1[1], s.m2[1]))) for l, r in raw]
    hdr = dict(s.rc, fx=1.0, fy=1.0, cx=0.0, cy=0.0, b=1.0)  # a header camera the flag must not use
    got = run_app(tmp_path, "raw", raw, hdr, "--preset", "euroc", "--dataset-params", os.path.join(PARAMS, "euroc_params.yaml"))
    assert len(got) == 3 * synth.RESULT_DTYPE.itemsize
    assert got == run_app(tmp_path, "rect", rect, s.rc, "--preset", "euroc")


def test_app_fld_reads_the_swapped_plane(tmp_path, hip):
    """use_fld_lines : true through the handler mirror: with R = B both greys are equal and the colour file gives what the grey file
    gives; with R != B it gives what a feature file gives that holds ORB key-points of the BGR-weighted grey and FLD key-lines + LBD
    descriptors of the RGB-weighted grey, detected with the handler's parameters (kitti preset, fixed FAST threshold)."""
    cam = dict(synth.KITTI_CAM, width=640, height=240)
    pairs = synth.make_stereo_image_sequence(91, 4, cam)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("use_fld_lines : true\nadaptative_fast : false\n")
    args = ("--preset", "kitti", "-c", str(cfg))
    same = [(colorize(l, True), colorize(r, True)) for l, r in pairs]
    assert all(np.array_equal(nc.gray(l, "bgr"), nc.gray(l, "rgb")) for l, _ in same)
    got = run_app(tmp_path, "same", same, cam, *args)
    assert got == run_app(tmp_path, "same_gray", [(nc.gray(l), nc.gray(r)) for l, r in same], cam, *args)
    assert any(r["ints"][7] > 0 for r in synth.read_results(str(tmp_path / "same.res")))

    color = [(colorize(l), colorize(r)) for l, r in pairs]
    K, M, Lth = 4096, 512, int(0.025 * 240)
    orb = capi.Orb(hip, 2, 640, 240, K, 2000, 20, 19, 1, 1.2)
    fld = capi.Fld(hip, 2, 640, 240, capi.fld_params(Lth, nfeatures=100), max_keylines=M)
    lbd = capi.Lbd(hip, 2, 640, 240, max_keylines=M)

    def features(color_pairs, order_lines):
        frames = []
        for l, r in color_pairs:
            pts = orb.detect(np.stack([nc.gray(l, "bgr"), nc.gray(r, "bgr")]))
            plane = np.stack([nc.gray(l, order_lines), nc.gray(r, order_lines)])
            recs = [q for q, _ in fld.detect(plane)]
            xy = [np.stack([q["sx"], q["sy"], q["ex"], q["ey"], q["angle"]], 1) for q in recs]
            ld = lbd.compute(plane, xy, [q["num_pixels"] for q in recs])
            frames.append(dict(kp_l=pts[0]["kp"], oct_l=pts[0]["octave"], desc_l=pts[0]["desc"], kp_r=pts[1]["kp"], desc_r=pts[1]["desc"],
                               kl_l=xy[0][:, :4], ang_l=xy[0][:, 4], oct_ll=np.zeros(len(xy[0]), np.int32), ldesc_l=ld[0],
                               kl_r=xy[1][:, :4], ldesc_r=ld[1]))
        return frames

    try:
        got = run_app(tmp_path, "color", color, cam, *args)
        assert got == run_app(tmp_path, "feat_rgb", features(color, "rgb"), cam, *args)
        assert got != run_app(tmp_path, "feat_bgr", features(color, "bgr"), cam, *args)  # the planes do differ in what they give
        assert any(r["ints"][7] > 0 for r in synth.read_results(str(tmp_path / "color.res")))
    finally:
        orb.close(); fld.close(); lbd.close()
