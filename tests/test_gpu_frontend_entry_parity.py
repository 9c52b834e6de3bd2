"""The two entry points of every front-end object on one detector: the host-buffer call (staged through the object's own device block,
csrc/frontend_layout.h) and the `_dev` call on torch buffers must give the same bits — on the first images, on a second set through the
same object (the staging is reused and holds the first call's bytes), and for ORB and LBD on a larger object created after a smaller
one.  Every case must find something, so that equal outputs are not two empty ones.  (The rectifier and the colour entry points have
this in test_gpu_rectify.py and test_gpu_color.py.)"""
import numpy as np
import pytest

from stvo_amd import capi, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def scenes(seed, B, cols, rows):
    """B different images; a few rectangles and discs each, so that small images still hold corners and edges"""
    return np.stack([synth.make_image(seed + 17 * b, cols, rows, n_rects=12, n_discs=3) for b in range(B)])


def to_dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    torch.cuda.synchronize()
    return t


def zeros_dev(shape, dtype):
    import torch
    t = torch.zeros(shape, dtype=dtype, device=DEV)
    torch.cuda.synchronize()
    return t


# ---- ORB ---------------------------------------------------------------------------------------------------------------------------
ORB_KEYS = ("kp", "response", "angle", "desc", "octave")


def orb_both(hip, orb, imgs):
    """(host-buffer results, `_dev` results) of one detector, as lists of per-image dicts"""
    import torch
    B, K = orb.B, orb.K
    host = orb.detect(imgs)
    img = to_dev(imgs)
    kp, resp, ang = zeros_dev((B, K, 2), torch.float32), zeros_dev((B, K), torch.float32), zeros_dev((B, K), torch.float32)
    desc, n = zeros_dev((B, K, 32), torch.uint8), zeros_dev((B,), torch.int32)
    octv, ntot = zeros_dev((B, K), torch.int32), zeros_dev((B,), torch.int32)
    orb.detect_dev(img.data_ptr(), kp.data_ptr(), resp.data_ptr(), ang.data_ptr(), desc.data_ptr(), n.data_ptr(), octv.data_ptr(), ntot.data_ptr())
    hip.synchronize()
    nn = n.cpu().numpy()
    dev = [dict(kp=kp[b, :nn[b]].cpu().numpy(), response=resp[b, :nn[b]].cpu().numpy(), angle=ang[b, :nn[b]].cpu().numpy(),
                desc=desc[b, :nn[b]].cpu().numpy(), octave=octv[b, :nn[b]].cpu().numpy(), n_total=int(ntot[b])) for b in range(B)]
    return host, dev


def orb_same(host, dev, what):
    found = 0
    for b, (h, d) in enumerate(zip(host, dev)):
        assert h["n_total"] == d["n_total"], (what, b)
        for k in ORB_KEYS:
            assert h[k].shape == d[k].shape and h[k].tobytes() == d[k].tobytes(), (what, b, k)
        found += len(h["kp"])
    print(what, "key-points:", [len(h["kp"]) for h in host])
    assert found >= 1, what
    return found


@pytest.mark.parametrize("score", [1, 0], ids=["fast", "harris"])
@pytest.mark.parametrize("nlevels", [1, 3])
def test_orb_entry_points_agree(hip, nlevels, score):
    kw = dict(max_keypoints=64, nfeatures=60, fast_threshold=20, edge_threshold=19, nlevels=nlevels, scale_factor=1.2, score=score)
    small = capi.Orb(hip, 1, 64, 64, **kw)  # the smaller object first: the larger one below cuts larger blocks in the same process
    try:
        orb_same(*orb_both(hip, small, scenes(3, 1, 64, 64)), ("small", nlevels, score))
        orb = capi.Orb(hip, 2, 96, 80, **kw)
        try:
            first = orb_both(hip, orb, scenes(11, 2, 96, 80))
            orb_same(*first, ("first", nlevels, score))
            second = orb_both(hip, orb, scenes(29, 2, 96, 80))
            orb_same(*second, ("second", nlevels, score))
            assert any(a["kp"].tobytes() != b["kp"].tobytes() for a, b in zip(first[0], second[0]))  # (other images, other results)
            if nlevels > 1:
                assert max(int(h["octave"].max(initial=0)) for h in first[0] + second[0]) >= 1         # a higher level took part
        finally:
            orb.close()
        orb_same(*orb_both(hip, small, scenes(5, 1, 64, 64)), ("small again", nlevels, score))
    finally:
        small.close()


# ---- the key-line detectors ------------------------------------------------------------------------------------------------------------
def lines_both(hip, det, imgs):
    """(host-buffer results, `_dev` results) of an Lsd or Fld detector: lists of per-image (records, responses)"""
    import torch
    B, M = det.B, det.M
    host = det.detect(imgs)
    img = to_dev(imgs)
    rec, resp, n = zeros_dev((B, M, capi.KEYLINE_DTYPE.itemsize), torch.uint8), zeros_dev((B, M), torch.float32), zeros_dev((B,), torch.int32)
    det.detect_dev(img.data_ptr(), rec.data_ptr(), resp.data_ptr(), n.data_ptr())
    hip.synchronize()
    nn = n.cpu().numpy()
    r = rec.cpu().numpy().view(capi.KEYLINE_DTYPE).reshape(B, M)
    return host, [(r[b, :nn[b]].copy(), resp[b, :nn[b]].cpu().numpy()) for b in range(B)]


def lines_same(host, dev, what):
    found = 0
    for b, ((hr, hs), (dr, ds)) in enumerate(zip(host, dev)):
        assert len(hr) == len(dr) and hr.tobytes() == dr.tobytes(), (what, b)
        assert hs.tobytes() == ds.tobytes(), (what, b)
        found += len(hr)
    print(what, "key-lines:", sum(len(h[0]) for h in host))
    assert found >= 1, what


LSD_CASES = {"scale1": dict(scale=1.0), "scale0.8": dict(scale=0.8), "refine": dict(scale=1.0, refine=1)}


@pytest.mark.parametrize("name", list(LSD_CASES))
def test_lsd_entry_points_agree(hip, name):
    lsd = capi.Lsd(hip, 2, 64, 48, capi.lsd_params(**LSD_CASES[name]), max_keylines=64)
    try:
        first = lines_both(hip, lsd, scenes(41, 2, 64, 48))
        lines_same(*first, (name, "first"))
        second = lines_both(hip, lsd, scenes(59, 2, 64, 48))
        lines_same(*second, (name, "second"))
        assert any(a[0].tobytes() != b[0].tobytes() for a, b in zip(first[0], second[0]))
    finally:
        lsd.close()


def test_lsd_entry_points_agree_above_the_small_batch_route(hip):
    """one image more than the many-wave search takes (LSD_WAVES_MAX_B = 128): the detector has no second arena"""
    B = 129
    four = scenes(71, 4, 32, 32)
    lsd = capi.Lsd(hip, B, 32, 32, capi.lsd_params(scale=1.0), max_keylines=32)
    try:
        lines_same(*lines_both(hip, lsd, four[np.arange(B) % 4]), "B129 first")
        lines_same(*lines_both(hip, lsd, four[(np.arange(B) + 1) % 4]), "B129 second")
    finally:
        lsd.close()


def test_fld_entry_points_agree(hip):
    fld = capi.Fld(hip, 2, 64, 48, capi.fld_params(5), max_keylines=64)
    try:
        first = lines_both(hip, fld, scenes(83, 2, 64, 48))
        lines_same(*first, "fld first")
        second = lines_both(hip, fld, scenes(97, 2, 64, 48))
        lines_same(*second, "fld second")
        assert any(a[0].tobytes() != b[0].tobytes() for a, b in zip(first[0], second[0]))
    finally:
        fld.close()


# ---- LBD ---------------------------------------------------------------------------------------------------------------------------
def lbd_both(hip, lbd, lsd, imgs, want_float):
    """the key-lines of `lsd` (at most lbd.M per image) described through both entry points, compared -> the byte descriptors per image"""
    import torch
    B, M = lbd.B, lbd.M
    found = lsd.detect(imgs)
    lines = [np.stack([r[f] for f in ("sx", "sy", "ex", "ey", "angle")], axis=1) for r, _ in found]
    host = lbd.compute(imgs, lines, [r["num_pixels"] for r, _ in found], want_float=want_float)
    host_d, host_f = host if want_float else (host, None)
    rec = np.zeros((B, M), capi.KEYLINE_DTYPE)
    for b, (r, _) in enumerate(found):
        rec[b, :len(r)] = r
    n = np.array([len(r) for r, _ in found], np.int32)
    img, drec, dn = to_dev(imgs), to_dev(rec.view(np.uint8)), to_dev(n)
    desc, df = zeros_dev((B, M, 32), torch.uint8), zeros_dev((B, M, 72), torch.float32)
    lbd.compute_dev(img.data_ptr(), drec.data_ptr(), dn.data_ptr(), desc.data_ptr(), df.data_ptr() if want_float else None)
    hip.synchronize()
    for b in range(B):
        assert host_d[b].tobytes() == desc[b, :n[b]].cpu().numpy().tobytes(), b
        if want_float:
            assert host_f[b].tobytes() == df[b, :n[b]].cpu().numpy().tobytes(), b
            assert n[b] == 0 or np.abs(host_f[b]).max() > 0
    if not want_float:
        assert not df.cpu().numpy().any()  # no float descriptor asked for, none written
    print("lbd key-lines:", n.tolist())
    assert n.sum() >= 1
    return [d.copy() for d in host_d]


@pytest.mark.parametrize("want_float", [False, True], ids=["bytes", "bytes+float"])
def test_lbd_entry_points_agree(hip, want_float):
    prm = capi.lsd_params(scale=1.0, nfeatures=8)
    small_lsd, small = capi.Lsd(hip, 1, 48, 32, prm, max_keylines=8), capi.Lbd(hip, 1, 48, 32, max_keylines=8)
    lsd = lbd = None
    try:
        lbd_both(hip, small, small_lsd, scenes(101, 1, 48, 32), want_float)  # the smaller object first
        lsd, lbd = capi.Lsd(hip, 2, 64, 48, prm, max_keylines=8), capi.Lbd(hip, 2, 64, 48, max_keylines=8)
        first = lbd_both(hip, lbd, lsd, scenes(41, 2, 64, 48), want_float)
        second = lbd_both(hip, lbd, lsd, scenes(59, 2, 64, 48), want_float)
        assert any(a.tobytes() != b.tobytes() for a, b in zip(first, second))
        lbd_both(hip, small, small_lsd, scenes(103, 1, 48, 32), want_float)
    finally:
        for o in (lbd, lsd, small, small_lsd):
            if o is not None:
                o.close()
