"""One image size per image in the LBD line descriptor (stvo_lbd_set_image_sizes, the MIXED instances of csrc/lbd_kernels.hip and of the
shared blur): in slots of 200 x 136 whose remainder holds noise, the descriptors (and float descriptors) of every image's key-lines must
be, bit for bit, those of the oracle on the crop and of a descriptor object created at that image's own size.

The slots, sizes and scenes are those of tests/test_gpu_lsd_sizes.py; the key-lines are the oracle's own detections on each crop.  A
descriptor that took the slot's border (for the blur's and the Sobel's reflection, or for the clamp of the 63-row support region) must
fail: every image smaller than its slot has a key-line whose support region crosses the image's right or bottom border — picked on the
CPU — and the oracle's descriptors of the crop differ from its descriptors of the whole noisy slot for the same lines."""
import numpy as np
import pytest

import test_gpu_lsd_sizes as L

pytestmark = pytest.mark.gpu

SLOT, SIZES, PERM, B, K = L.SLOT, L.SIZES, L.PERM, L.B, L.K

_lines = {}


def keylines(oracle, img):
    """the oracle's key-lines of one crop as (lines [n, 5], num_pixels [n])"""
    key = (img.tobytes(), img.shape)
    if key not in _lines:
        kl, _ = L.reference(oracle, img, 1.2, 0, 0, L.ML)
        _lines[key] = (np.stack([kl[f] for f in ("sx", "sy", "ex", "ey", "angle")], 1).astype(np.float32), kl["num_pixels"].astype(np.int32))
    return _lines[key]


def crosses_border(lines, npx, size):
    """key-lines whose support region (63 rows across, num_pixels along: computeLBD's corner arithmetic) reaches past the image's last
    column or row"""
    half_h = 31.0
    half_w = ((npx.astype(np.int16).astype(np.int32) - 1) // 2).astype(np.float64)
    mx, my = 0.5 * (lines[:, 0] + lines[:, 2]), 0.5 * (lines[:, 1] + lines[:, 3])
    c, s = np.cos(lines[:, 4].astype(np.float64)), np.sin(lines[:, 4].astype(np.float64))
    xs = np.stack([mx + a * c * half_w + b * s * half_h for a in (-1, 1) for b in (-1, 1)])
    ys = np.stack([my + a * s * half_w + b * c * half_h for a in (-1, 1) for b in (-1, 1)])
    return (xs.max(0) > size[0] - 1) | (ys.max(0) > size[1] - 1)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check(hip, oracle, lbd, sizes, guard):
    from stvo_amd import capi
    buf = L.slots(oracle, sizes)
    n = len(sizes)
    sets = [keylines(oracle, L.crop(buf[i], sizes[i % n])) for i in range(B)]
    assert all(0 < len(s[0]) <= K for s in sets)
    lbd.set_image_sizes(sizes)
    got, got_f = lbd.compute(buf, [s[0] for s in sets], [s[1] for s in sets], want_float=True)
    for e, size in enumerate(sizes):
        members = [i for i in range(B) if i % n == e]
        imgs = np.stack([L.crop(buf[i], size) for i in members])
        uni = capi.Lbd(hip, len(members), size[0], size[1], max_keylines=K)
        try:
            ref, ref_f = uni.compute(imgs, [sets[i][0] for i in members], [sets[i][1] for i in members], want_float=True)
        finally:
            uni.close()
        for j, i in enumerate(members):
            assert same_bits(got_f[i], ref_f[j]) and np.array_equal(got[i], ref[j]), ("uniform", i, size)
            orc, orc_f = oracle.lbd_compute(imgs[j], sets[i][0], sets[i][1], want_float=True)
            assert same_bits(got_f[i], orc_f) and np.array_equal(got[i], orc), ("oracle", i, size)
            if guard and size != SLOT:
                # on the CPU: a line's support region crosses this image's border, and the slot's border gives other descriptors
                assert crosses_border(sets[i][0], sets[i][1], size).any(), (i, size)
                slot_d, slot_f = oracle.lbd_compute(buf[i], sets[i][0], sets[i][1], want_float=True)
                assert not same_bits(slot_f, orc_f), (i, size)
    return buf, sets, got, got_f


def test_every_image_is_its_own_crop(hip, oracle):
    from stvo_amd import capi
    lbd = capi.Lbd(hip, B, SLOT[0], SLOT[1], max_keylines=K)
    try:
        check(hip, oracle, lbd, SIZES, guard=True)            # n = B / 2
        check(hip, oracle, lbd, SIZES + PERM, guard=True)     # n = B
        # no table: every image fills its slot, noise included, as on an object that never had one
        buf, sets, _, _ = check(hip, oracle, lbd, PERM, guard=False)
        lbd.set_image_sizes(None)
        full, full_f = lbd.compute(buf, [s[0] for s in sets], [s[1] for s in sets], want_float=True)
        for i in range(B):
            orc, orc_f = oracle.lbd_compute(buf[i], sets[i][0], sets[i][1], want_float=True)
            assert same_bits(full_f[i], orc_f) and np.array_equal(full[i], orc), ("no table", i)
    finally:
        lbd.close()


def test_two_tables_without_a_synchronisation_and_refusals(hip, oracle):
    import torch
    from stvo_amd import capi
    lbd = capi.Lbd(hip, B, SLOT[0], SLOT[1], max_keylines=K)
    try:
        tables = [SIZES, PERM]
        want, dev = [], []
        for sizes in tables:
            buf, sets, got, _ = check(hip, oracle, lbd, sizes, guard=False)
            want.append(got)
            rec = np.zeros((B, K), capi.KEYLINE_DTYPE)
            n = np.zeros(B, np.int32)
            for b in range(B):
                ln, npx = sets[b]
                n[b] = len(ln)
                for k, f in enumerate(("sx", "sy", "ex", "ey", "angle")):
                    rec[f][b, :len(ln)] = ln[:, k]
                rec["num_pixels"][b, :len(ln)] = npx
            dev.append(dict(img=torch.from_numpy(buf).cuda(), rec=torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda(),
                            n=torch.from_numpy(n).cuda(), desc=torch.zeros(B * K * 32, dtype=torch.uint8, device="cuda"), nn=n))
        torch.cuda.synchronize()
        for sizes, t in zip(tables, dev):   # enqueued back to back: each computation reads its own table
            lbd.set_image_sizes(sizes)
            lbd.compute_dev(t["img"].data_ptr(), t["rec"].data_ptr(), t["n"].data_ptr(), t["desc"].data_ptr())
        hip.synchronize()
        for t, exp in zip(dev, want):
            d = t["desc"].cpu().numpy().reshape(B, K, 32)
            for i in range(B):
                assert np.array_equal(d[i, :t["nn"][i]], exp[i]), ("back to back", i)
        # every refusal leaves the previous table (PERM) in force
        for sizes in ([(200, 136)] * 3, [(200, 136)] * 11, [(201, 136)], [(200, 137)], [(7, 64)], [(64, 7)]):
            with pytest.raises(capi.StvoError):
                lbd.set_image_sizes(sizes)
        one = np.array([[128, 64]], np.int32)
        assert hip.lib.stvo_lbd_set_image_sizes(lbd.h, one.ctypes.data, 0) != 0
        assert hip.lib.stvo_lbd_set_image_sizes(None, one.ctypes.data, 1) != 0
        with pytest.raises(ValueError):
            lbd.set_image_sizes([200, 136])
        t = dev[1]
        lbd.compute_dev(t["img"].data_ptr(), t["rec"].data_ptr(), t["n"].data_ptr(), t["desc"].data_ptr())
        hip.synchronize()
        d = t["desc"].cpu().numpy().reshape(B, K, 32)
        for i in range(B):
            assert np.array_equal(d[i, :t["nn"][i]], want[1][i]), ("refused", i)
    finally:
        lbd.close()
