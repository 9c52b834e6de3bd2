"""One image size, and minimum length, per image in the LSD key-line detector (stvo_lsd_set_image_sizes, the MIXED instances of
csrc/lsd_kernels.hip): every image of a batch of slots 200 x 136 must come back, bit for bit, as a detector created at that image's own
size with that minimum length gives it for the crop, and as the oracle states it — key-line records, responses, n_lines, the counts,
the raw segments and the scaled image — while the rest of every slot holds noise.

The five sizes sit on the seams of the kernels: the full slot; 199 x 135 (cols % 4 = 3, rows % 16 != 0: the blur's last word, the
16-row tiles of the gradient); 129 x 65 and 128 x 64 (one past and on the 64 x 64 unit of the counting sort and the 16-row tiles, in
the input and — 155 x 78, 154 x 77 — in the scaled image); 64 x 64.

A detector that ignored the sizes (or took the slot's border, clamps, pixel count or smallest region) must fail: every image's crop has
a kept key-line with an end within 4 pixels of its own right or bottom border, under every setting run here (the scene seeds are picked
for that on the CPU, with the oracle), and the noise begins right behind that border."""
import numpy as np
import pytest

from stvo_amd import synth

pytestmark = pytest.mark.gpu

SLOT = (200, 136)                                                      # cols, rows
SIZES = [(200, 136), (199, 135), (129, 65), (128, 64), (64, 64)]
PERM = [SIZES[(e + 2) % 5] for e in range(5)]
B, K, ML, NF_CUT = 10, 512, 5.0, 4
# (scale, lsd_refine, nfeatures): both scales and both searches uncut, and the cut on either search
SETTINGS = [(1.2, 0, 0), (1.2, 1, 0), (1.0, 0, 0), (1.0, 1, 0), (1.2, 0, NF_CUT), (1.0, 1, NF_CUT)]
MIN_LENGTHS = [ML, 4 * ML, ML, 2.5 * ML, ML]                           # per entry of SIZES; two of them above the detector's own

_scenes = {}
_refs = {}


def crop(scene, size):
    return np.ascontiguousarray(scene[:size[1], :size[0]])


def reference(oracle, img, scale, refine, nf, ml):
    """the statement for one image: (key-lines, raw segments) of the oracle"""
    key = (img.tobytes(), img.shape, scale, refine, nf, ml)
    if key not in _refs:
        _refs[key] = (oracle.lsd_detect(img, oracle.lsd_opts(min_length=ml, nfeatures=nf, refine=refine, scale=scale)),
                      oracle.lsd_segments(img, oracle.lsd_opts(refine=refine, scale=scale)))
    return _refs[key]


def near_border(kl, size):
    return len(kl) > 0 and bool(np.any((np.maximum(kl["sx"], kl["ex"]) >= size[0] - 4) | (np.maximum(kl["sy"], kl["ey"]) >= size[1] - 4)))


def scenes(oracle):
    """image i: a scene of its own at slot size, of which it is the top-left crop.  The seed is the first whose crop at SIZES[i % 5] and at
    PERM[i % 5] has, under every setting, a kept key-line that ends near its own right or bottom border and more lines than the cut keeps."""
    if not _scenes:
        for i in range(B):
            for seed in range(3000 + 100 * i, 3100 + 100 * i):
                sc = synth.make_image(seed, cols=SLOT[0], rows=SLOT[1], n_rects=40, n_discs=6, noise=3.0)
                ok = True
                for size in (SIZES[i % 5], PERM[i % 5]):
                    for scale, refine, nf in SETTINGS:
                        kl, _ = reference(oracle, crop(sc, size), scale, refine, nf, ML)
                        ok = ok and near_border(kl, size) and (nf == 0 and len(kl) > NF_CUT or nf != 0 and len(kl) == NF_CUT)
                if ok:
                    _scenes[i] = sc
                    break
            assert i in _scenes, "no seed puts a key-line near the border of image %d" % i
    return [_scenes[i] for i in range(B)]


def slots(oracle, sizes):
    """[B][rows][cols]: seeded noise everywhere, then every image top-left in its slot"""
    rng = np.random.default_rng(78)
    buf = rng.integers(0, 256, (B, SLOT[1], SLOT[0])).astype(np.uint8)
    for i, sc in enumerate(scenes(oracle)):
        c, r = sizes[i % len(sizes)]
        buf[i, :r, :c] = sc[:r, :c]
    return buf


def params(scale, refine, nf, ml=ML):
    from stvo_amd import capi
    return capi.lsd_params(min_length=ml, nfeatures=nf, refine=refine, scale=scale)


def same_bytes(got, ref, what):
    (rec, resp), (urec, uresp) = got, ref
    assert len(rec) == len(urec), (what, len(rec), len(urec))
    assert rec.tobytes() == urec.tobytes(), what            # the records as they lie in memory, angle included
    assert resp.tobytes() == uresp.tobytes(), what


def same_as_oracle(got, kl, what):
    rec, resp = got
    assert len(rec) == len(kl), (what, len(rec), len(kl))
    for f in ("sx", "sy", "ex", "ey", "num_pixels"):
        assert np.array_equal(rec[f], kl[f]), (what, f)
    assert np.array_equal(resp, kl["response"]), what
    # KeyLine::angle = atan2 in double, rounded to float: the device's atan2 and the host's may differ in the last place (tests/test_gpu_lsd.py)
    assert np.allclose(rec["angle"], kl["angle"], rtol=0, atol=4e-7), what


def run(lsd, buf):
    """everything a detection leaves, through the host entry points"""
    det = lsd.detect(buf)
    n_seg, n_pass = lsd.counts()
    segs, n = lsd.segments(buf)
    return dict(det=det, n_seg=n_seg.copy(), n_pass=n_pass.copy(), segs=segs, n=n.copy(), scaled=lsd.scaled_image(buf))


def check(hip, oracle, lsd, sizes, setting, min_lengths, guard):
    from stvo_amd import capi
    scale, refine, nf = setting
    buf = slots(oracle, sizes)
    lsd.set_image_sizes(sizes, min_lengths)
    out = run(lsd, buf)
    n = len(sizes)
    for e, size in enumerate(sizes):
        ml = ML if min_lengths is None else min_lengths[e]
        members = [i for i in range(B) if i % n == e]
        imgs = np.stack([crop(buf[i], size) for i in members])
        uni = capi.Lsd(hip, len(members), size[0], size[1], params(scale, refine, nf, ml), max_keylines=K)
        try:
            ref = run(uni, imgs)
            gw, gh = uni.geometry["cols"], uni.geometry["rows"]
        finally:
            uni.close()
        for j, i in enumerate(members):
            what = (setting, i, size, ml)
            same_bytes(out["det"][i], ref["det"][j], ("uniform",) + what)
            assert (out["n_seg"][i], out["n_pass"][i], out["n"][i]) == (ref["n_seg"][j], ref["n_pass"][j], ref["n"][j]), what
            assert out["segs"][i].tobytes() == ref["segs"][j].tobytes(), what
            assert np.array_equal(out["scaled"][i, :gh, :gw], ref["scaled"][j]), what
            kl, seg = reference(oracle, imgs[j], scale, refine, nf, ml)
            same_as_oracle(out["det"][i], kl, ("oracle",) + what)
            assert out["n"][i] == len(seg) and np.array_equal(out["segs"][i], seg), what
            if guard:
                assert near_border(kl, size), what
    return buf, out


@pytest.mark.parametrize("scale,refine,nf", SETTINGS, ids=["s%g-r%d-n%d" % s for s in SETTINGS])
def test_every_image_is_its_own_crop(hip, oracle, scale, refine, nf):
    from stvo_amd import capi
    setting = (scale, refine, nf)
    lsd = capi.Lsd(hip, B, SLOT[0], SLOT[1], params(scale, refine, nf), max_keylines=K)
    try:
        check(hip, oracle, lsd, SIZES, setting, None, guard=True)               # n = B / 2
        check(hip, oracle, lsd, SIZES + PERM, setting, None, guard=True)        # n = B: every image changes its size or keeps it
        # no table: every image fills its slot, noise included, as on a detector that never had one
        lsd.set_image_sizes(None)
        buf = slots(oracle, SIZES)
        full = run(lsd, buf)
        uni = capi.Lsd(hip, B, SLOT[0], SLOT[1], params(scale, refine, nf), max_keylines=K)
        try:
            ref = run(uni, buf)
        finally:
            uni.close()
        for i in range(B):
            same_bytes(full["det"][i], ref["det"][i], ("no table", i))
            assert full["segs"][i].tobytes() == ref["segs"][i].tobytes() and np.array_equal(full["scaled"][i], ref["scaled"][i]), i
    finally:
        lsd.close()


def test_sizes_differ_where_the_slot_would_be_wrong(hip, oracle):
    """what the guard of the test above rests on, stated on the CPU: the slot's own smallest region differs from two entries', and the
    crops' key-lines are not those of the slot-sized scene they are cut from"""
    from stvo_amd import capi
    import ctypes as C
    oracle.lib.orc_lsd_min_reg_size.argtypes = [C.c_int, C.c_int, C.c_double]
    oracle.lib.orc_lsd_min_reg_size.restype = C.c_int
    mins = []
    for c, r in SIZES:
        g = capi.lsd_geometry(params(1.2, 0, 0), c, r)
        mins.append(int(oracle.lib.orc_lsd_min_reg_size(g["cols"], g["rows"], 22.5)))
    assert mins[0] == 13 and mins[4] == 11 and sum(1 for m in mins if m != mins[0]) >= 2, mins
    sc = scenes(oracle)
    for i in (1, 2, 3, 4):
        own, _ = reference(oracle, crop(sc[i], SIZES[i]), 1.2, 0, 0, ML)
        whole, _ = reference(oracle, sc[i], 1.2, 0, 0, ML)
        assert len(own) != len(whole) or own.tobytes() != whole.tobytes(), i


@pytest.mark.parametrize("scale,refine", [(1.2, 0), (1.0, 1)])
def test_minimum_length_per_entry(hip, oracle, scale, refine):
    from stvo_amd import capi
    sc = scenes(oracle)
    # on the CPU first: a raised entry drops a line that the detector's own minimum length keeps
    dropped = 0
    for i in range(B):
        e = i % 5
        kept_own, _ = reference(oracle, crop(sc[i], SIZES[e]), scale, refine, 0, ML)
        kept_entry, _ = reference(oracle, crop(sc[i], SIZES[e]), scale, refine, 0, MIN_LENGTHS[e])
        assert len(kept_entry) <= len(kept_own)
        dropped += int(MIN_LENGTHS[e] > ML and 0 < len(kept_entry) < len(kept_own))
    assert dropped >= 1
    lsd = capi.Lsd(hip, B, SLOT[0], SLOT[1], params(scale, refine, 0), max_keylines=K)
    try:
        _, out = check(hip, oracle, lsd, SIZES, (scale, refine, 0), MIN_LENGTHS, guard=False)
        # the same sizes without the list: the detector's own value for all, the lines come back
        _, own = check(hip, oracle, lsd, SIZES, (scale, refine, 0), None, guard=False)
        assert sum(len(own["det"][i][0]) > len(out["det"][i][0]) for i in range(B)) >= 1
        assert all(len(own["det"][i][0]) == len(out["det"][i][0]) for i in range(B) if MIN_LENGTHS[i % 5] == ML)
    finally:
        lsd.close()


def test_two_tables_without_a_synchronisation(hip, oracle):
    """a second table set behind a detection that has only been enqueued: each detection reads its own (the table travels on the
    context's stream, the staging blocks alternate)"""
    import torch
    from stvo_amd import capi
    setting = (1.2, 0, 0)
    tables = [(SIZES, None), (PERM, MIN_LENGTHS), (SIZES + PERM, None)]
    lsd = capi.Lsd(hip, B, SLOT[0], SLOT[1], params(*setting), max_keylines=K)
    try:
        want = []
        for sizes, ml in tables:     # one after the other, through the synchronising entry point
            lsd.set_image_sizes(sizes, ml)
            want.append(lsd.detect(slots(oracle, sizes)))
        dev = [dict(img=torch.from_numpy(slots(oracle, sizes)).cuda(), rec=torch.zeros(B * K * capi.KEYLINE_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
                    resp=torch.zeros(B * K, dtype=torch.float32, device="cuda"), n=torch.zeros(B, dtype=torch.int32, device="cuda"))
               for sizes, _ in tables]
        torch.cuda.synchronize()
        for (sizes, ml), t in zip(tables, dev):   # enqueued back to back
            lsd.set_image_sizes(sizes, ml)
            lsd.detect_dev(t["img"].data_ptr(), t["rec"].data_ptr(), t["resp"].data_ptr(), t["n"].data_ptr())
        hip.synchronize()
        for t, exp in zip(dev, want):
            n = t["n"].cpu().numpy()
            rec = t["rec"].cpu().numpy().view(capi.KEYLINE_DTYPE).reshape(B, K)
            resp = t["resp"].cpu().numpy().reshape(B, K)
            for i in range(B):
                same_bytes((rec[i, :n[i]], resp[i, :n[i]]), exp[i], ("back to back", i))
    finally:
        lsd.close()


def test_argument_checks(hip, oracle):
    from stvo_amd import capi
    lsd = capi.Lsd(hip, B, SLOT[0], SLOT[1], params(1.2, 0, 0), max_keylines=K)
    try:
        buf = slots(oracle, SIZES)
        lsd.set_image_sizes(SIZES, MIN_LENGTHS)
        before = lsd.detect(buf)
        bad = [[(200, 136)] * 3,                      # B % n != 0
               [(200, 136)] * 11,                     # n > B
               [(201, 136)], [(200, 137)],            # larger than the slot
               [(7, 64)], [(64, 7)],                  # below what stvo_lsd_create takes
               [(200, 136), (128, 64), (64, 4), (128, 64), (64, 64)]]
        for sizes in bad:
            with pytest.raises(capi.StvoError):
                lsd.set_image_sizes(sizes)
        with pytest.raises(capi.StvoError):
            lsd.set_image_sizes(SIZES, [ML, ML, float("nan"), ML, ML])
        lib = hip.lib
        one = np.array([[128, 64]], np.int32)
        assert lib.stvo_lsd_set_image_sizes(lsd.h, one.ctypes.data, None, 0) != 0       # n <= 0
        assert lib.stvo_lsd_set_image_sizes(lsd.h, one.ctypes.data, None, -1) != 0
        assert lib.stvo_lsd_set_image_sizes(None, one.ctypes.data, None, 1) != 0
        with pytest.raises(ValueError):
            lsd.set_image_sizes([200, 136])
        with pytest.raises(ValueError):
            lsd.set_image_sizes(SIZES, [ML, ML])
        after = lsd.detect(buf)   # a refused call changes nothing: the previous table, minimum lengths included, is in force
        for i in range(B):
            same_bytes(after[i], before[i], ("refused", i))
    finally:
        lsd.close()
    # a blur radius other than 3 (lsd_scale 0.5: radius 5) runs the fused blur + resize, whose tile plan is per size
    lsd = capi.Lsd(hip, 2, SLOT[0], SLOT[1], capi.lsd_params(scale=0.5), max_keylines=K)
    try:
        assert lsd.geometry["radius"] != 3
        with pytest.raises(capi.StvoError, match="unsupported"):
            lsd.set_image_sizes([(128, 64)])
        lsd.set_image_sizes(None)
    finally:
        lsd.close()
