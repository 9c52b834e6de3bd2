"""One image size per image in the ORB front-end (stvo_orb_set_image_sizes, the MIXED instances of csrc/orb_kernels.hip): every image of
a batch of slots 200 x 136 must come back, bit for bit, as the oracle (and a detector created at that image's own size) gives it for the
crop — key-points, responses, angles, octaves, descriptors, n_kp, n_total — while the rest of every slot holds noise.

The five sizes sit on the seams of the kernels: the full slot; 199 x 135 (cols % 4 = 3: the word loads and the blur's last word);
129 x 65 (one pixel past the 64 x 64 FAST tile and the 16-row blur tile); 128 x 64 (on them); 64 x 64 (the smallest create accepts — at
four levels of 1.2 its level 3 is 37 wide and yields nothing while the slot's level 3, 116 wide, runs for the other images).

A detector that ignored the sizes (or took the slot's border, reflection or resize ratio) must fail: every image has a key-point within
edge_threshold + 3 of its own right or bottom border (the scene seeds are picked for that on the CPU, with the oracle), where the noise
beyond the border is inside the FAST circle's reach of the next pixel, inside the blur's taps and inside the patch of the descriptor."""
import numpy as np
import pytest

import np_harris
from stvo_amd import synth

pytestmark = pytest.mark.gpu

SLOT = (200, 136)                                                      # cols, rows
SIZES = [(200, 136), (199, 135), (129, 65), (128, 64), (64, 64)]
B, NF, K, TH, EDGE, SCALE = 10, 300, 512, 20, 19, 1.2
KEYS = ("kp", "response", "angle", "desc", "octave")
TH_PER_IMAGE = [14, 27]                                                # image i takes entry i % 2: not the period of the sizes

_scenes = {}
_refs = {}


def crop(scene, size):
    return np.ascontiguousarray(scene[:size[1], :size[0]])


def reference(oracle, img, nlevels, score, th=TH):
    """the statement for one image: the oracle's pyramid under orb_score 1, tests/np_harris.py's composition under orb_score 0"""
    ref = np_harris.detect_levels(oracle, img, NF, nlevels, SCALE, th, EDGE, cap=K, score=score)
    if score == 1:
        own = oracle.orb_detect_levels(img, NF, nlevels, SCALE, th, EDGE, cap=K)
        for k in KEYS:
            assert np.array_equal(own[k].view(np.uint8), ref[k].view(np.uint8)), k
    return ref


def near_border(ref, size):
    lvl0 = ref["kp"][ref["octave"] == 0]
    return len(lvl0) and bool(np.any((lvl0[:, 0] >= size[0] - (EDGE + 3)) | (lvl0[:, 1] >= size[1] - (EDGE + 3))))


def scenes(oracle):
    """image i: a scene of its own at slot size, of which it is the top-left crop.  The seed is the first whose crop at SIZES[i % 5] has a
    level-0 key-point near its right or bottom border under every setting the oracle states."""
    if not _scenes:
        for i in range(B):
            for seed in range(1000 + 100 * i, 1100 + 100 * i):
                sc = synth.make_image(seed, cols=SLOT[0], rows=SLOT[1], n_rects=60, n_discs=16, noise=4.0)
                img = crop(sc, SIZES[i % 5])
                if all(near_border(reference(oracle, img, nl, s, th), SIZES[i % 5])
                       for nl in (1, 4) for s in (1, 0) for th in {TH, TH_PER_IMAGE[i % 2]}):
                    _scenes[i] = sc
                    break
            assert i in _scenes, "no seed puts a key-point near the border of image %d" % i
    return [_scenes[i] for i in range(B)]


def slots(oracle, sizes):
    """[B][rows][cols]: seeded noise everywhere, then every image top-left in its slot"""
    rng = np.random.default_rng(77)
    buf = rng.integers(0, 256, (B, SLOT[1], SLOT[0])).astype(np.uint8)
    for i, sc in enumerate(scenes(oracle)):
        c, r = sizes[i % len(sizes)]
        buf[i, :r, :c] = sc[:r, :c]
    return buf


def same(got, ref, what):
    for k in KEYS:
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), (what, k)   # bitwise, floats included
    assert got["n_total"] == ref["n_total"], what


def uniform(hip, imgs, size, th, **kw):
    """a detector created at `size`, on images of that size"""
    from stvo_amd import capi
    orb = capi.Orb(hip, len(imgs), size[0], size[1], max_keypoints=K, nfeatures=NF, fast_threshold=TH, edge_threshold=EDGE,
                   scale_factor=SCALE, **kw)
    try:
        if th is not None:
            orb.set_fast_thresholds(th)
        return orb.detect(np.stack(imgs))
    finally:
        orb.close()


def check(hip, oracle, orb, sizes, nlevels, score, wta, th, guard):
    buf = slots(oracle, sizes)
    orb.set_image_sizes(sizes)
    out = orb.detect(buf)
    n = len(sizes)
    for e, size in enumerate(sizes):
        members = [i for i in range(B) if i % n == e]
        imgs = [crop(buf[i], size) for i in members]
        uni = uniform(hip, imgs, size, None if th is None else [th[i % len(th)] for i in members], nlevels=nlevels, score=score,
                      wta_k=wta[0], patch_size=wta[1])
        for j, i in enumerate(members):
            same(out[i], uni[j], ("uniform", i, size))
            if wta == (2, 31):   # (the oracle states this descriptor only)
                key = (i, size, nlevels, score, TH if th is None else th[i % len(th)])
                if key not in _refs:
                    _refs[key] = reference(oracle, imgs[j], nlevels, score, key[4])
                same(out[i], _refs[key], ("oracle", i, size))
                if guard:
                    assert near_border(_refs[key], size), (i, size)
    return buf, out


CASES = [(1, 1, (2, 31), False), (4, 1, (2, 31), False), (1, 0, (2, 31), False), (4, 0, (2, 31), False), (4, 1, (3, 31), False),
         (4, 1, (2, 21), False), (4, 1, (2, 31), True)]


@pytest.mark.parametrize("nlevels,score,wta,per_image_th", CASES,
                         ids=["n%d-s%d-w%d-p%d%s" % (c[0], c[1], c[2][0], c[2][1], "-th" if c[3] else "") for c in CASES])
def test_every_image_is_its_own_crop(hip, oracle, nlevels, score, wta, per_image_th):
    from stvo_amd import capi
    th = TH_PER_IMAGE if per_image_th else None
    orb = capi.Orb(hip, B, SLOT[0], SLOT[1], max_keypoints=K, nfeatures=NF, fast_threshold=TH, edge_threshold=EDGE, nlevels=nlevels,
                   scale_factor=SCALE, score=score, wta_k=wta[0], patch_size=wta[1])
    try:
        if th is not None:
            orb.set_fast_thresholds(th)
        _, out = check(hip, oracle, orb, SIZES, nlevels, score, wta, th, guard=True)
        if nlevels == 4:   # 64 x 64: levels 0 .. 2 only (level 3 is below the border), the full slot reaches level 3
            assert out[4]["octave"].max() <= 2 and out[0]["octave"].max() == 3
        # the sizes in another order, set again on the same detector: every image changes its size
        perm = [SIZES[(e + 2) % 5] for e in range(5)]
        check(hip, oracle, orb, perm, nlevels, score, wta, th, guard=False)
        # and a table of B entries, left and right images of a pair no longer alike
        check(hip, oracle, orb, SIZES + perm, nlevels, score, wta, th, guard=False)
        # no table: every image fills its slot, noise included, as on a detector that never had one
        orb.set_image_sizes(None)
        buf = slots(oracle, SIZES)
        full = orb.detect(buf)
        uni = uniform(hip, list(buf), SLOT, th, nlevels=nlevels, score=score, wta_k=wta[0], patch_size=wta[1])
        for i in range(B):
            same(full[i], uni[i], ("no table", i))
    finally:
        orb.close()


def test_argument_checks(hip, oracle):
    from stvo_amd import capi
    orb = capi.Orb(hip, B, SLOT[0], SLOT[1], max_keypoints=K, nfeatures=NF, fast_threshold=TH, edge_threshold=EDGE, nlevels=4,
                   scale_factor=SCALE)
    try:
        buf = slots(oracle, SIZES)
        orb.set_image_sizes(SIZES)
        before = orb.detect(buf)
        bad = [[(200, 136)] * 3,                      # B % n != 0
               [(200, 136)] * 11,                     # n > B
               [(201, 136)], [(200, 137)],            # larger than the slot
               [(63, 64)], [(64, 63)],                # below what stvo_orb_create takes
               [(200, 136), (128, 64), (64, 32), (128, 64), (64, 64)]]
        for sizes in bad:
            with pytest.raises(capi.StvoError):
                orb.set_image_sizes(sizes)
        lib = hip.lib
        one = np.array([[128, 64]], np.int32)
        assert lib.stvo_orb_set_image_sizes(orb.h, one.ctypes.data, 0) != 0       # n <= 0
        assert lib.stvo_orb_set_image_sizes(orb.h, one.ctypes.data, -1) != 0
        assert lib.stvo_orb_set_image_sizes(None, one.ctypes.data, 1) != 0
        with pytest.raises(ValueError):
            orb.set_image_sizes([200, 136])
        after = orb.detect(buf)   # a refused call changes nothing
        for i in range(B):
            same(after[i], before[i], ("refused", i))
    finally:
        orb.close()
    # 2 * edge_threshold >= a side
    orb = capi.Orb(hip, 2, SLOT[0], SLOT[1], max_keypoints=K, nfeatures=NF, edge_threshold=32)
    try:
        with pytest.raises(capi.StvoError):
            orb.set_image_sizes([(64, 64)])
        orb.set_image_sizes([(65, 65)])
    finally:
        orb.close()
