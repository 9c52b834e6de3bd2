"""The many-wave search under a size table: lsd_grow_xcd_kernel<false, true> (csrc/lsd_kernels.hip), launched for a detector of up to 128
images once stvo_lsd_set_table_route(STVO_LSD_TABLE_BY_BATCH) says that a table does not change the route (csrc/lsd_route.h).  The
committing wave alone is the sequential search, so every image must come back byte for byte as the one-wave route under the same table
gives it — hence as a detector of its own size gives it for the crop, and as the oracle states it.  The harness, the slots of 200 x 136,
the five sizes on the seams of the kernels and the scenes are those of tests/test_gpu_lsd_sizes.py (and, at lsd_scale 0.5, of
tests/test_gpu_lsd_scale_sizes.py).

  1  every image is its own crop on the many-wave route: 10, 2 and 5 images, lsd_scale 1, 1.2 and 0.5, uncut and cut, a minimum length
     per entry; every detection twice (the second on the scratch the first left), then once more on the one-wave route
  2  whatever the speculation does (none at all; a feeder never ahead; 124 waves crowding each other) the result is the one-wave route's
  3  tables that change behind detections that have only been enqueued — the slot's own size, every image shrunk (a larger image's ranks
     stay behind the end mark of the pseudo-ordering), the sizes permuted, no table, the first again — with the route toggled in between
  4  images of 8 x 8, 16 x 9 and 64 x 8 — fewer pixels than one batch of 64 ranks, than one span of 256 — beside a full slot
  5  where the setter must not change the route: lsd_refine 1, 129 images, STVO_LSD_WAVES=0, a value that is refused
  6  a seeded random pass: sizes, batch sizes 1 .. 24, scenes, noise and flat images"""
import numpy as np
import pytest

import lsd_scale_statement as st
import test_gpu_lsd_scale_sizes as sbase
import test_gpu_lsd_sizes as base
from stvo_amd import synth

pytestmark = pytest.mark.gpu

SLOT, SIZES, PERM, K, ML, MIN_LENGTHS, NF_CUT = base.SLOT, base.SIZES, base.PERM, base.K, base.ML, base.MIN_LENGTHS, base.NF_CUT
# the tables of test 1 per batch size: five sizes twice (two images per XCD), two images, five (no multiple of 8); image i is scene i of
# the harness, whose crops at SIZES[i % 5] and PERM[i % 5] are the ones picked to end a key-line at their own border
TABLES = {10: (SIZES, MIN_LENGTHS), 2: (SIZES[:2], MIN_LENGTHS[:2]), 5: (PERM, [MIN_LENGTHS[(e + 2) % 5] for e in range(5)])}
SMALL = [(200, 136), (8, 8), (16, 9), (64, 8)]     # test 4
# The scenes of test 4, picked on the CPU with the oracle (which takes all three sizes): the crops at 16 x 9 and 64 x 8 hold a segment at
# scale 1, and no crop's answer rests on a region within 64 pixels of its image's pixel count.  There lsd_grow_fast's list bound binds
# (its comment: images of w + h <= 64 scaled pixels — 8 x 8, 16 x 9 and every entry here at scale 0.5), in every search kernel and on
# either route as before this change: an 8 x 8 image grows no region at all, so its scene is one in which the oracle finds none.
SMALL_SEEDS = [3000, 3007, 3002, 3003]
RANDOM_SEEDS = [2, 9, 14, 23, 38, 39]              # test 6: 21, 11, 4, 1, 6 and 24 images (chosen on the CPU with the oracle: at most a quarter of the images below 5 segments)


def mod_for(scale):
    """the harness of a scale: the oracle's own detector at 1 and 1.2 (blur radius 3), the composed statement at 0.5 (radius 5)"""
    return sbase if scale == 0.5 else base


def routes():
    from stvo_amd import capi
    return capi.LSD_TABLE_ONE_WAVE, capi.LSD_TABLE_BY_BATCH, capi.LSD_SEARCH_ONE_WAVE, capi.LSD_SEARCH_ONE_WAVE_PLAIN, capi.LSD_SEARCH_MANY_WAVES


def same_run(a, b, n_img, what):
    """everything two detections left (base.run), byte for byte"""
    for i in range(n_img):
        base.same_bytes(a["det"][i], b["det"][i], what + (i,))
        assert (a["n_seg"][i], a["n_pass"][i], a["n"][i]) == (b["n_seg"][i], b["n_pass"][i], b["n"][i]), what + (i,)
        assert a["segs"][i].tobytes() == b["segs"][i].tobytes(), what + (i,)
    assert np.array_equal(a["scaled"], b["scaled"]), what


def slots_of(images, sizes, noise_seed=78):
    """[len(images)][rows][cols]: seeded noise everywhere, then image i top-left in its slot at sizes[i % n]"""
    rng = np.random.default_rng(noise_seed)
    buf = rng.integers(0, 256, (len(images), SLOT[1], SLOT[0])).astype(np.uint8)
    for i, sc in enumerate(images):
        c, r = sizes[i % len(sizes)]
        buf[i, :r, :c] = sc[:r, :c]
    return buf


def check_crops(hip, oracle, out, buf, sizes, setting, min_lengths, mod):
    """base.check for any number of images: every image against a detector of its own size on the crop, and against the oracle"""
    from stvo_amd import capi
    scale, refine, nf = setting
    n, n_img = len(sizes), len(buf)
    for e, size in enumerate(sizes):
        ml = ML if min_lengths is None else min_lengths[e]
        members = [i for i in range(n_img) if i % n == e]
        imgs = np.stack([base.crop(buf[i], size) for i in members])
        prm = mod.params(scale, refine, nf, ml) if mod is base else mod.params(scale, refine, nf, ml, flagged=False)
        uni = capi.Lsd(hip, len(members), size[0], size[1], prm, max_keylines=K)
        try:
            ref = base.run(uni, imgs)
            gw, gh = uni.geometry["cols"], uni.geometry["rows"]
        finally:
            uni.close()
        for j, i in enumerate(members):
            what = (setting, i, size, ml)
            base.same_bytes(out["det"][i], ref["det"][j], ("uniform",) + what)
            assert (out["n_seg"][i], out["n_pass"][i], out["n"][i]) == (ref["n_seg"][j], ref["n_pass"][j], ref["n"][j]), what
            assert out["segs"][i].tobytes() == ref["segs"][j].tobytes(), what
            assert np.array_equal(out["scaled"][i, :gh, :gw], ref["scaled"][j]), what
            kl, seg = mod.reference(oracle, imgs[j], scale, refine, nf, ml)
            assert out["n"][i] == len(seg), what
            if mod is base:
                base.same_as_oracle(out["det"][i], kl, ("oracle",) + what)
                assert np.array_equal(out["segs"][i], seg), what
            else:
                st.same_segments(out["segs"][i], seg, scale)
                st.check_keylines(out["det"][i], kl)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", [0, NF_CUT])
@pytest.mark.parametrize("scale", [1.0, 1.2, 0.5])
@pytest.mark.parametrize("n_img", [10, 2, 5])
def test_every_image_is_its_own_crop_on_many_waves(hip, oracle, n_img, scale, nf):
    from stvo_amd import capi
    ONE, BY_BATCH, S_ONE, _, S_MANY = routes()
    mod, setting = mod_for(scale), (scale, 0, nf)
    sizes, mls = TABLES[n_img]
    lsd = capi.Lsd(hip, n_img, SLOT[0], SLOT[1], mod.params(scale, 0, nf), max_keylines=K)
    try:
        assert lsd.search_route() == S_MANY                 # no table: the route of the batch size
        lsd.set_image_sizes(sizes, mls)
        assert lsd.search_route() == S_ONE                  # a table under the default table route
        lsd.set_table_route(BY_BATCH)
        assert lsd.search_route() == S_MANY
        if n_img == base.B:   # the harness as it stands: sets the same table, detects, compares with detectors of each size and the oracle
            buf, first = mod.check(hip, oracle, lsd, sizes, setting, mls, guard=False)
        else:
            buf = slots_of(mod.scenes(oracle)[:n_img], sizes)
            first = base.run(lsd, buf)
            check_crops(hip, oracle, first, buf, sizes, setting, mls, mod)
        assert lsd.search_route() == S_MANY
        again = base.run(lsd, buf)                          # on the scratch the first detections left
        same_run(again, first, n_img, ("again", setting))
        lsd.set_table_route(ONE)
        assert lsd.search_route() == S_ONE
        same_run(base.run(lsd, buf), first, n_img, ("one wave", setting))
        assert sum(int(x) for x in first["n"]) >= 5 * n_img  # (the images do hold segments)
    finally:
        lsd.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("knobs", [{"STVO_LSD_XCD_BLOCKS": "0"}, {"STVO_LSD_XCD_BLOCKS": "1", "STVO_LSD_FEED_AHEAD": "0"},
                                   {"STVO_LSD_XCD_BLOCKS": "31", "STVO_LSD_SEP": "4", "STVO_LSD_AHEAD": "1000000", "STVO_LSD_FEED_AHEAD": "100000"}])
def test_the_speculation_may_do_anything_under_a_table(hip, oracle, switches, knobs):
    """the knob sets of tests/test_gpu_lsd.py::test_lsd_xcd_kernel_under_hostile_settings, on two images of different sizes (an XCD each,
    as there: 31 speculating workgroups fill one), four repeats each"""
    from stvo_amd import capi
    ONE, BY_BATCH, S_ONE, _, S_MANY = routes()
    switches(knobs)
    sizes = [(199, 135), (129, 65)]
    sc = base.scenes(oracle)
    buf = slots_of([sc[1], sc[2]], sizes)
    lsd = capi.Lsd(hip, 2, SLOT[0], SLOT[1], base.params(1.2, 0, 0), max_keylines=K)
    try:
        lsd.set_image_sizes(sizes, [ML, 2 * ML])
        assert lsd.search_route() == S_ONE
        want = base.run(lsd, buf)
        for i in range(2):   # the one-wave route under a table is the oracle's (tests/test_gpu_lsd_sizes.py): once more, here
            _, seg = base.reference(oracle, base.crop(buf[i], sizes[i]), 1.2, 0, 0, ML)
            assert want["n"][i] == len(seg) >= 5 and np.array_equal(want["segs"][i], seg), i
        lsd.set_table_route(BY_BATCH)
        assert lsd.search_route() == S_MANY
        for rep in range(4):
            same_run(base.run(lsd, buf), want, 2, ("repeat", rep))
    finally:
        lsd.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------

def test_tables_that_change_without_a_synchronisation(hip, oracle):
    import torch
    from stvo_amd import capi
    ONE, BY_BATCH, S_ONE, _, S_MANY = routes()
    B = base.B
    shrunk = [(129, 65), (128, 64), (64, 64), (64, 64), (128, 64)]   # every image smaller than under the table before
    # (sizes, minimum lengths, table route); None: no table
    steps = [([SLOT], None, BY_BATCH), (shrunk, MIN_LENGTHS, BY_BATCH), (PERM, None, ONE), (PERM, None, BY_BATCH), (None, None, BY_BATCH),
             ([SLOT], None, BY_BATCH), (shrunk, None, ONE), (SIZES, MIN_LENGTHS, BY_BATCH)]
    bufs = [base.slots(oracle, s if s is not None else [SLOT]) for s, _, _ in steps]
    lsd = capi.Lsd(hip, B, SLOT[0], SLOT[1], base.params(1.2, 0, 0), max_keylines=K)
    never = capi.Lsd(hip, B, SLOT[0], SLOT[1], base.params(1.2, 0, 0), max_keylines=K)
    try:
        want = []
        for (sizes, ml, _), buf in zip(steps, bufs):     # one after the other on the one-wave route, through the synchronising entry point
            lsd.set_image_sizes(sizes, ml)
            assert lsd.search_route() == (S_ONE if sizes is not None else S_MANY)
            want.append(lsd.detect(buf))
        dev = [dict(img=torch.from_numpy(buf).cuda(), rec=torch.zeros(B * K * capi.KEYLINE_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
                    resp=torch.zeros(B * K, dtype=torch.float32, device="cuda"), n=torch.zeros(B, dtype=torch.int32, device="cuda"))
               for buf in bufs]
        torch.cuda.synchronize()
        for (sizes, ml, route), t in zip(steps, dev):    # enqueued back to back
            lsd.set_table_route(route)
            lsd.set_image_sizes(sizes, ml)               # (the table route survives it, NULL included)
            assert lsd.search_route() == (S_ONE if sizes is not None and route == ONE else S_MANY)
            lsd.detect_dev(t["img"].data_ptr(), t["rec"].data_ptr(), t["resp"].data_ptr(), t["n"].data_ptr())
        hip.synchronize()
        for k, (t, exp) in enumerate(zip(dev, want)):
            n = t["n"].cpu().numpy()
            rec = t["rec"].cpu().numpy().view(capi.KEYLINE_DTYPE).reshape(B, K)
            resp = t["resp"].cpu().numpy().reshape(B, K)
            for i in range(B):
                base.same_bytes((rec[i, :n[i]], resp[i, :n[i]]), exp[i], ("step", k, i))
        assert any(len(want[1][i][0]) != len(want[0][i][0]) for i in range(B))   # the tables do differ in what they give
        plain = never.detect(bufs[4])                    # no table: the bytes of a detector that never saw one
        for i in range(B):
            base.same_bytes(want[4][i], plain[i], ("never", i))
    finally:
        lsd.close(); never.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------

def small_images():
    return [synth.make_image(seed, cols=SLOT[0], rows=SLOT[1], n_rects=40, n_discs=6, noise=3.0) for seed in SMALL_SEEDS]


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_the_smallest_images_beside_a_full_slot(hip, oracle, scale):
    from stvo_amd import capi
    ONE, BY_BATCH, S_ONE, _, S_MANY = routes()
    mod, setting = mod_for(scale), (scale, 0, 0)
    buf = slots_of(small_images(), SMALL)
    mls = [ML, 1.0, 1.0, 1.0]
    if scale == 1.0:   # below one batch of 64 ranks, one span of 256 ranks, and just above: 64, 144, 512 pixels
        assert [c * r for c, r in SMALL[1:]] == [64, 144, 512]
        for e in (2, 3):
            assert len(base.reference(oracle, base.crop(buf[e], SMALL[e]), 1.0, 0, 0, 1.0)[1]) >= 1, e
    lsd = capi.Lsd(hip, 4, SLOT[0], SLOT[1], mod.params(scale, 0, 0), max_keylines=K)
    try:
        lsd.set_table_route(BY_BATCH)
        lsd.set_image_sizes(SMALL, mls)
        assert lsd.search_route() == S_MANY
        first = base.run(lsd, buf)
        check_crops(hip, oracle, first, buf, SMALL, setting, mls, mod)
        same_run(base.run(lsd, buf), first, 4, ("again", scale))
        lsd.set_table_route(ONE)
        same_run(base.run(lsd, buf), first, 4, ("one wave", scale))
        assert first["n"][0] >= 5
        if scale == 0.5:   # 4 x 4, 8 x 4 and 32 x 4 scaled pixels, three defined rows: nothing a segment could come from
            geo = [capi.lsd_geometry(mod.params(scale, 0, 0), c, r) for c, r in SMALL[1:]]
            assert [(g["cols"], g["rows"]) for g in geo] == [(4, 4), (8, 4), (32, 4)]
            assert [int(first["n"][i]) for i in (1, 2)] == [0, 0]
    finally:
        lsd.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------

def test_refinement_keeps_its_kernel(hip, oracle):
    from stvo_amd import capi
    ONE, BY_BATCH, _, S_PLAIN, _ = routes()
    lsd = capi.Lsd(hip, base.B, SLOT[0], SLOT[1], base.params(1.2, 1, 0), max_keylines=K)
    try:
        assert lsd.search_route() == S_PLAIN
        lsd.set_image_sizes(SIZES, MIN_LENGTHS)
        buf = base.slots(oracle, SIZES)
        want = base.run(lsd, buf)
        lsd.set_table_route(BY_BATCH)
        assert lsd.search_route() == S_PLAIN
        same_run(base.run(lsd, buf), want, base.B, ("refine",))
        lsd.set_image_sizes(None)
        assert lsd.search_route() == S_PLAIN
    finally:
        lsd.close()


def test_129_images_have_no_arena(hip, oracle):
    from stvo_amd import capi
    ONE, BY_BATCH, S_ONE, _, S_MANY = routes()
    sizes = SIZES[:3]                                       # 129 = 3 x 43
    sc = base.scenes(oracle)
    buf = slots_of([sc[i % 3] for i in range(129)], sizes)
    lsd = capi.Lsd(hip, 129, SLOT[0], SLOT[1], base.params(1.2, 0, 0), max_keylines=64)
    small = capi.Lsd(hip, 3, SLOT[0], SLOT[1], base.params(1.2, 0, 0), max_keylines=64)
    try:
        assert lsd.search_route() == S_ONE and small.search_route() == S_MANY
        lsd.set_image_sizes(sizes)
        want = lsd.detect(buf)
        lsd.set_table_route(BY_BATCH)                       # taken, and the detector stays on one wave
        assert lsd.search_route() == S_ONE
        got = lsd.detect(buf)
        small.set_table_route(BY_BATCH)
        small.set_image_sizes(sizes)
        assert small.search_route() == S_MANY
        three = small.detect(buf[:3])
        for i in range(129):
            base.same_bytes(got[i], want[i], ("129", i))
            base.same_bytes(got[i], three[i % 3], ("129 against 3", i))   # (image i is image i % 3)
        assert all(len(three[i][0]) >= 5 for i in range(3))
    finally:
        lsd.close(); small.close()


def test_waves_switched_off_and_a_refused_value(hip, oracle, switches):
    from stvo_amd import capi
    ONE, BY_BATCH, S_ONE, _, S_MANY = routes()
    buf = base.slots(oracle, SIZES)
    lsd = capi.Lsd(hip, base.B, SLOT[0], SLOT[1], base.params(1.2, 0, 0), max_keylines=K)
    try:
        lsd.set_image_sizes(SIZES, MIN_LENGTHS)
        lsd.set_table_route(BY_BATCH)
        for bad in (2, -1, 1 << 20):
            with pytest.raises(capi.StvoError):
                lsd.set_table_route(bad)
            assert lsd.search_route() == S_MANY             # the route in force is kept
        assert hip.lib.stvo_lsd_set_table_route(None, BY_BATCH) != 0 and hip.lib.stvo_lsd_search_route(lsd.h, None) != 0
        want = base.run(lsd, buf)
        lsd.set_table_route(ONE)
        for bad in (2, -1):
            with pytest.raises(capi.StvoError):
                lsd.set_table_route(bad)
            assert lsd.search_route() == S_ONE
    finally:
        lsd.close()
    switches({"STVO_LSD_WAVES": "0"})                       # read at creation: no arena
    off = capi.Lsd(hip, base.B, SLOT[0], SLOT[1], base.params(1.2, 0, 0), max_keylines=K)
    try:
        assert off.search_route() == S_ONE
        off.set_table_route(BY_BATCH)
        off.set_image_sizes(SIZES, MIN_LENGTHS)
        assert off.search_route() == S_ONE
        same_run(base.run(off, buf), want, base.B, ("waves off",))
    finally:
        off.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------

def random_case(seed):
    """-> (sizes [B], images [B] at slot size): B in 1 .. 24, sizes inside the slot, a scene, noise or a flat image each"""
    rng = np.random.default_rng(seed)
    n_img = int(rng.integers(1, 25))
    sizes, images = [], []
    for i in range(n_img):
        sizes.append((int(rng.integers(24, SLOT[0] + 1)), int(rng.integers(16, SLOT[1] + 1))))
        kind = int(rng.integers(0, 8))
        if kind == 0:
            img = np.full((SLOT[1], SLOT[0]), int(rng.integers(0, 256)), np.uint8)
        elif kind == 1:
            img = rng.integers(0, 256, (SLOT[1], SLOT[0])).astype(np.uint8)
        else:
            img = synth.make_image(1000 * seed + i, cols=SLOT[0], rows=SLOT[1], n_rects=40, n_discs=6, noise=3.0)
        images.append(img)
    return sizes, images


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_tables_on_both_routes(hip, oracle, seed):
    from stvo_amd import capi
    ONE, BY_BATCH, S_ONE, _, S_MANY = routes()
    sizes, images = random_case(seed)
    n_img = len(sizes)
    buf = slots_of(images, sizes, noise_seed=seed)
    scale = (1.2, 1.0)[seed % 2]
    lsd = capi.Lsd(hip, n_img, SLOT[0], SLOT[1], base.params(scale, 0, 0), max_keylines=K)
    try:
        lsd.set_image_sizes(sizes)
        assert lsd.search_route() == S_ONE
        want = base.run(lsd, buf)
        lsd.set_table_route(BY_BATCH)
        assert lsd.search_route() == S_MANY
        same_run(base.run(lsd, buf), want, n_img, ("seed", seed))
        assert sum(int(n) < 5 for n in want["n"]) * 4 <= n_img, want["n"]   # an image with no segment shows little
        i = int(np.argmax(want["n"]))                                          # and the one-wave route is the oracle's: one image per seed
        seg = oracle.lsd_segments(base.crop(buf[i], sizes[i]), oracle.lsd_opts(refine=0, scale=scale))
        assert want["n"][i] == len(seg) and np.array_equal(want["segs"][i], seg), i
    finally:
        lsd.close()
