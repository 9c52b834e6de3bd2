"""The rectifier bank on the GPU (stvo_rectify_bank_*): a calibration and an image size per pair of one launch, every crop of the
destination equal — bit for bit — to the numpy statement the uniform rectifier is held to (np_rectify.remap / np_color.remap_color /
np_color.gray applied to the crop of the source with the calibration's own maps; a copy for dist 0), and every byte outside the crops
left as it was.

Slots of 53 x 21 (an odd pitch: dword alignment changes from row to row), B = 7, calibrations 53 x 21 (the slot itself), 50 x 19,
7 x 5 (left side: the identity map), 3 x 2 (narrower than a quad), 1 x 1 from caller maps and a dist 0 calibration of 40 x 16.  The
seeded maps have integer positions in -3 .. cols + 2 and -3 .. rows + 2 and, on the two large calibrations, all 1024 fractions; the
fixture asserts what they are meant to hold: beyond each of the four sides pixels with none, one column / row (2 taps) and all 4 of
their taps outside (a 2 x 2 footprint on a rectangle never has exactly 1 tap beyond a side: the corner case, 3 taps outside, is asserted
instead), quads mixing inside and border pixels, quads straddling two rows.  Sources are noise over the whole slot, so a tap that
wrongly reads the slot beyond the image shows; destinations are prefilled with other noise."""
import ctypes as C

import numpy as np
import pytest
import torch

import np_color
import np_rectify as nr
from stvo_amd import capi

pytestmark = pytest.mark.gpu

SLOT_C, SLOT_R, B = 53, 21, 7
SIZES = [(53, 21), (50, 19), (7, 5), (3, 2), (1, 1), (40, 16)]   # calibration 5: dist 0
K = len(SIZES)
INVALID = -1  # STVO_ERR_INVALID_ARG


def seeded_maps(k):
    cols, rows = SIZES[k]
    rng = np.random.default_rng(100 + k)
    m1 = np.empty((2, rows, cols, 2), np.int16)
    m1[..., 0] = rng.integers(-3, cols + 3, (2, rows, cols))
    m1[..., 1] = rng.integers(-3, rows + 3, (2, rows, cols))
    m2 = rng.integers(0, 1024, (2, rows, cols)).astype(np.uint16)
    if 2 * cols * rows >= 1024:   # all 1024 fractions over the two sides, in a seeded order
        m2.reshape(-1)[rng.permutation(2 * cols * rows)[:1024]] = np.arange(1024, dtype=np.uint16)
    if k == 2:                # the identity on the left side
        yy, xx = np.mgrid[0:rows, 0:cols]
        m1[0, ..., 0], m1[0, ..., 1], m2[0] = xx, yy, 0
    return m1, m2


def check_maps_hold_what_they_are_meant_to(m1, m2, cols, rows):
    x, y = m1[..., 0].astype(int), m1[..., 1].astype(int)
    beyond = dict(left=(x < 0).astype(int) + (x + 1 < 0), right=(x >= cols).astype(int) + (x + 1 >= cols),
                  top=(y < 0).astype(int) + (y + 1 < 0), bottom=(y >= rows).astype(int) + (y + 1 >= rows))   # tap columns / rows beyond a side
    for side, cnt in beyond.items():
        assert {0, 1, 2} <= set(np.unique(cnt).tolist()), side       # none, one column / row (2 taps), both (all 4 taps)
    out_x = beyond["left"] + beyond["right"]
    out_y = beyond["top"] + beyond["bottom"]
    taps_out = 4 - (2 - np.minimum(out_x, 2)) * (2 - np.minimum(out_y, 2))
    assert {0, 2, 3, 4} <= set(np.unique(taps_out).tolist())
    assert len(np.unique(m2)) == 1024
    inside = (taps_out == 0).reshape(2, -1)
    npx = cols * rows
    quads = inside[:, :npx - npx % 4].reshape(2, -1, 4).sum(-1)
    assert ((quads > 0) & (quads < 4)).any() and (quads == 4).any() and (quads == 0).any()
    assert cols % 4 != 0                                              # quads straddle two rows


@pytest.fixture(scope="module")
def bank(hip):
    maps = [seeded_maps(k) for k in range(K - 1)]
    check_maps_hold_what_they_are_meant_to(*maps[0], *SIZES[0])
    check_maps_hold_what_they_are_meant_to(*maps[1], *SIZES[1])
    c = capi.RectCalib()
    c.form, c.width, c.height, c.b = capi.RECT_FORM_KITTI, SIZES[5][0], SIZES[5][1], 0.1
    c.fx, c.fy, c.cx, c.cy = 30.0, 30.0, 19.5, 7.5
    c.d[:] = [0.0, 0.0, 0.0, 0.0]
    rects = [capi.Rectifier(hip, B, maps=m) for m in maps] + [capi.Rectifier(hip, B, calib=c)]
    assert [r.dist for r in rects] == [1] * 5 + [0] and [(r.cols, r.rows) for r in rects] == SIZES
    bk = capi.RectifierBank(hip, B, SLOT_C, SLOT_R, rects)
    yield bk, maps + [None], rects
    bk.close()
    for r in rects:
        r.close()


_src, _src_dev, _expect = {}, {}, {}


def source(ch):
    """[2 sides][B][slot rows][slot cols][ch] noise, the same for every test"""
    if ch not in _src:
        _src[ch] = np.random.default_rng(7 + ch).integers(0, 256, (2, B, SLOT_R, SLOT_C, ch), dtype=np.uint8)
    return _src[ch]


def source_dev(ch):
    """the same on the device, resident for the whole module: a launch that has not run yet keeps reading it"""
    if ch not in _src_dev:
        _src_dev[ch] = torch.from_numpy(source(ch)).cuda()
    return _src_dev[ch]


def prefill(shape, seed=99):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def expected_crop(maps, ch, side, b, k):
    """the rectified crop [rows_k][cols_k][ch] of pair b's source under calibration k: computed once, shared, never changed"""
    key = (ch, side, b, k)
    if key not in _expect:
        cols, rows = SIZES[k]
        crop = np.ascontiguousarray(source(ch)[side, b, :rows, :cols])
        if maps[k] is None:
            out = crop.copy()
        elif ch == 1:
            out = nr.remap(crop[..., 0], maps[k][0][side], maps[k][1][side])[..., None]
        else:
            out = np_color.remap_color(crop, maps[k][0][side], maps[k][1][side])
        out.setflags(write=False)
        _expect[key] = out
    return _expect[key]


def run(bk, n, ch, gray=None, swapped=False):
    """one call on prefilled destinations -> (list of destination arrays, list of their prefills)"""
    src = source_dev(ch)
    if gray is None:
        fills = [prefill((2, B, SLOT_R, SLOT_C, ch))]
    else:
        fills = [prefill((2, B, SLOT_R, SLOT_C), 99)] + ([prefill((2, B, SLOT_R, SLOT_C), 98)] if swapped else [])
    dst = [torch.from_numpy(f).cuda() for f in fills]
    torch.cuda.synchronize()
    if gray is None:
        bk.rectify_dev(n, ch, src[0].data_ptr(), src[1].data_ptr(), dst[0][0].data_ptr(), dst[0][1].data_ptr())
    else:
        order, weights = gray
        sw = (dst[1][0].data_ptr(), dst[1][1].data_ptr()) if swapped else (None, None)
        bk.rectify_color_to_gray_dev(n, ch, src[0].data_ptr(), src[1].data_ptr(), dst[0][0].data_ptr(), dst[0][1].data_ptr(), sw[0], sw[1],
                                     order=order, weights=weights)
    return dst, fills


def judge(dst, fills, maps, assign, n, ch, gray=None):
    """every destination against its prefill with the expected crops of the first n pairs written over it"""
    for j, (got, fill) in enumerate(zip([d.cpu().numpy() for d in dst], fills)):
        want = fill.copy()
        for side in range(2):
            for b in range(n):
                k = assign[b]
                cols, rows = SIZES[k]
                crop = expected_crop(maps, ch, side, b, k)
                if gray is not None:
                    order = gray[0] if j == 0 else ("rgb" if gray[0] == "bgr" else "bgr")
                    crop = np_color.gray(crop, order, gray[1])
                want[side, b, :rows, :cols] = crop.reshape(want[side, b, :rows, :cols].shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (j, assign, n, ch, gray, bad[:5].tolist())


MIXED = [0, 1, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("assign,n", [(MIXED, B), ([0, 1, 1, 2, 3, 5, 5], B), ([1] * B, B), ([0] * B, B), ([5] * B, B), (MIXED, 3),
                                      ([5, 4, 3, 2, 1, 0, 0], B)],
                         ids=["mixed", "one_calibration_left_out", "all_on_50x19", "all_on_the_slot", "all_on_dist0", "n3", "reversed"])
def test_remap_per_pair(hip, bank, assign, n, ch):
    bk, maps, _ = bank
    bk.assign(assign)
    dst, fills = run(bk, n, ch)
    hip.synchronize()
    judge(dst, fills, maps, assign, n, ch)


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("order", ["bgr", "rgb"])
@pytest.mark.parametrize("weights", ["q14", "q15"])
@pytest.mark.parametrize("swapped", [False, True])
def test_fused_colour_to_grey(hip, bank, ch, order, weights, swapped):
    bk, maps, _ = bank
    bk.assign(MIXED)
    dst, fills = run(bk, B, ch, gray=(order, weights), swapped=swapped)
    hip.synchronize()
    judge(dst, fills, maps, MIXED, B, ch, gray=(order, weights))


def test_fused_on_a_subset_and_on_one_calibration(hip, bank):
    bk, maps, _ = bank
    for assign, n in (([1] * B, 3), ([5] * B, B), ([0, 1, 1, 2, 3, 5, 5], B)):
        bk.assign(assign)
        dst, fills = run(bk, n, 3, gray=("bgr", "q14"), swapped=True)
        hip.synchronize()
        judge(dst, fills, maps, assign, n, 3, gray=("bgr", "q14"))


def test_two_calls_with_an_assign_between_and_no_synchronisation(hip, bank):
    bk, maps, _ = bank
    first, second = MIXED, [5, 4, 3, 2, 1, 0, 0]
    bk.assign(first)
    d1, f1 = run(bk, B, 1)
    bk.assign(second)                    # travels behind the first launch, which reads the first table
    d2, f2 = run(bk, B, 3)               # (run's torch.cuda.synchronize waits for torch's copies, not for the context's stream)
    bk.assign(first)
    d3, f3 = run(bk, B, 4, gray=("bgr", "q15"))
    hip.synchronize()
    judge(d1, f1, maps, first, B, 1)
    judge(d2, f2, maps, second, B, 3)
    judge(d3, f3, maps, first, B, 4, gray=("bgr", "q15"))


def test_every_pair_starts_on_calibration_0_and_camera_forwards(hip, bank):
    _, maps, rects = bank
    fresh = capi.RectifierBank(hip, B, SLOT_C, SLOT_R, rects)
    try:
        assert fresh.calibs == [0] * B
        dst, fills = run(fresh, B, 1)
        hip.synchronize()
        judge(dst, fills, maps, [0] * B, B, 1)
        for k, r in enumerate(rects):
            assert fresh.camera(k) == r.camera
        assert (fresh.camera(5)["width"], fresh.camera(5)["height"]) == SIZES[5]
    finally:
        fresh.close()


def test_host_conveniences(hip, bank):
    bk, maps, _ = bank
    bk.assign(MIXED)
    for ch in (1, 3):
        tail = () if ch == 1 else (ch,)
        left = [np.ascontiguousarray(source(ch)[0, b, :SIZES[k][1], :SIZES[k][0]]).reshape((SIZES[k][1], SIZES[k][0]) + tail) for b, k in enumerate(MIXED)]
        right = [np.ascontiguousarray(source(ch)[1, b, :SIZES[k][1], :SIZES[k][0]]).reshape((SIZES[k][1], SIZES[k][0]) + tail) for b, k in enumerate(MIXED)]
        out_l, out_r = bk.rectify(left, right) if ch == 1 else bk.rectify_color(left, right)
        for side, out in ((0, out_l), (1, out_r)):
            for b, k in enumerate(MIXED):
                assert np.array_equal(out[b], expected_crop(maps, ch, side, b, k).reshape(out[b].shape)), (ch, side, b)
    with pytest.raises(ValueError):
        bk.rectify([np.zeros((21, 53), np.uint8)] * 2, [np.zeros((21, 53), np.uint8)] * 2)   # pair 1 is 50 x 19


def test_refused_arguments_leave_the_destination_untouched(hip, bank):
    bk, maps, rects = bank
    lib = hip.lib
    bk.assign(MIXED)
    src3, src1 = source_dev(3), source_dev(1)
    fill = prefill((4, B, SLOT_R, SLOT_C, 3))
    dst = torch.from_numpy(fill).cuda()
    torch.cuda.synchronize()
    s3l, s3r, s1l, s1r = src3[0].data_ptr(), src3[1].data_ptr(), src1[0].data_ptr(), src1[1].data_ptr()
    d = [dst[i].data_ptr() for i in range(4)]
    img, gray = lib.stvo_rectify_bank_images_dev, lib.stvo_rectify_bank_color_to_gray_dev
    slot1, slot3 = SLOT_R * SLOT_C, SLOT_R * SLOT_C * 3
    refused = [
        img(bk.h, 0, 1, s1l, s1r, d[0], d[1]), img(bk.h, B + 1, 1, s1l, s1r, d[0], d[1]), img(bk.h, -1, 3, s3l, s3r, d[0], d[1]),
        img(bk.h, B, 2, s1l, s1r, d[0], d[1]), img(bk.h, B, 0, s1l, s1r, d[0], d[1]), img(bk.h, B, 5, s1l, s1r, d[0], d[1]),
        img(bk.h, B, 1, None, s1r, d[0], d[1]), img(bk.h, B, 1, s1l, None, d[0], d[1]), img(bk.h, B, 1, s1l, s1r, None, d[1]),
        img(bk.h, B, 1, s1l, s1r, d[0], None), img(None, B, 1, s1l, s1r, d[0], d[1]),
        img(bk.h, B, 3, d[0], s3r, d[0], d[1]),                              # a destination that is a source
        img(bk.h, B, 3, s3l, d[1] + slot3 * (B - 1), d[0], d[1]),            # ... that shares its last slot with a source
        img(bk.h, B, 3, s3l, s3r, d[0], d[0] + slot3 * (B - 1)),             # the destinations overlap
        img(bk.h, B, 1, s1l, s1r, d[0], d[0] + slot1 * B - 1),               # ... by one byte
        gray(bk.h, 0, 3, 0, 0, s3l, s3r, d[0], d[1], None, None), gray(bk.h, B + 1, 3, 0, 0, s3l, s3r, d[0], d[1], None, None),
        gray(bk.h, B, 1, 0, 0, s3l, s3r, d[0], d[1], None, None), gray(bk.h, B, 2, 0, 0, s3l, s3r, d[0], d[1], None, None),
        gray(bk.h, B, 3, 2, 0, s3l, s3r, d[0], d[1], None, None), gray(bk.h, B, 3, -1, 0, s3l, s3r, d[0], d[1], None, None),
        gray(bk.h, B, 3, 0, 2, s3l, s3r, d[0], d[1], None, None), gray(bk.h, B, 3, 0, -1, s3l, s3r, d[0], d[1], None, None),
        gray(bk.h, B, 3, 0, 0, None, s3r, d[0], d[1], None, None), gray(bk.h, B, 3, 0, 0, s3l, None, d[0], d[1], None, None),
        gray(bk.h, B, 3, 0, 0, s3l, s3r, None, d[1], None, None), gray(bk.h, B, 3, 0, 0, s3l, s3r, d[0], None, None, None),
        gray(bk.h, B, 3, 0, 0, s3l, s3r, d[0], d[1], d[2], None), gray(bk.h, B, 3, 0, 0, s3l, s3r, d[0], d[1], None, d[3]),
        gray(bk.h, B, 3, 0, 0, d[0], s3r, d[0], d[1], None, None),                     # a plane inside a source
        gray(bk.h, B, 3, 0, 0, s3l, s3r, d[0], d[0] + slot1 * B - 1, None, None),      # planes that overlap by one byte
        gray(bk.h, B, 3, 0, 0, s3l, s3r, d[0], d[1], d[2], d[1]),                      # a swapped plane that is a grey plane
        gray(None, B, 3, 0, 0, s3l, s3r, d[0], d[1], None, None),
    ]
    hip.synchronize()
    assert refused == [INVALID] * len(refused), refused
    assert np.array_equal(dst.cpu().numpy(), fill)
    # an index out of range: refused, and the assignment in force stays in force
    for badk in (-1, K):
        a = np.array(MIXED, np.int32)
        a[3] = badk
        assert lib.stvo_rectify_bank_assign(bk.h, a.ctypes.data_as(C.c_void_p)) == INVALID
    assert lib.stvo_rectify_bank_assign(bk.h, None) == INVALID and lib.stvo_rectify_bank_assign(None, None) == INVALID
    with pytest.raises(capi.StvoError):
        bk.assign([0, 0, 0, 0, 0, 0, K])
    with pytest.raises(ValueError):
        bk.assign([0] * (B - 1))
    assert bk.calibs == MIXED
    out, fills = run(bk, B, 1)
    hip.synchronize()
    judge(out, fills, maps, MIXED, B, 1)
    # creation: a rectifier larger than the slot, none at all, a slot or a B that is nothing
    hs = (C.c_void_p * K)(*[r.h for r in rects])
    h = C.c_void_p()
    create = lib.stvo_rectify_bank_create
    assert create(hip.h, B, SLOT_C - 1, SLOT_R, hs, K, C.byref(h)) == INVALID and create(hip.h, B, SLOT_C, SLOT_R - 1, hs, K, C.byref(h)) == INVALID
    assert create(hip.h, B, SLOT_C, SLOT_R, hs, 0, C.byref(h)) == INVALID and create(hip.h, 0, SLOT_C, SLOT_R, hs, K, C.byref(h)) == INVALID
    assert create(hip.h, B, SLOT_C, SLOT_R, None, K, C.byref(h)) == INVALID and create(hip.h, B, SLOT_C, SLOT_R, hs, K, None) == INVALID
    hs_null = (C.c_void_p * 2)(rects[0].h, None)
    assert create(hip.h, B, SLOT_C, SLOT_R, hs_null, 2, C.byref(h)) == INVALID and not h.value
    rc = capi.RectCamera()
    assert lib.stvo_rectify_bank_camera(bk.h, K, C.byref(rc)) == INVALID and lib.stvo_rectify_bank_camera(bk.h, -1, C.byref(rc)) == INVALID
    assert lib.stvo_rectify_bank_camera(bk.h, 0, None) == INVALID


def test_a_slot_larger_than_every_image_and_many_pairs(hip):
    """a second shape: several quad blocks per calibration, chunks of pairs, a slot no calibration fills"""
    sizes = [(70, 33), (61, 40), (64, 16)]
    slot_c, slot_r, nb = 75, 41, 19
    rng = np.random.default_rng(3)
    maps = []
    for cols, rows in sizes:
        m1 = np.empty((2, rows, cols, 2), np.int16)
        m1[..., 0] = np.clip(np.mgrid[0:rows, 0:cols][1] + rng.integers(-4, 5, (2, rows, cols)), -3, cols + 2)
        m1[..., 1] = np.clip(np.mgrid[0:rows, 0:cols][0] + rng.integers(-4, 5, (2, rows, cols)), -3, rows + 2)
        maps.append((m1, rng.integers(0, 1024, (2, rows, cols)).astype(np.uint16)))
    rects = [capi.Rectifier(hip, nb, maps=m) for m in maps]
    bk = capi.RectifierBank(hip, nb, slot_c, slot_r, rects)
    try:
        assign = [int(v) for v in rng.integers(0, 3, nb)]
        bk.assign(assign)
        src = rng.integers(0, 256, (2, nb, slot_r, slot_c, 3), dtype=np.uint8)
        fill = prefill((2, nb, slot_r, slot_c))
        s, d = torch.from_numpy(src).cuda(), torch.from_numpy(fill).cuda()
        torch.cuda.synchronize()
        bk.rectify_color_to_gray_dev(nb, 3, s[0].data_ptr(), s[1].data_ptr(), d[0].data_ptr(), d[1].data_ptr())
        hip.synchronize()
        want = fill.copy()
        for side in range(2):
            for b, k in enumerate(assign):
                cols, rows = sizes[k]
                want[side, b, :rows, :cols] = np_color.gray(np_color.remap_color(np.ascontiguousarray(src[side, b, :rows, :cols]),
                                                                                 maps[k][0][side], maps[k][1][side]))
        assert np.array_equal(d.cpu().numpy(), want)
    finally:
        bk.close()
        for r in rects:
            r.close()
