"""The uniform remap kernel (stvo_rectify_images_dev, stvo_rectify_color_images_dev, stvo_rectify_color_to_gray_dev) where the other
uniform tests do not reach: images narrower than a quad and smaller than one, a pixel count that is no multiple of 4 with quads that
straddle rows, a ragged last chunk of images, and sources and destinations 1, 2, 3 and 4 bytes off a 256-byte boundary (4: a 4-channel
destination is dword-aligned in every image or in none), so that the aligned-dword store and the byte store both run and both are told
apart from a store that leaves its range.  Every comparison is an
equality against the numpy statements (tests/np_rectify.py, tests/np_color.py); the bytes around every destination keep their guard
value."""
import numpy as np
import pytest
import torch

import np_color as nc
import np_rectify as nr
from stvo_amd import capi

GUARD = 0xA5
PAD = 256
OTHER = {"bgr": "rgb", "rgb": "bgr"}
OFFSETS = (1, 2, 3, 4)


def caller_maps(rows, cols):
    """Seeded maps over every border, built as test_gpu_rectify.test_random_caller_maps_every_border builds them."""
    rng = np.random.default_rng(1000 * rows + cols)
    u = rng.uniform(-2, cols + 1, (2, rows, cols))
    v = rng.uniform(-2, rows + 1, (2, rows, cols))
    iu, iv = np.floor(u * 32).astype(np.int64), np.floor(v * 32).astype(np.int64)
    m1 = np.stack([iu >> 5, iv >> 5], -1).astype(np.int16)
    m2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    # the first quad of the left side wholly inside the source (where the image has an inside), so that these few quads also reach the
    # path without tap tests; in 5 x 3 that quad straddles two rows
    if rows > 1 and cols > 1:
        flat1, flat2 = m1[0].reshape(-1, 2), m2[0].reshape(-1)
        flat1[:4] = [[k % (cols - 1), (k // 2) % (rows - 1)] for k in range(4)]
        flat2[:4] = [33 * k + 7 for k in range(4)]
    return m1, m2


def to_device(host, off):
    """host bytes in a guarded device buffer, `off` bytes past a 256-byte boundary -> (tensor, pointer)"""
    flat = torch.from_numpy(np.ascontiguousarray(host).reshape(-1))
    buf = torch.full((flat.numel() + 2 * PAD + 4,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[PAD + off:PAD + off + flat.numel()] = flat.cuda()
    return buf, buf.data_ptr() + PAD + off


def destination(nbytes, off):
    buf = torch.full((nbytes + 2 * PAD + 4,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + PAD + off


def payload(buf, nbytes, off, shape):
    """the destination's bytes, after checking that every byte before and after them kept the guard value"""
    h = buf.cpu().numpy()
    assert (h[:PAD + off] == GUARD).all() and (h[PAD + off + nbytes:] == GUARD).all(), "a store left the destination"
    return h[PAD + off:PAD + off + nbytes].reshape(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(1, 1), (2, 7), (5, 3), (3, 6)])
def test_small_images_ragged_chunks_and_unaligned_buffers(hip, rows, cols):
    m1, m2 = caller_maps(rows, cols)
    rect = capi.Rectifier(hip, 5, maps=(m1, m2))
    rng = np.random.default_rng(rows * 31 + cols)
    px = rows * cols
    try:
        for n in (1, 5):
            for ch in (1, 3, 4):
                shape = (n, rows, cols) + ((ch,) if ch > 1 else ())
                L, R = (rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(2))
                if ch == 1:
                    want = [np.stack([nr.remap(im, m1[s], m2[s]) for im in side]) for s, side in enumerate((L, R))]
                else:
                    want = [nc.remap_color(L, m1[0], m2[0]), nc.remap_color(R, m1[1], m2[1])]
                for off in OFFSETS:
                    srcs = [to_device(L, off), to_device(R, 4 - off)]
                    torch.cuda.synchronize()
                    # the remap of every channel
                    dsts = [destination(n * px * ch, off), destination(n * px * ch, (off + 1) % 3 + 1)]
                    torch.cuda.synchronize()
                    if ch == 1:
                        rect.rectify_dev(n, srcs[0][1], srcs[1][1], dsts[0][1], dsts[1][1])
                    else:
                        rect.rectify_color_dev(n, ch, srcs[0][1], srcs[1][1], dsts[0][1], dsts[1][1])
                    hip.synchronize()
                    for s, d_off in enumerate((off, (off + 1) % 3 + 1)):
                        got = payload(dsts[s][0], n * px * ch, d_off, shape)
                        assert np.array_equal(got, want[s]), (n, ch, off, s)
                    if ch == 1:
                        continue
                    # the fused colour -> grey form, with and without the swapped planes, both weight sets
                    for two in (False, True):
                        for weights in ("q14", "q15"):
                            order = "bgr" if (off + two) % 2 else "rgb"
                            offs = [off, (off + 1) % 3 + 1, (off + 2) % 3 + 1, off]
                            planes = [destination(n * px, o) for o in offs[:4 if two else 2]]
                            torch.cuda.synchronize()
                            ptrs = [p[1] for p in planes] + [None, None]
                            rect.rectify_color_to_gray_dev(n, ch, srcs[0][1], srcs[1][1], ptrs[0], ptrs[1], ptrs[2], ptrs[3], order, weights)
                            hip.synchronize()
                            for k, (buf, _) in enumerate(planes):
                                got = payload(buf, n * px, offs[k], (n, rows, cols))
                                exp = nc.gray(want[k & 1], order if k < 2 else OTHER[order], weights)
                                assert np.array_equal(got, exp), (n, ch, off, two, weights, k)
    finally:
        rect.close()


def test_the_shapes_reach_both_store_paths():
    """Of the destinations above (image i of n = 5 at off + i * px * ch): some quads start dword-aligned and lie wholly inside the
    image, some do not, for every size with a whole quad; 1 x 1 has no whole quad at all, and 3 x 6 has quads across two rows and a
    last quad of 2 pixels."""
    for rows, cols in ((2, 7), (5, 3), (3, 6)):
        px = rows * cols
        for ch in (1, 3, 4):
            aligned = {(off + (i * px + q * 4) * ch) % 4 == 0 for off in OFFSETS for i in range(5) for q in range(px // 4)}
            assert aligned == {False, True}, (rows, cols, ch)
    assert 1 * 1 < 4 and (3 * 6) % 4 == 2 and 6 % 4 != 0 and 3 < 4 < 7
