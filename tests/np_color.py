"""Plain statement of what the colour entry points compute (stvo_color_to_gray*, stvo_rectify_color_*): cvtColor's 8-bit integer
grey conversion in its two published weight sets, and cv::remap of an interleaved colour image, which is np_rectify.remap on every
channel with the rounding per channel (the alpha channel is a channel like the others)."""
import numpy as np

import np_rectify

# (blue, green, red, shift): the table form of OpenCV 3.0 - 3.4.1 (R2Y 4899, G2Y 9617, B2Y 1868, yuv_shift 14) and the 15-bit
# weights of the later releases
WEIGHTS = {"q14": (1868, 9617, 4899, 14), "q15": (3735, 19235, 9798, 15)}


def gray(img, order="bgr", weights="q14"):
    """img uint8 [..., ch] with ch = 3 or 4 (a fourth channel is ignored) -> uint8 [...].  order "bgr": channel 0 is blue
    (COLOR_BGR2GRAY); "rgb": channel 0 is red (CV_RGB2GRAY on the same bytes)."""
    img = np.asarray(img, np.uint8)
    if img.shape[-1] not in (3, 4):
        raise ValueError("gray: 3 or 4 interleaved channels")
    if order not in ("bgr", "rgb"):
        raise ValueError("gray: order is 'bgr' or 'rgb'")
    wb, wg, wr, shift = WEIGHTS[weights]
    c0, c1, c2 = (img[..., k].astype(np.int64) for k in range(3))
    blue, red = (c0, c2) if order == "bgr" else (c2, c0)
    return ((wb * blue + wg * c1 + wr * red + (1 << (shift - 1))) >> shift).astype(np.uint8)


def remap_color(img, map1, map2):
    """cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) of uint8 [rows, cols, ch] (or [n, rows, cols, ch]) with CV_16SC2 maps."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 4:
        return np.stack([remap_color(im, map1, map2) for im in img])
    return np.stack([np_rectify.remap(np.ascontiguousarray(img[..., c]), map1, map2) for c in range(img.shape[-1])], -1)
