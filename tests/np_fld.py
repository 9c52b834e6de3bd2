"""A second statement of the FLD front-end's first stage — cv::Canny as FastLineDetector calls it (aperture 3, L1 gradient,
canny_th1 == canny_th2, OpenCV 3.4's portable path) plus lineDetection's corner quirk — in vectorised numpy, one value per pixel.
It shares no code with tests/cpp/fld_ref.c: Sobel with BORDER_REPLICATE on int32 planes, m = |dx| + |dy| padded with zeros, the
three-case non-maximum suppression with TG22, the threshold m > floor(th1)."""
import math

import numpy as np

TG22 = int(0.4142135623730950488 * (1 << 15) + 0.5)


def sobel3(img):
    """int32 dx, dy of cv::Sobel(ksize 3, BORDER_REPLICATE)."""
    p = np.pad(img.astype(np.int32), 1, mode="edge")
    a, b, c = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    d, f = p[1:-1, :-2], p[1:-1, 2:]
    g, h, i = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    dx = (c + 2 * f + i) - (a + 2 * d + g)
    dy = (g + 2 * h + i) - (a + 2 * b + c)
    return dx, dy


def canny_edges(img, th1=50.0, th2=50.0):
    """uint8 [rows, cols] 0 / 255: the edge map FastLineDetector walks (corner quirk applied)."""
    assert th1 == th2, "hysteresis is not stated"
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape
    dx, dy = sobel3(img)
    m = np.abs(dx) + np.abs(dy)
    mp = np.pad(m, 1)  # magnitude outside the image: 0

    def nb(oy, ox):  # magnitude of the neighbour (y + oy, x + ox), per pixel
        return mp[1 + oy:1 + oy + rows, 1 + ox:1 + ox + cols]

    low = math.floor(th1)
    xs = np.abs(dx).astype(np.int64)
    ys = np.abs(dy).astype(np.int64) << 15
    tg22x = xs * TG22
    tg67x = tg22x + (xs << 16)
    horiz = ys < tg22x
    vert = ~horiz & (ys > tg67x)
    diag = ~horiz & ~vert
    s = np.where((dx ^ dy) < 0, -1, 1)
    ok_h = (m > nb(0, -1)) & (m >= nb(0, 1))
    ok_v = (m > nb(-1, 0)) & (m >= nb(1, 0))
    up_m = np.where(s < 0, nb(-1, 1), nb(-1, -1))   # up[j - s]
    dn_p = np.where(s < 0, nb(1, -1), nb(1, 1))     # down[j + s]
    ok_d = (m > up_m) & (m > dn_p)
    e = (m > low) & ((horiz & ok_h) | (vert & ok_v) | (diag & ok_d))
    out = np.where(e, 255, 0).astype(np.uint8)
    out[:6, :6] = 0
    out[max(rows - 5, 0):, max(cols - 5, 0):] = 0
    return out
