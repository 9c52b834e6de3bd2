"""The scaled image of the LSD detector for every blur radius, stated in numpy, and the detector composed from it.

oracle/stvo_lsd_oracle.c:82-109 states cv::GaussianBlur on 8-bit data as OpenCV 3.x's separable fixed-point filter for the 7 x 7
kernel only (and refuses every other).  This module states the same filter with 7 replaced by n = 1 + 2h and 3 by h, defining
nothing new:

  weights     k_i = exp(-(i - h)^2 / (2 sigma^2)), sum accumulated in index order in double, w_i = lrint((float)(k_i / sum) * 256.0);
              h = 0: the single weight 256 (the identity; sigma may then be 0 and there is no Gaussian to evaluate)
  horizontal  integer sums under BORDER_REFLECT_101, the reflection repeated while the index is still outside
  vertical    integer sums, then (s + 2^15) >> 16, clamped to 0 .. 255: bytes, BEFORE the resize reads them

The composed detector: blur -> oracle.resize_linear_fxy(blurred, scale, scale) -> oracle.lsd_segments(scaled, scale = 1) -> coordinates
divided by scale.  The oracle at scale 1 returns float(x + 0.5), the detector float((x + 0.5) / scale): for a power-of-two scale the
division is exact and the composition bit-exact, otherwise the two differ by at most 2^-23 relative (one float rounding of the operand,
one of the result — derived, not measured).
"""
import math

import numpy as np

REL_BOUND = 2.0 ** -23

# (scale, sigma_scale, radius) of the pairs the tests run; (1.5, 0.0) is the only way to radius 0
PAIRS = [(1.5, 0.0, 0), (1.2, 0.26, 1), (1.2, 0.3, 2), (0.65, 0.6, 4), (0.5, 0.6, 5), (0.4, 0.6, 6), (0.5, 1.0, 8), (0.25, 0.6, 9),
         (0.22, 0.8, 14), (0.25, 1.0, 15)]


def sigma_radius(scale, sigma_scale):
    sigma = sigma_scale / scale if scale < 1 else sigma_scale
    return sigma, int(math.ceil(sigma * math.sqrt(2 * 3.0 * math.log(10.0))))


def weights(scale, sigma_scale):
    """(sigma, h, int32 [1 + 2h]) of a pair."""
    sigma, h = sigma_radius(scale, sigma_scale)
    if h == 0:
        return sigma, 0, np.array([256], np.int32)
    k = [math.exp(-float(i - h) * float(i - h) / (2.0 * sigma * sigma)) for i in range(1 + 2 * h)]
    s = 0.0
    for v in k:
        s += v
    return sigma, h, np.array([int(np.rint(float(np.float32(v / s)) * 256.0)) for v in k], np.int32)


def reflect101(p, n):
    while p < 0 or p >= n:
        if p < 0:
            p = -p
        if p >= n:
            p = 2 * n - 2 - p
    return p


def blur(img, w):
    """The fixed-point separable filter with the integer weights w on a uint8 image."""
    img = np.asarray(img, np.uint8).astype(np.int64)
    rows, cols = img.shape
    h = (len(w) - 1) // 2
    cx = np.array([[reflect101(x + i - h, cols) for x in range(cols)] for i in range(len(w))])
    cy = np.array([[reflect101(y + i - h, rows) for y in range(rows)] for i in range(len(w))])
    tmp = np.zeros((rows, cols), np.int64)
    for i, wi in enumerate(w):
        tmp += int(wi) * img[:, cx[i]]
    s = np.zeros((rows, cols), np.int64)
    for i, wi in enumerate(w):
        s += int(wi) * tmp[cy[i], :]
    return np.clip((s + (1 << 15)) >> 16, 0, 255).astype(np.uint8)


def scaled_image(oracle, img, scale, sigma_scale):
    if scale == 1:
        return np.asarray(img, np.uint8).copy()
    return oracle.resize_linear_fxy(blur(img, weights(scale, sigma_scale)[2]), scale, scale)


def segments(oracle, img, scale, sigma_scale, **opts):
    """The composed detector: float32 [n, 4] in detection order, in the coordinates of img."""
    seg = oracle.lsd_segments(scaled_image(oracle, img, scale, sigma_scale), oracle.lsd_opts(scale=1.0, **opts))
    return (seg.astype(np.float64) / scale).astype(np.float32)


def same_segments(got, want, scale):
    """Count and order, and the coordinates bit for bit at a power-of-two scale, within 2^-23 relative otherwise."""
    assert got.shape == want.shape, (got.shape, want.shape)
    if math.frexp(scale)[0] == 0.5:
        assert np.array_equal(got, want)
    else:
        g, w = got.astype(np.float64), want.astype(np.float64)
        assert np.all(np.abs(g - w) <= REL_BOUND * np.abs(w))


KEYLINE_DT = np.dtype([("sx", "<f4"), ("sy", "<f4"), ("ex", "<f4"), ("ey", "<f4"), ("length", "<f4"), ("response", "<f4"),
                       ("angle", "<f4"), ("num_pixels", "<i4")])


def keylines(oracle, seg, cols, rows, min_length, nfeatures):
    """The wrapper (LSDDetectorC::detectImpl for one octave + the top-N cut, as oracle/stvo_lsd_oracle.c: orc_lsd_detect restates it)
    applied to given segments: checkLineExtremes, length, min_length, numOfPixels, response, a stable top-N by response."""
    out = []
    f32 = np.float32
    for s in np.asarray(seg, np.float32):
        e = [f32(v) for v in s]
        for i, lim in ((0, cols), (2, cols), (1, rows), (3, rows)):
            if e[i] < 0:
                e[i] = f32(0)
            if e[i] >= lim:
                e[i] = f32(lim) - f32(1)
        d0, d1 = float(f32(e[0] - e[2])), float(f32(e[1] - e[3]))
        length = f32(math.sqrt(d0 * d0 + d1 * d1))
        if not float(length) > min_length:
            continue
        ang = f32(math.atan2(float(f32(e[3] - e[1])), float(f32(e[2] - e[0]))))
        out.append((e[0], e[1], e[2], e[3], length, length / f32(max(cols, rows)), ang,
                    oracle.line_iterator_count(cols, rows, e[0], e[1], e[2], e[3])))
    kl = np.array(out, KEYLINE_DT) if out else np.zeros(0, KEYLINE_DT)
    if nfeatures != 0 and len(kl) > nfeatures:
        kl = kl[np.argsort(-kl["response"], kind="stable")[:nfeatures]]
    return kl


def check_keylines(got, ref):
    """(records, responses) of capi.Lsd.detect against a KEYLINE_DT array, field by field as tests/test_gpu_lsd.py does."""
    rec, resp = got
    assert len(rec) == len(ref)
    for f in ("sx", "sy", "ex", "ey"):
        assert np.array_equal(rec[f], ref[f]), f
    assert np.array_equal(rec["num_pixels"], ref["num_pixels"])
    assert np.array_equal(resp, ref["response"])
    # KeyLine::angle = atan2 in double, rounded to float: the device's atan2 and the host's may differ in the last place
    assert np.allclose(rec["angle"], ref["angle"], rtol=0, atol=4e-7)
