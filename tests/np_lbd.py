"""A plain numpy statement of BinaryDescriptor::compute for key-lines that already exist, on octave 0 — the second witness for the LBD
kernels (csrc/lbd_kernels.hip) beside oracle/stvo_lbd_oracle.c.  Written from the reference-held source, not from the oracle or the
kernel; the lines cited are those of 3rdparty/line_descriptor/src/binary_descriptor_custom.cpp:
    the two weight tables of the constructor, integer divisions included        :217-258
    computeGaussianPyramid / computeSobel (GaussianBlur 5 x 5 sigma 1, Sobel 3 x 3 to int16)   :350-398
    binaryConversion                                                             :401-412
    computeImpl (octave 0: 32 bytes from the 32 band pairs of `combinations`, :74-108)          :539-687
    computeLBD                                                                   :1026-1340
cv::GaussianBlur on 8-bit data is OpenCV 3's fixed-point separable filter as the project states it everywhere (weights x 2^8 rounded,
both passes in integers, one rounding shift by 16, BORDER_REFLECT_101); cv::Sobel(ksize 3, CV_16S) is exact integer arithmetic.

One body, describe(), with a dtype parameter:
  float32     every operation of the source in the source's order, one rounding per operation (numpy contracts nothing), vectorised over
              the key-lines and the 63 rows of the support region, with python loops over the walk along the line and over the rows of the
              band sums, so that every sum keeps its order.  Bit for bit the descriptor of the oracle and of the kernels.
  longdouble  the sample positions and every decision stay in the source's types (float positions, `gDL > 0` on the float projection, the
              double `> 0.4` on the float component: they are taken from the float32 run); the VALUES — cos / sin, the weights, the
              projections, every sum, the square roots and the normalisations — are extended.  A variance that the extended arithmetic
              leaves below zero is taken as zero (in exact arithmetic it is never negative).  compute() reports per key-line how far the
              float descriptor is from this one.
cos / sin of the FLOAT direction are the double functions of the host's C library rounded to float, as oracle/stvo_lbd_oracle.c defines
them (the source calls the float overloads, :1130-1131).

Mutation switches (`mutate`, test-only): each turns one rule into its near miss; tests/test_lbd_statement_host.py shows that the
planned key-lines of tests/lbd_edge_cases.py tell every one of them from the rule."""
import math

import numpy as np

F32 = np.float32
BANDS, WBAND, ROWS, DESC = 9, 7, 63, 72          # NUM_OF_BANDS, widthOfBand_ (:109-114), heightOfLSP, descriptor_size

MUTATIONS = ("round_half_even",       # rint in place of round (half away from zero)
             "clamp_cols",            # the clamp ends at cols, not cols - 1
             "clamp_slot",            # under a size table: the clamp ends at the slot's last column / row, not the image's
             "swap_neighbour_weights",  # gaussCoefL_[r] and gaussCoefL_[r + 2 w] exchanged
             "invn3_outer",           # the outer bands divided by 3 w like the inner ones
             "clip_ge",               # >= in the 0.4 clip
             "binary_ge",             # >= in the binary conversion
             "bit_reverse",           # component i sets bit 7 - i
             "pairs_all",             # the pair rule without its omission
             "no_short_cast",         # numOfPixels as an int
             "steps_minus_1")         # the walk one step short


def pairs(omit=True):
    """The 32 band pairs as a rule: all (i, j), i < j, in lexicographic order, without (0, 7), (0, 8), (1, 7), (1, 8)."""
    p = [(i, j) for i in range(BANDS) for j in range(i + 1, BANDS) if not (omit and i < 2 and j > 6)]
    return p[:32]


def gaussian_blur5(img):
    """cv::GaussianBlur(img, img, Size(5, 5), 1) on 8-bit data (:358)"""
    img = np.asarray(img, np.uint8)
    k = np.array([math.exp(-(i - 2) ** 2 / 2.0) for i in range(5)])
    ki = np.rint((k / k.sum()).astype(F32).astype(np.float64) * 256.0).astype(np.int64)
    rows, cols = img.shape
    p = np.pad(img.astype(np.int64), ((0, 0), (2, 2)), mode="reflect")               # BORDER_REFLECT_101
    h = sum(ki[i] * p[:, i:i + cols] for i in range(5))
    p = np.pad(h, ((2, 2), (0, 0)), mode="reflect")
    v = sum(ki[i] * p[i:i + rows, :] for i in range(5))
    return np.clip((v + (1 << 15)) >> 16, 0, 255).astype(np.uint8)


def sobel3(img):
    """cv::Sobel(img, dx, CV_16SC1, 1, 0, 3), cv::Sobel(img, dy, CV_16SC1, 0, 1, 3) (:395-396)"""
    rows, cols = img.shape
    p = np.pad(np.asarray(img, np.int64), 1, mode="reflect")
    win = lambda dy, dx: p[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols]
    dx = (win(-1, 1) + 2 * win(0, 1) + win(1, 1)) - (win(-1, -1) + 2 * win(0, -1) + win(1, -1))
    dy = (win(1, -1) + 2 * win(1, 0) + win(1, 1)) - (win(-1, -1) + 2 * win(-1, 0) + win(-1, 1))
    return dx.astype(np.int16), dy.astype(np.int16)


def tables(V=np.float64):
    """gaussCoefL_[3 w], gaussCoefG_[9 w] (:228-258).  float64: as the source keeps them; longdouble: the same Gaussians, extended."""
    w = WBAND
    if V is np.longdouble:
        ex = lambda a: np.exp(np.longdouble(a))
    else:
        ex = lambda a: math.exp(a)
    u = float((w * 3 - 1) // 2)            # :231, an integer division: 10
    sigma = float((w * 2 + 1) // 2)        # :234, an integer division: 7
    inv = V(-1) / (V(2) * V(sigma) * V(sigma))
    L = np.array([ex((i - u) * (i - u) * inv) for i in range(3 * w)], V)
    u = float((BANDS * w - 1) // 2)        # :249: 31
    inv = V(-1) / (V(2) * V(u) * V(u))     # sigma = u (:252)
    G = np.array([ex((i - u) * (i - u) * inv) for i in range(BANDS * w)], V)
    return L, G


def cos_sin(angle):
    """(float) cos((double) direction), (float) sin((double) direction) of float32 angles, from the host's C library"""
    a = np.asarray(angle, F32)
    return (np.array([math.cos(float(x)) for x in a]).astype(F32), np.array([math.sin(float(x)) for x in a]).astype(F32))


def round_away(x):
    """round() of a float: half away from zero, computed in float64 (floor(|x| + 0.5) in float32 is wrong for 0.49999997)"""
    x = x.astype(np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def gradients(img, size=None):
    """(dx, dy) int16 of the image a key-line is described on: the whole array, or its top-left size = (cols, rows) inside a slot.
    -> dx, dy [slot rows, slot cols], cols, rows.  Outside a crop the arrays hold the slot's own gradients: only a clamp that forgets the
    size table reads them."""
    img = np.asarray(img, np.uint8)
    dx, dy = sobel3(gaussian_blur5(img))
    if size is None:
        return dx, dy, img.shape[1], img.shape[0]
    cols, rows = size
    cx, cy = sobel3(gaussian_blur5(img[:rows, :cols]))
    dx[:rows, :cols] = cx
    dy[:rows, :cols] = cy
    return dx, dy, cols, rows


def describe(V, dx, dy, cols, rows, lines, num_pixels, mutate=(), decisions=None):
    """computeLBD (:1095-1340) and binaryConversion for n key-lines.  V: float32 or longdouble (the module's docstring); decisions: the
    clip mask of the float32 run, for the longdouble run.  -> dict(value [n, 72] in V, desc [n, 32], clip [n, 72], trace: list of dicts)"""
    mut = set(mutate)
    assert mut <= set(MUTATIONS), mut - set(MUTATIONS)
    ext = V is not F32
    lines = np.asarray(lines, F32).reshape(-1, 5)
    n = len(lines)
    npx = np.asarray(num_pixels, np.int64).reshape(n)
    pitch = dx.shape[1]                                                       # realWidth: the pitch of the gradient rows
    fdx, fdy = dx.reshape(-1), dy.reshape(-1)
    image_w, image_h = cols - 1, rows - 1                                     # :1102-1103
    if "clamp_cols" in mut:
        image_w = cols
    if "clamp_slot" in mut:
        image_w, image_h = dx.shape[1] - 1, dx.shape[0] - 1
    half_h = (ROWS - 1) // 2
    length = npx if "no_short_cast" in mut else npx.astype(np.int16).astype(np.int64)   # (short) numOfPixels, :1117
    half_w = np.trunc((length - 1) / 2).astype(np.int64)                      # C's division truncates: (0 - 1) / 2 = 0
    steps = length - 1 if "steps_minus_1" in mut else length
    mid_x = (0.5 * (lines[:, 0] + lines[:, 2]).astype(np.float64)).astype(F32)   # :1121-1122 (the sum is a float sum)
    mid_y = (0.5 * (lines[:, 1] + lines[:, 3]).astype(np.float64)).astype(F32)
    dL0, dL1 = cos_sin(lines[:, 4])                                           # :1130-1131
    if ext:
        a = lines[:, 4].astype(V)
        v0, v1 = np.cos(a), np.sin(a)
    else:
        v0, v1 = dL0, dL1
    o0, o1 = -v1, v0                                                          # dO (:1134-1135)
    f_o0, f_o1 = -dL1, dL0
    x0 = -dL0 * half_w.astype(F32) + dL1 * F32(half_h) + mid_x                # :1138-1139
    y0 = -dL1 * half_w.astype(F32) - dL0 * F32(half_h) + mid_y
    X = np.empty((n, ROWS), F32); Y = np.empty((n, ROWS), F32)
    for h in range(ROWS):                                                     # the origin steps once per row (:1186-1187)
        X[:, h] = x0; Y[:, h] = y0
        x0 = x0 - dL1
        y0 = y0 + dL0
    tr = {k: np.zeros(n, np.int64) for k in ("clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "tie_x", "tie_y", "x_last", "x_cols",
                                             "x_m1", "y_last", "y_rows", "y_m1", "pp", "pn", "np", "nn", "w_neg_zero", "w_zero_neg", "w_m1_m1",
                                             "max_abs_g", "out_of_domain")}
    pL = np.zeros((n, ROWS), V); nL = np.zeros((n, ROWS), V); pO = np.zeros((n, ROWS), V); nO = np.zeros((n, ROWS), V)
    c0, c1, d0, d1 = dL0[:, None], dL1[:, None], f_o0[:, None], f_o1[:, None]
    e0, e1, g0, g1 = v0[:, None], v1[:, None], o0[:, None], o1[:, None]
    rnd = (lambda v: np.rint(v.astype(np.float64)).astype(np.int64)) if "round_half_even" in mut else round_away
    for w in range(int(max(steps.max(), 0)) if n else 0):                     # :1153-1185
        act = (w < steps)[:, None]
        cnt = lambda m: (m & act).sum(axis=1)
        tx, ty = rnd(X), rnd(Y)
        tr["out_of_domain"] += cnt((np.abs(tx) > 32767) | (np.abs(ty) > 32767))
        tr["tie_x"] += cnt(np.abs(X.astype(np.float64) - np.trunc(X.astype(np.float64))) == 0.5)
        tr["tie_y"] += cnt(np.abs(Y.astype(np.float64) - np.trunc(Y.astype(np.float64))) == 0.5)
        tr["clamp_left"] += cnt(tx < 0); tr["clamp_right"] += cnt(tx > image_w)
        tr["clamp_top"] += cnt(ty < 0); tr["clamp_bottom"] += cnt(ty > image_h)
        tr["x_last"] += cnt(tx == cols - 1); tr["x_cols"] += cnt(tx == cols); tr["x_m1"] += cnt(tx == -1)
        tr["y_last"] += cnt(ty == rows - 1); tr["y_rows"] += cnt(ty == rows); tr["y_m1"] += cnt(ty == -1)
        xc = np.clip(tx, 0, image_w); yc = np.clip(ty, 0, image_h)            # :1156, :1158
        at = np.minimum(yc * pitch + xc, fdx.size - 1)                        # (the minimum matters under clamp_cols only)
        sdx, sdy = fdx[at], fdy[at]                                           # :1162-1163
        tr["pp"] += cnt((sdx > 0) & (sdy > 0)); tr["pn"] += cnt((sdx > 0) & (sdy < 0))
        tr["np"] += cnt((sdx < 0) & (sdy > 0)); tr["nn"] += cnt((sdx < 0) & (sdy < 0))
        # the packed (dx, dy) word's sign-extension corners.  dx and dy of a 3 x 3 Sobel have one parity (both are the four corner pixels modulo 2),
        # so (-1, 0) and (0, -1) do not exist: the nearest words that do are a negative half beside a zero half, and both halves -1
        tr["w_neg_zero"] += cnt((sdx < 0) & (sdy == 0)); tr["w_zero_neg"] += cnt((sdx == 0) & (sdy < 0)); tr["w_m1_m1"] += cnt((sdx == -1) & (sdy == -1))
        tr["max_abs_g"] = np.maximum(tr["max_abs_g"], np.where(act, np.maximum(np.abs(sdx), np.abs(sdy)), 0).max(axis=1))
        fx, fy = sdx.astype(F32), sdy.astype(F32)
        gDL = fx * c0 + fy * c1                                               # :1164-1165, in float: the decisions
        gDO = fx * d0 + fy * d1
        if ext:
            ex_, ey_ = sdx.astype(V), sdy.astype(V)
            vDL = ex_ * e0 + ey_ * e1
            vDO = ex_ * g0 + ey_ * g1
        else:
            vDL, vDO = gDL, gDO
        pos = gDL > 0                                                         # :1166-1181
        pL = np.where(act & pos, pL + vDL, pL); nL = np.where(act & ~pos, nL - vDL, nL)
        pos = gDO > 0
        pO = np.where(act & pos, pO + vDO, pO); nO = np.where(act & ~pos, nO - vDO, nO)
        X = np.where(act, X + c0, X)                                          # :1182-1183
        Y = np.where(act, Y + c1, Y)
    coefL, coefG = tables(V if ext else np.float64)
    if not ext:
        coefL, coefG = coefL.astype(F32), coefG.astype(F32)                   # (float) gaussCoefG_[hID] (:1188), (float) gaussCoefL_[..]
    band = np.zeros((8, n, BANDS), V)
    with np.errstate(all="ignore"):
        for h in range(ROWS):                                                 # :1188-1240
            c = coefG[h]
            r = [c * pL[:, h], c * nL[:, h], None, None, c * pO[:, h], c * nO[:, h], None, None]
            r[2] = r[0] * r[0]; r[3] = r[1] * r[1]; r[6] = r[4] * r[4]; r[7] = r[5] * r[5]
            b, k = h // WBAND, h % WBAND
            up, down = k + 2 * WBAND, k
            if "swap_neighbour_weights" in mut:
                up, down = down, up
            for bd, kk in ((b, k + WBAND), (b - 1, up), (b + 1, down)):      # own band, the band above, the band below
                if bd < 0 or bd >= BANDS:
                    continue
                c = coefL[kk]
                for q in range(8):
                    band[q][:, bd] = band[q][:, bd] + (c * r[q] if q in (0, 1, 4, 5) else c * c * r[q])
        # :1253-1280 — mean and standard deviation per band
        inv2, inv3 = (V(1) / (V(WBAND) * V(2)), V(1) / (V(WBAND) * V(3))) if ext else (F32(1.0 / (WBAND * 2.0)), F32(1.0 / (WBAND * 3.0)))
        des = np.zeros((n, DESC), V)
        for bd in range(BANDS):
            inv = inv2 if (bd in (0, BANDS - 1) and "invn3_outer" not in mut) else inv3
            for mean_at, q1, q2 in ((0, 0, 2), (1, 1, 3), (2, 4, 6), (3, 5, 7)):
                t = band[q1][:, bd] * inv
                var = band[q2][:, bd] * inv - t * t
                if ext:
                    var = np.maximum(var, 0)
                des[:, 8 * bd + mean_at] = t
                des[:, 8 * bd + mean_at + 4] = np.sqrt(var)
        # :1283-1315 — means and standard deviations normalised apart
        tM = np.zeros(n, V); tS = np.zeros(n, V)
        for bd in range(BANDS):
            for i in range(4):
                tM = tM + des[:, 8 * bd + i] * des[:, 8 * bd + i]
            for i in range(4, 8):
                tS = tS + des[:, 8 * bd + i] * des[:, 8 * bd + i]
        tM = V(1) / np.sqrt(tM); tS = V(1) / np.sqrt(tS)
        for bd in range(BANDS):
            des[:, 8 * bd:8 * bd + 4] = des[:, 8 * bd:8 * bd + 4] * tM[:, None]
            des[:, 8 * bd + 4:8 * bd + 8] = des[:, 8 * bd + 4:8 * bd + 8] * tS[:, None]
        # :1322-1341 — the clip, decided in double on the float component, and the second normalisation
        if decisions is None:
            d64 = des.astype(np.float64)
            clip = (d64 >= 0.4) if "clip_ge" in mut else (d64 > 0.4)
        else:
            clip = decisions
        des = np.where(clip, V(0.4) if not ext else np.longdouble(4) / np.longdouble(10), des)
        t = np.zeros(n, V)
        for i in range(DESC):
            t = t + des[:, i] * des[:, i]
        t = V(1) / np.sqrt(t)
        des = des * t[:, None]
    # computeImpl :655-659 + binaryConversion :401-412
    pr = pairs(omit="pairs_all" not in mut)
    f1 = np.stack([des[:, 8 * i:8 * i + 8] for i, _ in pr], 1)                # [n, 32, 8]
    f2 = np.stack([des[:, 8 * j:8 * j + 8] for _, j in pr], 1)
    with np.errstate(invalid="ignore"):
        bits = (f1 >= f2) if "binary_ge" in mut else (f1 > f2)
        equal = (f1 == f2).sum(axis=(1, 2))
        margin = np.abs(f1 - f2)
    weight = 1 << (7 - np.arange(8) if "bit_reverse" in mut else np.arange(8))
    desc = (bits * weight).sum(axis=2).astype(np.uint8)
    nan = np.isnan(des).any(axis=1)
    trace = []
    for l in range(n):
        t = {k: int(v[l]) for k, v in tr.items()}
        t.update(length=int(length[l]), clipped=int(clip[l].sum()), nan=bool(nan[l]), equal_cmp=int(equal[l]),
                 nan_cmp=int(np.isnan(margin[l]).sum()))
        trace.append(t)
    return dict(value=des, desc=desc, clip=clip, trace=trace, margin=margin, bits=bits)


def compute(img, lines, num_pixels, dtype=np.float32, size=None, mutate=()):
    """BinaryDescriptor::compute for the octave-0 key-lines of one image.  img uint8 [rows, cols]; size = (cols, rows): the image is the
    top-left crop of img, a slot whose pitch the gradient rows keep (stvo_lbd_set_image_sizes); lines [n, 5] float32 (sPointInOctaveX,
    sPointInOctaveY, ePointInOctaveX, ePointInOctaveY, direction); num_pixels [n] (KeyLine::numOfPixels).
    dtype float32 -> dict(desc [n, 32] uint8, desc_f [n, 72] float32, trace)
    dtype longdouble -> the same keys from the extended values, and value [n, 72] longdouble, deviation [n] (max |float - extended| over
    the line's 72 components, NaN for a line whose float descriptor has a NaN), margin [n, 32, 8] (|f1 - f2| of every compared pair),
    bits [n, 32, 8]."""
    dx, dy, cols, rows = gradients(img, size)
    f = describe(F32, dx, dy, cols, rows, lines, num_pixels, mutate)
    if dtype in (np.float32, "float32"):
        return dict(desc=f["desc"], desc_f=f["value"], trace=f["trace"])
    assert dtype in (np.longdouble, "longdouble"), dtype
    e = describe(np.longdouble, dx, dy, cols, rows, lines, num_pixels, mutate, decisions=f["clip"])
    with np.errstate(invalid="ignore"):
        dev = np.abs(f["value"].astype(np.longdouble) - e["value"]).max(axis=1) if len(f["value"]) else np.zeros(0, np.longdouble)
    return dict(desc=e["desc"], desc_f=f["value"], value=e["value"], deviation=dev, margin=e["margin"], bits=e["bits"], trace=f["trace"],
                desc_float32=f["desc"])
