"""The LDS geometry of the fused blur + resize of the LSD detector (stvo-pl_amd/csrc/lsd_scale_plan.h), run on the host through
tests/cpp/lsd_scale_plan_host.cpp, against a restatement in Python of the host plan and of the kernel's per-tile arithmetic (the taps in
float32 as lsd_scale_kernels.hip: resize_taps forms them).

What stvo_lsd_set_image_sizes rests on at a blur radius other than 3: the MIXED instance of lsd_blur_resize_kernel runs every image of
a batch under the SLOT's plan (tile and dynamic LDS), so every tile of every image that fits the slot must need no more LDS than the
slot's plan provides — the kernel leaves a tile that does not fit unwritten.  Checked here for four slots, the ten (scale, sigma_scale)
pairs of tests/lsd_scale_statement.py and 44 crops per slot (the slot itself, 8 x 8, slot_w x 8, 8 x slot_h among them).  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lsd_scale_statement as st

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "lsd_scale_plan_host.cpp")
HDRS = [os.path.join(ROOT, "stvo-pl_amd", "csrc", "lsd_scale_plan.h")]
i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")

SLOTS = [(200, 136), (1242, 376), (97, 61), (53, 21)]
BUDGET = 64 * 1024


@pytest.fixture(scope="module")
def lph():
    so = os.path.join(HERE, "cpp", "liblsd_scale_plan_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        tmp = "%s.%d.so" % (so[:-3], os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SRC])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.lph_plan.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, i32p]
    lib.lph_layout.argtypes = [C.c_int] * 7 + [i32p]; lib.lph_layout.restype = C.c_longlong
    lib.lph_tile.argtypes = [C.c_int] * 9 + [i32p]; lib.lph_tile.restype = C.c_longlong
    lib.lph_max_tile_bytes.argtypes = [C.c_int, i32p, C.c_int, i32p, C.c_int, C.c_int, C.c_int]; lib.lph_max_tile_bytes.restype = C.c_longlong
    return lib


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def layout(nx, ny, ncp, nr, hk, tw, th):
    """br_layout: (sr, scp, ncp, bytes)"""
    sr = ny + 2 * hk
    scp = (4 * ((nx + 3) // 4) + 2 * hk + 4) & ~3
    return sr, scp, ncp, 4 * sr * ncp + 16 * (tw + th) + sr * scp + ((nr * ncp + 3) & ~3)


def plan(cols, rows, scale, hk):
    """plan_blur_resize_u8: (tw_log, th_log, lds_bytes) or None"""
    step = 1.0 / scale
    twl, thl = 6, 4
    while True:
        tw, th = 1 << twl, 1 << thl
        nx = int(min(math.ceil((tw - 1) * step) + 4, cols))
        ny = int(min(math.ceil((th - 1) * step) + 4, rows))
        ncp = min(4 * ((nx + 3) // 4), max(2 * tw, 4))
        nr = min(ny, 2 * th)
        b = layout(nx, ny, ncp, nr, hk, tw, th)[3]
        if b <= BUDGET:
            return twl, thl, b
        if twl == 0 and thl == 0:
            return None
        if twl >= thl:
            twl -= 1
        else:
            thl -= 1


def taps(d, step, n, x_axis):
    """resize_taps: the two source indices of destination index d (the position in double, rounded to float32, then floor)"""
    s = int(math.floor(float(np.float32((d + 0.5) * step - 0.5))))
    if x_axis:
        s = 0 if s < 0 else s
        s = n - 1 if s >= n - 1 else s
    return min(max(s, 0), n - 1), min(max(s + 1, 0), n - 1)


def tile(cmin, cmax, rmin, rmax, ntw, nth, hk, tw, th):
    """the kernel's layout of one tile: (nx, xlist, ylist, nr, sr, scp, ncp, bytes)"""
    nx, ny = cmax - cmin + 1, rmax - rmin + 1
    xlist, ylist = nx > 2 * ntw, ny > 2 * nth
    nr = 2 * nth if ylist else ny
    sr, scp, ncp, b = layout(nx, ny, 4 * (((2 * ntw if xlist else nx) + 3) // 4), nr, hk, tw, th)
    return nx, int(xlist), int(ylist), nr, sr, scp, ncp, b


def scaled(n, scale):
    return int(np.rint(n * scale))   # cvRound: half to even


def axis_tiles(n_src, n_dst, step, t_log, x_axis):
    """per tile of one axis under tile size 1 << t_log: (first tap, last tap, outputs)"""
    t = 1 << t_log
    out = []
    for d0 in range(0, n_dst, t):
        nt = min(t, n_dst - d0)
        out.append((taps(d0, step, n_src, x_axis)[0], taps(d0 + nt - 1, step, n_src, x_axis)[1], nt))
    return out


def crops(slot):
    """44 sizes that fit the slot: the slot, the three thin corners, one less than the slot, then a seeded spread"""
    w, h = slot
    out = [(w, h), (8, 8), (w, 8), (8, h), (w - 1, h - 1), (w, h - 1), (w - 1, h), (9, 9)]
    rng = np.random.default_rng(w * 1000 + h)
    while len(out) < 44:
        c = (int(rng.integers(8, w + 1)), int(rng.integers(8, h + 1)))
        if c not in out:
            out.append(c)
    return out


# ---- the header against it ------------------------------------------------------------------------------------------------------------

def header_plan(lph, cols, rows, scale, hk):
    out = np.zeros(3, np.int32)
    return tuple(int(v) for v in out) if lph.lph_plan(cols, rows, scale, hk, out) else None


def test_budget(lph):
    assert lph.lph_budget() == BUDGET


@pytest.mark.parametrize("slot", SLOTS, ids=["%dx%d" % s for s in SLOTS])
def test_plan_and_layout_against_the_restatement(lph, slot):
    for scale, sigma_scale, hk in st.PAIRS:
        assert st.sigma_radius(scale, sigma_scale)[1] == hk
        for cols, rows in [slot] + crops(slot)[:8]:
            p = header_plan(lph, cols, rows, scale, hk)
            assert p == plan(cols, rows, scale, hk) and p is not None and p[2] <= BUDGET, (cols, rows, scale)
        rng = np.random.default_rng(hk)
        out = np.zeros(3, np.int32)
        for _ in range(50):
            nx, ny, tw, th = (int(v) for v in rng.integers(1, 300, 4))
            ncp, nr = 4 * int(rng.integers(1, 80)), int(rng.integers(1, 2 * th + 1))
            b = lph.lph_layout(nx, ny, ncp, nr, hk, tw, th, out)
            assert tuple(int(v) for v in out) + (b,) == layout(nx, ny, ncp, nr, hk, tw, th)


def test_tile_layout_against_the_restatement(lph):
    rng = np.random.default_rng(5)
    out = np.zeros(7, np.int32)
    seen = set()
    for _ in range(2000):
        cmin, rmin = int(rng.integers(0, 500)), int(rng.integers(0, 500))
        ntw, nth = int(rng.integers(1, 65)), int(rng.integers(1, 17))
        cmax, rmax = cmin + int(rng.integers(0, 5 * ntw)), rmin + int(rng.integers(0, 5 * nth))
        hk = int(rng.integers(0, 16))
        b = lph.lph_tile(cmin, cmax, rmin, rmax, ntw, nth, hk, 64, 16, out)
        want = tile(cmin, cmax, rmin, rmax, ntw, nth, hk, 64, 16)
        assert tuple(int(v) for v in out) + (b,) == want
        seen.add((want[1], want[2]))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}   # runs and pairs on both axes


@pytest.mark.parametrize("slot", SLOTS, ids=["%dx%d" % s for s in SLOTS])
def test_every_tile_of_every_crop_fits_the_slots_lds(lph, slot):
    """the bound the MIXED instance of the kernel runs under"""
    sizes = crops(slot)
    assert len(sizes) == 44 and len(set(sizes)) == 44 and all(8 <= c <= slot[0] and 8 <= r <= slot[1] for c, r in sizes)
    if slot == (1242, 376):
        sizes = sizes + [(1241, 376), (1242, 375), (1226, 370)]   # KITTI 00-02, 03, 04-10
    tightest = 0.0
    for scale, sigma_scale, hk in st.PAIRS:
        twl, thl, lds = header_plan(lph, slot[0], slot[1], scale, hk)
        tw, th = 1 << twl, 1 << thl
        step = 1.0 / scale
        xs, ys = {}, {}   # the tiles of an axis depend on that axis's size alone
        for cols, rows in sizes:
            assert header_plan(lph, cols, rows, scale, hk) is not None, (cols, rows, scale)   # a plan of its own
            if cols not in xs:
                xs[cols] = np.ascontiguousarray(axis_tiles(cols, scaled(cols, scale), step, twl, True), np.int32)
            if rows not in ys:
                ys[rows] = np.ascontiguousarray(axis_tiles(rows, scaled(rows, scale), step, thl, False), np.int32)
            xc, yr = xs[cols], ys[rows]
            need = lph.lph_max_tile_bytes(len(xc), xc.reshape(-1), len(yr), yr.reshape(-1), hk, tw, th)
            assert 0 < need <= lds, (slot, (cols, rows), scale, hk, need, lds)
            # the same from the restatement, for the corners of the tile grid
            for i in (0, len(xc) - 1):
                for j in (0, len(yr) - 1):
                    assert tile(xc[i][0], xc[i][1], yr[j][0], yr[j][1], xc[i][2], yr[j][2], hk, tw, th)[7] <= lds
            tightest = max(tightest, need / lds)
    assert tightest > 0.9   # (the bound is not vacuous: some tile comes close to what the plan provides)


def test_the_slots_tile_differs_from_a_small_images_own(lph):
    """tests/test_gpu_lsd_scale_sizes.py rests on it: in slots of 200 x 136 the two coarsest pairs run 32 x 16 tiles while a detector created
    at 64 x 64 runs 64 x 16 — the same bytes must come out of both"""
    for scale, sigma_scale in ((0.22, 0.8), (0.25, 1.0)):
        hk = st.sigma_radius(scale, sigma_scale)[1]
        assert header_plan(lph, 200, 136, scale, hk)[:2] == (5, 4)
        assert header_plan(lph, 64, 64, scale, hk)[:2] == (6, 4)


def test_the_kernel_and_the_header_state_one_tile_layout():
    """lsd_blur_resize_kernel keeps the four lines of the tile's layout as its own text (the header says why); br_tile_layout, which the
    checks above run, must be those lines: compared as text, comments and white space dropped"""
    import re

    def statements(path, begin, end):
        text = open(path).read()
        body = text[text.index(begin):]
        body = re.sub(r"//[^\n]*", "", body[:body.index(end)])
        return [re.sub(r"\s+", " ", s).strip() for s in body.split(";")]
    kernel = statements(os.path.join(ROOT, "stvo-pl_amd", "csrc", "lsd_scale_kernels.hip"), "const int nx = cmax - cmin + 1", "if (l.bytes > a.lds_bytes)")
    header = statements(HDRS[0], "const int nx = cmax - cmin + 1", "// The tile of the scaled image and the dynamic LDS")
    assert kernel[:3] == header[:3] and len(kernel[0]) > 20
    call = "br_layout(nx, ny, 4 * (((xlist ? 2 * ntw : nx) + 3) / 4), nr, hk, tw, th)"
    assert kernel[3] == "const BrLayout l = " + call
    assert "return " + call in header
