"""The geometry of one image size under a line detector's parameters (stvo-pl_amd/csrc/lsd_sizes.h), run on the host through
tests/cpp/lsd_sizes_host.cpp: what stvo_lsd_set_image_sizes writes into its device table — the scaled size, the smallest region, the
resize's inverse ratio, the minimum length, the two rows that drive the shared blur and resize — against stvo_lsd_geometry (which forms
the slot's own values with the same functions) and the oracle's statement (orc_lsd_scaled_size, orc_lsd_min_reg_size).  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "lsd_sizes_host.cpp")
HDRS = [os.path.join(ROOT, "stvo-pl_amd", "csrc", n) for n in ("lsd_sizes.h", "orb_sizes.h")]
NEW_SYMBOLS = ("stvo_lsd_set_image_sizes", "stvo_lbd_set_image_sizes")
i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")

SLOT = (200, 136)
TEST_SIZES = [(200, 136), (199, 135), (129, 65), (128, 64), (64, 64)]        # the sizes of tests/test_gpu_lsd_sizes.py
KITTI_SIZES = [(1241, 376), (1242, 375), (1226, 370)]                         # KITTI 00-02, 03, 04-10
SCALES = [1.0, 1.2, 0.8]
ANG_TH = 22.5


@pytest.fixture(scope="module")
def lsh():
    so = os.path.join(HERE, "cpp", "liblsd_sizes_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        tmp = "%s.%d.so" % (so[:-3], os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SRC])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.lsh_row.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, i32p, C.POINTER(C.c_double), i32p, f64p]
    lib.lsh_scaled_extent.argtypes = [C.c_int, C.c_double]; lib.lsh_scaled_extent.restype = C.c_double
    lib.lsh_min_reg_size.argtypes = [C.c_int, C.c_int, C.c_double]
    lib.lsh_inv_ratio.argtypes = [C.c_double]; lib.lsh_inv_ratio.restype = C.c_double
    lib.lsh_entry_min_length.argtypes = [C.c_void_p, C.c_int, C.c_double]; lib.lsh_entry_min_length.restype = C.c_double
    lib.lsh_sizes_ok.argtypes = [i32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]
    lib.lsh_lbd_sizes_ok.argtypes = [i32p, C.c_int, C.c_int, C.c_int, C.c_int]
    return lib


def row(lib, cols, rows, scale, min_length=0.0):
    out, ml = np.zeros(5, np.int32), C.c_double()
    srows, sinv = np.zeros(6, np.int32), np.zeros(4)
    lib.lsh_row(cols, rows, scale, ANG_TH, min_length, out, C.byref(ml), srows, sinv)
    return dict(cols=int(out[0]), rows=int(out[1]), w=int(out[2]), h=int(out[3]), min_reg_size=int(out[4]), min_length=ml.value,
                srows=srows.reshape(2, 3), sinv=sinv.reshape(2, 2))


def oracle_statement(oracle, cols, rows, scale):
    oracle.lib.orc_lsd_scaled_size.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    oracle.lib.orc_lsd_scaled_size.restype = None
    oracle.lib.orc_lsd_min_reg_size.argtypes = [C.c_int, C.c_int, C.c_double]
    oracle.lib.orc_lsd_min_reg_size.restype = C.c_int
    w, h = C.c_int(cols), C.c_int(rows)
    if scale != 1:
        oracle.lib.orc_lsd_scaled_size(cols, rows, scale, C.byref(w), C.byref(h))
    return w.value, h.value, int(oracle.lib.orc_lsd_min_reg_size(w.value, h.value, ANG_TH))


def test_row_is_32_bytes(lsh):
    assert lsh.lsh_row_bytes() == 32


@pytest.mark.parametrize("scale", SCALES)
def test_rows_against_geometry_and_the_oracle(lsh, oracle, scale):
    from stvo_amd import capi
    for cols, rows in TEST_SIZES + KITTI_SIZES:
        r = row(lsh, cols, rows, scale, min_length=0.025 * min(cols, rows))
        geo = capi.lsd_geometry(capi.lsd_params(scale=scale), cols, rows)
        ow, oh, omin = oracle_statement(oracle, cols, rows, scale)
        assert (r["cols"], r["rows"]) == (cols, rows)
        assert (r["w"], r["h"]) == (geo["cols"], geo["rows"]) == (ow, oh), (cols, rows, scale)
        assert r["min_reg_size"] == omin == lsh.lsh_min_reg_size(ow, oh, ANG_TH), (cols, rows, scale)
        assert r["min_length"] == 0.025 * min(cols, rows)
        assert lsh.lsh_scaled_extent(cols, scale) == float(ow) and lsh.lsh_scaled_extent(rows, scale) == float(oh)
        if scale == 1:
            assert (r["w"], r["h"]) == (cols, rows)
        else:
            assert (r["w"], r["h"]) == (int(np.rint(cols * scale)), int(np.rint(rows * scale)))   # half to even, as cvRound
        # the rows of the blur and the resize: the input size, then the scaled size with 1 / scale as the uniform path forms it
        assert r["srows"].tolist() == [[cols, rows, 1], [ow, oh, 1]]
        inv = np.float64(1.0) / np.float64(scale)
        assert r["sinv"][0].tolist() == [1.0, 1.0]
        assert r["sinv"][1, 0].tobytes() == inv.tobytes() == r["sinv"][1, 1].tobytes()
        assert np.float64(lsh.lsh_inv_ratio(scale)).tobytes() == inv.tobytes()


def test_min_reg_size_differs_from_the_slots(lsh):
    """a detector that took the slot's smallest region for every image is wrong for these: by hand, 200 x 136 at 1.2 is 240 x 163,
    -(2.5 (log10 240 + log10 163) + log10 11) / log10 0.125 = 13.87 -> 13; 64 x 64 is 77 x 77: 11.60 -> 11"""
    slot = row(lsh, SLOT[0], SLOT[1], 1.2)["min_reg_size"]
    assert slot == 13
    assert row(lsh, 64, 64, 1.2)["min_reg_size"] == 11
    own = [row(lsh, c, r, 1.2)["min_reg_size"] for c, r in TEST_SIZES]
    assert sum(1 for v in own if v != slot) >= 2, own


def test_scaled_sizes_are_monotone_in_the_size(lsh):
    """every entry's scaled image fits the slot's scaled buffer: rint of a monotone function"""
    for scale in (0.5, 0.8, 1.2, 1.37, 2.0):
        ext = [lsh.lsh_scaled_extent(n, scale) for n in range(8, 1300)]
        assert all(b >= a for a, b in zip(ext, ext[1:]))


def test_minimum_length_per_entry(lsh):
    ml = np.array([9.4, 9.375, 9.25])
    assert [lsh.lsh_entry_min_length(ml.ctypes.data, i, 5.0) for i in range(3)] == [9.4, 9.375, 9.25]
    assert [lsh.lsh_entry_min_length(None, i, 5.0) for i in range(3)] == [5.0, 5.0, 5.0]
    # the reference's Config::minLineLength() x min(width, height) for the three KITTI sizes
    assert [0.025 * min(c, r) for c, r in KITTI_SIZES] == [9.4, 9.375, 9.25]


def test_validation(lsh):
    def ok(sizes, B, slot=SLOT, scale=1.2, ml=None):
        a = np.ascontiguousarray(sizes, np.int32).reshape(-1, 2)
        m = None if ml is None else np.ascontiguousarray(ml, np.float64)
        return bool(lsh.lsh_sizes_ok(a, None if m is None else m.ctypes.data, len(a), B, slot[0], slot[1], scale))
    assert ok(TEST_SIZES, 10) and ok(TEST_SIZES * 2, 10) and ok([(199, 135)], 3) and ok([(8, 8)], 2)
    assert ok(TEST_SIZES, 10, ml=[1.0, 2.0, 3.0, 4.0, 0.0])
    assert not ok(TEST_SIZES, 10, ml=[1.0, 2.0, float("nan"), 4.0, 0.0])
    assert not ok([(200, 136)] * 3, 10)                               # B % n != 0
    assert not ok([(200, 136)] * 11, 10)                              # n > B
    assert not ok([(201, 136)], 10) and not ok([(200, 137)], 10)      # larger than the slot
    assert not ok([(7, 64)], 10) and not ok([(64, 7)], 10)            # below what stvo_lsd_create takes
    assert not ok([(8, 8)], 2, scale=0.05) and not ok([(10, 10)], 2, scale=0.05) and ok([(12, 12)], 2, scale=0.05)   # nothing is left: rint(0.4) = rint(0.5) = 0
    assert not lsh.lsh_sizes_ok(np.zeros((1, 2), np.int32), None, 0, 10, 200, 136, 1.2)

    def lbd_ok(sizes, B, slot=SLOT):
        a = np.ascontiguousarray(sizes, np.int32).reshape(-1, 2)
        return bool(lsh.lsh_lbd_sizes_ok(a, len(a), B, slot[0], slot[1]))
    assert lbd_ok(TEST_SIZES, 10) and lbd_ok([(8, 8)], 2)
    assert not lbd_ok([(200, 136)] * 3, 10) and not lbd_ok([(201, 136)], 10) and not lbd_ok([(200, 137)], 10)
    assert not lbd_ok([(7, 8)], 2) and not lbd_ok([(8, 7)], 2)


def test_what_create_refuses_as_a_size_is_refused(lsh):
    """the check of an entry against stvo_lsd_geometry's own verdict on that size, for sizes inside an accepted slot"""
    from stvo_amd import capi
    for scale in (1.0, 1.2, 0.8, 0.05):
        prm = capi.lsd_params(scale=scale, sigma_scale=0.6 if scale > 0.1 else 0.1)
        capi.lsd_geometry(prm, 200, 136)
        for size in [(8, 8), (7, 9), (9, 7), (10, 10), (12, 8), (64, 64), (200, 136)]:
            try:
                capi.lsd_geometry(prm, *size)
                accepted = True
            except capi.StvoError:
                accepted = False
            a = np.array([size], np.int32)
            assert bool(lsh.lsh_sizes_ok(a, None, 1, 2, 200, 136, scale)) == accepted, (scale, size)


def test_header_declares_and_library_exports_the_new_symbols():
    from stvo_amd import capi
    hdr = open(os.path.join(ROOT, "include", "stvo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
