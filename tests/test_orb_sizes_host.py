"""The geometry of the ORB pyramid per image size (stvo-pl_amd/csrc/orb_sizes.h), run on the host through tests/cpp/orb_sizes_host.cpp:
what stvo_orb_set_image_sizes writes into its device table — level sizes, the resize's inverse scales, the rule by which a level yields
anything — against the oracle's statement oracle.orb_levels (orc_orb_levels) and the expression stvo_orb_create hands the resize kernel,
1.0 / ((double)dsize / ssize).  No GPU.  The header is also what stvo_orb_create forms the slot's own levels with, so the existing ORB
suites hold it on the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "orb_sizes_host.cpp")
HDR = os.path.join(ROOT, "stvo-pl_amd", "csrc", "orb_sizes.h")
NEW_SYMBOLS = ("stvo_orb_set_image_sizes", "stvo_seq_restart_cameras")
i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def osh():
    so = os.path.join(HERE, "cpp", "liborb_sizes_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        tmp = "%s.%d.so" % (so[:-3], os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SRC])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.osh_level_sizes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, i32p, i32p, f64p, f64p, i32p]
    lib.osh_budgets.argtypes = [C.c_int, C.c_int, C.c_double, i32p]
    lib.osh_sizes_ok.argtypes = [i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    return lib


def table(lib, cols, rows, nfeatures, nlevels, scale, edge_th):
    lc, lr, act = (np.zeros(nlevels, np.int32) for _ in range(3))
    sx, sy = np.zeros(nlevels), np.zeros(nlevels)
    lib.osh_level_sizes(cols, rows, nfeatures, nlevels, scale, edge_th, lc, lr, sx, sy, act)
    return lc, lr, sx, sy, act


def test_row_is_32_bytes(osh):
    assert osh.osh_row_bytes() == 32


@pytest.mark.parametrize("scale", [1.2, 2.0])
@pytest.mark.parametrize("nlevels", [1, 4, 8])
def test_levels_against_the_oracle(osh, oracle, nlevels, scale):
    nfeatures, edge_th = 600, 19
    sizes = [(c, r) for c in range(64, 261, 7) for r in (64, 65, 97, 136, 260)] + [(c, c) for c in range(64, 261)] + \
            [(260, r) for r in range(64, 261)]
    seen_inactive = seen_odd = 0
    for cols, rows in sizes:
        _, oc, orr, onf = oracle.orb_levels(cols, rows, nfeatures, nlevels, scale)
        lc, lr, sx, sy, act = table(osh, cols, rows, nfeatures, nlevels, scale, edge_th)
        assert np.array_equal(lc, oc) and np.array_equal(lr, orr), (cols, rows)
        nf = np.zeros(nlevels, np.int32)
        osh.osh_budgets(nfeatures, nlevels, scale, nf)
        if nlevels > 1:
            assert np.array_equal(nf, onf)
        else:
            assert nf[0] == nfeatures   # one level takes the whole budget (stvo_orb_create)
        # the rule of orc_orb_detect_levels / stvo_orb_create (the kernels' word loads ask for 16 pixels, less than any border allows)
        want = [int(nf[l] > 0 and 2 * edge_th < oc[l] and 2 * edge_th < orr[l] and oc[l] >= 16 and orr[l] >= 16) for l in range(nlevels)]
        assert list(act) == want, (cols, rows)
        seen_inactive += want.count(0)
        seen_odd += int(any(v % 2 for v in oc[1:]))
        assert sx[0] == 1.0 and sy[0] == 1.0
        for l in range(1, nlevels):
            with np.errstate(divide="ignore", invalid="ignore"):   # (a level of 0 pixels — 64 / 2^7 — divides by zero in C as here)
                ex = np.float64(1.0) / (np.float64(oc[l]) / np.float64(oc[l - 1]))   # doubles: the expression of the uniform path
                ey = np.float64(1.0) / (np.float64(orr[l]) / np.float64(orr[l - 1]))
            for got, exp in ((sx[l], ex), (sy[l], ey)):
                assert np.float64(got).tobytes() == exp.tobytes() or (np.isnan(got) and np.isnan(exp)), (cols, rows, l)
    if nlevels > 1:
        assert seen_inactive and seen_odd   # the sweep meets levels below the border and levels of odd size


def test_levels_are_monotone_in_the_size(osh):
    """every entry's level fits the slot's level buffer: cvRound of a monotone function"""
    for scale in (1.2, 1.37, 2.0):
        prev = None
        for c in range(64, 400):
            lc = table(osh, c, c, 500, 8, scale, 19)[0]
            if prev is not None:
                assert np.all(lc >= prev)
            prev = lc


def test_validation(osh):
    def ok(sizes, B, slot=(200, 136), edge=19):
        a = np.ascontiguousarray(sizes, np.int32).reshape(-1, 2)
        return bool(osh.osh_sizes_ok(a, len(a), B, slot[0], slot[1], edge))
    assert ok([(200, 136), (64, 64)], 10) and ok([(128, 64)] * 5, 10) and ok([(199, 135)], 3)
    assert not ok([(200, 136)] * 3, 10)                 # B % n != 0
    assert not ok([(200, 136)] * 11, 10)                # n > B
    assert not ok([(201, 136)], 10) and not ok([(200, 137)], 10)      # larger than the slot
    assert not ok([(63, 64)], 10) and not ok([(64, 63)], 10)          # below what create takes
    assert not ok([(64, 64)], 10, edge=32) and ok([(65, 65)], 10, edge=32)   # 2 * edge_threshold >= size
    assert not osh.osh_sizes_ok(np.zeros((1, 2), np.int32), 0, 10, 200, 136, 19)


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
    assert lib.stvo_abi_version() == 3
