"""Builds and binds tests/cpp/frontend_layout_host.cpp (the product's frontend_layout.h and gaussian_q8.h, run on the host) — TEST
INFRASTRUCTURE ONLY.  Every layout call returns ({buffer: offset, -1 = not cut} in the order it is cut, total bytes)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "frontend_layout_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror"]

ORB_HEAD = ("pattern", "th_own", "effective")
ORB_LEVEL = ("blur", "hist", "cand", "hkey", "n_cand", "img", "kp", "resp", "ang", "desc", "n", "n_tot")
ORB_STAGING = ("img", "kp", "resp", "ang", "oct", "desc", "n", "n_total")
LBD_ARENA = ("blur", "dxy")
LBD_STAGING = ("img", "lines", "n", "desc", "desc_f")
LSD_ARENA = ("blur", "scaled", "img", "px", "k32", "cnt", "order", "reg", "kmax", "seg", "n_seg", "lines", "response", "n_lines", "n_pass")
LSD_XCD = ("stamp", "wlist", "pend", "ctl")
FLD_ARENA = ("img", "ebits", "sbits", "wsum", "lab", "tmp", "list", "cnt", "n_edge", "pts", "ch_at", "ch", "n_ch", "sg", "dseg", "n_seg",
             "err", "lines", "response", "n_lines")
SIDES = ("src_l", "src_r", "dst_l", "dst_r")
GRAY = ("src", "gray", "swapped")
CONSTS = ("sizeof_LsdPx", "sizeof_FldChain", "sizeof_keyline", "LSD_UNIT", "LSD_CTL", "FLD_UNIT", "FLD_BINS", "FLD_SEG_CAP", "LBD_DESC_FLOATS")

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "cpp", "libfrontend_layout_host.so")
    csrc = os.path.join(HERE, "..", "stvo-pl_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, h) for h in ("frontend_layout.h", "carver.h", "gaussian_q8.h")] + \
        [os.path.join(HERE, "..", "include", "stvo_types.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = "%s.%d.so" % (so[:-3], os.getpid())  # (test processes running side by side each build their own and rename it into place)
        subprocess.check_call(["g++", "-O1"] + FLAGS + ["-fPIC", "-shared", "-o", tmp, SRC])
        os.replace(tmp, so)
    _lib = C.CDLL(so)
    return _lib


def consts():
    lib = load()
    return {k: lib.flh_const(i) for i, k in enumerate(CONSTS)}


def _call(fn, names, *args):
    out = (C.c_longlong * (len(names) + 8))()
    n = getattr(load(), fn)(*args, out)
    assert n >= len(names) + 1
    return dict(zip(names, out[:len(names)])), int(out[len(names)]), [int(v) for v in out[len(names) + 1:n]]


def orb_arena(B, K, cols, rows):
    """cols / rows: the sizes of the levels"""
    names = ORB_HEAD + tuple("L%d.%s" % (l, k) for l in range(len(cols)) for k in ORB_LEVEL)
    arr = C.c_int * len(cols)
    return _call("flh_orb_arena", names, B, K, len(cols), arr(*cols), arr(*rows))[:2]


def orb_cand_cap(cols, rows):
    return load().flh_orb_cand_cap(cols, rows)


def orb_staging(B, cols, rows, K):
    return _call("flh_orb_staging", ORB_STAGING, B, cols, rows, K)[:2]


def lbd_arena(B, cols, rows):
    return _call("flh_lbd_arena", LBD_ARENA, B, cols, rows)[:2]


def lbd_staging(B, cols, rows, M):
    return _call("flh_lbd_staging", LBD_STAGING, B, cols, rows, M)[:2]


def lsd_arena(B, cols, rows, w, h, n_bins, seg_cap, K, blur7):
    return _call("flh_lsd_arena", LSD_ARENA, B, cols, rows, w, h, n_bins, seg_cap, K, int(blur7))[:2]


def lsd_xcd_route(refine, B, npx):
    """whether stvo_lsd_create cuts the small-batch arena"""
    return bool(load().flh_lsd_xcd_route(refine, B, C.c_longlong(npx)))


def lsd_xcd_arena(B, npx, nw):
    """-> (offsets, total, (stamp_bytes, pend_ctl_bytes): the two spans a call clears)"""
    off, total, spans = _call("flh_lsd_xcd_arena", LSD_XCD, B, C.c_longlong(npx), nw)
    return off, total, tuple(spans)


def fld_arena(B, cols, rows, L, K):
    return _call("flh_fld_arena", FLD_ARENA, B, cols, rows, L, K)[:2]


def fld_geometry(npx, L):
    """-> (nw, nunits, capacity of the chain and segment stores)"""
    out = (C.c_int * 3)()
    load().flh_fld_geometry(npx, L, out)
    return tuple(out)


def rectify_staging(B, cols, rows):
    return _call("flh_rectify_staging", SIDES, B, cols, rows)[:2]


def color_rectify_staging(n, cols, rows, channels):
    return _call("flh_color_rectify_staging", SIDES, n, cols, rows, channels)[:2]


def gray_staging(npix, channels):
    return _call("flh_gray_staging", GRAY, C.c_longlong(npix), channels)[:2]


def gaussian_q8(radius, sigma):
    w = np.full(1 + 2 * radius + 1, -7, np.int32)  # (one guard entry behind the weights)
    load().flh_gaussian_q8(radius, C.c_double(sigma), w.ctypes.data_as(C.c_void_p))
    assert w[-1] == -7
    return w[:-1]
