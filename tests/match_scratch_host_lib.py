"""Builds and binds tests/cpp/match_scratch_host.cpp (the product's match_scratch.h: the matcher's scratch views, its capacity
predicate, knn_pick_nseg and block_threshold, run on the host) — TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "match_scratch_host.cpp")
HDR = os.path.join(HERE, "..", "stvo-pl_amd", "csrc", "match_scratch.h")
FLAGS = ["-std=c++17", "-Wall", "-Wextra"]  # no HIP include path: the header is host-pure

VIEWS = ("knn12_seg0", "knn12_seg1", "claim", "cand", "qsel", "nsel0", "nsel1", "nsel2", "nsel3", "nsel4", "blocked", "tsel")
ARRAYS = ("knn12", "knn21", "cand", "claim", "qsel", "nsel")
BASE = {a: (k + 1) << 40 for k, a in enumerate(ARRAYS)}  # far apart: an address names its array

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "cpp", "libmatch_scratch_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in (SRC, HDR)):
        subprocess.check_call(["g++", "-O1"] + FLAGS + ["-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    lib.msh_views.argtypes = [C.c_int, C.c_int, C.c_longlong, i64p, i64p]
    lib.msh_fits.argtypes = [C.c_int, C.c_int, C.c_longlong]
    lib.msh_pick_nseg.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int]
    lib.msh_block_threshold.argtypes = [C.c_int, C.c_float]
    lib.msh_nseg_limits.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    _lib = lib
    return lib


def views(B, row_stride, capacity):
    """-> ({view: (array it lies in, byte offset in that array)}, per)"""
    base = np.array([BASE[a] for a in ARRAYS], np.int64)
    out = np.zeros(len(VIEWS) + 1, np.int64)
    assert load().msh_views(B, row_stride, capacity, base, out) == len(out)
    res = {}
    for name, addr in zip(VIEWS, out[:-1].tolist()):
        arr = ARRAYS[(addr >> 40) - 1]
        res[name] = (arr, addr - BASE[arr])
    return res, int(out[-1])


def fits(B, row_stride, capacity):
    return bool(load().msh_fits(B, row_stride, capacity))


def pick_nseg(B, max_n, capacity, forced=0):
    return int(load().msh_pick_nseg(B, max_n, capacity, forced))


def block_threshold(d0, nnr):
    return int(load().msh_block_threshold(d0, float(nnr)))


def nseg_limits():
    lo, hi = C.c_int(), C.c_int()
    load().msh_nseg_limits(C.byref(lo), C.byref(hi))
    return lo.value, hi.value
