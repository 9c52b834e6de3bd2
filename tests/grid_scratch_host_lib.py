"""Builds and binds tests/cpp/grid_scratch_host.cpp (the product's grid_scratch.h: the scratch of the stereo grid matchers, its element
counts, the matrix dimensions and the carve, run on the host) — TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "grid_scratch_host.cpp")
HDRS = [os.path.join(HERE, "..", "stvo-pl_amd", "csrc", h) for h in ("grid_scratch.h", "carver.h")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra"]  # no HIP include path: the headers are host-pure

ARRAYS = ("cover", "top2", "owner2", "elig", "elig_cnt", "ovf")
POINTERS = ARRAYS + ("misfit",)
ROWS, ELIG, ALL = 1, 2, 3  # GridScratchParts

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "cpp", "libgrid_scratch_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1"] + FLAGS + ["-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    lib.gsh_counts.argtypes = [C.c_int] * 5 + [i64p]
    lib.gsh_dims.argtypes = [C.c_int, C.c_int, i64p]
    lib.gsh_route_words.argtypes = [C.c_int]
    lib.gsh_route_words.restype = C.c_longlong
    lib.gsh_carve.argtypes = [C.c_int] * 6 + [C.c_longlong, i64p]
    _lib = lib
    return lib


def counts(B, rows1, rows2, with_bit_matrix, with_misfit):
    """-> {array: elements}"""
    out = np.zeros(6, np.int64)
    assert load().gsh_counts(B, rows1, rows2, int(with_bit_matrix), int(with_misfit), out) == 6
    return dict(zip(ARRAYS, out.tolist()))


def dims(rows1, rows2):
    """-> (words64, n1p, words of one frame's matrix)"""
    out = np.zeros(3, np.int64)
    assert load().gsh_dims(rows1, rows2, out) == 3
    return tuple(out.tolist())


def route_words(B):
    return int(load().gsh_route_words(B))


def elig_slots():
    return int(load().gsh_elig_slots())


def carve(B, rows1, rows2, with_bit_matrix, with_misfit, first=ALL, lead=0):
    """-> ({pointer: byte offset, -1 = null, -2 = a half touched the other's}, the carver's offset behind the carve)"""
    out = np.zeros(8, np.int64)
    assert load().gsh_carve(B, rows1, rows2, int(with_bit_matrix), int(with_misfit), first, lead, out) == 8
    return dict(zip(POINTERS, out[:7].tolist())), int(out[7])
