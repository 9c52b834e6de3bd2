"""Builds and binds tests/cpp/pose_scratch_host.cpp (the product's pose_scratch.h: the route of a pose launch and the arena bytes of the
batch kernels, run on the host) — TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "pose_scratch_host.cpp")
HDRS = [os.path.join(HERE, "..", "stvo-pl_amd", "csrc", h) for h in ("pose_scratch.h", "debug_switches.h")] + \
       [os.path.join(HERE, "..", "include", h) for h in ("stvo_hip.h", "stvo_types.h")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra"]  # no HIP include path: the headers are host-pure

FIELDS = ("batch", "waves", "inline_sync", "start_flag", "arena_bytes")

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "cpp", "libpose_scratch_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1"] + FLAGS + ["-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.psh_route.argtypes = [C.c_int] * 6 + [np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")]
    lib.psh_pair_words.argtypes = [C.c_int]
    lib.psh_pair_words.restype = C.c_longlong
    _lib = lib
    return lib


def unset():
    return int(load().psh_unset())


def route(B, compact, evaluation, cus, pose_kernel=None, pose2p_nw=None):
    """-> {field: value} of stvo::pose_route; a switch given as None is unset"""
    u = unset()
    out = np.zeros(5, np.int64)
    assert load().psh_route(B, int(compact), int(evaluation), cus, u if pose_kernel is None else pose_kernel,
                            u if pose2p_nw is None else pose2p_nw, out) == 5
    d = dict(zip(FIELDS, out.tolist()))
    for k in ("batch", "inline_sync", "start_flag"):
        d[k] = bool(d[k])
    return d


def pair_words(compact):
    return int(load().psh_pair_words(int(compact)))


def constants():
    lib = load()
    return dict(word_bytes=lib.psh_word_bytes(), max_points=lib.psh_max_points(), max_lines=lib.psh_max_lines())
