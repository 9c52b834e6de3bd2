"""Builds and binds tests/cpp/track_host.cpp (the product's track_update.h compiled for the host) — TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

from np_tracks import PARK, RESTART, RUN, TRACK

HERE = os.path.dirname(os.path.abspath(__file__))
MODE_RUN, MODE_INIT, MODE_PARK = 0, 1, 2
SENTINEL = np.array([(-77, 777, 7, -7)], TRACK)[0]
_lib = None


def sources():
    src = os.path.join(HERE, "cpp", "track_host.cpp")
    hdrs = [os.path.join(HERE, "..", "stvo-pl_amd", "csrc", "track_update.h"), os.path.join(HERE, "..", "include", "stvo_types.h")]
    return src, hdrs


def load():
    global _lib
    if _lib is not None:
        return _lib
    src, hdrs = sources()
    so = os.path.join(HERE, "cpp", "libtrack_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.tkh_sizes.argtypes = [C.POINTER(C.c_int)]; lib.tkh_sizes.restype = None
    lib.tkh_step.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.tkh_step.restype = C.c_int
    lib.tkh_step_batch.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 7; lib.tkh_step_batch.restype = None
    _lib = lib
    return lib


def sizes():
    out = (C.c_int * 2)()
    load().tkh_sizes(out)
    return tuple(out)


def mode_of(ctl, first):
    return MODE_INIT if (first or ctl == RESTART) else (MODE_PARK if ctl == PARK else MODE_RUN)


def step(prev_state, m12, inl, n_cur, ctl=RUN, first=False, new_kf=0, lanes=1, cap=None):
    """np_tracks.step by the header: returns (record, state) of capacity `cap` (default n_cur) whose rows beyond n_cur hold SENTINEL."""
    cap = n_cur if cap is None else cap
    n_prev = len(prev_state)
    prev = np.ascontiguousarray(prev_state, TRACK)
    m12 = np.ascontiguousarray(m12[:n_prev] if m12 is not None else np.zeros(0), np.int32)
    inl = np.ascontiguousarray(inl[:n_prev] if inl is not None else np.zeros(0), np.int32)
    rec, nxt = np.full(max(cap, 1), SENTINEL, TRACK), np.full(max(cap, 1), SENTINEL, TRACK)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    load().tkh_step(n_prev, p(m12), p(inl), p(prev), n_cur, mode_of(ctl, first), int(new_kf), p(rec), p(nxt), lanes)
    return rec[:cap], nxt[:cap]
