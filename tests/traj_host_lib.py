"""Builds and binds tests/cpp/traj_host.cpp (the product's traj_update.h compiled for the host) — TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

from stvo_amd.ctypes_types import POSE_RESULT_DTYPE, TRAJ_RECORD_DTYPE, TRAJ_STATE_DTYPE, TrajParams

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(HERE, "cpp", "traj_host.cpp")
    so = os.path.join(HERE, "cpp", "libtraj_host.so")
    hdrs = [os.path.join(HERE, "..", "stvo-pl_amd", "csrc", h) for h in ("traj_update.h", "pose_math.h")] + \
           [os.path.join(HERE, "..", "include", "stvo_types.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.trh_sizes.argtypes = [C.POINTER(C.c_int)]; lib.trh_sizes.restype = None
    lib.trh_init.argtypes = [C.c_int, C.c_void_p]; lib.trh_init.restype = None
    lib.trh_update.argtypes = [C.c_int, C.c_void_p, C.POINTER(TrajParams), C.c_void_p, C.c_void_p]; lib.trh_update.restype = None
    _lib = lib
    return lib


def sizes():
    out = (C.c_int * 3)()
    load().trh_sizes(out)
    return tuple(out)


def init(B):
    state = np.zeros(B, dtype=TRAJ_STATE_DTYPE)
    load().trh_init(B, state.ctypes.data_as(C.c_void_p))
    return state


def update(results, prm, state, want_records=True):
    """One update of len(state) streams in place; results: POSE_RESULT_DTYPE array of the same length.  Returns the records."""
    B = len(state)
    assert results.dtype == POSE_RESULT_DTYPE and len(results) == B and state.dtype == TRAJ_STATE_DTYPE
    results = np.ascontiguousarray(results)
    rec = np.zeros(B, dtype=TRAJ_RECORD_DTYPE) if want_records else None
    load().trh_update(B, results.ctypes.data_as(C.c_void_p), C.byref(prm), state.ctypes.data_as(C.c_void_p),
                      rec.ctypes.data_as(C.c_void_p) if want_records else None)
    return rec
