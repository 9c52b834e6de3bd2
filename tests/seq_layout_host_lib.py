"""Builds and binds tests/cpp/seq_layout_host.cpp (the product's seq_layout.h and the pipeline layout of seq_state.h, run on a null base on
the host) — TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SRC = os.path.join(HERE, "cpp", "seq_layout_host.cpp")
# seq_state.h includes the HIP headers; g++ reads them in host mode and nothing of the runtime is called or linked
FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")]

RAW = ("kp_l", "oct_l", "desc_l", "n_kp_l", "kp_r", "desc_r", "n_kp_r", "kl_l", "oct_ll", "ldesc_l", "n_kl_l", "kl_r", "ldesc_r", "n_kl_r")
SET = ("rc", "desc", "n", "spl", "epl", "sP", "eP", "le", "s2l", "s2lm", "ldesc", "nl")
MAIN = ("raw0", "raw1", "cams", "inv_wh", "qtab", "join_flag", "pose_flag", "pxy_l", "pstart", "pitems", "prank", "pperm", "prange", "pcell",
        "plstart", "plperm", "pstart2", "pperm2", "pcell2", "plstart2", "plperm2", "lxy_l", "lstart", "litems", "lrank", "lperm", "ldir",
        "top2", "owner2", "elig", "elig_cnt", "govf", "elig_l", "elig_cnt_l", "govf_l", "m12s_p", "m12s_l", "m12p", "m12l", "inlp",
        "inll", "results", "counts", "m12l_alt", "cover_l", "top2_l", "owner2_l", "knn12_l", "knn21_l", "cand_l", "need_l", "qsel_l",
        "nsel_l") + tuple("set%d.%s" % (t, k) for t in range(3) for k in SET)
FETCH = ("off_m12s_l", "off_m12p", "off_m12l", "off_inlp", "off_inll", "off_flag", "m12_span", "inl_span")

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "cpp", "libseq_layout_host.so")
    csrc = os.path.join(HERE, "..", "stvo-pl_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, h) for h in ("carver.h", "seq_layout.h", "seq_state.h", "grid_scratch.h", "kernels.h", "ctx_internal.h", "step_plan.h")] + \
        [os.path.join(HERE, "..", "include", h) for h in ("stvo_hip.h", "stvo_types.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1"] + FLAGS + ["-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    lib.slh_raw.argtypes = [C.c_int, C.c_int, C.c_int, i64p]
    lib.slh_main.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, i64p]
    lib.slh_keyframe.argtypes = [C.c_int, C.c_int, C.c_int, i64p]
    _lib = lib
    return lib


def raw(B, K, M):
    """-> ({array: offset}, first byte of the key-line part, raw_frame_bytes)"""
    out = np.zeros(16, np.int64)
    assert load().slh_raw(B, K, M, out) == 16
    return dict(zip(RAW, out[:14].tolist())), int(out[14]), int(out[15])


def main(B, K, M, ws):
    """-> ({buffer: offset, -1 = not cut} in the order of MAIN, {FETCH entry: bytes}, total bytes)"""
    out = np.zeros(len(MAIN) + len(FETCH) + 1, np.int64)
    assert load().slh_main(B, K, M, ws, out) == len(out)
    return dict(zip(MAIN, out[:len(MAIN)].tolist())), dict(zip(FETCH, out[len(MAIN):-1].tolist())), int(out[-1])


def keyframe(B, K, M):
    """-> ({array of the set: offset, -1 = not cut}, offset of the headers, total bytes)"""
    out = np.zeros(14, np.int64)
    assert load().slh_keyframe(B, K, M, out) == 14
    return dict(zip(SET, out[:12].tolist())), int(out[12]), int(out[13])
