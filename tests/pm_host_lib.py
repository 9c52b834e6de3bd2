"""Builds and binds tests/cpp/pm_host.cpp (the product's pose_math.h compiled for the host) — TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

from stvo_amd.ctypes_types import Cam

HERE = os.path.dirname(os.path.abspath(__file__))
f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(HERE, "cpp", "pm_host.cpp")
    so = os.path.join(HERE, "cpp", "libpm_host.so")
    hdr = os.path.join(HERE, "..", "stvo-pl_amd", "csrc", "pose_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    for n in ("pmh_expmap", "pmh_logmap", "pmh_inverse_se3", "pmh_adjoint", "pmh_inverse6", "pmh_inverse6_mem", "pmh_eig6", "pmh_step_pose",
              "pmh_eig6_ql"):
        getattr(lib, n).argtypes = [f64p, f64p]; getattr(lib, n).restype = None
    lib.pmh_unccomp.argtypes = [f64p] * 4
    lib.pmh_solve6.argtypes = [f64p, f64p, f64p, C.POINTER(C.c_double)]; lib.pmh_solve6.restype = C.c_int
    lib.pmh_solve6_spd.argtypes = [f64p, f64p, f64p, C.POINTER(C.c_double)]; lib.pmh_solve6_spd.restype = C.c_int
    lib.pmh_solve6_mem.argtypes = [f64p, f64p, f64p, C.POINTER(C.c_double)]; lib.pmh_solve6_mem.restype = C.c_int
    lib.pmh_inverse6_spd.argtypes = [f64p, f64p]; lib.pmh_inverse6_spd.restype = C.c_int
    lib.pmh_line_overlap.argtypes = [f64p] * 4; lib.pmh_line_overlap.restype = C.c_double
    lib.pmh_stereo_row_overlap.argtypes = [C.c_double] * 5; lib.pmh_stereo_row_overlap.restype = C.c_double
    lib.pmh_stereo_line_disparities.argtypes = [C.c_double] * 5 + [f64p]; lib.pmh_stereo_line_disparities.restype = None
    for n in ("pmh_normal_eq", "pmh_normal_eq_q"):
        getattr(lib, n).argtypes = [f64p, C.POINTER(Cam), C.c_double, C.c_void_p, C.c_int, C.c_double, C.c_double, f64p]
        getattr(lib, n).restype = None
    _lib = lib
    return lib


def unpack28(acc):
    """acc[0..20] upper triangle of H (row-major), acc[21..26] g, acc[27] e (not yet divided by n)."""
    H = np.zeros((6, 6)); k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = acc[k]; k += 1
    return H, acc[21:27].copy(), acc[27]
