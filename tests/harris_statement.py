"""ctypes binding of the plain-C Harris statement tests/cpp/harris_ref.c — test infrastructure, compiled at first use into a
temporary directory (nothing is written into the repository)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "harris_ref.c")
_cached = None


class Statement:
    def __init__(self, lib):
        self.lib = lib
        u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"); i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
        f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
        lib.harris_responses.argtypes = [u8p, C.c_int, C.c_int, i32p, i32p, f32p, i32p]; lib.harris_responses.restype = None
        lib.harris_response_sums.argtypes = [C.c_int, C.c_int, C.c_int]; lib.harris_response_sums.restype = C.c_float

    def responses(self, img, xs, ys):
        """-> (float32 responses [n], int32 sums a, b, c [n, 3])"""
        img = np.ascontiguousarray(img, np.uint8)
        xs = np.ascontiguousarray(xs, np.int32); ys = np.ascontiguousarray(ys, np.int32)
        out = np.zeros(len(xs), np.float32); abc = np.zeros((len(xs), 3), np.int32)
        self.lib.harris_responses(img.reshape(-1), img.shape[1], len(xs), xs, ys, out, abc.reshape(-1))
        return out, abc

    def response_of_sums(self, a, b, c):
        return np.float32(self.lib.harris_response_sums(int(a), int(b), int(c)))


def load():
    global _cached
    if _cached is None:
        d = tempfile.mkdtemp(prefix="harris_ref_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libharris_ref.so")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC])
        _cached = Statement(C.CDLL(so))
    return _cached
