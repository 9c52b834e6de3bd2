"""ctypes binding of the FLD CPU statement tests/cpp/fld_ref.c — test infrastructure.  The statement is compiled at first use
(gcc -O2 -ffp-contract=off) into a temporary directory and linked against oracle/liboracle.so (orc_fast_atan2, orc_sincos_det,
orc_line_iterator_count)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import oracle_lib
from stvo_amd.capi import KEYLINE_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "fld_ref.c")
DIST_TH = 1.414213562
RANK_CAP = 8192  # segments per image the device ranks for the top-N cut (stvo_fld_counts tells about the rest)

u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")


class Statement:
    def __init__(self, lib):
        self.lib = lib
        lib.fld_edges.argtypes = [u8p, C.c_int, C.c_int, C.c_double, C.c_double, u8p]
        lib.fld_edges.restype = C.c_int
        lib.fld_segments.argtypes = [u8p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_double, C.c_double, f32p, C.c_int]
        lib.fld_segments.restype = C.c_int
        lib.fld_keylines.argtypes = [u8p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, f32p, C.POINTER(C.c_int)]
        lib.fld_keylines.restype = C.c_int
        lib.fld_atan2_det_n.argtypes = [f64p, f64p, f64p, C.c_int]
        lib.fld_atan2_det_n.restype = None
        lib.fld_walk_edges.argtypes = [u8p, C.c_int, C.c_int, i32p, C.c_int, i32p, C.c_int]
        lib.fld_walk_edges.restype = C.c_int

    def edges(self, img, th1=50.0, th2=50.0):
        img = np.ascontiguousarray(img, np.uint8)
        out = np.zeros(img.shape, np.uint8)
        rc = self.lib.fld_edges(img.reshape(-1), img.shape[1], img.shape[0], th1, th2, out.reshape(-1))
        if rc:
            raise ValueError("fld_edges: not stated")
        return out

    def segments(self, img, L, dist_th=DIST_TH, th=50.0):
        """FastLineDetector::detect: float32 [n, 4] in detection order."""
        img = np.ascontiguousarray(img, np.uint8)
        cap = 4096
        while True:
            seg = np.zeros((cap, 4), np.float32)
            n = self.lib.fld_segments(img.reshape(-1), img.shape[1], img.shape[0], int(L), dist_th, th, th, seg.reshape(-1), cap)
            if n < 0:
                raise ValueError(f"fld_segments: {n}")
            if n <= cap:
                return seg[:n].copy()
            cap = n

    def keylines(self, img, L, nfeatures=300, K=512, dist_th=DIST_TH, th=50.0):
        """(key-lines as KEYLINE_DTYPE records, responses float32, segments found)."""
        img = np.ascontiguousarray(img, np.uint8)
        rec = np.zeros(max(K, 1), KEYLINE_DTYPE)
        resp = np.zeros(max(K, 1), np.float32)
        nf = C.c_int(0)
        n = self.lib.fld_keylines(img.reshape(-1), img.shape[1], img.shape[0], int(L), dist_th, th, th, nfeatures, K, RANK_CAP,
                                  rec.ctypes.data_as(C.c_void_p), resp, C.byref(nf))
        if n < 0:
            raise ValueError(f"fld_keylines: {n}")
        return rec[:n].copy(), resp[:n].copy(), nf.value

    def atan2(self, y, x):
        y = np.ascontiguousarray(y, np.float64); x = np.ascontiguousarray(x, np.float64)
        out = np.empty_like(y)
        self.lib.fld_atan2_det_n(y, x, out, len(y))
        return out

    def walk(self, edges):
        """The chains of lineDetection's scan on a 0 / 255 edge map: list of int32 [n, 2] (x, y) point lists, short ones included."""
        e = np.ascontiguousarray(edges, np.uint8).copy()
        cap = int(np.count_nonzero(e))
        xy = np.zeros((max(cap, 1), 2), np.int32)
        lens = np.zeros(max(cap, 1), np.int32)
        n = self.lib.fld_walk_edges(e.reshape(-1), e.shape[1], e.shape[0], xy.reshape(-1), cap, lens, cap)
        out, o = [], 0
        for k in range(n):
            out.append(xy[o:o + lens[k]].copy())
            o += lens[k]
        return out


_cached = None


def load():
    global _cached
    if _cached is None:
        oracle_lib.load()  # builds oracle/liboracle.so when needed
        d = tempfile.mkdtemp(prefix="fld_ref_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libfld_ref.so")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC,
                               "-L" + oracle_lib.ORACLE_DIR, "-loracle", "-Wl,-rpath," + oracle_lib.ORACLE_DIR, "-lm"])
        _cached = Statement(C.CDLL(so))
    return _cached
