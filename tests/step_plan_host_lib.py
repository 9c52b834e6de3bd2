"""Builds and binds tests/cpp/step_plan_host.cpp (the product's step_plan.h compiled for the host) — TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UNSET = -2 ** 31   # debug_switches.h: DBG_UNSET

FACTS = ("B", "K", "M", "cus", "has_points", "has_lines", "best_lr_matches", "lines_now", "lines_prev", "track", "frame_idx", "raw_split",
         "raw_max_lines", "set_lines_cap_prev", "set_lines_cap_cur", "st_dirty", "fetch", "zero_copy", "timing", "timing_events",
         "has_alt_m12l", "cells_differ", "grid_points_fused_ok", "match_small_ok_K", "match_small_ok_M", "pose_inline_sync_ok",
         "pose_batch_kernel_selected", "pose_start_flag_ok", "pose2p_waves_per_pair")
SWITCHES = ("pose_kernel", "seq_inline", "line_fused", "match_small", "match_lazy", "grid_tail", "cells_ahead", "lines_ahead", "grid_cells")
HISTORY = ("fork_rec_frame", "pose_flag_frame", "sl_forked_frame")
SCHEDULE = ("pose_kernel", "pose_waves", "fused_cells", "cells_ahead", "lines_ahead", "gate", "mid_fork", "line_fused")   # include/stvo_hip.h: STVO_SCHED_*
PLAN = ("light", "par", "mid_fork", "fork_at_start", "line_forked", "zero_nl", "point_stage", "line_stage", "clear_nl", "lean_cells", "has_tail",
        "fused_cells", "cells_ahead", "lines_ahead", "gate", "Mk", "line_lds", "line_fused", "points_route", "points_small_cap", "points_nseg_cap",
        "lines_route", "lines_small_cap", "lines_nseg_cap", "track", "match_lines_run", "clear_m12l", "use_alt_m12l", "inline_sync",
        "fetch_by_pose", "inl_zero_copy", "lazy_eig", "pose_flagged", "join_signal", "fetch_copy", "inl_copy") + \
    tuple("sched_" + k for k in SCHEDULE) + ("lds_asked", "lds_asked_bytes")
SMALL, BOTH_DIRS, LAZY, ONE_WAY = 0, 1, 2, 3   # step_plan.h: MatchRoute

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(HERE, "cpp", "step_plan_host.cpp")
    so = os.path.join(HERE, "cpp", "libstep_plan_host.so")
    csrc = os.path.join(HERE, "..", "stvo-pl_amd", "csrc")
    deps = [src, os.path.join(csrc, "step_plan.h"), os.path.join(csrc, "debug_switches.h"), os.path.join(HERE, "..", "include", "stvo_hip.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    lib.sph_plan.argtypes = [i32p, i32p, np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"), C.c_int, C.c_int, i32p]
    lib.sph_plan.restype = None
    _lib = lib
    return lib


def plan(facts, switches=None, history=(-2, -2, -2), lds_fits=True, commit=False):
    """plan_step on `facts` (dict over FACTS), `switches` (dict over SWITCHES, the others unset) and `history` (HISTORY order) ->
    (dict over PLAN, history after commit() if `commit` else as given)."""
    lib = load()
    assert set(facts) == set(FACTS), set(facts) ^ set(FACTS)
    assert not set(switches or {}) - set(SWITCHES)
    f = np.array([int(facts[k]) for k in FACTS], np.int32)
    s = np.array([int((switches or {}).get(k, UNSET)) for k in SWITCHES], np.int32)
    h = np.array(history, np.int64)
    out = np.zeros(len(PLAN), np.int32)
    lib.sph_plan(f, s, h, 1 if lds_fits else 0, 1 if commit else 0, out)
    return dict(zip(PLAN, (int(v) for v in out))), tuple(int(v) for v in h)
