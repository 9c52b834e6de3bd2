"""Snapshots of single streams, the host-pure part (stvo-pl_amd/csrc/stream_snapshot.h and the planner's import fact in step_plan.h),
built with g++ alone through tests/cpp/snapshot_host.cpp: the blob layout, the header check of an import, a plain C++ pack -> unpack,
the chunk table of the kernels' launch, and what a step after an import gives up.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "stvo-pl_amd", "csrc")
DEPS = [os.path.join(CSRC, h) for h in ("stream_snapshot.h", "seq_layout.h", "step_plan.h", "debug_switches.h")] + \
    [os.path.join(HERE, "..", "include", h) for h in ("stvo_hip.h", "stvo_types.h")]
NSEC = 25
MOTION, TRAJ, TRAJ_KF, TRACKS, KF_SETS = 1, 2, 4, 8, 16
OK, INVALID, CAPACITY = 0, -1, -4   # include/stvo_types.h: STVO_OK, STVO_ERR_INVALID_ARG, STVO_ERR_CAPACITY
CAPS = [(64, 64), (128, 64), (512, 64), (2048, 512)]
NAMES = ("header", "rc", "desc", "spl", "epl", "sP", "eP", "le", "s2l", "s2lm", "ldesc", "motion", "traj", "tracks_p", "tracks_l") + \
    tuple("kf_" + n for n in ("rc", "desc", "spl", "epl", "sP", "eP", "le", "s2l", "s2lm", "ldesc"))


def legal(f):
    return (not f & TRAJ_KF or f & TRAJ) and (not f & KF_SETS or f & TRACKS)


FLAGS = [f for f in range(32) if legal(f)]


def _build(src, out, extra):
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS + [src, os.path.join(HERE, "cpp", "snapshot_host.cpp")]):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall"] + extra + ["-o", out, src])


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(HERE, "cpp", "libsnapshot_host.so")
    _build(os.path.join(HERE, "cpp", "snapshot_host.cpp"), so, ["-fPIC", "-shared"])
    L = C.CDLL(so)
    i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    L.snh_layout.argtypes = [C.c_int, C.c_int, C.c_int, i64p]
    L.snh_sections.argtypes = [i32p]
    L.snh_stereo_set_bytes.argtypes = [C.c_int, C.c_int]
    L.snh_stereo_set_bytes.restype = C.c_longlong
    L.snh_check.argtypes = [C.c_int] * 10
    L.snh_roundtrip.argtypes = [C.c_int] * 9 + [C.c_uint]
    L.snh_chunks.argtypes = [C.c_int, C.c_int, C.c_int, i64p]
    L.snh_plan.argtypes = [i32p, i64p, i32p]
    L.snh_plan.restype = None
    return L


def layout(lib, K, M, flags):
    out = np.zeros(NSEC + 1, np.int64)
    assert lib.snh_layout(K, M, flags, out) == NSEC + 1
    return dict(zip(NAMES, out[:NSEC].tolist())), int(out[NSEC])


def sections(lib):
    out = np.zeros(NSEC * 4, np.int32)
    assert lib.snh_sections(out) == NSEC
    return out.reshape(NSEC, 4)


def test_there_are_eighteen_legal_flag_sets(lib):
    assert len(FLAGS) == 18 and 0 in FLAGS and 31 in FLAGS
    out = np.zeros(NSEC + 1, np.int64)
    for f in range(-1, 40):
        assert (lib.snh_layout(64, 64, f, out) == NSEC + 1) == (f in FLAGS), f
    assert lib.snh_layout(0, 64, 0, out) == -1 and lib.snh_layout(64, 0, 0, out) == -1


@pytest.mark.parametrize("K,M", CAPS)
def test_layout(lib, K, M):
    """Every section 256-aligned, pairwise disjoint, in cutting order and inside `bytes`; the sections of a feature that is off are not
    cut; the sizes are the row sizes of seq_layout.h."""
    sec = sections(lib)
    cap = {0: 1, 1: K, 2: M}
    size = [int(rb) * cap[int(rows)] for rb, rows, _, _ in sec]
    for flags in FLAGS:
        off, total = layout(lib, K, M, flags)
        end = 0
        for i, name in enumerate(NAMES):
            present = sec[i][3] == 0 or bool(flags & sec[i][3])
            assert (off[name] >= 0) == present, (flags, name)
            if not present:
                continue
            assert off[name] % 256 == 0 and off[name] >= end, (flags, name, off[name], end)   # disjoint from everything cut before
            end = off[name] + size[i]
        assert end <= total and total % 256 == 0 and total - end < 256
        assert off["header"] == 0 and size[0] == 256
        # a stereo set is 48 K + 152 M bytes of rows (seq_layout.h cuts the same arrays, each rounded up to 256)
        assert sum(size[1:11]) == 48 * K + 152 * M == sum(size[15:25])
        assert off["motion" if flags & MOTION else "traj" if flags & TRAJ else "tracks_p" if flags & TRACKS else "rc"] >= 0
        set_span = off["ldesc"] + size[10] - off["rc"]
        assert (set_span + 255) // 256 * 256 == lib.snh_stereo_set_bytes(K, M)
        if flags & KF_SETS:
            assert total - off["kf_rc"] == lib.snh_stereo_set_bytes(K, M)
        assert size[11] == 128 and size[12] == 856 and size[13] == 8 * K and size[14] == 8 * M


def test_bytes_grow_with_capacity_and_features(lib):
    for flags in FLAGS:
        prev = 0
        for K, M in CAPS:   # non-decreasing in K and M (CAPS is ordered in both)
            total = layout(lib, K, M, flags)[1]
            assert total >= prev
            prev = total
    for K, M in CAPS:
        for f in FLAGS:
            for bit in (MOTION, TRAJ, TRAJ_KF, TRACKS, KF_SETS):
                if not f & bit and legal(f | bit):
                    assert layout(lib, K, M, f | bit)[1] >= layout(lib, K, M, f)[1], (K, M, f, bit)
    assert layout(lib, 2048, 512, 0)[1] == 256 + 176128
    assert layout(lib, 2048, 512, 31)[1] == 256 + 2 * 176128 + 256 + 1024 + 20480   # about 373 KB with everything on


def test_header_check_returns_the_code_of_the_table(lib):
    K, M, f = 512, 64, 31
    args = (K, M, f, 300, 40, 280, 33)
    assert lib.snh_check(*args, K, M, 0) == OK
    for what in range(1, 10):   # magic, version, bytes, flags, camera, image size, mp, op, a stride shorter than the blob
        assert lib.snh_check(*args, K, M, what) == INVALID, what
    # other capacities: fits a smaller and a larger pipeline, by the counts alone
    assert lib.snh_check(*args, 320, 64, 0) == OK and lib.snh_check(*args, 2048, 512, 0) == OK
    assert lib.snh_check(K, M, f, 300, 40, 280, 33, 256, 64, 0) == CAPACITY       # n
    assert lib.snh_check(K, M, f, 100, 40, 280, 33, 256, 64, 0) == CAPACITY       # hdr.n_pts
    assert lib.snh_check(2048, 512, f, 100, 65, 0, 0, 2048, 64, 0) == CAPACITY    # nl
    assert lib.snh_check(2048, 512, f, 100, 64, 0, 65, 2048, 64, 0) == CAPACITY   # hdr.n_lines
    assert lib.snh_check(2048, 512, f, 100, 64, 0, 64, 128, 64, 0) == OK          # every count exactly at the capacity
    assert lib.snh_check(K, M, 0, 300, 40, 0, 0, 256, 64, 0) == CAPACITY and lib.snh_check(K, M, 0, 256, 40, 0, 0, 256, 64, 0) == OK
    # a malformed header is malformed whatever the capacities say
    assert lib.snh_check(K, M, f, 300, 40, 280, 33, 256, 64, 1) == INVALID
    # counts no exporter writes
    assert lib.snh_check(K, M, f, K + 1, 40, 0, 0, 2048, 512, 0) == INVALID and lib.snh_check(K, M, f, -1, 40, 0, 0, 2048, 512, 0) == INVALID


@pytest.mark.parametrize("K,M", CAPS)
def test_pack_unpack_roundtrip(lib, K, M):
    """Random rows at n in {0, 1, K - 1, K} x nl in {0, 1, M}, every legal flag set: the rows come back, every other blob byte is zero,
    the target's other rows stay and its track rows beyond the counts are zero; into the same and into other capacities."""
    seed = 0
    for flags, n, nl in itertools.product(FLAGS, (0, 1, K - 1, K), (0, 1, M)):
        kf_n, kf_nl = (n * 7 + 3) % (K + 1), (nl * 5 + 1) % (M + 1)
        need = max(n, kf_n if flags & KF_SETS else 0)
        for Kt in {K, 2 * K, max(64, (need + 63) // 64 * 64)}:
            seed += 1
            assert lib.snh_roundtrip(K, M, flags, n, nl, kf_n, kf_nl, Kt, M, seed) == 0, (flags, n, nl, Kt)


def test_standalone_program_under_sanitizers():
    """tests/cpp/snapshot_host_main.cpp: the same pack / unpack on exact-size arrays under AddressSanitizer and UBSan, a program of its own."""
    src, exe = os.path.join(HERE, "cpp", "snapshot_host_main.cpp"), os.path.join(HERE, "cpp", "snapshot_host_main")
    _build(src, exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ", 0 failures" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-2000:])


@pytest.mark.parametrize("K,M", CAPS + [(4096, 512)])
def test_chunk_table_tiles_every_section(lib, K, M):
    out = np.zeros(2, np.int64)
    for flags in FLAGS:
        n = lib.snh_chunks(K, M, flags, out)
        assert 0 < n <= 96 and out[1] == 1 and out[0] >= 16384, (flags, n, out)


# ---- the planner's import fact

PLAN = ("par", "mid_fork", "fork_at_start", "line_forked", "cells_ahead", "lines_ahead", "gate", "s_pose_kernel", "s_pose_waves", "s_fused_cells",
        "s_cells_ahead", "s_lines_ahead", "s_gate", "s_mid_fork", "s_line_fused")


def plan(lib, B, frame_idx, hist, raw_split=0, st_dirty=1, has_control=0, after_import=0, cus=256):
    out = np.zeros(len(PLAN), np.int32)
    lib.snh_plan(np.array([B, cus, frame_idx, raw_split, st_dirty, has_control, after_import], np.int32), np.array(hist, np.int64), out)
    return dict(zip(PLAN, out.tolist()))


def test_step_after_an_import_waits_for_its_own_fork(lib):
    """A batch step that would run the grid and the key-line stage ahead gives both up after an import, exactly as a step with a control
    does, and still records and awaits its own fork event; a single-stream step loses the event-free fork.  Without an import: as before."""
    ahead = plan(lib, 1024, 5, (4, 4, 4))
    assert ahead["cells_ahead"] == 1 and ahead["lines_ahead"] == 1 and ahead["gate"] == 1 and ahead["mid_fork"] == 1
    imp = plan(lib, 1024, 5, (4, 4, 4), after_import=1)
    ctl = plan(lib, 1024, 5, (4, 4, 4), has_control=1)
    assert imp == ctl
    assert imp["cells_ahead"] == 0 and imp["lines_ahead"] == 0 and imp["gate"] == 0 and imp["mid_fork"] == 1 and imp["line_forked"] == 1
    assert {k: v for k, v in imp.items() if "ahead" not in k and "gate" not in k} == {k: v for k, v in ahead.items() if "ahead" not in k and "gate" not in k}
    # whatever the history says (a restored pipeline has none)
    for hist in ((-2, -2, -2), (4, 4, 4), (4, -2, 4), (0, 0, 0)):
        p = plan(lib, 1024, 1, hist, after_import=1)
        assert p["cells_ahead"] == 0 and p["lines_ahead"] == 0 and p["gate"] == 0 and p["line_forked"] == 1, hist
    # single stream: the upload split the key-line arrays onto the line stream and nothing is pending — no event without an import ...
    free = plan(lib, 1, 5, (-2, -2, 4), raw_split=1, st_dirty=0)
    assert free["fork_at_start"] == 0 and free["line_forked"] == 0 and free["par"] == 1
    # ... and one with it
    imp1 = plan(lib, 1, 5, (-2, -2, 4), raw_split=1, st_dirty=0, after_import=1)
    assert imp1["fork_at_start"] == 1 and imp1["line_forked"] == 1
    assert imp1 == plan(lib, 1, 5, (-2, -2, 4), raw_split=1, st_dirty=0, has_control=1)
