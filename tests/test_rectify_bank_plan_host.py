"""The work split of the rectifier bank (stvo-pl_amd/csrc/rectify_bank_plan.h), run on the host through
tests/cpp/rectify_bank_plan_host.cpp: for every assignment below every (pair, side, quad) of every pair lies in exactly one item (an
item runs once per side, so the cover is checked per pair and quad), no item exists for a calibration without pairs, and the item count
stays within the bound the launch allocates for.  The same file as a stand-alone program plans into allocations of exactly the stated
sizes under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "rectify_bank_plan_host.cpp")
HDR = os.path.join(HERE, "..", "stvo-pl_amd", "csrc", "rectify_bank_plan.h")
FLAGS = ["-std=c++17", "-Wall", "-Wextra"]  # no HIP include path: the header is host-pure

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "cpp", "librectify_bank_plan_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1"] + FLAGS + ["-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    for name in ("rbp_max_items", "rbp_items_offset", "rbp_table_bytes"):
        getattr(lib, name).restype = C.c_longlong
    lib.rbp_max_items.argtypes = [C.c_int] * 4
    lib.rbp_items_offset.argtypes = [C.c_int]
    lib.rbp_table_bytes.argtypes = [C.c_int, C.c_longlong]
    lib.rbp_nquads.argtypes = [C.c_int, C.c_int]
    lib.rbp_plan.argtypes = [C.c_int, C.c_int, i32p, i32p, i32p, i32p, i32p, C.c_longlong]
    _lib = lib
    return lib


def plan(B, sizes, assign, slot):
    """-> (pairs [B], items [n, 4] = calib, qblock, pair_begin, pair_count, the bound)"""
    lib = load()
    K = len(sizes)
    bound = lib.rbp_max_items(B, K, slot[0], slot[1])
    pairs = np.full(B, -1, np.int32)
    items = np.full((bound + 1, 4), -7, np.int32)   # one row more than the bound: it must stay untouched
    cols = np.array([s[0] for s in sizes], np.int32)
    rows = np.array([s[1] for s in sizes], np.int32)
    n = lib.rbp_plan(B, K, np.asarray(assign, np.int32), cols, rows, pairs, items, bound)
    assert 0 < n <= bound, (n, bound)
    assert (items[n:] == -7).all()
    return pairs, items[:n].copy(), bound


def check_cover(B, sizes, assign, slot):
    lib = load()
    block = lib.rbp_block()
    pairs, items, bound = plan(B, sizes, assign, slot)
    assert sorted(pairs.tolist()) == list(range(B))                     # the pair list is a permutation of the pairs
    seen = [np.zeros(lib.rbp_nquads(*sizes[assign[b]]), np.int64) for b in range(B)]
    for k, qb, p0, cnt in items.tolist():
        assert 0 <= k < len(sizes) and cnt >= 1 and 0 <= p0 and p0 + cnt <= B
        nq = lib.rbp_nquads(*sizes[k])
        assert qb * block < nq                                            # no workgroup without a quad
        for b in pairs[p0:p0 + cnt].tolist():
            assert assign[b] == k                                         # a pair is walked under its own calibration only
            seen[b][qb * block:min(nq, (qb + 1) * block)] += 1
    for b in range(B):
        assert (seen[b] == 1).all(), (b, assign[b])                       # every quad of every pair exactly once (per side)
    assert set(items[:, 0].tolist()) == set(assign)                       # no item for a calibration without pairs
    return len(items), bound


SLOT = (53, 21)
SIZES = [(53, 21), (50, 19), (7, 5), (3, 2), (1, 1), (40, 16)]


@pytest.mark.parametrize("assign", [[0, 1, 1, 2, 3, 4, 5], [0, 1, 1, 2, 3, 4, 4], [0] * 7, [4] * 7, [5, 4, 3, 2, 1, 0, 0], [1, 1, 1]],
                         ids=["mixed", "one_left_out", "all_on_the_slot", "all_on_1x1", "reversed", "three_pairs"])
def test_small_bank(assign):
    check_cover(len(assign), SIZES, assign, SLOT)


def test_one_pair_each_and_k_1():
    check_cover(6, SIZES, list(range(6)), SLOT)
    check_cover(1, [(1, 1)], [0], (1, 1))
    check_cover(5, [(53, 21)], [0] * 5, SLOT)
    check_cover(3, [(1, 1)], [0] * 3, SLOT)


def test_benchmark_shape_and_chunks():
    """256 pairs over three dataset sizes in slots of 1242 x 480: several quad blocks and several chunks per calibration, and a
    calibration's chunks hold at least 4 pairs where it has them"""
    sizes = [(1241, 376), (1242, 375), (752, 480)]
    assign = [b % 3 for b in range(256)]
    n, bound = check_cover(256, sizes, assign, (1242, 480))
    assert n <= bound
    _, items, _ = plan(256, sizes, assign, (1242, 480))
    assert items[:, 3].min() >= 4
    # all on one calibration, and a calibration with a single pair beside a crowded one
    check_cover(256, sizes, [2] * 256, (1242, 480))
    check_cover(256, sizes, [0] * 255 + [1], (1242, 480))


def test_sizes_from_1x1_to_the_slot_stay_within_the_bound():
    rng = np.random.default_rng(11)
    for _ in range(40):
        B = int(rng.integers(1, 20))
        K = int(rng.integers(1, 6))
        slot = (int(rng.integers(1, 700)), int(rng.integers(1, 40)))
        sizes = [(int(rng.integers(1, slot[0] + 1)), int(rng.integers(1, slot[1] + 1))) for _ in range(K)]
        sizes[int(rng.integers(0, K))] = slot
        assign = rng.integers(0, K, B).tolist()
        check_cover(B, sizes, assign, slot)


def test_table_layout():
    lib = load()
    for B in (1, 3, 4, 5, 256):
        off = lib.rbp_items_offset(B)
        assert off % 16 == 0 and 4 * B <= off < 4 * B + 16
        assert lib.rbp_table_bytes(B, 10) == off + 160


def test_a_table_too_small_is_reported():
    lib = load()
    pairs = np.zeros(7, np.int32)
    items = np.full((2, 4), -7, np.int32)
    cols = np.array([s[0] for s in SIZES], np.int32)
    rows = np.array([s[1] for s in SIZES], np.int32)
    assert lib.rbp_plan(7, 6, np.array([0, 1, 1, 2, 3, 4, 5], np.int32), cols, rows, pairs, items, 1) == -1
    assert (items[1] == -7).all()


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rectify_bank_plan_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DRECTIFY_BANK_PLAN_HOST_MAIN"] + FLAGS +
                          ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 inconsistent" in out.stdout
