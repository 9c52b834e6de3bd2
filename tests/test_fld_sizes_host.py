"""What one image means to the FLD kernels under a detector's parameters (stvo-pl_amd/csrc/fld_sizes.h), run on the host as a program
of its own (tests/cpp/fld_sizes_host.cpp), plain and under -fsanitize=address,undefined: the rows stvo_fld_set_image_sizes writes into
its device table against fld_words / fld_units / fld_store_cap restated here, their monotonicity over every size the GPU test's slot
holds, every refusal, and the store rule at its edge.  No GPU."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "fld_sizes_host.cpp")
FLAG_SETS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
SLOT = (160, 120)
CROPS = [(16, 16), (33, 47), (64, 64), (65, 63), (97, 120), (160, 61), (47, 118), (160, 120), (159, 119), (96, 43)]   # tests/test_gpu_fld_sizes.py
KITTI_SIZES = [(1241, 376), (1242, 375), (1226, 370)]

_programs = {}


# frontend_layout.h, restated
def words(npx):
    return (npx + 63) // 64 * 2


def units(npx):
    return (npx + 4095) // 4096


def store_cap(npx, L):
    return npx // (L + 1) + 1


@pytest.fixture(scope="module", params=sorted(FLAG_SETS))
def ask(request, tmp_path_factory):
    """ask(lines) -> the program's answer lines; the program built once per flag set"""
    kind = request.param
    if kind not in _programs:
        exe = str(tmp_path_factory.mktemp("fld_sizes_" + kind) / "fld_sizes_host")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + FLAG_SETS[kind] + ["-o", exe, SRC])
        _programs[kind] = exe

    def run(lines):
        out = subprocess.run([_programs[kind]], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        answers = out.stdout.split("\n")
        assert answers[-2:] == ["end", ""], answers[-3:]
        return [a.split() for a in answers[:-2]]
    return run


def verdict(ask, entries, B, slot=SLOT, L_det=6, n=None):
    """(verdict, entry, need, have) for a list of (cols, rows) or (cols, rows, L)"""
    own = 1 if entries and len(entries[0]) == 3 else 0
    n = len(entries) if n is None else n
    line = "ok %d %d %d %d %d %d " % (slot[0], slot[1], L_det, B, n, own) + " ".join(" ".join(str(v) for v in e) for e in entries[:max(n, 0)])
    (a,) = ask([line])
    assert a[0] == "ok" and (a[1] == "0") == (a[5] == "1")     # fld_image_sizes_ok is the verdict "taken"
    return tuple(int(v) for v in a[1:5])


def test_rows_against_the_layout_functions(ask):
    sizes = CROPS + KITTI_SIZES + [(1024, 1024)]
    got = ask(["row %d %d %d" % (c, r, 1 + i % 7) for i, (c, r) in enumerate(sizes)])
    assert len(got) == len(sizes)
    for i, ((c, r), a) in enumerate(zip(sizes, got)):
        L = 1 + i % 7
        assert [int(v) for v in a[1:]] == [c, r, c * r, words(c * r), units(c * r), L, 32], (c, r)
    # a row the kernels read as 32 bytes; 64 x 64 is exactly one unit of the counting sort, 65 x 63 one pixel less: a partial last word
    by = {(int(a[1]), int(a[2])): a for a in got}
    assert by[(64, 64)][4:6] == ["128", "1"] and by[(65, 63)][3:6] == ["4095", "128", "1"] and by[(97, 120)][5] == "3"


def test_words_units_and_stores_are_monotone_over_every_size_of_the_slot(ask):
    """an image that fits its slot on both sides never has more pixels, edge words or sort units than the slot — nor, at a threshold no
    smaller than the detector's, a larger store: what lets the kernels keep the slot's blocks"""
    got = ask(["grid 16 %d 16 %d 6" % SLOT])
    assert len(got) == (SLOT[0] - 15) * (SLOT[1] - 15)
    tab = {(int(a[1]), int(a[2])): tuple(int(v) for v in a[3:6]) for a in got}
    for (c, r), (npx, nw, nu) in tab.items():
        assert (npx, nw, nu) == (c * r, words(c * r), units(c * r))
        for nb in ((c + 1, r), (c, r + 1)):
            if nb in tab:
                assert all(x <= y for x, y in zip(tab[(c, r)], tab[nb])), ((c, r), nb)
        assert nw * 32 >= npx and store_cap(npx, 6) <= store_cap(SLOT[0] * SLOT[1], 6)
    slot = tab[SLOT]
    assert all(all(x <= y for x, y in zip(v, slot)) for v in tab.values())
    assert all(store_cap(n, L + 1) <= store_cap(n, L) for n in (256, 4095, 19200) for L in range(1, 40))


def test_every_refusal(ask):
    INVALID, CAPACITY = 1, 2
    assert verdict(ask, CROPS, 10)[0] == 0 and verdict(ask, CROPS[:5], 10)[0] == 0 and verdict(ask, [(159, 119)], 3)[0] == 0
    assert verdict(ask, [(16, 16)], 2)[0] == 0
    assert verdict(ask, [(160, 120)] * 3, 10)[0] == INVALID                                       # B % n != 0
    assert verdict(ask, [(160, 120)] * 11, 10)[0] == INVALID                                      # n > B
    assert verdict(ask, [(160, 120)], 10, n=0)[0] == INVALID and verdict(ask, [(160, 120)], 10, n=-1)[0] == INVALID
    assert verdict(ask, [(161, 120)], 10)[0] == INVALID and verdict(ask, [(160, 121)], 10)[0] == INVALID    # larger than the slot
    assert verdict(ask, [(15, 64)], 10)[0] == INVALID and verdict(ask, [(64, 15)], 10)[0] == INVALID        # below what stvo_fld_create takes
    assert verdict(ask, [(64, 64, 0)], 10)[0] == INVALID and verdict(ask, [(64, 64, -3)], 10)[0] == INVALID  # L_i < 1
    assert verdict(ask, [(64, 64, 6), (64, 64, 0)], 10)[0] == INVALID
    # a bad shape or size is reported before any entry's store: the later entry is invalid, the earlier one only too large for the stores
    assert verdict(ask, [(159, 119, 5), (15, 64, 6)], 10)[0] == INVALID
    assert verdict(ask, [(159, 119, 5), (64, 64, 6)], 10)[:2] == (CAPACITY, 0)
    assert verdict(ask, [(64, 64, 6), (159, 119, 5)], 10)[:2] == (CAPACITY, 1)


def test_the_store_rule_at_its_edge(ask):
    """slot 160 x 120 at the detector's L = 6: 19200 / 7 + 1 = 2743 slots"""
    assert store_cap(160 * 120, 6) == 2743 and store_cap(159 * 119, 5) == 3154 and store_cap(97 * 120, 4) == 2329
    assert verdict(ask, [(159, 119, 5)], 2) == (2, 0, 3154, 2743)
    assert verdict(ask, [(97, 120, 4)], 2)[0] == 0
    assert verdict(ask, [(160, 120, 6)], 2)[0] == 0                       # equality
    assert verdict(ask, [(160, 120, 5)], 2) == (2, 0, 3201, 2743)
    # no list of thresholds: every entry keeps the detector's, which always fits
    assert verdict(ask, [(160, 120), (159, 119)], 2)[0] == 0
    # L_i >= L_det is sufficient at every size of the slot; the rule itself is what is checked, so a smaller image may take a smaller one
    assert all(verdict(ask, [(c, r, L)], 2)[0] == 0 for c, r in CROPS for L in (6, 7, 40))
    assert verdict(ask, [(64, 64, 1)], 2)[0] == 0 and store_cap(4096, 1) == 2049
    # the thresholds of tests/test_gpu_fld_sizes.py under a detector created at 1
    entries = [(c, r, max(1, int(0.05 * min(c, r)))) for c, r in CROPS]
    assert sorted({e[2] for e in entries}) == [1, 2, 3, 4, 5, 6]
    assert verdict(ask, entries, 10, L_det=1)[0] == 0 and verdict(ask, entries, 10, L_det=2)[0] == 0
    assert verdict(ask, entries, 10, L_det=6)[0] == 2


def test_header_declares_and_library_exports_the_new_symbol():
    from stvo_amd import capi
    hdr = open(os.path.join(ROOT, "include", "stvo_hip.h")).read()
    assert re.search(r"#define\s+STVO_ABI_VERSION\s+3\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    lib = capi.load()
    assert re.search(r"\bstvo_fld_set_image_sizes\s*\(", hdr)
    assert "stvo_fld_set_image_sizes" in capi.EXPORTS and hasattr(lib, "stvo_fld_set_image_sizes")
    assert hasattr(capi.Fld, "set_image_sizes")
