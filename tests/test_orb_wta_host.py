"""orb_wta_k 3 / 4 and orb_patch_size other than 31 on the CPU: the pattern generator of csrc/orb_pattern.h — as a stand-alone host
program (plain and under -fsanitize=address,undefined) and through stvo_orb_pattern — against the numpy statement tests/np_orb_wta.py;
the statement itself against what the project already trusts at (2, 31) and on constructed intensities; the planned cases' facts; the
Config keys.  No GPU.  tests/test_gpu_orb_wta.py compares the kernels with the same statement."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import np_orb
import np_orb_wta as nw
import orb_wta_cases as wc
from stvo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
CASES = {c["name"]: c for c in wc.all_cases()}
SETTINGS = [(k, P) for k in (2, 3, 4) for P in range(2, 64)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.load()


@pytest.fixture(scope="module")
def stand_in(lib):
    return capi.orb_pattern(2, 31)


def rc_of(fn):
    """The library's verdict of a call through capi (0: accepted)."""
    try:
        fn()
    except capi.StvoError as e:
        return int(re.search(r"\((-?\d+)\):", str(e)).group(1))
    return 0


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_pattern_program_equals_the_statement(tmp_path, flags):
    exe = str(tmp_path / "orb_pattern_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(HERE, "cpp", "orb_pattern_host_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [l.split() for l in run.stdout.splitlines()]
    pats = {(int(f[1]), int(f[2])): (int(f[3]), np.frombuffer(bytes.fromhex(f[4]), np.int8)) for f in lines if f[0] == "pattern"}
    assert sorted(pats) == sorted(SETTINGS) and len(pats) == 186
    pool31 = pats[(2, 31)][1].reshape(512, 2)
    for (k, P), (n, raw) in pats.items():
        ref = nw.effective_pattern(k, P, pool31)
        assert n == len(ref) == (512, 384, 512)[k - 2], (k, P)
        assert np.array_equal(raw[:2 * n].reshape(-1, 2), ref) and not raw[2 * n:].any(), (k, P)
    geo = {int(f[1]): [int(v) for v in f[2:]] for f in lines if f[0] == "geometry"}
    assert sorted(geo) == list(range(2, 64))
    for P, (h, R, *um) in geo.items():
        assert h == P // 2 and R == nw.reach(P) and um == nw.umax_table(h).tolist(), P
    assert geo[31][2:] == np_orb.umax_table().tolist()
    verdicts = {(int(f[1]), int(f[2])): (int(f[3]), int(f[4])) for f in lines if f[0] == "verdict"}
    assert len(verdicts) == 12 and all(untouched == 1 for _, untouched in verdicts.values())
    for (k, P), (v, _) in verdicts.items():
        assert v == (1 if (k not in (2, 3, 4) or P < 2) else 2), (k, P, v)      # 1: invalid, 2: unsupported (patch_size > 63)
    assert ["pool", "range", "1"] in lines
    for d, k in itertools.product((1, 2, 3, 4), (2, 3, 4)):
        assert ["pool", "distinct", str(d), str(k), "0" if (k == 2 or d >= k) else "1"] in lines


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "stvo_hip.h")).read()
    for name in ("stvo_orb_set_descriptor", "stvo_orb_pattern"):
        assert name in capi.EXPORTS and hasattr(lib, name) and f"int {name}(" in hdr, name


def test_library_pattern_equals_the_statement(lib, stand_in):
    assert stand_in.shape == (512, 2) and np.abs(stand_in).max() <= 13
    pool = wc.make_pool(5)
    for k, P in SETTINGS:
        got = capi.orb_pattern(k, P)
        assert got.dtype == np.int8 and np.array_equal(got, nw.effective_pattern(k, P, stand_in)), (k, P)
        if P in (21, 31):                                         # a caller's pool is read at patch size 31 and only there
            assert np.array_equal(capi.orb_pattern(k, P, pool), nw.effective_pattern(k, P, pool)), (k, P)
    assert np.array_equal(capi.orb_pattern(4, 21, pool), capi.orb_pattern(4, 21))


def test_library_verdicts(lib):
    for k, P, want in [(1, 31, -1), (5, 31, -1), (0, 2, -1), (-3, 31, -1), (2, 1, -1), (3, 0, -1), (4, -5, -1), (2, 64, -5), (3, 64, -5),
                       (4, 1 << 20, -5), (5, 64, -1), (1, 1, -1), (2, 2, 0), (4, 63, 0), (3, 31, 0)]:
        assert rc_of(lambda: capi.orb_pattern(k, P)) == want, (k, P)
    bad = np.zeros((256, 4), np.int8)
    bad[100, 2] = -14
    assert rc_of(lambda: capi.orb_pattern(2, 31, bad)) == -1
    assert rc_of(lambda: capi.orb_pattern(2, 27, bad)) == 0       # not read
    two = np.zeros((512, 2), np.int8)
    two[::2] = (3, -4)
    assert [rc_of(lambda: capi.orb_pattern(k, 31, two)) for k in (2, 3, 4)] == [0, -1, -1]
    two[5] = (1, 1)
    assert [rc_of(lambda: capi.orb_pattern(k, 31, two)) for k in (2, 3, 4)] == [0, 0, -1]
    # a refused call leaves the output alone
    out = np.full(1024, 77, np.int8)
    import ctypes as C
    n = C.c_int32(-9)
    assert lib.stvo_orb_pattern(3, 64, None, out, C.byref(n)) == -5 and n.value == -9 and np.all(out == 77)
    assert lib.stvo_orb_pattern(4, 31, two.ctypes.data, out, C.byref(n)) == -1 and n.value == -9 and np.all(out == 77)
    assert lib.stvo_orb_pattern(4, 31, None, out, None) == 0 and out.any()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_pattern_properties(k, stand_in):
    for P in range(2, 64):
        pts = nw.effective_pattern(k, P, stand_in)
        h = 13 if P == 31 else P // 2
        assert len(pts) == (512, 384, 512)[k - 2] and np.abs(pts).max() <= h, (k, P)
        if P != 31 and P >= 6:
            assert pts.min() == -h and pts.max() == h, (k, P)    # the range is used to its ends
        if k > 2:
            tup = pts.reshape(128, k, 2)
            for i, j in itertools.combinations(range(k), 2):
                assert not np.any((tup[:, i] == tup[:, j]).all(axis=1)), (k, P, i, j)
    # P = 2 and P = 3 share the half patch 1: nine different points at the most, and the draw of four different ones still ends
    assert np.array_equal(nw.effective_pattern(k, 2), nw.effective_pattern(k, 3))
    assert len({tuple(p) for p in nw.random_pool(2)}) == 9
    assert not np.array_equal(nw.random_pool(26), nw.random_pool(28))


def test_rng_is_the_multiply_with_carry_generator():
    r = nw.Rng(0)
    assert r.state == 0xFFFFFFFF
    r = nw.Rng(0x12345678)
    s = 0x12345678
    for _ in range(5):
        s = (s & 0xFFFFFFFF) * 4164903690 + (s >> 32)
        assert s < 1 << 64 and r.next() == s & 0xFFFFFFFF
    assert nw.Rng(7).uniform(5, 5) == 5 and all(-3 <= nw.Rng(i + 1).uniform(-3, 4) <= 3 for i in range(50))


def test_statement_at_2_31_is_the_trusted_one(oracle):
    """(2, 31) of the new statement = np_orb.detect_levels = oracle/stvo_orb_oracle.c, bit for bit, on the committed ORB goldens (and the
    goldens themselves), one level and four."""
    g = np.load(os.path.join(HERE, "golden", "orb_goldens.npz"))
    pat = oracle.orb_default_pattern().reshape(256, 4)
    assert np.array_equal(pat.reshape(512, 2), capi.orb_pattern(2, 31))
    for c, (seed, cols, rows, nf, th) in enumerate(g["cases"]):
        img = g[f"img_{c}"]
        for nlev in (1, 4) if c == 0 else (1,):
            a = nw.detect_levels(img, int(nf), nlev, 1.2, int(th), 19, pat, 4096, 2, 31)
            b = np_orb.detect_levels(img, int(nf), nlev, 1.2, int(th), 19, pat, 4096)
            o = oracle.orb_detect_levels(img, nfeatures=int(nf), nlevels=nlev, scale_factor=1.2, fast_th=int(th), edge_th=19, pattern=pat, cap=4096)
            for k in ("kp", "response", "angle", "desc", "octave"):
                assert a[k].shape == b[k].shape == o[k].shape, (c, nlev, k)
                assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) and np.array_equal(a[k].view(np.uint8), o[k].view(np.uint8)), (c, nlev, k)
            assert a["n_total"] == b["n_total"] and len(a["kp"]) > 50
            assert np.array_equal(a["trace"]["rot"].reshape(-1, 256, 4), b["trace"]["rot"])
            if nlev == 1:
                for k in ("kp", "response", "angle", "desc"):
                    assert np.array_equal(a[k], g[f"{k}_{c}"]), (c, k)


def test_wta3_every_branch_and_every_equality():
    """All 27 orderings of three values from {1, 2, 3} against the definition 'index of the first strict maximum as the ternary writes
    it': t2 > t1 ? (t2 > t0 ? 2 : 0) : (t1 > t0)."""
    t = np.array(list(itertools.product((1, 2, 3), repeat=3)), np.int64)
    got = nw.wta3_values(t[None])[0]
    for (t0, t1, t2), v in zip(t.tolist(), got.tolist()):
        want = (2 if t2 > t0 else 0) if t2 > t1 else int(t1 > t0)
        assert v == want, (t0, t1, t2)
    pick = {tuple(r): int(v) for r, v in zip(t.tolist(), got.tolist())}
    assert pick[(2, 2, 1)] == 0 and pick[(1, 2, 2)] == 1 and pick[(2, 1, 2)] == 0 and pick[(2, 2, 2)] == 0    # t0 = t1, t1 = t2, t0 = t2, all
    assert pick[(1, 1, 2)] == 2 and pick[(2, 1, 1)] == 0 and pick[(1, 2, 1)] == 1 and pick[(1, 2, 3)] == 2 and pick[(3, 2, 1)] == 0
    assert set(got.tolist()) == {0, 1, 2}
    d = nw.pack(np.array([[0, 1, 2, 0] + [0] * 124]), 2)
    assert d.shape == (1, 32) and d[0, 0] == 0b00100100 and not d[0, 1:].any()


def test_wta4_every_branch_and_every_equality():
    """All 256 orderings of four values from {1 .. 4} against the definition written as the reference's statements."""
    t = np.array(list(itertools.product((1, 2, 3, 4), repeat=4)), np.int64)
    got = nw.wta4_values(t[None])[0]
    for (t0, t1, t2, t3), v in zip(t.tolist(), got.tolist()):
        a, b = 0, 2
        if t1 > t0:
            t0, a = t1, 1
        if t3 > t2:
            t2, b = t3, 3
        assert v == (a if t0 > t2 else b)
    pick = {tuple(r): int(v) for r, v in zip(t.tolist(), got.tolist())}
    assert pick[(2, 2, 1, 1)] == 0 and pick[(1, 1, 2, 2)] == 2 and pick[(3, 3, 3, 3)] == 2            # pairs equal; all equal
    assert pick[(1, 3, 3, 2)] == 2 and pick[(1, 3, 2, 3)] == 3 and pick[(3, 1, 2, 3)] == 3            # t0' = t2' after the swaps: the second pair wins
    assert pick[(1, 4, 2, 3)] == 1 and pick[(4, 1, 3, 2)] == 0 and pick[(1, 2, 3, 4)] == 3 and pick[(1, 2, 4, 3)] == 2
    assert set(got.tolist()) == {0, 1, 2, 3}
    d = nw.pack(np.array([[3, 2, 1, 0, 1] + [0] * 123]), 2)
    assert d[0, 0] == 0b00011011 and d[0, 1] == 0b01 and not d[0, 2:].any()


def test_moments_for_any_half_patch_are_the_trusted_ones_at_15():
    img = np.random.default_rng(1).integers(0, 256, (80, 90)).astype(np.uint8)
    xy = np.array([[40, 40], [31, 33], [58, 48]])
    assert np.array_equal(nw.disc_mask(15), np_orb.disc_mask()) and nw.disc_mask(31).sum() > 2900 and nw.disc_mask(1).sum() == 5
    for a, b in zip(nw.moments(img, xy, 15), np_orb.moments(img, xy)):
        assert np.array_equal(a, b)
    # the farthest a rotated point gets, h sqrt 2, is never near a rounding tie: at least 0.01 from every half (h = 6: 8.485), where the
    # three float operations of a rotated coordinate err by less than 44 * 3 * 2^-24 < 1e-5 — so no point rounds beyond round(h sqrt 2)
    for h in range(1, 32):
        f = h * 2 ** 0.5 % 1
        assert abs(f - 0.5) > 0.01 and round(h * 2 ** 0.5) <= nw.reach(2 * h + 1 if h != 15 else 30), h


@pytest.mark.parametrize("name", list(CASES))
def test_case_sits_on_its_edge(name):
    c = CASES[name]
    c["facts"](c, wc.expected(c))


def test_refusals_follow_the_border_rule():
    assert set(wc.ENTRY_SUBSET) <= set(CASES)
    for k, P, e, code in wc.REFUSED:
        ok_k, ok_lo, ok_hi = k in (2, 3, 4), P >= 2, P <= 63
        if code == -5:
            assert ok_k and ok_lo and not ok_hi
        else:
            assert not ok_k or not ok_lo or (ok_hi and P != 31 and e < nw.reach(P)), (k, P, e)
    assert nw.reach(27) == 19 and nw.reach(28) == 20 and nw.reach(63) == 44 and nw.reach(41) == 29 and nw.reach(21) == 15 and nw.reach(31) == 19


def test_host_config_reads_the_descriptor_keys(tmp_path):
    host = os.path.join(ROOT, "stvo-pl_amd", "host")
    exe = str(tmp_path / "orb_wta_config_probe")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + host, "-o", exe, os.path.join(HERE, "cpp", "orb_wta_config_probe.cpp"),
                           os.path.join(host, "config.cpp")])
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("orb_nfeatures : 700\norb_wta_k : 4   # was set to 2\norb_patch_size : 27\n")
    out = subprocess.run([exe, str(cfg)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["default", "2", "31", "kitti", "2", "31", "euroc", "2", "31", "file", "4", "27"]
    cfg.write_text("orb_wta_k : 3\n")                               # a missing key keeps the current value
    out = subprocess.run([exe, str(cfg)], capture_output=True, text=True, check=True).stdout.split()
    assert out[-3:] == ["file", "3", "31"]
