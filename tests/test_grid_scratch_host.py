"""The scratch of the stereo grid matchers (stvo-pl_amd/csrc/grid_scratch.h), run on the host: element counts, matrix dimensions and
the carve against a plain statement of the sizes (restated here in Python), every array 256-byte aligned and disjoint from the others,
misfit == ovf + B in one buffer — and the counts the C-ABI calls (run_grid) take to the context's arena against what they asked for
before the header existed."""
import subprocess

import pytest

import grid_scratch_host_lib as gsh
from grid_scratch_host_lib import ALL, ARRAYS, ELIG, ROWS

ELEM = dict(cover=8, top2=8, owner2=4, elig=4, elig_cnt=4, ovf=4)
GRID_ELIG = 16  # kernels of grid_kernels.hip: eligible pairs a right feature keeps


def up(n, m):
    return -(-n // m) * m


def plain_counts(B, rows1, rows2, bm, mf):
    """the plain statement: [B][words64][n1p] masks, [B][rows1] top-2 records, [B][rows2] owners, [B][16][rows2] eligible pairs and
    [B][rows2] counts of them, ovf[B] — with misfit[B] behind it where the one-workgroup point matcher may run"""
    words64, n1p = up(rows2, 64) // 64, up(rows1, 64)
    return dict(cover=B * words64 * n1p if bm else 0, top2=B * rows1, owner2=B * rows2, elig=B * GRID_ELIG * rows2, elig_cnt=B * rows2,
                ovf=2 * B if mf else B)


def plain_carve(B, rows1, rows2, bm, mf, order, lead=0):
    """offsets when the arrays are cut in `order`, each size rounded up to 256 bytes"""
    n = plain_counts(B, rows1, rows2, bm, mf)
    off, at = lead, {}
    for k in order:
        if k == "cover" and not bm:
            at[k] = -1
            continue
        at[k] = off
        off += up(n[k] * ELEM[k], 256)
    at["misfit"] = at["ovf"] + 4 * B if mf else -1
    return at, off


ROW_EDGES = [(64, 64), (128, 128), (2048, 2048), (2112, 2112), (64, 2112), (2112, 128), (1, 1), (1, 65), (65, 1)]
FLAGS = [(False, False), (False, True), (True, False), (True, True)]


def test_constants():
    assert gsh.elig_slots() == GRID_ELIG


@pytest.mark.parametrize("rows1,rows2", ROW_EDGES + [(1, 2048), (63, 64), (64, 65), (2047, 2049)], ids=lambda v: str(v))
def test_matrix_dims(rows1, rows2):
    words64, n1p, words = gsh.dims(rows1, rows2)
    assert words64 == -(-rows2 // 64) and n1p % 64 == 0 and rows1 <= n1p < rows1 + 64 and words == words64 * n1p


@pytest.mark.parametrize("B", [1, 3072])
@pytest.mark.parametrize("rows1,rows2", ROW_EDGES, ids=lambda v: str(v))
@pytest.mark.parametrize("bm,mf", FLAGS, ids=lambda v: str(int(v)))
def test_counts_and_carve_equal_the_plain_statement(B, rows1, rows2, bm, mf):
    assert gsh.counts(B, rows1, rows2, bm, mf) == plain_counts(B, rows1, rows2, bm, mf)
    assert gsh.route_words(B) == 2 * B
    for lead in (0, 256, 7 * 256):
        got, end = gsh.carve(B, rows1, rows2, bm, mf, ALL, lead)
        want, want_end = plain_carve(B, rows1, rows2, bm, mf, ARRAYS, lead)
        assert got == want and end == want_end
        # 256-byte alignment, disjointness, everything inside what the carver counts
        n = plain_counts(B, rows1, rows2, bm, mf)
        cut = sorted((got[k], n[k] * ELEM[k], k) for k in ARRAYS if got[k] >= 0)
        assert (got["cover"] >= 0) == bm and len(cut) == (6 if bm else 5)
        for o, size, k in cut:
            assert o % 256 == 0 and o >= lead and size > 0, k
        for (o, size, k), (o2, _, k2) in zip(cut, cut[1:]):
            assert o + size <= o2, (k, k2)
        assert cut[-1][0] + cut[-1][1] <= end
        # misfit == ovf + B, inside the one buffer the two share
        assert got["misfit"] == (got["ovf"] + 4 * B if mf else -1)
        if mf:
            assert got["misfit"] + 4 * B <= got["ovf"] + n["ovf"] * 4


@pytest.mark.parametrize("B,rows1,rows2", [(1, 64, 64), (3, 2112, 128), (3072, 128, 128)])
@pytest.mark.parametrize("bm,mf", FLAGS, ids=lambda v: str(int(v)))
def test_halves(B, rows1, rows2, bm, mf):
    """the two halves one after the other cut the same arrays as one carve does; a half leaves the other's pointers alone"""
    rows, elig = ("cover", "top2", "owner2"), ("elig", "elig_cnt", "ovf")
    assert gsh.carve(B, rows1, rows2, bm, mf, ROWS) == gsh.carve(B, rows1, rows2, bm, mf, ALL) == plain_carve(B, rows1, rows2, bm, mf, rows + elig)
    got = gsh.carve(B, rows1, rows2, bm, mf, ELIG, 512)
    assert -2 not in got[0].values() and got == plain_carve(B, rows1, rows2, bm, mf, elig + rows, 512)


@pytest.mark.parametrize("n1,n2", [(1, 1), (1, 65), (1, 2048), (300, 2048), (2048, 1)])
def test_run_grid_asks_for_what_it_asked(n1, n2):
    """stvo_match_grid_points / _lines (run_grid), one frame pair with the bit-matrix: words64 = ceil(n2 / 64), n1p = n1 rounded up to 64;
    cover n1p * words64 words, top2 n1, owner n2, elig 16 n2, elig_cnt n2, ovf 1 — the element counts of its arena_alloc calls"""
    words64, n1p = (n2 + 63) // 64, (n1 + 63) & ~63
    assert gsh.dims(n1, n2)[:2] == (words64, n1p)
    assert gsh.counts(1, n1, n2, True, False) == dict(cover=n1p * words64, top2=n1, owner2=n2, elig=GRID_ELIG * n2, elig_cnt=n2, ovf=1)


def test_pipeline_key_point_scratch_has_no_matrix():
    """stvo::seq_layout, headline shape (B 3072, K 1024): the key-points' carve cuts no bit-matrix — 402 653 184 bytes less than with one"""
    B, K = 3072, 1024
    with_bm, without = gsh.carve(B, K, K, True, True)[1], gsh.carve(B, K, K, False, True)[1]
    assert with_bm - without == B * (K // 64) * K * 8 == 402653184


def _run_program(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-g"] + gsh.FLAGS + extra + ["-DGRID_SCRATCH_HOST_MAIN", "-o", exe, gsh.SRC])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()
    assert p.returncode == 0, out + err
    assert out.count("arrays inside") == 48 and "INCONSISTENT" not in out and "48 shapes, 0 inconsistent" in out
    return err


def test_stand_alone_program_builds_and_runs(tmp_path):
    """the same source with its own main: the arrays cut from a real allocation of the size the carve states, every one written end to end"""
    _run_program(tmp_path, "grid_scratch_host_main", [])
