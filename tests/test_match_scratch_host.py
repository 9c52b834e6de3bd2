"""The scratch of the descriptor matcher (stvo-pl_amd/csrc/match_scratch.h), run on the host: every view against the arithmetic the
launch code of the parent commit d9a1982 carried (restated here in Python, the tsel expression literally), the views one path uses at
the same time disjoint and inside their arrays, the capacity predicate against the parent's two ABI checks — and block_threshold
against its definition."""
import subprocess

import numpy as np
import pytest

import match_scratch_host_lib as msh

UINT2, INT32 = 8, 4


def ctx_capacity(max_rows, max_batch):
    """stvo_ctx_create: elements of knn12 / knn21"""
    return max_rows * max(2 * max_batch, 16)


def parent_views(B, row_stride, cap):
    """(array, byte offset) of what the parent's launch code handed its kernels"""
    per = B * row_stride
    v = {"knn12_seg0": ("knn12", 0), "knn12_seg1": ("knn12", per * UINT2),  # out = knn12 + seg * B * row_stride (+ frame_off)
         "claim": ("claim", 0),                                             # reinterpret_cast<uint32_t*>(w.need)
         "cand": ("cand", 0), "qsel": ("qsel", 0),
         "blocked": ("knn21", 0),                                           # reinterpret_cast<int32_t*>(w.knn21)
         # reinterpret_cast<int32_t*>(w.knn21 + (w.knn_capacity - per)) + per
         "tsel": ("knn21", (cap - per) * UINT2 + per * INT32)}
    for k in range(5):
        v["nsel%d" % k] = ("nsel", k * B * INT32)                           # nsel[k * (size_t)B + b]
    return v, per


def parent_refuses(B, row_stride, cap):
    """stvo_match_nnr_mutual_batched_dev and check_batch: (size_t)2 * B * row_stride > ctx->knn_capacity"""
    return 2 * B * row_stride > cap


def parent_pick_nseg(B, max_n, cap):
    tiles = (max_n + 255) // 256
    nseg = (2048 + B * tiles - 1) // (B * tiles if B * tiles > 0 else 1)
    nseg = min(max(nseg, 2), 16)
    if B * tiles >= 4096:
        nseg = 1
    per_seg = max(B, 1) * max(max_n, 1)
    while nseg > 1 and nseg * per_seg > cap:
        nseg -= 1
    return nseg


def check_disjoint_inside(spans, sizes):
    """spans: (array, offset, bytes, name); pairwise disjoint within an array, each inside it"""
    for arr, off, n, name in spans:
        assert 0 <= off and off + n <= sizes[arr], (name, arr, off, n, sizes[arr])
    by = sorted(spans)
    for (a, o, n, k), (a2, o2, _, k2) in zip(by, by[1:]):
        assert a != a2 or o + n <= o2, (k, k2)


def check_case(B, row_stride, cap, rows_cap, batch_cap):
    """cap: elements of knn12 / knn21; rows_cap: entries of cand / claim / qsel; batch_cap: rows of nsel hold this many frames"""
    assert msh.fits(B, row_stride, cap) and not parent_refuses(B, row_stride, cap)
    got, per = msh.views(B, row_stride, cap)
    want, want_per = parent_views(B, row_stride, cap)
    assert per == want_per
    assert got == want
    # tsel is the LAST per int32 of knn21, blocked its first
    assert got["tsel"][1] + per * INT32 == cap * UINT2 and got["blocked"][1] == 0
    sizes = dict(knn12=cap * UINT2, knn21=cap * UINT2, cand=rows_cap * INT32, claim=rows_cap * INT32, qsel=rows_cap * INT32,
                 nsel=batch_cap * 5 * INT32)
    picked = msh.pick_nseg(B, row_stride, cap)
    assert picked == parent_pick_nseg(B, row_stride, cap)
    lo, hi = msh.nseg_limits()
    most = min(hi, cap // per)  # nseg at its cap: as many segments as the arrays hold
    assert 1 <= picked <= most
    for nseg in (picked, most):
        seg = [("knn12", got["knn12_seg0"][1] + s * (got["knn12_seg1"][1] - got["knn12_seg0"][1]), per * UINT2, "knn12[%d]" % s) for s in range(nseg)]
        row = lambda k: got[k] + (per * INT32, k)
        nsel = lambda ks: [got["nsel%d" % k] + (B * INT32, "nsel%d" % k) for k in ks]
        # LAZY on the matrix cores: forward top-2, claims, column lists, the five counters, the row list S
        check_disjoint_inside(seg + [row("claim"), row("qsel"), row("tsel")] + nsel(range(5)), sizes)
        # LAZY on the VALU kernels: forward top-2, candidates, claims, the column list and its counter, the verdicts
        check_disjoint_inside(seg + [row("cand"), row("claim"), row("qsel"), row("blocked")] + nsel([0]), sizes)
        # BOTH_DIRS: knn21 holds the reverse top-2, segment for segment
        check_disjoint_inside(seg + [("knn21", s * per * UINT2, per * UINT2, "knn21[%d]" % s) for s in range(nseg)], sizes)
    # no launch uses blocked and tsel together, but a problem that fits keeps them apart all the same
    check_disjoint_inside([row("blocked"), row("tsel")], sizes)


CTX_CASES = [(1, 1), (1, 2), (1, 8192), (1, 8193), (1, 65535), (9, 33), (64, 4096)]


@pytest.mark.parametrize("B,row_stride", CTX_CASES, ids=lambda v: str(v))
def test_views_equal_parent_context_scratch(B, row_stride):
    """a context created for exactly this problem: max_rows = row_stride, max_batch = B"""
    check_case(B, row_stride, ctx_capacity(row_stride, B), B * row_stride, B)


def test_exact_fit_and_one_frame_more():
    cap = ctx_capacity(4096, 64)
    assert 2 * 64 * 4096 == cap
    assert msh.fits(64, 4096, cap)
    assert not msh.fits(65, 4096, cap) and parent_refuses(65, 4096, cap)


@pytest.mark.parametrize("B", [1, 64, 1024])
@pytest.mark.parametrize("M", [64, 128, 512])
def test_views_equal_parent_pipeline_keyline_scratch(B, M):
    """stvo::seq_layout: knn_capacity = 4 B M, per-row arrays of B M entries, nsel of 5 B"""
    check_case(B, M, 4 * B * M, B * M, B)


@pytest.mark.parametrize("B,row_stride", CTX_CASES + [(65, 4096), (1024, 512), (3072, 1024)], ids=lambda v: str(v))
def test_predicate_agrees_with_parent_checks(B, row_stride):
    per = B * row_stride
    for cap in (0, per, 2 * per - 1, 2 * per, 2 * per + 1, ctx_capacity(row_stride, B), ctx_capacity(4096, 64), 4 * per):
        assert msh.fits(B, row_stride, cap) == (not parent_refuses(B, row_stride, cap)), cap


def f32(x):
    return np.float32(x)


NNRS = [f32(0.5), f32(0.75), f32(0.9), f32(1.0), np.nextafter(f32(0.75), f32(0)), np.nextafter(f32(0.75), f32(1))]


@pytest.mark.parametrize("nnr", NNRS, ids=lambda v: "%.9g" % v)
def test_block_threshold_is_its_definition(nnr):
    """the largest d' in [d0, 256] for which float(d0) < float(d') * nnr is false"""
    dp = np.arange(257, dtype=np.float32)
    prod = (dp * nnr).astype(np.float32)  # float32 products, as the kernels form them
    for d0 in range(257):
        false_at = [d for d in range(d0, 257) if not (f32(d0) < prod[d])]
        assert false_at and false_at[0] == d0  # nnr <= 1: a row never passes the test against its own distance
        assert msh.block_threshold(d0, nnr) == max(false_at), d0


def _run_program(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-g"] + msh.FLAGS + extra + ["-DMATCH_SCRATCH_HOST_MAIN", "-o", exe, msh.SRC])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()
    assert p.returncode == 0, out + err
    assert out.count("views inside") == 16 and "INCONSISTENT" not in out and "16 shapes" in out and ", 0 inconsistent" in out
    return err


def test_stand_alone_program_builds_and_runs(tmp_path):
    """the same source with its own main: the arrays allocated for real, every view written end to end"""
    _run_program(tmp_path, "match_scratch_host_main", [])


def test_stand_alone_program_under_sanitizers(tmp_path):
    """... and with AddressSanitizer + UndefinedBehaviorSanitizer: a view that left its array would be a finding"""
    err = _run_program(tmp_path, "match_scratch_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "ERROR" not in err and "runtime error" not in err, err
