"""The stereo point matcher of the device pipeline at its edges: grid_points_fused_kernel (grid_kernels.hip; one workgroup per frame,
with point_cells.h in front) and the scan formulation that takes its place for a frame that does not fit, by switch, and by capacity.
The case frames are those of tests/point_match_cases.py, which tests/test_point_match_host.py has shown to be fair and to hit their
edges on the CPU.  Every comparison is exact integer equality of raw match indices — fetch_matches()[0] of the FIRST step, the frames
of a set side by side as streams — with the oracle, with the traced plain statement and with the plan; there is no tolerance here.
The candidates are recomputed from the device's own window gather (debug_grid) and the route every frame took is read from the
device (debug_point_route): the plan's restatement of the capacity rule is judged by them, not trusted."""
import numpy as np
import pytest

import np_model
import point_match_cases as cases
from stvo_amd.ctypes_types import opt_params

pytestmark = pytest.mark.gpu

SETS = [cs["name"] for cs in cases.point_sets()]
# what the plan is after, in words of the device: frame -> (misfit on the one-workgroup route, ovf where the scan formulation runs)
PLANNED = {"P4 narrow right key-points": (0, 0), "P4 wide right key-points": (0, 0), "P4 chains of 17": (0, 1),
           "P5 256 right key-points with 17 candidates": (0, 0), "P5 257 right key-points with 17 candidates": (1, 0),
           "P5 64 right key-points share 128 candidates": (0, 0), "P5 64 right key-points share 129 candidates": (1, 0),
           f"P5 narrow right key-points, {cases.SMALL_CAP} eligible pairs beyond four": (0, 0),
           f"P5 narrow right key-points, {cases.SMALL_CAP + 1} eligible pairs beyond four": (0, 0)}
# ... with STVO_GRID_FUSED_CAP = SMALL_CAP / TINY_CAP: the frame whose narrow eligible pairs sum to the cap fits, one more does not
PLANNED_CAPPED = {f"P5 narrow right key-points, {cases.SMALL_CAP} eligible pairs beyond four": 0,
                  f"P5 narrow right key-points, {cases.SMALL_CAP + 1} eligible pairs beyond four": 1,
                  f"P5 narrow right key-points, {cases.TINY_CAP} eligible pairs beyond four": 0,
                  f"P5 narrow right key-points, {cases.TINY_CAP + 1} eligible pairs beyond four": 1}
FUSED, ALL_MISFIT, SCAN = "one workgroup per frame", "every frame misfits", "scan formulation"


def planned_route(cf, t, mp, route, cap):
    """(misfit, ovf) the device must report for this frame"""
    if route == SCAN:
        misfit = 0
    elif route == ALL_MISFIT:
        misfit = 1
    else:
        misfit = cases.planned_misfit(t, cap)
        if cap is None and cf["name"] in PLANNED:
            assert misfit == PLANNED[cf["name"]][0], cf["name"]
        if cap is not None and cf["name"] in PLANNED_CAPPED:
            assert misfit == PLANNED_CAPPED[cf["name"]], cf["name"]
    ovf = cases.planned_ovf(t, mp)
    if cf["name"] in PLANNED:
        assert ovf == PLANNED[cf["name"]][1], cf["name"]
    return misfit, ovf if (misfit or route == SCAN) else 0


def check_stream(dev, b, cf, res, ms_p, counts, where, grid):
    ref, mdl, t, tail = res
    f = cf["frame"]
    n_l = len(f["kp_l"])
    got = ms_p[b, :n_l]
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, (where, "left rows", bad[:8], "device", got[bad[:8]], "oracle", ref[bad[:8]],
                           "(best, second)", [(int(t["best"][i]), int(t["second"][i])) for i in bad[:8]])
    assert np.array_equal(got, t["m12"]) and np.array_equal(got, mdl), where
    for i, j in cf["expect"].items():
        assert got[i] == j, (where, "left row", i, "planned", j, "device", int(got[i]))
    assert (ms_p[b, n_l:] == -1).all(), (where, "rows beyond n_l")
    assert counts[b, 0] == len(tail["src"]), (where, "stereo points", counts[b, 0], len(tail["src"]))
    assert np.array_equal(dev.debug_stereo(b)["desc"], f["desc_l"][tail["src"]]), (where, "kept rows")
    if grid and n_l:   # the device's own window gather: candidates per left row, and from them per right key-point
        _, _, cells_l, off, cand = dev.debug_grid(b, lines=False)
        assert len(off) == n_l + 1
        assert [cand[off[i]:off[i + 1]].tolist() for i in range(n_l)] == t["cands"], (where, "candidates")
        assert np.array_equal(np.bincount(cand, minlength=len(f["kp_r"]))[:len(f["kp_r"])], t["r_cand"]), (where, "candidates per right key-point")
        assert np.array_equal(cells_l, cases.cells_of(f["kp_l"], cases.GRID_CAM)), (where, "left cells")


def run_points(oracle, frames, cam, mp, switches, env, K, route, fused_cells=None, grid_streams=None, tag=""):
    from stvo_amd import capi
    switches(env)
    cap = int(env["STVO_GRID_FUSED_CAP"]) if int(env.get("STVO_GRID_FUSED_CAP", "-1")) >= 0 else None
    B = len(frames)
    res = [cases.frame_result(oracle, cf, cam, mp) for cf in frames]
    ctx = capi.Context(device_id=0, max_rows=(K + 63) & ~63, max_batch=B)
    dev = capi.Sequences(ctx, B, K, 64, cam, mp, opt_params("kitti", has_lines=0))
    try:
        dev.enable_fetch(True)
        _, counts = dev.push([cf["frame"] for cf in frames])
        if fused_cells is not None:
            assert dev.last_schedule()["fused_cells"] == fused_cells, (tag, env)
        ms_p = dev.fetch_matches()[0]
        words = dev.debug_point_route()   # before debug_grid, whose kernels clear ovf
        for b, (cf, r) in enumerate(zip(frames, res)):
            where = (tag, cf["name"], "stream", b, env, "K", K)
            check_stream(dev, b, cf, r, ms_p, counts, where, grid_streams is None or b in grid_streams)
            assert tuple(words[b]) == planned_route(cf, r[2], mp, route, cap), (where, "(misfit, ovf)", tuple(words[b]))
    finally:
        dev.close()
        ctx.close()


def run_set(oracle, cs, switches, env, route, K=None, fused_cells=None):
    if cs["cap"] is not None and "STVO_GRID_FUSED_CAP" not in env and route == FUSED:
        env = dict(env, STVO_GRID_FUSED_CAP=str(cs["cap"]))
    K = cs["K"] if K is None else K
    ws = int(cs["mp"].matching_s_ws)
    if ws > 16:   # the rule of stvo_seq_create: the left cell sort, and with it the one-workgroup route, ends there
        route, fused_cells = SCAN, 0
    run_points(oracle, cs["frames"], cs["cam"], cs["mp"], switches, env, K, route, fused_cells, tag=cs["name"])


@pytest.mark.parametrize("name", SETS)
def test_points_default_route(oracle, switches, name):
    """one workgroup per frame, which builds the cells of its frame itself"""
    run_set(oracle, cases.get_set(name), switches, {}, FUSED, fused_cells=1)


@pytest.mark.parametrize("name", SETS)
def test_points_cells_launch(oracle, switches, name):
    """STVO_GRID_CELLS=0: point_cells_kernel as its own launch, the persistent matcher behind it"""
    run_set(oracle, cases.get_set(name), switches, {"STVO_GRID_CELLS": "0"}, FUSED, fused_cells=0)


@pytest.mark.parametrize("name", SETS)
def test_points_scan_formulation(oracle, switches, name):
    run_set(oracle, cases.get_set(name), switches, {"STVO_GRID_FUSED": "0"}, SCAN, fused_cells=0)


@pytest.mark.parametrize("name", SETS)
def test_points_every_frame_misfits(oracle, switches, name):
    """STVO_GRID_FUSED_CAP=-1: the one-workgroup kernel hands every frame to the scan formulation it carries"""
    run_set(oracle, cases.get_set(name), switches, {"STVO_GRID_FUSED_CAP": "-1"}, ALL_MISFIT, fused_cells=1)


@pytest.mark.parametrize("name", SETS)
def test_points_tail_launch(oracle, switches, name):
    """STVO_GRID_TAIL=0: the tail of the association as its own launch"""
    run_set(oracle, cases.get_set(name), switches, {"STVO_GRID_TAIL": "0"}, FUSED, fused_cells=1)


@pytest.mark.parametrize("K", [64, 512, 2048])
@pytest.mark.parametrize("name", cases.SMALL_SETS)
def test_points_small_sets_in_every_capacity(oracle, switches, name, K):
    """the LDS arrays of the kernel are narrower than the stride of the batch (2048: as wide)"""
    run_set(oracle, cases.get_set(name), switches, {}, FUSED, K=K, fused_cells=1)


def test_points_capacity_ends_at_2048():
    """2049 key-points per image: stvo_seq_create refuses (STVO_POSE_MAX_POINTS), so the scan formulation is never reached by capacity —
    only by matching_s_ws above 16, by a frame that misfits, or by a switch, which the tests above cover; P6 (left row 2047, scan
    position 2047) runs on it in test_points_scan_formulation and test_points_every_frame_misfits"""
    from stvo_amd import capi
    cs = cases.get_set("P6 index range")
    ctx = capi.Context(device_id=0, max_rows=2112, max_batch=1)
    try:
        with pytest.raises(capi.StvoError, match="capacity"):
            capi.Sequences(ctx, 1, 2049, 64, cs["cam"], cs["mp"], opt_params("kitti", has_lines=0))
    finally:
        ctx.close()


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("env", [{}, {"STVO_GRID_FUSED_CAP": str(cases.SMALL_CAP)}], ids=["default-cap", "small-cap"])
def test_points_more_streams_than_cus(oracle, switches, env):
    """2 x CUs + 3 streams: every persistent workgroup takes two or three frames of different sizes and prefetches the next while it
    finishes the current one; misfits come first, in the middle and last in a workgroup's list.  Every stream against its frame's
    expectation; the misfit words exactly the planned ones."""
    cyc = cases.cycle_frames()
    B = 2 * cu_count() + 3
    frames = [cyc[b % len(cyc)] for b in range(B)]
    mp = cases.get_set("P2+P3 kitti")["mp"]
    # what the lists of the workgroups look like (workgroup w takes the streams w, w + CUs, ..), by the planned words
    cap = int(env["STVO_GRID_FUSED_CAP"]) if env else None
    mis = [cases.planned_misfit(cases.frame_result(oracle, cf, cases.GRID_CAM, mp)[2], cap) for cf in frames]
    lists = [list(range(w, B, cu_count())) for w in range(cu_count())]
    assert all(len({frames[b]["name"] for b in li}) == len(li) for li in lists), "a workgroup meets the same frame twice"
    assert any(mis[li[0]] and not mis[li[1]] for li in lists) and any(mis[li[-1]] and not mis[li[0]] for li in lists)
    assert any(len(li) == 3 and mis[li[1]] and not mis[li[0]] and not mis[li[2]] for li in lists) or cap is not None
    assert any(len(li) == 3 and mis[li[1]] for li in lists)
    run_points(oracle, frames, cases.GRID_CAM, mp, switches, env, 512, FUSED, fused_cells=0, grid_streams=set(range(0, B, 37)), tag="cycle")


def test_points_more_than_64_frames_per_workgroup(oracle, switches):
    """64 x CUs + 1 streams of at most 64 key-points, alternating fit and misfit under STVO_GRID_FUSED_CAP: the first workgroup takes a
    65th frame, whose misfit flag it reads back from memory (the mask in registers holds 64)"""
    from stvo_amd import capi
    env = {"STVO_GRID_FUSED_CAP": str(cases.TINY_CAP)}
    switches(env)
    pair = cases.tiny_cap_frames()
    mp = cases.get_set("P2+P3 kitti")["mp"]
    res = [cases.frame_result(oracle, cf, cases.GRID_CAM, mp) for cf in pair]
    cus = cu_count()
    B = 64 * cus + 1
    # stream b = workgroup b % CUs, trip b // CUs: fit and misfit alternate along every workgroup's list AND across the workgroups;
    # the 65th frame of workgroup 0 misfits
    kind = [((b // cus) + (b % cus) + 1) % 2 for b in range(B - 1)] + [1]
    ctx = capi.Context(device_id=0, max_rows=64, max_batch=B)
    dev = capi.Sequences(ctx, B, 64, 64, cases.GRID_CAM, mp, opt_params("kitti", has_lines=0))
    try:
        dev.enable_fetch(True)
        _, counts = dev.push([pair[k]["frame"] for k in kind])
        ms_p = dev.fetch_matches()[0]
        words = dev.debug_point_route()
        kind = np.asarray(kind)
        for k in (0, 1):
            ref, mdl, t, tail = res[k]
            sel = np.nonzero(kind == k)[0]
            n_l = len(ref)
            assert np.array_equal(ref, t["m12"]) and (ref >= 0).sum() > 3
            bad = sel[(ms_p[sel, :n_l] != ref).any(axis=1)]
            assert len(bad) == 0, ("streams", bad[:8], "kind", k)
            assert (ms_p[sel, n_l:] == -1).all() and (counts[sel, 0] == len(tail["src"])).all()
            assert (words[sel, 0] == PLANNED_CAPPED[pair[k]["name"]]).all() and (words[sel, 1] == 0).all(), ("misfit words", k)
        for b in (0, B - 1):
            check_stream(dev, b, pair[kind[b]], res[kind[b]], ms_p, counts, ("many frames", b), True)
    finally:
        dev.close()
        ctx.close()


# ---- the C-ABI entry point: general windows, the cover + bit-matrix formulation -------------------------------------------------------
def gather(cells1, start, items, w, n2):
    """GridStructure::get for every left cell, out-of-range ids dropped (matching.cpp:141), as ascending lists"""
    out = []
    for x, y in np.asarray(cells1).tolist():
        s = set()
        for xx in range(max(0, x - w[0]), min(cases.COLS, x + w[1] + 1)):
            for yy in range(max(0, y - w[2]), min(cases.ROWS, y + w[3] + 1)):
                c = yy * cases.COLS + xx
                s.update(int(i) for i in items[start[c]:start[c + 1]] if 0 <= i < n2)
        out.append(sorted(s))
    return out


def check_capi(oracle, hip, cells1, d1, cells2, owner, d2, w, ratio, mutual, where, expect=None):
    start, items = oracle.grid_build(cells2, owner)
    n2 = len(d2)
    ref, n_ref = oracle.match_grid_points(cells1, d1, start, items, d2, w, ratio, mutual)
    mdl = np_model.match_grid(gather(cells1, start, items, w, n2), d1, d2, ratio, bool(mutual))
    got, n = hip.match_grid_points(cells1, d1, start, items, d2, w, ratio, mutual)
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, (where, "left rows", bad[:8], "device", got[bad[:8]], "oracle", ref[bad[:8]])
    assert np.array_equal(got, mdl) and n == n_ref == int((ref >= 0).sum()), where
    if expect is not None:
        assert np.array_equal(got, expect), where


@pytest.mark.parametrize("mutual", [1, 0])
@pytest.mark.parametrize("w", [(10, 0, 0, 0), (3, 2, 1, 1)], ids=["stereo-window", "general-window"])
def test_capi_points_probes(oracle, hip, mutual, w):
    """the P2 / P3 probes as cells and a CSR grid; with the stereo window the trace's matches are the expectation"""
    cs = cases.get_set("P2+P3 kitti" if mutual else "P2+P3 kitti, best_lr off")
    for cf, (ref, mdl, t, tail) in zip(cs["frames"], cases.results(oracle, cs)):
        f = cf["frame"]
        check_capi(oracle, hip, cases.cells_of(f["kp_l"], cs["cam"]), f["desc_l"], cases.cells_of(f["kp_r"], cs["cam"]), None, f["desc_r"], w,
                   float(cs["mp"].min_ratio_12_p_d), mutual, (cf["name"], w, mutual), t["m12"] if w == (10, 0, 0, 0) else None)


@pytest.mark.parametrize("mutual", [1, 0])
@pytest.mark.parametrize("n1,n2", [(63, 63), (64, 64), (65, 65), (255, 128), (256, 129), (257, 64), (64, 129)])
def test_capi_points_sizes_and_windows(oracle, hip, n1, n2, mutual):
    """the mask words (n2 at 63 .. 129) and the padding of the left rows (n1 at 63 .. 257) with windows open on every side, items
    listed in two cells, ids outside [0, n2), and few distinct distances: rows that share a right key-point at equal, falling and
    rising distances are the common case"""
    rng = np.random.default_rng(1000 * n1 + n2)
    cells1 = np.stack([rng.integers(-3, 70, n1), rng.integers(-2, 50, n1)], axis=1).astype(np.int32)
    cells1[:8] = [(-1, 5), (0, 0), (63, 47), (64, 47), (70, 10), (10, -1), (10, 48), (66, 0)]
    n_items = n2 + 24
    cells2 = np.stack([rng.integers(0, 64, n_items), rng.integers(0, 48, n_items)], axis=1).astype(np.int32)
    cells2[:6] = [(0, 0), (63, 47), (-1, 3), (64, 3), (5, -1), (5, 48)]        # the last four: the sink
    owner = np.arange(n_items, dtype=np.int32)
    owner[n2:n2 + 12] = rng.integers(0, n2, 12)                                # items listed in a second cell
    owner[n2 + 12:] = [-1, -7, n2, n2 + 1, n2 + 100, 2 ** 30, -1, n2, -2, n2 + 5, n2 + 6, -3]   # ids outside [0, n2)
    d1 = np.stack([cases.therm(int(k)) for k in rng.integers(0, 9, n1)])
    d2 = np.stack([cases.therm(int(k)) for k in rng.integers(0, 9, n2)])
    for w in ((6, 2, 1, 2), (0, 5, 3, 0), (63, 63, 0, 0)):
        for ratio in (0.75, 1.0):
            check_capi(oracle, hip, cells1, d1, cells2, owner, d2, w, ratio, mutual, (n1, n2, w, ratio, mutual))
