"""What the tails of the stereo association WRITE on the device, record by record: fused_tail (grid_kernels.hip, the last phase of the
one-workgroup point matchers), point_tail_kernel, line_tail_kernel and the tail of line_stereo_fused_kernel (stereo_assoc_kernels.hip), read
back through the stvo_seq_debug_stereo test hook and compared with the oracle and with the extended-precision statement
(tests/np_stereo_tail.py) on the case frames of tests/stereo_tail_cases.py, which tests/test_stereo_tail_host.py has proved on
the CPU.  Every case frame is one stream of a Sequences object and one push runs the whole set; it is the FIRST push, which only
builds the stereo sets, so no pose kernel runs on records that were built to be extreme.

Judgement.  Points (n, rc, the kept descriptor rows) are copies and float differences: bit-exact in every group.  Lines: nl, the
kept rows (through the serial numbers in the descriptors), spl, epl, ldesc, s2l, s2lm are copies and multiplication chains:
bit-exact.  sP, eP, le are bit-exact on the dyadic frames, where every operation has one answer in any evaluation order; on the generic
frames the device contracts into FMAs and the oracle does not, so they are judged against the longdouble statement: per component the
bound is max(floor, 16 x the oracle's own deviation from that statement) — the factor DESIGN.md section 3 uses for the pose terms — with
the floor derived from the case: 8 x 2^-52 x max(|xl|, |xr|, 1) / |disparity| relative for sP / eP (one rounding of the
re-intersected abscissa, amplified by the subtraction), 8 x 2^-52 x (|x_s y_e| + |y_s x_e|) / |x_s y_e - y_s x_e| relative for le's third
component (one rounding of a product, amplified by the subtraction) and 8 x 2^-52 relative for its first two."""
import numpy as np
import pytest

import np_stereo_tail as st
import stereo_tail_cases as cases
from stvo_amd.ctypes_types import opt_params

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52

DEFAULT = {}
SEPARATE = {"STVO_GRID_TAIL": "0", "STVO_LINE_FUSED": "0"}  # point_tail_kernel and line_tail_kernel as launches of their own


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def check_points(where, f, p, rec):
    """p: orc_stereo_points of the frame, rec: debug_stereo"""
    src = p["src_idx"]
    assert rec["n"] == len(src), (where, "stereo points", rec["n"], len(src))
    exp = np.concatenate([f["kp_l"][src], p["disp"].astype(np.float32)[:, None], f["oct_l"][src].astype(np.float32)[:, None]], axis=1)
    assert np.array_equal(exp[:, 2].astype(np.float64), p["disp"])  # the oracle's disparity is a float difference widened
    if not same_bits(rec["rc"], exp.astype(np.float32)):
        k = int(np.nonzero((bits(rec["rc"]) != bits(exp.astype(np.float32))).reshape(len(src), -1).any(axis=1))[0][0])
        raise AssertionError((where, "stereo point", k, "left key-point", int(src[k]), "device", rec["rc"][k].tolist(), "oracle", exp[k].tolist()))
    assert np.array_equal(rec["desc"], f["desc_l"][src]), (where, "kept descriptor rows (they carry the left serial numbers)",
                                                            rec["desc"][:, :4].copy().view("<u4").ravel()[:8], src[:8])


def line_bounds(f, cam, sl, l):
    """per-component bounds for sP, eP, le of the kept lines of a generic frame: sl = the statement (float64 + longdouble), l = the oracle"""
    LD = np.longdouble
    src = sl["src"]
    out = {}
    for key, xcol, dcol, xr in (("sP", 0, "sdisp_ld", 0), ("eP", 2, "edisp_ld", 1)):
        xl = np.abs(f["kl_l"][src, xcol].astype(np.float64))
        amp = np.maximum(np.maximum(xl, np.abs(sl["xr"]).max(axis=1)), 1.0) / np.abs(sl[dcol].astype(np.float64))
        floor = (8.0 * EPS * amp)[:, None] * np.abs(sl[key + "_ld"]).astype(np.float64)
        orc_dev = np.abs(l[key].astype(LD) - sl[key + "_ld"]).astype(np.float64)
        out[key] = np.maximum(floor, 16.0 * orc_dev)
    k = f["kl_l"][src].astype(np.float64)
    a, b = k[:, 0] * k[:, 3], k[:, 1] * k[:, 2]
    amp = np.stack([np.ones(len(src)), np.ones(len(src)), (np.abs(a) + np.abs(b)) / np.abs(a - b)], axis=1)
    floor = 8.0 * EPS * amp * np.abs(sl["le_ld"]).astype(np.float64)
    out["le"] = np.maximum(floor, 16.0 * np.abs(l["le"].astype(LD) - sl["le_ld"]).astype(np.float64))
    return out


def check_lines(where, cs, cf, l, rec, ratios):
    f = cf["frame"]
    src = l["src_idx"]
    assert rec["nl"] == len(src), (where, "stereo lines", rec["nl"], len(src))
    assert np.array_equal(rec["ldesc"], f["ldesc_l"][src]), (where, "kept line descriptor rows (they carry the left serial numbers)",
                                                              rec["ldesc"][:, :4].copy().view("<u4").ravel()[:8], src[:8])
    lv = f["oct_ll"][src]
    exact = dict(spl=l["spl"], epl=l["epl"], s2l=l["sigma2"], s2lm=cases.safe_copy_sigma2(l["sigma2"], lv, cs["mp"]))
    if cf["exact"]:
        exact.update(sP=l["sP"], eP=l["eP"], le=l["le"])
    for key, exp in exact.items():
        if not same_bits(rec[key], exp):
            k = int(np.nonzero((rec[key] != exp).reshape(len(src), -1).any(axis=1))[0][0])
            i = int(src[k])
            raise AssertionError((where, key, "stereo line", k, "left key-line", i, cf["names_l"][i], "device", rec[key][k].tolist(),
                                  "oracle", np.asarray(exp)[k].tolist()))
    for key in ("sP", "eP", "le"):
        assert np.array_equal(np.isfinite(rec[key]), np.isfinite(l[key])), (where, key, "finite exactly where the oracle's are")
    if not cf["exact"] and len(src):
        sl = st.stereo_lines(f["kl_l"], f["oct_ll"], f["kl_r"], cf["plan_l"], cs["cam"], cs["mp"])
        assert np.array_equal(sl["src"], src)
        bound = line_bounds(f, cs["cam"], sl, l)
        for key in ("sP", "eP", "le"):
            dev = np.abs(rec[key].astype(np.longdouble) - sl[key + "_ld"]).astype(np.float64)
            r = dev / bound[key]
            for c in range(3):
                ratios[key, c] = max(ratios.get((key, c), 0.0), float(r[:, c].max()))
            if (r > 1.0).any():
                k, c = np.unravel_index(int(np.argmax(r)), r.shape)
                raise AssertionError((where, key, "component", int(c), "stereo line", int(k), "left key-line", int(src[k]), "device deviation",
                                      dev[k, c], "bound", bound[key][k, c]))


def run_set(cs, switches, env, expect_schedule, M=None, ratios=None):
    """one Sequences object, one push of the set's frames under the switches `env`; every stream against the oracle"""
    import oracle_lib
    from stvo_amd import capi
    switches(env)
    orc = oracle_lib.load()
    res = cases.oracle_results(orc, cs)
    B, K, M = len(cs["frames"]), cs["K"], M or cs["M"]
    frames = [cf["frame"] for cf in cs["frames"]]
    has_lines = any(len(f["kl_l"]) and len(f["kl_r"]) for f in frames)
    ratios = {} if ratios is None else ratios
    ctx = capi.Context(device_id=0, max_rows=max(K, 512), max_batch=B)
    dev = capi.Sequences(ctx, B, K, M, cs["cam"], cs["mp"], opt_params("kitti"))
    try:
        with pytest.raises(capi.StvoError):
            dev.debug_stereo(0)  # before the first step no set belongs to a frame
        dev.enable_fetch(True)
        _, counts = dev.push(frames)
        sched = dev.last_schedule()
        for k, v in expect_schedule.items():
            if k != "line_fused" or has_lines:
                assert sched[k] == v, (cs["name"], env, k, sched)
        ms_p, ms_l = dev.fetch_matches()[:2]
        for b, (cf, (p, l)) in enumerate(zip(cs["frames"], res)):
            f = cf["frame"]
            where = (cs["name"], cf["name"], "stream", b, env)
            n1, m1 = len(f["kp_l"]), len(f["kl_l"])
            assert np.array_equal(ms_p[b, :n1], cf["plan_p"]), (where, "the point matcher did not return the plan")
            if has_lines:
                assert np.array_equal(ms_l[b, :m1], cf["plan_l"]), (where, "the line matcher did not return the plan")
            rec = dev.debug_stereo(b)
            assert (rec["n"], rec["nl"]) == (counts[b, 0], counts[b, 1]), where
            check_points(where, f, p, rec)
            check_lines(where, cs, cf, l, rec, ratios)
    finally:
        dev.close()
        ctx.close()
    return ratios


@pytest.mark.parametrize("route", ["default", "separate launches"])
@pytest.mark.parametrize("name", [cs["name"] for cs in cases.filter_sets()])
def test_filter_edges(switches, name, route):
    """the well-defined edges of the point and line filters and the generic frames, on the default route (the tails as the last phase of
    the one-workgroup matchers) and with point_tail_kernel / line_tail_kernel as launches of their own"""
    cs = [s for s in cases.filter_sets() if s["name"] == name][0]
    if route == "default":
        ratios = run_set(cs, switches, DEFAULT, dict(fused_cells=1, line_fused=1))
    else:
        ratios = run_set(cs, switches, SEPARATE, dict(line_fused=0))
    if name == "generic":
        assert len(ratios) == 9
        print(f"[stereo tail, {route}] largest device deviation / bound on the generic frames: " +
              ", ".join(f"{k}[{c}] {v:.3f}" for (k, c), v in sorted(ratios.items())))


COMPACTION_ROUTES = {
    "default": (DEFAULT, dict(fused_cells=1, line_fused=1), 320),
    "separate launches": (SEPARATE, dict(line_fused=0), 320),
    "scan matcher, fused lines at M = 512": ({"STVO_GRID_FUSED": "0", "STVO_LINE_FUSED": "1"}, dict(fused_cells=0, line_fused=1), 512),
    "cells kernel in front of the matcher": ({"STVO_GRID_CELLS": "0"}, dict(fused_cells=0, line_fused=1), 320),
}


@pytest.mark.parametrize("route", list(COMPACTION_ROUTES))
def test_compaction_shapes(switches, route):
    """1 .. 2048 key-points and 1 .. 320 key-lines x six keep patterns: every wave, chunk and tid + 1024 seam of the ordered compaction,
    on every route that reaches a tail; a kept row carries its serial number, so a swap shows in the record"""
    env, sched, M = COMPACTION_ROUTES[route]
    cs = cases.compaction_set()
    assert sorted({len(cf["frame"]["kp_l"]) for cf in cs["frames"]}) == cases.POINT_COUNTS
    assert sorted({len(cf["frame"]["kl_l"]) for cf in cs["frames"]}) == cases.LINE_COUNTS
    run_set(cs, switches, env, sched, M=M)


def test_persistent_workgroups_run_the_tail_for_two_frames(switches):
    """more frames than CUs: the point matcher is launched with one persistent workgroup per CU, and three of them run the tail for a
    second frame; counts and keep patterns differ from frame to frame"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cs = cases.persistent_set(cus + 3)
    run_set(cs, switches, DEFAULT, dict(fused_cells=0, line_fused=1))


def test_debug_stereo_capacity(switches):
    """caller-supplied capacities: too small is STVO_ERR_CAPACITY (-4) with the counts filled in, never a partial copy"""
    import ctypes as C
    from stvo_amd import capi
    switches(DEFAULT)
    cs = [s for s in cases.filter_sets() if s["name"] == "kitti"][0]
    frames = [cf["frame"] for cf in cs["frames"]]
    ctx = capi.Context(device_id=0, max_rows=512, max_batch=len(frames))
    dev = capi.Sequences(ctx, len(frames), cs["K"], cs["M"], cs["cam"], cs["mp"], opt_params("kitti"))
    try:
        _, counts = dev.push(frames)
        assert counts[0, 0] > 1 and counts[1, 1] > 1
        n, nl = C.c_int32(-1), C.c_int32(-1)
        rc = np.full(4, 7.0, np.float32); desc = np.zeros(32, np.uint8); d = [np.full(3, 7.0) for _ in range(7)]
        for b, caps in ((0, (1, 64)), (1, (64, 1))):
            code = ctx.lib.stvo_seq_debug_stereo(dev.h, b, caps[0], C.byref(n), rc, desc, caps[1], C.byref(nl), *d, desc)
            assert code == -4 and (n.value, nl.value) == (counts[b, 0], counts[b, 1])
            assert (rc == 7.0).all() and all((a == 7.0).all() for a in d)
        assert ctx.lib.stvo_seq_debug_stereo(dev.h, len(frames), 1, C.byref(n), rc, desc, 1, C.byref(nl), *d, desc) == -1
    finally:
        dev.close()
        ctx.close()
