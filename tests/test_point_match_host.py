"""The case frames of tests/point_match_cases.py on the CPU: the plain traced statement of matchGrid, the oracle, the numpy model (which
visits the candidates in the opposite order) and the plan's own expectations agree on every frame; every edge a case records is
carried by the rows it names; the counts and capacities of P4 / P5 are hit exactly.  tests/test_gpu_point_match.py then holds the
device against the same expectations."""
import numpy as np
import pytest

import point_match_cases as cases

SETS = [cs["name"] for cs in cases.point_sets()]


def flag(t, f, name):
    """a recorded edge as a predicate over the left rows"""
    nl = len(f["kp_l"])
    if name == "outside_trunc":    # a negative coordinate that (int) truncates INTO the grid, with a candidate there
        return (f["kp_l"].min(axis=1) < 0) & (t["outside"] == 0) & (t["n_cand"] > 0)
    if name == "r_outside":        # the partner of the row, the right key-point of the same descriptor, lies outside the grid
        out = np.zeros(nl, bool)
        for i in range(nl):
            same = np.nonzero((f["desc_r"] == f["desc_l"][i]).all(axis=1))[0]
            out[i] = len(same) > 0 and bool(t["r_outside"][same].all())
        return out
    if name == "bait":             # a right key-point outside the grid holds exactly this row's descriptor
        return np.array([bool(((f["desc_r"] == f["desc_l"][i]).all(axis=1) & (t["r_outside"] > 0)).any()) for i in range(nl)])
    if name == "three":
        return t["n_elig"] == 3
    if name == "chain":
        return t["n_elig"] >= 1
    if name == "decisive":         # refused by one bit: best + 1 == second
        return (t["refused"] > 0) & (t["second"] == t["best"] + 1)
    if name == "last_row":
        return np.arange(nl) == nl - 1
    return t[name] > 0


@pytest.mark.parametrize("name", SETS)
def test_point_cases_are_fair_and_hit_their_edges(oracle, name):
    cs = cases.get_set(name)
    lr = bool(cs["mp"].best_lr_matches)
    for cf, (ref, mdl, t, tail) in zip(cs["frames"], cases.results(oracle, cs)):
        where = (name, cf["name"])
        f = cf["frame"]
        assert np.array_equal(ref, t["m12"]), (where, "oracle and trace disagree at", np.nonzero(ref != t["m12"])[0][:10])
        assert np.array_equal(mdl, t["m12"]), (where, "numpy model and trace disagree at", np.nonzero(mdl != t["m12"])[0][:10])
        for i, j in cf["expect"].items():
            assert ref[i] == j, (where, "left row", i, "planned", j, "oracle", int(ref[i]), "(best, second)", int(t["best"][i]), int(t["second"][i]))
        for e, rows in cf["edges"].items():
            hit = flag(t, f, e)
            assert all(hit[i] for i in rows), (where, e, [i for i in rows if not hit[i]])
        if not lr:
            assert t["skipped"].sum() == 0 and t["lost_mutual"].sum() == 0
        for j, (n, e) in cf.get("right_counts", {}).items():   # P4 / P5: candidates and eligible pairs per right key-point, exactly
            assert (int(t["r_cand"][j]), int(t["r_chain"][j])) == (n, e), (where, "right key-point", j, "planned", (n, e))
        assert (ref >= 0).sum() > 0 and len(tail["src"]) > 0, (where, "no probe passes the tail filters")


def _all(oracle, pred=lambda cs: True):
    return [(cs, cf, r) for cs in cases.point_sets() if pred(cs) for cf, r in zip(cs["frames"], cases.results(oracle, cs))]


def test_point_edge_counts(oracle):
    """every edge the suite is after occurs on the planned rows, with best_lr_matches on and off where it belongs to both"""
    def count(key, pred=lambda cs: True):
        return sum(int(flag(r[2], cf["frame"], key).sum()) for cs, cf, r in _all(oracle, pred))

    lr_on = lambda cs: bool(cs["mp"].best_lr_matches)  # noqa: E731
    lr_off = lambda cs: not cs["mp"].best_lr_matches  # noqa: E731
    for k, n in dict(no_cand=40, outside=30, outside_trunc=9, r_outside=12, bait=12, single=30, tie=2, on_edge=10, refused=40, three=12,
                     skipped=100, lost_mutual=60, none_eligible=100, decisive=8, last_row=30).items():
        assert count(k, lr_on) >= n, (k, count(k, lr_on))
    assert count("on_edge", lr_off) >= 4 and count("refused", lr_off) >= 10 and count("single", lr_off) >= 5
    assert count("skipped", lr_off) == 0 and count("lost_mutual", lr_off) == 0
    # P2: every (best, second) pair of the plan is what its row has, in both index orders
    for ratio, pairs in cases.RATIO_PAIRS.items():
        cs = [s for s in cases.point_sets() if s["name"].startswith("P2") and abs(float(s["mp"].min_ratio_12_p_d) - ratio) < 1e-6
              and s["mp"].best_lr_matches][0]
        t = cases.results(oracle, cs)[0][2]
        got = [(int(b), int(s)) for b, s in zip(t["best"], t["second"])]
        for p in pairs:
            assert got.count(p) >= 2, (ratio, p)
    # the 0.8 pairs are equalities in double — refused — which the float 0.8f would accept
    cs = cases.get_set("P2 ratio 0.8 (double)")
    t = cases.results(oracle, cs)[0][2]
    assert float(cs["mp"].min_ratio_12_p_d) == 0.8
    for b, s in cases.RATIO_PAIRS[0.8]:
        rows = np.nonzero((t["best"] == b) & (t["second"] == s))[0]
        assert len(rows) == 2 and (t["m12"][rows] == -1).all() and (t["on_edge"][rows] == 1).all()
        assert float(b) < float(s) * float(np.float32(0.8)), "the float 0.8f, widened, would accept this pair"


def test_point_counts_and_capacities(oracle):
    """P4 / P5 / P6: candidates and eligible pairs per right key-point on every planned value, the demand of the capacity frames on
    the planned side of each boundary of the one-workgroup route"""
    res = {cf["name"]: (cs, r) for cs, cf, r in _all(oracle)}
    p4 = [r[2] for cs, cf, r in _all(oracle, lambda cs: cs["name"] == "P4 counts")]
    cand = set(np.concatenate([t["r_cand"] for t in p4]).tolist())
    assert cand >= {0, 1, 15, 16, 17, 63, 64, 65, 129}, sorted(cand)
    for wide in (False, True):
        chains = set()
        for t in p4:
            sel = (t["r_cand"] > cases.WIDE_OVER) == wide
            chains |= set(t["r_chain"][sel].tolist())
        assert chains >= ({1, 4, 5, 16, 17} if wide else {1, 4, 5, 16}), (wide, sorted(chains))
    assert [cases.planned_ovf(t, cases.get_set("P4 counts")["mp"]) for t in p4] == [0, 0, 1]
    assert all(cases.planned_misfit(t) == 0 for t in p4)

    def dem(name):
        return cases.demand(res[name][1][2])

    assert dem("P5 256 right key-points with 17 candidates") == (256 * 17, 256)
    assert dem("P5 257 right key-points with 17 candidates") == (257 * 17, 257)
    assert dem("P5 64 right key-points share 128 candidates") == (8192, 64)
    assert dem("P5 64 right key-points share 129 candidates") == (8256, 64)
    C = cases.SMALL_CAP
    for extra in (C, C + 1):
        t = res[f"P5 narrow right key-points, {extra} eligible pairs beyond four"][1][2]
        assert cases.demand(t) == (extra, 0) and (t["r_cand"] <= cases.WIDE_OVER).all()
        assert cases.planned_misfit(t, C) == int(extra > C) and cases.planned_misfit(t) == 0
    for name, mis in (("P5 256 right key-points with 17 candidates", 0), ("P5 257 right key-points with 17 candidates", 1),
                      ("P5 64 right key-points share 128 candidates", 0), ("P5 64 right key-points share 129 candidates", 1)):
        t = res[name][1][2]
        assert cases.planned_misfit(t) == mis
        assert (t["refused"] > 0).sum() >= 10 and (t["lost_mutual"] > 0).sum() >= 3, (name, "no probes ride along")
    # P6: the last left row and the last right key-points of the last cell carry the probe
    cf = cases.get_set("P6 index range")["frames"][0]
    t = res[cf["name"]][1][2]
    f = cf["frame"]
    assert len(f["kp_l"]) == len(f["kp_r"]) == 2048 and t["m12"][2047] == 2046 and (t["best"][2047], t["second"][2047]) == (0, 256)
    assert t["best"][0] == 256 and t["single"][0] == 1 and t["m12"][0] == 0
    c2 = cases.cells_of(f["kp_r"], cases.GRID_CAM)
    assert (c2[2046:] == (63, 47)).all() and ((c2[:2046, 1] * 64 + c2[:2046, 0]) < 47 * 64 + 63).all()   # scan positions 2046, 2047
    # the cycle of the persistent-workgroup test holds an empty frame, a one-point frame, both kinds of misfit
    fr = cases.cycle_frames()
    assert {len(cf["frame"]["kp_l"]) for cf in fr} >= {0, 1} and len(fr) >= 15 and len(fr) % 2 == 1
    mp = cases.get_set("P2+P3 kitti")["mp"]
    mis = [cases.planned_misfit(cases.frame_result(oracle, cf, cases.GRID_CAM, mp)[2]) for cf in fr]
    assert mis[:3] == [0, 0, 1] and 3 <= sum(mis) < len(fr) - 8
