"""The case frames of tests/line_match_cases.py on the CPU: they are fair (the oracle and the numpy model, which visits the candidates
in the opposite order, agree on every one, so no case depends on the reference's unordered_set order), they hit the edges they
record, and the frame-to-frame cases get the stereo sets they plan, completely and in order.  tests/test_gpu_line_match.py then
holds the device against the same expectations."""
import numpy as np
import pytest

import line_match_cases as cases
import np_model
from stvo_amd.ctypes_types import opt_params

STEREO = [cs["name"] for cs in cases.stereo_sets()]
F2F = [cs["name"] for cs in cases.f2f_sets()]


def flag(t, name):
    if name == "gate_close":   # |dot| within a few ulp of line_sim_th
        return t["gate_margin"] < 1e-6
    if name == "dot_eq_th":
        return t["gate_margin"] == 0.0
    return t[name] > 0


@pytest.mark.parametrize("name", STEREO)
def test_stereo_cases_are_fair_and_hit_their_edges(oracle, name):
    cs = [s for s in cases.stereo_sets() if s["name"] == name][0]
    for cf, (ref, mdl, t) in zip(cs["frames"], cases.stereo_results(oracle, cs)):
        where = (name, cf["name"])
        assert np.array_equal(ref, mdl), (where, "oracle and numpy model disagree at", np.nonzero(ref != mdl)[0][:10])
        for i, j in cf["expect"].items():
            if j is not None:
                assert ref[i] == j, (where, "left row", i, "planned", j, "oracle", int(ref[i]))
        for e, rows in cf["edges"].items():
            if not cs["mp"].best_lr_matches and e in ("run_equal", "run_greater", "run_taken", "none_eligible", "single"):
                continue   # the running minimum belongs to best_lr_matches
            hit = flag(t, e)
            assert all(hit[i] for i in rows), (where, e, [i for i in rows if not hit[i]])


def test_stereo_edge_counts(oracle):
    """every edge the suite is after occurs, in the planned sets and in the sweeps"""
    res = {cs["name"]: cases.stereo_results(oracle, cs) for cs in cases.stereo_sets()}

    def count(pred, key, what=lambda r, m, t, k: int(flag(t, k).sum())):
        return sum(what(r, m, t, key) for cs in cases.stereo_sets() if pred(cs) for r, m, t in res[cs["name"]])

    planned = lambda cs: cs["name"].startswith(("S1", "S2", "S3", "S4"))  # noqa: E731
    sweep = lambda cs: cs["name"].startswith(("S6", "S7"))  # noqa: E731
    lr_on = lambda cs: planned(cs) and cs["mp"].best_lr_matches  # noqa: E731
    lr_off = lambda cs: planned(cs) and not cs["mp"].best_lr_matches  # noqa: E731
    floor = dict(nan_l=30, win_absent=5, win_clipped=10, start_only=3, end_only=3, gated=3, gate_close=4, dot_eq_th=1, nan_r_cand=2,
                 clipped_r_cand=4, run_equal=4, run_greater=4, run_taken=5, tie=10, on_edge=8, single=6, none_eligible=1, no_cand=10)
    for k, n in floor.items():
        assert count(lr_on if k.startswith(("run_", "none_")) else planned, k) >= n, k
    assert count(lr_off, "tie") >= 5 and count(lr_off, "on_edge") >= 4 and count(lr_off, "single") >= 3
    assert count(lr_off, "run_equal") == 0   # best_lr_matches off: no running minimum
    for k in ("nan_l", "win_clipped", "gated", "run_equal", "run_greater", "run_taken", "tie", "single", "none_eligible", "no_cand", "clipped_r_cand"):
        assert count(sweep, k) >= 20, k     # low-entropy descriptors: ties and equal distances are the common case
    matched = lambda r, m, t, k: int((r >= 0).sum())  # noqa: E731
    assert count(planned, None, matched) >= 80 and count(sweep, None, matched) >= 500
    # S6: every count on either side, nl != nr within a frame, no left lines, no right lines
    s6 = [cf["frame"] for cs in cases.stereo_sets() if cs["name"].startswith("S6") for cf in cs["frames"]]
    assert {len(f["kl_l"]) for f in s6} >= set(cases.COUNTS) and {len(f["kl_r"]) for f in s6} >= set(cases.COUNTS)
    assert all(len(f["kl_l"]) != len(f["kl_r"]) for f in s6)
    assert {cs["M"] for cs in cases.stereo_sets()} >= {64, 128, 320, 512}


@pytest.mark.parametrize("name", F2F)
def test_f2f_cases_get_their_sets_and_hit_their_edges(oracle, name):
    cs = [s for s in cases.f2f_sets() if s["name"] == name][0]
    mp = cs["mp"]
    nnr, lr = float(mp.min_ratio_12_l), bool(mp.best_lr_matches)
    for b, (s, r) in enumerate(zip(cs["streams"], cases.f2f_results(oracle, cs, opt_params("kitti")))):
        where = (name, s.name, "stream", b)
        # the condition of every f2f case: the planned lines survive the stereo stage completely and in order
        for step, plan in enumerate((s.A, s.B)):
            assert np.array_equal(r["sets"][step], plan), (where, "step", step, len(r["sets"][step]), len(plan))
            assert (r["raw"][step] >= 0).all()
        m, n = oracle.match(s.A, s.B, nnr, int(lr))
        mdl = np_model.match(s.A, s.B, nnr, lr)
        assert np.array_equal(m, mdl), (where, np.nonzero(m != mdl)[0][:10])
        if len(s.A) and len(s.B):
            assert r["ref"]["n_matched_ls"] == n == int((mdl >= 0).sum()), where
        t = cases.f2f_trace(s.A, s.B, nnr, lr)
        for e, rows in s.edges.items():
            if e == "pairs":      # clusters: query row k has exactly the planned (best, second)
                D = np.sort(np_model.hamming_matrix(s.A, s.B), axis=1)[:, :2]
                assert [tuple(x) for x in D.tolist()] == [tuple(p) for p in rows], where
                for k, (d0, d1) in enumerate(rows):
                    assert bool(t["on_edge"][k]) == (np.float32(d0) == np.float32(d1) * np.float32(nnr)) and bool(t["tie"][k]) == (d0 == d1)
            elif e == "pair":
                D = np_model.hamming_matrix(s.A, s.B)
                assert tuple(sorted(D[0].tolist())) == tuple(rows), where
                claim = np.float32(rows[0]) < np.float32(rows[1]) * np.float32(nnr)
                assert (m[0] >= 0) == bool(claim), (where, "the reverse scan was to keep row 0's claim")
            elif e == "kept":
                if lr:
                    assert all(t["kept"][i] for i in rows), (where, e)
            else:
                assert all(t[e][i] > 0 for i in rows), (where, e, [i for i in rows if not t[e][i]])


def test_f2f_edge_counts():
    """ties, ratio edges and the mutual check's cases occur in the planned streams and, by themselves, in the sweeps; every size"""
    tot, sweep = {}, {}
    sizes_a, sizes_b = set(), set()
    for cs in cases.f2f_sets():
        nnr, lr = float(cs["mp"].min_ratio_12_l), bool(cs["mp"].best_lr_matches)
        for s in cs["streams"]:
            t = cases.f2f_trace(s.A, s.B, nnr, lr)
            into = sweep if cs["name"].startswith(("F4", "F5")) else tot
            for k, v in t.items():
                into[k] = into.get(k, 0) + int(v.sum())
            if cs["name"].startswith("F4"):
                sizes_a.add(len(s.A)); sizes_b.add(len(s.B))
                assert len(s.A) != len(s.B)
    for k, n in dict(tie=20, on_edge=8, claim=100, rev_other=8, rev_fail=8, shared_equal=8, shared_diff=4, dup_train_best=8, dup_query=12, kept=60).items():
        assert tot[k] >= n, (k, tot[k])
    for k in ("tie", "claim", "rev_other", "rev_fail", "shared_equal", "shared_diff", "kept"):
        assert sweep[k] >= 50, (k, sweep[k])
    assert sizes_a >= set(cases.F2F_SIZES) and sizes_b >= set(cases.F2F_SIZES)
    assert sizes_a | sizes_b >= {129, 255, 256, 257, 511, 512}
