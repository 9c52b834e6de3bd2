"""The tails of the stereo association (src/stereoFrame.cpp:152-172, :351-395, :405-415, :473-508) on the CPU: the oracle
(orc_stereo_points / orc_stereo_lines), the product's host functions (pm::stereo_row_overlap / pm::stereo_line_disparities, which the
line kernels and host/stereoFrame.cpp share) and the plain second statement tests/np_stereo_tail.py, over the case frames of
tests/stereo_tail_cases.py — the frames tests/test_gpu_stereo_tail.py then runs through the device.  Proves the cases (the matcher
returns the plan, every branch is reached, the generic frames keep their distance from every threshold, the quirk matters) and
the statement before a GPU is involved."""
import itertools

import numpy as np
import pytest

import np_stereo_tail as st
import pm_host_lib
import stereo_tail_cases as cases

PERSISTENT_B = 259  # 256 CUs + 3, what the GPU test builds on an MI355X


def all_sets():
    return cases.filter_sets() + [cases.compaction_set(), cases.persistent_set(PERSISTENT_B)]


@pytest.fixture(scope="module")
def statements():
    """{(set name, frame index): (statement of the points, statement of the lines)} from the PLAN, computed once"""
    out = {}
    for cs in all_sets():
        for k, cf in enumerate(cs["frames"]):
            f = cf["frame"]
            out[cs["name"], k] = (st.stereo_points(f["kp_l"], f["oct_l"], f["kp_r"], cf["plan_p"], cs["cam"], cs["mp"]),
                                  st.stereo_lines(f["kl_l"], f["oct_ll"], f["kl_r"], cf["plan_l"], cs["cam"], cs["mp"]))
    return out


def test_the_matcher_returns_the_plan(oracle):
    n = 0
    for cs in all_sets():
        for cf, (p, l) in zip(cs["frames"], cases.oracle_results(oracle, cs)):
            f = cf["frame"]
            if len(f["kp_l"]) and len(f["kp_r"]):  # (:126-127 / :315-316: nothing is matched against an empty side)
                assert np.array_equal(p["m12_raw"], cf["plan_p"]), (cs["name"], cf["name"], np.nonzero(p["m12_raw"] != cf["plan_p"])[0][:8])
            else:
                assert not (cf["plan_p"] >= 0).any()
            if len(f["kl_l"]) and len(f["kl_r"]):
                assert np.array_equal(l["m12_raw"], cf["plan_l"]), (cs["name"], cf["name"], np.nonzero(l["m12_raw"] != cf["plan_l"])[0][:8])
            else:
                assert not (cf["plan_l"] >= 0).any()
            n += 1
    assert n == 10 + 54 + PERSISTENT_B


def test_every_named_case_takes_the_branch_it_was_built_for(statements):
    tags_p, tags_l, ovs = set(), set(), {}
    for cs in all_sets():
        for k, cf in enumerate(cs["frames"]):
            sp, sl = statements[cs["name"], k]
            for kind, s, exp, names in (("point", sp, cf["expect_p"], cf["names_p"]), ("line", sl, cf["expect_l"], cf["names_l"])):
                bad = np.nonzero((exp >= 0) & (exp != s["tag"]))[0]
                assert len(bad) == 0, [(cs["name"], cf["name"], kind, names[i], "built for", st.TAG_NAMES[exp[i]], "took", st.TAG_NAMES[s["tag"][i]])
                                       for i in bad[:5]]
            tags_p |= set(sp["tag"].tolist()); tags_l |= set(sl["tag"].tolist())
            for o, t in zip(sl["ov"], sl["tag"]):
                if o >= 0:
                    ovs.setdefault(int(o), set()).add(bool(t == st.KEPT))
    assert tags_p == {st.NONE, st.EPIPOLAR, st.DISPARITY, st.KEPT}
    assert tags_l == {st.NONE, st.DISPARITY, st.RATIO, st.HORIZONTAL, st.OV_DISJOINT, st.OV_SPANS, st.OV_PARTIAL, st.OV_SHORT, st.KEPT}
    # every outcome of lineSegmentOverlapStereo is reached, and the two that yield a fraction on either side of stereo_overlap_th
    assert set(ovs) == {st.OV_FLAT, st.OV_DISJOINT, st.OV_SPANS, st.OV_PARTIAL, st.OV_SHORT}
    assert ovs[st.OV_SPANS] == {True, False} and ovs[st.OV_PARTIAL] == {True, False}


def test_both_sides_of_every_threshold(statements):
    """a kept and a dropped feature on either side of every threshold the issue lists, by the names the builders gave them"""
    fate = {}
    for cs in cases.filter_sets():
        for k, cf in enumerate(cs["frames"]):
            sp, sl = statements[cs["name"], k]
            for i, nm in enumerate(cf["names_p"]):
                if nm:
                    fate[cs["name"], nm] = int(sp["tag"][i])
            for i, nm in enumerate(cf["names_l"]):
                if nm:
                    fate[cs["name"], nm] = int(sl["tag"][i])
    K, E, D, R, H = st.KEPT, st.EPIPOLAR, st.DISPARITY, st.RATIO, st.HORIZONTAL
    assert fate["kitti", "dy = 0"] == K and fate["kitti", "dy = the smallest subnormal float"] == E
    assert fate["kitti", "dy = one ulp of the rows"] == E and fate["euroc", "dy = one ulp of the rows"] == K
    for side in ("yl above", "yr above"):
        assert [fate["euroc", f"dy = float(1.0) {k:+d} ulp, {side}"] for k in (-1, 0, 1)] == [K, K, E]
        # 0.3f = 0.300000011920929 > 0.3: a row difference of 0.3f is dropped; a comparison in float would keep it
        assert [fate["epip 0.3", f"dy = float(0.3) {k:+d} ulp, {side}"] for k in (-1, 0, 1)] == [K, E, E]
    for s in ("kitti", "euroc", "epip 0.3"):
        assert [fate[s, "disparity = " + n] for n in ("the float below 1", "min_disp exactly", "the float above 1", "0", "-2")] == [D, K, K, D, D]
    assert fate["min_disp 600", "float 600.0 (kept), double 600 - u/2"] == K
    assert fate["min_disp 600 + 2.25 ulp", "float 600 + 2u (dropped), double 600 + 2.5u"] == D
    assert [fate["kitti", n] for n in ("ratio 7 / 10 = 0.7 exactly, ds > de", "ratio 7 / 10 = 0.7 exactly, ds < de", "ratio just below 0.7, ds > de",
                                        "ratio just below 0.7, ds < de", "one disparity negative", "both negative (ratio 10 / 7: not reset)")] == [K, K, R, R, R, D]
    f01 = np.float32(0.1)
    assert [fate["kitti", f"left rows differ by {float(v)!r}"] for v in (cases.nxt(f01, -1), f01, cases.nxt(f01, 1))] == [H, K, K]
    assert fate["kitti", "left rows equal"] == H
    assert fate["kitti", "eln - spn = 1 / 128 <= 0.01f"] == st.OV_SHORT and fate["kitti", "eln - spn = 1 / 64 > 0.01f: overlap 1"] == K
    assert all(v == D for (s, n), v in fate.items() if n.startswith("horizontal right line"))
    assert sum(n.startswith("horizontal right line") for (s, n) in fate) == 3


def ulps(a, b):
    """distance of two float64 arrays in units of the last place of the larger (0 where both are equal, NaN / inf included)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, d)


def test_oracle_against_the_statement(oracle, statements):
    worst = 0.0
    for cs in all_sets():
        for k, (cf, (p, l)) in enumerate(zip(cs["frames"], cases.oracle_results(oracle, cs))):
            sp, sl = statements[cs["name"], k]
            where = (cs["name"], cf["name"])
            assert np.array_equal(p["src_idx"], sp["src"]), where  # the same kept indices in the same order
            assert np.array_equal(l["src_idx"], sl["src"]), where
            pairs = [(p["pl"], sp["rc"][:, :2].astype(np.float64)), (p["disp"], sp["rc"][:, 2].astype(np.float64)), (p["P"], sp["P"]),
                     (p["sigma2"], sp["sigma2"]), (l["spl"], sl["spl"]), (l["epl"], sl["epl"]), (l["sdisp"], sl["sdisp"]),
                     (l["edisp"], sl["edisp"]), (l["sP"], sl["sP"]), (l["eP"], sl["eP"]), (l["le"], sl["le"]), (l["sigma2"], sl["s2l"])]
            for a, b in pairs:
                if cf["exact"]:
                    assert np.array_equal(a, b), where  # bit for bit on the dyadic frames
                elif a.size:
                    u = float(ulps(a, b).max())
                    worst = max(worst, u)
                    assert u <= 4.0, (where, u)
    print(f"oracle vs float64 statement on the generic frames: {worst:.2f} ulp at most")


def test_generic_frames_keep_their_distance_from_every_threshold(statements):
    """the condition under which the GPU test compares the decisions of the generic frames: no quantity a decision depends on is, in
    extended precision, closer than a relative 1e-9 to its threshold — for every matched line of every generic frame, none left out"""
    cs = [s for s in cases.filter_sets() if s["name"] == "generic"][0]
    assert len(cs["frames"]) == 3
    for k, cf in enumerate(cs["frames"]):
        sl = statements[cs["name"], k][1]
        assert len(cf["frame"]["kp_l"]) == 400 and len(cf["frame"]["kl_l"]) == 120
        m = sl["margin"][cf["plan_l"] >= 0]
        assert len(m) > 90 and m.min() >= 1e-9, (cf["name"], m.min())


def test_the_quirk_matters():
    """:367 reads the overwritten sp_r.  A statement with the quirk removed must disagree with the reference's on at least a tenth of
    the quirk frame, and flip the verdict where the left start row is the right end row."""
    cs = cases.filter_sets()[0]
    cf = [c for c in cs["frames"] if c["name"] == "line quirk"][0]
    f = cf["frame"]
    a = st.stereo_lines(f["kl_l"], f["oct_ll"], f["kl_r"], cf["plan_l"], cs["cam"], cs["mp"], quirk=True)
    b = st.stereo_lines(f["kl_l"], f["oct_ll"], f["kl_r"], cf["plan_l"], cs["cam"], cs["mp"], quirk=False)
    n = len(f["kl_l"])
    differs = a["tag"] != b["tag"]
    ka, kb = {int(i): r for i, r in zip(a["src"], range(len(a["src"])))}, {int(i): r for i, r in zip(b["src"], range(len(b["src"])))}
    for i in set(ka) & set(kb):
        if a["edisp"][ka[i]] != b["edisp"][kb[i]] or not np.array_equal(a["eP"][ka[i]], b["eP"][kb[i]]):
            differs[i] = True
    flips = [i for i, nm in enumerate(cf["names_l"]) if nm.startswith("left start row = right end row")]
    assert len(flips) == 4 and all(a["tag"][i] == st.DISPARITY and b["tag"][i] == st.KEPT for i in flips)
    assert differs.sum() * 10 >= n, (int(differs.sum()), n)
    assert (a["tag"] == st.KEPT).sum() >= 8  # and the quirk frame is not all drops


def test_no_statement_keeps_a_pair_with_a_horizontal_right_line(oracle):
    cs = cases.filter_sets()[0]
    cf = [c for c in cs["frames"] if c["name"] == "line filters"][0]
    f = cf["frame"]
    idx = [i for i, nm in enumerate(cf["names_l"]) if nm.startswith("horizontal right line")]
    assert len(idx) == 3
    l = cases.oracle_results(oracle, cs)[cs["frames"].index(cf)][1]
    assert not set(idx) & set(l["src_idx"].tolist())
    for quirk in (True, False):
        s = st.stereo_lines(f["kl_l"], f["oct_ll"], f["kl_r"], cf["plan_l"], cs["cam"], cs["mp"], quirk=quirk)
        assert not set(idx) & set(s["src"].tolist())
    # what the three cases were built to produce in the first re-intersection: x / 0, 0 / 0, and inf * 0 in the second
    got = []
    for i in idx:
        lft, r = f["kl_l"][i].astype(np.float64), f["kl_r"][cf["plan_l"][i]].astype(np.float64)
        spx, epx = st.reintersect(lft[:2], lft[2:], r[:2], r[2:])
        got.append((bool(np.isinf(spx)), bool(np.isnan(spx)), bool(np.isnan(epx))))
    assert got == [(True, False, False), (False, True, True), (True, False, True)]


SPECIAL = [0.0, -0.0, 1.0, -1.0, 0.1, 0.0999999, 0.7, 7.0, 10.0, -3.0, 264.0, 392.0, 391.9921875, 1e-320, np.inf, -np.inf, np.nan]


def same(a, b):
    return (np.isnan(a) and np.isnan(b)) or (a == b and np.signbit(a) == np.signbit(b))


def test_host_functions_against_the_statement(oracle, statements):
    """pm::stereo_row_overlap / pm::stereo_line_disparities (line_tail_frame and host/stereoFrame.cpp call these) and the oracle's
    orc_line_overlap_stereo against the statement: over every matched line of the filter frames and a dense sweep of NaN / +-inf / equal
    arguments — where std::min / std::max (the reference) and fmin / fmax part ways."""
    pm = pm_host_lib.load()
    n = 0
    out2 = np.zeros(2)

    def check(yl_s, yl_e, yr_s, yr_e, th):
        ov, _ = st.row_overlap(yl_s, yl_e, yr_s, yr_e, th)
        got = pm.pmh_stereo_row_overlap(yl_s, yl_e, yr_s, yr_e, th)
        assert same(got, float(ov)), ("pm::stereo_row_overlap", yl_s, yl_e, yr_s, yr_e, got, ov)
        got = oracle.line_overlap_stereo(yl_s, yl_e, yr_s, yr_e, th)
        assert same(got, float(ov)), ("orc_line_overlap_stereo", yl_s, yl_e, yr_s, yr_e, got, ov)

    def check_disp(a, b, c, d, ratio):
        ds, de, _ = st.line_disparities(a, b, c, d, ratio)
        pm.pmh_stereo_line_disparities(a, b, c, d, ratio, out2)
        assert same(out2[0], float(ds)) and same(out2[1], float(de)), ("pm::stereo_line_disparities", a, b, c, d, out2, ds, de)

    for cs in cases.filter_sets():
        th, ratio = cs["mp"].line_horiz_th, cs["mp"].ls_min_disp_ratio
        for cf in cs["frames"]:
            f = cf["frame"]
            for i in np.nonzero(cf["plan_l"] >= 0)[0]:
                l, r = f["kl_l"][i].astype(np.float64), f["kl_r"][cf["plan_l"][i]].astype(np.float64)
                check(l[1], l[3], r[1], r[3], th)
                spx, epx = st.reintersect(l[:2], l[2:], r[:2], r[2:])
                check_disp(l[0], l[2], float(spx), float(epx), ratio)
                n += 1
    assert n > 300
    for v in itertools.product(SPECIAL, repeat=4):
        check(*v, 0.1)
        check_disp(*v, 0.7)
