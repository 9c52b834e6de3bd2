"""The adaptive FAST threshold on the CPU alone: the numpy statement of the rule (tests/np_fast_adapt.py, written from the reference's
updateFrame) against the thresholds pipeline_ref.run_sequence chains, the shipped parameter presets, and the fairness of the GPU
tests' streams (tests/fast_adapt_cases.py): the chain the GPU is compared with must move the threshold in every way the rule can."""
import ctypes as C

import numpy as np
import pytest

import fast_adapt_cases as fc
import np_fast_adapt
from stvo_amd import capi


@pytest.fixture(scope="module")
def chain(oracle):
    return fc.cpu_chain(oracle)


def moves(chain, prm):
    """Every updateFrame of the chain: (stream, frame, threshold before, after, unclipped target, status, lost)"""
    out = []
    for s, c in enumerate(chain):
        for k, r in enumerate(c["ref"], start=1):
            before, after = c["th"][k], c["after"][k - 1]
            free = np_fast_adapt.update(before, r["T"], r["err"], r["n_inliers_pt"], -10 ** 6, 10 ** 6, prm.inc_th, prm.feat_th, prm.err_th)
            lost = bool(np.all(r["T"] == np.eye(4))) or r["err"] > float(np.float32(prm.err_th))
            out.append((s, k, before, after, free, r["status"], lost))
    return out


def test_presets_are_the_shipped_values():
    k, e = capi.fast_adapt_params("kitti"), capi.fast_adapt_params("euroc")
    assert (k.min_th, k.max_th, k.inc_th, k.feat_th, k.err_th) == (7, 30, 5, 50, 0.5)      # config_kitti.yaml
    assert (e.min_th, e.max_th, e.inc_th, e.feat_th, e.err_th) == (5, 50, 5, 50, 0.5)      # config.yaml, config_euroc / _full / _fast.yaml
    o = capi.fast_adapt_params("euroc", max_th=28, err_th=0.3)
    assert (o.min_th, o.max_th) == (5, 28) and o.err_th == np.float32(0.3) and o.err_th != 0.3   # the float the reference compares with
    assert C.sizeof(capi.FastAdapt) == 20
    with pytest.raises(TypeError):
        capi.fast_adapt_params("kitti", maxth=3)
    with pytest.raises(KeyError):
        capi.fast_adapt_params("tum")


def test_statement_against_the_reference_chain(chain):
    prm = fc.params()
    assert len(chain) == len(fc.STREAMS)
    for s, c in enumerate(chain):
        assert len(c["th"]) == fc.N_FRAMES and len(c["ref"]) == fc.N_FRAMES - 1
        assert c["th"][0] == c["th"][1] == fc.TH0        # initialize() has no updateFrame(): the second frame is detected at the start value
        for k, r in enumerate(c["ref"], start=1):
            got = np_fast_adapt.update(c["th"][k], r["T"], r["err"], r["n_inliers_pt"], prm.min_th, prm.max_th, prm.inc_th, prm.feat_th, prm.err_th)
            assert got == r["fast"], (s, k, c["th"][k], got, r["fast"])
            if k + 1 < fc.N_FRAMES:
                assert c["th"][k + 1] == r["fast"]
        print("stream", fc.STREAMS[s], "thresholds", c["th"], "->", c["after"][-1], "status", [r["status"] for r in c["ref"]],
              "inliers", [r["n_inliers_pt"] for r in c["ref"]], "err", [round(float(r["err"]), 3) for r in c["ref"]])


def test_the_chain_moves_the_threshold_in_every_way(chain):
    """What makes the GPU comparison worth having — if a change of synth loses one of these, this fails instead of the GPU tests
    passing with less coverage."""
    prm = fc.params()
    mv = moves(chain, prm)
    assert any(a > b for _, _, b, a, _, _, _ in mv), "no rise"
    assert any(a < b for _, _, b, a, _, _, _ in mv), "no fall"
    assert any(f < prm.min_th and a == prm.min_th for _, _, b, a, f, _, _ in mv), "no move cut at min_th"
    assert any(f > prm.max_th and a == prm.max_th for _, _, b, a, f, _, _ in mv), "no move cut at max_th"
    assert any(st == 3 and lost for _, _, _, _, _, st, lost in mv), "no frame lost by rejection"
    assert any(st == 0 and lost for _, _, _, _, _, st, lost in mv), "no committed frame lost by err > err_th"
    assert any(st == 0 and not lost and a != b for _, _, b, a, _, st, lost in mv), "no move by the inlier count"
    assert any(len({c["th"][k] for c in chain}) > 1 for k in range(fc.N_FRAMES)), "the streams never hold different thresholds"


def test_the_chain_meets_the_capacity_cut(chain, oracle):
    """The chain caps the ORB oracle's output at the device pipeline's capacity (fc.MAX_KP).  At least one image of it must have more
    key-points than that, so that the cut — the first MAX_KP of the row-major order — is part of what the GPU is compared with, and
    most must have fewer, so that the comparison is not one of truncated frames."""
    over = [(s, k, side, n) for s, c in enumerate(chain) for k, lr in enumerate(c["uncut"]) for side, n in enumerate(lr) if n > fc.MAX_KP]
    total = sum(2 * len(c["uncut"]) for c in chain)
    print("images of the chain above MAX_KP (stream, frame, side, key-points):", over, "of", total)
    assert over, "no image of the chain exceeds MAX_KP: the capacity cut is not exercised"
    assert 2 * len(over) < total
    s, k, side, n = over[0]
    img = fc.images()[s][k][side]
    kw = dict(nfeatures=fc.NFEATURES, nlevels=1, fast_th=chain[s]["th"][k], pattern=oracle.orb_default_pattern())
    full, cut = oracle.orb_detect_levels(img, cap=1 << 16, **kw), oracle.orb_detect_levels(img, cap=fc.MAX_KP, **kw)
    assert len(full["kp"]) == n and len(cut["kp"]) == fc.MAX_KP
    for f in ("kp", "response", "angle", "desc", "octave"):   # the cut is a prefix of the uncut order
        assert np.array_equal(cut[f], full[f][:fc.MAX_KP]), f


def test_statement_edges():
    """The rows of the rule and the one-sided clips, by hand (kitti values)."""
    T = np.eye(4); T[0, 3] = 0.1
    u = lambda th, n, T=T, err=0.1, err_th=0.5: np_fast_adapt.update(th, T, err, n, 7, 30, 5, 50, err_th)
    assert [u(20, n) for n in (49, 50, 99, 100, 150, 151, 200, 201, 1000)] == [10, 15, 15, 20, 20, 25, 25, 25, 25]
    assert u(20, 120, T=np.eye(4)) == 10 and u(20, 120, err=-1.0) == 20
    off = np.eye(4); off[0, 0] = np.nextafter(1.0, 2.0)
    assert u(20, 120, T=off) == 20
    assert u(20, 120, err=0.5) == 20 and u(20, 120, err=np.nextafter(0.5, 1.0)) == 10
    assert [u(20, 120, err=e, err_th=0.3) for e in (0.3, 0.30000001, 0.3000001)] == [20, 20, 10]
    assert u(16, 49) == 7 and u(17, 49) == 7 and u(18, 49) == 8 and u(26, 151) == 30 and u(24, 151) == 29
    assert u(1, 151) == 6 and u(50, 99) == 45   # outside the range on the other side: not pulled in
