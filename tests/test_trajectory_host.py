"""Trajectory and key-frame decision on the CPU alone: the product's traj_update.h compiled for the host (tests/cpp/traj_host.cpp)
against the extended-precision statement (tests/np_trajectory.py) and the oracle's pieces, on the shared inputs of
tests/trajectory_cases.py.  The kernel runs the same text per lane; tests/test_gpu_trajectory.py judges it by the same statement."""
import ctypes as C

import numpy as np
import pytest

import np_trajectory as npt
import traj_host_lib
import trajectory_cases as tc
from stvo_amd import capi
from stvo_amd.ctypes_types import TRAJ_RECORD_DTYPE, TRAJ_STATE_DTYPE, TrajParams

# What the host function may deviate from the extended-precision statement: it is a double statement of the same products, as the
# oracle is, with another order of operations inside the helpers (one reciprocal of theta, sincos) — so the oracle's own largest
# deviation per field, times 8 (the factor the device gets), plus one ulp of the field's largest magnitude.


def test_layout_and_presets():
    assert traj_host_lib.sizes() == (C.sizeof(TrajParams), TRAJ_STATE_DTYPE.itemsize, TRAJ_RECORD_DTYPE.itemsize) == (32, 856, 448)
    p = capi.traj_params("kitti")
    assert (p.keyframes, p.min_entropy_ratio, p.max_kf_t_dist, p.max_kf_r_dist) == (1, 0.85, 5.0, 15.0)   # config_euroc.yaml:4-6, src/config.cpp
    e = capi.traj_params("euroc", keyframes=False, max_kf_t_dist=2.0)
    assert (e.keyframes, e.min_entropy_ratio, e.max_kf_t_dist, e.max_kf_r_dist) == (0, 0.85, 2.0, 15.0)
    with pytest.raises(TypeError):
        capi.traj_params("kitti", max_t=3)
    with pytest.raises(KeyError):
        capi.traj_params("tum")
    s = traj_host_lib.init(3)
    for b in range(3):   # as `initialize` leaves the handler: Tfw_cov is the identity, not zero
        d = tc.state_to_dict(s[b])
        assert np.array_equal(d["Tfw"], np.eye(4)) and np.array_equal(d["Tfw_cov"], np.eye(6)) and np.array_equal(d["T_prevKF"], np.eye(4))
        assert not d["cov_prevKF_currF"].any() and d["entropy_first_prevKF"] == 0.0
        assert (d["prev_f_iskf"], d["N_prevKF_currF"], d["n_frames"], d["n_keyframes"]) == (1, 0, 0, 0)


def test_stepwise_parity():
    """Case 1: 60 frames with failed frames in between, every update from the same double state by the three statements."""
    c = tc.stepwise()
    d = c["decisions"]
    assert d["host"] == d["ld"] == d["oracle"]
    assert 3 <= sum(d["host"]) < len(d["host"])   # both outcomes occur
    for i in c["ints"]:
        assert i["host"] == i["ld"] == i["oracle"]
    failed = [f for f in range(tc.N_FRAMES) if c["results"][f]["status"] != 0]
    assert failed and all(d["host"][f] == 1 for f in failed)
    assert [int(r[0]["frame"]) for r in c["records"]] == list(range(1, tc.N_FRAMES + 1))
    b = tc.bounds()
    print("\nfield                  magnitude   host dev    oracle dev  host / oracle   bound")
    for k in npt.FIELDS:
        h, o = c["deviation"]["host"][k], c["deviation"]["oracle"][k]
        print(f"{k:22s} {c['magnitude'][k]:10.3e}  {h:10.3e}  {o:10.3e}  {h / o if o else float('inf') if h else 0.0:10.2f}  {b[k]:10.3e}")
    for k in npt.FIELDS:
        assert c["deviation"]["host"][k] <= b[k], k
    # after a reset: I, I, 0 exactly, and the record keeps the pose from before it
    for f, s in enumerate(c["states"]):
        st = tc.state_to_dict(s[0])
        if d["host"][f]:
            assert np.array_equal(st["Tfw"], np.eye(4)) and np.array_equal(st["Tfw_cov"], np.eye(6)) and not st["cov_prevKF_currF"].any()
            assert st["prev_f_iskf"] == 1 and st["N_prevKF_currF"] == 0
        else:
            assert np.array_equal(st["Tfw"].reshape(-1), c["records"][f][0]["Tfw"])


def test_decision_guard():
    """No frame of case 1 lies within 1e-9 (relative) of a threshold in the extended-precision statement: every decision is compared."""
    assert tc.stepwise()["guarded"] == 0


@pytest.mark.parametrize("case", tc.triggers(), ids=lambda c: c[0])
def test_trigger_alone(case):
    """2a-2g: every operand of the OR fires alone at least once — asserted on the extended-precision statement — and the host
    function fires there too, and nowhere before."""
    name, p, results, idx, term = case
    prm = tc.prm_dict(p)
    for q in (p, tc.common_params()):   # the case's own thresholds (the others out of reach), and the set the device batch shares
        ld, _ = tc.run_ld(tc.prm_dict(q), results)
        fired = [f for f, (rec, terms) in enumerate(ld) if terms]
        assert fired and fired[0] == idx, (name, fired)
        assert ld[idx][1] == {term}, (name, ld[idx][1])
        assert not any(tc.near_threshold(rec, tc.prm_dict(q)) for rec, _ in ld[:idx + 1])
    ld, _ = tc.run_ld(prm, results)
    first = idx
    state = traj_host_lib.init(1)
    for f in range(len(results)):
        before = tc.state_to_dict(state[0])
        rec = traj_host_lib.update(results[f:f + 1], p, state)
        assert int(rec[0]["new_kf"]) == ld[f][0]["new_kf"], (name, f)
        if f == first:
            assert before["N_prevKF_currF"] <= 10 or term == "count"
    if name == "entropy":
        assert 1 <= first <= 10
    if name == "count":   # 11 frames pass (N reaches 11), the 12th fires
        assert first == 11 and [t for _, t in ld[:11]] == [set()] * 11
    if name == "singular":
        s1 = traj_host_lib.init(1)
        kf_off = capi.traj_params("kitti", max_kf_t_dist=tc.FAR, max_kf_r_dist=tc.FAR)
        rec = traj_host_lib.update(results[:1], kf_off, s1)
        assert np.isposinf(rec[0]["entropy_ratio"]) and rec[0]["new_kf"] == 1
        # the reset keeps entropy_first_prevKF: the literal, exactly
        assert float(s1[0]["entropy_first_prevKF"]) == npt.ENTROPY_OF_SINGULAR == -999999999.99
    if name == "nan":
        s1 = traj_host_lib.init(1)
        recs = [traj_host_lib.update(results[f:f + 1], p, s1)[0] for f in range(2)]
        assert np.isnan(recs[1]["entropy_ratio"]) and recs[1]["new_kf"] == 1 and np.array_equal(s1[0]["Tfw_cov"], np.eye(6).reshape(-1))


def test_keyframes_off():
    """2h: 40 frames with keyframes off: never a reset, Tfw is the chained product, the record's decision fields are 0.
    "The same tolerance as case 1" is read in two ways, both asserted.  Step-wise, as case 1 itself compares (every update from
    the same double state): the case-1 bound, unchanged.  For the final pose against the product of all 40 increments in extended
    precision, which case 1 has no counterpart of: 40 times that bound — every update adds at most the step bound and the
    updates that follow carry an error on through a rigid motion (|R e| = |e|; the lever of a rotation error over the few units
    of path left is below the translation part of the bound), so the errors add and do not grow."""
    c = tc.stepwise(keyframes=False, n=40)
    assert not any(c["decisions"]["host"]) and c["guarded"] == 0
    last = tc.state_to_dict(c["states"][-1][0])
    assert last["n_keyframes"] == 0 and last["n_frames"] == 40 and last["prev_f_iskf"] == 1 and last["N_prevKF_currF"] == 0
    for r in c["records"]:
        assert r[0]["entropy_ratio"] == 0 and r[0]["t"] == 0 and r[0]["r"] == 0 and r[0]["new_kf"] == 0
    b = tc.bounds()
    for k in ("Tfw", "Tfw_cov"):   # step-wise, as case 1
        assert c["deviation"]["host"][k] <= 8.0 * c["deviation"]["oracle"][k] + float(np.spacing(c["magnitude"][k])), k
    # and the whole chain: the product of the increments in extended precision, re-normalised as the reference does at every frame
    ld, s = tc.run_ld(tc.prm_dict(c["prm"]), c["results"])
    T = np.eye(4, dtype=npt.LD)
    for r in c["results"]:
        if r["status"] == 0:
            T = T @ np.asarray(r["T"], dtype=npt.LD).reshape(4, 4)
    assert np.max(np.abs(last["Tfw"] - T)) <= 40 * b["Tfw"]
    assert np.max(np.abs(last["Tfw"] - s["Tfw"])) <= 40 * b["Tfw"]


def test_batch_checker_on_the_host_function():
    """The checker the device tests use (trajectory_cases.check_batch), run on the host function: every stream at another phase of
    case 1 for 13 updates, and the triggers side by side under their shared thresholds.  Nothing is left out by the guard."""
    b = tc.bounds()
    for p, results in ((tc.stepwise()["prm"], tc.phased(65, 13)), (tc.common_params(), tc.trigger_batch())):
        worst, dec, guarded = tc.check_batch(tc.host_update, p, results, traj_host_lib.init(len(results)), b)
        assert guarded == 0
        assert dec.any(axis=1).all()      # every stream meets a key-frame: the 12-frame rule passes through all of them
    assert [int(np.argmax(d)) for d in dec] == [c[3] for c in tc.triggers()]
