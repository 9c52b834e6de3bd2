"""The ORB kernels (csrc/orb_kernels.hip, through capi.Orb) against the plain statement (tests/np_orb.py) on the planned images of
tests/orb_edge_cases.py: key-points, responses, angles, descriptors and octaves bit for bit, and n_total.  Every group runs twice on the
same detector (scratch reuse: histograms and counters are reset by the kernels).  tests/test_orb_edges_host.py holds the oracle to the
same statement and checks that every case sits on the edge it was planned for."""
import numpy as np
import pytest

import orb_edge_cases as ec

pytestmark = pytest.mark.gpu
CASES = {c["name"]: c for c in ec.all_cases()}


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_equal_the_statement(hip, name):
    from stvo_amd import capi
    c = CASES[name]
    p = c["prm"]
    B, rows, cols = c["images"].shape
    exp = ec.expected(c)
    orb = capi.Orb(hip, B, cols, rows, max_keypoints=p["max_keypoints"], nfeatures=p["nfeatures"], fast_threshold=p["fast_th"],
                   edge_threshold=p["edge_th"], nlevels=p["nlevels"], scale_factor=p["scale_factor"])
    try:
        orb.set_pattern(c["pattern"])
        if c["thresholds"] is not None:
            orb.set_fast_thresholds(c["thresholds"])
        for run in range(2):
            out = orb.detect(c["images"])
            for b in range(B):
                for k in ("kp", "response", "angle", "desc", "octave"):
                    assert out[b][k].shape == exp[b][k].shape, (name, run, b, k, out[b][k].shape, exp[b][k].shape)
                    assert np.array_equal(out[b][k].view(np.uint8), exp[b][k].view(np.uint8)), (name, run, b, k)
                assert out[b]["n_total"] == exp[b]["n_total"], (name, run, b)
    finally:
        orb.close()
