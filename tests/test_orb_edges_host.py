"""The ORB oracle (oracle/stvo_orb_oracle.c) against the plain statement (tests/np_orb.py) on the planned images of
tests/orb_edge_cases.py, bit for bit, and every case's "this input really sits on its edge" facts.  No GPU.  tests/test_gpu_orb_edges.py
compares the kernels with the same statement: where they differ, this file says which side is wrong."""
import math
import os
import subprocess

import numpy as np
import pytest

import np_orb
import orb_edge_cases as ec

CASES = {c["name"]: c for c in ec.all_cases()}


def same(got, ref, what):
    for k in ("kp", "response", "angle", "desc", "octave"):
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), (what, k)   # bitwise, floats included


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_the_statement(oracle, name):
    c = CASES[name]
    p = c["prm"]
    for b, e in enumerate(ec.expected(c)):
        r = oracle.orb_detect_levels(c["images"][b], nfeatures=p["nfeatures"], nlevels=p["nlevels"], scale_factor=p["scale_factor"],
                                     fast_th=ec.threshold_of(c, b), edge_th=p["edge_th"], pattern=c["pattern"], cap=p["max_keypoints"])
        same(r, e, (name, b))


@pytest.mark.parametrize("name", list(CASES))
def test_case_sits_on_its_edge(name):
    c = CASES[name]
    c["facts"](c, ec.expected(c))


def test_score_by_counting_thresholds():
    """The statement's arc-minimum form of the FAST score against the definition taken literally — for every t, is there an arc of 9 all
    brighter than I + t or all darker than I - t — on the threshold cells."""
    img, _ = ec.threshold_cells(20)
    img = img[20:70, 20:120]
    b, d = np_orb.fast_side_scores(img)
    diff = np_orb.ring_differences(img)
    ext = np.concatenate([diff, diff[:8]])
    count = np.zeros(diff.shape[1:], np.int64)
    for t in range(0, 80):
        hit = np.zeros(count.shape, bool)
        for k in range(16):
            hit |= (ext[k:k + 9] > t).all(axis=0) | (ext[k:k + 9] < -t).all(axis=0)
        count += hit                                             # corner at t implies corner at every smaller t
    got = np.maximum(b, d)[3:-3, 3:-3]
    assert got.max() < 79 and np.array_equal(count - 1, got)


def test_no_reachable_angle_rounds_a_pattern_coordinate_at_a_tie():
    """cvRound's half-to-even rule in the rotation: for every angle a single off-centre pixel can give (every lattice direction of the
    patch) and every int8 pair in [-13, 13]^2, no rotated coordinate lands on x.5 exactly — such a tie cannot be planted with a planned
    image, which is why orb_edge_cases holds none (the host sweep of csrc/orb_rotate.h covers the rounding itself)."""
    disc = np_orb.disc_mask()
    uv = [(u, v) for v in range(-15, 16) for u in range(-15, 16) if disc[v + 15, u + 15]]
    ang = np.unique(np_orb.fast_atan2(np.array([20 * v for _, v in uv], np.float32), np.array([20 * u for u, _ in uv], np.float32)))
    assert len(ang) == 464
    rad = ang * np.float32(math.pi / 180.0)
    a = np.array([math.cos(float(r)) for r in rad]).astype(np.float32)[:, None, None]
    b = np.array([math.sin(float(r)) for r in rad]).astype(np.float32)[:, None, None]
    P = np.arange(-13, 14).astype(np.float32)
    for v in (P[None, :, None] * a - P[None, None, :] * b, P[None, :, None] * b + P[None, None, :] * a):
        assert not np.any(np.abs(v - np.floor(v)) == np.float32(0.5))


def test_rotation_header_on_the_host_full_sweep():
    """tests/cpp/orb_rotate_host_main.cpp: csrc/orb_rotate.h (what orb_describe_kernel rotates the pattern with) compiled for the host, a
    program of its own — (float)cos / (float)sin of EVERY float angle in [0, 360] degrees against the C library, and the rounded
    coordinates of every int8 pair in [-13, 13]^2 against the plain form.  The full sweep: 1.14 G angles, about 30 core-seconds."""
    here = os.path.dirname(os.path.abspath(__file__))
    src, exe = os.path.join(here, "cpp", "orb_rotate_host_main.cpp"), os.path.join(here, "cpp", "orb_rotate_host_main")
    hdr = os.path.join(here, "..", "stvo-pl_amd", "csrc", "orb_rotate.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-o", exe, src])
    out = subprocess.run([exe, "full"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "full sweep: 1135869953 angles" in out.stdout and " 0 mismatches" in out.stdout
