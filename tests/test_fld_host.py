"""The FLD statement (tests/cpp/fld_ref.c) on the CPU: its edge map against the numpy second statement (tests/np_fld.py), analytic
cases of the chain walk, the segment fit, the filters, the orientation and the top-N cut, and its deterministic atan2 against libm.
Runs without a GPU."""
import math

import numpy as np
import pytest

import fld_statement
import np_fld
from stvo_amd import capi, synth


@pytest.fixture(scope="module")
def stmt():
    return fld_statement.load()


def step_image(cols=64, rows=48, x0=32, dark=50, bright=200):
    img = np.full((rows, cols), dark, np.uint8)
    img[:, x0:] = bright
    return img


@pytest.mark.parametrize("cols,rows,seed", [(64, 48, 0), (1241, 376, 1), (37, 23, 2), (16, 16, 3), (333, 217, 4)])
def test_edges_match_numpy_on_scenes(stmt, cols, rows, seed):
    img = synth.make_image(seed, cols, rows, n_rects=max(5, cols * rows // 500), n_discs=max(2, cols * rows // 2000))
    e = stmt.edges(img)
    assert np.array_equal(e, np_fld.canny_edges(img))
    assert np.count_nonzero(e) > 0


def test_edges_match_numpy_on_noise_and_borders(stmt):
    rng = np.random.default_rng(7)
    for shape in ((100, 120), (17, 31), (64, 64)):
        img = rng.integers(0, 256, shape).astype(np.uint8)
        e = stmt.edges(img)
        assert np.array_equal(e, np_fld.canny_edges(img))
        rows, cols = shape
        # the corner quirk clears the two corners, not the border strips: edges remain on all four borders
        assert not e[:6, :6].any() and not e[rows - 5:, cols - 5:].any()
        assert e[0, 6:].any() and e[rows - 1, :cols - 5].any() and e[6:, 0].any() and e[:rows - 5, cols - 1].any()


def test_edges_nms_ties_in_each_direction_case(stmt):
    """Ramps: constant gradients make every magnitude equal to its neighbours' — the strict and the non-strict comparisons of the
    three direction cases decide.  Horizontal: m > left and m >= right; vertical: m > up and m >= down; diagonal: both strict."""
    yy, xx = np.mgrid[0:40, 0:50]
    cases = {"horizontal": 10 * xx, "vertical": 10 * yy, "diagonal": 2 * (xx + yy), "anti-diagonal": 2 * (xx - yy) + 100}
    for name, ramp in cases.items():
        img = np.clip(ramp, 0, 255).astype(np.uint8)
        e = stmt.edges(img)
        assert np.array_equal(e, np_fld.canny_edges(img)), name
    # the horizontal ramp: column 1 (a larger magnitude than column 0, a tie with column 2) is the only edge column
    e = stmt.edges(np.clip(cases["horizontal"], 0, 255).astype(np.uint8))
    assert set(np.nonzero(e.any(axis=0))[0]) == {1}
    e = stmt.edges(np.clip(cases["vertical"], 0, 255).astype(np.uint8))
    assert set(np.nonzero(e.any(axis=1))[0]) == {1}


def test_step_edge_one_segment_oriented_by_the_brighter_side(stmt):
    img = step_image()
    seg = stmt.segments(img, 9)
    assert np.array_equal(seg, np.array([[31, 0, 31, 47]], np.float32))
    mirrored = np.ascontiguousarray(img[:, ::-1])  # bright on the left: the same edge column, the ends swapped
    assert np.array_equal(stmt.segments(mirrored, 9), np.array([[31, 47, 31, 0]], np.float32))


def test_chain_shorter_than_L_plus_one_gives_nothing(stmt):
    img = step_image()  # one chain of 48 points
    assert len(stmt.segments(img, 47)) == 1
    assert len(stmt.segments(img, 48)) == 0


def test_segment_near_one_border_is_dropped(stmt):
    img = np.full((48, 64), 50, np.uint8)
    img[:3, :] = 200  # a horizontal edge at row 2: both ends within 5 px of the top border
    assert len(stmt.segments(img, 9)) == 0
    img = np.full((48, 64), 50, np.uint8)
    img[:12, :] = 200  # the same edge further down is kept
    assert len(stmt.segments(img, 9)) == 1


def test_length_threshold_truncates():
    assert capi.fld_params(0.025 * min(1241, 376)).length_threshold == 9   # KITTI: 9.4 -> 9
    assert capi.fld_params(0.025 * min(752, 480)).length_threshold == 12   # EuRoC
    assert capi.fld_params(0.025 * min(640, 240)).length_threshold == 6


def test_walk_later_neighbour_wins_a_tie(stmt):
    """At (10, 6), moving down (direction 1), the neighbours (11, 7) (direction 0) and (9, 7) (direction 2) differ by 1 from the chain
    direction: the later one in getPointChain's order, (9, 7), is taken."""
    e = np.zeros((20, 20), np.uint8)
    for x, y in ((10, 5), (10, 6), (11, 7), (9, 7)):
        e[y, x] = 255
    chains = stmt.walk(e)
    assert [c.tolist() for c in chains] == [[[10, 5], [10, 6], [9, 7]], [[11, 7]]]


def test_top_n_cut_keeps_ties_in_detection_order(stmt):
    img = np.full((48, 64), 30, np.uint8)
    for x0 in (20, 40):
        img[:, x0:x0 + 10] = 200  # four edges of equal length
    seg = stmt.segments(img, 9)
    assert len(seg) == 4 and len(set(np.hypot(seg[:, 0] - seg[:, 2], seg[:, 1] - seg[:, 3]).tolist())) == 1
    rec, resp, n = stmt.keylines(img, 9, nfeatures=2)
    assert n == 4
    got = np.stack([rec["sx"], rec["sy"], rec["ex"], rec["ey"]], axis=1)
    assert np.array_equal(got, seg[:2])
    assert np.array_equal(rec["num_pixels"], [48, 48]) and np.all(resp == np.float32(47) / np.float32(64))


def test_atan2_det_within_one_ulp_of_libm(stmt):
    rng = np.random.default_rng(11)
    n = 1_000_000
    y = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 9, n)
    x = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 9, n)
    k = n // 10  # axes, zeros, signed zeros and integer pixel differences
    special = np.array([0.0, -0.0, 1.0, -1.0, 3.0, -7.0, 1e-300, -1e300])
    y[:k] = rng.choice(special, k); x[k:2 * k] = rng.choice(special, k)
    y[2 * k:3 * k] = rng.integers(-2000, 2001, k); x[2 * k:3 * k] = rng.integers(-2000, 2001, k)
    got = stmt.atan2(y, x)
    want = np.array([math.atan2(a, b) for a, b in zip(y.tolist(), x.tolist())])
    assert np.array_equal(np.signbit(got), np.signbit(want))
    gi, wi = got.view(np.int64), want.view(np.int64)
    assert np.max(np.abs(gi - wi)) <= 1
    axes = (y == 0) | (x == 0)  # on the axes: exactly +-0, +-pi / 2, +-pi
    assert np.array_equal(got[axes], want[axes])
