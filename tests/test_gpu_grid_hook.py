"""The key-point side of the stvo_seq_debug_grid test hook.  The pipeline keeps no candidate bit-matrix for the key-points (its point
routes derive their masks from ranges): the hook materialises the masks of ONE frame into a matrix it allocates for the call and frees
before it returns.  Here: every candidate list it reports against the oracle's GridStructure::get (orc_grid_window_gather over
orc_grid_build, the gather tests/test_gpu_grid.py and tests/test_oracle_matching.py rest on) — two mask words (K 128) and the largest
matrix (K 2048), frames with no right key-point, with one bit in the second word and with a full capacity of them, left key-points in
grid columns 0 and 63 and up to matching_s_ws columns right of the grid — and, against a second pipeline with the same input that is
never asked, that the hook leaves no state behind."""
import numpy as np
import pytest

import point_match_cases as cases
from stereo_tail_cases import GRID_CAM
from stvo_amd import synth
from stvo_amd.ctypes_types import match_params, opt_params

pytestmark = pytest.mark.gpu

CELL = 32.0  # GRID_CAM: a grid cell is 32 x 32 pixels


def make_frame(rng, n_l, n_r, ws):
    """left key-points: a share each in grid column 0, in column 63 and 1 .. ws columns right of the grid, the rest anywhere on it;
    right key-points anywhere on the grid"""
    def inside(n, x_lo=0, x_hi=64):
        return np.stack([rng.uniform(x_lo * CELL, x_hi * CELL - 0.5, n), rng.uniform(0.0, 48 * CELL - 0.5, n)], axis=1).astype(np.float32)
    q = n_l // 8
    kp_l = np.concatenate([inside(q, 0, 1), inside(q, 63, 64), inside(q, 64, 64 + ws), inside(q, 64 + ws - 1, 64 + ws), inside(n_l - 4 * q)])
    kp_l, kp_r = kp_l[rng.permutation(n_l)], inside(n_r)
    last = -1
    if n_r:  # the right key-point at the LAST scan position (cell order, index order within a cell) gets left key-point 0 into its cell
        c_r = cases.cells_of(kp_r, GRID_CAM)
        last = int(np.lexsort((np.arange(n_r), c_r[:, 1] * 64 + c_r[:, 0]))[-1])
        kp_l[0] = kp_r[last]
    e4, e32 = np.zeros((0, 4), np.float32), np.zeros((0, 32), np.uint8)
    return dict(kp_l=kp_l, oct_l=rng.integers(0, 4, n_l).astype(np.int32), desc_l=synth.random_desc(rng, n_l), kp_r=kp_r,
                desc_r=synth.random_desc(rng, n_r), kl_l=e4, oct_ll=np.zeros(0, np.int32), ldesc_l=e32, kl_r=e4, ldesc_r=e32, last_right=last)


def oracle_candidates(oracle, f, ws):
    c_l, c_r = cases.cells_of(f["kp_l"], GRID_CAM), cases.cells_of(f["kp_r"], GRID_CAM)
    start, items = oracle.grid_build(c_r)
    n_r = len(c_r)
    return c_l, [sorted(oracle.window_gather(start, items, int(x), int(y), (ws, 0, 0, 0), n_r).tolist()) for x, y in c_l.tolist()]


# (max_keypoints, right key-points per frame; None = the capacity K), left key-points per frame
SHAPES = [(65, [0, 65, None], [96, 128, 64]), (2048, [2048, 700], [400, 2048])]


@pytest.mark.parametrize("env", [{}, {"STVO_GRID_FUSED": "0"}], ids=["default route", "STVO_GRID_FUSED=0"])
@pytest.mark.parametrize("max_kp,n_right,n_left", SHAPES, ids=["B3-K128", "B2-K2048"])
def test_key_point_hook_on_a_matrix_of_its_own(oracle, switches, env, max_kp, n_right, n_left):
    from stvo_amd import capi
    switches(env)
    B, K = len(n_right), (max_kp + 63) & ~63
    n_right = [K if n is None else n for n in n_right]
    mp, op = match_params("kitti"), opt_params("kitti", has_lines=0)
    ws = int(mp.matching_s_ws)
    rng = np.random.default_rng(20 + max_kp)
    steps = [[make_frame(rng, n_left[b], n_right[b], ws) for b in range(B)] for _ in range(3)]
    left_cols = np.concatenate([cases.cells_of(f["kp_l"], GRID_CAM)[:, 0] for f in steps[1]])
    assert (left_cols == 0).any() and (left_cols == 63).any() and (left_cols == 64 + ws - 1).any() and left_cols.max() == 64 + ws - 1
    ctx = capi.Context(device_id=0, max_rows=K, max_batch=B)
    pipes = [capi.Sequences(ctx, B, max_kp, 64, GRID_CAM, mp, op) for _ in range(2)]
    try:
        assert pipes[0].strides()[0] == K
        for dev in pipes:
            dev.enable_fetch(True)
            dev.push(steps[0])
            dev.push(steps[1])  # a tracked step
        asked = pipes[0]
        for b in [B - 1, 0, B // 2]:  # last, first, middle: the matrix of a call belongs to that call's frame alone
            f = steps[1][b]
            c_l, want = oracle_candidates(oracle, f, ws)
            _, _, cells_l, off, cand = asked.debug_grid(b, lines=False)
            assert np.array_equal(cells_l, c_l), (b, "left cells")
            assert len(off) == len(c_l) + 1
            got = [cand[off[i]:off[i + 1]].tolist() for i in range(len(c_l))]
            assert got == want, (b, "candidates", [i for i in range(len(c_l)) if got[i] != want[i]][:8])
            if n_right[b] == 0:
                assert len(cand) == 0
            else:  # the right key-point at the last scan position — at 65 of them the ONE bit of the second mask word — is a candidate
                assert f["last_right"] in want[0] and f["last_right"] in got[0]
        # the hook left nothing behind: the next step of the pipeline that was asked equals that of the one that was not
        out = []
        for dev in pipes:
            res, counts = dev.push(steps[2])
            out.append((res.tobytes(), counts.copy(), dev.fetch_matches()))
        assert out[0][0] == out[1][0], "pose results differ after the hook"
        assert np.array_equal(out[0][1], out[1][1]), "counts differ after the hook"
        for a, b_ in zip(out[0][2], out[1][2]):
            assert np.array_equal(a, b_), "match indices differ after the hook"
        assert (out[0][2][0] >= 0).any()  # (the steps matched something)
    finally:
        for dev in pipes:
            dev.close()
        ctx.close()
