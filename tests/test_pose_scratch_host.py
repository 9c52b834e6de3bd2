"""The route of a pose launch and the arena of the batch pose kernels (stvo-pl_amd/csrc/pose_scratch.h), run on the host, against a
plain statement written here: which kernel a launch of B frame pairs takes, with how many waves per pair, whether the in-kernel
ordering and the start flag are honoured, and how many bytes of arena the launch works in."""
import pytest

import pose_scratch_host_lib as psh

CUS = 256
MAX_POINTS, MAX_LINES = 2048, 512  # STVO_POSE_MAX_POINTS / STVO_POSE_MAX_LINES (include/stvo_hip.h)


def plain_route(B, compact, evaluation, cus, pose_kernel, pose2p_nw):
    """the plain statement (a switch given as None is unset)"""
    batch = (not evaluation) and (pose_kernel == 4 or (pose_kernel != 1 and B > 256))
    if not batch:
        waves = 0
    elif pose2p_nw is not None and pose2p_nw > 0:
        waves = 4 if pose2p_nw >= 4 else 2
    else:
        waves = 2 if B > 2 * cus else 4
    return dict(batch=batch, waves=waves, inline_sync=1 <= B <= 16 and pose_kernel != 4, start_flag=B > 0 and compact and batch,
                arena_bytes=B * 16 * (7 * 512 + (0 if compact else 3 * 2048)) if batch else 0)


BS = [0, 1, 16, 17, 256, 257, 2 * CUS, 2 * CUS + 1]


def test_constants():
    c = psh.constants()
    assert c == dict(word_bytes=16, max_points=MAX_POINTS, max_lines=MAX_LINES)
    # per frame pair: 7 parts per key-line, 3 more per stereo point in the double form, 16-byte words
    assert psh.pair_words(True) == 7 * MAX_LINES and psh.pair_words(False) == 7 * MAX_LINES + 3 * MAX_POINTS
    assert psh.pair_words(True) * 16 == 57344 and psh.pair_words(False) * 16 == 155648


@pytest.mark.parametrize("nw", [None, 2, 4], ids=lambda v: "nw%s" % v)
@pytest.mark.parametrize("which", [None, 1, 4], ids=lambda v: "kernel%s" % v)
@pytest.mark.parametrize("evaluation", [False, True], ids=["optimise", "evaluate"])
@pytest.mark.parametrize("compact", [False, True], ids=["doubles", "compact"])
def test_route_equals_the_plain_statement(compact, evaluation, which, nw):
    for B in BS:
        assert psh.route(B, compact, evaluation, CUS, which, nw) == plain_route(B, compact, evaluation, CUS, which, nw), B


def test_planes_of_either_wave_count_fill_the_pair():
    """what the batch kernels address: LPT * 7 * BLOCK key-line words and PPT * 3 * BLOCK point words per pair, BLOCK = 64 waves —
    the same for two and four waves per pair, and what the header states"""
    for waves in (2, 4):
        block = 64 * waves
        ppt, lpt = -(-MAX_POINTS // block), -(-MAX_LINES // block)
        assert lpt * 7 * block == psh.pair_words(True) and (ppt * 3 + lpt * 7) * block == psh.pair_words(False)


def test_headline_figures():
    """no switch: one pair and 256 pairs on the latency kernel, nothing of the arena; 1024 streams of the pipeline on two waves per
    pair with 57 344 bytes each; 512 pairs of doubles on four waves with 155 648 bytes each"""
    assert psh.route(1, True, False, CUS) == dict(batch=False, waves=0, inline_sync=True, start_flag=False, arena_bytes=0)
    assert psh.route(256, False, False, CUS) == dict(batch=False, waves=0, inline_sync=False, start_flag=False, arena_bytes=0)
    assert psh.route(1024, True, False, CUS) == dict(batch=True, waves=2, inline_sync=False, start_flag=True, arena_bytes=1024 * 57344)
    assert psh.route(512, False, False, CUS) == dict(batch=True, waves=4, inline_sync=False, start_flag=False, arena_bytes=512 * 155648)
