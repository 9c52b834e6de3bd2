"""stvo_amd.ragged.plan: N sequences of different lengths packed onto B lock-step streams, longest first onto the stream that frees up
earliest, RESTART where a stream takes its next sequence and PARK when nothing is left.  Pure host code: no GPU, no library."""
import heapq

import numpy as np
import pytest

from stvo_amd import ragged

RUN, RESTART, PARK = ragged.STREAM_RUN, ragged.STREAM_RESTART, ragged.STREAM_PARK

CASES = [
    ([2, 3, 4, 6, 3], 2),
    ([5, 5, 5, 5], 2),
    ([1, 1, 1, 1, 1, 1, 1], 3),      # length-1 sequences: a RESTART every step
    ([7], 1),
    ([3, 9, 2], 1),                  # one stream: one sequence after the other
    ([4, 2], 5),                     # fewer sequences than streams
    ([], 3),                         # nothing to do
    ([1], 4),
    ([10, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], 2),
    (list(range(1, 14)), 4),
]


def makespan(lengths, B):
    """Longest-first list scheduling, stated independently: a heap of the times at which the streams free up."""
    free = [0] * B
    heapq.heapify(free)
    for n in sorted(lengths, reverse=True):
        heapq.heappush(free, heapq.heappop(free) + n)
    return max(free) if lengths else 0


@pytest.mark.parametrize("lengths,B", CASES, ids=[f"N{len(l)}-B{b}" for l, b in CASES])
def test_plan_properties(lengths, B):
    steps = ragged.plan(lengths, B)
    assert len(steps) == makespan(lengths, B)
    seen = {i: [] for i in range(len(lengths))}      # sequence -> [(step, stream, frame)]
    for t, st in enumerate(steps):
        assert isinstance(st.control, np.ndarray) and st.control.dtype == np.int32 and st.control.shape == (B,)
        assert len(st.consume) == B
        for b, c in enumerate(st.consume):
            if c is None:
                # PARK only on a stream with nothing left: nothing is consumed on it in any later step
                assert st.control[b] == PARK
                assert all(later.consume[b] is None for later in steps[t:])
                continue
            i, k = c
            seen[i].append((t, b, k))
            # RESTART exactly on frame 0 of every sequence but those starting in step 0
            assert st.control[b] == (RESTART if (k == 0 and t > 0) else RUN), (t, b, c)
    for i, n in enumerate(lengths):
        got = seen[i]
        # every (sequence, frame) exactly once, in order, in consecutive steps of ONE stream
        assert [k for _, _, k in got] == list(range(n)), (i, got)
        assert len({b for _, b, _ in got}) == 1
        assert [t for t, _, _ in got] == list(range(got[0][0], got[0][0] + n))
    # every stream-step is a consumed frame or a park
    consumed = sum(c is not None for st in steps for c in st.consume)
    parked = sum(int((st.control == PARK).sum()) for st in steps)
    assert consumed == sum(lengths) and consumed + parked == len(steps) * B


def test_plan_is_longest_first_onto_the_earliest_free_stream():
    steps = ragged.plan([2, 3, 4, 6, 3], 2)
    # 6 -> stream 0 (0..5); 4 -> stream 1 (0..3); 3 (sequence 1) -> stream 1 (4..6); 3 (sequence 4) -> stream 0 (6..8); 2 -> stream 1 (7..8)
    assert len(steps) == 9
    assert [st.consume[0] for st in steps] == [(3, k) for k in range(6)] + [(4, k) for k in range(3)]
    assert [st.consume[1] for st in steps] == [(2, k) for k in range(4)] + [(1, k) for k in range(3)] + [(0, k) for k in range(2)]
    assert [st.control.tolist() for st in steps] == [[RUN, RUN]] * 4 + [[RUN, RESTART], [RUN, RUN], [RESTART, RUN], [RUN, RESTART], [RUN, RUN]]


def test_plan_degenerate_inputs():
    assert ragged.plan([], 3) == []
    steps = ragged.plan([4, 2], 5)
    assert len(steps) == 4
    assert steps[0].control.tolist() == [RUN, RUN, PARK, PARK, PARK]      # streams without any sequence are parked from the start
    assert steps[2].control.tolist() == [RUN, PARK, PARK, PARK, PARK]
    ones = ragged.plan([1, 1, 1], 1)
    assert [st.control.tolist() for st in ones] == [[RUN], [RESTART], [RESTART]]
    assert [st.consume for st in ones] == [[(0, 0)], [(1, 0)], [(2, 0)]]
    for bad in (([3, 0], 2), ([-1], 1), ([2], 0)):
        with pytest.raises(ValueError):
            ragged.plan(*bad)


def test_empty_frame_has_every_feature_array():
    fr = ragged.empty_frame()
    assert set(fr) == {"kp_l", "oct_l", "desc_l", "kp_r", "desc_r", "kl_l", "oct_ll", "ldesc_l", "kl_r", "ldesc_r"}
    assert all(len(v) == 0 for v in fr.values())
