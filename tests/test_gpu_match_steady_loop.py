"""The forward matcher's split tile loop (csrc/match_mfma.hip) through stvo_match_nnr_mutual_batched_dev: raw m12 of every frame against
the oracle, bit-exact, mutual 0 and 1.

The scan runs a STEADY loop (two groups of two tiles per turn, nothing conditional) while the tiles it fetches ahead are all full, and
the general group in front of it and behind it.  What that can get wrong sits at the tile counts around the loop's entry and exit: the
train counts put 1 .. 16 tiles in ONE segment (STVO_KNN_NSEG=1: below, at and above the loop's first and second turn, odd counts, a
ragged last tile) and the benchmark's 1647 rows, against 1, 33, 129 and 257 query rows (one-block form, which has no steady loop; two-block form
with idle waves, which stay with the general group at the same barriers; a second query tile); the launch's own choice of segments is
taken with one frame of 2048 / 2047 train rows.  Rows: i.i.d.; all identical (the order rests on the train index alone); bits in one
nibble position only, and their complements (the extremes of anything an operand encoding derives per row from its bits per nibble
position); and an exact copy of every query at the last train index of a tile or the first of the next (the hand-over between the two
accumulator sets and between the loops)."""
import numpy as np
import pytest
import torch

from stvo_amd import synth

pytestmark = pytest.mark.gpu

B = 9
ROW_STRIDE = 2048
N1 = [1, 33, 129, 257]                                                   # one-block form, two-block form, a second query tile
# 1 .. 10 tiles; then the steady loop's own edges: it holds two groups and fetches two groups ahead, so behind the first group (tiles
# 0, 1) its first turn needs 10 full tiles and its second 14 — 32 k - 1, 32 k, 32 k + 1 rows give k - 1, k, k full tiles
N2 = [32 * k + e for k in range(1, 16) for e in (-1, 0, 1)] + [1647]
KINDS = ["iid", "identical", "one_class", "duplicate_at_tile_edge"]
CLASS_MASK = [0x11, 0x22, 0x44, 0x88]


def _rand(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def _class_rows(rng, n):
    """Rows whose set bits sit in one nibble class only, and their complements; every other row has the whole class set (cleared)."""
    d = rng.integers(0, 4, n)
    mask = np.array(CLASS_MASK, np.uint8)[d][:, None]
    rows = np.where((np.arange(n) % 2 == 0)[:, None], mask, _rand(rng, n) & mask).astype(np.uint8)
    comp = rng.integers(0, 2, n).astype(bool)
    rows[comp] ^= 0xFF
    return rows


def _frame(rng, kind, n1, n2, i):
    """(d1, d2): n1 query rows, n2 train rows; i numbers the frames of a kind."""
    if kind == "iid":
        d1, d2 = _rand(rng, n1), _rand(rng, n2)
        k = min(n1, n2) // 2
        if k:
            d1[rng.permutation(n1)[:k]] = synth.flip_bits(rng, d2[rng.permutation(n2)[:k]], 0.06)
    elif kind == "identical":                      # every distance 0: the lowest train index wins
        row = _class_rows(rng, 1) if i % 2 else _rand(rng, 1)
        d1, d2 = np.repeat(row, n1, 0), np.repeat(row, n2, 0)
    elif kind == "one_class":                      # on the query side, the train side, both
        side = i % 3
        d1 = _rand(rng, n1) if side == 1 else _class_rows(rng, n1)
        d2 = _rand(rng, n2) if side == 0 else _class_rows(rng, n2)
        if side == 2 and n2 > 2:                   # some queries a few bits off a train row: distinct nearest distances among the ties
            k = max(1, n1 // 3)
            d1[rng.permutation(n1)[:k]] = synth.flip_bits(rng, d2[rng.integers(0, n2, k)], 0.02)
    else:                                          # a random background, one exact copy of the query at the last index of a tile or the first of the next
        d1, d2 = _rand(rng, n1), _rand(rng, n2)
        edges = [j for j in range(31, n2, 32)] + [j for j in range(32, n2, 32)]
        at = rng.permutation(np.array(edges, dtype=np.int64))[:n1]
        d2[at] = d1[:len(at)]
    return np.ascontiguousarray(d1), np.ascontiguousarray(d2)


def _run(hip, oracle, rng, kind, pairs, nnr=0.75):
    """One launch per mutual flag over the frames `pairs` = [(n1, n2)]; returns the number of matches the oracle expects."""
    nb = len(pairs)
    d1 = _rand(rng, nb * ROW_STRIDE).reshape(nb, ROW_STRIDE, 32)       # rows past a frame's count hold random bytes
    d2 = _rand(rng, nb * ROW_STRIDE).reshape(nb, ROW_STRIDE, 32)
    frames = []
    for b, (n1, n2) in enumerate(pairs):
        a, c = _frame(rng, kind, n1, n2, b)
        d1[b, :n1], d2[b, :n2] = a, c
        frames.append((a, c))
    n1_d = torch.tensor([p[0] for p in pairs], dtype=torch.int32).cuda()
    n2_d = torch.tensor([p[1] for p in pairs], dtype=torch.int32).cuda()
    d1_d, d2_d = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    matched = 0
    for mutual in (1, 0):
        m12_d = torch.full((nb, ROW_STRIDE), -7, dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        hip._chk(hip.lib.stvo_match_nnr_mutual_batched_dev(hip.h, nb, ROW_STRIDE, d1_d.data_ptr(), n1_d.data_ptr(), d2_d.data_ptr(),
                                                           n2_d.data_ptr(), nnr, mutual, m12_d.data_ptr()))
        hip.synchronize()
        m12 = m12_d.cpu().numpy()
        for b, ((n1, n2), (a, c)) in enumerate(zip(pairs, frames)):
            exp, _ = oracle.match(a, c, nnr, mutual)
            got = m12[b, :n1]
            assert np.array_equal(got, exp), (kind, mutual, b, n1, n2, np.nonzero(got != exp)[0][:10])
            matched += int((exp >= 0).sum())
    return matched


@pytest.mark.parametrize("kind", KINDS)
def test_tile_counts_in_one_segment(hip, oracle, switches, kind):
    switches({"STVO_KNN_NSEG": "1"})
    rng = np.random.default_rng(77 + KINDS.index(kind))
    pairs = [(n1, n2) for n2 in N2 for n1 in N1]
    pairs += pairs[:-len(pairs) % B]               # fill the last launch
    matched = sum(_run(hip, oracle, rng, kind, pairs[i:i + B]) for i in range(0, len(pairs), B))
    assert (matched == 0) == (kind == "identical"), matched   # (the inputs do decide matches, except where every distance ties)


@pytest.mark.parametrize("kind", KINDS)
def test_segments_as_the_launch_picks_them(hip, oracle, kind):
    rng = np.random.default_rng(177 + KINDS.index(kind))
    for n2 in (2048, 2047):
        _run(hip, oracle, rng, kind, [(257, n2)])                       # B = 1: several train segments
    _run(hip, oracle, rng, kind, [(n1, 1647) for n1 in N1 + N1] + [(1647, 1647)])
