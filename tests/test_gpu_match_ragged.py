"""K1m's query-tile assignment and its one-block form (csrc/match_mfma.hip) through stvo_match_nnr_mutual_batched_dev: raw m12 of every
frame against the oracle, bit-exact.

A frame's slots of the launch decide from the frame's own row count which query tile they scan (full tiles in the main section, the
ragged or last tile in the end section, the rest leave), and a tile of at most 128 rows runs with one block of 32 rows per wave.  What
that can get wrong sits at row counts around the 32-row blocks, the 128-row switch and the 256-row tiles, at a capacity whose last
tiles are empty (2048) and at one that a frame can fill (512), with a batch one past a multiple of 8 (the XCD remap, `b >= B`)."""
import numpy as np
import pytest
import torch

from stvo_amd import synth

pytestmark = pytest.mark.gpu

B = 9
N1 = [0, 1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 255, 256, 257, 384, 385, 1647, 1792, 1793, 2047, 2048]
N2 = [1, 2, 33, 64, 65, 95, 1647, 2048]
KINDS = ["iid", "identical", "few_distinct", "extremes"]


def _rand(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def _nibble_rows():
    """All-zero, all-one, and every bit of one nibble position set (and cleared): the extremes of a per-row constant built from the
    row's bits per nibble position."""
    rows = [np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8)]
    for d in range(4):
        rows.append(np.full(32, 0x11 << d, np.uint8))
        rows.append(np.full(32, 0xFF ^ (0x11 << d), np.uint8))
    return np.stack(rows)


def _frame(rng, kind, n1, n2):
    """(d1, d2): n1 query rows, n2 train rows."""
    if kind == "iid":
        d2 = _rand(rng, n2)
        d1 = _rand(rng, n1)
        k = min(n1, n2) // 2
        if k:
            d1[rng.permutation(n1)[:k]] = synth.flip_bits(rng, d2[rng.permutation(n2)[:k]], 0.06)
    elif kind == "identical":          # every distance 0: best == second wherever there are two train rows, the lowest index first
        row = _rand(rng, 1)
        d1 = np.repeat(row, n1, 0)
        d2 = np.repeat(row, n2, 0)
    elif kind == "few_distinct":       # five rows, repeated: ties in every tile; queries a few bits off, one of them unique in the train set
        base = _rand(rng, 5)
        d2 = base[np.arange(n2) % 5].copy()
        if n2 > 40:
            d2[n2 - 1] = synth.flip_bits(rng, base[:1], 0.2)[0]     # a row that occurs once: its claimants have a unique best
        d1 = synth.flip_bits(rng, d2[rng.integers(0, max(n2, 1), n1)], 0.03) if n1 else np.zeros((0, 32), np.uint8)
    else:                              # extremes of the rows' bit counts per nibble position on both sides, in a random background
        ext = _nibble_rows()
        d2 = _rand(rng, n2)
        d1 = _rand(rng, n1)
        if n2:
            at = rng.permutation(n2)[:len(ext)]
            d2[at] = synth.flip_bits(rng, ext[:len(at)], 0.02)
        if n1:
            at = rng.permutation(n1)[:len(ext)]
            d1[at] = ext[:len(at)]
    return np.ascontiguousarray(d1), np.ascontiguousarray(d2)


def _calls(row_stride, kind_index):
    """The row counts of every frame of every call: each n1 that fits the capacity once, n2 cycling through its list."""
    n1s = [n for n in N1 if n <= row_stride]
    n2s = [n for n in N2 if n <= row_stride]
    if row_stride not in n1s:
        n1s += [row_stride - 1, row_stride]     # a frame that fills its capacity
        n2s += [row_stride]
    for j in range(-len(n1s) % B):              # fill the last call: counts inside the one-block range and around it again
        n1s.append([100, 128, 129, 1, 300, 111, 257, 64][j])
    pairs = [(n1, n2s[(3 * i + kind_index) % len(n2s)]) for i, n1 in enumerate(n1s)]
    if row_stride == 2048:
        pairs[n1s.index(2048)] = (2048, 2048)   # the largest case
        pairs[n1s.index(1647)] = (1647, 1647)   # the benchmark's shape
    return [pairs[i:i + B] for i in range(0, len(pairs), B)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row_stride", [2048, 512])
def test_ragged_tiles_match_the_oracle(hip, oracle, row_stride, kind):
    rng = np.random.default_rng(1000 * row_stride + KINDS.index(kind))
    nnr = 0.9 if kind == "few_distinct" else 0.75
    matched = 0
    for call in _calls(row_stride, KINDS.index(kind)):
        # rows past a frame's count hold random bytes: they are scanned but must not reach a result
        d1 = _rand(rng, B * row_stride).reshape(B, row_stride, 32)
        d2 = _rand(rng, B * row_stride).reshape(B, row_stride, 32)
        frames = []
        for b, (n1, n2) in enumerate(call):
            a, c = _frame(rng, kind, n1, n2)
            d1[b, :n1] = a
            d2[b, :n2] = c
            frames.append((a, c))
        n1_d = torch.tensor([p[0] for p in call], dtype=torch.int32).cuda()
        n2_d = torch.tensor([p[1] for p in call], dtype=torch.int32).cuda()
        d1_d = torch.from_numpy(d1).cuda()
        d2_d = torch.from_numpy(d2).cuda()
        for mutual in (1, 0):
            m12_d = torch.full((B, row_stride), -7, dtype=torch.int32).cuda()
            torch.cuda.synchronize()
            hip._chk(hip.lib.stvo_match_nnr_mutual_batched_dev(hip.h, B, row_stride, d1_d.data_ptr(), n1_d.data_ptr(), d2_d.data_ptr(),
                                                               n2_d.data_ptr(), nnr, mutual, m12_d.data_ptr()))
            hip.synchronize()
            m12 = m12_d.cpu().numpy()
            for b, ((n1, n2), (a, c)) in enumerate(zip(call, frames)):
                if n1 == 0:
                    continue
                exp, _ = oracle.match(a, c, nnr, mutual)
                got = m12[b, :n1]
                assert np.array_equal(got, exp), (row_stride, kind, mutual, b, n1, n2, np.nonzero(got != exp)[0][:10])
                matched += int((exp >= 0).sum())
    assert (matched == 0) == (kind == "identical"), matched   # (the inputs do decide matches, except where every distance ties)
