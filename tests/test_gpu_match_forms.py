"""The forms of launch_match (stvo-pl_amd/csrc/kernels.h) that stvo_match_nnr_mutual_batched_dev reaches — ONE_WAY (mutual = 0) and LAZY
(mutual = 1) — on both paths, the matrix cores and the VALU kernels (STVO_KNN_MFMA=0): raw m12 of every frame against the oracle,
bit-exact.  Small frames at the edges of the 32-row blocks and the 128 / 256-row tiles inside row_stride = 257, B = 1 and B = 9 (one
group of eight frames per XCD round is crossed).  BOTH_DIRS is reachable through the pipeline only: the sequence tests cover it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_match_ragged import _frame, _rand

pytestmark = pytest.mark.gpu

ROW_STRIDE = 257
COUNTS = [0, 1, 2, 31, 33, 127, 129, 257]


def _draws(B):
    """(n1, n2) of every frame of every call: each count appears on either side at least once for either B"""
    rng = np.random.default_rng(257 + B)
    n1s = COUNTS + [int(rng.choice(COUNTS))]
    n2s = [COUNTS[(3 * i + 5) % len(COUNTS)] for i in range(len(n1s))]
    pairs = list(zip(n1s, n2s))
    return [pairs[i:i + B] for i in range(0, len(pairs), B)]


@pytest.mark.parametrize("B", [1, 9])
def test_forms_match_the_oracle(hip, oracle, B):
    rng = np.random.default_rng(4100 + B)
    matched = 0
    for call in _draws(B):
        # rows past a frame's count hold random bytes: they are scanned but must not reach a result
        d1 = _rand(rng, B * ROW_STRIDE).reshape(B, ROW_STRIDE, 32)
        d2 = _rand(rng, B * ROW_STRIDE).reshape(B, ROW_STRIDE, 32)
        frames = []
        for b, (n1, n2) in enumerate(call):
            a, c = _frame(rng, "few_distinct" if b % 3 == 2 and n2 > 0 else "iid", n1, n2)
            d1[b, :n1] = a
            d2[b, :n2] = c
            frames.append((a, c))
        n1_d = torch.tensor([p[0] for p in call], dtype=torch.int32).cuda()
        n2_d = torch.tensor([p[1] for p in call], dtype=torch.int32).cuda()
        d1_d = torch.from_numpy(d1).cuda()
        d2_d = torch.from_numpy(d2).cuda()
        for mutual in (0, 1):
            m12_d = torch.full((B, ROW_STRIDE), -7, dtype=torch.int32).cuda()
            torch.cuda.synchronize()
            hip._chk(hip.lib.stvo_match_nnr_mutual_batched_dev(hip.h, B, ROW_STRIDE, d1_d.data_ptr(), n1_d.data_ptr(), d2_d.data_ptr(),
                                                               n2_d.data_ptr(), 0.75, mutual, m12_d.data_ptr()))
            hip.synchronize()
            m12 = m12_d.cpu().numpy()
            for b, ((n1, n2), (a, c)) in enumerate(zip(call, frames)):
                assert (m12[b, n1:] == -1).all(), (B, mutual, b, n1, n2)   # every row of the stride is written, rows past the count match nothing
                if n1 == 0:
                    continue
                exp, _ = oracle.match(a, c, 0.75, mutual)
                got = m12[b, :n1]
                assert np.array_equal(got, exp), (B, mutual, b, n1, n2, np.nonzero(got != exp)[0][:10])
                matched += int((exp >= 0).sum())
    assert matched > 0


def test_valu_kernels_agree_too():
    """the same cases with STVO_KNN_MFMA=0, in a child process (the switch is read once per process)"""
    env = dict(os.environ, STVO_KNN_MFMA="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "test_forms_match_the_oracle"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
