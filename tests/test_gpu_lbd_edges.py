"""The LBD kernels (csrc/lbd_kernels.hip) on the planned key-lines of tests/lbd_edge_cases.py against the plain statement
(tests/np_lbd.py, float32) and the oracle: the 72 floats (NaN payloads included) and the 32 bytes bit for bit, through the host entry
(capi.Lbd.compute) and through the device entry with sentinel-filled outputs, whose rows beyond n_lines must come back untouched.  Every
case runs a second time as the top-left crop of a larger slot under a size table (stvo_lbd_set_image_sizes).  The hard angles of
tests/golden/lbd_hard_angles.npz — where the device's and the host's cos / sin may round to different floats — run as lines of every
length residue.  tests/test_lbd_statement_host.py holds the CPU side: that every case sits on its edge, and that the set tells every
near miss of the statement from the rule."""
import numpy as np
import pytest

import lbd_edge_cases as ec

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in ec.all_cases() + ec.crop_cases() + [ec.hard_angle_lines()]}
SENTINEL_BYTE, SENTINEL_FLOAT = 0xA5, np.float32(-12345.5)


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def records(c):
    from stvo_amd import capi
    B, M = len(c["images"]), c["M"]
    rec = np.zeros((B, M), capi.KEYLINE_DTYPE)
    for b in range(B):
        ln = c["lines"][b][:M]
        for k, f in enumerate(("sx", "sy", "ex", "ey", "angle")):
            rec[f][b, :len(ln)] = ln[:, k]
        rec["num_pixels"][b, :len(ln)] = c["npx"][b][:M]
    n = np.array([len(l) for l in c["lines"]] if c["n_lines"] is None else c["n_lines"], np.int32)
    return rec, n


@pytest.mark.parametrize("name", list(CASES))
def test_planned_case(hip, oracle, name):
    import torch
    from stvo_amd import capi
    c = CASES[name]
    B, rows, cols = c["images"].shape
    M, exp, cnt = c["M"], ec.expected(c), ec.counts(c)
    lbd = capi.Lbd(hip, B, cols, rows, max_keylines=M)
    try:
        if c["size"] is not None:
            lbd.set_image_sizes([c["size"]])
        if c["n_lines"] is None:                                    # the host entry
            got, got_f = lbd.compute(c["images"], c["lines"], c["npx"], want_float=True)
            for b in range(B):
                assert bits_equal(got_f[b], exp[b]["desc_f"]), ("statement, floats", name, b)
                assert np.array_equal(got[b], exp[b]["desc"]), ("statement, bytes", name, b)
        # the device entry: n_lines as the case gives them, outputs filled with sentinels
        rec, n = records(c)
        t_img = torch.from_numpy(np.ascontiguousarray(c["images"])).cuda()
        t_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
        t_n = torch.from_numpy(n).cuda()
        t_desc = torch.full((B, M, 32), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
        t_f = torch.full((B, M, 72), float(SENTINEL_FLOAT), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        lbd.compute_dev(t_img.data_ptr(), t_rec.data_ptr(), t_n.data_ptr(), t_desc.data_ptr(), t_f.data_ptr())
        hip.synchronize()
        d, f = t_desc.cpu().numpy(), t_f.cpu().numpy()
        for b in range(B):
            k = cnt[b]
            im = c["images"][b] if c["size"] is None else np.ascontiguousarray(c["images"][b][:c["size"][1], :c["size"][0]])
            orc, orc_f = oracle.lbd_compute(im, c["lines"][b][:k], c["npx"][b][:k], want_float=True)
            assert bits_equal(f[b, :k], exp[b]["desc_f"]), ("statement, floats", name, b)
            assert np.array_equal(d[b, :k], exp[b]["desc"]), ("statement, bytes", name, b)
            assert bits_equal(f[b, :k], orc_f) and np.array_equal(d[b, :k], orc), ("oracle", name, b)
            assert np.all(d[b, k:] == SENTINEL_BYTE) and np.all(f[b, k:] == SENTINEL_FLOAT), ("rows beyond n_lines", name, b)
    finally:
        lbd.close()
