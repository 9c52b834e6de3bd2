"""One image size, and length threshold, per image in the FLD key-line detector (stvo_fld_set_image_sizes, the MIXED instances of
csrc/fld_kernels.hip): every image of a batch of slots 160 x 120 must come back, bit for bit, as the CPU statement tests/cpp/fld_ref.c
gives it for the crop and as a detector created at that image's own size with that threshold returns it — the edge map, the raw
segments in detection order, the counts, the key-line records and the responses — while the rest of every slot holds noise.

The ten crops: 16 x 16 (the minimum), 33 x 47 (odd on both sides, words straddle rows), 64 x 64 (exactly one counting-sort unit of
4096), 65 x 63 (4095 pixels, a partial last word), 97 x 120 (full height), 160 x 61 (full width), 47 x 118 (cols < rows: the response
divisor flips against the slot's), the slot itself, 159 x 119, 96 x 43.  Crop i has the threshold max(1, int(0.05 min(c, r))) — 1 … 6 —
under a detector created at 1.

A detector that ignored the sizes (or took the slot's border, corner quirk, neighbours, clamps or pixel count) must fail; the first test
states on the CPU what that rests on, before anything touches the GPU."""
import numpy as np
import pytest

import fld_statement
from stvo_amd import synth
from test_gpu_fld import same_f32

pytestmark = pytest.mark.gpu

SLOT = (160, 120)                                                      # cols, rows
CROPS = [(16, 16), (33, 47), (64, 64), (65, 63), (97, 120), (160, 61), (47, 118), (160, 120), (159, 119), (96, 43)]
B, K, L_DET, NF_CUT = 10, 512, 1, 10
NFS = [0, NF_CUT]

_images = {}
_refs = {}
_uniform = {}


@pytest.fixture(scope="module")
def stmt():
    return fld_statement.load()


def image(k):
    if k not in _images:
        c, r = CROPS[k]
        _images[k] = synth.make_image(300 + 10 * k, c, r, n_rects=max(6, c * r // 300), n_discs=max(2, c * r // 1500))
        assert _images[k].shape == (r, c)
    return _images[k]


def threshold(k):
    return max(1, int(0.05 * min(CROPS[k])))


def reference(stmt, k, nf):
    """the statement for crop k at its own threshold, computed once"""
    if (k, nf) not in _refs:
        img, L = image(k), threshold(k)
        rec, resp, found = stmt.keylines(img, L, nf, K)
        _refs[(k, nf)] = dict(edges=stmt.edges(img), segs=stmt.segments(img, L), rec=rec, resp=resp, found=found)
    return _refs[(k, nf)]


def slots(ks, noise):
    """[B][rows][cols]: seeded noise (or zeros) everywhere, then crop ks[i % len(ks)] top-left in slot i"""
    rng = np.random.default_rng(78)
    buf = rng.integers(0, 256, (B, SLOT[1], SLOT[0])).astype(np.uint8)
    if not noise:
        buf[:] = 0
    for i in range(B):
        c, r = CROPS[ks[i % len(ks)]]
        buf[i, :r, :c] = image(ks[i % len(ks)])
    return buf


def near_border(seg, size):
    return len(seg) > 0 and bool(np.any((np.maximum(seg[:, 0], seg[:, 2]) >= size[0] - 8) | (np.maximum(seg[:, 1], seg[:, 3]) >= size[1] - 8)))


def run(fld, buf):
    """everything a detection leaves, through the host entry points"""
    det = fld.detect(buf)
    counts = fld.counts().copy()
    edges = fld.edges(buf)
    segs, n = fld.segments(buf)
    return dict(det=det, counts=counts, edges=edges, segs=segs, n=n.copy())


def uniform(hip, k, nf):
    """a detector created at crop k's own size and threshold, on the crop alone; computed once"""
    from stvo_amd import capi
    if (k, nf) not in _uniform:
        c, r = CROPS[k]
        fld = capi.Fld(hip, 1, c, r, capi.fld_params(threshold(k), nfeatures=nf), max_keylines=K)
        try:
            _uniform[(k, nf)] = run(fld, image(k)[None])
        finally:
            fld.close()
    return _uniform[(k, nf)]


def same_run(a, i, b, j, what):
    (rec, resp), (urec, uresp) = a["det"][i], b["det"][j]
    assert len(rec) == len(urec), (what, len(rec), len(urec))
    assert rec.tobytes() == urec.tobytes() and resp.tobytes() == uresp.tobytes(), what
    assert (a["counts"][i], a["n"][i]) == (b["counts"][j], b["n"][j]), what
    assert a["segs"][i].tobytes() == b["segs"][j].tobytes(), what


def check(hip, stmt, fld, ks, nf, noise=True, lengths=True):
    """one table of the crops ks, one run, every image against the statement and against its uniform detector"""
    fld.set_image_sizes([CROPS[k] for k in ks], [threshold(k) for k in ks] if lengths else None)
    out = run(fld, slots(ks, noise))
    for i in range(B):
        k = ks[i % len(ks)]
        (c, r), what = CROPS[k], (i, CROPS[k], threshold(k), nf, noise)
        ref = reference(stmt, k, nf)
        want = np.zeros((SLOT[1], SLOT[0]), np.uint8)
        want[:r, :c] = ref["edges"]
        assert np.array_equal(out["edges"][i], want), what                      # the crop's edge map top-left, 0 around it
        assert out["n"][i] == len(ref["segs"]) == out["counts"][i] == ref["found"], what
        assert same_f32(out["segs"][i], ref["segs"]), what
        rec, resp = out["det"][i]
        assert len(rec) == len(ref["rec"]) and rec.tobytes() == ref["rec"].tobytes(), what
        assert same_f32(resp, ref["resp"]), what
        uni = uniform(hip, k, nf)
        same_run(out, i, uni, 0, ("uniform",) + what)
        assert np.array_equal(out["edges"][i, :r, :c], uni["edges"][0]), what
    return out


def test_what_the_check_rests_on(stmt):
    """on the CPU, before the GPU: every crop yields segments, one of them ends near the crop's own right or bottom border, and the
    crop's edge map is not the crop region of the edge map of its noise-filled slot — so the slot's border, corner quirk or neighbours,
    leaked into an image, cannot pass"""
    buf = slots(list(range(B)), noise=True)
    counts = []
    for k, (c, r) in enumerate(CROPS):
        ref = reference(stmt, k, 0)
        counts.append(len(ref["segs"]))
        assert len(ref["segs"]) >= 1 and ref["found"] == len(ref["segs"]) <= K, (k, len(ref["segs"]))
        assert near_border(ref["segs"], (c, r)), k
        if (c, r) != SLOT:
            differ = int(np.count_nonzero(stmt.edges(buf[k])[:r, :c] != ref["edges"]))
            print("crop %d x %d: %d segments, edge map differs from the slot's in %d pixels" % (c, r, len(ref["segs"]), differ))
            assert 10 <= differ <= 95, (k, differ)
    assert counts[0] == 1 and max(counts) == 88 and max(counts) > NF_CUT > min(counts), counts
    assert sorted({threshold(k) for k in range(B)}) == [1, 2, 3, 4, 5, 6]
    assert CROPS[6][0] < CROPS[6][1] and SLOT[0] > SLOT[1]                      # the response divisor flips
    assert CROPS[2][0] * CROPS[2][1] == 4096 and CROPS[3][0] * CROPS[3][1] == 4095


@pytest.mark.parametrize("nf", NFS, ids=["uncut", "cut"])
def test_every_image_is_its_own_crop(hip, stmt, nf):
    from stvo_amd import capi
    everyone = list(range(B))
    fld = capi.Fld(hip, B, SLOT[0], SLOT[1], capi.fld_params(L_DET, nfeatures=nf), max_keylines=K)
    try:
        noisy = check(hip, stmt, fld, everyone, nf)                             # n = B, and the first call of a new detector
        clean = check(hip, stmt, fld, everyone, nf, noise=False)                # the bytes outside the images influence nothing
        for i in range(B):
            same_run(noisy, i, clean, i, ("zero-filled", i))
        assert np.array_equal(noisy["edges"], clean["edges"])
        check(hip, stmt, fld, everyone[:5], nf)                                 # n = B / 2: images i and i + 5 share an entry
        check(hip, stmt, fld, everyone[5:], nf)
        check(hip, stmt, fld, everyone[::-1], nf)                               # every slot changes its size: nothing of the last run is in reach
        # no list of thresholds: the detector's own for every entry
        fld.set_image_sizes([CROPS[k] for k in everyone])
        own = fld.detect(slots(everyone, True))
        for k in everyone:
            rec, resp, _ = stmt.keylines(image(k), L_DET, nf, K)
            assert own[k][0].tobytes() == rec.tobytes() and same_f32(own[k][1], resp), k
        # no table: every image fills its slot, noise included, as on a detector that never had one
        fld.set_image_sizes(None)
        buf = slots(everyone, True)
        full = run(fld, buf)
        never = capi.Fld(hip, B, SLOT[0], SLOT[1], capi.fld_params(L_DET, nfeatures=nf), max_keylines=K)
        try:
            ref = run(never, buf)
        finally:
            never.close()
        for i in range(B):
            same_run(full, i, ref, i, ("no table", i))
        assert np.array_equal(full["edges"], ref["edges"])
        assert np.array_equal(full["edges"][3], stmt.edges(buf[3]))
    finally:
        fld.close()


def test_two_tables_without_a_synchronisation(hip, stmt):
    """a second table set behind a detection that has only been enqueued: each detection reads its own (the table travels on the
    context's stream, the staging blocks alternate)"""
    import torch
    from stvo_amd import capi
    tables = [list(range(B)), list(range(B))[::-1], [5, 6, 7, 8, 9], [2, 0]]
    fld = capi.Fld(hip, B, SLOT[0], SLOT[1], capi.fld_params(L_DET, nfeatures=0), max_keylines=K)
    try:
        dev = [dict(img=torch.from_numpy(slots(ks, True)).cuda(), rec=torch.zeros(B * K * capi.KEYLINE_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
                    resp=torch.zeros(B * K, dtype=torch.float32, device="cuda"), n=torch.zeros(B, dtype=torch.int32, device="cuda"))
               for ks in tables]
        torch.cuda.synchronize()
        for ks, t in zip(tables, dev):   # enqueued back to back; the first of them is the detector's first call
            fld.set_image_sizes([CROPS[k] for k in ks], [threshold(k) for k in ks])
            fld.detect_dev(t["img"].data_ptr(), t["rec"].data_ptr(), t["resp"].data_ptr(), t["n"].data_ptr())
        hip.synchronize()
        for ks, t in zip(tables, dev):
            n = t["n"].cpu().numpy()
            rec = t["rec"].cpu().numpy().view(capi.KEYLINE_DTYPE).reshape(B, K)
            resp = t["resp"].cpu().numpy().reshape(B, K)
            for i in range(B):
                ref = reference(stmt, ks[i % len(ks)], 0)
                assert n[i] == len(ref["rec"]) and rec[i, :n[i]].tobytes() == ref["rec"].tobytes(), (ks, i)
                assert same_f32(resp[i, :n[i]], ref["resp"]), (ks, i)
    finally:
        fld.close()


def test_refusals_leave_the_table_in_force(hip, stmt):
    from stvo_amd import capi
    everyone = list(range(B))
    fld = capi.Fld(hip, B, SLOT[0], SLOT[1], capi.fld_params(L_DET, nfeatures=0), max_keylines=K)
    six = capi.Fld(hip, 2, SLOT[0], SLOT[1], capi.fld_params(6, nfeatures=0), max_keylines=K)
    try:
        before = check(hip, stmt, fld, everyone, 0)
        bad = [[(160, 120)] * 3,                      # B % n != 0
               [(160, 120)] * 11,                     # n > B
               [(161, 120)], [(160, 121)],            # larger than the slot
               [(15, 64)], [(64, 15)],                # below what stvo_fld_create takes
               [(160, 120), (64, 64), (64, 4), (64, 64), (64, 64)]]
        for sizes in bad:
            with pytest.raises(capi.StvoError):
                fld.set_image_sizes(sizes)
        with pytest.raises(capi.StvoError):
            fld.set_image_sizes(CROPS[:5], [1, 2, 0, 4, 5])                     # L_i < 1
        lib = hip.lib
        one = np.array([[64, 64]], np.int32)
        assert lib.stvo_fld_set_image_sizes(fld.h, one.ctypes.data, None, 0) == -1       # n <= 0: STVO_ERR_INVALID_ARG
        assert lib.stvo_fld_set_image_sizes(fld.h, one.ctypes.data, None, -1) == -1
        assert lib.stvo_fld_set_image_sizes(None, one.ctypes.data, None, 1) == -1
        with pytest.raises(ValueError):
            fld.set_image_sizes([160, 120])
        with pytest.raises(ValueError):
            fld.set_image_sizes(CROPS[:5], [1, 2])
        after = run(fld, slots(everyone, True))   # a refused call changes nothing: the previous table, thresholds included, is in force
        for i in range(B):
            same_run(after, i, before, i, ("refused", i))
        assert np.array_equal(after["edges"], before["edges"])
        # the store rule: a detector created at 6 holds 19200 / 7 + 1 = 2743 segment slots per image
        six.set_image_sizes([(97, 120), (160, 120)], [4, 6])                    # 2329 and, with equality, 2743
        held = six.detect(slots([4, 7], True)[:2])
        with pytest.raises(capi.StvoError, match=r"(?s)entry 1 .*3154.*2743") as e:
            six.set_image_sizes([(97, 120), (159, 119)], [4, 5])
        assert "(-4)" in str(e.value) or "capacity" in str(e.value).lower()
        again = six.detect(slots([4, 7], True)[:2])
        for i, k in enumerate((4, 7)):
            assert again[i][0].tobytes() == held[i][0].tobytes() and again[i][1].tobytes() == held[i][1].tobytes()
            assert held[i][0].tobytes() == stmt.keylines(image(k), (4, 6)[i], 0, K)[0].tobytes()
    finally:
        fld.close()
        six.close()
