"""Feature tracks per stream on the CPU: csrc/track_update.h compiled for the host (tests/cpp/track_host.cpp) against the plain
statement tests/np_tracks.py — every field of every row exactly, rows at or beyond the count untouched —, the ctypes twins against
sizeof in C, and the new symbols of the library.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_tracks
import track_host_lib as th
from np_tracks import PARK, RESTART, RUN, TRACK

COUNTS = [0, 1, 63, 64, 65, 300, 2048]   # 2048: STVO_POSE_MAX_POINTS, the capacity


def random_state(rng, n, age_hi=100):
    s = np.zeros(n, TRACK)
    s["idx"] = rng.integers(0, 5000, n)
    s["age"] = rng.integers(0, age_hi, n)
    s["kf"] = rng.integers(0, 2, n)
    s["inlier"] = rng.integers(-1, 2, n)
    return s


def random_matches(rng, n_prev, n_cur):
    """About half of the previous features matched, into a third of the current ones: duplicates are the rule."""
    if n_cur == 0:
        return np.full(n_prev, -1, np.int32), rng.integers(-1, 2, n_prev).astype(np.int32)
    m12 = np.where(rng.random(n_prev) < 0.5, rng.integers(0, (n_cur + 2) // 3, n_prev), -1).astype(np.int32)
    return m12, rng.integers(0, 2, n_prev).astype(np.int32)


def both(prev, m12, inl, n_cur, lanes=1, **kw):
    want = np_tracks.step(prev, m12, inl, n_cur, **kw)
    got = th.step(prev, m12, inl, n_cur, lanes=lanes, cap=n_cur + 3, **kw)
    for w, g in zip(want, got):
        assert g[:n_cur].tobytes() == w.tobytes()
        assert (g[n_cur:] == th.SENTINEL).all()          # rows at or beyond the count are not written
    return want


def test_sizes_equal_sizeof_in_c():
    from stvo_amd.ctypes_types import KF_HEADER_DTYPE, KfHeader, TRACK_DTYPE, Track
    assert th.sizes() == (8, 16)
    assert (C.sizeof(Track), C.sizeof(KfHeader)) == th.sizes() == (TRACK_DTYPE.itemsize, KF_HEADER_DTYPE.itemsize)
    assert TRACK_DTYPE == TRACK
    assert [(n, TRACK_DTYPE.fields[n][1]) for n in TRACK_DTYPE.names] == [("idx", 0), ("age", 4), ("kf", 6), ("inlier", 7)]
    assert [getattr(Track, n).offset for n in ("idx", "age", "kf", "inlier")] == [0, 4, 6, 7]


@pytest.mark.parametrize("n_cur", COUNTS)
@pytest.mark.parametrize("n_prev", COUNTS)
def test_propagation_with_duplicates(n_prev, n_cur):
    rng = np.random.default_rng(1000 * n_prev + n_cur)
    prev = random_state(rng, n_prev)
    m12, inl = random_matches(rng, n_prev, n_cur)
    for lanes in (1, 64, 256):
        both(prev, m12, inl, n_cur, lanes=lanes)
    if n_prev >= 63 and n_cur >= 63:
        matched = m12[m12 >= 0]
        assert len(np.unique(matched)) < len(matched)    # the case has duplicates


def test_largest_i1_wins_all_four_fields():
    prev = np.array([(10, 1, 1, 0), (20, 2, 0, 0), (30, 3, 1, 0), (40, 4, 0, 0)], TRACK)
    m12 = np.array([2, 0, 2, 2], np.int32)
    inl = np.array([1, 1, 0, 1], np.int32)
    rec, state = both(prev, m12, inl, 3, lanes=64)
    assert rec[2].tolist() == (40, 5, 0, 1)              # i1 = 3, not 0 or 2
    assert rec[0].tolist() == (20, 3, 0, 1)
    assert rec[1].tolist() == (1, 0, 0, -1)              # unmatched: its own position
    assert state.tobytes() == rec.tobytes()


def test_age_saturates():
    prev = np.array([(5, 65533, 1, 1), (6, 65534, 1, 1), (7, 65535, 1, 1)], TRACK)
    m12 = np.array([0, 1, 2], np.int32)
    rec, _ = both(prev, m12, np.ones(3, np.int32), 3)
    assert rec["age"].tolist() == [65534, 65535, 65535]
    rec, _ = both(rec, m12, np.ones(3, np.int32), 3)
    assert rec["age"].tolist() == [65535, 65535, 65535]


def test_keyframe_reset_then_propagation_from_it():
    rng = np.random.default_rng(7)
    prev = random_state(rng, 80)
    m12, inl = random_matches(rng, 80, 70)
    rec, state = both(prev, m12, inl, 70, new_kf=1)
    plain, _ = np_tracks.step(prev, m12, inl, 70, new_kf=0)
    assert rec.tobytes() == plain.tobytes()              # the record keeps the values from before the reset
    assert state["idx"].tolist() == list(range(70)) and (state["age"] == 0).all() and (state["kf"] == 1).all()
    m12b, inlb = random_matches(rng, 70, 65)
    rec2, _ = both(state, m12b, inlb, 65)
    hit = m12b[m12b >= 0]
    assert len(hit) and (rec2["kf"][hit] == 1).all() and (rec2["age"][hit] == 1).all()
    assert all(rec2["idx"][i2] == max(i1 for i1 in range(70) if m12b[i1] == i2) for i2 in set(hit.tolist()))
    un = np.setdiff1d(np.arange(65), hit)
    assert (rec2["kf"][un] == 0).all() and (rec2["idx"][un] == un).all() and (rec2["inlier"][un] == -1).all()


@pytest.mark.parametrize("n_cur", [0, 1, 65, 300])
def test_first_frame_restart_and_park(n_cur):
    rng = np.random.default_rng(n_cur)
    prev = random_state(rng, 90)
    m12, inl = random_matches(rng, 90, n_cur)            # present, and to be ignored
    for kw, kf in ((dict(first=True), 1), (dict(ctl=RESTART), 1), (dict(ctl=PARK), 0), (dict(ctl=PARK, new_kf=1), 0)):
        rec, state = both(prev, m12, inl, n_cur, lanes=64, **kw)
        assert rec["idx"].tolist() == list(range(n_cur)) and (rec["age"] == 0).all() and (rec["kf"] == kf).all() and (rec["inlier"] == -1).all()
        assert state.tobytes() == rec.tobytes()


def test_park_then_run_and_a_whole_chain():
    """np_tracks.Stream and the header side by side over a script with every control: first, RUN, key-frame, PARK, RUN, RESTART, RUN."""
    rng = np.random.default_rng(11)
    script = [(RUN, True, 0), (RUN, False, 0), (RUN, False, 1), (RUN, False, 0), (PARK, False, 0), (RUN, False, 0), (RESTART, False, 0),
              (RUN, False, 0)]
    ref = np_tracks.Stream()
    state = [np.zeros(0, TRACK), np.zeros(0, TRACK)]
    serials = []
    for ctl, first, new_kf in script:
        counts = (int(rng.integers(60, 130)), int(rng.integers(0, 40)))
        under_ctl = first or ctl != RUN
        n_prev = (0, 0) if under_ctl else (len(state[0]), len(state[1]))
        mi = [random_matches(rng, 2048 if k == 0 else 512, counts[k]) for k in range(2)]
        want = ref.step(counts, m12=(mi[0][0], mi[1][0]), inl=(mi[0][1], mi[1][1]), n_prev=n_prev, ctl=ctl, first=first, new_kf=new_kf)
        for k in range(2):
            rec, state[k] = th.step(state[k][:n_prev[k]], mi[k][0], mi[k][1], counts[k], ctl=ctl, first=first, new_kf=new_kf, lanes=256)
            assert rec.tobytes() == want[k].tobytes() and state[k].tobytes() == ref.state[k].tobytes()
        serials.append(ref.serial)
    assert serials == [1, 1, 2, 2, 2, 2, 1, 1]
    # the RUN behind the PARK propagated from the parked frame's rows: kf 0 everywhere
    assert (want[0]["kf"] == 0).sum() > 0


def test_sanitized_stand_alone_program():
    """tests/cpp/track_host_main.cpp: the header's functions on exact-size buffers under AddressSanitizer and UBSan, as a program of its own."""
    here = os.path.dirname(os.path.abspath(__file__))
    src, exe = os.path.join(here, "cpp", "track_host_main.cpp"), os.path.join(here, "cpp", "track_host_main")
    deps = [src, os.path.join(here, "cpp", "track_host.cpp")] + th.sources()[1]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout


def test_new_symbols_are_exported():
    from stvo_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    lib = capi.load()
    for name in ("stvo_seq_set_tracks", "stvo_seq_read_tracks", "stvo_seq_tracks_dev", "stvo_seq_keyframe_headers", "stvo_seq_read_keyframe"):
        assert name in capi.EXPORTS and hasattr(lib, name), name
