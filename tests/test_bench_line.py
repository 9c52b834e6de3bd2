"""The ONE stdout line of bench.py must stay short: the driver keeps a bounded tail of stdout, and round 5's 20 KB line was recorded as
`"parsed": null` — the round's headline went unmeasured.  short_line() is fed the largest record a run has produced (round 5's own,
profiles/r05_bench.json.txt) and a record bloated far beyond it."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (top level of bench.py imports nothing that needs a GPU)

REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
            "config", "roofline", "cpu_baseline")
ROOF = ("bound", "achieved", "peak", "unit", "frac", "traffic")


def _round5_record():
    for ln in open(os.path.join(ROOT, "profiles", "r05_bench.json.txt")):
        if ln.startswith("{"):
            return json.loads(ln)
    raise AssertionError("profiles/r05_bench.json.txt holds no JSON line")


def _check(line):
    assert "\n" not in line and len(line) < bench.SHORT_LINE_MAX, len(line)
    out = json.loads(line)
    for k in REQUIRED:
        assert k in out, k
    for k in ROOF:
        assert k in out["roofline"], k
    assert out["roofline"]["bound"] in ("hbm", "mfma")
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in out["cpu_baseline"], k
    assert "workload" in out["config"] and "model" not in out["config"]
    return out


def test_short_line_of_the_round_5_record_fits():
    full = _round5_record()
    assert len(json.dumps(full)) > 15000          # the record that cost round 5 its driver measurement
    out = _check(bench.short_line(full))
    assert abs(out["value"] - full["value"]) / full["value"] < 1e-5
    assert abs(out["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-5
    assert out["config"]["value_clustered"] > 0
    assert out["cpu_baseline"]["speedup_vs_1_core"]["seq_push"] > 1
    assert out["legs"]["orb_images_per_s"] > 0 and out["legs"]["lsd_one_image_ms"] > 0 and out["legs"]["configs3_gn_frame_pairs_per_s"] > 0


def test_short_line_survives_bloat_and_failed_legs():
    full = _round5_record()
    for k in list(full):
        if isinstance(full[k], dict):
            full[k]["note"] = "x" * 5000            # prose never reaches the line
            full[k]["another_leg"] = {"rows": list(range(500))}
    full["config"]["workload"] = full["config"]["workload"][:300]
    full["orb_front_end"] = {"error": "StvoError: out of memory"}
    full["per_rank_frame_pairs_per_s"] = [1.25e6] * 8
    full["n_gpus"] = full["rccl_ranks"] = 8
    out = _check(bench.short_line(full))
    assert out["legs"]["orb_images_per_s"] == "error"
    assert len(out["per_rank_frame_pairs_per_s"]) == 8


def test_short_line_without_extras_or_cpu_baseline():
    full = _round5_record()
    for k in ("cpu_baseline", "latency", "configs1", "configs3", "orb_front_end", "lsd_front_end", "images_to_poses", "images_to_poses_with_lines",
              "reverse_check_correlated", "headline_clustered"):
        full.pop(k, None)
    line = bench.short_line(full)
    out = json.loads(line)
    assert len(line) < bench.SHORT_LINE_MAX and "cpu_baseline" not in out and "legs" not in out and out["roofline"]["frac"] > 0


def test_write_extras_round_trip(tmp_path):
    full = _round5_record()
    p = tmp_path / "bench_extras.json"
    bench.write_extras(full, str(p))
    assert json.load(open(p))["value"] == full["value"]


def _pose_results(n):
    from stvo_amd.ctypes_types import POSE_RESULT_DTYPE
    res = np.zeros(n, POSE_RESULT_DTYPE)
    res["T"] = np.arange(n * 16, dtype=np.float64).reshape(n, 16)
    res["status"] = np.arange(n) % 4
    res["iters"] = np.arange(2 * n, dtype=np.int32).reshape(n, 2)
    return res, np.arange(4 * n, dtype=np.int32).reshape(n, 4)


def test_dump_outputs_writes_every_field_as_float64(tmp_path):
    res, counts = _pose_results(10)
    bench.dump_outputs(str(tmp_path / "d"), res, counts)
    names = {p.name for p in (tmp_path / "d").iterdir()}
    assert names == {f"{k}.npy" for k in res.dtype.names} | {"counts.npy"}
    T = np.load(tmp_path / "d" / "T.npy")
    assert T.dtype == np.float64 and T.shape == (10, 16) and np.array_equal(T, res["T"])
    assert np.array_equal(np.load(tmp_path / "d" / "iters.npy"), res["iters"])
    assert np.array_equal(np.load(tmp_path / "d" / "counts.npy"), counts)


def test_dump_outputs_samples_past_the_size_limit(tmp_path, monkeypatch):
    res, counts = _pose_results(1000)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100 * 1000)
    for k in range(2):
        bench.dump_outputs(str(tmp_path / f"d{k}"), res, counts)
    assert sum(p.stat().st_size for p in (tmp_path / "d0").iterdir()) <= 100 * 1000 + 128 * 20
    rows = np.load(tmp_path / "d0" / "stream_index.npy").astype(np.int64)
    assert 0 < len(rows) < 1000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "d1" / "stream_index.npy"))   # a fixed sample
    assert np.array_equal(np.load(tmp_path / "d0" / "T.npy"), res["T"][rows])
    assert np.array_equal(np.load(tmp_path / "d0" / "counts.npy"), counts[rows])


def test_short_line_of_a_plain_run():
    """Without --full the record holds the headline alone: the line keeps the contract's keys and their meaning."""
    import argparse
    streams = [[{"kp_l": np.zeros((100, 2)), "kp_r": np.zeros((90, 2)), "kl_l": np.zeros((10, 4))} for _ in range(4)] for _ in range(8)]
    args = argparse.Namespace(steps=3, warmup=2)
    full = bench.headline_record(args, 1, None, 8 * 3, 0.006, [0.006], None, streams, 1.0)
    out = json.loads(bench.short_line(full))
    assert out["metric"] == "stereo frames/s (match+optimizePose)" and out["unit"] == "frame-pairs/s" and out["higher_is_better"] is True
    assert out["dtype"] == "u8/fp4+f64" and out["steps"] == 3 and out["warmup"] == 2 and out["repeats"]["n"] == 1
    assert out["value"] == pytest.approx(4000.0) and out["ms_per_step"] == pytest.approx(2.0)
    assert out["config"]["streams_per_gpu"] == 8 and out["config"]["keypoints_per_image"] == 95.0
    assert "roofline" not in out and "cpu_baseline" not in out and out["parity_sampled"] is None
