"""bench.py's command line on the GPU: a plain run measures the headline alone (no kernel events, no roofline, no
CPU baseline) and --dump-outputs writes what its last timed step decoded, the same from run to run; --full adds
the roofline and the CPU baseline. Small batches of the C1 config (regular (3,6) N=8000 IB, i_max = 10)."""
import json
import os

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu
ARGS = ["--gpus", "1", "--config", "C1", "--batch-per-gpu", "64", "--warmup", "1"]


def _run(capsys, argv):
    bench.main(argv)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_its_outputs(capsys, tmp_path):
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    line = _run(capsys, ARGS + ["--steps", "3", "--dump-outputs", d1])
    assert line["full"] is False and line["roofline"] is None and line["cpu_baseline"] is None
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "codewords/s" and line["dtype"] == "u4"
    assert line["ms_per_step"] > 0
    # value = codewords per second of the timed steps: B / ms_per_step (both rounded in the line)
    assert line["value"] == pytest.approx(64 / (line["ms_per_step"] * 1e-3), rel=0.02)
    assert sorted(os.listdir(d1)) == ["decoded.npy", "decoded_columns.npy", "stop_iteration.npy"]
    out = np.load(os.path.join(d1, "decoded.npy"))
    cols = np.load(os.path.join(d1, "decoded_columns.npy"))
    stop = np.load(os.path.join(d1, "stop_iteration.npy"))
    assert out.dtype == np.float32 and out.shape == (8000, 64)
    assert cols.dtype == np.float64 and np.array_equal(cols, np.arange(64))
    assert stop.dtype == np.float32 and stop.tolist() == [line["stop_iteration"]["max"]] == [9.0]
    assert np.array_equal(out, np.round(out)) and out.min() >= 0 and out.max() <= 15      # cluster ids
    # the dump is the batch the line's error count was taken from (all-zero codeword: clusters 0..7 are errors)
    data_len = line["decoded_bits"] // 64
    assert int((out[:data_len] < 8).sum()) == line["decoded_bit_errors"]
    # same arguments, same inputs: a second run (another number of steps) decodes the same outputs
    _run(capsys, ARGS + ["--steps", "1", "--dump-outputs", d2])
    for f in ("decoded.npy", "decoded_columns.npy", "stop_iteration.npy"):
        assert np.array_equal(np.load(os.path.join(d1, f)), np.load(os.path.join(d2, f))), f


def test_full_run_adds_roofline_and_cpu_baseline(capsys, monkeypatch):
    for v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):     # the baseline's workers set them
        monkeypatch.setenv(v, os.environ.get(v, "1"))
    line = _run(capsys, ARGS + ["--steps", "2", "--full", "--cpu-sample", "8", "--cpu-procs", "2"])
    assert line["full"] is True and line["steps"] == 2 and line["ms_per_step"] > 0
    roof = line["roofline"]
    assert roof["avg_launch_ms"] > 0 and 0 < roof["frac"] <= 1
    cpu = line["cpu_baseline"]
    assert cpu["value"] > 0 and cpu["cores"] == 2 and "outputs equal GPU: True" in cpu["sample"]
