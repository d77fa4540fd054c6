"""bench.py's plain run and its options: --steps is the number of timed steps (one region unless --full or --regions),
--dump-outputs writes the last timed step's outputs, and a plain run reports the headline only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_regions_default_to_one_plain_and_fifteen_with_full():
    assert bench.parse([]).regions == 1 and not bench.parse([]).full
    assert bench.parse(["--full"]).regions == 15
    assert bench.parse(["--full", "--regions", "3"]).regions == 3
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"


def test_dump_outputs_float32_and_a_fixed_sample_of_large_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    big = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    small = torch.tensor([-3, 5], dtype=torch.int8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small, "wide": big.double()[:1]})
    a = np.load(tmp_path / "a" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (100,)
    assert np.all(np.diff(a) > 0) and len(set(a.tolist())) == 100        # distinct elements in index order
    assert np.array_equal(a, np.load(tmp_path / "b" / "big.npy"))          # the same positions in every run
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.tolist() == [-3.0, 5.0]
    w = np.load(tmp_path / "a" / "wide.npy")
    assert w.dtype == np.float64 and w.shape == (1, 100)


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--batch", "4", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["steps"] == 3 and res["regions"]["n"] == 1 and res["ms_per_step"] > 0
    assert abs(res["value"] - 4 / res["ms_per_step"] * 1e3) < 1e-6 * res["value"]
    assert not {"roofline", "e2e", "configs", "cpu_baseline"} & set(res)
    y = np.load(out / "output.npy")
    assert y.dtype == np.float32 and y.shape == (4, 64 * 64, 64) and np.isfinite(y).all()
    r = np.load(out / "output_range.npy")
    assert r.dtype == np.float32 and r.shape == (2,) and np.isfinite(r).all() and r[0] < r[1]
