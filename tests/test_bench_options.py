"""CPU: bench.py's --full and --dump-outputs.  A plain run measures the headline
only (the CPU baselines and the companion timings are --full's); --dump-outputs
writes float32 / float64 .npy files within its byte budget, a larger array as the
same seeded sample of its elements every time."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _parse(b, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return b.parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    b = _bench()
    a = _parse(b, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.no_cpu_baseline and not a.fp32_companion and not a.config_companions
    for mode in ("rollout", "loop"):
        assert _parse(b, monkeypatch, "--mode", mode).no_cpu_baseline


def test_full_runs_every_leg_unless_one_is_dropped(monkeypatch):
    b = _bench()
    a = _parse(b, monkeypatch, "--full")
    assert a.full and not a.no_cpu_baseline and a.fp32_companion and a.config_companions
    a = _parse(b, monkeypatch, "--full", "--no-cpu-baseline", "--no-fp32-companion")
    assert a.no_cpu_baseline and not a.fp32_companion and a.config_companions


def test_dump_outputs_writes_float_arrays(tmp_path):
    b = _bench()
    arrays = {"f32": torch.arange(12, dtype=torch.float32).reshape(3, 4),
              "f64": torch.linspace(0, 1, 5, dtype=torch.float64),
              "i64": torch.tensor([[3], [-2]]),
              "bf16": torch.tensor([1.5, -0.25], dtype=torch.bfloat16),
              "absent": None}
    b.dump_outputs(str(tmp_path / "out"), arrays)
    got = {p.name: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert sorted(got) == ["bf16.npy", "f32.npy", "f64.npy", "i64.npy"]
    assert got["f32.npy"].dtype == np.float32 and got["f32.npy"].shape == (3, 4)
    assert got["f64.npy"].dtype == np.float64
    assert got["i64.npy"].dtype == np.float32 and got["i64.npy"].tolist() == [[3.0], [-2.0]]
    assert got["bf16.npy"].dtype == np.float32 and got["bf16.npy"].tolist() == [1.5, -0.25]
    assert np.array_equal(got["f32.npy"], arrays["f32"].numpy())
    assert np.array_equal(got["f64.npy"], arrays["f64"].numpy())


def test_dump_outputs_samples_within_the_budget(tmp_path):
    b = _bench()
    assert b.DUMP_BUDGET_BYTES == 64 * 2 ** 20
    big = torch.arange(1000, dtype=torch.float32)
    small = torch.arange(10, dtype=torch.float64)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, budget=800)
    a_big, b_big = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(a_big, b_big)                       # the same elements every run
    assert a_big.shape == (100,) and len(set(a_big.tolist())) == 100
    assert np.all(np.diff(a_big) > 0) and 0 <= a_big[0] and a_big[-1] < 1000
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())  # under its share: whole
    assert a_big.nbytes + small.numpy().nbytes <= 800


def test_steps_below_one_are_rejected(monkeypatch):
    import pytest
    b = _bench()
    for bad in (("--steps", "0"), ("--steps", "-3"), ("--warmup", "-1")):
        with pytest.raises(SystemExit):
            _parse(b, monkeypatch, *bad)
    assert _parse(b, monkeypatch, "--steps", "1", "--warmup", "0").steps == 1
