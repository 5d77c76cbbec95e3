"""CPU: driver.run_sequential issues the calls of the reference's training loop
(per_run.py:212-289) in the reference's order, driven with duck-typed fakes.

The runner adds 20 env steps per train run, the buffer can sample after two
inserts, the learner records its calls.  The expected traces below are written
out by hand from the reference's rules:

  * the loop runs while t_env <= t_max (:212), so the last iteration starts at 100;
  * train from the second iteration on (:218), priorities updated with + 1e-6 (:237-238);
  * tests when (t_env - last_test_T) / test_interval >= 1 from last_test_T = -41
    (:202,241): at 20, 60, 100 — max(1, 4 // 2) = 2 runs each (:240,255-256);
  * a checkpoint when model_save_time == 0 or 50 env steps later (:265-268):
    at 20, 80 — in a directory named by t_env (:270-272);
  * episode += batch_size_run (:281), then the "episode" log line when
    t_env - last_log_T >= 30 from last_log_T = 0 (:283-286): at 40, 80, 120;
  * accumulated_episodes = 4: an iteration whose next episode count is no multiple
    of 4 `continue`s once the buffer can sample (:220-222) — skipping its tests,
    its episode increment and its log line, so after the one update at episode 2 -> 4
    every later iteration is skipped, as in the reference.
"""
import os
import types

import pytest

from t2omca_amd.driver import run_sequential
from t2omca_amd.statlog import StatsLogger


class FakeBatch:
    def __init__(self, t=7):
        self.t = t

    def max_t_filled(self):
        return 5

    def __getitem__(self, item):
        assert item == (slice(None), slice(None, 5))
        return FakeBatch(5)


class FakeRunner:
    batch_size = 2

    def __init__(self, trace):
        self.trace, self.t_env = trace, 0

    def run(self, test_mode=False):
        if not test_mode:
            self.t_env += 20
        self.trace.append(("run", "test" if test_mode else "train", self.t_env))
        return FakeBatch()


class FakeBuffer:
    def __init__(self, trace):
        self.trace, self.inserts = trace, 0

    def insert_episode_batch(self, batch):
        assert isinstance(batch, FakeBatch)
        self.inserts += 1
        self.trace.append(("insert",))

    def can_sample(self, batch_size):
        assert batch_size == 3
        return self.inserts >= 2

    def sample(self, batch_size, t_env):
        self.trace.append(("sample", batch_size, t_env))
        return FakeBatch(), "idx", "weights"

    def update_priorities(self, idx, priorities, add=0.0):
        self.trace.append(("update_priorities", idx, priorities, add))


class FakeLearner:
    def __init__(self, trace):
        self.trace = trace

    def train(self, batch, t_env, episode, weights):
        assert batch.t == 5 and weights == "weights"  # truncated to the filled steps
        self.trace.append(("train", t_env, episode))
        return {"td_errors_abs": "prio"}

    def save_models(self, path):
        assert os.path.isdir(path)
        self.trace.append(("save", os.path.basename(path)))


class TraceLogger(StatsLogger):
    def __init__(self, trace):
        super().__init__(out=lambda line: None)
        self.trace = trace

    def log_stat(self, key, value, t):
        super().log_stat(key, value, t)
        self.trace.append(("log_stat", key, value, t))


def _train(t, episode):
    return [("sample", 3, t), ("train", t, episode), ("update_priorities", "idx", "prio", 1e-6)]


def _tests(t):
    return [("run", "test", t)] * 2


def _log(episode, t):
    return [("log_stat", "episode", episode, t)]


def _it(t):
    return [("run", "train", t), ("insert",)]


TRACE_FULL = (
    _it(20) + _tests(20) + [("save", "20")]                        # no sample yet; model_save_time == 0
    + _it(40) + _train(40, 2) + _log(4, 40)
    + _it(60) + _train(60, 4) + _tests(60)
    + _it(80) + _train(80, 6) + [("save", "80")] + _log(8, 80)
    + _it(100) + _train(100, 8) + _tests(100)
    + _it(120) + _train(120, 10) + _log(12, 120))

TRACE_ACCUMULATED = (
    _it(20) + _tests(20)                                           # episode 0 -> 2 (the buffer cannot sample yet)
    + _it(40) + _train(40, 2) + _log(4, 40)                        # next episode 4: a multiple of 4
    + _it(60) + _it(80) + _it(100) + _it(120))                     # next episode 6, never advanced: skipped


@pytest.mark.parametrize("extra,want", [({}, TRACE_FULL),
                                        ({"accumulated_episodes": 4, "save_model": False}, TRACE_ACCUMULATED)])
def test_run_sequential_call_trace(tmp_path, extra, want):
    trace = []
    args = types.SimpleNamespace(t_max=100, test_interval=40, log_interval=30, save_model=True, save_model_interval=50,
                                 test_nepisode=4, batch_size_run=2, batch_size=3, local_results_path=str(tmp_path),
                                 unique_token="tok")
    for k, v in extra.items():
        setattr(args, k, v)
    logger = TraceLogger(trace)
    runner = FakeRunner(trace)
    got = run_sequential(runner, FakeBuffer(trace), FakeLearner(trace), logger, args)
    assert got is logger
    assert trace == want, "\n".join(f"{i}: {a} | {b}" for i, (a, b) in enumerate(zip(trace, want)) if a != b)
    assert runner.t_env == 120
    saved = sorted(os.listdir(tmp_path / "models" / "tok")) if args.save_model else []
    assert saved == (["20", "80"] if args.save_model else [])
    assert [e for e in trace if e[0] == "update_priorities"] and all(
        e[3] == 1e-6 for e in trace if e[0] == "update_priorities")


def test_optional_args_default_off(tmp_path):
    """Only the required fields: no accumulation, no checkpoints."""
    trace = []
    args = types.SimpleNamespace(t_max=30, test_interval=1000, log_interval=1000, test_nepisode=2, batch_size_run=2,
                                 batch_size=3)
    run_sequential(FakeRunner(trace), FakeBuffer(trace), FakeLearner(trace), TraceLogger(trace), args)
    assert [e[0] for e in trace] == ["run", "insert", "run",                      # t_env 20, one test run
                                     "run", "insert", "sample", "train", "update_priorities"]
    assert not any(e[0] == "save" for e in trace)


def test_stats_logger():
    lines = []
    log = StatsLogger(out=lines.append)
    log.log_stat("return_mean", 2, 10)
    log.log_stat("return_mean", 3.5, 20)
    log.log_stat("episode", 4, 20)
    assert log.stats["return_mean"] == [(10, 2.0), (20, 3.5)]
    assert all(isinstance(v, float) for _, v in log.stats["return_mean"])
    log.print_recent_stats()
    assert len(lines) == 1 and "return_mean: 3.5000" in lines[0] and "20" in lines[0] and "\n" not in lines[0]
