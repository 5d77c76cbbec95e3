"""CPU: driver.run_sequential's start-up (per_run.py:159-198) and run-state files,
driven with the duck-typed fakes of tests/test_driver_host.py grown a state_dict.

The loop's settings are those of test_driver_host (20 env steps per train run,
t_max = 100, tests every 40, checkpoints every 50, the log line every 30), so its
hand-written TRACE_FULL is the straight run here too: checkpoints at t_env 20 and
80, and at 80 the checkpoint is followed by the "episode" log line of the SAME
iteration — the line a resumed run has to issue before its first rollout.
"""
import os
import types

import pytest
import torch

from t2omca_amd.driver import find_checkpoint, load_run_state, run_sequential, save_run_state
from t2omca_amd.statlog import StatsLogger
from tests.test_driver_host import (TRACE_FULL, FakeBuffer, FakeLearner, FakeRunner, TraceLogger, _it, _log, _tests,
                                    _train)


class FakeEnv:
    def __init__(self):
        self.normaliser = 0

    def state_dict(self):
        return {"format": 1, "normaliser": self.normaliser}

    def load_state_dict(self, sd):
        self.normaliser = sd["normaliser"]


class StateRunner(FakeRunner):
    test_nepisode = 4

    def __init__(self, trace):
        super().__init__(trace)
        self.env = FakeEnv()
        self.log_train_stats_t = -100000

    def run(self, test_mode=False):
        self.env.normaliser += 1
        return super().run(test_mode)

    def evaluate(self):
        for _ in range(max(1, self.test_nepisode // self.batch_size)):
            self.run(test_mode=True)

    def state_dict(self):
        return {"format": 1, "t_env": self.t_env, "log_train_stats_t": self.log_train_stats_t}

    def load_state_dict(self, sd):
        self.t_env, self.log_train_stats_t = sd["t_env"], sd["log_train_stats_t"]


class StateBuffer(FakeBuffer):
    def state_dict(self, include_data=True):
        return {"format": 1, "inserts": self.inserts, "include_data": include_data,
                "p": torch.arange(3, dtype=torch.float32)}

    def load_state_dict(self, sd):
        self.inserts = sd["inserts"] if sd["include_data"] else 0


class StateLearner(FakeLearner):
    def save_models(self, path):
        super().save_models(path)
        for name in ("agent.th", "mixer.th", "opt.th"):
            with open(os.path.join(path, name), "w") as f:
                f.write("model")

    def load_models(self, path):
        self.trace.append(("load_models", path))

    def state_dict(self):
        return {"format": 1, "updates": sum(e[0] == "train" for e in self.trace)}

    def load_state_dict(self, sd):
        self.updates = sd["updates"]


def _args(tmp_path, **extra):
    args = types.SimpleNamespace(t_max=100, test_interval=40, log_interval=30, save_model=True, save_model_interval=50,
                                 test_nepisode=4, batch_size_run=2, batch_size=3, local_results_path=str(tmp_path),
                                 unique_token="tok")
    for k, v in extra.items():
        setattr(args, k, v)
    return args


def _objects():
    trace = []
    return trace, StateRunner(trace), StateBuffer(trace), StateLearner(trace), TraceLogger(trace)


def _run(args):
    trace, runner, buffer, learner, logger = _objects()
    assert run_sequential(runner, buffer, learner, logger, args) is logger
    return trace, runner, buffer, learner, logger


def _stats(logger):
    return {k: list(v) for k, v in logger.stats.items()}


# ---- find_checkpoint (per_run.py:164-184) ------------------------------------------

def _dirs(tmp_path, *names):
    for n in names:
        (tmp_path / n).mkdir()


def test_find_checkpoint_picks_the_largest_step(tmp_path):
    _dirs(tmp_path, "20", "100", "9")  # numerically, not as strings ("9" > "100")
    assert find_checkpoint(str(tmp_path), 0) == (str(tmp_path / "100"), 100)


def test_find_checkpoint_picks_the_nearest_step(tmp_path):
    _dirs(tmp_path, "20", "80", "200")
    assert find_checkpoint(str(tmp_path), 90) == (str(tmp_path / "80"), 80)
    assert find_checkpoint(str(tmp_path), 150) == (str(tmp_path / "200"), 200)
    assert find_checkpoint(str(tmp_path), 1) == (str(tmp_path / "20"), 20)


def test_find_checkpoint_tie_goes_to_the_smaller_step(tmp_path):
    _dirs(tmp_path, "120", "80", "20")
    assert find_checkpoint(str(tmp_path), 100) == (str(tmp_path / "80"), 80)
    assert find_checkpoint(str(tmp_path), 50) == (str(tmp_path / "20"), 20)


def test_find_checkpoint_ignores_files_and_other_names(tmp_path):
    _dirs(tmp_path, "40", "latest", "60x", "-70")
    (tmp_path / "900").write_text("a file named by a number")
    assert find_checkpoint(str(tmp_path), 0) == (str(tmp_path / "40"), 40)
    assert find_checkpoint(str(tmp_path), 900) == (str(tmp_path / "40"), 40)


def test_find_checkpoint_missing_directory_is_none(tmp_path):
    assert find_checkpoint(str(tmp_path / "nowhere"), 0) is None
    trace, runner, buffer, learner, logger = _objects()
    args = _args(tmp_path, checkpoint_path=str(tmp_path / "nowhere"))
    assert run_sequential(runner, buffer, learner, logger, args) is logger
    assert trace == [] and runner.t_env == 0  # the reference logs and returns (:164-168)


def test_find_checkpoint_empty_directory_raises(tmp_path):
    _dirs(tmp_path, "notes")
    with pytest.raises(ValueError, match=str(tmp_path)):
        find_checkpoint(str(tmp_path), 0)


# ---- start-up ---------------------------------------------------------------------------

def test_weights_only_resume_is_the_reference_start(tmp_path):
    """No run state in the directory: load_models, t_env = step, counters from zero
    (:187-188, 201-205), then the ordinary loop — first test at once, the first
    checkpoint at once (model_save_time == 0), the episode count from 0."""
    ckpt = tmp_path / "ckpt"
    _dirs(tmp_path, "ckpt")
    _dirs(ckpt, "20", "60")
    trace, runner, *_ = _run(_args(tmp_path, checkpoint_path=str(ckpt), load_step=0, t_max=110))
    want = ([("load_models", str(ckpt / "60"))]
            + _it(80) + _tests(80) + [("save", "80")] + _log(2, 80)
            + _it(100) + _train(100, 2)
            + _it(120) + _train(120, 4) + _tests(120) + _log(6, 120))
    assert trace == want, "\n".join(f"{i}: {a} | {b}" for i, (a, b) in enumerate(zip(trace, want)) if a != b)
    assert runner.t_env == 120


def test_evaluate_runs_the_test_episodes_only(tmp_path):
    ckpt = tmp_path / "ckpt"
    _dirs(tmp_path, "ckpt")
    _dirs(ckpt, "20", "60")
    trace, runner, buffer, learner, logger = _run(_args(tmp_path, checkpoint_path=str(ckpt), load_step=25,
                                                        evaluate=True))
    # exactly the load, max(1, 4 // 2) = 2 test runs, the "episode" line with value t_env (:192-196)
    assert trace == [("load_models", str(ckpt / "20"))] + _tests(20) + _log(20, 20)
    assert runner.log_train_stats_t == runner.t_env == 20
    assert logger.stats["episode"] == [(20, 20.0)]
    assert not any(e[0] in ("train", "save", "insert", "sample") or e[:2] == ("run", "train") for e in trace)
    assert not (tmp_path / "models").exists()


def test_evaluate_without_checkpoint_path(tmp_path):
    trace, runner, *_ = _run(_args(tmp_path, evaluate=True))
    assert trace == _tests(0) + _log(0, 0) and runner.log_train_stats_t == 0


# ---- run state ---------------------------------------------------------------------------

@pytest.mark.parametrize("load_step,from_step", [(0, 80), (30, 20)])
def test_run_state_resume_equals_the_straight_run(tmp_path, load_step, from_step):
    """A straight run against fresh objects resumed from a checkpoint's run state:
    the calls after that checkpoint and the whole logger are equal — at 80 that
    includes the "episode" line of the checkpoint's own iteration."""
    trace, runner, buffer, learner, logger = _run(_args(tmp_path / "a", save_run_state=True, run_state_keep=0))
    assert trace == TRACE_FULL, "the run state changes no call of the loop"
    models = tmp_path / "a" / "models" / "tok"
    assert sorted(os.listdir(models / "80")) == ["agent.th", "mixer.th", "opt.th", "run_state.th"]
    cut = trace.index(("save", str(from_step))) + 1
    if from_step == 80:
        assert trace[cut] == ("log_stat", "episode", 8, 80)

    trace2, runner2, buffer2, learner2, logger2 = _run(_args(tmp_path / "b", save_run_state=True, run_state_keep=0,
                                                             checkpoint_path=str(models), load_step=load_step))
    assert trace2 == trace[cut:], "\n".join(f"{i}: {a} | {b}" for i, (a, b) in enumerate(zip(trace2, trace[cut:]))
                                           if a != b)
    assert _stats(logger2) == _stats(logger)
    assert (runner2.t_env, runner2.env.normaliser, buffer2.inserts) == (runner.t_env, runner.env.normaliser,
                                                                       buffer.inserts)
    assert learner2.updates == sum(e[0] == "train" for e in trace[:cut])
    assert not any(e[0] == "load_models" for e in trace2)


def test_run_state_holds_the_loop_counters_and_survives_weights_only_load(tmp_path):
    _run(_args(tmp_path, save_run_state=True, run_state_keep=0))
    name = tmp_path / "models" / "tok" / "80" / "run_state.th"
    state = torch.load(name, weights_only=True)  # plain containers and tensors only
    assert state["format"] == 1 and state["world_size"] == 1
    # written in mid-iteration: before `episode += 2` and before the log line at 80
    assert state["loop"] == {"episode": 6, "last_test_T": 60, "last_log_T": 40, "model_save_time": 80}
    assert set(state) >= {"env", "runner", "buffer", "learner", "logger", "loop", "world_size"}
    assert state["runner"]["t_env"] == 80
    assert torch.equal(state["buffer"]["p"], torch.arange(3, dtype=torch.float32))
    assert state["logger"]["stats"]["episode"] == [[40, 4.0]]


def test_save_replay_buffer_false_becomes_include_buffer(tmp_path):
    _run(_args(tmp_path, save_run_state=True, save_replay_buffer=False))
    state = torch.load(tmp_path / "models" / "tok" / "80" / "run_state.th", weights_only=True)
    assert state["buffer"]["include_data"] is False


def test_run_state_keep_removes_older_run_states_only(tmp_path):
    models = tmp_path / "models" / "tok"
    _run(_args(tmp_path, save_run_state=True))  # run_state_keep = 1
    assert sorted(os.listdir(models / "20")) == ["agent.th", "mixer.th", "opt.th"]
    assert sorted(os.listdir(models / "80")) == ["agent.th", "mixer.th", "opt.th", "run_state.th"]
    _run(_args(tmp_path / "all", save_run_state=True, run_state_keep=0))
    for step in ("20", "80"):
        assert "run_state.th" in os.listdir(tmp_path / "all" / "models" / "tok" / step)
    _run(_args(tmp_path / "two", save_run_state=True, run_state_keep=2, save_model_interval=40))
    held = {d: "run_state.th" in os.listdir(tmp_path / "two" / "models" / "tok" / d)
            for d in os.listdir(tmp_path / "two" / "models" / "tok")}
    assert held == {"20": False, "60": True, "100": True}


def test_run_state_keep_larger_than_the_number_of_checkpoints(tmp_path):
    """keep = 4 with three checkpoints (20, 60, 100): nothing is removed at any of them."""
    _run(_args(tmp_path, save_run_state=True, run_state_keep=4, save_model_interval=40))
    models = tmp_path / "models" / "tok"
    assert sorted(os.listdir(models), key=int) == ["20", "60", "100"]
    for d in ("20", "60", "100"):
        assert "run_state.th" in os.listdir(models / d), d
    # ... and keep = 4 of six checkpoints (one per iteration, 20 .. 120) holds the newest four
    _run(_args(tmp_path / "six", save_run_state=True, run_state_keep=4, save_model_interval=20))
    models = tmp_path / "six" / "models" / "tok"
    held = {d: "run_state.th" in os.listdir(models / d) for d in os.listdir(models)}
    assert held == {"20": False, "40": False, "60": True, "80": True, "100": True, "120": True}, held


def test_run_state_is_written_under_a_temporary_name_then_renamed(tmp_path, monkeypatch):
    """torch.save goes to <name>.tmp while the final name does not exist yet, and the
    rename to the final name comes after the write has returned."""
    import t2omca_amd.driver as driver
    events = []
    real_save, real_replace = torch.save, os.replace

    def save(obj, f, *a, **kw):
        final = str(f)[:-len(".tmp")]
        events.append(("save", str(f), os.path.exists(final)))
        real_save(obj, f, *a, **kw)
        events.append(("saved", os.path.getsize(f) > 0, os.path.exists(final)))

    def replace(src, dst):
        events.append(("replace", str(src), str(dst), os.path.getsize(src) > 0))
        real_replace(src, dst)

    monkeypatch.setattr(driver.torch, "save", save)
    monkeypatch.setattr(driver.os, "replace", replace)
    _run(_args(tmp_path, save_run_state=True, run_state_keep=0, t_max=10))
    monkeypatch.undo()
    name = str(tmp_path / "models" / "tok" / "20" / "run_state.th")
    assert events == [("save", name + ".tmp", False), ("saved", True, False),
                      ("replace", name + ".tmp", name, True)]
    names = [f for _, _, files in os.walk(tmp_path) for f in files]
    assert "run_state.th" in names and not [f for f in names if f.endswith(".tmp")]
    assert torch.load(name, weights_only=True)["runner"]["t_env"] == 20


def test_interrupted_checkpoint_resumes_from_the_last_complete_one(tmp_path):
    """A process killed after save_models and before the run state's rename leaves
    its newest directory with the model files (and perhaps a .tmp) only.  With
    load_step == 0 the restart warns and continues from the newest directory that
    holds a run state, exactly as a resume from that checkpoint; an explicit
    load_step is taken at its word (the reference's weights-only start)."""
    trace, *_, logger = _run(_args(tmp_path / "a", save_run_state=True, run_state_keep=0))
    models = tmp_path / "a" / "models" / "tok"
    os.replace(models / "80" / "run_state.th", models / "80" / "run_state.th.tmp")  # the kill
    cut = trace.index(("save", "20")) + 1
    with pytest.warns(UserWarning, match="no complete run state"):
        trace2, *_, logger2 = _run(_args(tmp_path / "b", save_run_state=True, run_state_keep=0,
                                         checkpoint_path=str(models)))
    assert trace2 == trace[cut:] and _stats(logger2) == _stats(logger)
    trace3, runner3, *_ = _run(_args(tmp_path / "c", checkpoint_path=str(models), load_step=80, t_max=70))
    assert trace3[0] == ("load_models", str(models / "80")) and runner3.t_env == 80
    # no run state anywhere: the newest directory, the reference's way, without a warning
    os.remove(models / "20" / "run_state.th")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        trace4, *_ = _run(_args(tmp_path / "d", checkpoint_path=str(models), t_max=70))
    assert trace4[0] == ("load_models", str(models / "80"))


def test_directory_with_other_files_than_this_world_size_is_refused(tmp_path):
    """A single process's file beside a stray rank file: refused with both lists
    named, whichever way it came about."""
    trace, runner, buffer, learner, logger = _objects()
    _dirs(tmp_path, "40")
    runner.t_env = 40
    loop = {"episode": 4, "last_test_T": 20, "last_log_T": 40, "model_save_time": 20}
    save_run_state(str(tmp_path / "40"), runner, buffer, learner, logger, loop)
    (tmp_path / "40" / "run_state.rank1.th").write_bytes(b"")
    with pytest.raises(ValueError, match=r"needs \['run_state.th'\].*holds \['run_state.rank1.th', 'run_state.th'\]"):
        load_run_state(str(tmp_path / "40"), runner, buffer, learner, logger)
    with pytest.raises(ValueError, match="world_size 1 needs"):
        run_sequential(runner, buffer, learner, logger, _args(tmp_path, checkpoint_path=str(tmp_path), load_step=40))


def test_save_run_state_follows_save_models(tmp_path):
    """The run state is written after the model files, so a directory that holds one is complete."""
    seen = []

    class Learner(StateLearner):
        def state_dict(self):
            seen.append(sorted(os.listdir(path)))
            return super().state_dict()

    trace, runner, buffer, _, logger = _objects()
    path = str(tmp_path / "models" / "tok" / "20")
    run_sequential(runner, buffer, Learner(trace), logger, _args(tmp_path, save_run_state=True, t_max=10))
    assert seen == [["agent.th", "mixer.th", "opt.th"]]


def test_load_run_state_checks_the_directory_number(tmp_path):
    trace, runner, buffer, learner, logger = _objects()
    _dirs(tmp_path, "40")
    runner.t_env = 60
    loop = {"episode": 4, "last_test_T": 20, "last_log_T": 40, "model_save_time": 20}
    save_run_state(str(tmp_path / "40"), runner, buffer, learner, logger, loop)
    with pytest.raises(ValueError, match="t_env"):
        load_run_state(str(tmp_path / "40"), runner, buffer, learner, logger)
    runner.t_env = 40
    save_run_state(str(tmp_path / "40"), runner, buffer, learner, logger, loop)
    runner.t_env = 0
    assert load_run_state(str(tmp_path / "40"), runner, buffer, learner, logger) == loop
    assert runner.t_env == 40


def test_run_state_of_another_world_size_is_refused(tmp_path):
    """Per-rank files in the directory, none for a single process: an error, not a
    silent weights-only resume."""
    trace, runner, buffer, learner, logger = _objects()
    _dirs(tmp_path, "40")
    (tmp_path / "40" / "run_state.rank0.th").write_bytes(b"")
    (tmp_path / "40" / "run_state.rank1.th").write_bytes(b"")
    with pytest.raises(ValueError, match="world_size"):
        run_sequential(runner, buffer, learner, logger, _args(tmp_path, checkpoint_path=str(tmp_path)))
    assert trace == []


def test_stats_logger_state_round_trips_through_weights_only_load(tmp_path):
    log = StatsLogger(out=lambda line: None)
    log.log_stat("return_mean", 2, 10)
    log.log_stat("return_mean", 3.5, 20)
    log.log_stat("episode", 4, 20)
    sd = log.state_dict()
    assert sd == {"format": 1, "stats": {"return_mean": [[10, 2.0], [20, 3.5]], "episode": [[20, 4.0]]}}
    assert type(sd["stats"]) is dict
    torch.save(sd, tmp_path / "log.th")
    back = StatsLogger(out=lambda line: None)
    back.log_stat("stale", 1, 1)
    back.load_state_dict(torch.load(tmp_path / "log.th", weights_only=True))
    assert dict(back.stats) == dict(log.stats)
    back.log_stat("new_key", 1.0, 30)  # still a defaultdict of lists
    assert back.stats["new_key"] == [(30, 1.0)] and back.recent()["return_mean"] == 3.5
    with pytest.raises(ValueError, match="format"):
        back.load_state_dict({"format": 2, "stats": {}})
