"""GPU: the statistics RolloutRunner logs equal the reference runner's.

Five envs run two train and three test episodes each; the recorded actions are
replayed on five oracle envs (oracle/ref_env.RefEnv, bit-exact with the
reference env), and the expected log values are formed from their info dicts and
Python-float returns by the reference's own rule (parallel_runner.py:202-231):
per key the sum over the terminated steps' dicts (a missing key counts 0) divided
by n_episodes, and np.mean of the returns.

Tolerance: both sides sum the same doubles, each in some fixed order, so each is
within n * 2^-53 * Σ|x| of the exact sum and they differ by at most
n * 2^-52 * Σ|x|; the mean adds the rounding of one division, 2^-52 |mean|.

The log schedule is the reference's, `elif` included (:212-219).  The runner is
built with runner_log_interval = 0, so every train run logs (with epsilon).  With
that interval the `elif` would also fire after every TEST run — test statistics
would never wait for test_nepisode episodes — so the interval is raised before
the first two test runs, which must then log once, after the second
(10 = 2 x 5 episodes); a third test run with the interval back at 0 shows the
`elif` firing in test mode, epsilon included, as it does in the reference.
"""
import numpy as np
import pytest
import torch

from oracle.ref_env import RefEnv
from tests.gpu_util import require_gpu

pytestmark = pytest.mark.gpu
N, M, A, T, SEED = 5, 2, 3, 4, 11
EPS = 2.0 ** -52
REF_KEYS = ("return", "reward", "delay_reward", "overtime_penalty", "channel_utilization_rate", "conflict_ratio",
            "episode_limit", "task_completion_rate", "task_completion_delay")
MODES = (False, False, True, True, True)  # test_mode of the five runs


def _agent():
    from t2omca_amd.modules import TransformerAgent
    from t2omca_amd.synthetic import make_args
    torch.manual_seed(0)
    return TransformerAgent(None, make_args(A)).cuda()


def _runner(agent, **kw):
    from t2omca_amd.env import VecEnv
    from t2omca_amd.runner import RolloutRunner
    env = VecEnv(N, mec_num=M, agv_num=A, episode_limit=T, seed=SEED)
    return RolloutRunner(agent, env, seed=3, epsilon_start=0.5, **kw)


@pytest.fixture(scope="module")
def runs():
    """The five runs of the logging runner: per run its batch (host), returns,
    a snapshot of the logger and of the accumulators; and the oracle replay."""
    require_gpu()
    from t2omca_amd.statlog import StatsLogger
    agent = _agent()
    logger = StatsLogger()
    runner = _runner(agent, logger=logger, test_nepisode=10, runner_log_interval=0)
    assert runner.batch_size == N and runner.log_train_stats_t == -100000
    refs = [RefEnv(M, A, T, SEED, e) for e in range(N)]
    out = []
    for i, test_mode in enumerate(MODES):
        runner.runner_log_interval = 10 ** 9 if i in (2, 3) else 0  # (module docstring)
        eps = 0.0 if test_mode else runner.schedule.eval(runner.t_env)
        batch = runner.run(test_mode=test_mode)
        torch.cuda.synchronize()
        acts = batch["actions"][:, :T, :, 0].cpu().numpy()
        infos, returns = [], []
        for e, ref in enumerate(refs):
            ref.worker_reset()
            ret = 0
            for t in range(T):
                r, done, info = ref.worker_step(acts[e, t])[:3]
                ret += r
                if done:
                    infos.append(info)
            returns.append(ret)
        assert len(infos) == N
        out.append(dict(test_mode=test_mode, eps=eps, t_env=runner.t_env, infos=infos, returns=returns,
                        batch={k: v.cpu().clone() for k, v in batch.items()},
                        last_returns=runner.last_returns.cpu().clone(),
                        logged={k: list(v) for k, v in logger.stats.items()},
                        train_stats=runner.train_stats, test_stats=runner.test_stats))
    return agent, out


def _expected(infos, returns):
    """(value, tolerance) per logged key from the reference's rule over these episodes."""
    n = len(returns)
    exp = {"return_mean": (float(np.mean(returns)), n * EPS * sum(abs(x) for x in returns) / n)}
    keys = set.union(*[set(d) for d in infos])
    for k in keys:
        vals = [d.get(k, 0) for d in infos]
        exp[k + "_mean"] = (sum(vals) / n, len(vals) * EPS * sum(abs(float(v)) for v in vals) / n)
    return {k: (v, tol + EPS * abs(v)) for k, (v, tol) in exp.items()}


def _new_entries(runs_, i):
    """{key: [(t, value), ...]} logged by run i alone."""
    before = runs_[i - 1]["logged"] if i else {}
    return {k: v[len(before.get(k, [])):] for k, v in runs_[i]["logged"].items() if len(v) > len(before.get(k, []))}


def _check_logged(new, prefix, infos, returns, t_env, eps):
    exp = _expected(infos, returns)
    assert set(exp) == {k + "_mean" for k in REF_KEYS}, "the oracle's info keys are the reference's set"
    want_keys = {prefix + k for k in exp} | ({"epsilon"} if eps is not None else set())
    assert set(new) == want_keys
    for k, (v, tol) in exp.items():
        (t, got), = new[prefix + k]
        print(f"{prefix + k}: logged {got!r} expected {v!r} tol {tol:.3e}")
        assert t == t_env and abs(got - v) <= tol, (k, got, v, tol)
    assert new[prefix + "episode_limit_mean"][0][1] == 1.0
    if eps is not None:
        assert new["epsilon"] == [(t_env, eps)]


def test_train_runs_log_the_reference_statistics(runs):
    _, r = runs
    for i in (0, 1):
        assert r[i]["t_env"] == (i + 1) * N * T
        _check_logged(_new_entries(r, i), "", r[i]["infos"], r[i]["returns"], r[i]["t_env"], r[i]["eps"])
        assert r[i]["train_stats"]["n_episodes"] == 0  # cleared by the log
    assert r[0]["eps"] == 0.5 and r[1]["eps"] < 0.5


def test_test_statistics_wait_for_test_nepisode(runs):
    _, r = runs
    assert _new_entries(r, 2) == {}, "5 of 10 test episodes: nothing logged yet"
    assert r[2]["test_stats"]["n_episodes"] == N
    want = sum(r[2]["returns"])
    assert abs(r[2]["test_stats"]["return"] - want) <= N * EPS * sum(abs(x) for x in r[2]["returns"])
    assert r[2]["test_stats"]["episode_limit"] == N
    # after the second test run: both runs' episodes, no epsilon (the `if` branch)
    _check_logged(_new_entries(r, 3), "test_", r[2]["infos"] + r[3]["infos"], r[2]["returns"] + r[3]["returns"],
                  r[3]["t_env"], None)
    assert r[3]["t_env"] == r[1]["t_env"], "test runs do not advance t_env"
    assert all(v == 0 for v in r[3]["test_stats"].values()), "the accumulator is cleared by the log"


def test_elif_fires_in_test_mode_as_in_the_reference(runs):
    _, r = runs
    _check_logged(_new_entries(r, 4), "test_", r[4]["infos"], r[4]["returns"], r[4]["t_env"], 0.0)


def test_statistics_do_not_disturb_the_run(runs):
    """A runner with the same seeds and no logger: the same batches and returns, bit for bit."""
    agent, r = runs
    plain = _runner(agent)
    assert plain.logger is None and not plain.collect_stats and plain._acc is None
    for i, test_mode in enumerate(MODES):
        batch = plain.run(test_mode=test_mode)
        torch.cuda.synchronize()
        assert set(batch.keys()) == set(r[i]["batch"])
        for k, v in batch.items():
            assert torch.equal(v.cpu(), r[i]["batch"][k]), (i, k)
        assert torch.equal(plain.last_returns.cpu(), r[i]["last_returns"])
    with pytest.raises(RuntimeError):
        plain.train_stats


def test_collect_stats_without_logger(runs):
    agent, r = runs
    quiet = _runner(agent, collect_stats=True)
    assert quiet.logger is None
    for i in (0, 1):
        quiet.run(test_mode=False)
    s = quiet.train_stats  # never logged, so never cleared: both runs
    assert s["n_episodes"] == 2 * N and s["episode_limit"] == 2 * N
    rets = r[0]["returns"] + r[1]["returns"]
    assert abs(s["return"] - sum(rets)) <= len(rets) * EPS * sum(abs(x) for x in rets)
    assert quiet.test_stats["n_episodes"] == 0
