"""GPU: the NQLearner statistics TDLearner logs (loss_td, grad_norm, td_error_abs,
q_taken_mean, target_mean), when it logs them, and that logging leaves the update alone.

Every logged value is recomputed in fp64 on the host from the SAME call's
outputs (info["qtot"], info["targets"], loss_sum, mask_sum, grad_norm) and the
batch's masks, so the only differences are fp64 summation order — at most
n * 2^-52 * Σ|x| against math.fsum for each of the three sums, plus the rounding
of the quotient — and, for loss_td, one fp32 ulp (a quotient of two fp32 scalars).
"""
import math

import pytest
import torch

from tests.gpu_util import require_gpu
from tests.test_gpu_learner import _setup

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
KEYS = ("loss_td", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean")


def _batch(B, T, A):
    from t2omca_amd.synthetic import make_batch
    batch, w = make_batch(B, T, A, seed=7)
    batch["terminated"][1, T // 2] = 1      # a terminated episode: the next slot is filled (the
    batch["filled"][1, T // 2 + 2:] = 0     # runner's last pre-transition data) but masked
    batch["filled"][B - 1, T - 2:] = 0      # an unfilled tail
    return batch, w


def _expected(info, batch, A):
    """{key: (value, tolerance)} from one train() call's own outputs."""
    q, tgt = info["qtot"].double().cpu(), info["targets"].double().cpu()
    B, T = q.shape
    term = batch["terminated"][:, :T, 0].double().cpu()
    m = batch["filled"][:, :T, 0].double().cpu()
    m[:, 1:] *= 1.0 - term[:, :-1]
    msum = math.fsum(m.flatten().tolist())
    out = {}
    for key, x, div in (("td_error_abs", (q - tgt).abs() * m, msum), ("q_taken_mean", q * m, msum * A),
                        ("target_mean", tgt * m, msum * A)):
        x = x.flatten().tolist()
        v = math.fsum(x) / div
        out[key] = (v, len(x) * EPS * math.fsum(abs(t) for t in x) / div + EPS * abs(v))
    loss_td = float(info["loss_sum"]) / float(info["mask_sum"])
    assert float(info["mask_sum"]) == msum
    out["loss_td"] = (loss_td, 2.0 ** -23 * abs(loss_td))
    out["grad_norm"] = (float(info["grad_norm"]), 0.0)
    return out


def _train_logged_and_twin(A, B, T, **kw):
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.statlog import StatsLogger
    batch, w = _batch(B, T, A)
    logger = StatsLogger()
    agent, mixer, _, _ = _setup(A, seed=5)
    learner = TDLearner(agent, mixer, priorities_to_cpu=False, logger=logger, learner_log_interval=20, **kw)
    assert learner.log_stats_t == -21
    expected = {}
    for step, t_env in enumerate((0, 10, 25)):
        info = learner.train(batch, t_env, step, per_weight=w)
        torch.cuda.synchronize()
        expected[t_env] = _expected(info, batch, A)
    agent2, mixer2, _, _ = _setup(A, seed=5)
    twin = TDLearner(agent2, mixer2, priorities_to_cpu=False, **kw)
    assert twin.logger is None and twin._stat is None
    for step, t_env in enumerate((0, 10, 25)):
        twin.train(batch, t_env, step, per_weight=w)
    torch.cuda.synchronize()
    return learner, twin, logger, expected


def _check(learner, twin, logger, expected):
    assert set(logger.stats) == set(KEYS)
    for key in KEYS:
        entries = logger.stats[key]
        assert [t for t, _ in entries] == [0, 25], "logged at t_env 0 and 25, not at 10 (-21 -> 0 -> 25)"
        for t_env, got in entries:
            want, tol = expected[t_env][key]
            print(f"t_env {t_env} {key}: logged {got!r} expected {want!r} tol {tol:.3e}")
            assert math.isfinite(got) and abs(got - want) <= tol, (t_env, key, got, want, tol)
    assert learner.log_stats_t == 25
    # logging must not touch the update: the twin without a logger is bit-identical
    for name in ("params", "exp_avg", "exp_avg_sq"):
        a, b = getattr(learner, name), getattr(twin, name)
        assert torch.isfinite(a).all() and torch.equal(a, b), name


def test_learner_logs_nqlearner_statistics():
    require_gpu()
    learner, twin, logger, expected = _train_logged_and_twin(3, 5, 6)
    assert not learner._pipelined(5)
    _check(learner, twin, logger, expected)


def test_learner_logs_on_the_pipelined_path():
    """16 AGVs x 4 episodes: the update runs in step ranges on two streams and reuses
    its Qtot buffers; the statistics read the copy _finish is given."""
    require_gpu()
    learner, twin, logger, expected = _train_logged_and_twin(16, 4, 5, pipeline="auto")
    assert learner._pipelined(4)
    _check(learner, twin, logger, expected)
