"""GPU, data parallel: logged statistics are the GLOBAL ones on every rank.

Two ranks (gloo, both on cuda:0, fresh child processes as in
tests/test_gpu_dp_learner.py) each train on half of a 6-episode batch with ragged
masks, with a logger; one all-reduce of [loss_sum, mask_sum, Σm, Σ|td|m, Σq m, Σtgt m]
before the host read makes both log the full batch's values.  They are compared
with a single-process learner on the whole batch, from rank 0's initial parameters:

  * td_error_abs, q_taken_mean, target_mean: the per-episode Qtot / targets are the
    same floats in a shard as in the full batch, so the two sides differ only in fp64
    summation order: at most n * 2^-52 * Σ|x| on a sum, plus one quotient rounding;
  * loss_td: its numerator is an fp32 sum of n = B*T non-negative terms on both
    sides, each within n * 2^-24 of exact, so n * 2^-23 relative;
  * grad_norm: the data-parallel gradient equals the full-batch one to 1e-6
    normwise (the bar of tests/test_gpu_dp_learner.py), so the norms differ by at
    most sqrt(N) * 1e-6 relative (| ||a|| - ||b|| | <= ||a - b|| <= sqrt(N) max|a - b|).

Each rank also runs a small rollout with statistics on: the accumulator,
all-reduced on the read, counts both ranks' episodes on both ranks.
"""
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from tests.gpu_util import require_gpu

pytestmark = pytest.mark.gpu
A, B, T = 8, 6, 7
N_ENVS, T_ENV = 3, 4
EPS = 2.0 ** -52
KEYS = ("loss_td", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean")


def _batch(device):
    from t2omca_amd.synthetic import make_batch
    batch, w = make_batch(B, T, A, seed=11, device=device)
    batch["terminated"][1, 3] = 1  # ragged masks: the shards' Σ mask differ
    batch["filled"][4, 5:] = 0
    return batch, w


def _learner(seed, device, logger):
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.modules import TransformerAgent, TransformerMixer
    from t2omca_amd.synthetic import make_args
    torch.manual_seed(seed)
    args = make_args(A, device=str(device))
    agent = TransformerAgent(None, args).to(device)
    mixer = TransformerMixer(args).to(device)
    return TDLearner(agent, mixer, logger=logger, learner_log_interval=1, priorities_to_cpu=False)


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from t2omca_amd.distributed import shard_bounds
        from t2omca_amd.env import VecEnv
        from t2omca_amd.runner import RolloutRunner
        from t2omca_amd.statlog import StatsLogger
        logger = StatsLogger()
        learner = _learner(100 + rank, dev, logger)  # different init per rank: the broadcast fixes it
        batch, w = _batch(dev)
        lo, hi = shard_bounds(B, rank, world)
        learner.train({k: v[lo:hi] for k, v in batch.items()}, 0, 0, per_weight=w[lo:hi])
        env = VecEnv(N_ENVS, mec_num=2, agv_num=A, episode_limit=T_ENV, seed=5)
        runner = RolloutRunner(learner.agent, env, seed=3, collect_stats=True)
        runner.run()
        local = runner._acc[0].cpu().tolist()
        stats = runner.train_stats
        torch.cuda.synchronize()
        out.put((rank, {k: list(v) for k, v in logger.stats.items()}, stats, local))
    finally:
        dist.destroy_process_group()


def test_dp_ranks_log_global_statistics():
    require_gpu()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = {r: rest for r, *rest in (q.get(timeout=240) for _ in procs)}
    finally:
        for p in procs:
            p.join(timeout=60)
    for p in procs:
        assert p.exitcode == 0
    (log0, stats0, local0), (log1, stats1, local1) = res[0], res[1]
    assert set(log0) == set(KEYS) and log0 == log1, "both ranks log identical values"

    # the single-process learner on the whole batch, from rank 0's init
    from t2omca_amd.statlog import StatsLogger
    dev = torch.device("cuda", 0)
    logger = StatsLogger()
    full = _learner(100, dev, logger)
    batch, w = _batch(dev)
    info = full.train(batch, 0, 0, per_weight=w)
    torch.cuda.synchronize()
    qt, tgt = info["qtot"].double().cpu(), info["targets"].double().cpu()
    m = batch["filled"][:, :T, 0].double().cpu()
    m[:, 1:] *= 1.0 - batch["terminated"][:, :T - 1, 0].double().cpu()
    msum = float(m.sum())
    tol = {"loss_td": B * T * 2.0 ** -23, "grad_norm": math.sqrt(full.params.numel()) * 1e-6}
    for key, x, div in (("td_error_abs", (qt - tgt).abs() * m, msum), ("q_taken_mean", qt * m, msum * A),
                        ("target_mean", tgt * m, msum * A)):
        tol[key] = (B * T * EPS * float(x.abs().sum()) / div, EPS)
    for key in KEYS:
        (t0, got), = log0[key]
        (t1, want), = logger.stats[key]
        bar = tol[key][0] + tol[key][1] * abs(want) if isinstance(tol[key], tuple) else tol[key] * abs(want)
        print(f"{key}: ranks {got!r} full batch {want!r} |diff| {abs(got - want):.3e} tol {bar:.3e}")
        assert t0 == t1 == 0 and math.isfinite(got) and abs(got - want) <= bar, (key, got, want, bar)

    # runner accumulators: each rank ran N_ENVS envs (of its own seed stream), the read is global
    assert local0[0] == local1[0] == N_ENVS
    assert stats0["n_episodes"] == stats1["n_episodes"] == 2 * N_ENVS
    assert stats0 == stats1
    assert stats0["episode_limit"] == 2 * N_ENVS
    want = local0[1] + local1[1]
    assert abs(stats0["return"] - want) <= EPS * abs(want)  # gloo's one addition of the two partial sums
    assert local0[1] != local1[1], "the ranks draw different episodes"
