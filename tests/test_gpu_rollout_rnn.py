"""GPU: the closed loop with the GRU agent (RolloutRunner with modules.RNNAgent) in both
observation modes, and three iterations of driver.run_sequential with rnn + qmix.

Greedy runs are checked from the returned batch alone: Q is recomputed on the CPU in fp64
with tests/rnn_model from the batch's observations and actions (the last-action one-hot
of step t is the stored action of step t - 1); every stored action must be available and
equal the avail-masked argmax wherever the masked top-two gap exceeds GAP = 1e-4, and at
most 5 % of the (env, step, agent) entries may fall under that gap (asserted; measured
0 of them in every case).  The modules are drawn with torch.manual_seed(0), env seed 11,
runner seed 13.  (The 5 % figure was not pre-computed with oracle/ref_env.py driving the
model on the CPU: the test asserts it on the batch it checks.)

The loop: 3 AGVs, 4 envs, T = 5, three iterations of 20 env steps with an update in
each, a checkpoint with its run state at 20; a run resumed from it by fresh objects
built from other seeds ends bit-identical (test_gpu_resume.py's comparison), fp32 only.
"""
import types

import pytest
import torch

from tests import rnn_model
from tests.gpu_util import require_gpu
from tests.test_gpu_resume import _differing, _example, _final, _same

pytestmark = pytest.mark.gpu

M, C = 2, 4
NA = C + 1
GAP = 1e-4


def make(A, n, T, entity, wire=False, flags=True, seed=0, channels=C, **runner_kw):
    from t2omca_amd.env import VecEnv
    from t2omca_amd.modules import make_agent
    from t2omca_amd.runner import RolloutRunner
    torch.manual_seed(seed)
    na = channels + 1
    args = types.SimpleNamespace(n_agents=A, n_actions=na, agent="rnn", obs_last_action=flags, obs_agent_id=flags,
                                 device="cuda")
    n_obs = 9 * A if entity else 6
    agent = make_agent(n_obs + ((na + A) if flags else 0), args).cuda()
    env = VecEnv(n, mec_num=M, agv_num=A, num_channels=channels, episode_limit=T, seed=11, obs_entity_mode=entity,
                 wire=wire)
    return agent, env, RolloutRunner(agent, env, seed=13, compact_obs=wire, **runner_kw)


def model_q(agent, batch, obs):
    p = rnn_model.param_dict(agent)
    sh = agent.shape
    x = rnn_model.build_inputs(obs.cpu().double(), batch["actions"].cpu(), sh.NA, sh.last_action, sh.agent_id)
    n, _, A, _ = x.shape
    return rnn_model.unroll(p, x, torch.zeros(n, A, sh.H, dtype=torch.float64))[0]


def check_actions(tag, agent, batch, obs):
    q = model_q(agent, batch, obs)
    avail = batch["avail_actions"].cpu()
    acts = batch["actions"].cpu()[..., 0]
    assert bool(torch.gather(avail, 3, acts.unsqueeze(3)).all()), "an unavailable action was stored"
    qm = q.clone()
    qm[avail == 0] = -float("inf")
    top = qm.topk(2, dim=3).values
    clear = (top[..., 0] - top[..., 1]) > GAP  # (one available action: an infinite gap)
    share = 1.0 - float(clear.double().mean())
    wrong = int((acts != qm.argmax(3))[clear].sum())
    print(f"rnn rollout {tag}: {share:.4f} of the entries under the gap, {wrong} of {int(clear.sum())} clear entries "
          f"differ from the fp64 argmax")
    assert share <= 0.05, share
    assert wrong == 0, wrong


@pytest.mark.parametrize("A,n,T", [(3, 4, 5), (16, 2, 4)])
@pytest.mark.parametrize("mode", ["entity", "flat", "entity_wire", "entity_plain"])
def test_greedy_run(A, n, T, mode):
    require_gpu()
    from t2omca_amd import ops
    entity = mode != "flat"
    agent, env, runner = make(A, n, T, entity, wire=mode == "entity_wire", flags=mode != "entity_plain")
    batch = runner.run(test_mode=True)
    torch.cuda.synchronize()
    assert runner.t_env == 0 and runner.episode == 1
    assert tuple(batch["actions"].shape) == (n, T + 1, A, 1) and tuple(batch["state"].shape) == (n, T + 1, 8 * A)
    if mode == "entity_wire":
        assert "obs" not in batch.keys() and tuple(batch["obs_wire"].shape) == (n, T + 1, A, 4)
        obs = ops.obs_expand(batch["obs_wire"], batch["obs_nrm_n"], batch["obs_nrm"])
    else:
        obs = batch["obs"]
        assert tuple(obs.shape) == (n, T + 1, A, 9 * A if entity else 6)
    check_actions(f"{mode} ({A},{n},{T})", agent, batch, obs)
    assert bool(batch["filled"].all()) and bool(torch.isfinite(runner.last_returns).all())


@pytest.mark.parametrize("entity", [True, False])
def test_exploring_run(entity):
    """ε = 1: every stored action is available, and t_env advances."""
    require_gpu()
    A, n, T = 3, 4, 5
    agent, env, runner = make(A, n, T, entity, epsilon_start=1.0, epsilon_finish=1.0)
    batch = runner.run(test_mode=False)
    torch.cuda.synchronize()
    assert runner.t_env == n * T and runner.episode == 1
    acts = batch["actions"][..., 0]
    assert bool(torch.gather(batch["avail_actions"], 3, acts.unsqueeze(3)).all())
    assert int(acts.max()) < NA and int(acts.min()) >= 0
    batch = runner.run(test_mode=False)
    assert runner.t_env == 2 * n * T


def test_input_width_is_checked():
    require_gpu()
    from t2omca_amd.env import VecEnv
    from t2omca_amd.modules import TransformerAgent, make_agent
    from t2omca_amd.runner import RolloutRunner
    from t2omca_amd.synthetic import make_args
    A = 3
    flat_env = VecEnv(2, mec_num=M, agv_num=A, num_channels=C, episode_limit=3, seed=1, obs_entity_mode=False)
    args = types.SimpleNamespace(n_agents=A, n_actions=NA, agent="rnn", device="cuda")
    with pytest.raises(ValueError, match="input_shape must be 14"):
        RolloutRunner(make_agent(9 * A + NA + A, args).cuda(), flat_env)
    with pytest.raises(ValueError, match="agents / actions"):
        RolloutRunner(make_agent(6 + 6 + A, types.SimpleNamespace(**{**vars(args), "n_actions": 6})).cuda(), flat_env)
    with pytest.raises(ValueError, match="transformer agent reads entity observations"):
        RolloutRunner(TransformerAgent(None, make_args(A, n_actions=NA)).cuda(), flat_env)


# ---- the loop -------------------------------------------------------------------
A_, N_, T_ = 3, 4, 5
LOOP = dict(t_max=59, batch_size=4, batch_size_run=4, test_interval=40, test_nepisode=4, log_interval=20,
            save_model=True, save_model_interval=20, save_run_state=True, run_state_keep=0, unique_token="tok")


def _objects(seed):
    from t2omca_amd.env import VecEnv
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.modules import make_agent, make_mixer
    from t2omca_amd.replay import PrioritizedReplayBuffer
    from t2omca_amd.runner import RolloutRunner
    from t2omca_amd.statlog import StatsLogger
    from t2omca_amd.synthetic import make_args
    logger = StatsLogger(out=lambda line: None)
    torch.manual_seed(seed)
    args = types.SimpleNamespace(**{**vars(make_args(A_, n_actions=NA, mixer="qmix")), "agent": "rnn"})
    agent, mixer = make_agent(9 * A_ + NA + A_, args).cuda(), make_mixer(args).cuda()
    learner = TDLearner(agent, mixer, target_update_interval=8, logger=logger, learner_log_interval=20)
    env = VecEnv(N_, mec_num=M, agv_num=A_, num_channels=C, episode_limit=T_, seed=seed + 1)
    runner = RolloutRunner(agent, env, seed=seed + 2, epsilon_anneal_time=400, logger=logger, test_nepisode=4,
                           runner_log_interval=20)
    buffer = PrioritizedReplayBuffer(_example(), 12, T_ + 1, 0.6, 0.4, 1000, seed=seed + 3)
    return runner, buffer, learner, logger


def _loop_run(seed, results, **extra):
    from t2omca_amd.driver import run_sequential
    objs = _objects(seed)
    run_sequential(*objs, types.SimpleNamespace(**LOOP, local_results_path=str(results), **extra))
    return objs, _final(*objs)


def test_three_iterations_and_resume(tmp_path):
    require_gpu()
    (runner, buffer, learner, logger), straight = _loop_run(5, tmp_path / "a")
    assert runner.t_env == 60 and learner.step_count == 3 and learner.agent_kind == "rnn"
    losses = [v for _, v in logger.stats["loss_td"]]
    assert losses and all(torch.isfinite(torch.tensor(v)) for v in losses), losses
    # the priorities were updated: no longer the inserted episodes' max_priority ** alpha
    p = buffer.p[:buffer.episodes_in_buffer].cpu()
    assert bool(torch.isfinite(p).all()) and len(set(p.tolist())) > 1, p
    models = tmp_path / "a" / "models" / "tok"
    _, resumed = _loop_run(31, tmp_path / "b", checkpoint_path=str(models), load_step=20)
    assert _same(resumed, straight), _differing(resumed, straight)
    assert straight["learner"]["agent"] == "rnn" and straight["learner"]["step_count"] == 3
