"""GPU: rollouts with a NoisyNet agent (RolloutRunner with an agent built for
action_selector "noisy-new").

Shapes: 3 AGVs, 4 envs, T = 5 (the exact instance, 12 rows: under a wave) and 16 AGVs,
30 envs, T = 4 (480 rows).  Sigmas 0.3·N(0, 1), so the noisy Q is far from the mean Q.

  * test_mode: the mean head, today's fused path — the batch is bit-equal to the batch of
    a plain agent carrying (u_w, u_b).
  * train mode with ε = 0: every action is the masked argmax of the restated noisy Q
    (tests/noisy_model.py on numpy ε: kind "runner", the runner's seed, counter = episode)
    on the run's own h, wherever the top-two gap exceeds 1e-5·max|q| (the fp32 forward
    bar; inside it fp32 may legitimately pick the other action).  The share of rows left
    out is printed and must stay <= 5 %; a row's gap is a continuous quantity of order
    max|q|, so the expected share is of order 1e-5·NA (measured on an MI355X: 0 at the
    small shape, 0 and 0.0004 — one row of 2400 — at the large one).  The actions must also
    differ from the mean head's greedy ones at >= 5 % of rows (measured 0.53 - 0.87).
  * two runs of the same episode number from equal seeds are bit-equal; the next episode
    draws another ε (and still matches the restatement at its own counter).
  * resume: one driver.run_sequential loop of tests/test_gpu_resume.py (its helpers
    imported, its modules replaced by noisy ones) resumed from its latest checkpoint ends
    bit-identical to the uninterrupted run, with no state beyond the seeds and counters.
"""
import types

import pytest
import torch

from tests import noisy_model as nm
from tests.gpu_util import require_gpu

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 4, 5), (16, 2, 30, 4)]  # A, M, envs, T
IDS = ["a3-n4-T5", "a16-n30-T4"]


def _agents(A, seed=0):
    """(noisy agent with 0.3·N(0, 1) sigmas, plain agent carrying its means)."""
    from t2omca_amd.modules import TransformerAgent
    from t2omca_amd.synthetic import make_args
    args = make_args(A)
    torch.manual_seed(seed)
    noisy = TransformerAgent(None, types.SimpleNamespace(**{**vars(args), "action_selector": "noisy-new"})).cuda()
    torch.manual_seed(seed)
    plain = TransformerAgent(None, args).cuda()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        noisy.q_basic.s_w.copy_(0.3 * torch.randn(noisy.q_basic.s_w.shape, generator=g))
        noisy.q_basic.s_b.copy_(0.3 * torch.randn(noisy.q_basic.s_b.shape, generator=g))
    assert torch.equal(noisy.q_basic.u_w, plain.q_basic.weight) and torch.equal(noisy.q_basic.u_b, plain.q_basic.bias)
    return noisy, plain


def _runner(agent, A, M, n, T, **kw):
    from t2omca_amd.env import VecEnv
    from t2omca_amd.runner import RolloutRunner
    env = VecEnv(n, mec_num=M, agv_num=A, episode_limit=T, seed=11)
    return RolloutRunner(agent, env, seed=3, **kw)


def _equal_batches(a, b):
    assert a.keys() == b.keys()
    return all(torch.equal(a[k], b[k]) for k in a.keys())


@pytest.mark.parametrize("A,M,n,T", SHAPES, ids=IDS)
def test_test_mode_is_the_plain_agents_rollout(A, M, n, T):
    require_gpu()
    noisy, plain = _agents(A)
    rn, rp = _runner(noisy, A, M, n, T), _runner(plain, A, M, n, T)
    assert rn.noisy and not rp.noisy
    bn, bp = rn.run(test_mode=True), rp.run(test_mode=True)
    torch.cuda.synchronize()
    assert _equal_batches(bn, bp) and torch.equal(rn.last_returns, rp.last_returns)
    assert rn.state_dict()["noisy"] is True and rp.state_dict()["noisy"] is False
    with pytest.raises(ValueError, match="noisy"):
        rp.load_state_dict(rn.state_dict())
    old = {k: v for k, v in rp.state_dict().items() if k != "noisy"}  # saved before the field existed: plain
    rp.load_state_dict(old)
    with pytest.raises(ValueError, match="noisy"):
        rn.load_state_dict(old)


def _check_episode(runner, noisy, batch, episode):
    """The batch's actions against the restated noisy head on the run's own h."""
    from t2omca_amd import ops
    A, T1 = runner.A, runner.T + 1
    nl = noisy.q_basic
    E, NA = nl.in_features, nl.out_features
    flat = torch.cat([p.detach().reshape(-1) for p in noisy.parameters()])
    q_mean, h = ops.agent_unroll_fwd(runner.shape, ops.pack_params(runner.shape, flat[:runner.shape.n_params]),
                                     batch["obs"])
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    ew, eb = (torch.from_numpy(x).double() for x in nm.noise_normal(E, NA, T1, runner.seed, "runner", episode))
    q = nm.noisy_head(d(h), d(nl.u_w), d(nl.u_b), d(nl.s_w), d(nl.s_b), ew, eb)
    on = batch["avail_actions"].cpu() != 0
    qm = q.masked_fill(~on, -float("inf"))
    top2 = qm.topk(2, dim=-1).values
    decided = (top2[..., 0] - top2[..., 1]) > 1e-5 * float(q.abs().max())
    out = float((~decided).double().mean())
    acts = batch["actions"][..., 0].cpu()
    mean_acts = d(q_mean).masked_fill(~on, -float("inf")).argmax(-1)
    moved = float((qm.argmax(-1) != mean_acts).double().mean())
    print(f"episode {episode}: {out:.4f} of the rows left out (top-two gap within 1e-5 max|q|); the noisy greedy "
          f"action differs from the mean head's at {moved:.3f}")
    assert out <= 0.05, out
    assert moved >= 0.05, moved
    assert torch.equal(acts[decided], qm.argmax(-1)[decided])
    return ew


@pytest.mark.parametrize("A,M,n,T", SHAPES, ids=IDS)
def test_train_mode_actions_follow_the_noisy_head(A, M, n, T):
    require_gpu()
    noisy, _ = _agents(A)
    greedy = dict(epsilon_start=0.0, epsilon_finish=0.0)
    r1, r2 = _runner(noisy, A, M, n, T, **greedy), _runner(noisy, A, M, n, T, **greedy)
    b1 = r1.run()
    e0 = _check_episode(r1, noisy, b1, 0)
    b2 = r2.run()
    torch.cuda.synchronize()
    assert _equal_batches(b1, b2) and torch.equal(r1.last_returns, r2.last_returns)  # the same episode: the same bits
    assert r1.episode == 1 and r1.t_env == n * T
    b3 = r1.run()
    e1 = _check_episode(r1, noisy, b3, 1)
    assert not torch.equal(e0, e1)  # consecutive episodes draw different noise
    assert not torch.equal(b3["actions"], b1["actions"])
    # the ε schedule still applies as configured: with ε = 1 every action is a uniform draw
    r3 = _runner(noisy, A, M, n, T, epsilon_start=1.0, epsilon_finish=1.0)
    b4 = r3.run()
    assert not torch.equal(b4["actions"], b1["actions"])


def test_resumed_noisy_run_is_identical(monkeypatch, tmp_path):
    require_gpu()
    import tests.test_gpu_resume as tr

    def noisy_modules(seed):
        from t2omca_amd.modules import TransformerAgent, TransformerMixer
        from t2omca_amd.synthetic import make_args
        torch.manual_seed(seed)
        args = make_args(tr.A, n_actions=tr.NA)
        agent = TransformerAgent(None, types.SimpleNamespace(**{**vars(args), "action_selector": "noisy-new"}))
        with torch.no_grad():  # sigmas large enough that the noise decides actions
            agent.q_basic.s_w.fill_(0.3)
            agent.q_basic.s_b.fill_(0.3)
        return agent.cuda(), TransformerMixer(args).cuda()

    monkeypatch.setattr(tr, "_modules", noisy_modules)
    objs, straight = tr._loop_run(5, "fp32", tmp_path / "a")
    runner, _, learner, _ = objs
    assert runner.noisy and learner.noisy and learner.step_count == 10
    assert straight["learner"]["noisy"] is True and straight["runner"]["noisy"] is True
    sig = learner.params[learner.na_net:learner.na]
    assert float((sig - 0.3).abs().max()) > 1e-4  # the sigmas were trained
    models = tmp_path / "a" / "models" / "tok"
    _, resumed = tr._loop_run(31, "fp32", tmp_path / "c", checkpoint_path=str(models), load_step=0)
    assert tr._same(resumed, straight), tr._differing(resumed, straight)
