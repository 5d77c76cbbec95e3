"""GPU: the env kernel, the action selection and the closed loop at action counts other
than five (n_actions = num_channels + 1; every other GPU env test runs num_channels = 4).

The env kernel (t2o_env.hip) against the numpy restatement (oracle/ref_env.py, itself
pinned to the reference env at C = 1 and C = 7 by tests/golden/env_m2_a8_c1_t6.npz and
env_m4_a5_c7_t5.npz, which tests/test_gpu_env.py and test_gpu_wire.py replay on the GPU
too).  Bar: bit-exact, test_gpu_env._rollout_vs_oracle's.  What a channel count reaches:

  * lane_map(A, M, C) caps the envs of a wave at 1088 / (M (C + 1)) collision counters:
    at C = 4 the cap binds at M = 16 only (13 envs); at M = 16 it is 4 envs at C = 15 and
    8 at C = 7, and the [g][mec][channel] counter index runs with another row length;
  * the utilisation sums C + 1 terms count / C per MEC in fp64 (environment_multi_mec.py
    :327-329): dyadic at C = 4, where no order of additions can matter; not at 3, 7, 15;
  * C = 1: two actions, so every pair of offloaders of a MEC collides.

t2o_select_actions against oracle/ref_mac.select_actions, exactly, at 1, 2, 3, 8, 16 and
32 actions (32 is the kernel's limit; 33 is refused without a launch).

The closed loop (RolloutRunner: env -> agent step -> selection -> env) at C = 7 and C = 1
in tests/test_gpu_rollout.py's form, its batch through the learner at C = 7, and the GRU
agent with QMIX at C = 15 (16 actions, the agent kernels' limit) with one update.

MEASURED on an MI355X: every env case bit-exact, utilisation included; the selection exact
at every count and epsilon; the C = 15 GRU rollout has no entry under the argmax gap and 0 of
72 clear entries off the fp64 argmax.  Nothing here failed before or after this file.
"""
import ctypes

import pytest
import torch

from tests.gpu_util import require_gpu
from tests.test_gpu_env import _rollout_vs_oracle
from tests.test_gpu_rollout import rollout_batch_feeds_learner, rollout_vs_replay_and_unroll, select_actions_vs_oracle
from tests.test_gpu_wire import obs_expand_vs_env

pytestmark = pytest.mark.gpu

# (NE, M, A, C, T)
ENV_CASES = [
    (6, 2, 16, 1, 6),    # two actions: every pair of offloaders of a MEC collides
    (9, 4, 8, 3, 6),     # utilisation terms 1/3
    (9, 16, 3, 15, 5),   # 1088 / (16 * 16) = 4 envs per wave: two full waves and one env in the third
    (11, 16, 3, 7, 5),   # 1088 / (16 * 8) = 8 envs per wave, the second wave partial
    (4, 1, 1, 15, 8),    # one AGV, 16 actions
]


@pytest.mark.parametrize("NE,M,A,C,T", ENV_CASES, ids=lambda v: str(v))
def test_env_channel_counts_vs_oracle(NE, M, A, C, T):
    require_gpu()
    _rollout_vs_oracle(NE=NE, M=M, A=A, T=T, eps=2, seed=40 + C, num_channels=C)


def test_env_flat_obs_three_actions_vs_oracle():
    """obs_entity_mode=False (get_obs_agent's flat branch) at 64 AGVs and two channels."""
    require_gpu()
    _rollout_vs_oracle(NE=3, M=4, A=64, T=4, eps=1, seed=46, obs_entity_mode=False, num_channels=2)


def test_obs_expand_at_eight_actions():
    """The wire format at C = 7: t2o_obs_expand rebuilds the env's own dense obs (the wire rows
    carry no action-count field; the dense obs they expand to must not depend on one)."""
    obs_expand_vs_env(8, 2, 16, 6, 2, num_channels=7)


@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("na", [1, 2, 3, 8, 16, 32])
def test_select_actions_action_counts(na, eps):
    """test_gpu_rollout.test_select_actions_matches_oracle's tie-heavy integer Q and masks at
    other action counts, exactly against the oracle (its uniform draws included)."""
    select_actions_vs_oracle(eps, na)


def test_select_actions_refuses_33():
    """MAC_MAXNA = 32: T2O_EINVAL, and nothing is written."""
    require_gpu()
    from t2omca_amd import _lib, ops
    rows, na = 8, 33
    q = torch.zeros(rows, na, device="cuda")
    avail = torch.ones(rows, na, dtype=torch.int32, device="cuda")
    out = torch.full((rows,), -7, dtype=torch.int64, device="cuda")
    rc = _lib.lib().t2o_select_actions(_lib.ptr(q), _lib.ptr(avail), _lib.ptr(out), rows, na, 0.5,
                                       ctypes.c_uint64(1), 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1  # T2O_EINVAL
    assert bool((out == -7).all())
    with pytest.raises(RuntimeError, match="select_actions"):
        ops.select_actions(q, avail, 0.5, seed=1)


@pytest.mark.parametrize("A,M,n,T,C", [(8, 4, 6, 5, 7), (3, 2, 5, 4, 1)])
def test_rollout_replay_and_unroll_channel_counts(A, M, n, T, C):
    """The runner's per-step agent launches (head of C + 1 columns: 8 fills two 4-column
    groups, 2 half of one), the masked argmax and the env at C channels."""
    rollout_vs_replay_and_unroll(A, M, n, T, "fp32", num_channels=C)


def test_rollout_batch_feeds_learner_eight_actions():
    """A C = 7 rollout batch through the transformer learner (8 actions: the mixer's Q
    selection at its full width) against the fp64 oracle."""
    rollout_batch_feeds_learner(num_channels=7)


def test_rnn_qmix_rollout_sixteen_actions_trains():
    """The GRU agent's closed loop at C = 15 (a 16-wide last-action one-hot): the greedy run
    is the fp64 model's masked argmax (test_gpu_rollout_rnn.check_actions), and an exploring
    run's batch trains one QMIX update with finite results that move the parameters."""
    require_gpu()
    import types

    from t2omca_amd.learner import TDLearner
    from t2omca_amd.modules import make_mixer
    from t2omca_amd.synthetic import make_args
    from tests.test_gpu_rollout_rnn import check_actions, make
    A, n, T, C = 3, 4, 5, 15
    agent, env, runner = make(A, n, T, True, channels=C)
    assert env.n_actions == 16 and agent.shape.NA == 16
    batch = runner.run(test_mode=True)
    torch.cuda.synchronize()
    check_actions(f"C=15 ({A},{n},{T})", agent, batch, batch["obs"])
    agent, env, runner = make(A, n, T, True, channels=C, epsilon_start=1.0, epsilon_finish=1.0)
    batch = runner.run(test_mode=False)
    acts = batch["actions"][..., 0]
    assert bool(torch.gather(batch["avail_actions"], 3, acts.unsqueeze(3)).all())
    assert 0 <= int(acts.min()) and int(acts.max()) < 16 and int(acts.max()) > 4
    torch.manual_seed(1)
    mixer = make_mixer(types.SimpleNamespace(**vars(make_args(A, n_actions=16, mixer="qmix")))).cuda()
    learner = TDLearner(agent, mixer)
    before = learner.params.clone()
    info = learner.train(batch, 0, 0, per_weight=torch.ones(n, device="cuda"))
    torch.cuda.synchronize()
    assert learner.step_count == 1 and bool(torch.isfinite(learner.grad).all())
    assert bool(torch.isfinite(info["qtot"]).all()) and bool(torch.isfinite(info["td_errors_abs"]).all())
    assert float(learner.grad[-1]) == n * T and not torch.equal(learner.params, before)
