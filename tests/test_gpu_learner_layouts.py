"""GPU: one TD update, the same replay batch at other addresses (learner level).

TDLearner.train (per_run.py:224-238 is the caller) reads the batch in place through
the element strides of the unroll ABI (include/t2omca.h: obs_sb / obs_st, st_*,
act_*, av_*, the TD loss's rw_* / tm_* / fl_*).  The rollout runner hands it
time-major storage viewed [B, T+1, ...]; the reference driver slices
[:, :max_t_filled] out of longer replay slabs.  Every case here runs one update on
one synthetic batch with ragged masks, presented

  contiguous   dense [B, T+1, ...] tensors;
  time-major   [T+1, B, ...] storage viewed [B, T+1, ...] (episode stride < step
               stride), as runner.py produces;
  slab         a [:, :T+1] slice of replay slabs carved from a poisoned arena
               (tests/arena.py): two more steps per episode, a padded step stride and
               a padded episode stride at once; every element outside the slice is a
               NaN (floats) or -1 / 255 (actions, avail, masks);

from the same parameters and optimiser state, and asserts that Q_tot, the targets,
the priorities, the whole raw gradient (its Σ mask slot included) and the
parameters after the optimiser step are BIT-IDENTICAL across the presentations and
finite, and that no byte of the slabs outside the slice changed.  No tolerance: the
kernels compute the same values in the same order wherever the inputs lie
("memory contract").  A swapped sb / st in any kernel family the
update runs, or a used read of a step or a row outside the slice, fails here.

The contiguous presentation is what tests/test_gpu_configs.py and
test_gpu_fullgrid.py hold against the fp64 oracle at these shapes.
"""
import types

import pytest
import torch

from tests.arena import Arena
from tests.gpu_util import require_gpu
from tests.test_gpu_fullgrid import _ragged

pytestmark = pytest.mark.gpu


def _modules(A, noisy):
    from t2omca_amd.modules import TransformerAgent, TransformerMixer
    from t2omca_amd.synthetic import make_args
    torch.manual_seed(7)
    args = make_args(A)
    if noisy:
        agent = TransformerAgent(None, types.SimpleNamespace(**{**vars(args), "action_selector": "noisy-new"}))
        g = torch.Generator().manual_seed(8)
        with torch.no_grad():  # sigmas large enough that the noisy Q is far from the mean Q
            agent.q_basic.s_w.copy_(0.3 * torch.randn(agent.q_basic.s_w.shape, generator=g))
            agent.q_basic.s_b.copy_(0.3 * torch.randn(agent.q_basic.s_b.shape, generator=g))
    else:
        agent = TransformerAgent(None, args)
    return agent.cuda(), TransformerMixer(args).cuda()


def _time_major(base):
    out = {}
    for k, v in base.items():
        if k in ("obs_nrm_n", "obs_nrm"):  # per episode: no time axis
            out[k] = v
            continue
        out[k] = v.transpose(0, 1).contiguous().transpose(0, 1)
        assert out[k].stride(0) < out[k].stride(1)
    return out


def _slabs(base, arena):
    """Each field a [:, :T+1] slice of a slab two steps longer, its step stride and
    its episode stride padded (floats by multiples of 4 elements: every step stays
    16-byte aligned)."""
    out = {}
    for k, v in base.items():
        row = 1
        for n in v.shape[2:]:
            row *= n
        if v.dtype.is_floating_point:
            st = (row + 3) // 4 * 4 + 4
            sb = (v.shape[1] + 2) * st + 8
        else:
            st = row + 3
            sb = (v.shape[1] + 2) * st + 5
        inner, n = [], 1
        for s in reversed(v.shape[2:]):
            inner.append(n)
            n *= s
        out[k] = arena.place(v, (sb, st) + tuple(reversed(inner)), name=k)
        assert out[k].shape == v.shape and out[k].stride(0) > v.shape[1] * out[k].stride(1) and torch.equal(out[k], v)
    return out


def _check_case(A, B, T, precision, pipelined, base=None, presentations=("time-major", "slab"), agent_mixer=None,
                **learner_kw):
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.synthetic import make_batch
    agent, mixer = agent_mixer or _modules(A, False)
    learner = TDLearner(agent, mixer, precision=precision, priorities_to_cpu=False, **learner_kw)
    assert learner._pipelined(B) == pipelined, (learner.sa.instance, learner.sm.instance)
    if base is None:
        base, w = make_batch(B, T, A, seed=21)
        base = _ragged(base, 22)
    else:
        g = torch.Generator(device="cuda").manual_seed(23)
        w = 0.5 + 0.5 * torch.rand(B, device="cuda", generator=g)
    assert all(v.is_contiguous() for v in base.values())
    snap = (learner.params.clone(), learner.target_params.clone(), learner.exp_avg.clone(),
            learner.exp_avg_sq.clone(), learner.step_count)

    def update(batch):
        info = learner.train(batch, 0, 0, per_weight=w)
        torch.cuda.synchronize()
        out = dict(qtot=info["qtot"].clone(), targets=info["targets"].clone(),
                   td_errors_abs=info["td_errors_abs"].clone(), grad=learner.grad.clone(),
                   params=learner.params.clone())
        learner.params.copy_(snap[0])
        learner.target_params.copy_(snap[1])
        learner.exp_avg.copy_(snap[2])
        learner.exp_avg_sq.copy_(snap[3])
        learner.step_count = snap[4]
        learner._sync_replicas()  # (pack caches dropped, targets re-packed)
        return out

    ref = update(base)
    for k, v in ref.items():
        assert torch.isfinite(v).all(), k
    assert float(ref["grad"][-1]) > 0 and not torch.equal(ref["params"], snap[0])
    for how in presentations:
        arena = None
        if how == "time-major":
            batch = _time_major(base)
        else:
            arena = Arena(sum(4 * v.numel() * v.element_size() for v in base.values()) + (1 << 20), "cuda")
            batch = _slabs(base, arena)
            arena.check("before the update")
        got = update(batch)
        if arena is not None:
            arena.check(f"after the update on the {how} batch")
        for k, v in ref.items():
            assert torch.isfinite(got[k]).all(), (how, k)
            assert torch.equal(got[k], v), (how, k, int((got[k] != v).sum()), float((got[k] - v).abs().max()))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sequential_update_A8_across_layouts(precision):
    """8 AGVs x 3 episodes x T = 5: the exact agent and one-tile mixer instances,
    24 rows (1.5 tiles), the sequential update."""
    require_gpu()
    _check_case(8, 3, 5, precision, pipelined=False)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pipelined_update_A16_across_layouts(precision):
    """16 AGVs x 3 episodes x T = 4: the decoupled multi-tile mixer (19 query rows) and
    the agent BPTT in step ranges on two streams."""
    require_gpu()
    _check_case(16, 3, 4, precision, pipelined=True)


def test_runtime_instance_A5_across_layouts():
    """5 AGVs x 3 episodes x T = 4, fp32: the runtime-entity instances of capacity 8,
    15 rows (one partial tile)."""
    require_gpu()
    _check_case(5, 3, 4, "fp32", pipelined=False)


def test_q_lambda_update_A16_across_layouts():
    """Peng's Q(λ) targets (the taken mix and t2o_td_qlambda) at 16 AGVs, pipelined."""
    require_gpu()
    _check_case(16, 3, 4, "fp32", pipelined=True, q_lambda=True)


def test_noisy_agent_update_A8_across_layouts():
    """A NoisyNet agent (t2o_noisy_head_fwd / _bwd / _wgrad on the strided actions) at 8 AGVs."""
    require_gpu()
    _check_case(8, 3, 5, "fp32", pipelined=False, agent_mixer=_modules(8, True))


def test_wire_observations_A8_contiguous_and_time_major():
    """The compact wire observations of a VecEnv(wire=True) rollout (obs_wire, obs_nrm_n,
    obs_nrm; t2o_obs_expand reads the wire through its strides): contiguous and
    time-major, as the runner produced them."""
    require_gpu()
    from t2omca_amd.env import VecEnv
    from t2omca_amd.runner import RolloutRunner
    A, B, T = 8, 3, 5
    agent, mixer = _modules(A, False)
    env = VecEnv(B, mec_num=4, agv_num=A, episode_limit=T, seed=3, wire=True)
    env.get_env_info()
    batch = RolloutRunner(agent, env, seed=5, compact_obs=True, epsilon_start=0.5).run()
    assert "obs" not in batch and batch["obs_wire"].shape == (B, T + 1, A, 4)
    assert batch["obs_wire"].stride(0) < batch["obs_wire"].stride(1)  # the runner's time-major storage
    base = _ragged({k: v.contiguous() for k, v in batch.items()}, 22)
    _check_case(A, B, T, "fp32", pipelined=False, base=base, presentations=("time-major",),
                agent_mixer=(agent, mixer))
