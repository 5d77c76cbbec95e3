"""GPU: the whole TD update against the fp64 oracle with masked actions and target
networks that differ from the online ones; post-termination data must not matter.

Every other whole-update oracle test feeds synthetic.make_batch (all actions
available) and all but one leave target == online, where "target Q at the
avail-masked online argmax" equals "max of the target Q": a double-Q selection
(mix_qv, qmode 2) that takes the argmax of the wrong network or ignores avail
passes them.  Here

  * avail_actions is tests/gpu_util.masked_avail (Bernoulli(0.5) per action, action
    0 always available, agent 0 down to action 0 everywhere, one (b, t) with every
    agent down to it, step T drawn like the rest), seeded batch seed + 100, passed
    as the int32 the kernels read and once more as uint8, which the learner converts;
  * the fp32 cases perturb the target parameters by 0.01·N(0, 1) and give the oracle
    those targets;
  * the batch is make_batch(seed=3) drawn on the CPU (so the preconditions below
    can be, and were, computed without a device) and the modules torch.manual_seed(0)
    up to 12 AGVs, 4 from 13 (tests/grad_blocks.module_seed: with seed 0 the mixer's
    hyper_b2 ReLU is off at every record of these short unrolls and its reference
    gradient identically zero, which no per-block comparison can use).

Preconditions, computed from the oracle alone and asserted in every case, so that a
pass means something: (a) the masked argmax differs from the unmasked one in >= 25 %
of (b, t, a); (b) the smallest top-two gap of the oracle's masked online Q over rows
with >= 2 available actions is >= 1e-4·max|Q|, 10x the fp32 forward bar, so fp32
cannot legitimately pick another action.  Their values at seed 3:

  (A, B, T)        moved   gap            (A, B, T)          moved   gap
  (8, 6, 5)        0.590   1.17e-03       (13, 3, 5)         0.573   3.08e-03
  (3, 5, 4)        0.693   3.65e-03       (40, 2, 4)         0.542   2.31e-03
  (16, 3, 4)       0.533   1.61e-03       (63, 2, 3)         0.567   2.92e-03
  (64, 2, 3)       0.574   6.78e-04       (5, 4, 6)          0.607   6.95e-04
  (8, 3, 5) emb 64 / 4 heads, generic     0.535   6.38e-04

fp32 bars (the project's): qtot, targets, priorities <= 1e-5, gradients <= 3e-5
against the tie-aware oracle.  bf16 (2e-2 / 6e-2) runs the same masks with targets
EQUAL to online: bf16 Q errors (~1e-2) do flip near-tied argmaxes, and only with
equal networks does a flip change the target by no more than the gap itself (which
is why the existing bf16 tests pass); with distinct targets a flip would move the
target by the networks' difference at another action, which no bf16 bar covers.

detach_mixer_hidden=True (gh=None into the agent BPTT, sequential and pipelined) is
checked against the oracle run with the same flag, and its gradient must differ
from the attached run's by > 1e-3 normwise.

test_post_termination_data_is_ignored needs no oracle: every episode terminates at
its own step L_b (L_b = 0 and T-1 included; terminated[b, L_b] = 1, filled 0
after); a second batch replaces obs, state, reward, actions and avail at every step
> L_b by other finite draws.  PyMARL's recursion gives ret_t = 0 and m_t = 0 past
L_b, so those steps enter every sum as exact zeros, and the update is
bit-reproducible: the raw gradient (Σ mask slot included), the priorities, and
qtot / targets at t <= L_b must be torch.equal between the two runs.

Measured on an MI355X (normwise qtot / targets / priorities / gradient; no ReLU tie
was overridden in any case; the rows from 13 AGVs up with the seed-0 modules used
before the per-block check, whose figures per case are in DESIGN.md §5):
  exact-8                  5.8e-7  3.7e-7  2.1e-7  2.7e-7
  two-tile-decoupled-16    4.1e-7  3.6e-7  2.3e-7  1.7e-7
  two-tile-one-wave-16     4.1e-7  3.6e-7  2.3e-7  1.8e-7
  five-tile-64             1.3e-7  4.6e-7  2.4e-7  5.8e-7
  exact-3                  3.2e-7  2.9e-7  4.7e-7  5.4e-7
  runtime-5                3.3e-7  1.5e-7  2.0e-7  3.6e-7
  runtime-13               3.7e-7  7.2e-7  3.5e-7  5.1e-7
  runtime-40               1.1e-7  5.1e-7  4.1e-7  4.1e-7
  runtime-63               8.3e-8  1.1e-6  3.8e-7  1.1e-6
  generic-5                2.3e-7  3.9e-7  2.0e-7  1.8e-7
  generic-E64H4            2.3e-7  9.2e-8  2.0e-7  1.2e-7
  bf16-8                   1.0e-2  7.9e-3  6.3e-3  8.4e-3
  bf16-16                  4.8e-3  8.3e-3  6.1e-3  5.7e-3
  bf16-64                  1.2e-3  1.0e-2  7.6e-3  4.8e-2
  detach-8 / detach-16     5.8e-7  3.7e-7  2.1e-7  1.3e-7 / 4.1e-7  3.6e-7  2.3e-7  1.2e-7
                           (gradient 2.1e-1 / 3.0e-1 away from the attached run's)
The uint8 run equals the int32 run bit for bit on the MFMA instances; the generic
kernels' gradient differs by 1.2e-7 / 2.3e-7 (their float atomics), so that
comparison is held to 1e-6, the summation-order bar of test_gpu_fullgrid.py.
Post-termination: 0 of 84007 raw gradient elements differ, fp32 and bf16, both shapes.
"""
import pytest
import torch

from tests.gpu_util import (argmax_preconditions, masked_avail, normwise, oracle_td_tie_aware, require_gpu,
                            split_flat)
from tests.grad_blocks import assert_blocks_bf16, assert_blocks_fp32, emulated_bf16_grad, module_seed
from tests.test_gpu_generic import _args, _cfg_of

pytestmark = pytest.mark.gpu

TOL = {"fp32": (1e-5, 3e-5), "bf16": (2e-2, 6e-2)}
SEED = 3


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    """The tuned instances and the default mixer choice unless a case says otherwise."""
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)


def make_learner(cfg, model_seed=None, **kw):
    """(learner, pa, pm); the modules drawn with torch.manual_seed(model_seed), by default
    grad_blocks.module_seed(A), which leaves every parameter block a gradient to compare."""
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.modules import TransformerAgent, TransformerMixer
    torch.manual_seed(module_seed(cfg["n_agents"]) if model_seed is None else model_seed)
    args = _args(cfg)
    agent, mixer = TransformerAgent(None, args).cuda(), TransformerMixer(args).cuda()
    pa = {k: v.detach().cpu().double() for k, v in agent.state_dict().items()}
    pm = {k: v.detach().cpu().double() for k, v in mixer.state_dict().items()}
    return TDLearner(agent, mixer, **kw), pa, pm


def masked_batch(A, B, T, seed, n_actions=5):
    """make_batch drawn on the CPU with the masked avail_actions; CPU tensors."""
    from t2omca_amd.synthetic import make_batch
    batch, w = make_batch(B, T, A, n_actions=n_actions, seed=seed, device="cpu")
    batch["avail_actions"] = masked_avail(B, T + 1, A, n_actions, seed=seed + 100)
    return batch, w


def to_cuda(batch):
    return {k: v.cuda() for k, v in batch.items()}


def perturb_targets(learner, seed=1):
    g = torch.Generator().manual_seed(seed)
    learner.target_params.add_((0.01 * torch.randn(learner.target_params.numel(), generator=g)).cuda())
    learner._pack_targets()


class Snapshot:
    """The learner's state before an update (to run another update from it)."""

    def __init__(self, learner):
        self.learner = learner
        self.params, self.targets = learner.params.clone(), learner.target_params.clone()
        self.m, self.v, self.step = learner.exp_avg.clone(), learner.exp_avg_sq.clone(), learner.step_count
        self.last = learner.last_target_update_episode

    def restore(self):
        ln = self.learner
        ln.params.copy_(self.params)
        ln.target_params.copy_(self.targets)
        ln.exp_avg.copy_(self.m)
        ln.exp_avg_sq.copy_(self.v)
        ln.step_count, ln.last_target_update_episode = self.step, self.last
        ln._params_written()
        ln._pack_targets()


def update(learner, batch, w, episode_num=0):
    """One train(); returns clones of (raw grad, qtot, targets, priorities), info."""
    info = learner.train(batch, 0, episode_num, per_weight=w)
    torch.cuda.synchronize()
    return (learner.grad.clone(), info["qtot"].clone(), info["targets"].clone(),
            info["td_errors_abs"].clone().cpu()), info


def check_update(tag, learner, pa, pm, cfg, batch, w, out, *, pa_tgt=None, pm_tgt=None, detach=False, blocks=True):
    """One update's (raw grad, qtot, targets, prio) against the tie-aware fp64 oracle
    at the precision's bars, the argmax preconditions asserted; the gradient flat and
    per parameter block (fp32: each block < 3e-5 of its own maximum; bf16: each block's
    relative L2 <= max(2^-8, 4 x the bf16-operand emulation of the oracle)); returns the
    errors, the normalised gradient and the oracle's extras."""
    graw, qtot, targets, prio = out
    g = (graw[:-1] / graw[-1]).cpu()
    fp32 = learner.precision == "fp32"
    o_prio, ex, ref_g, ties = oracle_td_tie_aware(pa, pm, cfg, batch, w, g if fp32 else None, pa_tgt=pa_tgt,
                                                  pm_tgt=pm_tgt, detach_mixer_hidden=detach)
    moved, gap = argmax_preconditions(ex["mac_out"], batch["avail_actions"])
    errs = dict(qtot=normwise(qtot, ex["qtot"]), targets=normwise(targets, ex["targets"]),
                prio=normwise(prio, o_prio), grad=normwise(g, ref_g))
    print(f"{tag} {learner.precision}: argmax moved {moved:.3f} gap {gap:.2e};",
          {k: f"{v:.2e}" for k, v in errs.items()}, "relu ties", ties)
    assert moved >= 0.25, moved
    assert gap >= 1e-4, gap
    tf, tg = TOL[learner.precision]
    assert errs["qtot"] < tf and errs["targets"] < tf and errs["prio"] < tf, errs
    assert errs["grad"] < tg, errs
    # every parameter block on its own scale (tests/grad_blocks.py)
    if not blocks:
        pass
    elif fp32:
        assert_blocks_fp32(g, ref_g, pa, pm, tag=tag)
    else:
        emu = emulated_bf16_grad(pa, pm, cfg, batch, w, pa_tgt=pa_tgt, pm_tgt=pm_tgt, detach_mixer_hidden=detach)
        assert_blocks_bf16(g, ref_g, emu, pa, pm, tag=tag)
    ex["ref_grad"] = ref_g
    return errs, g, ex


def _case(tag, cfg, B, T, precision="fp32", distinct=True, detach=False, instance=None, piped=None):
    learner, pa, pm = make_learner(cfg, precision=precision, detach_mixer_hidden=detach)
    if instance is not None:
        assert learner.sa.instance == instance and learner.sm.instance == instance
    if piped is not None:
        assert bool(learner._pipelined(B)) == piped
    pat = pmt = None
    if distinct:
        perturb_targets(learner)
        pat, pmt = split_flat(learner.target_params, pa, pm)
    cpu, w = masked_batch(cfg["n_agents"], B, T, SEED)
    snap = Snapshot(learner)
    out, _ = update(learner, to_cuda(cpu), w.cuda())
    errs, g, ex = check_update(tag, learner, pa, pm, cfg, cpu, w, out, pa_tgt=pat, pm_tgt=pmt, detach=detach)
    # avail_actions as uint8 (the learner converts): the same update
    snap.restore()
    cpu8 = dict(cpu, avail_actions=cpu["avail_actions"].to(torch.uint8))
    (graw, qtot, targets, prio), _ = update(learner, to_cuda(cpu8), w.cuda())
    tf, tg = TOL[precision]
    e8 = dict(qtot=normwise(qtot, out[1]), targets=normwise(targets, out[2]), prio=normwise(prio, out[3]),
              grad=normwise(graw, out[0]))
    print(f"{tag} uint8 avail vs int32:", {k: f"{v:.2e}" for k, v in e8.items()})
    assert normwise(qtot, ex["qtot"]) < tf and normwise(targets, ex["targets"]) < tf
    assert normwise((graw[:-1] / graw[-1]).cpu(), ex["ref_grad"]) < tg
    assert e8["qtot"] < 1e-6 and e8["targets"] < 1e-6 and e8["prio"] < 1e-6 and e8["grad"] < 1e-6, e8
    return g


FP32_CASES = [
    # tag, A, B, T, env, instance, pipelined
    ("exact-8", 8, 6, 5, {}, "exact", False),
    ("two-tile-decoupled-16", 16, 3, 4, {}, "exact", True),
    ("two-tile-one-wave-16", 16, 3, 4, {"T2O_MIXER_SPLIT": "0"}, "exact", False),
    ("five-tile-64", 64, 2, 3, {}, "exact", None),
    # (3 AGVs with the default network has an exact instance of its own; 5 AGVs is
    # the padded runtime-entity instance below the one-tile boundary instead)
    ("exact-3", 3, 5, 4, {}, "exact", False),
    ("runtime-5", 5, 4, 6, {}, "runtime", False),
    ("runtime-13", 13, 3, 5, {}, "runtime", False),
    ("runtime-40", 40, 2, 4, {}, "runtime", None),
    ("runtime-63", 63, 2, 3, {}, "runtime", None),
]


@pytest.mark.parametrize("tag,A,B,T,env,instance,piped", FP32_CASES, ids=[c[0] for c in FP32_CASES])
def test_masked_distinct_targets_fp32(monkeypatch, tag, A, B, T, env, instance, piped):
    require_gpu()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _case(tag, _cfg_of(A), B, T, instance=instance, piped=piped)


@pytest.mark.parametrize("tag,cfg,B,T", [("generic-5", _cfg_of(5), 4, 6),
                                         ("generic-E64H4", _cfg_of(8, E=64, H=4), 3, 5)],
                         ids=["generic-5", "generic-E64H4"])
def test_masked_distinct_targets_generic(monkeypatch, tag, cfg, B, T):
    """T2O_GENERIC=1: the runtime-shaped kernels' own double-Q selection."""
    require_gpu()
    monkeypatch.setenv("T2O_GENERIC", "1")
    _case(tag, cfg, B, T, instance="generic")


@pytest.mark.parametrize("A,B,T", [(8, 6, 5), (16, 3, 4), (64, 2, 3)])
def test_masked_bf16(A, B, T):
    """bf16 with the same masks and targets equal to online: a near-tied argmax that
    bf16 flips then changes the target only by the gap itself (module docstring)."""
    require_gpu()
    _case(f"bf16-{A}", _cfg_of(A), B, T, precision="bf16", distinct=False)


@pytest.mark.parametrize("A,B,T,piped", [(8, 6, 5, False), (16, 3, 4, True)])
def test_detach_mixer_hidden(A, B, T, piped):
    """detach_mixer_hidden=True: no gradient from the mixer's hidden-state input into
    the agent BPTT (gh=None), against the oracle with the same flag; the flag must
    change the gradient."""
    require_gpu()
    g_det = _case(f"detach-{A}", _cfg_of(A), B, T, detach=True, piped=piped)
    g_att = _case(f"attached-{A}", _cfg_of(A), B, T, detach=False, piped=piped)
    diff = normwise(g_det, g_att)
    print(f"detach-{A}: gradient differs from the attached run's by {diff:.2e}")
    assert diff > 1e-3, diff


def _terminating(cpu, lengths):
    """Episode b terminates at step lengths[b]: terminated there, filled 0 after."""
    B, T1 = cpu["filled"].shape[:2]
    term = torch.zeros(B, T1, 1, dtype=torch.uint8)
    filled = torch.ones(B, T1, 1, dtype=torch.int64)
    for b, L in enumerate(lengths):
        term[b, L, 0] = 1
        filled[b, L + 1:, 0] = 0
    return dict(cpu, terminated=term, filled=filled)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("A,B,T,piped", [(8, 6, 5, False), (16, 3, 4, True)])
def test_post_termination_data_is_ignored(A, B, T, piped, precision):
    require_gpu()
    lengths = ([0, T - 1] + [(2 * i + 1) % T for i in range(B)])[:B]
    learner, _, _ = make_learner(_cfg_of(A), precision=precision)
    assert bool(learner._pipelined(B)) == piped
    perturb_targets(learner)
    one, w = masked_batch(A, B, T, SEED)
    one = _terminating(one, lengths)
    other, _ = masked_batch(A, B, T, SEED + 50)
    two = dict(one)
    for k in ("obs", "state", "reward", "actions", "avail_actions"):
        two[k] = one[k].clone()
        for b, L in enumerate(lengths):
            two[k][b, L + 1:] = other[k][b, L + 1:]
    snap = Snapshot(learner)
    g1, q1, t1, p1 = update(learner, to_cuda(one), w.cuda())[0]
    snap.restore()
    g2, q2, t2, p2 = update(learner, to_cuda(two), w.cuda())[0]
    assert torch.isfinite(g1).all() and torch.isfinite(q2).all() and torch.isfinite(t2).all()
    assert float(g1[-1]) == float(sum(L + 1 for L in lengths))
    # the replaced steps did reach the kernels: Q_tot past an early end differs
    assert any(not torch.equal(q1[b, L + 1:], q2[b, L + 1:]) for b, L in enumerate(lengths) if L + 1 < T)
    ndiff = int((g1 != g2).sum())
    print(f"A={A} {precision}: raw gradient elements differing {ndiff} of {g1.numel()}, "
          f"normwise {normwise(g2, g1):.2e}")
    assert torch.equal(g1, g2), ndiff
    assert torch.equal(p1, p2)
    for b, L in enumerate(lengths):
        assert torch.equal(q1[b, :L + 1], q2[b, :L + 1]), b
        assert torch.equal(t1[b, :L + 1], t2[b, :L + 1]), b
