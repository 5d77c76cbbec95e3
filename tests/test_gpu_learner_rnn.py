"""GPU: whole TD updates with the GRU agent (TDLearner with modules.RNNAgent under the
QMIX, VDN and QPLEX mixers) against the fp64 oracle, whose agent and mixer
are tests/rnn_model.td_forward_rnn's (substituted for ref_learner.td_forward with
monkeypatch.setattr, so that oracle_td_tie_aware / check_update work unchanged).

Modules: torch.manual_seed(module_seed(A)), the agent (entity observations, both
one-hots: IN = 9·A + 5 + A) first and then the mixer.  Batch: make_batch(seed 3) drawn on
the CPU, masked_avail seed 103, targets perturbed by 0.01·N(0, 1).  check_update asserts
the argmax preconditions (moved >= 0.25, gap >= 1e-4) and the per-block fitness
(grad_blocks.FIT_SHARE) in every case and prints their values.  The seed is 0 except at 8 AGVs:
there the seed-0 agent's masked argmax differs from the unmasked one at only 0.146 of
(b, t, a) on batch seed 3 (0.128 on seed 4; one action's Q dominates), under the 0.25 the
precondition asks, so its modules are drawn under seed 1 (0.500 / 0.465, gap 3.3e-3 /
3.2e-3).  With these seeds the fp64 model alone meets the preconditions and the fitness
at every shape and mixer (computed on the CPU before any GPU run).

The QPLEX mixer's seed.  Drawn straight after the agent, the QPLEX mixer gives at (3, 5, 4)
a key extractor's last bias (key_extractors.1.2.bias, one scalar) a share of 1.2e-4: fit by
FIT_SHARE, but that gradient is a sum over the rows of signed terms far larger than their
sum, which float32 arithmetic in any order loses (test_gpu_learner_qplex.py's docstring
describes the same block).  The fp64 oracle itself, evaluated in float32 on the CPU, is
2.5e-5 off on that block, at the 3e-5 bar, and <= 1.5e-6 on every other block of every
shape; the mixer kernels (which this agent does not change) measured 3.7e-5 there.  With
the QPLEX mixer drawn under module_seed(A) + 1, + 2, + 3 the float32 oracle's worst block
over the four shapes is 6.4e-6, 1.2e-5 and 1.6e-6: + 3 (QPLEX_MIXER_SEED) is the first draw
that leaves the float32 oracle within 2e-6 everywhere, chosen on the CPU from the oracle
alone.  The QMIX and VDN mixers are drawn straight after the agent.

Bars (the project's, test_gpu_learner_mixers.py's): qtot, targets, priorities 1e-5;
gradient 3e-5 flat and per parameter tensor.  Two gloo ranks against the full batch:
gradient 3e-5, parameters 1e-6.

The data-parallel case's seed.  Adam's first step is lr·g / (|g| + eps): where a
parameter's gradient lies within a few eps = 1e-8 of zero, a difference of 1e-9 between two
summation orders moves the parameter by a visible share of lr.  Of this agent's ~100,000
parameters some always do.  The fp64 oracle evaluated in float32 on the CPU, the full batch
against the sum of its two halves, gives gradients 3e-8 - 1.7e-7 apart (normwise) and
parameters after that step 4.5e-7 - 8e-6 apart over the module seeds 100 - 169; at seed 100
(test_gpu_learner_mixers.py's) 4.9e-8 and 6.0e-6, and the kernels measured 9.8e-8 and 6.6e-6
there: the gradient bar met 300 times over, the parameter bar missed as float32 itself
misses it.  DP_SEED = 110 is the first seed from 100 up at which the float32 oracle's
parameters stay under the bar (5.7e-7), chosen on the CPU from the oracle alone.

MEASURED on an MI355X, with this file's own draws (qmix / vdn / qplex; no ReLU tie overridden):

  (A, B, T)    moved / gap       qtot                   targets                prio                   grad                   (worst tensor)
  (3, 5, 4)    0.613 / 8.84e-3   2.6e-7 1.6e-7 8.7e-8   6.4e-8 1.1e-7 6.2e-8   1.7e-7 5.5e-8 4.4e-8   2.0e-7 1.1e-7 2.1e-7   (9.7e-7 3.4e-7 6.2e-7)
  (8, 6, 5)    0.500 / 3.30e-3   1.7e-7 2.1e-7 3.2e-7   1.3e-7 6.7e-8 8.4e-8   3.0e-7 9.1e-8 1.9e-7   1.1e-7 1.1e-7 1.5e-7   (4.4e-7 3.0e-7 1.0e-6)
  (16, 3, 4)   0.604 / 2.28e-3   1.8e-7 1.2e-7 1.2e-7   1.3e-7 7.2e-8 1.1e-7   2.2e-7 2.5e-8 1.9e-7   1.6e-7 6.1e-8 2.2e-7   (5.2e-7 1.7e-7 1.4e-6)
  (64, 2, 3)   0.459 / 1.25e-3   6.8e-7 5.3e-7 9.7e-7   1.8e-7 2.5e-7 3.8e-7   1.6e-7 6.1e-8 4.5e-7   1.8e-7 6.7e-8 7.1e-7   (1.2e-6 2.7e-7 1.4e-5)
  (the worst tensor is a mixer's in every qmix and qplex case, QPLEX's at 64 AGVs a key extractor's last bias with a
  share of 8.8e-5; the agent's own worst tensor is rnn.bias_hh / bias_ih / fc1.bias at <= 7.3e-7.)
  q_lambda, rmsprop, overlap=False at (8, 6, 5) and (16, 3, 4): every figure <= 3.8e-7, tensors <= 6.9e-7; qtot_taken
  <= 2.2e-7, qtot_tgt <= 1.7e-7; RMSprop transition square_avg 8.8e-9 / 2.9e-7, p 8.7e-9 / 8.9e-9 (bar 1.1e-7).
  The second update after the swap: figures <= 1.9e-7, tensors <= 7.3e-7; Adam step 2 m 6.2e-8 v 7.4e-8 p 7.5e-9
  (bar 2.0e-8).  precision="bf16" and a repeated update: bit-equal.  Two gloo ranks against the full batch: gradient
  1.7e-7, parameters 2.1e-7 (at seed 100: 9.8e-8 and 6.6e-6; see "The data-parallel case's seed" above).
  The mixer gradient is 1.3 (normwise) away from the transformer-agent learner's on the same batch, qtot 1.25.
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from tests import rnn_model
from tests.gpu_util import adam_errors, adam_ref, normwise, require_gpu, split_flat
from tests.qlambda_model import rmsprop_errors, rmsprop_ref
from tests.test_gpu_generic import _args, _cfg_of
from tests.test_gpu_learner_masks import (SEED, TOL, Snapshot, check_update, masked_batch, perturb_targets, to_cuda,
                                          update)
from tests.test_gpu_learner_qlambda import _preconditions

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 4), (8, 6, 5), (16, 3, 4), (64, 2, 3)]
OPTION_SHAPES = [(8, 6, 5), (16, 3, 4)]
KINDS = ["qmix", "vdn", "qplex"]
NA = 5
QPLEX_MIXER_SEED = 3


def module_seed(A):
    """The torch.manual_seed of a case's modules (module docstring)."""
    return 1 if A == 8 else 0


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)


def modules(A, kind, device="cuda", seed=None, n_actions=NA):
    from t2omca_amd.modules import make_agent, make_mixer
    torch.manual_seed(module_seed(A) if seed is None else seed)
    args = _args(_cfg_of(A, n_actions=n_actions), device=str(device))
    args.mixer, args.agent = kind, "rnn"
    agent = make_agent(9 * A + n_actions + A, args).to(device)
    if kind == "qplex":  # (module docstring: the QPLEX mixer's seed)
        torch.manual_seed((module_seed(A) if seed is None else seed) + QPLEX_MIXER_SEED)
    return agent, make_mixer(args).to(device)


def make_learner(A, kind, seed=None, n_actions=NA, **kw):
    from t2omca_amd.learner import TDLearner
    agent, mixer = modules(A, kind, seed=seed, n_actions=n_actions)
    assert agent.kind == "rnn" and mixer.kind == kind
    pa = {k: v.detach().cpu().double() for k, v in agent.state_dict().items()}
    pm = {k: v.detach().cpu().double() for k, v in mixer.state_dict().items()}
    return TDLearner(agent, mixer, **kw), pa, pm


def _oracle(monkeypatch, kind, **kw):
    from oracle import ref_learner
    monkeypatch.setattr(ref_learner, "td_forward", rnn_model.td_forward_rnn(kind, **kw))


def _update(monkeypatch, tag, kind, A, B, T, *, q_lambda=False, n_actions=NA, seed=None, **kw):
    """One update from perturbed targets against the substituted oracle at the fp32 bars."""
    learner, pa, pm = make_learner(A, kind, seed=seed, n_actions=n_actions, q_lambda=q_lambda, **kw)
    assert learner.agent_kind == "rnn" and learner.mixer_kind == kind and not learner._pipelined(B)
    assert list(pa) == list(rnn_model.KEYS) and learner.na == sum(v.numel() for v in pa.values())
    perturb_targets(learner)
    pat, pmt = split_flat(learner.target_params, pa, pm)
    cpu, w = masked_batch(A, B, T, SEED, n_actions)
    snap = Snapshot(learner)
    out, info = update(learner, to_cuda(cpu), w.cuda())
    _oracle(monkeypatch, kind, q_lambda=q_lambda)
    errs, g, ex = check_update(f"rnn {tag} {kind}", learner, pa, pm, _cfg_of(A, n_actions=n_actions), cpu, w, out,
                               pa_tgt=pat, pm_tgt=pmt)
    return learner, snap, out, info, ex, (cpu, w, g, pa, pm)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,B,T", SHAPES)
def test_update_fp32(monkeypatch, A, B, T, kind):
    require_gpu()
    _update(monkeypatch, f"({A},{B},{T})", kind, A, B, T)


def test_dispatch_took(monkeypatch):
    """Same batch and mixer: the GRU learner's na and gradient are not the transformer learner's."""
    require_gpu()
    from tests.test_gpu_learner_mixers import make_learner as make_transformer_agent_learner
    A, B, T = 8, 6, 5
    learner, _, out, _, _, (cpu, w, g, _, _) = _update(monkeypatch, "dispatch", "qmix", A, B, T)
    other, _, _ = make_transformer_agent_learner(_cfg_of(A), "qmix")
    assert getattr(other, "agent_kind", "transformer") == "transformer" and other.mixer_kind == "qmix"
    perturb_targets(other)
    (graw, qtot, _, _), _ = update(other, to_cuda(cpu), w.cuda())
    assert other.na != learner.na and other.nm == learner.nm
    diff = normwise(g[learner.na:], (graw[other.na:-1] / graw[-1]).cpu())
    print(f"rnn dispatch: mixer gradient {diff:.2e} away from the transformer-agent learner's, qtot "
          f"{normwise(out[1], qtot):.2e}")
    assert diff > 1e-3 and normwise(out[1], qtot) > 1e-3


OPTIONS = [("q_lambda", dict(q_lambda=True)), ("rmsprop", dict(optimizer="rmsprop", optim_alpha=0.99, optim_eps=1e-5)),
           ("serial", dict(overlap=False))]


@pytest.mark.parametrize("A,B,T", OPTION_SHAPES)
@pytest.mark.parametrize("name,kw", OPTIONS, ids=[o[0] for o in OPTIONS])
def test_options(monkeypatch, name, kw, A, B, T):
    require_gpu()
    learner, snap, out, info, ex, (cpu, w, g, _, _) = _update(monkeypatch, f"{name} ({A},{B},{T})", "qmix", A, B, T,
                                                               **kw)
    if name == "q_lambda":
        _preconditions(f"rnn {name} {A}", cpu, ex)
        ek, et = normwise(info["qtot_taken"], ex["qtot_taken"]), normwise(info["qtot_tgt"], ex["qtot_tgt"])
        print(f"rnn {name} {A}: qtot_taken {ek:.2e} qtot_tgt {et:.2e}")
        assert ek < TOL["fp32"][0] and et < TOL["fp32"][0], (ek, et)
    if name == "rmsprop":
        graw = out[0]
        ref = rmsprop_ref(snap.params, graw[:-1], snap.v, lr=learner.lr, alpha=0.99, eps=1e-5, weight_decay=0.0,
                          max_norm=learner.clip, grad_div=float(graw[-1]))
        es, ep, bar_p = rmsprop_errors(learner.params, learner.exp_avg_sq, ref, snap.params)
        print(f"rnn rmsprop {A}: square_avg {es:.2e} p {ep:.2e} (bar {bar_p:.2e})")
        assert es <= 1e-6 and ep <= bar_p, (es, ep, bar_p)
        assert learner.step_count == 1 and not learner.exp_avg.any()


@pytest.mark.parametrize("A,B,T", OPTION_SHAPES)
def test_bf16_equals_fp32_and_repeats(A, B, T):
    """precision='bf16' runs the same fp32 kernels: bit-equal outputs; and two updates
    from the same state are bit-equal."""
    require_gpu()
    cpu, w = masked_batch(A, B, T, SEED)
    outs = {}
    for prec in ("fp32", "bf16"):
        learner, _, _ = make_learner(A, "qmix", precision=prec)
        perturb_targets(learner)
        snap = Snapshot(learner)
        outs[prec], _ = update(learner, to_cuda(cpu), w.cuda())
        params = learner.params.clone()
        snap.restore()
        again, _ = update(learner, to_cuda(cpu), w.cuda())
        assert all(torch.equal(a, b) for a, b in zip(outs[prec], again)) and torch.equal(params, learner.params)
    assert all(torch.equal(a, b) for a, b in zip(outs["fp32"], outs["bf16"]))


@pytest.mark.parametrize("A,B,T", OPTION_SHAPES)
def test_second_update_after_target_swap(monkeypatch, A, B, T):
    """Update 0 fires the target swap (PyMARL's rule at interval 1, episode 1); update 1
    runs from the swapped targets and the first update's Adam moments."""
    require_gpu()
    learner, pa, pm = make_learner(A, "qmix", target_update_interval=1)
    perturb_targets(learner)
    cpu, w = masked_batch(A, B, T, SEED)
    update(learner, to_cuda(cpu), w.cuda(), episode_num=1)
    assert torch.equal(learner.target_params, learner.params) and learner.step_count == 1
    cpu2, w2 = masked_batch(A, B, T, SEED + 1)
    snap = Snapshot(learner)
    out, info = update(learner, to_cuda(cpu2), w2.cuda(), episode_num=1)
    pa_s, pm_s = split_flat(snap.params, pa, pm)
    pa_t, pm_t = split_flat(snap.targets, pa, pm)
    _oracle(monkeypatch, "qmix")
    check_update(f"rnn second update ({A},{B},{T})", learner, pa_s, pm_s, _cfg_of(A), cpu2, w2, out, pa_tgt=pa_t,
                 pm_tgt=pm_t)
    graw = out[0]
    ref = adam_ref(snap.params, graw[:-1], snap.m, snap.v, 2, lr=learner.lr, betas=learner.betas, eps=learner.eps,
                   weight_decay=learner.wd, max_norm=learner.clip, grad_div=float(graw[-1]))
    em, ev, ep, bar_p = adam_errors(learner.params, learner.exp_avg, learner.exp_avg_sq, ref, snap.params)
    print(f"rnn Adam step 2 ({A},{B},{T}): m {em:.2e} v {ev:.2e} p {ep:.2e} (bar {bar_p:.2e})")
    assert em <= 1e-6 and ev <= 1e-6 and ep <= bar_p, (em, ev, ep, bar_p)
    assert learner.step_count == 2 and torch.equal(learner.target_params, snap.targets)


# ---- checkpoints and state -----------------------------------------------------
def test_checkpoints_and_state(tmp_path):
    require_gpu()
    from tests.test_gpu_learner_mixers import make_learner as make_transformer_agent_learner
    A, B, T = 8, 6, 5
    learner, _, _ = make_learner(A, "qmix")
    cpu, w = masked_batch(A, B, T, SEED)
    update(learner, to_cuda(cpu), w.cuda())
    rnn_dir, tr_dir = tmp_path / "rnn", tmp_path / "transformer"
    rnn_dir.mkdir()
    tr_dir.mkdir()
    learner.save_models(str(rnn_dir))
    saved = torch.load(os.path.join(rnn_dir, "agent.th"), weights_only=True)
    assert tuple(saved) == rnn_model.KEYS
    assert {k: tuple(v.shape) for k, v in saved.items()} == rnn_model.shapes(9 * A + NA + A, 64, NA)
    fresh, _, _ = make_learner(A, "qmix")
    fresh.load_models(str(rnn_dir))
    assert torch.equal(fresh.params, learner.params) and fresh.step_count == learner.step_count == 1
    assert torch.equal(fresh.exp_avg, learner.exp_avg) and torch.equal(fresh.exp_avg_sq, learner.exp_avg_sq)
    assert torch.equal(fresh.target_params[:fresh.na], learner.params[:learner.na])
    sd = learner.state_dict()
    assert sd["agent"] == "rnn" and sd["mixer"] == "qmix" and sd["na"] == learner.na
    fresh2, _, _ = make_learner(A, "qmix")
    fresh2.load_state_dict(sd)
    assert torch.equal(fresh2.params, learner.params) and torch.equal(fresh2.target_params, learner.target_params)
    a, _ = update(learner, to_cuda(cpu), w.cuda(), 1)
    b, _ = update(fresh2, to_cuda(cpu), w.cuda(), 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the other kind of agent is refused in both directions, naming both kinds, before anything is overwritten
    other, _, _ = make_transformer_agent_learner(_cfg_of(A), "qmix")
    other.save_models(str(tr_dir))
    for ln, path, state in ((other, rnn_dir, sd), (fresh, tr_dir, other.state_dict())):
        before = ln.params.clone()
        with pytest.raises(ValueError, match=r"(?s)agent.*transformer.*rnn|agent.*rnn.*transformer"):
            ln.load_models(str(path))
        with pytest.raises(ValueError, match="agent"):
            ln.load_state_dict(state)
        assert torch.equal(ln.params, before)
    # a state saved before the field existed is a transformer agent's
    old = {k: v for k, v in other.state_dict().items() if k != "agent"}
    other.load_state_dict(old)
    with pytest.raises(ValueError, match="agent"):
        learner.load_state_dict({**old, "na": learner.na, "nm": learner.nm})


def test_unsupported_options():
    require_gpu()
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.modules import TransformerMixer
    agent, mixer = modules(8, "qmix")
    with pytest.raises(ValueError, match="flat mixers.*supported"):
        TDLearner(agent, TransformerMixer(_args(_cfg_of(8))).cuda())
    with pytest.raises(ValueError, match="pipeline=True"):
        TDLearner(agent, mixer, pipeline=True)
    agent.args.action_selector = "noisy-new"
    with pytest.raises(ValueError, match="noisy"):
        TDLearner(agent, mixer)
    agent.args.action_selector = "epsilon_greedy"
    for kw in (dict(contract="pair"), dict(detach_mixer_hidden=True), dict(pipeline="auto")):  # no effect
        learner = TDLearner(*modules(8, "qmix"), **kw)
        cpu, w = masked_batch(8, 6, 5, SEED)
        out, _ = update(learner, to_cuda(cpu), w.cuda())
        assert all(bool(torch.isfinite(x).all()) for x in out)


# ---- data parallel ---------------------------------------------------------------
DP_A, DP_B, DP_T = 8, 6, 5
DP_SEED = 110  # (module docstring: the data-parallel case's seed)


def _dp_learner(seed, device, pg=None):
    from t2omca_amd.learner import TDLearner
    return TDLearner(*modules(DP_A, "qmix", device=device, seed=seed), process_group=pg, target_update_interval=2)


def _dp_batch(device):
    cpu, w = masked_batch(DP_A, DP_B, DP_T, SEED)
    cpu["terminated"][1, 3] = 1  # ragged masks: the shards' Σ mask differ
    cpu["filled"][4, 4:] = 0
    return {k: v.to(device) for k, v in cpu.items()}, w.to(device)


def _dp_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from t2omca_amd.distributed import shard_bounds
        learner = _dp_learner(DP_SEED + rank, dev)  # different init per rank: the broadcast must fix it
        batch, w = _dp_batch(dev)
        lo, hi = shard_bounds(DP_B, rank, world)
        learner.train({k: v[lo:hi] for k, v in batch.items()}, 0, 0, per_weight=w[lo:hi])
        torch.cuda.synchronize()
        out.put((rank, torch.stack([learner.params, learner.grad[:-1] / learner.grad[-1]]).cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_dp_two_ranks():
    """Two gloo ranks on one device equal the full-batch update from the same state."""
    require_gpu()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=240) for _ in procs)
    finally:
        for p in procs:
            p.join(timeout=60)
    for p in procs:
        assert p.exitcode == 0
    r0, r1 = torch.from_numpy(res[0]), torch.from_numpy(res[1])
    assert torch.equal(r0, r1)
    dev = torch.device("cuda", 0)
    full = _dp_learner(DP_SEED, dev)
    batch, w = _dp_batch(dev)
    full.train(batch, 0, 0, per_weight=w)
    torch.cuda.synchronize()
    gerr = normwise(r0[1], (full.grad[:-1] / full.grad[-1]).cpu())
    err = normwise(r0[0], full.params.cpu())
    print(f"dp rnn qmix: grad {gerr:.2e}, params {err:.2e}")
    assert gerr < 3e-5 and err < 1e-6, (gerr, err)
