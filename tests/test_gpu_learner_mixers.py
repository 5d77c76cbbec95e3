"""GPU: whole TD updates with the QMIX and VDN mixers (TDLearner with modules.QMixer /
VDNMixer) against the fp64 oracle, whose mixer is tests/qmix_model's
restatement (substituted for ref_learner.td_forward with monkeypatch.setattr, so that
oracle_td_tie_aware / check_update work unchanged).

Modules: torch.manual_seed(0), the agent first and then the mixer.  Batch:
make_batch(seed 3) drawn on the CPU, masked_avail seed 103, targets perturbed by
0.01·N(0, 1).  check_update asserts the argmax preconditions (moved >= 0.25, gap >=
1e-4) and the per-block fitness (grad_blocks.FIT_SHARE) in every case and prints their
values, which the MEASURED table below records.

Bars (the project's): fp32 qtot, targets, priorities 1e-5; gradient 3e-5 flat and per
parameter block; bf16 (agent in bf16, mixer fp32) 2e-2 / 6e-2 with targets equal to
online, as test_gpu_learner_masks.test_masked_bf16.

MEASURED on an MI355X, with this file's own draws (qmix / vdn; no ReLU tie overridden):

  (A, B, T)    moved / gap       smallest share    qtot    targets prio    grad    (worst block)
  (3, 5, 4)    0.693 / 3.65e-3   5.0e-3 / 4.5e-3   2.3e-7  2.3e-7  8.4e-8  3.3e-7  (2.5e-6)  /  2.2e-7 1.8e-7 2.7e-7 3.0e-7 (9.4e-7)
  (8, 6, 5)    0.590 / 1.17e-3   3.2e-3 / 3.8e-3   3.1e-7  2.0e-7  1.0e-7  2.3e-7  (7.4e-7)  /  2.2e-7 2.0e-7 5.7e-8 1.1e-7 (4.7e-7)
  (5, 4, 6)    0.607 / 6.95e-4   1.1e-2 / 5.6e-3   2.4e-7  2.3e-7  1.9e-7  2.7e-7  (6.1e-7)  /  3.6e-7 1.4e-7 1.5e-7 1.4e-7 (7.5e-7)
  (16, 3, 4)   0.554 / 2.94e-3   4.1e-3 / 3.0e-3   2.6e-7  3.8e-7  1.9e-7  2.8e-7  (9.2e-7)  /  1.5e-7 3.6e-7 1.4e-7 9.5e-8 (3.7e-7)
  (64, 2, 3)   0.557 / 1.21e-3   3.5e-3 / 2.7e-3   6.9e-8  4.0e-7  1.1e-7  1.7e-7  (1.3e-6)  /  1.5e-7 1.1e-7 1.8e-7 2.1e-7 (3.9e-7)
  q_lambda, rmsprop, noisy, pair, overlap=False at (8, 6, 5) and (16, 3, 4): every figure <= 5.9e-7, blocks <= 9.2e-7;
  RMSprop transition square_avg 3.4e-7 / 7.3e-7, p 5.8e-8 / 5.9e-8 (bar 1.6e-7).
  bf16 (bars 2e-2 / 6e-2; qtot targets prio grad): (8, 6, 5) qmix 3.7e-3 6.8e-3 3.1e-3 6.8e-3, vdn 3.8e-3 5.9e-3 4.8e-3
  7.8e-3; (16, 3, 4) qmix 3.6e-3 6.5e-3 3.7e-3 5.1e-3, vdn 3.2e-3 7.1e-3 3.6e-3 4.1e-3; qtot against the fp64 mixer on
  last_qv <= 1.1e-7.  Two gloo ranks against the full batch: gradient 1.5e-7, parameters 4.5e-8.
  Every agent gradient is 0.86 - 1.0 (normwise) away from the transformer-mixer learner's on the same batch.
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from tests import qmix_model
from tests.gpu_util import normwise, require_gpu, split_flat
from tests.qlambda_model import rmsprop_errors, rmsprop_ref
from tests.test_gpu_generic import _args, _cfg_of
from tests.test_gpu_learner_masks import (SEED, TOL, Snapshot, check_update, masked_batch, perturb_targets, to_cuda,
                                          update)
from tests.test_gpu_learner_qlambda import _preconditions

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 4), (8, 6, 5), (5, 4, 6), (16, 3, 4), (64, 2, 3)]
OPTION_SHAPES = [(8, 6, 5), (16, 3, 4)]


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)


def modules(cfg, kind, noisy=False, device="cuda", seed=0):
    from t2omca_amd.modules import TransformerAgent, make_mixer
    torch.manual_seed(seed)
    args = _args(cfg, device=str(device))
    args.mixer = kind
    if noisy:
        args.action_selector = "noisy-new"
    agent = TransformerAgent(None, args).to(device)
    return agent, make_mixer(args).to(device)


def make_learner(cfg, kind, noisy=False, **kw):
    from t2omca_amd.learner import TDLearner
    agent, mixer = modules(cfg, kind, noisy)
    assert mixer.kind == kind
    pa = {k: v.detach().cpu().double() for k, v in agent.state_dict().items()}
    pm = {k: v.detach().cpu().double() for k, v in mixer.state_dict().items()}
    return TDLearner(agent, mixer, **kw), pa, pm


def _oracle(monkeypatch, kind, **kw):
    from oracle import ref_learner
    monkeypatch.setattr(ref_learner, "td_forward", qmix_model.td_forward_mixer(kind, **kw))


def _update(monkeypatch, tag, kind, A, B, T, *, noisy=False, q_lambda=False, n_actions=5, **kw):
    """One update from perturbed targets against the substituted oracle at the fp32 bars."""
    cfg = _cfg_of(A, n_actions=n_actions)
    learner, pa, pm = make_learner(cfg, kind, noisy=noisy, q_lambda=q_lambda, **kw)
    assert learner.mixer_kind == kind and not learner._pipelined(B)
    assert learner.nm == {"qmix": sum(v.numel() for v in pm.values()), "vdn": 0}[kind]
    perturb_targets(learner)
    pat, pmt = split_flat(learner.target_params, pa, pm)
    cpu, w = masked_batch(A, B, T, SEED, n_actions)
    snap = Snapshot(learner)
    out, info = update(learner, to_cuda(cpu), w.cuda())
    noise = None
    if noisy:
        noise = tuple((e[0].cpu().double(), e[1].cpu().double()) for e in learner.last_noise)
    _oracle(monkeypatch, kind, q_lambda=q_lambda, noise=noise)
    errs, g, ex = check_update(f"{tag} {kind}", learner, pa, pm, cfg, cpu, w, out, pa_tgt=pat, pm_tgt=pmt)
    qv_on, qv_tg = learner.last_qv
    assert qv_on.shape == (B, T, A) and qv_tg.shape == (B, T + 1, A)
    return learner, snap, out, info, ex, (cpu, w, g)


@pytest.mark.parametrize("kind", ["qmix", "vdn"])
@pytest.mark.parametrize("A,B,T", SHAPES)
def test_update_fp32(monkeypatch, A, B, T, kind):
    require_gpu()
    from tests.test_gpu_learner_masks import make_learner as make_transformer_learner
    learner, _, _, _, _, (cpu, w, g) = _update(monkeypatch, f"({A},{B},{T})", kind, A, B, T)
    # the dispatch took: the agent gradient differs from the transformer-mixer learner's on this batch
    other, _, _ = make_transformer_learner(_cfg_of(A), model_seed=0)
    perturb_targets(other)
    (graw, _, _, _), _ = update(other, to_cuda(cpu), w.cuda())
    na = learner.na
    assert other.na == na
    diff = normwise(g[:na], (graw[:na] / graw[-1]).cpu())
    print(f"({A},{B},{T}) {kind}: agent gradient {diff:.2e} away from the transformer-mixer learner's")
    assert diff > 1e-3, diff


OPTIONS = [("q_lambda", "qmix", dict(q_lambda=True)), ("q_lambda", "vdn", dict(q_lambda=True)),
           ("rmsprop", "qmix", dict(optimizer="rmsprop", optim_alpha=0.99, optim_eps=1e-5)),
           ("noisy", "qmix", dict(noisy=True)), ("pair", "qmix", dict(contract="pair")),
           ("serial", "qmix", dict(overlap=False))]


@pytest.mark.parametrize("A,B,T", OPTION_SHAPES)
@pytest.mark.parametrize("name,kind,kw", OPTIONS, ids=[f"{o[0]}-{o[1]}" for o in OPTIONS])
def test_options(monkeypatch, name, kind, kw, A, B, T):
    require_gpu()
    learner, snap, out, info, ex, (cpu, w, g) = _update(monkeypatch, f"{name} ({A},{B},{T})", kind, A, B, T, **kw)
    if name == "q_lambda":
        _preconditions(f"{name} {kind} {A}", cpu, ex)
        ek, et = normwise(info["qtot_taken"], ex["qtot_taken"]), normwise(info["qtot_tgt"], ex["qtot_tgt"])
        print(f"{name} {kind} {A}: qtot_taken {ek:.2e} qtot_tgt {et:.2e}")
        assert ek < TOL["fp32"][0] and et < TOL["fp32"][0], (ek, et)
    if name == "rmsprop":
        graw = out[0]
        ref = rmsprop_ref(snap.params, graw[:-1], snap.v, lr=learner.lr, alpha=0.99, eps=1e-5, weight_decay=0.0,
                          max_norm=learner.clip, grad_div=float(graw[-1]))
        es, ep, bar_p = rmsprop_errors(learner.params, learner.exp_avg_sq, ref, snap.params)
        print(f"rmsprop {A}: square_avg {es:.2e} p {ep:.2e} (bar {bar_p:.2e})")
        assert es <= 1e-6 and ep <= bar_p, (es, ep, bar_p)
        assert learner.step_count == 1 and not learner.exp_avg.any()
    if name == "noisy":
        assert learner.noisy and float(g[learner.na_net:learner.na].abs().max()) > 0


@pytest.mark.parametrize("kind", ["qmix", "vdn"])
@pytest.mark.parametrize("A,B,T", OPTION_SHAPES)
def test_bf16(monkeypatch, A, B, T, kind):
    """A bf16 agent under the fp32 mixers, targets equal to online.  Measured: see the
    module docstring's reference."""
    require_gpu()
    cfg = _cfg_of(A)
    learner, pa, pm = make_learner(cfg, kind, precision="bf16")
    cpu, w = masked_batch(A, B, T, SEED)
    snap = Snapshot(learner)
    out, info = update(learner, to_cuda(cpu), w.cuda())
    assert all(bool(torch.isfinite(x).all()) for x in out)
    # the mixer is fp32: qtot is the restatement on the GPU's own chosen Q
    qv = learner.last_qv[0].cpu().double()
    want = qmix_model.mix(kind, pm, qv, cpu["state"][:, :T].double())
    eq = normwise(info["qtot"], want)
    print(f"bf16 ({A},{B},{T}) {kind}: qtot against the fp64 mixer on last_qv {eq:.2e}")
    assert eq < 1e-5, eq
    _oracle(monkeypatch, kind)
    check_update(f"bf16 ({A},{B},{T}) {kind}", learner, pa, pm, cfg, cpu, w, out, blocks=False)
    snap.restore()
    again, _ = update(learner, to_cuda(cpu), w.cuda())
    assert all(torch.equal(a, b) for a, b in zip(out, again))


# ---- checkpoints and state -----------------------------------------------------
@pytest.mark.parametrize("kind", ["qmix", "vdn"])
def test_checkpoints_and_state(tmp_path, kind):
    require_gpu()
    from tests.test_gpu_learner_masks import make_learner as make_transformer_learner
    A, B, T = 8, 6, 5
    cfg = _cfg_of(A)
    learner, _, pm = make_learner(cfg, kind)
    cpu, w = masked_batch(A, B, T, SEED)
    update(learner, to_cuda(cpu), w.cuda())
    learner.save_models(str(tmp_path))
    saved = torch.load(os.path.join(tmp_path, "mixer.th"), weights_only=True)
    assert list(saved) == (list(qmix_model.KEYS) if kind == "qmix" else [])
    fresh, _, _ = make_learner(cfg, kind)
    fresh.load_models(str(tmp_path))
    assert torch.equal(fresh.params, learner.params) and fresh.step_count == learner.step_count == 1
    assert torch.equal(fresh.exp_avg, learner.exp_avg) and torch.equal(fresh.exp_avg_sq, learner.exp_avg_sq)
    sd = learner.state_dict()
    assert sd["mixer"] == kind and sd["nm"] == learner.nm
    fresh2, _, _ = make_learner(cfg, kind)
    fresh2.load_state_dict(sd)
    assert torch.equal(fresh2.params, learner.params) and torch.equal(fresh2.target_params, learner.target_params)
    # both continue bit for bit
    a, _ = update(learner, to_cuda(cpu), w.cuda(), 1)
    b, _ = update(fresh2, to_cuda(cpu), w.cuda(), 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # another kind's checkpoint or run state is refused, naming both, before anything is overwritten
    other_kind = "vdn" if kind == "qmix" else "qmix"
    for other, name in ((make_learner(cfg, other_kind)[0], other_kind),
                        (make_transformer_learner(cfg, model_seed=0)[0], "transformer")):
        before = other.params.clone()
        with pytest.raises(ValueError, match=rf"{kind}.*{name}"):
            other.load_models(str(tmp_path))
        with pytest.raises(ValueError, match="mixer"):
            other.load_state_dict(sd)
        assert torch.equal(other.params, before)
    # a state saved before the field existed is a transformer mixer's
    tr = make_transformer_learner(cfg, model_seed=0)[0]
    old = {k: v for k, v in tr.state_dict().items() if k != "mixer"}
    tr.load_state_dict(old)
    with pytest.raises(ValueError, match="mixer"):
        learner.load_state_dict({**old, "na": learner.na, "nm": learner.nm})


@pytest.mark.parametrize("kind", ["qmix", "vdn"])
def test_pipeline_option(kind):
    require_gpu()
    from t2omca_amd.learner import TDLearner
    cfg = _cfg_of(16)
    with pytest.raises(ValueError, match="pipeline=True"):
        TDLearner(*modules(cfg, kind), pipeline=True)
    learner = TDLearner(*modules(cfg, kind), pipeline="auto")
    cpu, w = masked_batch(16, 3, 4, SEED)
    out, _ = update(learner, to_cuda(cpu), w.cuda())
    assert all(bool(torch.isfinite(x).all()) for x in out)


def test_logging():
    require_gpu()
    from t2omca_amd.statlog import StatsLogger
    for kind in ("qmix", "vdn"):
        log = StatsLogger(out=lambda line: None)
        learner, _, _ = make_learner(_cfg_of(8), kind, logger=log, learner_log_interval=1)
        cpu, w = masked_batch(8, 6, 5, SEED)
        learner.train(to_cuda(cpu), 10, 0, per_weight=w.cuda())
        torch.cuda.synchronize()
        recent = log.recent()
        assert set(recent) >= {"loss_td", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"}, recent
        assert all(torch.isfinite(torch.tensor(v)) for v in recent.values()), recent


# ---- data parallel ---------------------------------------------------------------
DP_A, DP_B, DP_T = 8, 6, 5


def _dp_learner(seed, device, pg=None):
    from t2omca_amd.learner import TDLearner
    return TDLearner(*modules(_cfg_of(DP_A), "qmix", device=device, seed=seed), process_group=pg,
                     target_update_interval=2)


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
        learner = _dp_learner(100 + rank, dev)  # different init per rank: the broadcast must fix it
        batch, w = _dp_batch(dev)
        lo, hi = shard_bounds(DP_B, rank, world)
        learner.train({k: v[lo:hi] for k, v in batch.items()}, 0, 0, per_weight=w[lo:hi])
        torch.cuda.synchronize()
        out.put((rank, torch.stack([learner.params, learner.grad[:-1] / learner.grad[-1]]).cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_dp_two_ranks_qmix():
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
    full = _dp_learner(100, dev)
    batch, w = _dp_batch(dev)
    full.train(batch, 0, 0, per_weight=w)
    torch.cuda.synchronize()
    gerr = normwise(r0[1], (full.grad[:-1] / full.grad[-1]).cpu())
    err = normwise(r0[0], full.params.cpu())
    print(f"dp qmix: grad {gerr:.2e}, params {err:.2e}")
    assert gerr < 1e-6 and err < 1e-6, (gerr, err)
