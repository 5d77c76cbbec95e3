"""GPU: whole TD updates with the learner's two other PyMARL2 switches, q_lambda=True
(Peng's Q(λ) targets, t2o_td_qlambda fed by a third mixer unroll: the target mixer on
the target Q at the batch's actions) and optimizer="rmsprop" (t2o_rmsprop_step),
against tests/qlambda_model.td_forward_qlambda through the tie-aware fp64 oracle
(tests.gpu_util.oracle_td_tie_aware looks ref_learner.td_forward up when called, so
the Q(λ) version is substituted with monkeypatch.setattr).

Inputs are those of tests/test_gpu_learner_masks.py (its helpers imported): batch seed
3 drawn on the CPU, masked_avail seed 103, target parameters perturbed by 0.01·N(0, 1);
bars TOL["fp32"]: 1e-5 on qtot, targets, qtot_taken and priorities, 3e-5 on the gradient.

Preconditions, from the oracle alone, asserted in every fp32 case (beside check_update's
argmax ones): the share of (b, t) with |Q'_t − Qk_t| > 1e-3·max|Q'| is >= 0.5, and the
Q(λ) targets differ from the TD(λ) targets of the same target mix by >= 1e-2 normwise
— a learner that dropped the correction, or fed the kernel the double-Q mix twice,
fails the targets bar by orders of magnitude.  Computed on the CPU at seed 3:
share 1.000 at (8,6,5), (3,5,4), (16,3,4) and (5,4,6); difference 1.1 - 3.1.

The RMSprop transition is checked, like the Adam one in test_gpu_learner_steps.py, on
the learner's own normalised gradient against rmsprop_ref.  bf16 operands do not reach
the target kernel: info["targets"] must equal the fp64 formula on the GPU's own target
mix and taken mix at the fp32 bar.  Every update is bit-reproducible run to run
(pipelined and bf16 cases here).  Checkpoints: opt.th is a standard torch RMSprop
state_dict, load_models / load_state_dict resume bit for bit, and files or states of
the other optimiser are a ValueError naming both.  Data parallel: two gloo ranks on one
device equal the full-batch update from their state.
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from oracle.ref_learner import build_td_lambda_targets
from tests.gpu_util import normwise, require_gpu, split_flat
from tests.qlambda_model import build_q_lambda_targets, rmsprop_errors, rmsprop_ref, td_forward_qlambda
from tests.test_gpu_generic import _cfg_of
from tests.test_gpu_learner_masks import (SEED, TOL, Snapshot, check_update, make_learner, masked_batch,
                                          perturb_targets, to_cuda, update)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    """The tuned instances and the default mixer choice unless a case says otherwise."""
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)


def _masks(cpu):
    term = cpu["terminated"][:, :-1, 0].double()
    mask = cpu["filled"][:, :-1, 0].double()
    mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
    return cpu["reward"][:, :-1, 0].double(), term, mask


def _preconditions(tag, cpu, ex, gamma=0.99, lam=0.6):
    """From the oracle's extras alone: the correction is there and moves the targets."""
    q1, qk = ex["qtot_tgt"].double(), ex["qtot_taken"].double()
    share = float(((q1[:, :-1] - qk).abs() > 1e-3 * q1.abs().max()).double().mean())
    r, term, mask = _masks(cpu)
    diff = normwise(ex["targets"], build_td_lambda_targets(r, term, mask, q1, gamma, lam))
    print(f"{tag}: |Q' - Qk| > 1e-3 max|Q'| at {share:.3f} of (b, t); Q(λ) vs TD(λ) targets {diff:.2e}")
    assert share >= 0.5, share
    assert diff >= 1e-2, diff


def _ql_update(monkeypatch, tag, cfg, B, T, *, instance=None, piped=None, **kw):
    """One q_lambda update from perturbed targets against the Q(λ) oracle at the fp32
    bars; returns (learner, snapshot before it, its outputs, info, oracle extras)."""
    from oracle import ref_learner
    monkeypatch.setattr(ref_learner, "td_forward", td_forward_qlambda)
    learner, pa, pm = make_learner(cfg, q_lambda=True, **kw)
    if instance is not None:
        assert learner.sa.instance == instance and learner.sm.instance == instance
    if piped is not None:
        assert bool(learner._pipelined(B)) == piped
    perturb_targets(learner)
    pat, pmt = split_flat(learner.target_params, pa, pm)
    cpu, w = masked_batch(cfg["n_agents"], B, T, SEED)
    snap = Snapshot(learner)
    out, info = update(learner, to_cuda(cpu), w.cuda())
    errs, g, ex = check_update(tag, learner, pa, pm, cfg, cpu, w, out, pa_tgt=pat, pm_tgt=pmt)
    _preconditions(tag, cpu, ex)
    assert info["qtot_taken"].shape == (B, T) and info["qtot_tgt"].shape == (B, T + 1)
    ek, et = normwise(info["qtot_taken"], ex["qtot_taken"]), normwise(info["qtot_tgt"], ex["qtot_tgt"])
    print(f"{tag}: qtot_taken {ek:.2e} qtot_tgt {et:.2e}")
    assert ek < TOL["fp32"][0] and et < TOL["fp32"][0], (ek, et)
    return learner, snap, out, info, ex, (cpu, w)


FP32_CASES = [
    # tag, A, B, T, instance, pipelined
    ("exact-8", 8, 6, 5, "exact", False),
    ("two-tile-decoupled-16", 16, 3, 4, "exact", True),
    ("runtime-5", 5, 4, 6, "runtime", False),
]


@pytest.mark.parametrize("tag,A,B,T,instance,piped", FP32_CASES, ids=[c[0] for c in FP32_CASES])
def test_qlambda_update_fp32(monkeypatch, tag, A, B, T, instance, piped):
    require_gpu()
    _ql_update(monkeypatch, tag, _cfg_of(A), B, T, instance=instance, piped=piped)


def test_qlambda_update_generic(monkeypatch):
    """The emb-64 / 4-head network: the runtime-shaped kernels' one-network mixer unroll."""
    require_gpu()
    monkeypatch.setenv("T2O_GENERIC", "1")
    _ql_update(monkeypatch, "generic-E64H4", _cfg_of(8, E=64, H=4), 3, 5, instance="generic")


def test_qlambda_update_rmsprop(monkeypatch):
    """(8, 6, 5) with optimizer="rmsprop": the same gradient bars, then the RMSprop
    transition on the learner's own normalised gradient (square_avg in exp_avg_sq,
    exp_avg untouched), at the bars of tests/test_gpu_rmsprop.py."""
    require_gpu()
    kw = dict(optimizer="rmsprop", optim_alpha=0.99, optim_eps=1e-5)
    learner, snap, out, info, _, _ = _ql_update(monkeypatch, "exact-8 rmsprop", _cfg_of(8), 6, 5, instance="exact",
                                                piped=False, **kw)
    graw = out[0]
    ref = rmsprop_ref(snap.params, graw[:-1], snap.v, lr=learner.lr, alpha=0.99, eps=1e-5, weight_decay=0.0,
                      max_norm=learner.clip, grad_div=float(graw[-1]))
    es, ep, bar_p = rmsprop_errors(learner.params, learner.exp_avg_sq, ref, snap.params)
    en = abs(float(info["grad_norm"]) - ref[2]) / ref[2]
    print(f"RMSprop step 1: square_avg {es:.2e} p {ep:.2e} (bar {bar_p:.2e}) grad norm err {en:.2e}")
    assert es <= 1e-6 and ep <= bar_p and en <= 1e-5, (es, ep, bar_p, en)
    assert learner.step_count == 1 and not learner.exp_avg.any()
    assert float((ref[0] - snap.params.cpu().double()).abs().max()) > 1e-4  # the step is there


def test_qlambda_bf16_targets_and_reproducibility():
    """bf16 operands stop at the mixers: the target kernel is fp32, so info["targets"] is
    the fp64 formula on the GPU's own target mix / taken mix at the fp32 bar; and two
    updates from the same state are equal bit for bit."""
    require_gpu()
    A, B, T = 8, 6, 5
    learner, _, _ = make_learner(_cfg_of(A), precision="bf16", q_lambda=True)
    perturb_targets(learner)
    cpu, w = masked_batch(A, B, T, SEED)
    snap = Snapshot(learner)
    out1, info1 = update(learner, to_cuda(cpu), w.cuda())
    r, term, mask = _masks(cpu)
    q1, qk = info1["qtot_tgt"].cpu().double(), info1["qtot_taken"].cpu().double()
    want = build_q_lambda_targets(r, term, mask, q1, qk, learner.gamma, learner.td_lambda)
    err = normwise(info1["targets"], want)
    away = normwise(build_td_lambda_targets(r, term, mask, q1, learner.gamma, learner.td_lambda), want)
    print(f"bf16: targets vs the formula on the GPU's own mixes {err:.2e}; TD(λ) targets {away:.2e} away")
    assert err < 1e-5, err
    assert away >= 1e-2, away
    keep = [t.clone() for t in (*out1, info1["qtot_taken"], info1["qtot_tgt"])]
    snap.restore()
    out2, info2 = update(learner, to_cuda(cpu), w.cuda())
    for a, b in zip(keep, (*out2, info2["qtot_taken"], info2["qtot_tgt"])):
        assert torch.equal(a, b)


def test_qlambda_pipelined_update_is_reproducible():
    """(16, 3, 4), fp32, the pipelined path (two streams): the third unroll and the
    target kernel are ordered after their producers, so two runs from one Snapshot
    give equal raw gradients, priorities, targets and taken mix, bit for bit."""
    require_gpu()
    A, B, T = 16, 3, 4
    learner, _, _ = make_learner(_cfg_of(A), q_lambda=True)
    assert learner._pipelined(B)
    perturb_targets(learner)
    cpu, w = masked_batch(A, B, T, SEED)
    snap = Snapshot(learner)
    runs = []
    for _ in range(3):
        snap.restore()
        out, info = update(learner, to_cuda(cpu), w.cuda())
        runs.append([t.clone() for t in (*out, info["qtot_taken"], info["qtot_tgt"])])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_default_learner_has_no_qlambda_outputs_and_bad_options_raise():
    require_gpu()
    A, B, T = 8, 3, 4
    learner, _, _ = make_learner(_cfg_of(A))
    assert (learner.q_lambda, learner.optimizer, learner.alpha) == (False, "adam", 0.99)
    cpu, w = masked_batch(A, B, T, SEED)
    _, info = update(learner, to_cuda(cpu), w.cuda())
    assert "qtot_taken" not in info and "qtot_tgt" not in info
    for kw in (dict(optimizer="sgd"), dict(optimizer="RMSprop"), dict(q_lambda="yes"), dict(optim_alpha=1.0),
               dict(optim_alpha=-0.1)):
        with pytest.raises(ValueError):
            make_learner(_cfg_of(A), **kw)


# ---- checkpoints ---------------------------------------------------------------------

KW = dict(q_lambda=True, optimizer="rmsprop", optim_eps=1e-5)


def _modules(A, seed):
    from t2omca_amd.modules import TransformerAgent, TransformerMixer
    from t2omca_amd.synthetic import make_args
    torch.manual_seed(seed)
    args = make_args(A)
    return TransformerAgent(None, args).cuda(), TransformerMixer(args).cuda()


def _third_update(learner, batch, w):
    info = learner.train(batch, 0, 0, per_weight=w)
    torch.cuda.synchronize()
    return [t.clone() for t in (learner.grad, learner.params, learner.exp_avg_sq, info["td_errors_abs"],
                                info["targets"], info["qtot_taken"])]


def test_rmsprop_checkpoints(tmp_path):
    require_gpu()
    from t2omca_amd.learner import TDLearner
    A, B, T = 8, 6, 5
    cpu, w = masked_batch(A, B, T, SEED)
    batch, w = to_cuda(cpu), w.cuda()
    l0 = TDLearner(*_modules(A, 0), **KW)
    for _ in range(2):
        l0.train(batch, 0, 0, per_weight=w)
    l0.save_models(str(tmp_path))
    sd = l0.state_dict()
    assert (sd["q_lambda"], sd["optimizer"], float(sd["optim_alpha"])) == (True, "rmsprop", 0.99)

    # a plain torch RMSprop over same-shaped CPU parameters loads opt.th
    params = [torch.nn.Parameter(torch.zeros(p.shape)) for m in (l0.agent, l0.mixer) for p in m.parameters()]
    opt = torch.optim.RMSprop(params)
    opt.load_state_dict(torch.load(tmp_path / "opt.th", map_location="cpu", weights_only=True))
    off = 0
    for p in params:
        st = opt.state[p]
        assert set(st) == {"step", "square_avg"}
        assert torch.equal(st["square_avg"].reshape(-1), l0.exp_avg_sq[off:off + p.numel()].cpu())
        assert int(float(st["step"])) == l0.step_count == 2
        off += p.numel()
    assert off == l0.params.numel()
    g = opt.param_groups[0]
    assert (g["alpha"], g["eps"], g["momentum"], g["centered"]) == (0.99, 1e-5, 0, False)

    # load_models into a fresh learner (the target agent then comes from agent.th and the
    # target mixer is kept, as in PyMARL2: aligned with the uninterrupted learner's here),
    # and load_state_dict into another (the saved state carries the targets)
    l1 = TDLearner(*_modules(A, 5), **KW)
    l1.load_models(str(tmp_path))
    assert l1.step_count == 2 and torch.equal(l1.params, l0.params) and torch.equal(l1.exp_avg_sq, l0.exp_avg_sq)
    assert not l1.exp_avg.any()
    l1.target_params.copy_(l0.target_params)
    l1._pack_targets()
    l2 = TDLearner(*_modules(A, 6), **KW)
    l2.load_state_dict(sd)
    want = _third_update(l0, batch, w)
    for ln in (l1, l2):
        for a, b in zip(want, _third_update(ln, batch, w)):
            assert torch.equal(a, b)
    assert l0.step_count == l1.step_count == l2.step_count == 3


def test_checkpoints_of_the_other_optimiser_are_refused(tmp_path):
    require_gpu()
    from t2omca_amd.learner import TDLearner
    A, B, T = 8, 3, 4
    cpu, w = masked_batch(A, B, T, SEED)
    batch, w = to_cuda(cpu), w.cuda()
    adam, rms = TDLearner(*_modules(A, 0)), TDLearner(*_modules(A, 0), **KW)
    for ln, name in ((adam, "adam"), (rms, "rmsprop")):
        ln.train(batch, 0, 0, per_weight=w)
        os.makedirs(tmp_path / name)
        ln.save_models(str(tmp_path / name))
    for ln, other in ((rms, "adam"), (adam, "rmsprop")):
        before = (ln.step_count, ln.exp_avg.clone(), ln.exp_avg_sq.clone())
        with pytest.raises(ValueError, match=r"(?s)(Adam.*RMSprop|RMSprop.*Adam)") as e:
            ln.load_models(str(tmp_path / other))
        print(e.value)
        assert ln.step_count == before[0] and torch.equal(ln.exp_avg, before[1]) and torch.equal(ln.exp_avg_sq,
                                                                                                 before[2])
    # before the first step an opt.th has no per-parameter state: told apart by its param_groups
    fresh = TDLearner(*_modules(A, 1))
    os.makedirs(tmp_path / "fresh")
    fresh.save_models(str(tmp_path / "fresh"))
    with pytest.raises(ValueError, match="Adam"):
        rms.load_models(str(tmp_path / "fresh"))
    adam.load_models(str(tmp_path / "fresh"))
    assert adam.step_count == 0
    # run states
    with pytest.raises(ValueError, match="optimizer"):
        rms.load_state_dict(dict(rms.state_dict(), optimizer="adam"))
    with pytest.raises(ValueError, match="optimizer"):
        TDLearner(*_modules(A, 2), optimizer="rmsprop").load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="q_lambda"):
        TDLearner(*_modules(A, 2), q_lambda=True).load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="optim_alpha"):
        TDLearner(*_modules(A, 2), optimizer="rmsprop", optim_alpha=0.9).load_state_dict(
            TDLearner(*_modules(A, 2), optimizer="rmsprop").state_dict())
    # a state written before the three keys existed means the defaults
    old = {k: v for k, v in adam.state_dict().items() if k not in ("q_lambda", "optimizer", "optim_alpha")}
    assert len(old) == len(adam.state_dict()) - 3
    again = TDLearner(*_modules(A, 3))
    again.load_state_dict(old)
    assert torch.equal(again.params, adam.params) and again.step_count == adam.step_count
    with pytest.raises(ValueError, match="q_lambda"):
        rms.load_state_dict(old)


# ---- data parallel -------------------------------------------------------------------

DP_B, DP_T, DP_A, DP_UPDATES = 6, 7, 8, 2


def _dp_batch(device):
    from t2omca_amd.synthetic import make_batch
    batch, w = make_batch(DP_B, DP_T, DP_A, seed=11, device=device)
    batch["terminated"][1, 3] = 1  # ragged masks: the shards' Σ mask differ
    batch["filled"][4, 5:] = 0
    return batch, w


def _dp_learner(seed, device, pg=None):
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.modules import TransformerAgent, TransformerMixer
    from t2omca_amd.synthetic import make_args
    torch.manual_seed(seed)
    args = make_args(DP_A, device=str(device))
    return TDLearner(TransformerAgent(None, args).to(device), TransformerMixer(args).to(device), process_group=pg,
                     target_update_interval=2, **KW)


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
        shard = {k: v[lo:hi] for k, v in batch.items()}

        def state(grad):
            return torch.stack([learner.params, learner.target_params, learner.exp_avg_sq,
                                grad]).detach().cpu().clone()

        hist = [state(torch.zeros_like(learner.params))]
        for u in range(DP_UPDATES):
            learner.train(shard, 0, u, per_weight=w[lo:hi])
            torch.cuda.synchronize()
            hist.append(state(learner.grad[:-1] / learner.grad[-1]))  # the all-reduced, Σmask-normalised grad
        out.put((rank, torch.stack(hist).numpy()))
    finally:
        dist.destroy_process_group()


def test_dp_two_ranks_qlambda_rmsprop():
    """Two gloo ranks on one device, q_lambda=True and optimizer="rmsprop", ragged masks,
    two updates: the ranks stay bit-identical, and each update's gradient and post-update
    parameters equal the full-batch update from the replicas' state (<= 1e-6 normwise)."""
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
    r0, r1 = torch.from_numpy(res[0]), torch.from_numpy(res[1])  # [update, (params, target, square_avg, grad), n]
    assert torch.equal(r0, r1)
    dev = torch.device("cuda", 0)
    full = _dp_learner(100, dev)  # rank 0's init
    batch, w = _dp_batch(dev)
    assert torch.equal(full.params.cpu(), r0[0, 0])
    for u in range(DP_UPDATES):
        for buf, k in ((full.params, 0), (full.target_params, 1), (full.exp_avg_sq, 2)):
            buf.copy_(r0[u, k].to(dev))
        full._params_written()
        full._pack_targets()
        full.train(batch, 0, u, per_weight=w)
        torch.cuda.synchronize()
        gerr = normwise(r0[u + 1, 3], (full.grad[:-1] / full.grad[-1]).cpu())
        err = normwise(r0[u + 1, 0], full.params.cpu())
        print(f"update {u} from the replicas' state: grad {gerr:.2e}, params {err:.2e}")
        assert gerr < 1e-6, (u, gerr)
        assert err < 1e-6, (u, err)
