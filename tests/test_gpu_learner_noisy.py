"""GPU: whole TD updates with a NoisyNet agent (modules.TransformerAgent with
action_selector "noisy-new") against tests/noisy_model.td_forward_noisy
through the tie-aware fp64 oracle (tests.gpu_util.oracle_td_tie_aware looks
ref_learner.td_forward up when called, so the noisy version, bound to the update's ε,
is substituted with monkeypatch.setattr).

Inputs are those of tests/test_gpu_learner_masks.py (its helpers imported): modules
torch.manual_seed(grad_blocks.module_seed(A)) (0; 4 at 16 AGVs), batch seed 3 drawn on the CPU, masked_avail seed 103, target
parameters (sigmas included) perturbed by 0.01·N(0, 1); the sigmas are 0.3·N(0, 1)
from a generator seeded 7, the learner's noise_seed is 11.  The oracle takes the ε the
learner drew (learner.last_noise), which is first held to one fp32 ulp of the numpy
restatement at (noise_seed, kind, step_count).  Bars TOL["fp32"]: 1e-5 on qtot,
targets and priorities, 3e-5 on the gradient (sigma slots included).

Preconditions, from the oracle alone, printed and asserted in every fp32 case beside
check_update's argmax ones (moved >= 0.25, gap >= 1e-4 — here of the NOISY online Q):
the targets computed with noise differ from those with ε = 0 by >= 1e-2 normwise, and
the masked argmax under the noisy online Q differs from the mean-head one at >= 5 % of
(b, t, a).  Computed on the CPU first, at noise_seed 11:

  case                   moved   gap        targets vs ε=0   argmax differs
  (8, 6, 5) exact        0.490   5.13e-04   1.97e+00         0.438
  (16, 3, 4) pipelined   0.412   1.21e-03   1.42e+00         0.517
  (5, 4, 6) runtime      0.571   9.30e-03   7.79e+00         0.371
  (8, 3, 5) E64/H4       0.438   3.16e-03   9.75e-01         0.486
  (8, 6, 5) Q(λ)         0.490   5.13e-04   1.79e+00         0.438

The sigma gradients' share of the gradient norm is printed and must be > 0.  bf16
operands stop at the fused kernels, the head and the target kernel are fp32:
info["targets"] is the Q(λ) formula on the GPU's own mixes at 1e-5.  Updates are
bit-reproducible from one Snapshot (sequential and pipelined); a second update draws
another ε, the same step_count the same; checkpoints resume bit for bit and the other
head's files and states are refused; two gloo ranks on one device stay bit-identical
and equal the full-batch update; a plain agent's update launches none of the head's
kernels.

Measured on an MI355X (normwise qtot / targets / priorities / gradient; sigma gradients'
share of the gradient norm; the head's mean / sigma slots alone; no ReLU tie overridden):
  exact-8                  2.1e-7  1.1e-6  1.6e-7  2.4e-7   0.117   1.8e-7 / 1.1e-7
  two-tile-decoupled-16    2.2e-7  4.3e-7  1.7e-7  1.6e-7   0.148   2.6e-7 / 2.1e-7
  runtime-5                1.3e-7  1.6e-7  2.0e-7  7.9e-7   0.138   2.1e-7 / 4.8e-7
  generic-E64H4            1.9e-7  2.7e-7  1.2e-7  3.9e-7   0.107   2.3e-7 / 2.0e-7
  exact-8 Q(λ) rmsprop     2.1e-7  3.1e-7  1.8e-7  1.0e-7   0.120   2.7e-7 / 7.8e-8
contract="pair" equals "side" bit for bit; bf16 targets 6.4e-8 from the formula.
"""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import noisy_model as nm
from tests.gpu_util import normwise, require_gpu, split_flat
from tests.grad_blocks import module_seed
from tests.test_gpu_generic import _args, _cfg_of
from tests.test_gpu_learner_masks import (SEED, TOL, Snapshot, check_update, masked_batch, perturb_targets, to_cuda,
                                          update)

pytestmark = pytest.mark.gpu

NOISE_SEED, SIGMA_SEED = 11, 7


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    """The tuned instances and the default mixer choice unless a case says otherwise."""
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)


def noisy_modules(cfg, device="cuda", seed=None):
    """The noisy agent and the mixer of a config (module seed grad_blocks.module_seed(A)
    unless given), sigmas 0.3·N(0, 1)."""
    from t2omca_amd.modules import TransformerAgent, TransformerMixer
    torch.manual_seed(module_seed(cfg["n_agents"]) if seed is None else seed)
    args = _args(cfg, device=device)
    args.action_selector = "noisy-new"
    agent, mixer = TransformerAgent(None, args), TransformerMixer(args)
    g = torch.Generator().manual_seed(SIGMA_SEED)
    with torch.no_grad():
        agent.q_basic.s_w.copy_(0.3 * torch.randn(agent.q_basic.s_w.shape, generator=g))
        agent.q_basic.s_b.copy_(0.3 * torch.randn(agent.q_basic.s_b.shape, generator=g))
    return agent.to(device), mixer.to(device)


def make_noisy_learner(cfg, **kw):
    from t2omca_amd.learner import TDLearner
    agent, mixer = noisy_modules(cfg)
    pa = {k: v.detach().cpu().double() for k, v in agent.state_dict().items()}
    pm = {k: v.detach().cpu().double() for k, v in mixer.state_dict().items()}
    learner = TDLearner(agent, mixer, noise_seed=NOISE_SEED, **kw)
    assert learner.noisy and learner.na == learner.na_net + cfg["n_actions"] * (cfg["emb"] + 1)
    return learner, pa, pm


def restated_noise(cfg, T1, counter, seed=NOISE_SEED):
    """((eps_w, eps_b) online, target) of an update at step_count = counter: fp64 tensors
    of the fp32 values the kernel writes."""
    return tuple(tuple(torch.from_numpy(x).double() for x in
                       nm.noise_normal(cfg["emb"], cfg["n_actions"], T1, seed, kind, counter))
                 for kind in ("learner_online", "learner_target"))


def _ulp_ok(dev, ref):
    dev, ref = dev.cpu().numpy(), ref.numpy().astype(np.float32)
    return bool((np.abs(dev.astype(np.float64) - ref) <= np.spacing(np.abs(ref))).all())


def _masks(cpu):
    term = cpu["terminated"][:, :-1, 0].double()
    mask = cpu["filled"][:, :-1, 0].double()
    mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
    return cpu["reward"][:, :-1, 0].double(), term, mask


def noise_preconditions(tag, pa, pm, pat, pmt, cfg, cpu, w, eps_on, eps_tg, q_lambda=False):
    """From the oracle alone: how far the noise moves the targets and the greedy actions."""
    c64 = {k: (v.double() if v.is_floating_point() else v) for k, v in cpu.items()}
    run = functools.partial(nm.td_forward_noisy, pa, pm, pat, pmt, c64, cfg, per_weight=w.double(), q_lambda=q_lambda)
    with torch.no_grad():
        _, _, ex = run(eps_on=eps_on, eps_tg=eps_tg)
        _, _, ex0 = run(eps_on=None, eps_tg=None)
    tdiff = normwise(ex["targets"], ex0["targets"])
    on = cpu["avail_actions"] != 0
    am = ex["mac_out"].masked_fill(~on, -9999999.0).argmax(-1)
    am0 = ex0["mac_out"].masked_fill(~on, -9999999.0).argmax(-1)
    share = float((am != am0).double().mean())
    print(f"{tag}: targets with noise vs ε = 0 {tdiff:.2e} normwise; "
          f"masked argmax differs at {share:.3f} of (b, t, a)")
    assert tdiff >= 1e-2, tdiff
    assert share >= 0.05, share
    return tdiff, share


def _noisy_update(monkeypatch, tag, cfg, B, T, *, instance=None, piped=None, q_lambda=False, **kw):
    """One update from perturbed targets against the noisy oracle at the fp32 bars."""
    from oracle import ref_learner
    learner, pa, pm = make_noisy_learner(cfg, q_lambda=q_lambda, **kw)
    if instance is not None:
        assert learner.sa.instance == instance and learner.sm.instance == instance
    if piped is not None:
        assert bool(learner._pipelined(B)) == piped
    perturb_targets(learner)
    pat, pmt = split_flat(learner.target_params, pa, pm)
    cpu, w = masked_batch(cfg["n_agents"], B, T, SEED)
    snap = Snapshot(learner)
    out, info = update(learner, to_cuda(cpu), w.cuda())
    # the ε the learner drew: the restatement's at (noise_seed, kind, step_count = 0)
    want = restated_noise(cfg, T + 1, 0)
    eps = []
    for dev, ref in zip(learner.last_noise, want):
        assert dev[0].shape == ref[0].shape and _ulp_ok(dev[0], ref[0]) and _ulp_ok(dev[1], ref[1])
        eps.append((dev[0].cpu().double(), dev[1].cpu().double()))
    monkeypatch.setattr(ref_learner, "td_forward",
                        functools.partial(nm.td_forward_noisy, eps_on=eps[0], eps_tg=eps[1], q_lambda=q_lambda))
    errs, g, ex = check_update(tag, learner, pa, pm, cfg, cpu, w, out, pa_tgt=pat, pm_tgt=pmt)
    noise_preconditions(tag, pa, pm, pat, pmt, cfg, cpu, w, eps[0], eps[1], q_lambda=q_lambda)
    ns = learner.n_head
    sig = g[learner.na_net:learner.na]
    share = float(sig.norm() / g.norm())
    err_sig = normwise(sig, ex["ref_grad"][learner.na_net:learner.na])
    err_mu = normwise(g[learner.na_net - ns:learner.na_net], ex["ref_grad"][learner.na_net - ns:learner.na_net])
    print(f"{tag}: sigma gradients carry {share:.3f} of the gradient norm; head slots alone: means {err_mu:.2e} "
          f"sigmas {err_sig:.2e}")
    assert share > 0
    assert err_sig < TOL["fp32"][1] and err_mu < TOL["fp32"][1], (err_mu, err_sig)
    return learner, snap, out, info, ex, (cpu, w)


FP32_CASES = [
    # tag, A, B, T, instance, pipelined
    ("exact-8", 8, 6, 5, "exact", False),
    ("two-tile-decoupled-16", 16, 3, 4, "exact", True),
    ("runtime-5", 5, 4, 6, "runtime", False),
]


@pytest.mark.parametrize("tag,A,B,T,instance,piped", FP32_CASES, ids=[c[0] for c in FP32_CASES])
def test_noisy_update_fp32(monkeypatch, tag, A, B, T, instance, piped):
    require_gpu()
    _noisy_update(monkeypatch, tag, _cfg_of(A), B, T, instance=instance, piped=piped)


def test_noisy_update_generic(monkeypatch):
    """The emb-64 / 4-head network: the runtime-shaped agent kernels with gh alone, the
    head kernels' 16-lanes-per-row instances."""
    require_gpu()
    monkeypatch.setenv("T2O_GENERIC", "1")
    _noisy_update(monkeypatch, "generic-E64H4", _cfg_of(8, E=64, H=4), 3, 5, instance="generic")


def test_noisy_update_qlambda_rmsprop(monkeypatch):
    """q_lambda=True and optimizer="rmsprop" on the noisy agent: the taken mix reads the
    noisy target Q; the RMSprop transition covers the sigma block."""
    require_gpu()
    from tests.qlambda_model import rmsprop_errors, rmsprop_ref
    learner, snap, out, info, ex, _ = _noisy_update(monkeypatch, "exact-8 Q(λ) rmsprop", _cfg_of(8), 6, 5,
                                                    instance="exact", piped=False, q_lambda=True, optimizer="rmsprop",
                                                    optim_eps=1e-5)
    ek = normwise(info["qtot_taken"], ex["qtot_taken"])
    print(f"qtot_taken {ek:.2e}")
    assert ek < TOL["fp32"][0], ek
    graw = out[0]
    ref = rmsprop_ref(snap.params, graw[:-1], snap.v, lr=learner.lr, alpha=0.99, eps=1e-5, weight_decay=0.0,
                      max_norm=learner.clip, grad_div=float(graw[-1]))
    es, ep, bar_p = rmsprop_errors(learner.params, learner.exp_avg_sq, ref, snap.params)
    print(f"RMSprop step 1: square_avg {es:.2e} p {ep:.2e} (bar {bar_p:.2e})")
    assert es <= 1e-6 and ep <= bar_p, (es, ep, bar_p)
    moved = (learner.params - snap.params)[learner.na_net:learner.na].abs().max()
    assert float(moved) > 1e-4  # the sigmas are trained


def test_pair_contract_equals_side(monkeypatch):
    """contract="pair" (both tapes in one launch after the agent BPTT): the head's launches
    are the same, the gradient equals contract="side"'s to summation order."""
    require_gpu()
    A, B, T = 8, 6, 5
    outs = []
    for contract in ("side", "pair"):
        learner, _, _ = make_noisy_learner(_cfg_of(A), contract=contract)
        perturb_targets(learner)
        cpu, w = masked_batch(A, B, T, SEED)
        outs.append(update(learner, to_cuda(cpu), w.cuda())[0])
    e = [normwise(a, b) for a, b in zip(outs[1], outs[0])]
    print("pair vs side (grad, qtot, targets, prio):", " ".join(f"{x:.2e}" for x in e))
    assert max(e) < 1e-6, e
    ln = learner
    assert torch.equal(outs[0][0][ln.na_net - ln.n_head:ln.na], outs[1][0][ln.na_net - ln.n_head:ln.na])


def test_noisy_bf16_targets():
    """bf16 operands stop at the fused kernels: the head, the mixes' inputs and the target
    kernel are fp32, so info["targets"] is the Q(λ) formula on the GPU's own target mix /
    taken mix at the fp32 bar."""
    require_gpu()
    from oracle.ref_learner import build_td_lambda_targets
    from tests.qlambda_model import build_q_lambda_targets
    A, B, T = 8, 6, 5
    learner, _, _ = make_noisy_learner(_cfg_of(A), precision="bf16", q_lambda=True)
    perturb_targets(learner)
    cpu, w = masked_batch(A, B, T, SEED)
    _, info = update(learner, to_cuda(cpu), w.cuda())
    r, term, mask = _masks(cpu)
    q1, qk = info["qtot_tgt"].cpu().double(), info["qtot_taken"].cpu().double()
    want = build_q_lambda_targets(r, term, mask, q1, qk, learner.gamma, learner.td_lambda)
    err = normwise(info["targets"], want)
    away = normwise(build_td_lambda_targets(r, term, mask, q1, learner.gamma, learner.td_lambda), want)
    print(f"bf16: targets vs the formula on the GPU's own mixes {err:.2e}; TD(λ) targets {away:.2e} away")
    assert err < 1e-5, err
    assert away >= 1e-2, away
    assert torch.isfinite(learner.grad).all() and learner.grad[learner.na_net:learner.na].abs().max() > 0


@pytest.mark.parametrize("A,B,T,piped", [(8, 6, 5, False), (16, 3, 4, True)], ids=["sequential", "pipelined"])
def test_noisy_update_is_reproducible_and_counters_move_the_noise(A, B, T, piped):
    """Three updates from one Snapshot (it restores step_count, so they draw the same ε)
    are equal bit for bit; the next update (step_count 1) draws another ε."""
    require_gpu()
    learner, _, _ = make_noisy_learner(_cfg_of(A))
    assert bool(learner._pipelined(B)) == piped
    perturb_targets(learner)
    cpu, w = masked_batch(A, B, T, SEED)
    batch, w = to_cuda(cpu), w.cuda()
    snap = Snapshot(learner)
    runs = []
    for _ in range(3):
        snap.restore()
        out, _ = update(learner, batch, w)
        runs.append([t.clone() for t in (*out, learner.params, *learner.last_noise[0], *learner.last_noise[1])])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    assert learner.step_count == 1
    out2, _ = update(learner, batch, w)
    second = [t.clone() for t in (*learner.last_noise[0], *learner.last_noise[1])]
    for a, b in zip(runs[0][-4:], second):
        assert not torch.equal(a, b)
    want = restated_noise(_cfg_of(A), T + 1, 1)
    assert _ulp_ok(second[0], want[0][0]) and _ulp_ok(second[2], want[1][0])
    assert not torch.equal(second[0], second[2])  # online and target draw independently
    # another noise_seed: another update
    other, _, _ = make_noisy_learner(_cfg_of(A))
    other.noise_seed = NOISE_SEED + 1
    perturb_targets(other)
    out3, _ = update(other, batch, w)
    assert not torch.equal(out3[0], runs[0][0]) and normwise(out3[2], runs[0][2]) > 1e-3


def test_plain_agent_launches_nothing_of_the_head(monkeypatch):
    """The default path is unchanged: a plain agent's update calls none of the head's ops
    and records none of their timer tags; a noisy agent's records two head forwards, one
    backward and one weight-gradient sum (sequential), per step range when pipelined."""
    require_gpu()
    from t2omca_amd import ops
    from tests.test_gpu_learner_masks import make_learner
    A, B, T = 8, 6, 5
    cpu, w = masked_batch(A, B, T, SEED)
    plain, _, _ = make_learner(_cfg_of(A))
    assert not plain.noisy and plain.na == plain.na_net == plain.sa.n_params
    tags = []
    plain.timer = tags.append
    with monkeypatch.context() as m:
        def refuse(*a, **k):
            raise AssertionError("a plain agent's update reached the noisy head")
        for name in ("noise_normal", "noisy_head_fwd", "noisy_head_bwd", "noisy_head_wgrad"):
            m.setattr(ops, name, refuse)
        update(plain, to_cuda(cpu), w.cuda())
    assert tags and not [t for t in tags if "noisy" in t]
    noisy, _, _ = make_noisy_learner(_cfg_of(A))
    tags = []
    noisy.timer = tags.append
    update(noisy, to_cuda(cpu), w.cuda())
    count = {k: tags.count("begin:" + k) for k in ("noisy_fwd", "noisy_bwd", "noisy_wgrad")}
    assert count == {"noisy_fwd": 2, "noisy_bwd": 1, "noisy_wgrad": 1}, count
    piped, _, _ = make_noisy_learner(_cfg_of(16))
    assert piped._pipelined(3)
    tags = []
    piped.timer = tags.append
    cpu16, w16 = masked_batch(16, 3, 4, SEED)
    update(piped, to_cuda(cpu16), w16.cuda())
    count = {k: tags.count("begin:" + k) for k in ("noisy_fwd", "noisy_bwd", "noisy_wgrad")}
    assert count == {"noisy_fwd": 2 * len(piped._ranges(5)), "noisy_bwd": len(piped._ranges(4)), "noisy_wgrad": 1}


# ---- checkpoints ---------------------------------------------------------------------

def _learner(A, seed, noisy=True, **kw):
    from t2omca_amd.learner import TDLearner
    if noisy:
        return TDLearner(*noisy_modules(_cfg_of(A), seed=seed), noise_seed=NOISE_SEED, **kw)
    from t2omca_amd.modules import TransformerAgent, TransformerMixer
    torch.manual_seed(seed)
    args = _args(_cfg_of(A))
    return TDLearner(TransformerAgent(None, args).cuda(), TransformerMixer(args).cuda(), **kw)


def _third_update(learner, batch, w):
    info = learner.train(batch, 0, 0, per_weight=w)
    torch.cuda.synchronize()
    return [t.clone() for t in (learner.grad, learner.params, learner.exp_avg, learner.exp_avg_sq,
                                info["td_errors_abs"], info["targets"], *learner.last_noise[0])]


def test_noisy_checkpoints(tmp_path):
    require_gpu()
    A, B, T = 8, 6, 5
    cpu, w = masked_batch(A, B, T, SEED)
    batch, w = to_cuda(cpu), w.cuda()
    l0 = _learner(A, 0)
    for _ in range(2):
        l0.train(batch, 0, 0, per_weight=w)
    l0.save_models(str(tmp_path))
    sd = l0.state_dict()
    assert (sd["noisy"], sd["noise_seed"], sd["na"]) == (True, NOISE_SEED, l0.na_net + 5 * 33)
    agent_th = torch.load(tmp_path / "agent.th", map_location="cpu", weights_only=True)
    assert list(agent_th)[-4:] == ["q_basic.u_w", "q_basic.u_b", "q_basic.s_w", "q_basic.s_b"]
    assert torch.equal(agent_th["q_basic.s_w"].reshape(-1), l0.params[l0.na_net:l0.na_net + 160].cpu())

    # a plain torch Adam over same-shaped CPU parameters, in the modules' order, loads opt.th
    params = [torch.nn.Parameter(torch.zeros(p.shape)) for m in (l0.agent, l0.mixer) for p in m.parameters()]
    opt = torch.optim.Adam(params)
    opt.load_state_dict(torch.load(tmp_path / "opt.th", map_location="cpu", weights_only=True))
    off = 0
    for p in params:
        st = opt.state[p]
        assert torch.equal(st["exp_avg"].reshape(-1), l0.exp_avg[off:off + p.numel()].cpu())
        assert torch.equal(st["exp_avg_sq"].reshape(-1), l0.exp_avg_sq[off:off + p.numel()].cpu())
        assert int(float(st["step"])) == l0.step_count == 2
        off += p.numel()
    assert off == l0.params.numel()

    l1 = _learner(A, 5)
    l1.load_models(str(tmp_path))
    assert l1.step_count == 2 and torch.equal(l1.params, l0.params) and torch.equal(l1.exp_avg_sq, l0.exp_avg_sq)
    # (the target agent, sigmas included, came from agent.th; the target mixer is kept as
    # in PyMARL2: aligned with the uninterrupted learner's here)
    assert torch.equal(l1.target_params[:l1.na], l1.params[:l1.na])
    l1.target_params.copy_(l0.target_params)
    l1._pack_targets()
    l2 = _learner(A, 6)
    l2.load_state_dict(sd)
    want = _third_update(l0, batch, w)
    for ln in (l1, l2):
        for a, b in zip(want, _third_update(ln, batch, w)):
            assert torch.equal(a, b)
    assert l0.step_count == l1.step_count == l2.step_count == 3


def test_the_other_heads_checkpoints_are_refused(tmp_path):
    require_gpu()
    A, B, T = 8, 3, 4
    cpu, w = masked_batch(A, B, T, SEED)
    batch, w = to_cuda(cpu), w.cuda()
    noisy, plain = _learner(A, 0), _learner(A, 0, noisy=False)
    for ln, name in ((noisy, "noisy"), (plain, "plain")):
        ln.train(batch, 0, 0, per_weight=w)
        os.makedirs(tmp_path / name)
        ln.save_models(str(tmp_path / name))
    for ln, other in ((noisy, "plain"), (plain, "noisy")):
        before = (ln.step_count, ln.params.clone(), ln.target_params.clone(), ln.exp_avg.clone())
        with pytest.raises(ValueError, match="noisy") as e:
            ln.load_models(str(tmp_path / other))
        print(e.value)
        assert ln.step_count == before[0] and torch.equal(ln.params, before[1])
        assert torch.equal(ln.target_params, before[2]) and torch.equal(ln.exp_avg, before[3])
    # an opt.th of the other head beside the right agent.th: its per-parameter shapes differ
    os.makedirs(tmp_path / "mixed")
    for name in ("agent.th", "mixer.th"):
        torch.save(torch.load(tmp_path / "noisy" / name, weights_only=True), tmp_path / "mixed" / name)
    torch.save(torch.load(tmp_path / "plain" / "opt.th", weights_only=True), tmp_path / "mixed" / "opt.th")
    before = (noisy.params.clone(), noisy.exp_avg.clone())
    with pytest.raises(ValueError, match="opt.th") as e:
        noisy.load_models(str(tmp_path / "mixed"))
    print(e.value)
    assert torch.equal(noisy.params, before[0]) and torch.equal(noisy.exp_avg, before[1])
    # run states
    with pytest.raises(ValueError, match="noisy"):
        plain.load_state_dict(noisy.state_dict())
    with pytest.raises(ValueError, match="noisy"):
        noisy.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="noise_seed"):
        noisy.load_state_dict(dict(noisy.state_dict(), noise_seed=NOISE_SEED + 1))
    # a state written before the two keys existed means a plain agent
    old = {k: v for k, v in plain.state_dict().items() if k not in ("noisy", "noise_seed")}
    again = _learner(A, 3, noisy=False)
    again.load_state_dict(old)
    assert torch.equal(again.params, plain.params)
    with pytest.raises(ValueError, match="noisy"):
        noisy.load_state_dict(old)


# ---- data parallel -------------------------------------------------------------------

DP_B, DP_T, DP_A, DP_UPDATES = 6, 7, 8, 2
# the learner options of the Q(λ) test's data-parallel case.  (The parameter comparison
# needs a step that does not amplify the gradients' summation-order differences.  Adam's
# first step is lr·g / (|g| + eps) on the clipped gradient, slope eps / (|g| + eps)²: at
# its default eps = 1e-8 the parameters came out 3.5e-6 apart at update 0 with the
# gradients 2e-7 apart.  The same figure comes out of one process that steps once on
# the full-batch gradient and once on the sum of the two shards' gradients; its largest
# difference sits at one transformer weight of the agent, not in the head, whose gradient
# is 4.4e-5 and differs by 6.3e-7 where max|g| is 8.3e3, so after the clip to norm 10 it
# is 5e-8 or less, beside eps.  With eps = 1e-5 that comparison gives 2.2e-7.)
DP_KW = dict(q_lambda=True, optimizer="rmsprop", optim_eps=1e-5)


def _dp_batch(device):
    from t2omca_amd.synthetic import make_batch
    batch, w = make_batch(DP_B, DP_T, DP_A, seed=11, device=device)
    batch["terminated"][1, 3] = 1  # ragged masks: the shards' Σ mask differ
    batch["filled"][4, 5:] = 0
    return batch, w


def _dp_learner(seed, device, pg=None):
    from t2omca_amd.learner import TDLearner
    agent, mixer = noisy_modules(_cfg_of(DP_A), device=str(device), seed=seed)
    return TDLearner(agent, mixer, process_group=pg, target_update_interval=2, noise_seed=NOISE_SEED, **DP_KW)


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
            return torch.stack([learner.params, learner.target_params, learner.exp_avg, learner.exp_avg_sq,
                                grad]).detach().cpu().clone()

        hist = [state(torch.zeros_like(learner.params))]
        for u in range(DP_UPDATES):
            learner.train(shard, 0, u, per_weight=w[lo:hi])
            torch.cuda.synchronize()
            hist.append(state(learner.grad[:-1] / learner.grad[-1]))  # the all-reduced, Σmask-normalised grad
        out.put((rank, torch.stack(hist).numpy()))
    finally:
        dist.destroy_process_group()


def test_dp_two_ranks_noisy():
    """Two gloo ranks on one device, as in tests/test_gpu_learner_qlambda.py (q_lambda=True,
    optimizer="rmsprop", optim_eps=1e-5), ragged masks, two updates: both ranks draw the same
    network (noise_seed is not mixed with the rank), stay bit-identical, and each update's
    gradient and post-update parameters equal the full-batch update from the replicas'
    state (<= 1e-6 normwise), sigma block included."""
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
    r0, r1 = torch.from_numpy(res[0]), torch.from_numpy(res[1])  # [update, (params, target, m, v, grad), n]
    assert torch.equal(r0, r1)
    dev = torch.device("cuda", 0)
    full = _dp_learner(100, dev)  # rank 0's init
    batch, w = _dp_batch(dev)
    assert torch.equal(full.params.cpu(), r0[0, 0])
    for u in range(DP_UPDATES):
        for buf, k in ((full.params, 0), (full.target_params, 1), (full.exp_avg, 2), (full.exp_avg_sq, 3)):
            buf.copy_(r0[u, k].to(dev))
        full._params_written()
        full._pack_targets()
        full.step_count = u
        full.train(batch, 0, u, per_weight=w)
        torch.cuda.synchronize()
        g_full = (full.grad[:-1] / full.grad[-1]).cpu()
        gerr = normwise(r0[u + 1, 4], g_full)
        serr = normwise(r0[u + 1, 4][full.na_net:full.na], g_full[full.na_net:full.na])
        err = normwise(r0[u + 1, 0], full.params.cpu())
        print(f"update {u} from the replicas' state: grad {gerr:.2e} (sigma block {serr:.2e}), params {err:.2e}")
        assert gerr < 1e-6 and serr < 1e-6, (u, gerr, serr)
        assert err < 1e-6, (u, err)
