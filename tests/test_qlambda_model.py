"""CPU: tests/qlambda_model.py, the fp64 restatement the Q(λ) and RMSprop GPU tests
compare against, checked against what it must reduce to.

* With qvals equal to exp_qvals the off-policy correction is an exact zero and the
  Q(λ) targets are build_td_lambda_targets's, bit for bit.
* At λ = 0 the recursion has no carry: target_t = m_t (r_t + Q'_t − Qk_t + γ Q'_{t+1} (1 − term_t)).
* rmsprop_ref matches torch.optim.RMSprop (preceded by clip_grad_norm_) in fp64 over
  three steps, with and without weight decay.
* td_forward_qlambda differs from td_forward only in the targets, and its extras
  carry the taken mix.
"""
import pytest
import torch

from oracle.ref_learner import build_td_lambda_targets
from tests.qlambda_model import build_q_lambda_targets, rmsprop_ref


def _case(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    r, q1, qk = (torch.randn(B, n, generator=g, dtype=torch.float64) for n in (T, T + 1, T))
    lens = torch.randint(1, T + 1, (B,), generator=g)
    filled = (torch.arange(T)[None, :] < lens[:, None]).double()
    term = torch.zeros(B, T, dtype=torch.float64)
    ended = torch.rand(B, generator=g) < 0.5
    term[torch.arange(B)[ended], (lens - 1)[ended]] = 1.0
    mask = filled.clone()
    mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
    return r, term, mask, q1, qk


@pytest.mark.parametrize("B,T", [(1, 1), (7, 5), (4, 33)])
def test_reduces_to_td_lambda(B, T):
    r, term, mask, q1, _ = _case(B, T, 3 * B + T)
    ref = build_td_lambda_targets(r, term, mask, q1, 0.99, 0.6)
    assert torch.equal(build_q_lambda_targets(r, term, mask, q1, q1[:, :T].clone(), 0.99, 0.6), ref)
    assert torch.equal(build_q_lambda_targets(r, term, mask, q1, q1, 0.99, 0.6), ref)  # [B, T+1] qvals


def test_lambda_zero_is_one_step():
    r, term, mask, q1, qk = _case(6, 9, 5)
    got = build_q_lambda_targets(r, term, mask, q1, qk, 0.97, 0.0)
    want = mask * (r + (q1[:, :-1] - qk) + 0.97 * q1[:, 1:] * (1 - term))
    assert torch.equal(got, want)
    # and the correction matters: the TD(λ) targets are elsewhere
    assert (got - build_td_lambda_targets(r, term, mask, q1, 0.97, 0.0)).abs().max() > 0.1


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_rmsprop_ref_matches_torch(wd):
    g = torch.Generator().manual_seed(11)
    n, kw = 50, dict(lr=5e-4, alpha=0.99, eps=1e-5, weight_decay=wd)
    p = torch.nn.Parameter(torch.randn(n, generator=g, dtype=torch.float64))
    opt = torch.optim.RMSprop([p], **kw)
    mine, sq = p.detach().clone(), torch.zeros(n, dtype=torch.float64)
    for step in range(3):
        grad = torch.randn(n, generator=g, dtype=torch.float64) * (3.0 if step == 1 else 0.1)  # step 1: clipped
        p.grad = grad.clone()
        norm = float(torch.nn.utils.clip_grad_norm_([p], 10.0))
        opt.step()
        mine, sq, my_norm = rmsprop_ref(mine, grad, sq, max_norm=10.0, **kw)
        assert (norm > 10.0) == (step == 1)
        assert abs(my_norm - norm) <= 1e-12 * norm
        assert torch.allclose(mine, p.detach(), rtol=1e-13, atol=1e-15)
        assert torch.allclose(sq, opt.state[p]["square_avg"], rtol=1e-13, atol=0.0)
    # grad_div divides before the norm; max_norm = 0 switches the clip off
    a = rmsprop_ref(mine, 4.0 * grad, sq, max_norm=0.0, grad_div=4.0, **kw)
    b = rmsprop_ref(mine, grad, sq, max_norm=1e9, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_td_forward_qlambda_against_td_forward():
    """Same qtot, target mix and online Q as td_forward; targets = the formula on the
    extras; they reduce to td_forward's when the taken actions ARE the double-Q ones."""
    from oracle import ref_learner, ref_model
    from tests.qlambda_model import td_forward_qlambda
    from tests.test_gpu_generic import _cfg_of
    from t2omca_amd.synthetic import make_batch
    cfg = _cfg_of(3)
    pa = {k: v.double() for k, v in ref_model.init_params("agent", cfg, 0).items()}
    pm = {k: v.double() for k, v in ref_model.init_params("mixer", cfg, 1).items()}
    batch, w = make_batch(2, 3, 3, seed=3, device="cpu")
    batch = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    l0, p0, e0 = ref_learner.td_forward(pa, pm, pa, pm, batch, cfg, per_weight=w.double())
    l1, p1, e1 = td_forward_qlambda(pa, pm, pa, pm, batch, cfg, per_weight=w.double())
    for k in ("qtot", "qtot_tgt", "mac_out"):
        assert torch.equal(e0[k], e1[k]), k
    T = e1["qtot"].shape[1]
    assert e1["qtot_taken"].shape == (2, T)
    term = batch["terminated"][:, :-1, 0].double()
    mask = batch["filled"][:, :-1, 0].double()
    mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
    want = build_q_lambda_targets(batch["reward"][:, :-1, 0], term, mask, e1["qtot_tgt"], e1["qtot_taken"], 0.99, 0.6)
    assert torch.equal(e1["targets"], want)
    assert not torch.equal(e1["targets"], e0["targets"])
    # taken actions := the masked online argmax: Qk = Q' and the TD(λ) update comes back
    mac = e0["mac_out"].clone()
    mac[batch["avail_actions"] == 0] = -9999999
    greedy = dict(batch, actions=mac.max(dim=3, keepdim=True)[1])
    _, _, e2 = ref_learner.td_forward(pa, pm, pa, pm, greedy, cfg, per_weight=w.double())
    _, _, e3 = td_forward_qlambda(pa, pm, pa, pm, greedy, cfg, per_weight=w.double())
    assert torch.equal(e3["qtot_taken"], e3["qtot_tgt"][:, :-1]) and torch.equal(e3["targets"], e2["targets"])
