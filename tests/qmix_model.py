"""CPU restatement of the QMIX and VDN mixers (t2omca_amd.modules.QMixer / VDNMixer,
csrc/t2o_qmix.hip) in plain torch on a parameter dict, and the TD update with them.

Neither mixer ships with the reference: the definitions are the project's declared
ones (after PyMARL2's modules/mixers/nmix.py and vdn.py).  Test
infrastructure only; evaluated in whatever dtype the inputs have (the tests use fp64).
"""
import torch
import torch.nn.functional as F

from oracle import ref_learner, ref_model

KEYS = ("hyper_w1.0.weight", "hyper_w1.0.bias", "hyper_w1.2.weight", "hyper_w1.2.bias",
        "hyper_b1.0.weight", "hyper_b1.0.bias",
        "hyper_w2.0.weight", "hyper_w2.0.bias", "hyper_w2.2.weight", "hyper_w2.2.bias",
        "hyper_b2.0.weight", "hyper_b2.0.bias", "hyper_b2.2.weight", "hyper_b2.2.bias")


def pos(x, pos_func="abs", beta=1.0):
    """The hypernetwork weights' positivity function (n_transf_mixer.py:95-103)."""
    if pos_func == "abs":
        return x.abs()
    if pos_func == "softplus":
        return F.softplus(x, beta=beta)
    if pos_func == "quadratic":
        return 0.5 * x ** 2
    return x


def shapes(A, S, M=32, H=64):
    return dict(zip(KEYS, ((H, S), (H,), (A * M, H), (A * M,), (M, S), (M,), (H, S), (H,), (M, H), (M,),
                           (M, S), (M,), (1, M), (1,))))


def param_dict(module, dtype=torch.float64):
    return {k: v.detach().cpu().to(dtype).clone() for k, v in module.state_dict().items()}


def qmix_forward(p, q, s, pos_func="abs", beta=1.0):
    """q [b, T, A], s [b, T, S] -> y [b, T]."""
    b, T, A = q.shape
    lin = lambda x, n: x @ p[n + ".weight"].T + p[n + ".bias"]  # noqa: E731
    M = p["hyper_b1.0.bias"].numel()
    w1 = pos(lin(torch.relu(lin(s, "hyper_w1.0")), "hyper_w1.2"), pos_func, beta).view(b, T, A, M)
    b1 = lin(s, "hyper_b1.0")
    w2 = pos(lin(torch.relu(lin(s, "hyper_w2.0")), "hyper_w2.2"), pos_func, beta)
    b2 = lin(torch.relu(lin(s, "hyper_b2.0")), "hyper_b2.2")[..., 0]
    hidden = F.elu(torch.einsum("bta,btam->btm", q, w1) + b1)
    return (hidden * w2).sum(-1) + b2


def vdn_forward(q):
    return q.sum(2)


def mix(kind, p, q, s, pos_func="abs", beta=1.0):
    return vdn_forward(q) if kind == "vdn" else qmix_forward(p, q, s, pos_func, beta)


def td_forward_mixer(kind, pos_func="abs", beta=1.0, q_lambda=False, noise=None):
    """A function with ref_learner.td_forward's signature and extras (relu= included)
    whose mixer is `kind` ("qmix" / "vdn"): substitute it for ref_learner.td_forward
    with monkeypatch.setattr.  The mixers read the state only, so detach_mixer_hidden
    has no effect.  q_lambda: Peng's Q(λ) targets (tests/qlambda_model).  noise =
    (eps_on, eps_tg), each (eps_w [T+1, NA, E], eps_b [T+1, NA]): a noisy agent, its
    head (tests/noisy_model) applied to ref_model.agent_unroll's hidden states."""

    def agent_q(p, obs, h0, cfg, eps):
        if noise is None:
            return ref_model.agent_unroll(p, obs, h0, cfg=cfg)[0]
        from tests import noisy_model
        _, hs = ref_model.agent_unroll(noisy_model._plain(p), obs, h0, cfg=cfg)
        return noisy_model._head(p, hs, tuple(e.to(obs.dtype) for e in eps))

    def td_forward(p_agent, p_mixer, p_agent_tgt, p_mixer_tgt, batch, cfg, *, gamma=0.99, td_lambda=0.6,
                   per_weight=None, detach_mixer_hidden=False, relu=None):
        if relu is not None:
            prev, ref_model._ffn_relu = ref_model._ffn_relu, relu
            try:
                return td_forward(p_agent, p_mixer, p_agent_tgt, p_mixer_tgt, batch, cfg, gamma=gamma,
                                  td_lambda=td_lambda, per_weight=per_weight)
            finally:
                ref_model._ffn_relu = prev
        obs, state = batch["obs"], batch["state"]
        actions, avail = batch["actions"], batch["avail_actions"]
        B, T1, A, _ = obs.shape
        state = state.reshape(B, T1, -1)
        rewards = batch["reward"][:, :-1, 0]
        terminated = batch["terminated"][:, :-1, 0].float()
        mask = batch["filled"][:, :-1, 0].float()
        mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
        h0 = torch.zeros(B, A, cfg["emb"], dtype=obs.dtype)
        mac_out = agent_q(p_agent, obs, h0, cfg, noise and noise[0])
        chosen = torch.gather(mac_out[:, :-1], 3, actions[:, :-1]).squeeze(3)
        extra = {}
        with torch.no_grad():
            tgt_out = agent_q(p_agent_tgt, obs, h0, cfg, noise and noise[1])
            mac_det = mac_out.clone().detach()
            mac_det[avail == 0] = -9999999
            cur_max = mac_det.max(dim=3, keepdim=True)[1]
            target_max_q = torch.gather(tgt_out, 3, cur_max).squeeze(3)
            qtot_tgt = mix(kind, p_mixer_tgt, target_max_q, state, pos_func, beta)
            if q_lambda:
                from tests.qlambda_model import build_q_lambda_targets
                taken = torch.gather(tgt_out[:, :-1], 3, actions[:, :-1]).squeeze(3)
                qtot_taken = mix(kind, p_mixer_tgt, taken, state[:, :-1], pos_func, beta)
                targets = build_q_lambda_targets(rewards, terminated, mask, qtot_tgt, qtot_taken, gamma, td_lambda)
                extra["qtot_taken"] = qtot_taken
            else:
                targets = ref_learner.build_td_lambda_targets(rewards, terminated, mask, qtot_tgt, gamma, td_lambda)
        qtot = mix(kind, p_mixer, chosen, state[:, :-1], pos_func, beta)
        td_error = qtot - targets.detach()
        masked = 0.5 * td_error.pow(2) * mask
        if per_weight is not None:
            masked = masked.sum(1) * per_weight
        loss = masked.sum() / mask.sum()
        prio = ((td_error.abs() * mask).sum(1) / torch.sqrt(mask.sum(1))).detach()
        return loss, prio, dict(qtot=qtot.detach(), qtot_tgt=qtot_tgt, targets=targets, mac_out=mac_out.detach(),
                                **extra)
    return td_forward
