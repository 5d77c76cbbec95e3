"""CPU restatement of the QPLEX duelling mixer (t2omca_amd.modules.QPlexMixer,
csrc/t2o_qplex.hip) in plain torch on a parameter dict, and the TD update with it.

QPLEX does not ship with the reference: the definition is the project's declared one
(after PyMARL2's modules/mixers/dmaq_general.py, dmaq_si_weight.py and
learners/dmaq_qatten_learner.py at qplex.yaml's defaults).  Test infrastructure only;
evaluated in whatever dtype the inputs have (the tests use fp64).
"""
import torch
import torch.nn.functional as F

from oracle import ref_learner, ref_model

EPS = 1e-10


def _net(name):
    return [f"{name}.0.weight", f"{name}.0.bias", f"{name}.2.weight", f"{name}.2.bias"]


def keys(K=4):
    """The state_dict keys in registration (= flat parameter) order: 8 + 12·K."""
    out = _net("hyper_w_final") + _net("V")
    for ext in ("key_extractors", "agents_extractors", "action_extractors"):
        for k in range(K):
            out += _net(f"si_weight.{ext}.{k}")
    return out


def shapes(A, S, NA, H=64, HA=64, K=4):
    def net(n_in, hid, n_out):
        return [(hid, n_in), (hid,), (n_out, hid), (n_out,)]
    sh = net(S, H, A) + net(S, H, A)
    for n_in, n_out in ((S, 1), (S, A), (S + A * NA, A)):
        for _ in range(K):
            sh += net(n_in, HA, n_out)
    return dict(zip(keys(K), sh))


def n_kernels(p):
    return sum(1 for k in p if k.startswith("si_weight.key_extractors.") and k.endswith(".0.weight"))


def param_dict(module, dtype=torch.float64):
    return {k: v.detach().cpu().to(dtype).clone() for k, v in module.state_dict().items()}


def _mlp(p, name, x):
    h = torch.relu(x @ p[name + ".0.weight"].T + p[name + ".0.bias"])
    return h @ p[name + ".2.weight"].T + p[name + ".2.bias"]


def weights(p, s, u, NA):
    """w [b, T, A], v [b, T, A], λ [b, T, A] of states s [b, T, S] and joint actions u [b, T, A] (indices)."""
    w = _mlp(p, "hyper_w_final", s).abs() + EPS
    v = _mlp(p, "V", s)
    d = torch.cat([s, F.one_hot(u.long(), NA).to(s.dtype).flatten(2)], dim=2)
    lam = 0
    for k in range(n_kernels(p)):
        kap = _mlp(p, f"si_weight.key_extractors.{k}", s).abs() + EPS  # [b, T, 1]
        al = torch.sigmoid(_mlp(p, f"si_weight.agents_extractors.{k}", s))
        be = torch.sigmoid(_mlp(p, f"si_weight.action_extractors.{k}", d))
        lam = lam + kap * al * be
    return w, v, lam


def qplex_parts(p, q, m, u, s, NA):
    """(y_v, y_adv), each [b, T]: q, m [b, T, A], u [b, T, A] indices, s [b, T, S]."""
    w, v, lam = weights(p, s, u, NA)
    y_v = (w * q + v).sum(2)
    y_adv = ((w * (q - m)).detach() * (lam - 1.0)).sum(2)
    return y_v, y_adv


def qplex_forward(p, q, m, u, s, NA, parts=3):
    y_v, y_adv = qplex_parts(p, q, m, u, s, NA)
    return y_v if parts == 1 else y_adv if parts == 2 else y_v + y_adv


def masked_max(q, avail):
    qm = q.clone().detach()
    qm[avail == 0] = -9999999
    return qm.max(dim=3)


def td_forward_qplex(q_lambda=False, noise=None):
    """A function with ref_learner.td_forward's signature and extras (relu= included)
    whose mixer is QPLEX and whose rows are PyMARL2's dmaq_qatten_learner's with
    double_q: substitute it for ref_learner.td_forward with monkeypatch.setattr.
    q_lambda and noise as tests/qmix_model.td_forward_mixer."""

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
        NA = mac_out.shape[3]
        chosen = torch.gather(mac_out[:, :-1], 3, actions[:, :-1]).squeeze(3)
        max_on, cur_max = masked_max(mac_out, avail)  # (detached: no gradient reaches the maxima)
        extra = {}
        with torch.no_grad():
            tgt_out = agent_q(p_agent_tgt, obs, h0, cfg, noise and noise[1])
            max_tg = masked_max(tgt_out, avail)[0]
            target_q = torch.gather(tgt_out, 3, cur_max.unsqueeze(3)).squeeze(3)
            qtot_tgt = qplex_forward(p_mixer_tgt, target_q, max_tg, cur_max, state, NA)
            extra.update(rows_tg=(target_q, max_tg))
            if q_lambda:
                from tests.qlambda_model import build_q_lambda_targets
                taken = torch.gather(tgt_out[:, :-1], 3, actions[:, :-1]).squeeze(3)
                qtot_taken = qplex_forward(p_mixer_tgt, taken, max_tg[:, :-1], actions[:, :-1, :, 0], state[:, :-1], NA)
                targets = build_q_lambda_targets(rewards, terminated, mask, qtot_tgt, qtot_taken, gamma, td_lambda)
                extra["qtot_taken"] = qtot_taken
            else:
                targets = ref_learner.build_td_lambda_targets(rewards, terminated, mask, qtot_tgt, gamma, td_lambda)
        qtot = qplex_forward(p_mixer, chosen, max_on[:, :-1], actions[:, :-1, :, 0], state[:, :-1], NA)
        extra.update(rows_on=(chosen.detach(), max_on[:, :-1]))
        td_error = qtot - targets.detach()
        masked = 0.5 * td_error.pow(2) * mask
        if per_weight is not None:
            masked = masked.sum(1) * per_weight
        loss = masked.sum() / mask.sum()
        prio = ((td_error.abs() * mask).sum(1) / torch.sqrt(mask.sum(1))).detach()
        return loss, prio, dict(qtot=qtot.detach(), qtot_tgt=qtot_tgt, targets=targets, mac_out=mac_out.detach(),
                                **extra)
    return td_forward
