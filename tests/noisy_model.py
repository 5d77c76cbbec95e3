"""TEST INFRASTRUCTURE ONLY: fp64 restatement of the NoisyNet Q head
(include/t2omca.h t2o_noise_normal / t2o_noisy_head_*).

utils.noisy_liner does not ship with the reference, so the head is a DECLARED
definition (parity-unpinned): the independent-Gaussian NoisyNet layer as PyMARL2 uses it,

    q = (u_w + s_w ⊙ ε_w) h + (u_b + s_b ⊙ ε_b),   ε ~ N(0, 1) per element,

one ε per forward call (per timestep t of an unroll, shared by every episode and agent).
Noise: element k of step t (k = n·E + e for ε_w[n][e], k = NA·E + n for ε_b[n]) is
Box–Muller on env_spec.uniforms,

    u1 = U(seed', env = t, draw = c·4096 + 2k),  u2 = U(seed', t, c·4096 + 2k + 1),
    seed' = (4·seed + kind) mod 2^64,  z = sqrt(−2 ln(1 − u1)) · cos(2π u2)  in fp64,

rounded once to fp32 (kind 0 learner online, 1 learner target, 2 runner, 3 module).
"""
import numpy as np
import torch

from oracle import ref_model
from oracle.ref_learner import build_td_lambda_targets
from t2omca_amd.env_spec import uniforms

KINDS = {"learner_online": 0, "learner_target": 1, "runner": 2, "module": 3}
_M64 = (1 << 64) - 1


def noise64(E, NA, t0, t1, seed, kind, counter):
    """The fp64 Box–Muller values of steps [t0, t1): (eps_w [t1-t0, NA, E], eps_b [t1-t0, NA])."""
    nk = NA * (E + 1)
    assert nk <= 2048 and 0 <= counter < (1 << 28) and 0 <= t0 < t1 <= (1 << 24)
    seedp = (4 * int(seed) + KINDS.get(kind, kind)) & _M64
    z = np.empty((t1 - t0, nk))
    for t in range(t0, t1):
        u = uniforms(seedp, t, counter * 4096, 2 * nk)
        z[t - t0] = np.sqrt(-2.0 * np.log(1.0 - u[0::2])) * np.cos(2.0 * np.pi * u[1::2])
    return z[:, :NA * E].reshape(-1, NA, E), z[:, NA * E:]


def noise_normal(E, NA, T, seed, kind, counter):
    """What t2o_noise_normal writes: the fp64 values rounded once to fp32 (numpy arrays)."""
    w, b = noise64(E, NA, 0, T, seed, kind, counter)
    return w.astype(np.float32), b.astype(np.float32)


def noisy_head(h, u_w, u_b, s_w, s_b, eps_w=None, eps_b=None):
    """h [B, T, A, E] -> q [B, T, A, NA] with step t's weights W_t = u_w + s_w ⊙ eps_w[t],
    b_t = u_b + s_b ⊙ eps_b[t] (eps None: the mean head).  Differentiable torch."""
    if eps_w is None:
        return torch.einsum("btae,ne->btan", h, u_w) + u_b
    T = h.shape[1]
    W = u_w.unsqueeze(0) + s_w.unsqueeze(0) * eps_w[:T]
    b = u_b.unsqueeze(0) + s_b.unsqueeze(0) * eps_b[:T]
    return torch.einsum("btae,tne->btan", h, W) + b[None, :, None, :]


def noisy_head_grads(h, u_w, s_w, eps_w, eps_b, gchosen, actions, gh_in=None):
    """The head's backward written out (what t2o_noisy_head_bwd / _wgrad compute), fp64:
    returns (gh_out [B,T,A,E], du_w, du_b, ds_w, ds_b) for dL/dq[action] = gchosen [B,T,A]."""
    B, T, A, E = h.shape
    NA = u_w.shape[0]
    W = u_w.unsqueeze(0) + s_w.unsqueeze(0) * eps_w[:T]                 # [T, NA, E]
    idx = actions.reshape(B, T, A)
    Wa = W[torch.arange(T)[None, :, None].expand(B, T, A), idx]          # [B, T, A, E]
    gh = gchosen.unsqueeze(-1) * Wa
    if gh_in is not None:
        gh = gh + gh_in
    onehot = torch.nn.functional.one_hot(idx, NA).to(h.dtype)            # [B, T, A, NA]
    G = torch.einsum("btan,bta,btae->tne", onehot, gchosen, h)          # [T, NA, E]
    Gb = torch.einsum("btan,bta->tn", onehot, gchosen)
    return gh, G.sum(0), Gb.sum(0), (eps_w[:T] * G).sum(0), (eps_b[:T] * Gb).sum(0)


def _plain(p):
    """A noisy agent's parameters as the plain agent ref_model runs (q_basic = the means)."""
    q = {k: v for k, v in p.items() if not k.startswith("q_basic.")}
    q["q_basic.weight"], q["q_basic.bias"] = p["q_basic.u_w"], p["q_basic.u_b"]
    return q


def _head(p, hs, eps):
    return noisy_head(hs, p["q_basic.u_w"], p["q_basic.u_b"], p["q_basic.s_w"], p["q_basic.s_b"],
                      *(eps if eps is not None else (None, None)))


def td_forward_noisy(p_agent, p_mixer, p_agent_tgt, p_mixer_tgt, batch, cfg, *, eps_on, eps_tg, gamma=0.99,
                     td_lambda=0.6, per_weight=None, detach_mixer_hidden=False, relu=None, q_lambda=False):
    """oracle.ref_learner.td_forward with the noisy head applied to ref_model.agent_unroll's
    hidden states for both networks: eps_on / eps_tg = (eps_w [T+1, NA, E], eps_b [T+1, NA])
    fp64 tensors, or None for the mean head.  q_lambda: Peng's Q(λ) targets
    (tests/qlambda_model.py) on the noisy target Q."""
    if relu is not None:
        prev, ref_model._ffn_relu = ref_model._ffn_relu, relu
        try:
            return td_forward_noisy(p_agent, p_mixer, p_agent_tgt, p_mixer_tgt, batch, cfg, eps_on=eps_on,
                                    eps_tg=eps_tg, gamma=gamma, td_lambda=td_lambda, per_weight=per_weight,
                                    detach_mixer_hidden=detach_mixer_hidden, q_lambda=q_lambda)
        finally:
            ref_model._ffn_relu = prev
    obs, state = batch["obs"], batch["state"]
    actions, avail = batch["actions"], batch["avail_actions"]
    B, T1, A, _ = obs.shape
    E = cfg["emb"]
    rewards = batch["reward"][:, :-1, 0]
    terminated = batch["terminated"][:, :-1, 0].float()
    mask = batch["filled"][:, :-1, 0].float()
    mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
    h0 = torch.zeros(B, A, E, dtype=obs.dtype)
    _, hs = ref_model.agent_unroll(_plain(p_agent), obs, h0, cfg=cfg)
    mac_out = _head(p_agent, hs, eps_on)
    chosen = torch.gather(mac_out[:, :-1], 3, actions[:, :-1]).squeeze(3)
    obs_tok = None if cfg.get("state_entity_mode", True) else obs
    extra = {}
    with torch.no_grad():
        _, tgt_hs = ref_model.agent_unroll(_plain(p_agent_tgt), obs, h0, cfg=cfg)
        tgt_out = _head(p_agent_tgt, tgt_hs, eps_tg)
        mac_det = mac_out.clone().detach()
        mac_det[avail == 0] = -9999999
        cur_max = mac_det.max(dim=3, keepdim=True)[1]
        target_max_q = torch.gather(tgt_out, 3, cur_max).squeeze(3)
        hw0 = torch.zeros(B, 3, cfg["mixer_emb"], dtype=obs.dtype)
        qtot_tgt, _ = ref_model.mixer_unroll(p_mixer_tgt, target_max_q, tgt_hs, state, hw0, cfg=cfg, obs=obs_tok)
        if q_lambda:
            from tests.qlambda_model import build_q_lambda_targets
            taken_q = torch.gather(tgt_out, 3, actions).squeeze(3)
            qtot_taken, _ = ref_model.mixer_unroll(p_mixer_tgt, taken_q, tgt_hs, state, hw0, cfg=cfg, obs=obs_tok)
            targets = build_q_lambda_targets(rewards, terminated, mask, qtot_tgt, qtot_taken, gamma, td_lambda)
            extra["qtot_taken"] = qtot_taken[:, :-1]
        else:
            targets = build_td_lambda_targets(rewards, terminated, mask, qtot_tgt, gamma, td_lambda)
    hid = hs[:, :-1].detach() if detach_mixer_hidden else hs[:, :-1]
    hw0 = torch.zeros(B, 3, cfg["mixer_emb"], dtype=obs.dtype)
    qtot, _ = ref_model.mixer_unroll(p_mixer, chosen, hid, state[:, :-1], hw0, cfg=cfg,
                                     obs=None if obs_tok is None else obs[:, :-1])
    td_error = qtot - targets.detach()
    masked = 0.5 * td_error.pow(2) * mask
    if per_weight is not None:
        masked = masked.sum(1) * per_weight
    loss = masked.sum() / mask.sum()
    prio = ((td_error.abs() * mask).sum(1) / torch.sqrt(mask.sum(1))).detach()
    return loss, prio, dict(qtot=qtot.detach(), qtot_tgt=qtot_tgt, targets=targets, mac_out=mac_out.detach(),
                            tgt_out=tgt_out, hs=hs.detach(), **extra)
