"""Test helper (no tests here): the learner's two other PyMARL2 switches on the CPU.

* Peng's Q(λ) targets (NQLearner with q_lambda: True, utils/rl_utils.py
  build_q_lambda_targets), restated from the formula that defines them
  (include/t2omca.h t2o_td_qlambda), with Q' the target mixer's double-Q mix
  [B, T+1] and Qk the target mixer on the target Q of the taken actions:

      ret_T = Q'_T · (1 − Σ_t term_t)
      ret_t = λγ·ret_{t+1} + m_t · (r_t + (Q'_t − Qk_t) + (1−λ)γ · Q'_{t+1} · (1 − term_t))
      targets = ret_{0..T−1}

* td_forward_qlambda: oracle.ref_learner.td_forward with those targets, built from
  the same oracle.ref_model unrolls; same signature and return value, extras gain
  "qtot_taken".  tests.gpu_util.oracle_td_tie_aware looks ref_learner.td_forward up
  when it is called, so a test substitutes this with monkeypatch.setattr.

* rmsprop_ref: clip_grad_norm_ + torch.optim.RMSprop (momentum 0, not centered)
  in fp64, shaped like tests.gpu_util.adam_ref.
"""
import torch

from oracle import ref_model


def build_q_lambda_targets(rewards, terminated, mask, exp_qvals, qvals, gamma, td_lambda):
    """exp_qvals [B, T+1] (Q'), qvals [B, >=T] (Qk, steps 0..T-1 read), others [B, T]."""
    ret = exp_qvals.new_zeros(*exp_qvals.shape)
    ret[:, -1] = exp_qvals[:, -1] * (1 - torch.sum(terminated, dim=1))
    for t in range(ret.shape[1] - 2, -1, -1):
        corrected = rewards[:, t] + (exp_qvals[:, t] - qvals[:, t])
        ret[:, t] = td_lambda * gamma * ret[:, t + 1] + mask[:, t] * (
            corrected + (1 - td_lambda) * gamma * exp_qvals[:, t + 1] * (1 - terminated[:, t]))
    return ret[:, 0:-1]


def td_forward_qlambda(p_agent, p_mixer, p_agent_tgt, p_mixer_tgt, batch, cfg, *, gamma=0.99, td_lambda=0.6,
                       per_weight=None, detach_mixer_hidden=False, relu=None):
    """oracle.ref_learner.td_forward with q_lambda: True."""
    if relu is not None:
        prev, ref_model._ffn_relu = ref_model._ffn_relu, relu
        try:
            return td_forward_qlambda(p_agent, p_mixer, p_agent_tgt, p_mixer_tgt, batch, cfg, gamma=gamma,
                                      td_lambda=td_lambda, per_weight=per_weight,
                                      detach_mixer_hidden=detach_mixer_hidden)
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
    mac_out, hs = ref_model.agent_unroll(p_agent, obs, h0, cfg=cfg)
    chosen = torch.gather(mac_out[:, :-1], 3, actions[:, :-1]).squeeze(3)
    obs_tok = None if cfg.get("state_entity_mode", True) else obs
    with torch.no_grad():
        tgt_out, tgt_hs = ref_model.agent_unroll(p_agent_tgt, obs, h0, cfg=cfg)
        mac_det = mac_out.clone().detach()
        mac_det[avail == 0] = -9999999
        cur_max = mac_det.max(dim=3, keepdim=True)[1]
        target_max_q = torch.gather(tgt_out, 3, cur_max).squeeze(3)
        hw0 = torch.zeros(B, 3, cfg["mixer_emb"], dtype=obs.dtype)
        qtot_tgt, _ = ref_model.mixer_unroll(p_mixer_tgt, target_max_q, tgt_hs, state, hw0, cfg=cfg, obs=obs_tok)
        # the target mixer once more, on the target Q of the actions that were taken
        taken_q = torch.gather(tgt_out, 3, actions).squeeze(3)
        qtot_taken, _ = ref_model.mixer_unroll(p_mixer_tgt, taken_q, tgt_hs, state, hw0, cfg=cfg, obs=obs_tok)
        targets = build_q_lambda_targets(rewards, terminated, mask, qtot_tgt, qtot_taken, gamma, td_lambda)
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
                            qtot_taken=qtot_taken[:, :-1])


def rmsprop_ref(p, g, sq, *, lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=0.0, max_norm=10.0, grad_div=None):
    """clip_grad_norm_ + torch.optim.RMSprop (momentum 0, not centered) restated in
    fp64 on the CPU, applied to the inputs upcast.  Returns (p, square_avg, norm):
    the new state and the gradient norm before clipping."""
    p, g, sq = (x.detach().cpu().double() for x in (p, g, sq))
    if grad_div is not None:
        g = g / float(grad_div)
    norm = g.norm()
    if max_norm > 0:
        g = g * min(max_norm / (float(norm) + 1e-6), 1.0)
    if weight_decay != 0:
        g = g + weight_decay * p
    sq = alpha * sq + (1 - alpha) * g * g
    return p - lr * g / (sq.sqrt() + eps), sq, float(norm)


def rmsprop_errors(p_gpu, sq_gpu, ref, p_before):
    """(err_sq, err_p, bar_p) of one RMSprop transition against rmsprop_ref's result,
    as tests.gpu_util.adam_errors: square_avg normwise (bar 1e-6), p absolute against
    bar_p = 2^-24·max|p_ref| + 1e-5·max|p_ref - p_before|."""
    p_ref, sq_ref = ref[:2]
    p_before = p_before.detach().cpu().double()
    err_p = float((p_gpu.detach().cpu().double() - p_ref).abs().max())
    bar_p = 2.0 ** -24 * float(p_ref.abs().max()) + 1e-5 * float((p_ref - p_before).abs().max())
    sq_err = float((sq_gpu.detach().cpu().double() - sq_ref).abs().max() / max(float(sq_ref.abs().max()), 1e-30))
    return sq_err, err_p, bar_p
