"""Drop-in replacements for the reference's hot-path modules.

``TransformerAgent`` and ``TransformerMixer`` keep the reference constructor
signatures, the args fields they read, ``init_hidden`` and the forward
signatures (transf_agent.py:9-76, n_transf_mixer.py:13-91) and register
exactly the reference parameter tree, so ``state_dict`` keys/shapes match
(SURVEY.md §8 b) and checkpoints move between the two frameworks.

The forward passes run the HIP kernels (one-step unrolls of
t2o_agent_unroll_fwd / t2o_mixer_unroll_fwd); autograd is supported through
the BPTT kernels with T = 1.  The TD update itself does not go through these
per-step forwards: ``t2omca_amd.learner.TDLearner`` runs whole-unroll kernels
on the same parameters.  CPU tensors raise — there is no CPU fallback.
"""
import torch
import torch.nn as nn

from . import _lib, ops


class MultiHeadAttention(nn.Module):
    """Parameter container with the reference names (transformer.py:34-38)."""

    def __init__(self, emb, heads=8, mask=False):
        super().__init__()
        self.emb, self.heads, self.mask = emb, heads, mask
        self.tokeys = nn.Linear(emb, emb * heads, bias=False)
        self.toqueries = nn.Linear(emb, emb * heads, bias=False)
        self.tovalues = nn.Linear(emb, emb * heads, bias=False)
        self.unifyheads = nn.Linear(heads * emb, emb)


class TransformerBlock(nn.Module):
    """Parameter container (transformer.py:103-118)."""

    def __init__(self, emb, heads, mask, ff_hidden_mult=4, dropout=0.0):
        super().__init__()
        self.attention = MultiHeadAttention(emb, heads=heads, mask=mask)
        self.mask = mask
        self.norm1 = nn.LayerNorm(emb)
        self.norm2 = nn.LayerNorm(emb)
        self.ff = nn.Sequential(nn.Linear(emb, ff_hidden_mult * emb), nn.ReLU(),
                                nn.Linear(ff_hidden_mult * emb, emb))
        self.do = nn.Dropout(dropout)


class Transformer(nn.Module):
    """Parameter container (transformer.py:143-167); the compute is fused in HIP."""

    def __init__(self, emb, heads, depth, ff_hidden_mult=4, dropout=0.0):
        super().__init__()
        if dropout != 0.0:
            raise ValueError("t2omca_amd: dropout > 0 is not supported (the reference path uses 0)")
        self.tblocks = nn.Sequential(*[TransformerBlock(emb=emb, heads=heads, mask=False,
                                                        ff_hidden_mult=ff_hidden_mult, dropout=dropout)
                                       for _ in range(depth)])


class _PackCache:
    """The flat parameters and folded kernel pack of a module, rebuilt only when a
    parameter changes.

    The reference MAC calls the agent once per env step (parallel_runner.py:121 ->
    transf_agent.py:54-76) with the same weights until the learner's next update.
    Concatenating and re-packing them on every call (forward and again in the
    backward) cost two extra launches per step.  The key is every parameter's
    storage pointer and autograd version counter: optimiser steps,
    ``load_state_dict`` and ``copy_`` bump the version, re-binding a parameter
    changes its pointer, so a stale pack is never used.  A rebuild allocates new
    tensors, so a pack saved for an earlier backward is never overwritten.
    Writes the version counter cannot see — through ``p.data`` (``p.data.copy_``
    shares the storage, not the counter) or through raw device pointers (the
    learner's Adam kernel) — must be followed by ``invalidate()``."""

    def __init__(self):
        self.key = None
        self.flat = None
        self.pack = None
        self.rebuilds = 0

    def get(self, module, shape):
        params = tuple(module.parameters())
        key = tuple((p.data_ptr(), p._version) for p in params)
        if key != self.key:
            with torch.no_grad():
                flat = torch.cat([p.detach().reshape(-1) for p in params])
            # (a noisy agent's sigmas follow the plain agent's parameters: the pack reads the prefix)
            self.flat, self.pack = flat, ops.pack_params(shape, flat[:shape.n_params])
            self.key = key
            self.rebuilds += 1
        return params, self.flat, self.pack

    def invalidate(self):
        """For writers that bypass autograd's version counters (the learner's Adam
        kernel and broadcasts write the parameters through raw device pointers)."""
        self.key = None


def _split_like(gflat, shapes):
    """The flat gradient (reference parameter order) as one view per parameter."""
    out, o = [], 0
    for sh in shapes:
        n = sh.numel()
        out.append(gflat[o:o + n].view(sh))
        o += n
    return tuple(out)


def orthogonal_init_(m, gain=1.0):
    """PyMARL2's utils.th_utils.orthogonal_init_ (imported by n_transf_mixer.py:6,
    applied to every submodule at :48-50; the module itself is absent from the
    reference, so this restates its published form): orthogonal Linear weights,
    zero biases.  Bias-free Linears (the attention projections) keep no bias."""
    if isinstance(m, nn.Linear):
        nn.init.orthogonal_(m.weight.data, gain=gain)
        if m.bias is not None:
            nn.init.constant_(m.bias.data, 0)


class _AgentStep(torch.autograd.Function):
    """One agent step on the HIP kernels.  The parameters enter as separate inputs
    (their gradients leave as views of one flat buffer), and the cached flat copy
    and pack serve both directions."""

    @staticmethod
    def forward(ctx, shape, flat, pack, inputs, hidden, *params):
        b, a, nf = inputs.shape
        obs = inputs.detach().contiguous().view(b, 1, a, nf)
        h0 = hidden.detach().reshape(b * a, shape.E).contiguous()
        q, h = ops.agent_unroll_fwd(shape, pack, obs, h0_on=h0)
        ctx.save_for_backward(flat, pack, obs, h0, h)
        ctx.shape, ctx.param_shapes = shape, [p.shape for p in params]
        return q[:, 0], h[:, 0]

    @staticmethod
    def backward(ctx, gq, gh):
        flat, pack, obs, h0, h = ctx.saved_tensors
        shape = ctx.shape
        b, _, a, _ = obs.shape
        gq = (gq if gq is not None else torch.zeros_like(h[:, 0, :, :0])).contiguous().view(b, 1, a, -1)
        gh = (gh if gh is not None else torch.zeros_like(h[:, 0])).contiguous().view(b, 1, a, shape.E)
        gpack, gh0 = ops.agent_unroll_bwd(shape, pack, obs, h, h0=h0, gq=gq, gh=gh, want_gh0=True)
        gflat = torch.zeros_like(flat)
        ops.unpack_grads(shape, flat, gpack, gflat)
        return (None, None, None, None, gh0.view(b, a, shape.E)) + _split_like(gflat, ctx.param_shapes)


class NoisyLinear(nn.Module):
    """Parameter container of the NoisyNet head (transf_agent.py:37-39 builds
    ``NoisyLinear(emb, n_actions)`` from utils.noisy_liner, which does not ship with
    the reference; this is the DECLARED definition of DESIGN.md §5, the
    independent-Gaussian layer as PyMARL2 uses it):

        training:  q = (u_w + s_w ⊙ ε_w) h + (u_b + s_b ⊙ ε_b),  ε ~ N(0, 1), fresh per call
        eval:      q = u_w h + u_b

    The means take nn.Linear's default initialisation, the sigmas are 0.017.
    Registered in the order u_w, u_b, s_w, s_b: an agent's flat parameters are then a
    plain agent's (q_basic.weight = u_w, q_basic.bias = u_b) followed by the sigmas."""

    SIGMA_INIT = 0.017

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        if not bias:
            raise ValueError("t2omca_amd: NoisyLinear is built with a bias (transf_agent.py:38)")
        self.in_features, self.out_features = in_features, out_features
        lin = nn.Linear(in_features, out_features)  # its default initialisation, its random draws
        self.u_w = nn.Parameter(lin.weight.detach().clone())
        self.u_b = nn.Parameter(lin.bias.detach().clone())
        self.s_w = nn.Parameter(torch.full((out_features, in_features), self.SIGMA_INIT))
        self.s_b = nn.Parameter(torch.full((out_features,), self.SIGMA_INIT))


class _NoisyHead(torch.autograd.Function):
    """The noisy head of one step on the HIP kernels (t2o_noisy_head_*): gradients to
    h and the four parameters.  The backward kernel works on one action's gradient per
    row (the learner's chosen-Q form), so a full dL/dq runs it once per action, each
    pass adding to dL/dh and to the weight-gradient sums."""

    @staticmethod
    def forward(ctx, h, u_w, u_b, s_w, s_b, eps_w, eps_b):
        b, a, E = h.shape
        h4 = h.detach().contiguous().view(b, 1, a, E)
        pw = [p.detach().contiguous() for p in (u_w, u_b, s_w, s_b)]
        q = torch.empty(b, 1, a, u_w.shape[0], device=h.device)
        ops.noisy_head_fwd(h4, q, pw[0], pw[1], pw[2], pw[3], eps=(eps_w, eps_b))
        ctx.save_for_backward(h4, pw[0], pw[2], eps_w, eps_b)
        return q[:, 0]

    @staticmethod
    def backward(ctx, gq):
        h4, u_w, s_w, eps_w, eps_b = ctx.saved_tensors
        b, _, a, E = h4.shape
        NA = u_w.shape[0]
        gq = gq.contiguous()
        gh = gpart = None
        g = [torch.zeros_like(u_w), torch.zeros(NA, device=u_w.device),
             torch.zeros_like(u_w), torch.zeros(NA, device=u_w.device)]
        for n in range(NA):
            act = torch.full((b, 1, a), n, dtype=torch.int64, device=h4.device)
            gh, gpart = ops.noisy_head_bwd(gq[:, :, n].contiguous().view(b, 1, a), act, h4, u_w, s_w, eps_w,
                                           gh_in=gh, gh_out=gh, gpart=gpart)
            ops.noisy_head_wgrad(gpart, b, a, g[0], g[1], g[2], g[3], eps=(eps_w, eps_b))
        return gh[:, 0], g[0], g[1], g[2], g[3], None, None


class TransformerAgent(nn.Module):
    """transf_agent.py:8-76 drop-in (HIP forward/backward).

    ``args.action_selector == "noisy-new"`` builds the NoisyLinear head
    (transf_agent.py:37-39): ``noisy`` is then True, and a training-mode forward draws
    fresh noise (counter-based: seed ``noise_seed`` = args.noise_seed or 0, kind
    "module", counter ``noise_calls``, which it increments) and runs the head on the
    noisy-head kernels; an eval-mode forward is the mean head, the fused path."""

    kind = "transformer"

    def __init__(self, input_shape, args):
        super().__init__()
        self.args = args
        self.n_agents = args.n_agents
        self.n_entities = getattr(self.args, "n_entities_obs", self.args.n_entities)
        self.feat_dim = args.obs_entity_feats
        self.emb_dim = args.emb
        self.feat_embedding = nn.Linear(self.feat_dim, self.emb_dim)
        self.transformer = Transformer(args.emb, args.heads, args.depth, args.ff_hidden_mult, args.dropout)
        self.noisy = getattr(self.args, "action_selector", None) == "noisy-new"
        self.noise_seed = int(getattr(self.args, "noise_seed", 0))
        self.noise_calls = 0  # training-mode forwards so far: the next one's noise counter
        if self.noisy:
            self.q_basic = NoisyLinear(args.emb, args.n_actions)
        else:
            self.q_basic = nn.Linear(args.emb, args.n_actions)
        self.shape = ops.NetShape(ops.AGENT, args.emb, args.heads, args.depth, self.feat_dim, args.n_actions,
                                  args.ff_hidden_mult * args.emb, self.n_entities)
        self._pack_cache = _PackCache()

    def init_hidden(self):
        return torch.zeros(1, self.args.emb, device=self.args.device)

    def forward(self, inputs, hidden_state):
        b, a, _ = inputs.size()
        if b * a * self.emb_dim != hidden_state.numel():
            hidden_state = hidden_state.expand(b, a, self.emb_dim)
        params, flat, pack = self._pack_cache.get(self, self.shape)
        q, h = _AgentStep.apply(self.shape, flat, pack, inputs, hidden_state, *params)
        if self.noisy and self.training:
            # the fused step's q (the mean head) is unused; h carries the gradient
            nl = self.q_basic
            eps_w, eps_b = ops.noise_normal(self.emb_dim, nl.out_features, 1, self.noise_seed, "module",
                                            self.noise_calls, device=h.device)
            self.noise_calls += 1
            q = _NoisyHead.apply(h, nl.u_w, nl.u_b, nl.s_w, nl.s_b, eps_w, eps_b)
        return q.view(b, a, -1), h.view(b, a, -1)


class _RnnStep(torch.autograd.Function):
    """One GRU agent step on the HIP kernels (t2o_rnn_fwd / t2o_rnn_bwd with one step):
    the parameters enter as separate inputs, their gradients leave as views of one flat
    buffer (the slab sum, in the parameter order).  `inputs` is the built input row, so
    the kernels see it as an observation without one-hots."""

    @staticmethod
    def forward(ctx, shape, inputs, hidden, *params):
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1) for p in params])
        b, a, nf = inputs.shape
        obs = inputs.detach().contiguous().view(b, 1, a, nf)
        h0 = hidden.detach().reshape(b, a, shape.H).contiguous()
        fwd = ops.rnn_agent_fwd(shape, flat, obs, h0_on=h0)
        ctx.save_for_backward(flat, obs, h0, fwd["x_on"], fwd["gi_on"], fwd["h_on"])
        ctx.shape, ctx.param_shapes = shape, [p.shape for p in params]
        return fwd["q_on"][:, 0], fwd["h_on"][:, 0]

    @staticmethod
    def backward(ctx, gq, gh):
        flat, obs, h0, x, gi, h = ctx.saved_tensors
        shape = ctx.shape
        b, _, a, _ = obs.shape
        gq = (gq if gq is not None else torch.zeros(b, a, shape.NA, device=obs.device)).contiguous()
        gh = None if gh is None else gh.contiguous().view(b, 1, a, shape.H)
        slabs, nslab, gh0 = ops.rnn_agent_bwd(shape, flat, obs, dict(x_on=x, gi_on=gi, h_on=h), h0=h0,
                                              gq=gq.view(b, 1, a, shape.NA), gh=gh, want_gh0=True)
        gflat = ops.reduce_slabs(slabs, nslab, torch.empty_like(flat))
        return (None, None, gh0) + _split_like(gflat, ctx.param_shapes)


class RNNAgent(nn.Module):
    """The recurrent agent of the QMIX baselines, PyMARL2's modules/agents/n_rnn_agent.py
    `RNNAgent` with use_layer_norm=False: fc1 -> ReLU -> GRUCell -> fc2, shared by all
    agents.  No agent but the transformer ships with the reference: this is the DECLARED
    definition of DESIGN.md §5, parity-unpinned.

    ``input_shape`` is the width of the built input (BasicMAC._build_inputs): the
    flattened observation, then the one-hot of the last action if args.obs_last_action
    (default True), then the one-hot of the agent if args.obs_agent_id (default True).
    H = args.rnn_hidden_dim (64).  Torch's default initialisation; args.use_orthogonal
    applies orthogonal_init_ to fc1 and fc2 as PyMARL2 does.  ``forward`` takes the built
    inputs [b, a, input_shape]; ``shape`` describes how the learner and the runner build
    them from observations and actions inside the kernels."""

    kind = "rnn"

    def __init__(self, input_shape, args):
        super().__init__()
        self.args = args
        self.n_agents = A = int(args.n_agents)
        self.n_actions = NA = int(args.n_actions)
        self.hidden_dim = H = int(getattr(args, "rnn_hidden_dim", 64))
        self.input_shape = IN = int(input_shape)
        self.obs_last_action = bool(getattr(args, "obs_last_action", True))
        self.obs_agent_id = bool(getattr(args, "obs_agent_id", True))
        if getattr(args, "use_layer_norm", False):
            raise ValueError("RNNAgent: use_layer_norm=True is not supported (the GRU kernels have no LayerNorm)")
        if H not in ops.RNN_HIDDEN:
            raise ValueError(f"RNNAgent: rnn_hidden_dim={H}: the GRU kernels take {ops.RNN_LIMITS}")
        obs_dim = IN - (NA if self.obs_last_action else 0) - (A if self.obs_agent_id else 0)
        if not (1 <= A <= 64 and 1 <= NA <= 16 and obs_dim >= 1 and IN <= 656):
            raise ValueError(f"RNNAgent: n_agents={A}, n_actions={NA}, input width {IN} (obs width {obs_dim}): the "
                             f"GRU kernels take {ops.RNN_LIMITS}")
        self.fc1 = nn.Linear(IN, H)
        self.rnn = nn.GRUCell(H, H)
        self.fc2 = nn.Linear(H, NA)
        if getattr(args, "use_orthogonal", False):
            orthogonal_init_(self.fc1)
            orthogonal_init_(self.fc2, gain=getattr(args, "gain", 0.01))
        self.shape = ops.RnnShape(A, obs_dim, NA, H, self.obs_last_action, self.obs_agent_id)
        self._step_shape = ops.RnnShape(A, IN, NA, H, False, False)  # forward's rows are built inputs

    def init_hidden(self):
        return torch.zeros(1, self.hidden_dim, device=self.args.device)

    def forward(self, inputs, hidden_state):
        if not inputs.is_cuda:
            raise RuntimeError("RNNAgent.forward needs HIP-device tensors (no CPU fallback)")
        b, a, _ = inputs.size()
        if b * a * self.hidden_dim != hidden_state.numel():
            hidden_state = hidden_state.expand(b, a, self.hidden_dim)
        q, h = _RnnStep.apply(self._step_shape, inputs, hidden_state.reshape(b, a, self.hidden_dim),
                              *self.parameters())
        return q.view(b, a, -1), h.view(b, a, -1)


def make_agent(input_shape, args):
    """args.agent: "rnn" or "n_rnn" (PyMARL2's name) -> RNNAgent, absent or anything else
    -> the reference's TransformerAgent."""
    if getattr(args, "agent", None) in ("rnn", "n_rnn"):
        return RNNAgent(input_shape, args)
    return TransformerAgent(input_shape, args)


class _MixerStep(torch.autograd.Function):
    """One mixer step on the HIP kernels (parameters as separate inputs, as _AgentStep)."""

    @staticmethod
    def forward(ctx, shape, flat, pack, qvals, hidden_states, hyper_weights, states, *params):
        b = qvals.shape[0]
        A, E = shape.agents, shape.E
        qv = qvals.detach().reshape(b, 1, A).contiguous()
        hid = hidden_states.detach().reshape(b, 1, A, E).contiguous()
        hw0 = hyper_weights.detach().reshape(b, 3, E).contiguous()
        st = states.detach().reshape(b, 1, -1).contiguous()
        out = ops.mixer_unroll_fwd(shape, pack, st, hid, qmode_on=0, qv_on=qv, hw0_on=hw0)
        ctx.save_for_backward(flat, pack, qv, hid, hw0, st, out["y"], out["hw"], out["qv"], out["xout"])
        ctx.xmid = out["xmid"]
        ctx.shape, ctx.param_shapes = shape, [p.shape for p in params]
        return out["y"].view(b, 1, 1), out["hw"][:, 0]

    @staticmethod
    def backward(ctx, gy, ghw):
        flat, pack, qv, hid, hw0, st, y, hw, qvo, xout = ctx.saved_tensors
        shape = ctx.shape
        b = qv.shape[0]
        gy = (gy if gy is not None else torch.zeros_like(y)).reshape(b, 1).contiguous()
        ghw = ghw.reshape(b, 1, 3, shape.E).contiguous() if ghw is not None else None
        fwd = dict(y=y, hw=hw, qv=qvo, xout=xout, xmid=ctx.xmid)
        gpack, gqv, ghid, ghw0 = ops.mixer_unroll_bwd(shape, pack, st, hid, fwd, gy, hw0=hw0, ghw_ext=ghw,
                                                      want_ghw0=True)
        gflat = torch.zeros_like(flat)
        ops.unpack_grads(shape, flat, gpack, gflat)
        return ((None, None, None, gqv.view(b, 1, -1), ghid.view(b, -1, shape.E), ghw0, None)
                + _split_like(gflat, ctx.param_shapes))


class TransformerMixer(nn.Module):
    """n_transf_mixer.py:12-102 drop-in (HIP forward/backward).

    Every pos_func of the reference (:95-103: softplus with qmix_pos_func_beta,
    quadratic, abs, anything else = identity), both input branches (:60-63:
    state_entity_mode -> the n_entities_state state tokens; otherwise the
    n_agents * n_entities obs tokens, which needs state_entity_feats == the obs
    feature width), n_entities_state != n_agents and use_orthogonal (:48-50).
    Shapes without a tuned MFMA instance run the runtime-shaped kernels."""

    kind = "transformer"

    def __init__(self, args, abs=True):
        super().__init__()
        self.args = args
        self.n_agents = args.n_agents
        self.n_entities = getattr(self.args, "n_entities_state", self.args.n_entities)
        self.feat_dim = args.state_entity_feats
        self.emb_dim = args.mixer_emb
        self.feat_embedding = nn.Linear(self.feat_dim, self.emb_dim)
        self.transformer = Transformer(args.mixer_emb, args.mixer_heads, args.mixer_depth,
                                       args.ff_hidden_mult, args.dropout)
        self.qmix_pos_func = getattr(self.args, "qmix_pos_func", "abs")
        self.custom_space = args.env_args.get("state_entity_mode", True)
        self.hyper_b2 = nn.Linear(self.emb_dim, 1)
        if getattr(args, "use_orthogonal", False):
            for m in self.modules():
                orthogonal_init_(m)
        pos = _lib.POS_FUNCS.get(self.qmix_pos_func, 3)
        beta = float(getattr(args, "qmix_pos_func_beta", 1.0)) if self.qmix_pos_func == "softplus" else 1.0
        # state tokens: the state's entities, or (obs branch) every agent's obs entities
        n_tok = self.n_entities if self.custom_space else self.n_agents * self.n_entities
        self.shape = ops.NetShape(ops.MIXER, args.mixer_emb, args.mixer_heads, args.mixer_depth, self.feat_dim, 1,
                                  args.ff_hidden_mult * args.mixer_emb, n_tok, n_agents=self.n_agents,
                                  pos_func=pos, pos_beta=beta)
        self._pack_cache = _PackCache()

    def init_hidden(self):
        # n_transf_mixer.py:52-53 (shape [1, A, E] as in the reference)
        return torch.zeros(1, self.n_agents, self.args.emb, device=self.args.device)

    def forward(self, qvals, hidden_states, hyper_weights, states, obs):
        b = qvals.size(0)
        hyper_weights = hyper_weights.expand(b, 3, self.emb_dim)
        tokens = states if self.custom_space else obs  # n_transf_mixer.py:60-63
        params, flat, pack = self._pack_cache.get(self, self.shape)
        return _MixerStep.apply(self.shape, flat, pack, qvals, hidden_states, hyper_weights, tokens, *params)


class _QMixStep(torch.autograd.Function):
    """QMixer.forward on the HIP kernels (t2o_qmix_fwd / t2o_qmix_bwd): the parameters
    enter as separate inputs, their gradients leave as views of one flat buffer (the
    slab sum, in the parameter order)."""

    @staticmethod
    def forward(ctx, shape, qvals, states, *params):
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1) for p in params])
        qv = qvals.detach().contiguous()
        st = states.detach()
        if st.stride(2) != 1:
            st = st.contiguous()
        y = ops.qmix_fwd(shape, flat, st, qv)
        ctx.save_for_backward(flat, qv, st)
        ctx.shape, ctx.param_shapes = shape, [p.shape for p in params]
        return y.unsqueeze(2)

    @staticmethod
    def backward(ctx, gy):
        flat, qv, st = ctx.saved_tensors
        gqv, slabs, nslab = ops.qmix_bwd(ctx.shape, flat, st, qv, gy.reshape(qv.shape[:2]).contiguous())
        gflat = ops.reduce_slabs(slabs, nslab, torch.empty_like(flat))
        return (None, gqv, None) + _split_like(gflat, ctx.param_shapes)


class QMixer(nn.Module):
    """The classic QMIX hypernetwork mixer, PyMARL2's modules/mixers/nmix.py `Mixer`.
    It does not ship with the reference (n_transf_mixer.py only): this is the DECLARED
    definition of DESIGN.md §5, parity-unpinned.  Per (episode, step) row

        w1 = pos(hyper_w1(s)).view(A, M)    b1 = hyper_b1(s)
        w2 = pos(hyper_w2(s))               b2 = hyper_b2(s)
        y  = elu(q @ w1 + b1) @ w2 + b2

    with M = args.mixing_embed_dim (32), H = args.hypernet_embed (64), the state width
    S = prod(args.state_shape) (default: the state's entities x state_entity_feats) and
    pos the qmix_pos_func of TransformerMixer (``abs=False``: identity).  Torch's
    default initialisation.  What the kernels do not take is a ValueError here."""

    kind = "qmix"

    def __init__(self, args, abs=True):
        super().__init__()
        self.args = args
        self.n_agents = A = int(args.n_agents)
        self.embed_dim = M = int(getattr(args, "mixing_embed_dim", 32))
        self.hypernet_embed = H = int(getattr(args, "hypernet_embed", 64))
        state_shape = getattr(args, "state_shape", None)
        if state_shape is None:
            state_shape = getattr(args, "n_entities_state", args.n_entities) * args.state_entity_feats
        self.state_dim = S = int(torch.Size([state_shape] if isinstance(state_shape, int) else state_shape).numel())
        self.qmix_pos_func = getattr(args, "qmix_pos_func", "abs") if abs else "identity"
        if not (1 <= A <= 64 and 1 <= S <= 1024 and M in (16, 32) and H in (32, 64)):
            raise ValueError(f"QMixer: n_agents={A}, state width {S}, mixing_embed_dim={M}, hypernet_embed={H}: the "
                             f"QMIX kernels take {ops.QMIX_LIMITS}")
        self.hyper_w1 = nn.Sequential(nn.Linear(S, H), nn.ReLU(inplace=True), nn.Linear(H, A * M))
        self.hyper_b1 = nn.Sequential(nn.Linear(S, M))
        self.hyper_w2 = nn.Sequential(nn.Linear(S, H), nn.ReLU(inplace=True), nn.Linear(H, M))
        self.hyper_b2 = nn.Sequential(nn.Linear(S, M), nn.ReLU(inplace=True), nn.Linear(M, 1))
        pos = _lib.POS_FUNCS.get(self.qmix_pos_func, 3)
        beta = float(getattr(args, "qmix_pos_func_beta", 1.0)) if self.qmix_pos_func == "softplus" else 1.0
        self.shape = ops.QmixShape(A, S, M, H, pos_func=pos, pos_beta=beta)
        # the learner reads the state whatever state_entity_mode says (these mixers take no obs tokens)
        self.custom_space = True

    def forward(self, qvals, states):
        if not qvals.is_cuda:
            raise RuntimeError("QMixer.forward needs HIP-device tensors (no CPU fallback)")
        b, T = qvals.shape[:2]
        return _QMixStep.apply(self.shape, qvals.reshape(b, T, self.n_agents), states.reshape(b, T, self.state_dim),
                               *self.parameters())


class _VDNStep(torch.autograd.Function):
    """VDNMixer.forward on the HIP kernels: the row sum of the select kernel's family
    (t2o_vdn_bwd spreads the gradient back)."""

    @staticmethod
    def forward(ctx, qvals):
        qv = qvals.detach().contiguous()
        ctx.A = qv.shape[2]
        return ops.vdn_fwd(qv).unsqueeze(2)

    @staticmethod
    def backward(ctx, gy):
        return ops.vdn_bwd(gy[..., 0].contiguous(), A=ctx.A)


class VDNMixer(nn.Module):
    """PyMARL2's modules/mixers/vdn.py: y = Σ_a q_a.  No parameters.  (Declared, absent
    from the reference: DESIGN.md §5.)"""

    kind = "vdn"
    custom_space = True

    def forward(self, qvals, states=None):
        if not qvals.is_cuda:
            raise RuntimeError("VDNMixer.forward needs HIP-device tensors (no CPU fallback)")
        return _VDNStep.apply(qvals)


class _QPlexStep(torch.autograd.Function):
    """QPlexMixer.forward on the HIP kernels (t2o_qplex_fwd / t2o_qplex_bwd): `parts` 1 is
    y_v, 2 is y_adv.  The parameters enter as separate inputs, their gradients leave as
    views of one flat buffer (the slab sum, in the parameter order).  No gradient reaches
    the maxima, and none reaches q through y_adv (its c = w (q − m) is a constant)."""

    @staticmethod
    def forward(ctx, shape, parts, qvals, states, qmax, act, *params):
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1) for p in params])
        qv = qvals.detach().contiguous()
        st = states.detach()
        if st.stride(2) != 1:
            st = st.contiguous()
        y = ops.qplex_fwd(shape, flat, st, qv, qmax, act, parts=parts)
        ctx.save_for_backward(flat, qv, st, qmax, act)
        ctx.shape, ctx.parts, ctx.param_shapes = shape, parts, [p.shape for p in params]
        return y.unsqueeze(2)

    @staticmethod
    def backward(ctx, gy):
        flat, qv, st, qmax, act = ctx.saved_tensors
        gqv, slabs, nslab = ops.qplex_bwd(ctx.shape, flat, st, qv, qmax, act, gy.reshape(qv.shape[:2]).contiguous(),
                                          parts=ctx.parts)
        gflat = ops.reduce_slabs(slabs, nslab, torch.empty_like(flat))
        return (None, None, gqv, None, None, None) + _split_like(gflat, ctx.param_shapes)


class _SIWeight(nn.Module):
    """The parameter tree of PyMARL2's dmaq_si_weight.DMAQ_SI_Weight at adv_hypernet_layers 2."""

    def __init__(self, A, S, NA, HA, K):
        super().__init__()
        def net(n_in, n_out):
            return nn.Sequential(nn.Linear(n_in, HA), nn.ReLU(), nn.Linear(HA, n_out))
        self.key_extractors = nn.ModuleList([net(S, 1) for _ in range(K)])
        self.agents_extractors = nn.ModuleList([net(S, A) for _ in range(K)])
        self.action_extractors = nn.ModuleList([net(S + A * NA, A) for _ in range(K)])


class QPlexMixer(nn.Module):
    """The QPLEX duelling mixer, PyMARL2's modules/mixers/dmaq_general.py `DMAQer` with
    dmaq_si_weight.py at qplex.yaml's defaults.  It does not ship with the reference
    (n_transf_mixer.py only): this is the DECLARED definition of DESIGN.md §5,
    parity-unpinned.  Per (episode, step) row, with sg the stop-gradient,

        w = |hyper_w_final(s)| + 1e-10      v = V(s)
        λ = Σ_k (|key_k(s)| + 1e-10) · sigmoid(agents_k(s)) · sigmoid(action_k([s ; onehot(u)]))
        y_v = Σ_a (w_a q_a + v_a)           y_adv = Σ_a sg[w_a (q_a − m_a)] (λ_a − 1)

    with H = args.hypernet_embed (64), HA = args.adv_hypernet_embed (64), K =
    args.num_kernel (4), the state width S = prod(args.state_shape) (default: the state's
    entities x state_entity_feats) and NA = args.n_actions.  Torch's default
    initialisation.  What the kernels do not take is a ValueError here."""

    kind = "qplex"
    custom_space = True  # the learner reads the state whatever state_entity_mode says

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.n_agents = A = int(args.n_agents)
        self.n_actions = NA = int(args.n_actions)
        self.hypernet_embed = H = int(getattr(args, "hypernet_embed", 64))
        self.adv_hypernet_embed = HA = int(getattr(args, "adv_hypernet_embed", 64))
        self.num_kernel = K = int(getattr(args, "num_kernel", 4))
        state_shape = getattr(args, "state_shape", None)
        if state_shape is None:
            state_shape = getattr(args, "n_entities_state", args.n_entities) * args.state_entity_feats
        self.state_dim = S = int(torch.Size([state_shape] if isinstance(state_shape, int) else state_shape).numel())
        layers = int(getattr(args, "adv_hypernet_layers", 2))
        weighted, minus_one = getattr(args, "weighted_head", True), getattr(args, "is_minus_one", True)
        if not (1 <= A <= 64 and 1 <= S <= 1024 and 1 <= NA <= 16 and H in (32, 64) and HA in (32, 64) and
                1 <= K <= 10 and layers == 2 and weighted is True and minus_one is True):
            raise ValueError(f"QPlexMixer: n_agents={A}, state width {S}, n_actions={NA}, hypernet_embed={H}, "
                             f"adv_hypernet_embed={HA}, num_kernel={K}, adv_hypernet_layers={layers}, "
                             f"weighted_head={weighted}, is_minus_one={minus_one}: the QPLEX kernels take "
                             f"{ops.QPLEX_LIMITS}")
        self.hyper_w_final = nn.Sequential(nn.Linear(S, H), nn.ReLU(), nn.Linear(H, A))
        self.V = nn.Sequential(nn.Linear(S, H), nn.ReLU(), nn.Linear(H, A))
        self.si_weight = _SIWeight(A, S, NA, HA, K)
        self.shape = ops.QplexShape(A, S, NA, H, HA, K)

    def forward(self, agent_qs, states, actions=None, max_q_i=None, is_v=False):
        """PyMARL2's DMAQer.forward: is_v=True -> y_v [b, T, 1]; is_v=False -> y_adv, with
        `actions` one-hot [b, T, A, NA] or an index [b, T, A] and `max_q_i` [b, T, A]."""
        if not agent_qs.is_cuda:
            raise RuntimeError("QPlexMixer.forward needs HIP-device tensors (no CPU fallback)")
        b, T = agent_qs.shape[:2]
        A = self.n_agents
        q = agent_qs.reshape(b, T, A)
        if is_v:  # (the kernels read both arrays in either part: zeros, which y_v does not depend on)
            qmax = torch.zeros(b, T, A, device=q.device)
            act = torch.zeros(b, T, A, device=q.device, dtype=torch.int32)
        else:
            if actions is None or max_q_i is None:
                raise ValueError("QPlexMixer.forward: is_v=False needs actions and max_q_i")
            idx = actions.argmax(dim=3) if actions.dim() == 4 and actions.shape[3] == self.n_actions else actions
            act = idx.reshape(b, T, A).to(torch.int32).contiguous()
            qmax = max_q_i.detach().reshape(b, T, A).float().contiguous()
        return _QPlexStep.apply(self.shape, 1 if is_v else 2, q, states.reshape(b, T, self.state_dim), qmax, act,
                                *self.parameters())


def make_mixer(args):
    """args.mixer: "qmix" -> QMixer, "vdn" -> VDNMixer, "dmaq" (PyMARL2's name) or "qplex"
    -> QPlexMixer, absent or anything else -> the reference's TransformerMixer."""
    name = getattr(args, "mixer", None)
    if name == "qmix":
        return QMixer(args)
    if name == "vdn":
        return VDNMixer()
    if name in ("dmaq", "qplex"):
        return QPlexMixer(args)
    return TransformerMixer(args)
