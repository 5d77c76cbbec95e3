"""GPU TD update with the reference driver's learner contract.

per_run.py:224-238 calls

    info = learner.train(episode_sample, runner.t_env, episode, weights)
    buffer.update_priorities(idx, (info["td_errors_abs"].flatten() + 1e-6).numpy().tolist())

The reference's learner module is absent, so the semantics are
the PyMARL2 NQLearner ones (oracle/ref_learner.py restates them on the CPU;
parity-unpinned beyond the agent/mixer arithmetic).  One ``train`` call is a
fixed sequence of HIP launches on the current stream (no host sync until the
priorities are copied out):

  pack(online agent, online mixer)                 t2o_pack_params x2
  agent unroll fwd, online + target, t = 0..T      t2o_agent_unroll_fwd (1 launch)
  mixer unroll fwd, online (chosen Q, t < T) +
        target (double-Q, t <= T)                  t2o_mixer_unroll_fwd (1 launch)
  [q_lambda: mixer unroll fwd, the target mixer on
   the target Q at the taken actions, t < T        t2o_mixer_unroll_fwd (one network)]
  TD(λ) targets, loss, dL/dQtot, priorities        t2o_td_loss
  [q_lambda: Peng's Q(λ) targets instead           t2o_td_qlambda]
  mixer BPTT -> dL/dq_chosen, dL/dhidden           t2o_mixer_unroll_bwd
  mixer tape contraction + slab sum + unfold       side stream, issued here; it
                                                   runs as the agent BPTT's waves drain
  agent BPTT, its tape contraction, slab sum,      t2o_agent_unroll_bwd, ...
  unfold into the reference parameter order        t2o_unpack_grads
  [data parallel: all_reduce of the flat grad + Σ mask over RCCL in two
   halves, the mixer's from the side stream; neither runs under a BPTT kernel,
   whose waves hold every SIMD]
  (contract="pair": both tapes in one launch after the agent BPTT, one all-reduce)
  clip_grad_norm_ + Adam                           t2o_adam_step
  [optimizer="rmsprop": clip_grad_norm_ + RMSprop  t2o_rmsprop_step]

A noisy agent (modules.TransformerAgent with action_selector "noisy-new",
``agent.noisy``) adds the NoisyNet head's launches — a plain agent
issues none of them:

  ε of the online and the target network, T+1 steps each   t2o_noise_normal x2 (side stream,
      (seed noise_seed, counter step_count, kinds 0 / 1)    beside the packs)
  after the agent unroll (per step range when pipelined):
      q_on, q_tg overwritten from h_on, h_tg               t2o_noisy_head_fwd x2
  after the mixer BPTT (per step range when pipelined):
      dL/dh = dL/dhidden + dL/dq_chosen · W_t[action],
      per-step weight-gradient partials                     t2o_noisy_head_bwd
  the agent BPTT then runs on dL/dh alone (no q gradient: the fused head adds zeros
  to q_basic's slots), and after t2o_unpack_grads
      Σ_t partials into the u_w, u_b, s_w, s_b slots        t2o_noisy_head_wgrad
The mixers, the TD loss and the Q(λ) taken mix read the q arrays and run unchanged.
The head is fp32 in both precisions.  noise_seed is NOT mixed with the rank: every
data-parallel rank draws the same network, so the shard sum is the full-batch gradient.

A QMIX or VDN mixer (modules.QMixer / VDNMixer, ``mixer.kind`` "qmix" / "vdn"; DESIGN.md
§5) replaces the two mixer steps — a TransformerMixer learner launches exactly the above:

  chosen Q (t < T) and double-Q selection (t <= T),        t2o_q_select (1 launch; vdn:
      both networks                                         its row sums are the mix)
  qmix: both networks' mix                                  t2o_qmix_fwd (1 launch)
  [q_lambda: the target Q at the actions, and its mix       t2o_q_select, t2o_qmix_fwd (one network)]
  dL/dq_chosen, the rows' activations                       t2o_qmix_bwd phase 1 (vdn: t2o_vdn_bwd)
  qmix: weight-gradient slabs, their sum into the flat      t2o_qmix_bwd phase 2, t2o_reduce_slabs: side
      gradient, the mixer half's all-reduce                 stream, beside the agent BPTT
These mixers read the state alone: no gradient reaches the agents' hidden states
(detach_mixer_hidden has no effect), they are fp32 in both precisions, read their
parameters straight from the flat buffers (no pack), and run the sequential update
(pipeline=True is a ValueError; "auto" never pipelines them).

A QPLEX mixer (modules.QPlexMixer, ``mixer.kind`` "qplex", PyMARL2's mixer: dmaq with
its dmaq_qatten_learner and double_q) is the third of these flat mixers:

  chosen / double-Q Q, each network's avail-masked         t2o_qplex_select (1 launch)
      maximum of its own Q and the action used
  both networks' y_v + y_adv                                t2o_qplex_fwd (1 launch, parts 3)
  [q_lambda: the target Q, maxima at the batch's actions,   t2o_qplex_select, t2o_qplex_fwd (one network)]
      and their mix
  dL/dq_chosen = dL/dy · w, the rows' activations           t2o_qplex_bwd phase 1
  weight-gradient slabs, their sum, the all-reduce          t2o_qplex_bwd phase 2, t2o_reduce_slabs: side stream
No gradient reaches the maxima; ``learner.last_qmax`` keeps them beside ``last_qv``.

A GRU agent (modules.RNNAgent, ``agent.kind`` "rnn", PyMARL2's agent: rnn)
under one of the flat mixers replaces the agent's launches — a transformer-agent learner
launches exactly the above:

  both networks' fc1, ReLU and W_ih products over every    t2o_rnn_fwd (two launches: the
      (episode, step, agent) row, then the recurrence       time-parallel rows, the recurrence)
  the reverse recurrence from dL/dq_chosen, the rows'      t2o_rnn_bwd (three launches),
      dL/dx, the weight-gradient slabs and their sum        t2o_reduce_slabs
It reads its parameters straight from the flat buffers (no pack), builds its inputs
(observation, last action's one-hot, agent's one-hot) inside the kernels, and is fp32 in
both precisions.  A transformer mixer, pipeline=True and a noisy head are ValueErrors.
"""
import dataclasses
import os

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .distributed import allreduce_async, broadcast_state, wait_all
from .state import check_fields, copy_checked


OPTIMIZERS = {"adam": "Adam", "rmsprop": "RMSprop"}  # TDLearner(optimizer=...): the torch.optim class of opt.th
MIXERS = ("transformer", "qmix", "vdn", "qplex")  # modules.TransformerMixer / QMixer / VDNMixer / QPlexMixer .kind
AGENTS = ("transformer", "rnn")  # modules.TransformerAgent / RNNAgent .kind


def _agent_kind_of(state_dict):
    """Which of AGENTS wrote this agent.th (None: neither), by its keys."""
    if "rnn.weight_hh" in state_dict and "fc1.weight" in state_dict:
        return "rnn"
    if any(k.startswith("transformer.tblocks") for k in state_dict):
        return "transformer"
    return None


def _mixer_kind_of(state_dict):
    """Which of MIXERS wrote this mixer.th (None: none of them), by its keys."""
    if not state_dict:
        return "vdn"
    if "hyper_w1.0.weight" in state_dict:
        return "qmix"
    if "hyper_w_final.0.weight" in state_dict:
        return "qplex"
    if any(k.startswith("transformer.tblocks") for k in state_dict):
        return "transformer"
    return None


def _optimiser_of(opt_state):
    """Which of OPTIMIZERS wrote this torch optimiser state_dict (None: neither): by
    its per-parameter state, or, saved before the first step, by its param_groups."""
    seen = [st for st in opt_state.get("state", {}).values() if st] or list(opt_state.get("param_groups", []))
    for d in seen:
        if "exp_avg" in d or "betas" in d:
            return "adam"
        if "square_avg" in d or "alpha" in d:
            return "rmsprop"
    return None


def _bind_flat(modules, device):
    """Move the modules' parameters into one flat fp32 buffer (views)."""
    params = [p for m in modules for p in m.parameters()]
    n = sum(p.numel() for p in params)
    flat = torch.empty(n, device=device, dtype=torch.float32)
    off = 0
    for p in params:
        k = p.numel()
        flat[off:off + k].copy_(p.detach().reshape(-1))
        p.data = flat[off:off + k].view_as(p)
        off += k
    return flat


class TDLearner:
    def __init__(self, agent, mixer, *, lr=1e-3, gamma=0.99, td_lambda=0.6, grad_norm_clip=10.0,
                 target_update_interval=200, optim_betas=(0.9, 0.999), optim_eps=1e-8, weight_decay=0.0,
                 detach_mixer_hidden=False, process_group=None, priorities_to_cpu=True, precision="fp32",
                 overlap=True, td_algo="auto", contract="side", pipeline="auto", pipeline_ranges=6,
                 logger=None, learner_log_interval=10000, q_lambda=False, optimizer="adam", optim_alpha=0.99,
                 noise_seed=0):
        # options first (a bad value fails here, not inside the first train())
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        if contract not in ("pair", "side"):
            raise ValueError("contract must be 'pair' or 'side'")
        if td_algo not in ops.TD_ALGOS:
            raise ValueError(f"td_algo must be one of {sorted(ops.TD_ALGOS)}, got {td_algo!r}")
        if pipeline not in ("auto", True, False) or int(pipeline_ranges) < 1:
            raise ValueError("pipeline must be 'auto', True or False and pipeline_ranges >= 1")
        if pipeline is True and (contract == "pair" or not overlap):
            raise ValueError("pipeline=True runs the mixer's contraction on the side stream: it needs "
                             "contract='side' and overlap=True")
        if q_lambda not in (True, False):
            raise ValueError(f"q_lambda must be True or False, got {q_lambda!r}")
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {list(OPTIMIZERS)}, got {optimizer!r}")
        if not 0.0 <= float(optim_alpha) < 1.0:
            raise ValueError(f"optim_alpha must lie in [0, 1), got {optim_alpha!r}")
        # which mixer (modules.*.kind): the reference's TransformerMixer, or the declared QMIX / VDN
        self.mixer_kind = getattr(mixer, "kind", "transformer")
        if self.mixer_kind not in MIXERS:
            raise ValueError(f"mixer.kind must be one of {list(MIXERS)}, got {self.mixer_kind!r}")
        if pipeline is True and self.mixer_kind != "transformer":
            raise ValueError(f"pipeline=True runs the update in step ranges, which needs the decoupled transformer "
                             f"mixer; a {self.mixer_kind} mixer runs the sequential update (pipeline='auto' or False)")
        # which agent (modules.*.kind): the reference's TransformerAgent, or the declared GRU agent
        self.agent_kind = getattr(agent, "kind", "transformer")
        if self.agent_kind not in AGENTS:
            raise ValueError(f"agent.kind must be one of {list(AGENTS)}, got {self.agent_kind!r}")
        if self.agent_kind == "rnn":
            if self.mixer_kind == "transformer":
                raise ValueError("an rnn agent trains under the flat mixers (qmix, vdn, qplex) that are supported; "
                                 "the transformer mixer reads the transformer agent's hidden tokens")
            if pipeline is True:
                raise ValueError("pipeline=True runs the update in step ranges, which the rnn agent's kernels do "
                                 "not take (pipeline='auto' or False)")
            if getattr(getattr(agent, "args", None), "action_selector", None) == "noisy-new":
                raise ValueError("an rnn agent has no noisy head (action_selector='noisy-new' needs the "
                                 "transformer agent)")
        # the transformer mixer's MFMA unroll selects the chosen / double-Q values from Q rows it
        # keeps in registers, narrower than the agent head (include/t2omca.h t2o_mixer_unroll_fwd;
        # its runtime-shaped kernels read the rows from memory and take every agent head)
        n_actions = getattr(getattr(agent, "shape", None), "NA", None)
        if self.mixer_kind == "transformer" and n_actions is not None and not mixer.shape.generic:
            max_actions = int(ops.lib().t2o_mixer_max_actions())
            if n_actions > max_actions:
                raise ValueError(f"the transformer mixer's Q selection takes at most {max_actions} actions "
                                 f"(t2o_mixer_max_actions), this agent has {n_actions}; the qmix, vdn and dmaq "
                                 f"mixers take up to 16")
        dev = next(agent.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("TDLearner needs the modules on a HIP device (no CPU fallback)")
        self.agent, self.mixer = agent, mixer
        # bf16: MFMA operands (weights, activations entering a matrix product) in
        # bf16; accumulation, LayerNorm, softmax, recurrent state, TD targets, grads
        # and the Adam master weights stay fp32
        prec = 1 if precision == "bf16" else 0
        self.precision = precision
        # (the GRU agent's ops.RnnShape: fp32 in both precisions)
        self.sa = agent.shape if self.agent_kind == "rnn" else dataclasses.replace(agent.shape, prec=prec)
        if self.mixer_kind == "transformer":
            self.sm = dataclasses.replace(mixer.shape, prec=prec)
        else:  # ops.QmixShape / QplexShape (fp32 in both precisions), or None: VDN has no parameters
            self.sm = getattr(mixer, "shape", None)
        # a noisy agent's flat parameters: the plain agent's na_net floats (what the packs and
        # the fused kernels read), then the head's NA·(E+1) sigmas
        self.noisy = bool(getattr(agent, "noisy", False))
        self.noise_seed = int(noise_seed)
        self.na_net, self.nm = self.sa.n_params, self.sm.n_params if self.sm is not None else 0
        self.n_head = self.sa.NA * (self.sa.E + 1)
        self.na = self.na_net + (self.n_head if self.noisy else 0)
        assert self.na == sum(p.numel() for p in agent.parameters())
        assert self.nm == sum(p.numel() for p in mixer.parameters())
        self.device = dev
        self.params = _bind_flat([agent, mixer], dev)
        self.grad = torch.zeros(self.na + self.nm + 1, device=dev)  # last slot: Σ mask
        # (optimizer="rmsprop": exp_avg_sq is RMSprop's square_avg and exp_avg stays zero)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.target_params = self.params.clone()
        self.pg = process_group
        # data parallel: every replica starts from rank 0's parameters (ranks that
        # initialised with different seeds would otherwise drift apart silently)
        broadcast_state([self.params, self.target_params], self.pg)
        self._params_written()
        self.adam_ws = torch.empty(int(ops.lib().t2o_adam_workspace_floats()), device=dev)
        self.grad_norm = torch.zeros(1, device=dev)
        self.lr, self.betas, self.eps, self.wd = lr, optim_betas, optim_eps, weight_decay
        # PyMARL2 NQLearner's two other switches: Peng's Q(λ) targets (args.q_lambda) and
        # RMSprop(lr, alpha=optim_alpha, eps=optim_eps) (args.optimizer != 'adam')
        self.q_lambda, self.optimizer, self.alpha = bool(q_lambda), optimizer, float(optim_alpha)
        self.gamma, self.td_lambda, self.clip = gamma, td_lambda, grad_norm_clip
        self.target_update_interval = target_update_interval
        self.detach_mixer_hidden = detach_mixer_hidden
        self.priorities_to_cpu = priorities_to_cpu
        self.overlap = overlap  # mixer tape contraction on a side stream beside the agent BPTT
        self.td_algo = td_algo  # ops.TD_ALGOS
        # "side" (default): the mixer's tape contraction on the side stream, issued
        # before the agent BPTT — it cannot run beside the BPTT (whose waves hold
        # every SIMD) but its workgroups take the CUs the BPTT's last waves free;
        # "pair": both contractions in one launch after the agent BPTT, measured
        # 15 us slower per update (profiles/r4_b/: 2.455 vs 2.438 ms)
        self.contract = contract
        # small replay batches: the agent and the (decoupled) mixer recurrences run
        # side by side on two streams in step ranges (_pipelined).  "auto": wherever
        # the layout and batch allow it (never with contract="pair", which contracts
        # both tapes in one launch after the agent BPTT); True: required — train()
        # raises when the update cannot be pipelined; False: never
        self.pipeline, self.pipeline_ranges = pipeline, int(pipeline_ranges)
        self.step_count = 0
        self.last_target_update_episode = 0
        self.timer = None   # optional callable(tag) recording HIP events around the big kernels
        if self.agent_kind != "rnn":  # (the GRU agent reads the flat parameters: no pack)
            self.pack_a = torch.empty(self.sa.layout().pack_floats, device=dev)
            self.pack_at = torch.empty_like(self.pack_a)
        if self.mixer_kind == "transformer":  # (the other mixers read the flat parameters: no pack)
            self.pack_m = torch.empty(self.sm.layout().pack_floats, device=dev)
            self.pack_mt = torch.empty_like(self.pack_m)
        self._pack_targets()
        self._slabs = {}
        # logged statistics (PyMARL2 NQLearner: every learner_log_interval env steps);
        # without a logger train() issues nothing for them
        self.logger = logger
        self.learner_log_interval = learner_log_interval
        self.log_stats_t = -learner_log_interval - 1
        self._stat = torch.zeros(6, dtype=torch.float64, device=dev) if logger is not None else None

    # -- parameters --------------------------------------------------------
    def _params_written(self):
        """The Adam kernel and the replica broadcasts write the modules' parameters
        through raw pointers, which autograd's version counters do not see: drop the
        modules' cached kernel packs (modules._PackCache) so their next per-step
        forward re-packs."""
        for m in (self.agent, self.mixer):
            cache = getattr(m, "_pack_cache", None)
            if cache is not None:
                cache.invalidate()

    def agent_params(self, target=False):
        src = self.target_params if target else self.params
        return src[:self.na]

    def mixer_params(self, target=False):
        src = self.target_params if target else self.params
        return src[self.na:]

    def _head_views(self, flat):
        """(u_w [NA, E], u_b [NA], s_w, s_b) of a noisy agent's head as views of a flat
        buffer laid out like the parameters (params, target_params, grad): the means are
        the plain agent's last NA·(E+1) floats (q_basic.weight, bias), the sigmas follow."""
        NA, E = self.sa.NA, self.sa.E
        o, n = self.na_net - self.n_head, self.na_net
        return (flat[o:o + NA * E].view(NA, E), flat[o + NA * E:n],
                flat[n:n + NA * E].view(NA, E), flat[n + NA * E:n + self.n_head])

    def _draw_noise(self, T1):
        """ε of this update's online and target network (kinds 0 / 1, counter step_count:
        a function of the seeds and the step alone, so a resumed run draws the same),
        two launches on the current stream into buffers the learner keeps."""
        NA, E = self.sa.NA, self.sa.E
        out = []
        for name, kind in (("on", "learner_online"), ("tg", "learner_target")):
            eps = (self._buf("eps_w_" + name, (T1, NA, E)), self._buf("eps_b_" + name, (T1, NA)))
            out.append(ops.noise_normal(E, NA, T1, self.noise_seed, kind, self.step_count, out=eps))
        self.last_noise = tuple(out)  # (online, target), each (eps_w [T+1, NA, E], eps_b [T+1, NA])
        return self.last_noise

    def _pack_targets(self):
        if self.agent_kind != "rnn":
            ops.pack_params(self.sa, self.target_params[:self.na_net], self.pack_at)
        if self.mixer_kind == "transformer":
            ops.pack_params(self.sm, self.target_params[self.na:], self.pack_mt)

    def update_targets(self):
        self.target_params.copy_(self.params)
        self._pack_targets()

    def _world(self):
        if self.pg is not None or (dist.is_available() and dist.is_initialized()):
            return dist.get_world_size(self.pg)
        return 1

    def _buf(self, key, shape):
        t = self._slabs.get(key)
        n = 1
        for d in shape:
            n *= d
        if t is None or t.numel() < n:
            t = torch.empty(n, device=self.device)
            self._slabs[key] = t
        return t[:n].view(shape)

    def _side_stream(self):
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(self.device)
        return self._side

    def _slab(self, key, n):
        t = self._slabs.get(key)
        if t is None or t.numel() < n:
            t = torch.empty(n, device=self.device)
            self._slabs[key] = t
        return t

    # -- checkpoints (per_run.py:159-189 load, :265-279 save) -----------------
    def cuda(self):
        """per_run.py:156 calls learner.cuda(); the learner already lives on its HIP device."""
        return self

    def _optimiser_view(self):
        """A torch.optim.Adam (or RMSprop) over the modules' parameters (mac then
        mixer, the order of a PyMARL2 NQLearner's optimiser) carrying this learner's
        moments, so opt.th is that optimiser's standard state_dict."""
        params = list(self.agent.parameters()) + list(self.mixer.parameters())
        if self.optimizer == "rmsprop":
            opt = torch.optim.RMSprop(params, lr=self.lr, alpha=self.alpha, eps=self.eps, weight_decay=self.wd)
        else:
            opt = torch.optim.Adam(params, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.wd)
        off = 0
        for p in params:
            k = p.numel()
            if self.step_count:
                opt.state[p] = {"step": torch.tensor(float(self.step_count))}
                for name, buf in self._moments():
                    opt.state[p][name] = buf[off:off + k].view_as(p)
            off += k
        return opt

    def _moments(self):
        """(name in the torch optimiser's per-parameter state, flat buffer) pairs."""
        if self.optimizer == "rmsprop":
            return (("square_avg", self.exp_avg_sq),)
        return (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq))

    def save_models(self, path):
        """PyMARL layout: {path}/agent.th, mixer.th (reference state_dict keys) and
        opt.th (torch Adam / RMSprop state_dict)."""
        torch.save(self.agent.state_dict(), os.path.join(path, "agent.th"))
        torch.save(self.mixer.state_dict(), os.path.join(path, "mixer.th"))
        torch.save(self._optimiser_view().state_dict(), os.path.join(path, "opt.th"))

    def load_models(self, path):
        """Inverse of save_models; also takes checkpoints written by the reference
        framework.  As PyMARL2's NQLearner does, the target agent is reloaded from
        agent.th and the target mixer is left as it is; opt.th is optional, and one
        written by the other optimiser is a ValueError naming both, and so is a mixer.th
        of another kind of mixer (told by its keys: transformer, qmix, qplex, or vdn's empty
        dict), and an agent.th of the other kind of agent (transformer or rnn).  opt.th follows the
        modules' parameter order (a noisy agent: q_basic.u_w, u_b, s_w, s_b last of the
        agent's); an agent.th of the other head, or an opt.th whose per-parameter shapes
        are not these modules', is a ValueError that says so.  Every check comes before
        anything is overwritten."""
        def load(name):
            return torch.load(os.path.join(path, name), map_location=self.device, weights_only=True)
        saved = load("opt.th") if os.path.exists(os.path.join(path, "opt.th")) else None
        held = _optimiser_of(saved) if saved is not None else None
        if held is not None and held != self.optimizer:  # (before anything is overwritten)
            raise ValueError(f"opt.th holds the state of a {OPTIMIZERS[held]} optimiser, this learner runs "
                             f"{OPTIMIZERS[self.optimizer]} (optimizer={self.optimizer!r})")
        agent_sd = load("agent.th")
        if _agent_kind_of(agent_sd) != self.agent_kind:
            raise ValueError(f"agent.th holds a {_agent_kind_of(agent_sd)} agent, this learner's agent is a "
                             f"{self.agent_kind} one (the kinds are {' and '.join(AGENTS)})")
        if ("q_basic.u_w" in agent_sd) != self.noisy:
            kinds = ("a NoisyLinear (noisy-new)", "a plain Linear")
            raise ValueError(f"agent.th holds {kinds['q_basic.u_w' not in agent_sd]} q_basic head, this learner's "
                             f"agent has {kinds[self.noisy]} one (noisy={self.noisy})")
        mixer_sd = load("mixer.th")
        if _mixer_kind_of(mixer_sd) != self.mixer_kind:
            raise ValueError(f"mixer.th holds a {_mixer_kind_of(mixer_sd)} mixer, this learner's mixer is a "
                             f"{self.mixer_kind} one")
        if saved is not None:
            params = list(self.agent.parameters()) + list(self.mixer.parameters())
            ids = [i for g in saved.get("param_groups", []) for i in g["params"]]
            if len(ids) != len(params):
                raise ValueError(f"opt.th holds the state of {len(ids)} parameters, this learner's modules have "
                                 f"{len(params)} (a checkpoint of another network or head?)")
            for n, (i, p) in enumerate(zip(ids, params)):
                for name, _ in self._moments():
                    st = saved.get("state", {}).get(i)
                    if st and name in st and tuple(st[name].shape) != tuple(p.shape):
                        raise ValueError(f"opt.th: {name} of parameter {n} is {tuple(st[name].shape)}, this "
                                         f"learner's parameter {n} is {tuple(p.shape)}: its per-parameter shapes "
                                         f"do not match these modules' parameter order")
        with torch.no_grad():
            self.agent.load_state_dict(agent_sd)  # copies into the flat-buffer views
            self.mixer.load_state_dict(mixer_sd)
            self.target_params[:self.na].copy_(self.params[:self.na])
        if saved is None:
            self._sync_replicas()
            return
        opt = self._optimiser_view()
        opt.load_state_dict(saved)
        off, steps = 0, set()
        for p in list(self.agent.parameters()) + list(self.mixer.parameters()):
            k = p.numel()
            st = opt.state.get(p)
            if st:
                for name, buf in self._moments():
                    buf[off:off + k].copy_(st[name].reshape(-1))
                steps.add(int(float(st["step"])))
            off += k
        if len(steps) > 1:
            raise ValueError(f"opt.th: parameters carry different {OPTIMIZERS[self.optimizer]} step counts "
                             f"{sorted(steps)}")
        self.step_count = steps.pop() if steps else 0
        self._sync_replicas()

    # -- saved state (driver.save_run_state) -------------------------------------
    def state_dict(self):
        """The whole learner, unlike save_models' PyMARL files: the flat parameters,
        the target parameters (agent AND mixer half), the Adam moments and step
        count, and the two schedule counters (target update, log).  CPU copies,
        ordered after the update queued on the current stream (train() ends with
        the main stream waiting for the side stream)."""
        return {"format": 1, "na": self.na, "nm": self.nm, "precision": self.precision,
                "params": self.params.detach().cpu(), "target_params": self.target_params.detach().cpu(),
                "exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu(),
                "step_count": int(self.step_count),
                "last_target_update_episode": int(self.last_target_update_episode),
                "log_stats_t": int(self.log_stats_t),
                # (optim_alpha as a 0-d fp64 tensor: every value here is a tensor, an int or a str)
                "q_lambda": self.q_lambda, "optimizer": self.optimizer,
                "optim_alpha": torch.tensor(self.alpha, dtype=torch.float64),
                # the NoisyNet head: with it `na` covers the sigmas; its noise is a function of
                # noise_seed and step_count alone, so no further state
                "noisy": self.noisy, "noise_seed": self.noise_seed,
                # the kind of mixer (MIXERS) the mixer half of the flat buffers belongs to
                "mixer": self.mixer_kind,
                # the kind of agent (AGENTS) the agent half belongs to
                "agent": self.agent_kind}

    def load_state_dict(self, sd):
        """In place into the flat buffers, which the modules' parameters view; then
        _sync_replicas: the modules' pack caches dropped, the targets re-packed and
        data-parallel ranks aligned (a collective with a process group).  ValueError
        naming the field when the parameter counts, the precision, the targets
        (q_lambda) or the optimiser differ; a state saved before the last three
        existed holds their defaults.  Likewise `noisy` (a state saved before it
        existed is a plain agent's), and with a noisy agent `noise_seed`; and `mixer`, the
        kind of mixer (a state saved before it existed is a transformer mixer's); and
        `agent`, the kind of agent (a state saved before it existed is a transformer agent's)."""
        sd = {"q_lambda": False, "optimizer": "adam", "optim_alpha": 0.99, "noisy": False, "noise_seed": 0,
              "mixer": "transformer", "agent": "transformer", **sd}
        sd["optim_alpha"] = float(sd["optim_alpha"])
        # (noisy before na: a noisy state in a plain learner is told by its name, not by its size)
        head = {"noisy": self.noisy, **({"noise_seed": self.noise_seed} if self.noisy else {})}
        check_fields("TDLearner", sd, {"format": 1, "agent": self.agent_kind, "mixer": self.mixer_kind, **head, "na": self.na, "nm": self.nm, "precision": self.precision,
                                       "q_lambda": self.q_lambda, "optimizer": self.optimizer,
                                       "optim_alpha": self.alpha})
        with torch.no_grad():
            for name in ("params", "target_params", "exp_avg", "exp_avg_sq"):
                copy_checked("TDLearner", name, getattr(self, name), sd[name])
        self.step_count = int(sd["step_count"])
        self.last_target_update_episode = int(sd["last_target_update_episode"])
        self.log_stats_t = int(sd["log_stats_t"])
        self._sync_replicas()

    def _sync_replicas(self):
        """Data parallel: rank 0's params, target params, Adam moments and step
        count on every rank (after a checkpoint load), then re-pack the targets."""
        if self._world() > 1:
            step = torch.tensor([float(self.step_count)], device=self.device)
            broadcast_state([self.params, self.target_params, self.exp_avg, self.exp_avg_sq, step], self.pg)
            self.step_count = int(step.item())
        self._params_written()
        self._pack_targets()

    # -- the TD update -------------------------------------------------------
    def _pipelined(self, B):
        """Run the update's recurrences in step ranges on two streams?  Only where the
        mixer runs decoupled (a multi-tile mixer at a small batch, t2o_mixer_split)
        and the agent BPTT is the pipelined kernel (depth 2), which take ranges."""
        if self.mixer_kind != "transformer":
            return False  # (the QMIX / VDN mixers run the sequential update)
        if self.pipeline is False or self.contract == "pair" or self.sa.D != 2 or self.sa.generic or self.sm.generic:
            return False
        lib = ops.lib()
        if int(lib.t2o_agent_bwd_ranges(ops.ctypes.byref(self.sa.layout()), 1)) != 1:
            return False  # (e.g. T2O_AGENT_BWD=single: the one-wave BPTT takes only the whole unroll)
        return int(lib.t2o_mixer_split(ops.ctypes.byref(self.sm.layout()), int(B))) == 1

    def _ranges(self, n):
        """pipeline_ranges step ranges covering [0, n), in order."""
        k = min(self.pipeline_ranges, n)
        cuts = [round(i * n / k) for i in range(k + 1)]
        return [(cuts[i], cuts[i + 1]) for i in range(k) if cuts[i] < cuts[i + 1]]

    def train(self, batch, t_env=0, episode_num=0, per_weight=None):
        if "obs" in _keys(batch):
            obs = batch["obs"]
        else:  # compact wire-format batch: dense obs rebuilt on the device
            wire = batch["obs_wire"]
            b, T1, A = wire.shape[:3]
            obs = ops.obs_expand(wire, batch["obs_nrm_n"], batch["obs_nrm"],
                                 out=self._buf("obs", (b, T1, A, 9 * A)))
        # the mixer's tokens: the state (state_entity_mode) or every agent's obs
        # entities (n_transf_mixer.py:60-63)
        state = batch["state"] if self.mixer.custom_space else obs.flatten(2)
        actions = batch["actions"]
        avail = batch["avail_actions"]
        B, T1, A, _ = obs.shape
        T = T1 - 1
        dev = self.device
        if avail.dtype != torch.int32:
            avail = avail.int()
        act = actions[..., 0] if actions.dim() == 4 else actions
        if act.dtype != torch.int64:
            act = act.long()
        if act.stride(2) != 1:
            act = act.contiguous()
        reward = batch["reward"][:, :, 0]
        term = batch["terminated"][:, :, 0]  # uint8 / int64 as the EpisodeBatch keeps them: read in place
        filled = batch["filled"][:, :, 0] if "filled" in _keys(batch) else None
        w = None
        if per_weight is not None:
            w = torch.as_tensor(np.asarray(per_weight) if not torch.is_tensor(per_weight) else per_weight,
                                dtype=torch.float32).to(dev).reshape(B).contiguous()

        if self.mixer_kind != "transformer":
            return self._train_flat_mixer(obs, state, act, avail, reward, term, filled, w, t_env, episode_num)
        # the gradient buffer is cleared on the side stream, off the critical path
        # (after the previous update's Adam, which read it)
        main = torch.cuda.current_stream(dev)
        side = self._side_stream() if self.overlap else main
        side.wait_stream(main)
        with torch.cuda.stream(side):
            if self.noisy:  # both networks' ε, beside the packs (main waits before the first head launch)
                eps_on, eps_tg = self._draw_noise(T1)
                noise_drawn = side.record_event()
            self.grad.zero_()
            ops.pack_params(self.sm, self.params[self.na:], self.pack_m)  # beside the agent's pack + forward
            mixer_packed = side.record_event()  # (main waits for it before the mixer: grad is clear by then too)
        ops.pack_params(self.sa, self.params[:self.na_net], self.pack_a)
        hmid = self._buf("hmid", (B, T1, self.sa.D - 1, A, self.sa.E)) if self.sa.D > 1 else None
        piped = self._pipelined(B) and side is not main
        if self.pipeline is True and not piped:
            raise RuntimeError(f"pipeline=True, but this update cannot run in step ranges (layout instance "
                               f"{self.sa.instance}/{self.sm.instance}, {B} episodes: the mixer must run decoupled "
                               f"and the agent BPTT must be the pipelined kernel)")
        mixer_kw = dict(qmode_on=1, actions=act, avail=avail, T_on=T, pack_tg=self.pack_mt, qmode_tg=2, T_tg=T1,
                        timer=self.timer)
        if piped:
            # 1+2 in step ranges: agent range k (main) || mixer recurrence range k-1
            # (side), then every (episode, step)'s mixer rows (side)
            E = self.sa.E
            q_on, q_tg = (self._buf(k, (B, T1, A, self.sa.NA)) for k in ("q_on", "q_tg"))
            h_on, h_tg = (self._buf(k, (B, T1, A, E)) for k in ("h_on", "h_tg"))
            o_on, o_tg = ({"y": self._buf("y" + n, (B, Tn)), "hw": self._buf("hw" + n, (B, Tn, 3, E)),
                           "qv": self._buf("qv" + n, (B, Tn, A)), "xout": self._buf("xo" + n, (B, Tn, A + 3, E)),
                           "xmid": (self._buf("xm" + n, (B, Tn, self.sm.D - 1, A + 3, E)) if n == "on" else None)}
                          for n, Tn in (("on", T), ("tg", T1)))
            # (launchers: each wrapper's arguments converted once, then one C call per
            # range — the host must stay ahead of ranges of ~0.1 ms)
            agent_go = ops.agent_unroll_fwd(self.sa, self.pack_a, obs, pack_tg=self.pack_at, timer=self.timer,
                                            hmid_on=hmid, outs=(q_on, h_on, q_tg, h_tg), launcher=True)
            mixer_go = ops.mixer_unroll_fwd(self.sm, self.pack_m, state, h_on, q_on=q_on, hid_tg=h_tg, q_tg=q_tg,
                                            outs=(o_on, o_tg), launcher=True, **mixer_kw)
            if self.noisy:
                main.wait_event(noise_drawn)
                heads_go = self._head_fwd(q_on, h_on, q_tg, h_tg, eps_on, eps_tg, launcher=True)
            for t0, t1 in self._ranges(T1):
                agent_go(t0, t1)
                if self.noisy:  # the range's q from its h, before the mixer may read them
                    heads_go(t0, t1)
                agent_done = main.record_event()
                with torch.cuda.stream(side):
                    side.wait_event(agent_done)
                    mixer_go(1, t0, t1)
            with torch.cuda.stream(side):
                mixer_go(2)
            if self.q_lambda:
                # main has run the last agent range and is idle while the side stream
                # finishes the mixers: the taken mix goes here, beside them
                o_tk = self._taken_mix(state, h_tg, q_tg, act, B, T)
            main.wait_stream(side)
        else:
            # 1. agents: online + target over t = 0..T
            q_on, h_on, q_tg, h_tg = ops.agent_unroll_fwd(self.sa, self.pack_a, obs, pack_tg=self.pack_at,
                                                          timer=self.timer, hmid_on=hmid)
            if self.noisy:  # the noisy head's q over the fused (mean-head) q, both networks
                main.wait_event(noise_drawn)
                self._head_fwd(q_on, h_on, q_tg, h_tg, eps_on, eps_tg)
            # 2. mixers: online on chosen Q (t < T), target on double-Q (t <= T)
            main.wait_event(mixer_packed)
            o_on, o_tg = ops.mixer_unroll_fwd(self.sm, self.pack_m, state, h_on, q_on=q_on, hid_tg=h_tg, q_tg=q_tg,
                                              **mixer_kw)
            if self.q_lambda:
                # the taken mix after them on this stream: at a batch that fills the chip
                # a second stream buys nothing (measured)
                o_tk = self._taken_mix(state, h_tg, q_tg, act, B, T)
        # 3. TD(λ) targets / loss (un-normalised: Σ mask is applied in Adam so the
        #    data-parallel sum over ranks divides by the GLOBAL Σ mask)
        #    (Σ mask also lands in grad[-1] straight from the kernel: grad was cleared
        #    on the side stream before the mixer forward, which waited for it)
        td_kw = dict(gamma=self.gamma, td_lambda=self.td_lambda, mask_sum=1.0, algo=self.td_algo,
                     mask_sum_acc=self.grad[-1:])
        if self.q_lambda:
            # Peng's Q(λ): Qtot_tgt_t - Qtot_taken_t corrects every step's reward (the taken
            # mix ran on this stream, the target mix on it or on the side stream joined above)
            td = ops.td_qlambda(o_on["y"], o_tg["y"], o_tk["y"], reward, term, filled, w, **td_kw)
            # (o_tk, and the pipelined path's o_tg: buffers the next update reuses)
            td["qtot_taken"], td["qtot_tgt"] = o_tk["y"].clone(), o_tg["y"].clone() if piped else o_tg["y"]
        else:
            td = ops.td_loss(o_on["y"], o_tg["y"], reward, term, filled, w, **td_kw)
        # 4. mixer BPTT (its weight-grad tape is contracted after the agent BPTT)
        tape_m = self._slab("tape_m", ops.tape_floats(self.sm, ops.mixer_tape_tiles(B, T, A, self.sm)))
        tape_a = self._slab("tape_a", ops.tape_floats(self.sa, ops.agent_tape_tiles(B, T, A)))
        slabs_m = self._slab("m", ops.mixer_slab_count(B) * self.sm.layout().grad_total)
        nwork = ops.mixer_work_floats(self.sm, B, T)
        work_m = self._slab("work_m", nwork) if nwork else None
        slabs_a = self._slab("a", ops.agent_slab_count(B, A) * self.sa.layout().grad_total)
        if piped:
            # 4+5 in step ranges: the mixer's parallel part, then per range from the
            # last down its recurrence (side) || the agent BPTT of the range after (main)
            gqv, ghid = self._buf("gqv", (B, T, A)), self._buf("ghid", (B, T, A, self.sm.E))
            carry_m, carry_a = self._buf("carry_m", (B, 3, self.sm.E)), self._buf("carry_a", (B * A, self.sa.E))
            mixer_go = ops.mixer_unroll_bwd(self.sm, self.pack_m, state, h_on, o_on, td["gq"], slabs=slabs_m,
                                            timer=self.timer, tape=tape_m, work=work_m, outs=(gqv, ghid),
                                            carry=carry_m, launcher=True)
            gh, gchosen, head_go = None if self.detach_mixer_hidden else ghid, gqv, None
            if self.noisy:
                # the head's backward turns each range's dL/dq_chosen (+ dL/dhidden) into the
                # dL/dh the agent BPTT runs on alone
                head_go, gh, gpart = self._head_bwd(gqv, act, h_on, eps_on, gh, launcher=True)
                gchosen = None
            agent_go, _ = ops.agent_unroll_bwd(self.sa, self.pack_a, obs, h_on, gchosen=gchosen, actions=act,
                                               gh=gh, slabs=slabs_a,
                                               timer=self.timer, hmid=hmid, tape=tape_a, gcarry=carry_a,
                                               launcher=True)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                contract_m = mixer_go(1)
            for t_lo, t_hi in reversed(self._ranges(T)):
                with torch.cuda.stream(side):
                    mixer_go(2, t_lo, t_hi)
                    mixer_done = side.record_event()
                main.wait_event(mixer_done)
                if head_go is not None:
                    head_go(t_lo, t_hi)
                contract_a = agent_go(t_lo, t_hi)
            with torch.cuda.stream(side):
                gm = contract_m()
                ops.unpack_grads(self.sm, self.params[self.na:], gm, self.grad[self.na:self.na + self.nm])
                work_m_ = allreduce_async(self.grad[self.na:], self.pg)
            ga = contract_a()
            ops.unpack_grads(self.sa, self.params[:self.na_net], ga, self.grad[:self.na_net])
            if self.noisy:
                self._head_wgrad(gpart, B, A, eps_on)
            work_a = allreduce_async(self.grad[:self.na], self.pg)
            main.wait_stream(side)
            wait_all((work_m_, work_a))
            # (o_on: reused buffers)
            return self._finish(episode_num, td, {"y": o_on["y"].clone()}, t_env, term, filled)
        contract_m, gqv, ghid, _ = ops.mixer_unroll_bwd(self.sm, self.pack_m, state, h_on, o_on, td["gq"],
                                                        slabs=slabs_m, timer=self.timer, tape=tape_m,
                                                        defer_contract=True, work=work_m)
        gh = None if self.detach_mixer_hidden else ghid
        if self.noisy:
            # 4b. the head's backward: dL/dh = dL/dhidden + dL/dq_chosen · W_t[action]; the agent
            #     BPTT then takes no q gradient (its fused head adds zeros to q_basic's slots)
            gh, gpart = self._head_bwd(gqv, act, h_on, eps_on, gh)
            gqv = None
        if self.contract == "pair":
            # 5. agent BPTT (grads of the chosen Q and, unless detached, of the hidden
            #    states), then both tapes contracted in one launch
            contract_a, _ = ops.agent_unroll_bwd(self.sa, self.pack_a, obs, h_on, gchosen=gqv, actions=act, gh=gh,
                                                 slabs=slabs_a, timer=self.timer, hmid=hmid, tape=tape_a,
                                                 defer_contract=True)
            gm, ga = ops.tape_contract_pair(contract_m, contract_a, timer=self.timer)
            # 6. grads in reference parameter order; data parallel: one all-reduce of
            #    [agent grads, mixer grads, Σ mask] (336 KB at the default network)
            ops.unpack_grads(self.sm, self.params[self.na:], gm, self.grad[self.na:self.na + self.nm])
            ops.unpack_grads(self.sa, self.params[:self.na_net], ga, self.grad[:self.na_net])
            if self.noisy:
                self._head_wgrad(gpart, B, A, eps_on)
            wait_all((allreduce_async(self.grad, self.pg),))
        else:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                gm = contract_m()
                ops.unpack_grads(self.sm, self.params[self.na:], gm, self.grad[self.na:self.na + self.nm])
                work_m = allreduce_async(self.grad[self.na:], self.pg)
            ga, _ = ops.agent_unroll_bwd(self.sa, self.pack_a, obs, h_on, gchosen=gqv, actions=act, gh=gh,
                                         slabs=slabs_a, timer=self.timer, hmid=hmid, tape=tape_a)
            ops.unpack_grads(self.sa, self.params[:self.na_net], ga, self.grad[:self.na_net])
            if self.noisy:
                self._head_wgrad(gpart, B, A, eps_on)
            work_a = allreduce_async(self.grad[:self.na], self.pg)
            main.wait_stream(side)
            wait_all((work_m, work_a))
        return self._finish(episode_num, td, o_on, t_env, term, filled)

    def _train_flat_mixer(self, obs, state, act, avail, reward, term, filled, w, t_env, episode_num):
        """train() with a QMIX, VDN or QPLEX mixer (module docstring): the agent unroll, the TD
        loss, the agent BPTT, the optimiser step and the statistics are the transformer
        path's; steps 2 and 4 are the select kernel and the flat mixers' kernels.  The
        mixers read the state alone, so gh is None: no gradient reaches the agents'
        hidden states from them and detach_mixer_hidden has no effect.  With a GRU agent
        (agent.kind "rnn") steps 1 and 5 are its kernels; contract and detach_mixer_hidden
        have no effect on them (no tape to contract, no gradient into the hidden states)."""
        B, T1, A, _ = obs.shape
        T = T1 - 1
        dev = self.device
        vdn, qplex = self.mixer_kind == "vdn", self.mixer_kind == "qplex"
        state = state.reshape(B, T1, -1) if state.dim() != 3 else state
        p_on, p_tg = self.params[self.na:], self.target_params[self.na:]
        main = torch.cuda.current_stream(dev)
        side = self._side_stream() if self.overlap else main
        side.wait_stream(main)
        with torch.cuda.stream(side):
            if self.noisy:
                eps_on, eps_tg = self._draw_noise(T1)
                noise_drawn = side.record_event()
            self.grad.zero_()
            grad_clear = side.record_event()
        rnn = self.agent_kind == "rnn"
        # 1. agents: online + target over t = 0..T
        if rnn:
            H, NA = self.sa.H, self.sa.NA
            fwd = {k: self._buf("rnn_" + k, (B, T1, A, n)) for k, n in
                   (("q_on", NA), ("h_on", H), ("gi_on", 3 * H), ("x_on", H), ("q_tg", NA), ("h_tg", H),
                    ("gi_tg", 3 * H))}
            ops.rnn_agent_fwd(self.sa, self.params[:self.na], obs, actions=act,
                              params_tg=self.target_params[:self.na], outs=fwd, timer=self.timer)
            q_on, h_on, q_tg, h_tg = fwd["q_on"], fwd["h_on"], fwd["q_tg"], fwd["h_tg"]
        else:
            ops.pack_params(self.sa, self.params[:self.na_net], self.pack_a)
            hmid = self._buf("hmid", (B, T1, self.sa.D - 1, A, self.sa.E)) if self.sa.D > 1 else None
            q_on, h_on, q_tg, h_tg = ops.agent_unroll_fwd(self.sa, self.pack_a, obs, pack_tg=self.pack_at,
                                                          timer=self.timer, hmid_on=hmid)
        if self.noisy:
            main.wait_event(noise_drawn)
            self._head_fwd(q_on, h_on, q_tg, h_tg, eps_on, eps_tg)
        # 2. chosen Q (t < T) and double-Q selection (t <= T); VDN's mix is the kernel's row sum
        qv_on, qv_tg = self._buf("qv_on", (B, T, A)), self._buf("qv_tg", (B, T1, A))
        y_on, y_tg = torch.empty(B, T, device=dev), torch.empty(B, T1, device=dev)
        if qplex:
            # ... and each network's avail-masked maximum of its own Q and the action used (int32)
            sel_on = (qv_on, self._buf("qm_on", (B, T, A)), self._buf("u_on", (B, T, A)).view(torch.int32))
            sel_tg = (qv_tg, self._buf("qm_tg", (B, T1, A)), self._buf("u_tg", (B, T1, A)).view(torch.int32))
            ops.qplex_select(q_on, qmode_on=1, actions=act, avail=avail, T_on=T, q_tg=q_tg, qmode_tg=2, T_tg=T1,
                             outs=(sel_on, sel_tg), timer=self.timer)
            ops.qplex_fwd(self.sm, p_on, state, *sel_on, params_tg=p_tg, qv_tg=sel_tg[0], qmax_tg=sel_tg[1],
                          act_tg=sel_tg[2], parts=3, outs=(y_on, y_tg), timer=self.timer)
            self.last_qmax = (sel_on[1], sel_tg[1])  # (buffers the next update reuses, as last_qv)
        else:
            ops.q_select(q_on, qmode_on=1, actions=act, avail=avail, T_on=T, q_tg=q_tg, qmode_tg=2, T_tg=T1,
                         outs=((qv_on, y_on if vdn else None), (qv_tg, y_tg if vdn else None)), timer=self.timer)
        if not vdn and not qplex:
            ops.qmix_fwd(self.sm, p_on, state, qv_on, params_tg=p_tg, qv_tg=qv_tg, outs=(y_on, y_tg), timer=self.timer)
        self.last_qv = (qv_on, qv_tg)  # what the mixers read (buffers the next update reuses)
        if self.q_lambda:  # the target mixer on the target Q at the batch's actions, t < T
            qv_tk, y_tk = self._buf("qv_tk", (B, T, A)), torch.empty(B, T, device=dev)
            if qplex:  # ... with the target network's own maxima
                sel_tk = (qv_tk, self._buf("qm_tk", (B, T, A)), self._buf("u_tk", (B, T, A)).view(torch.int32))
                ops.qplex_select(q_tg, qmode_on=1, actions=act, avail=avail, T_on=T, outs=sel_tk, timer=self.timer)
                ops.qplex_fwd(self.sm, p_tg, state, *sel_tk, parts=3, outs=y_tk, timer=self.timer)
            else:
                ops.q_select(q_tg, qmode_on=1, actions=act, T_on=T, outs=(qv_tk, y_tk if vdn else None),
                             timer=self.timer)
            if not vdn and not qplex:
                ops.qmix_fwd(self.sm, p_tg, state, qv_tk, outs=y_tk, timer=self.timer)
        # 3. TD(λ) / Q(λ) targets and the loss (Σ mask lands in grad[-1], cleared on the side stream)
        main.wait_event(grad_clear)
        td_kw = dict(gamma=self.gamma, td_lambda=self.td_lambda, mask_sum=1.0, algo=self.td_algo,
                     mask_sum_acc=self.grad[-1:])
        if self.q_lambda:
            td = ops.td_qlambda(y_on, y_tg, y_tk, reward, term, filled, w, **td_kw)
            td["qtot_taken"], td["qtot_tgt"] = y_tk, y_tg
        else:
            td = ops.td_loss(y_on, y_tg, reward, term, filled, w, **td_kw)
        # 4. the mixer's backward: dL/dq_chosen now, its weight gradients beside the agent BPTT
        gqv = self._buf("gqv", (B, T, A))
        mixer_dw = None
        if vdn:
            ops.vdn_bwd(td["gq"], gqv=gqv, timer=self.timer)
        elif qplex:
            slabs = self._slab("qplex", ops.qplex_slab_count(B, T) * self.nm)
            work = self._slab("qplex_work", ops.qplex_work_floats(self.sm, B, T))
            mixer_dw, _, _, nslab = ops.qplex_bwd(self.sm, p_on, state, *sel_on, td["gq"], parts=3, gqv=gqv,
                                                  slabs=slabs, work=work, timer=self.timer, launcher=True)
            mixer_dw(1)
        else:
            slabs = self._slab("qmix", ops.qmix_slab_count(B, T) * self.nm)
            work = self._slab("qmix_work", ops.qmix_work_floats(self.sm, B, T))
            mixer_dw, _, _, nslab = ops.qmix_bwd(self.sm, p_on, state, qv_on, td["gq"], gqv=gqv, slabs=slabs,
                                                 work=work, timer=self.timer, launcher=True)
            mixer_dw(1)
        gh, gchosen = None, gqv
        if self.noisy:  # dL/dh = dL/dq_chosen · W_t[action]; the agent BPTT then takes no q gradient
            gh, gpart = self._head_bwd(gqv, act, h_on, eps_on, None)
            gchosen = None
        if rnn:
            slabs_a = self._slab("rnn", ops.rnn_slab_count(B, T, A) * self.na)
            work_a_ = self._slab("rnn_work", ops.rnn_work_floats(self.sa, B, T))
        else:
            tape_a = self._slab("tape_a", ops.tape_floats(self.sa, ops.agent_tape_tiles(B, T, A)))
            slabs_a = self._slab("a", ops.agent_slab_count(B, A) * self.sa.layout().grad_total)

        def mixer_grads():
            if mixer_dw is not None:
                mixer_dw(2)
                ops.reduce_slabs(slabs, nslab, self.grad[self.na:self.na + self.nm])

        def agent_grads():
            # 5. agent BPTT, its gradients in the reference parameter order
            if rnn:
                _, nslab_a, _ = ops.rnn_agent_bwd(self.sa, self.params[:self.na], obs, fwd, T=T, actions=act,
                                                  gchosen=gchosen, slabs=slabs_a, work=work_a_, timer=self.timer)
                ops.reduce_slabs(slabs_a, nslab_a, self.grad[:self.na])
                return
            ga, _ = ops.agent_unroll_bwd(self.sa, self.pack_a, obs, h_on, gchosen=gchosen, actions=act, gh=gh,
                                         slabs=slabs_a, timer=self.timer, hmid=hmid, tape=tape_a)
            ops.unpack_grads(self.sa, self.params[:self.na_net], ga, self.grad[:self.na_net])
            if self.noisy:
                self._head_wgrad(gpart, B, A, eps_on)
        if self.contract == "pair":  # everything on this stream, one all-reduce
            agent_grads()
            mixer_grads()
            wait_all((allreduce_async(self.grad, self.pg),))
        else:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                mixer_grads()
                work_m = allreduce_async(self.grad[self.na:], self.pg)  # (vdn: Σ mask alone)
            agent_grads()
            work_a = allreduce_async(self.grad[:self.na], self.pg)
            main.wait_stream(side)
            wait_all((work_m, work_a))
        return self._finish(episode_num, td, {"y": y_on}, t_env, term, filled)

    def _taken_mix(self, state, h_tg, q_tg, act, B, T):
        """q_lambda: the target mixer once more, on the target Q at the batch's actions
        (t < T; qmode 1 from q_tg, the target agents' hidden states) — a one-network
        t2o_mixer_unroll_fwd, whole, on the current stream, which must be ordered after
        the target agent unroll.  Into buffers the learner keeps (allocated once and
        reused every update, like the pipelined update's other forward buffers)."""
        A, E = self.sm.agents, self.sm.E
        o_tk = {"y": self._buf("ytk", (B, T)), "hw": self._buf("hwtk", (B, T, 3, E)),
                "qv": self._buf("qvtk", (B, T, A)), "xout": self._buf("xotk", (B, T, A + 3, E)), "xmid": None}
        return ops.mixer_unroll_fwd(self.sm, self.pack_mt, state, h_tg, qmode_on=1, q_on=q_tg, actions=act, T_on=T,
                                    timer=self.timer, outs=(o_tk, None))

    def _head_fwd(self, q_on, h_on, q_tg, h_tg, eps_on, eps_tg, launcher=False):
        """The noisy head of both networks on the current stream: q_on / q_tg overwritten
        from h_on / h_tg (one launch per network).  launcher: go(t0, t1) per step range."""
        gos = []
        for q, h, eps, flat in ((q_on, h_on, eps_on, self.params), (q_tg, h_tg, eps_tg, self.target_params)):
            u_w, u_b, s_w, s_b = self._head_views(flat)
            gos.append(ops.noisy_head_fwd(h, q, u_w, u_b, s_w, s_b, eps=eps, timer=self.timer, launcher=True))

        def go(t0, t1):
            for g in gos:
                g(t0, t1)
        if launcher:
            return go
        go(0, q_on.shape[1])

    def _head_bwd(self, gqv, act, h_on, eps_on, gh_in, launcher=False):
        """The online head's backward (t2o_noisy_head_bwd) into buffers the learner keeps:
        returns (gh_out [B, T, A, E], gpart), with launcher first go(t_lo, t_hi)."""
        B, T, A = gqv.shape
        u_w, _, s_w, _ = self._head_views(self.params)
        gh_out = self._buf("gh_head", (B, T, A, self.sa.E))
        gpart = self._buf("gpart_head", (T, ops.noisy_head_parts(B, A), self.sa.NA, self.sa.E + 1))
        out = ops.noisy_head_bwd(gqv, act, h_on, u_w, s_w, eps_on[0], gh_in=gh_in, gh_out=gh_out, gpart=gpart,
                                 timer=self.timer, launcher=launcher)
        return out

    def _head_wgrad(self, gpart, B, A, eps_on):
        """Σ_t of the head's partials into its four slots of the flat gradient (+=, after
        t2o_unpack_grads left zeros in q_basic's slots)."""
        du_w, du_b, ds_w, ds_b = self._head_views(self.grad)
        ops.noisy_head_wgrad(gpart, B, A, du_w, du_b, ds_w, ds_b, eps=eps_on, timer=self.timer)

    def _log_stats(self, t_env, td, qtot, term, filled):
        """The NQLearner log values, when one is due: one library launch (the masked
        fp64 sums of |td|, Qtot and the targets, t2o_td_stats) beside two small copies
        that gather the loss, Σ mask and the gradient norm, with a process group one
        all-reduce (the sums become the global ones), then ONE host read of seven
        doubles."""
        st = self._stat
        st[:2].copy_(td["loss"])  # Σ_b w_b Σ_t ½ td² m (un-normalised), local Σ mask
        ops.td_stats(qtot, td["targets"], term, filled, out=st[2:])
        if self._world() > 1:
            dist.all_reduce(st, op=dist.ReduceOp.SUM, group=self.pg)
        loss_sum, mask_sum, m, abs_sum, q_sum, tgt_sum, grad_norm = torch.cat([st, self.grad_norm.double()]).tolist()
        # (the mixer kind's own field: the transformer / QMIX shape's agents, VDN's from the agent network)
        n_agents = self.sm.agents if self.sm is not None else self.agent.n_agents
        log = self.logger.log_stat
        log("loss_td", loss_sum / mask_sum, t_env)
        log("grad_norm", grad_norm, t_env)
        log("td_error_abs", abs_sum / m, t_env)
        log("q_taken_mean", q_sum / (m * n_agents), t_env)
        log("target_mean", tgt_sum / (m * n_agents), t_env)
        self.log_stats_t = t_env

    def _finish(self, episode_num, td, o_on, t_env=0, term=None, filled=None):
        # 7. clip + Adam (or RMSprop)
        self.step_count += 1
        opt_kw = dict(lr=self.lr, eps=self.eps, weight_decay=self.wd, max_grad_norm=self.clip, workspace=self.adam_ws,
                      grad_div=self.grad[-1:], grad_norm_out=self.grad_norm)
        if self.optimizer == "rmsprop":
            ops.rmsprop_step(self.params, self.grad[:-1], self.exp_avg_sq, alpha=self.alpha, **opt_kw)
        else:
            ops.adam_step(self.params, self.grad[:-1], self.exp_avg, self.exp_avg_sq, self.step_count,
                          betas=self.betas, **opt_kw)
        self._params_written()
        if self.logger is not None and t_env - self.log_stats_t >= self.learner_log_interval:
            self._log_stats(t_env, td, o_on["y"], term, filled)
        if (episode_num - self.last_target_update_episode) / self.target_update_interval >= 1.0:
            self.update_targets()
            self.last_target_update_episode = episode_num
        prio = td["prio"]
        info = {"td_errors_abs": prio.cpu() if self.priorities_to_cpu else prio,
                "loss_sum": td["loss"][0:1], "mask_sum": td["loss"][1:2], "grad_norm": self.grad_norm,
                "qtot": o_on["y"], "targets": td["targets"]}
        if self.q_lambda:  # what t2o_td_qlambda read: [B, T] and the target mix [B, T+1]
            info["qtot_taken"], info["qtot_tgt"] = td["qtot_taken"], td["qtot_tgt"]
        return info


def _keys(batch):
    try:
        return batch.keys()
    except AttributeError:
        return getattr(batch, "scheme", {}).keys()
