"""Closed-loop rollout on the device: VecEnv -> agent step -> ε-greedy -> VecEnv.

Batched replacement of parallel_runner.ParallelRunner.run
(parallel_runner.py:102-188) and of the absent controller's
``select_actions`` (:121), SURVEY.md §8 f2 / BASELINE configs[4].  Where the
reference steps one env per process and round-trips actions through the host
every timestep (:122, Pipe send/recv :131-170), here every env of the shard
steps in one launch, the agent forward and the action selection run on the
device, and each timestep's obs / state / avail are written by the env kernel
straight into the replay batch — nothing synchronises with the host until the
caller reads the batch.

The episode batch follows the reference's EpisodeBatch scheme (per_run.py:119-130)
and timestep bookkeeping exactly:
  * slot t holds the pre-transition data (state, avail_actions, obs) for t = 0..T
    and the actions selected from it (t = 0..T: the runner also selects at the
    final slot, :121 before the all-terminated break);
  * reward / terminated at t = 0..T-1; ``terminated`` is the env's flag unless the
    termination is the episode limit (:167-170), which for this env is always —
    so it stays 0 (environment_multi_mec.py:354-356);
  * filled = 1 on slots 0..T (mark_filled on the pre-transition update, :185).
Buffers are allocated time-major [T+1, n, ...] so each step's slice is dense for
the env kernel; the batch dict holds the [n, T+1, ...] views the learner takes
(its kernels accept any episode / timestep strides).

ε schedule: PyMARL's DecayThenFlatSchedule (linear), evaluated per rollout at
t_env as the reference's selector does; test_mode selects greedily.

A NoisyNet agent (modules.TransformerAgent with action_selector "noisy-new",
``agent.noisy``): a non-test run draws the episode's noise once
(t2o_noise_normal: kind "runner", this runner's seed, counter = ``episode``) and
applies the noisy head to each step's h before select_actions (one more launch per
step, t2o_noisy_head_fwd); the ε schedule still applies as configured.  test_mode
runs the mean head, which is the fused step: no new launch.

A GRU agent (modules.RNNAgent, ``agent.kind`` "rnn") steps on its own
kernels (t2o_rnn_fwd with one step, two launches, no pack): it takes the env's
observation in either mode (entity [A, 9A] or flat [A, 6]; its input width is checked
against the env), and the kernels add the one-hots of the previous step's actions (zeros
at t = 0) and of the agent index as the agent's flags ask.  The replay batch is the same.

compact_obs=True (the env must be a VecEnv(wire=True)): the
batch carries the observation wire format instead of the dense obs —
``obs_wire`` [n, T+1, A, 4] int32 plus the per-episode normaliser snapshot
``obs_nrm_n`` [n] / ``obs_nrm`` [n, 2, 9A] — and each step's dense obs goes only
to a one-step scratch buffer the agent reads.  ``ops.obs_expand`` (called by
TDLearner.train when the batch has no ``obs``) rebuilds the dense obs exactly.

Statistics (parallel_runner.py:193-231; off by default): with a ``logger`` (or
``collect_stats=True``) every run ends with ONE more launch, ``ops.episode_stats``,
which adds the run's returns and the terminated envs' info values to a device
accumulator of its mode (train / test) — no host read.  When the reference's
schedule (:212-219) says a log is due, ``_log`` reads that accumulator once,
logs the means under the reference's keys and clears it.
"""
import dataclasses

import torch
import torch.distributed as dist

from . import ops
from ._lib import EP_STATS
from .distributed import rank as dist_rank, rank_seed, world_size
from .env import INFO_KEYS
from .episode_batch import DeviceEpisodeBatch
from .state import check_fields, copy_checked

# what accumulator slots 2.. sum (include/t2omca.h t2o_episode_stats): the keys of the
# terminated step's info dict (environment_multi_mec.py:340-363), logged as key + "_mean"
STAT_KEYS = ("reward",) + INFO_KEYS[:4] + ("episode_limit",) + INFO_KEYS[4:]
assert len(STAT_KEYS) == EP_STATS - 2
# the columns of evaluate(per_episode=True)'s rows
EPISODE_INFO_KEYS = ("return",) + STAT_KEYS


class LinearSchedule:
    """DecayThenFlatSchedule(start, finish, time_length, decay="linear")."""

    def __init__(self, start=1.0, finish=0.05, time_length=50000):
        self.start, self.finish, self.time_length = float(start), float(finish), max(1, int(time_length))
        self.delta = (self.start - self.finish) / self.time_length

    def eval(self, t):
        return max(self.finish, self.start - self.delta * t)


class RolloutRunner:
    def __init__(self, agent, env, *, epsilon_start=1.0, epsilon_finish=0.05, epsilon_anneal_time=50000,
                 seed=None, compact_obs=False, precision="fp32", logger=None, test_nepisode=None,
                 runner_log_interval=2000, collect_stats=None, process_group=None):
        """logger: an object with ``log_stat(key, value, t)`` (statlog.StatsLogger); with
        one, or with collect_stats=True, the runner keeps the reference's run statistics
        (module docstring) and logs them on its schedule: test statistics once
        max(1, test_nepisode // n) test runs are accumulated (test_nepisode None: one
        run), otherwise every runner_log_interval env steps.  process_group: the means
        logged are those over every rank's episodes (one SUM all-reduce of the
        accumulator before it is read); every rank must then run the same number of
        envs and the same episode limit, and call run() / train_stats / test_stats in
        the same order, since whether a log is due is decided from host counters that
        are equal only then.

        precision: the agent step's MFMA operands — "fp32" (the reference's
        precision, default) or "bf16" (bf16 weight / activation operands, fp32
        accumulation, LayerNorm, softmax and recurrent state, as the learner's bf16
        mode; greedy actions can differ from fp32's where two Q values are within
        bf16 rounding)."""
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', not {precision!r}")
        # seed (None = 0) mixed with the data-parallel rank (distributed.rank_seed)
        # the data-parallel rank is always mixed in (rank 0 keeps `seed`), so ranks given
        # the same explicit seed still draw different streams
        seed = rank_seed(0 if seed is None else seed, dist_rank())
        self.rnn = getattr(agent, "kind", "transformer") == "rnn"
        entity = bool(getattr(env, "obs_entity_mode", True))
        if not entity and not self.rnn:
            raise ValueError("the transformer agent reads entity observations (VecEnv obs_entity_mode=True)")
        if compact_obs and getattr(env, "wire", None) is None:
            raise ValueError("compact_obs needs a VecEnv built with wire=True")
        self.compact_obs = bool(compact_obs)
        self.n_obs = 9 * env.A if entity else 6
        if env.A != (agent.shape.A if self.rnn else agent.shape.n_ent) or env.n_actions != agent.shape.NA:
            raise ValueError("agent and env disagree on agents / actions")
        if self.rnn and agent.shape.OBS != self.n_obs:
            sh = agent.shape
            raise ValueError(f"the rnn agent's input is {sh.IN} wide ({sh.OBS} of it the observation), the env's "
                             f"observation is {self.n_obs} wide: with its flags the agent's input_shape must be "
                             f"{self.n_obs + sh.IN - sh.OBS}")
        self.agent, self.env = agent, env
        # a NoisyNet head (modules.TransformerAgent, action_selector "noisy-new"): non-test
        # runs explore through it (noise kind "runner", seed = this runner's, counter =
        # episode), under the ε schedule as configured; test runs use the mean head
        self.noisy = bool(getattr(agent, "noisy", False))
        self.precision = precision
        # (the GRU agent's kernels are fp32 in both precisions)
        self.shape = dataclasses.replace(agent.shape, prec=1) if precision == "bf16" and not self.rnn else agent.shape
        self.n, self.T, self.A, self.NA = env.n_envs, env.T, env.A, env.n_actions
        self.device = env.device
        self.schedule = LinearSchedule(epsilon_start, epsilon_finish, epsilon_anneal_time)
        self.seed = int(seed)
        self.t_env = 0
        self.episode = 0
        self._bufs = None
        self.last_returns = None
        # optional callable(tag) recording HIP events around the step's three launches
        # (agent step, action selection, env step) on every timer_every-th timestep
        self.timer = None
        self.timer_every = 10
        # statistics (parallel_runner.py:48-55, 193-231)
        self.logger = logger
        self.collect_stats = bool(collect_stats) or logger is not None
        self.batch_size = self.n
        self.test_nepisode = self.n if test_nepisode is None else int(test_nepisode)
        self.runner_log_interval = runner_log_interval
        self.log_train_stats_t = -100000
        self.pg = process_group
        self._acc = None  # [2][EP_STATS] fp64 on the device: train, test
        self._n_acc = [0, 0]  # episodes in each accumulator (host: the schedule never synchronises)
        if self.collect_stats:
            self._acc = torch.zeros(2, EP_STATS, dtype=torch.float64, device=self.device)

    # -- replay batch ---------------------------------------------------------
    def _alloc(self):
        n, T1, A, NA, dev = self.n, self.T + 1, self.A, self.NA, self.device
        if self.compact_obs:
            obs = dict(obs_wire=torch.empty(T1, n, A, 4, dtype=torch.int32, device=dev))
            self._obs_step = torch.empty(n, A, 9 * A, device=dev)
        else:
            obs = dict(obs=torch.empty(T1, n, A, self.n_obs, device=dev))
        return dict(
            **obs,
            state=torch.empty(T1, n, 8 * A, device=dev),
            avail_actions=torch.empty(T1, n, A, NA, dtype=torch.int32, device=dev),
            actions=torch.zeros(T1, n, A, 1, dtype=torch.int64, device=dev),
            reward=torch.zeros(T1, n, 1, device=dev),
            terminated=torch.zeros(T1, n, 1, dtype=torch.uint8, device=dev),
            filled=torch.ones(T1, n, 1, dtype=torch.int64, device=dev),
        )

    def run(self, test_mode=False, new_buffers=True):
        """One episode of every env; returns the episode batch ([n, T+1, ...] device
        views as a DeviceEpisodeBatch, like ParallelRunner.run's EpisodeBatch,
        parallel_runner.py:221); the per-env episode returns [n] (fp64, on the
        device) are in self.last_returns."""
        if self._bufs is None or new_buffers:
            self._bufs = self._alloc()
        tm = self._bufs
        env, shape = self.env, self.shape
        flat = torch.cat([p.detach().reshape(-1) for p in self.agent.parameters()])
        if self.rnn:  # (no pack; two sets of step outputs, so that a step never writes the h it reads)
            step_outs = [{k: torch.empty(self.n, 1, self.A, w, device=self.device)
                          for k, w in (("q_on", shape.NA), ("h_on", shape.H), ("gi_on", 3 * shape.H))} for _ in (0, 1)]
        else:
            pack = ops.pack_params(shape, flat[:shape.n_params])  # (a noisy agent's sigmas follow the plain prefix)
        eps = 0.0 if test_mode else self.schedule.eval(self.t_env)
        noise = head = None
        if self.noisy and not test_mode:
            # the episode's ε, once: step t's slice serves that step's one forward call
            nl = self.agent.q_basic
            head = [p.detach().contiguous() for p in (nl.u_w, nl.u_b, nl.s_w, nl.s_b)]
            noise = ops.noise_normal(shape.E, shape.NA, self.T + 1, self.seed, "runner", self.episode,
                                     device=self.device)
        env.reset(dest=self._dest(tm, 0))
        ret = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        h = None
        for t in range(self.T + 1):
            timer = self.timer if self.timer is not None and t % self.timer_every == 0 else None
            mark = timer or (lambda tag: None)
            obs_t = self._obs_step if self.compact_obs else tm["obs"][t]
            if self.rnn:
                prev = tm["actions"][t - 1, :, :, 0].unsqueeze(1) if t > 0 and shape.last_action else None
                out = ops.rnn_agent_fwd(shape, flat, obs_t.unsqueeze(1), actions=prev, act_shift=1, h0_on=h,
                                        outs=step_outs[t % 2], want_x=False, timer=timer)
                q, h = out["q_on"], out["h_on"][:, 0]
            else:
                q, h_seq = ops.agent_unroll_fwd(shape, pack, obs_t.unsqueeze(1), h0_on=h, timer=timer)
                h = h_seq.view(self.n * self.A, shape.E)
            if noise is not None:  # the noisy head's q over the fused step's mean-head q
                ops.noisy_head_fwd(h_seq, q, *head, eps=(noise[0][t:t + 1], noise[1][t:t + 1]), timer=timer)
            counter = (self.episode * (self.T + 1) + t)
            mark("begin:select_actions")
            ops.select_actions(q[:, 0], tm["avail_actions"][t], eps, self.seed, counter,
                               out=tm["actions"][t, :, :, 0])
            mark("end:select_actions")
            if t == self.T:
                break
            mark("begin:env_step")
            reward, _, _, _, _, _ = env.step(tm["actions"][t, :, :, 0], dest=self._dest(tm, t + 1))
            mark("end:env_step")
            tm["reward"][t, :, 0].copy_(reward)
            ret += reward
        if not test_mode:
            self.t_env += self.n * self.T
        self.episode += 1
        batch = {k: v.transpose(0, 1) for k, v in tm.items()}
        if self.compact_obs:  # per-episode: the normaliser each episode's obs start from
            batch["obs_nrm_n"] = env.snap_n.clone()
            batch["obs_nrm"] = env.snap.clone()
        self.last_returns = ret
        if self.collect_stats:
            self._run_stats(bool(test_mode), ret, eps)
        return DeviceEpisodeBatch(batch)

    # -- statistics -----------------------------------------------------------------
    def _run_stats(self, test_mode, ret, eps):
        """The end of ParallelRunner.run (:202-219): this run into its mode's
        accumulator (one launch), then the log schedule."""
        env = self.env
        ops.episode_stats(env.reward, env.info, env.terminated, ret, self._acc[int(test_mode)])
        self._n_acc[int(test_mode)] += self.n
        if self.logger is None:
            return
        n_test_runs = max(1, self.test_nepisode // self.n) * self.n
        if test_mode and self._n_acc[1] == n_test_runs:
            self._log(test_mode)
        elif self.t_env - self.log_train_stats_t >= self.runner_log_interval:
            self._log(test_mode)
            self.logger.log_stat("epsilon", eps, self.t_env)
            self.log_train_stats_t = self.t_env

    def _sums(self, mode):
        """The accumulator of a mode on the host (over every rank with a process
        group): the one synchronising read of the statistics."""
        acc = self._acc[int(mode)]
        if world_size(self.pg) > 1:
            acc = acc.clone()
            dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=self.pg)
        return acc.tolist()

    def _log(self, test_mode):
        """ParallelRunner._log (:223-231)."""
        prefix = "test_" if test_mode else ""
        s = self._sums(test_mode)
        self.logger.log_stat(prefix + "return_mean", s[1] / s[0], self.t_env)
        for i, k in enumerate(STAT_KEYS):
            self.logger.log_stat(prefix + k + "_mean", s[2 + i] / s[0], self.t_env)
        self._acc[int(test_mode)].zero_()
        self._n_acc[int(test_mode)] = 0

    def _stats_dict(self, mode):
        if self._acc is None:
            raise RuntimeError("this runner collects no statistics (give it a logger or collect_stats=True)")
        s = self._sums(mode)
        return {"n_episodes": int(s[0]), "return": s[1], **{k: s[2 + i] for i, k in enumerate(STAT_KEYS)}}

    @property
    def train_stats(self):
        """The sums accumulated over the train runs since the last log, as the
        reference's train_stats dict plus "return" (Σ episode returns).  A
        synchronising read, for inspection (a collective with a process group)."""
        return self._stats_dict(False)

    @property
    def test_stats(self):
        """As train_stats, for the test runs."""
        return self._stats_dict(True)

    def evaluate(self, n_runs=None, new_buffers=True, per_episode=False):
        """max(1, test_nepisode // n) greedy runs (per_run.py:240,255-256), after which
        the test statistics are logged; returns the last run's batch.

        per_episode=True: returns (batch, rows) with ``rows`` a CPU fp64 tensor
        [episodes, len(EPISODE_INFO_KEYS)], one row per evaluated episode in run
        order: its return and the STAT_KEYS values of its terminal step (NaN for an
        env that did not terminate) — what evaluate_sequential collects as
        episode_info (per_run.py:80-94).  One host copy per run."""
        batch, rows = None, []
        for _ in range(max(1, self.test_nepisode // self.n) if n_runs is None else int(n_runs)):
            batch = self.run(test_mode=True, new_buffers=new_buffers)
            if per_episode:
                rows.append(self._episode_rows())
        return (batch, torch.cat(rows)) if per_episode else batch

    def _episode_rows(self):
        env = self.env
        done = env.terminated.double().unsqueeze(1)
        row = torch.cat([self.last_returns.unsqueeze(1), env.reward.unsqueeze(1), env.info[:, :4], done,
                         env.info[:, 4:]], dim=1).cpu()
        row[row[:, 6] == 0, 1:] = float("nan")
        return row

    # -- saved state (driver.save_run_state) ---------------------------------------------
    def _built_with(self):
        s = self.schedule
        return {"epsilon_schedule": [s.start, s.finish, s.time_length], "precision": self.precision,
                "compact_obs": self.compact_obs, "noisy": self.noisy}

    def state_dict(self):
        """t_env, the episode count (the ε-greedy draw counter), the seed in use, the
        log schedule's counter and the statistics accumulators.  The env is saved by
        its own state_dict, not nested here."""
        return {"format": 1, **self._built_with(), "t_env": int(self.t_env), "episode": int(self.episode),
                "seed": self.seed, "log_train_stats_t": int(self.log_train_stats_t),
                "acc": None if self._acc is None else self._acc.detach().cpu(), "n_acc": list(self._n_acc)}

    def load_state_dict(self, sd):
        sd = {"noisy": False, **sd}  # (a state saved before the noisy head existed: a plain agent)
        check_fields("RolloutRunner", sd, {"format": 1, **self._built_with()})
        if (sd["acc"] is None) != (self._acc is None):
            raise ValueError(f"RolloutRunner state: acc (the statistics accumulators) is "
                             f"{'absent' if sd['acc'] is None else 'present'} in the saved state, "
                             f"{'absent' if self._acc is None else 'present'} here")
        if self._acc is not None:
            copy_checked("RolloutRunner", "acc", self._acc, sd["acc"])
        self.t_env, self.episode, self.seed = int(sd["t_env"]), int(sd["episode"]), int(sd["seed"])
        self.log_train_stats_t = int(sd["log_train_stats_t"])
        self._n_acc = [int(v) for v in sd["n_acc"]]

    def _dest(self, tm, t):
        if self.compact_obs:
            return {"obs": self._obs_step, "wire": tm["obs_wire"][t], "state": tm["state"][t],
                    "avail": tm["avail_actions"][t]}
        return {"obs": tm["obs"][t], "state": tm["state"][t], "avail": tm["avail_actions"][t]}
