"""The reference's training loop (per_run.py:159-289) over objects the caller built.

    logger = run_sequential(runner, buffer, learner, logger, args)

``runner`` is a RolloutRunner (built with the same ``logger``, ``test_nepisode`` and
``runner_log_interval``), ``buffer`` a PrioritizedReplayBuffer, ``learner`` a
TDLearner (built with the logger and ``learner_log_interval``); any objects with
the same methods do.  ``args`` carries the reference's fields:

    t_max, batch_size, batch_size_run, test_interval, test_nepisode, log_interval   required
    accumulated_episodes (None), save_model (False), save_model_interval (2000000),
    local_results_path ("results"), unique_token ("t2omca"),
    checkpoint_path (""), load_step (0), evaluate (False)                           optional

and this project's own, all optional:

    save_run_state (False), save_replay_buffer (True), run_state_keep (1; 0 = keep all)

Each iteration, in the reference's order: a train rollout; insert_episode_batch;
when the buffer can sample — unless accumulated_episodes says to skip (:218-222)
— sample, truncate to the filled steps, train, and update the priorities on the
device (``td_errors_abs`` + 1e-6, :237-238, added inside the PER kernel); the
test runs every test_interval env steps (:241-256); a checkpoint in a directory
named by t_env (:265-279); ``episode += batch_size_run``; the "episode" log line
every log_interval env steps (:283-286).  The loop ends once t_env > t_max.

A NoisyNet agent (``action_selector: noisy-new``) needs nothing here: the runner and
the learner detect it, and their noise is a function of their seeds and counters.

The accumulated_episodes skip is the reference's ``continue``: it also skips the
rest of that iteration — tests, checkpoint, the episode count and the log line.

Start-up (:159-198).  With ``checkpoint_path`` the numbered directory chosen by
``find_checkpoint`` is loaded before the loop: the reference's way —
``learner.load_models``, ``runner.t_env = step``, counters from zero — unless the
directory holds a run state (below).  A missing ``checkpoint_path`` returns the
logger without running, as the reference does.  ``evaluate`` then runs the test
episodes once (``runner.evaluate()``), logs and returns: no training, no
checkpoint.

Run state.  The model files do not restore a run: the env's observation
normaliser, queues and draw counters, the replay, the target mixer, the
schedules' counters and the logger are not in them.  With ``save_run_state`` every
checkpoint also writes ``run_state.th`` (``run_state.rank{r}.th`` per rank with a
process group of more than one rank) beside the model files: the ``state_dict()``
of the env, the runner, the buffer (``save_replay_buffer=False``: its counters
only), the learner and the logger, the loop's counters and the world size.  A run
started with ``checkpoint_path`` on such a directory continues bit for bit: every
random draw is counter-based and the update is reproducible, so the resumed run
computes and logs what the uninterrupted one would have.  It continues from the
statement after the checkpoint block of the iteration that wrote the file —
``episode += batch_size_run``, that iteration's log line, then the next
iteration — because a checkpoint is written in mid-iteration.  The file is written
under a temporary name and renamed after ``save_models`` has returned, so a
killed process never leaves a truncated run state for a later scan to pick.  One
killed between the model files and the rename (or, with several ranks, between
two ranks' renames) leaves its newest directory without a complete run state:
with ``load_step == 0`` the start-up then warns and resumes from the newest
directory that holds one for every rank of this world size — the last complete
checkpoint — and loads the newest directory the reference's way only when no
directory has a run state.  An explicit ``load_step`` is taken at its word; a
chosen directory whose run-state files are not exactly this world size's is a
ValueError on every rank, before any of them loads.  A
buffer snapshot is the whole replay (``run_state_keep`` older ones are removed,
the model files stay); without it the resumed run starts from an empty buffer
and is no longer bit-exact.

Not here: animation / replay saving, sacred and tensorboard; evaluation with a
frozen observation normaliser (the reference env never asks for it).
"""
import os
import warnings

import torch

from .distributed import rank as dist_rank, world_size

LOOP_KEYS = ("episode", "last_test_T", "last_log_T", "model_save_time")


def find_checkpoint(checkpoint_path, load_step=0):
    """The numbered sub-directory of checkpoint_path to load (per_run.py:164-184), as
    (path, step): the largest step with load_step == 0, otherwise the one nearest to
    load_step.  Only sub-directories whose names are all digits count.  The steps
    are sorted numerically first, so a tie between two equally near steps goes to
    the SMALLER one (the reference's ``min`` over ``os.listdir`` leaves it to the
    listing order).  None when checkpoint_path is no directory (the reference logs
    and returns); ValueError when it holds no numbered directory (the reference
    would die in ``max([])``)."""
    if not os.path.isdir(checkpoint_path):
        return None
    steps = sorted(int(name) for name in os.listdir(checkpoint_path)
                   if name.isdigit() and os.path.isdir(os.path.join(checkpoint_path, name)))
    if not steps:
        raise ValueError(f"checkpoint_path {checkpoint_path!r} holds no numbered checkpoint directory")
    step = steps[-1] if load_step == 0 else min(steps, key=lambda s: abs(s - load_step))
    return os.path.join(checkpoint_path, str(step)), step


def _group(learner):
    return getattr(learner, "pg", None)


def run_state_file(path, group=None):
    """path/run_state.th, or path/run_state.rank{r}.th with more than one rank."""
    if world_size(group) > 1:
        return os.path.join(path, f"run_state.rank{dist_rank(group)}.th")
    return os.path.join(path, "run_state.th")


def _run_state_files(path):
    """Every rank's run-state file in a checkpoint directory."""
    return sorted(f for f in os.listdir(path) if f.startswith("run_state.") and f.endswith(".th"))


def _expected_files(group=None):
    """The run-state files a complete checkpoint of this world size holds."""
    world = world_size(group)
    return ["run_state.th"] if world == 1 else sorted(f"run_state.rank{r}.th" for r in range(world))


def has_run_state(path, group=None):
    """Does the checkpoint directory hold the run state of EVERY rank of this world
    size?  (Decided from the directory listing alone, so every rank that sees the
    same file system decides alike.)"""
    return all(os.path.isfile(os.path.join(path, f)) for f in _expected_files(group))


def newest_run_state(checkpoint_path, group=None):
    """(path, step) of the largest numbered sub-directory that holds a complete run
    state for this world size, or None."""
    steps = sorted((int(d) for d in os.listdir(checkpoint_path)
                    if d.isdigit() and has_run_state(os.path.join(checkpoint_path, d), group)), reverse=True)
    return (os.path.join(checkpoint_path, str(steps[0])), steps[0]) if steps else None


def save_run_state(path, runner, buffer, learner, logger, loop, include_buffer=True):
    """Write this rank's run state into the checkpoint directory ``path`` (module
    docstring); ``loop`` is the dict of the driver's counters (LOOP_KEYS).  Every
    rank stores the learner too, so that a file is self-contained.  Returns the
    file's name."""
    group = _group(learner)
    state = {"format": 1, "world_size": world_size(group), "rank": dist_rank(group),
             "loop": {k: int(loop[k]) for k in LOOP_KEYS},
             "env": runner.env.state_dict(), "runner": runner.state_dict(),
             "buffer": buffer.state_dict(include_data=include_buffer),
             "learner": learner.state_dict(), "logger": logger.state_dict()}
    name = run_state_file(path, group)
    tmp = name + ".tmp"
    torch.save(state, tmp)
    os.replace(tmp, name)
    return name


def load_run_state(path, runner, buffer, learner, logger):
    """Load this rank's run state from the checkpoint directory ``path`` into the
    five objects, in place; returns the loop counters.  ValueError when the directory
    does not hold exactly the files of this world size (written at another one, or a
    rank's file is missing: every rank sees that in the listing and raises before
    any of them loads, so none waits in the learner's broadcast), when the file
    says another world size, or when its runner's t_env is not the number the
    directory is named by."""
    group = _group(learner)
    name = run_state_file(path, group)
    if _run_state_files(path) != _expected_files(group):
        raise ValueError(f"{path}: a run at world_size {world_size(group)} needs {_expected_files(group)}, "
                         f"the directory holds {_run_state_files(path)}")
    state = torch.load(name, map_location="cpu", weights_only=True)
    if state.get("format") != 1:
        raise ValueError(f"{name}: format {state.get('format')!r}, expected 1")
    if state["world_size"] != world_size(group):
        raise ValueError(f"{name}: world_size is {state['world_size']} in the saved state, "
                         f"{world_size(group)} here")
    step = os.path.basename(os.path.normpath(path))
    if step.isdigit() and int(step) != state["runner"]["t_env"]:
        raise ValueError(f"{name}: the saved runner's t_env is {state['runner']['t_env']}, "
                         f"the directory is named {step}")
    runner.env.load_state_dict(state["env"])
    runner.load_state_dict(state["runner"])
    buffer.load_state_dict(state["buffer"])
    learner.load_state_dict(state["learner"])
    logger.load_state_dict(state["logger"])
    return dict(state["loop"])


def _prune_run_states(models_dir, step, keep, group=None):
    """After the run state of directory ``step`` is written: of the older numbered
    directories (smaller numbers) only the ``keep - 1`` newest keep this rank's
    run-state file; the model files stay."""
    base = os.path.basename(run_state_file("", group))
    older = sorted(int(d) for d in os.listdir(models_dir)
                   if d.isdigit() and int(d) < step and os.path.isfile(os.path.join(models_dir, d, base)))
    for old in older[:max(0, len(older) - (keep - 1))]:
        os.remove(os.path.join(models_dir, str(old), base))


def _log_episode(logger, episode, t_env, last_log_T, log_interval):
    """The "episode" log line every log_interval env steps (:283-286); returns last_log_T."""
    if (t_env - last_log_T) >= log_interval:
        logger.log_stat("episode", episode, t_env)
        logger.print_recent_stats()
        return t_env
    return last_log_T


def run_sequential(runner, buffer, learner, logger, args):
    accumulated_episodes = getattr(args, "accumulated_episodes", None)
    save_model = getattr(args, "save_model", False)
    save_model_interval = getattr(args, "save_model_interval", 2000000)
    results_path = getattr(args, "local_results_path", "results")
    unique_token = getattr(args, "unique_token", "t2omca")
    checkpoint_path = getattr(args, "checkpoint_path", "")
    with_run_state = getattr(args, "save_run_state", False)
    include_buffer = getattr(args, "save_replay_buffer", True)
    run_state_keep = getattr(args, "run_state_keep", 1)

    episode = 0
    last_test_T = -args.test_interval - 1
    last_log_T = 0
    model_save_time = 0
    resumed = False  # from a run state

    if checkpoint_path != "":
        found = find_checkpoint(checkpoint_path, getattr(args, "load_step", 0))
        if found is None:
            return logger
        model_path, step = found
        group = _group(learner)
        if getattr(args, "load_step", 0) == 0 and not has_run_state(model_path, group):
            # the newest directory has no complete run state — a process killed between
            # save_models and the rename, or between two ranks' renames — but an older
            # one may: that one is the last complete checkpoint
            complete = newest_run_state(checkpoint_path, group)
            if complete is not None:
                warnings.warn(f"{model_path} holds no complete run state (an interrupted checkpoint?); "
                              f"resuming from {complete[0]}")
                model_path, step = complete
        if _run_state_files(model_path):  # (incomplete or of another world size: load_run_state raises)
            loop = load_run_state(model_path, runner, buffer, learner, logger)
            episode, last_test_T, last_log_T, model_save_time = (loop[k] for k in LOOP_KEYS)
            resumed = True
        else:
            learner.load_models(model_path)
            runner.t_env = step

    if getattr(args, "evaluate", False):
        runner.log_train_stats_t = runner.t_env
        runner.evaluate()
        logger.log_stat("episode", runner.t_env, runner.t_env)
        logger.print_recent_stats()
        return logger

    if resumed:
        # the iteration that wrote the run state, from the statement after its checkpoint block
        episode += args.batch_size_run
        last_log_T = _log_episode(logger, episode, runner.t_env, last_log_T, args.log_interval)

    while runner.t_env <= args.t_max:
        # a whole episode of every env at a time
        episode_batch = runner.run(test_mode=False)
        buffer.insert_episode_batch(episode_batch)

        if buffer.can_sample(args.batch_size):
            next_episode = episode + args.batch_size_run
            if accumulated_episodes and next_episode % accumulated_episodes != 0:
                continue

            episode_sample, idx, weights = buffer.sample(args.batch_size, runner.t_env)
            # truncate the batch to its filled timesteps
            max_ep_t = episode_sample.max_t_filled()
            episode_sample = episode_sample[:, :max_ep_t]

            info = learner.train(episode_sample, runner.t_env, episode, weights)
            del episode_sample

            buffer.update_priorities(idx, info["td_errors_abs"], add=1e-6)

        # test runs once in a while
        n_test_runs = max(1, args.test_nepisode // runner.batch_size)
        if (runner.t_env - last_test_T) / args.test_interval >= 1.0:
            last_test_T = runner.t_env
            for _ in range(n_test_runs):
                runner.run(test_mode=True)

        if save_model and (runner.t_env - model_save_time >= save_model_interval or model_save_time == 0):
            model_save_time = runner.t_env
            models_dir = os.path.join(results_path, "models", unique_token)
            save_path = os.path.join(models_dir, str(runner.t_env))
            os.makedirs(save_path, exist_ok=True)
            learner.save_models(save_path)
            if with_run_state:
                loop = dict(zip(LOOP_KEYS, (episode, last_test_T, last_log_T, model_save_time)))
                save_run_state(save_path, runner, buffer, learner, logger, loop, include_buffer=include_buffer)
                if run_state_keep:
                    _prune_run_states(models_dir, runner.t_env, run_state_keep, _group(learner))

        episode += args.batch_size_run
        last_log_T = _log_episode(logger, episode, runner.t_env, last_log_T, args.log_interval)

    return logger
