"""The reference's training loop (per_run.py:200-289) over objects the caller built.

    logger = run_sequential(runner, buffer, learner, logger, args)

``runner`` is a RolloutRunner (built with the same ``logger``, ``test_nepisode`` and
``runner_log_interval``), ``buffer`` a PrioritizedReplayBuffer, ``learner`` a
TDLearner (built with the logger and ``learner_log_interval``); any objects with
the same methods do.  ``args`` carries the reference's fields:

    t_max, batch_size, batch_size_run, test_interval, test_nepisode, log_interval   required
    accumulated_episodes (None), save_model (False), save_model_interval (2000000),
    local_results_path ("results"), unique_token ("t2omca")                         optional

Each iteration, in the reference's order: a train rollout; insert_episode_batch;
when the buffer can sample — unless accumulated_episodes says to skip (:218-222)
— sample, truncate to the filled steps, train, and update the priorities on the
device (``td_errors_abs`` + 1e-6, :237-238, added inside the PER kernel); the
test runs every test_interval env steps (:241-256); a checkpoint in a directory
named by t_env (:265-279); ``episode += batch_size_run``; the "episode" log line
every log_interval env steps (:283-286).  The loop ends once t_env > t_max.

The accumulated_episodes skip is the reference's ``continue``: it also skips the
rest of that iteration — tests, checkpoint, the episode count and the log line.

Not here: checkpoint-directory discovery (:159-189), evaluate_sequential,
animation / replay saving, sacred and tensorboard.
"""
import os


def run_sequential(runner, buffer, learner, logger, args):
    accumulated_episodes = getattr(args, "accumulated_episodes", None)
    save_model = getattr(args, "save_model", False)
    save_model_interval = getattr(args, "save_model_interval", 2000000)
    results_path = getattr(args, "local_results_path", "results")
    unique_token = getattr(args, "unique_token", "t2omca")

    episode = 0
    last_test_T = -args.test_interval - 1
    last_log_T = 0
    model_save_time = 0

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
            save_path = os.path.join(results_path, "models", unique_token, str(runner.t_env))
            os.makedirs(save_path, exist_ok=True)
            learner.save_models(save_path)

        episode += args.batch_size_run

        if (runner.t_env - last_log_T) >= args.log_interval:
            logger.log_stat("episode", episode, runner.t_env)
            logger.print_recent_stats()
            last_log_T = runner.t_env

    return logger
