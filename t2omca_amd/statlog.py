"""The slice of PyMARL's utils.logging.Logger that the runner, the learner and
the driver call (parallel_runner.py:218,224-230, per_run.py:284-285):

    logger.log_stat(key, value, t)
    logger.print_recent_stats()

``stats[key]`` is the list of ``(t, value)`` pairs logged under ``key``, as
PyMARL keeps it.  No tensorboard, no sacred.

``state_dict()`` / ``load_state_dict(sd)`` save and restore ``stats`` (as
``{key: [[t, value], ...]}``: plain lists, so ``torch.load(weights_only=True)``
keeps it), for driver.save_run_state.
"""
from collections import defaultdict


class StatsLogger:
    def __init__(self, out=print):
        """out: callable taking the line ``print_recent_stats`` writes."""
        self.stats = defaultdict(list)
        self.out = out

    def log_stat(self, key, value, t):
        self.stats[key].append((t, float(value)))

    def state_dict(self):
        return {"format": 1, "stats": {k: [[t, v] for t, v in rows] for k, rows in self.stats.items()}}

    def load_state_dict(self, sd):
        if sd.get("format") != 1:
            raise ValueError(f"StatsLogger state: format {sd.get('format')!r}, expected 1")
        self.stats = defaultdict(list, {k: [(t, float(v)) for t, v in rows] for k, rows in sd["stats"].items()})

    def recent(self):
        """{key: latest value}."""
        return {k: v[-1][1] for k, v in self.stats.items() if v}

    def print_recent_stats(self):
        """One line: the latest ``t_env`` / ``episode`` and every key's latest value."""
        recent = self.recent()
        t = max((v[-1][0] for v in self.stats.values() if v), default=0)
        head = f"t_env: {t:>10} | episode: {int(recent.get('episode', 0)):>8}"
        body = " ".join(f"{k}: {recent[k]:.4f}" for k in sorted(recent) if k != "episode")
        self.out(f"{head} | {body}" if body else head)
