"""CPU: the host model of the replay buffer (oracle/ref_replay.RefBuffer) against a
naive list-of-episodes ring, and the precondition of the GPU tests' exact index
comparison: no stratum of any sampling case lies within fp64 summation-order
noise of a prefix-sum boundary."""
import numpy as np

from oracle import ref_replay
from tests import replay_cases as rc


class _NaiveRing:
    """One episode at a time into a list of slots; priorities as PyMARL2's loop."""

    def __init__(self, capacity, alpha):
        self.capacity, self.alpha = capacity, alpha
        self.slots = [None] * capacity
        self.p = [0.0] * capacity
        self.max_priority = 1.0
        self.pos = 0
        self.count = 0

    def insert(self, episodes):
        for e in episodes:
            self.slots[self.pos] = e
            self.p[self.pos] = self.max_priority ** self.alpha
            self.pos = (self.pos + 1) % self.capacity
            self.count = min(self.capacity, self.count + 1)

    def update(self, idx, v):
        for i, x in zip(idx, v):
            x = float(x)
            if x > 0 and np.isfinite(x):
                self.p[i] = x ** self.alpha
                self.max_priority = max(self.max_priority, x)


def test_model_ring_matches_naive_episode_list():
    cap, alpha = 37, 0.6
    rng = np.random.default_rng(2)
    scheme = {"obs": ((3, 2), np.float32), "actions": ((3, 1), np.int64), "obs_nrm_n": ((), np.int64)}
    model = ref_replay.RefBuffer(scheme, cap, alpha, 0.4, 100, seed=5)
    naive = _NaiveRing(cap, alpha)
    made = 0
    wraps = 0
    for step in range(120):
        m = int(rng.choice([1, 5, 20, 36, 37, 38, 90]))  # below, at and beyond the free tail and the capacity
        e = np.arange(made, made + m)
        made += m
        batch = {"obs": np.broadcast_to(e[:, None, None].astype(np.float32), (m, 3, 2)).copy(),
                 "actions": np.broadcast_to(e[:, None, None] * 3, (m, 3, 1)).copy(),
                 "obs_nrm_n": e * 11}
        before = model.buffer_index
        model.insert(batch)
        naive.insert(list(e))
        wraps += (before + m) // cap
        assert model.buffer_index == naive.pos and model.episodes_in_buffer == naive.count
        assert model.episodes_in_buffer == min(cap, made)
        k = naive.count
        assert np.array_equal(model.data["obs"][:k, 0, 0], np.array(naive.slots[:k], np.float32))
        assert np.array_equal(model.data["actions"][:k, 2, 0], np.array(naive.slots[:k]) * 3)
        assert np.array_equal(model.data["obs_nrm_n"][:k], np.array(naive.slots[:k]) * 11)
        assert np.array_equal(model.p, np.array(naive.p))
        # priorities with duplicates and invalid values, with and without the add constant
        n_up = int(rng.integers(1, 2 * k + 2))
        idx = rng.integers(0, k, n_up)
        pr = rng.uniform(0.0, 4.0, n_up).astype(np.float32)
        bad = rng.integers(0, 10, n_up)
        pr[bad == 0] = 0.0
        pr[bad == 1] = -2.0
        pr[bad == 2] = np.nan
        pr[bad == 3] = np.inf
        add = 1e-6 if step % 2 else 0.0
        valid = model.update(idx, pr, add=add)
        with np.errstate(invalid="ignore"):
            v = pr + np.float32(add)
        assert v.dtype == np.float32
        naive.update(idx, v)
        assert np.array_equal(valid, (v > 0) & np.isfinite(v))
        assert np.array_equal(model.p, np.array(naive.p)) and model.max_priority == naive.max_priority
        assert np.float32(model.max_priority) == model.max_priority
        # the gather returns the ring's rows
        got = model.gather(idx)
        assert np.array_equal(got["obs_nrm_n"], np.array([naive.slots[i] for i in idx]) * 11)
    assert wraps > 10
    # sampling consumes one draw per call and anneals beta past t_max
    d0 = model.draws
    i1, w1 = model.sample(8, 250)
    assert model.draws == d0 + 1 and abs(model.beta - (0.4 + 250 * 0.6 / 100)) < 1e-12
    i2, w2 = ref_replay.sample(model.p[:model.episodes_in_buffer], 8, model.beta, 5, d0)
    assert np.array_equal(i1, i2) and np.array_equal(w1, w2)


def test_update_last_valid_duplicate_wins():
    model = ref_replay.RefBuffer({"x": ((), np.int64)}, 4, 0.5, 0.4, 10)
    model.insert({"x": np.arange(4)})
    model.update([2, 2, 2, 1, 1], [4.0, 9.0, np.nan, 16.0, -1.0])
    assert model.p.tolist() == [1.0, 4.0, 3.0, 1.0] and model.max_priority == 16.0


def test_sampling_cases_keep_their_margin():
    """Every stratum of every case the GPU tests compare index-for-index is at least
    MIN_MARGIN (of the total) away from the nearest prefix-sum boundary."""
    cases = rc.sample_cases()
    assert len(cases) == 7 * 4 * 4 + 2
    worst = min(ref_replay.sample_margin(p, batch, rc.SEED, rc.COUNTER) for n, batch, shape, beta, p in cases)
    print(f"smallest stratum margin over {len(cases)} cases: {worst:.3e}")
    assert worst >= rc.MIN_MARGIN


def test_state_machine_schedule_covers_its_edges():
    """The GPU state-machine test's schedule wraps the ring at least twice, inserts
    more than the capacity at once, and samples past t_max."""
    sched = rc.sm_schedule()
    counts = [c for c, _, _ in sched]
    assert sum(counts) > 2 * rc.SM_CAPACITY and max(counts) > rc.SM_CAPACITY
    assert set(counts) == set(rc.SM_COUNTS)
    assert max(t for _, _, t in sched) > rc.SM_T_MAX
    pr = rc.sm_priorities(np.arange(5000), 3)
    with np.errstate(invalid="ignore"):
        skipped = ~((pr + np.float32(1e-6) > 0) & np.isfinite(pr))
    assert 0.05 < skipped.mean() < 0.15
