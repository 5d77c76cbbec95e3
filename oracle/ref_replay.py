"""TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

numpy restatement of PyMARL2's proportional PrioritizedReplayBuffer sampling
and priority update (the reference's components.episode_buffer is absent;
contract per_run.py:143-146, 216-238), written the way the
segment trees compute it:

    p_total = sum_tree.sum(0, n - 1);  every_range_len = p_total / batch
    mass_k  = u_k * every_range_len + k * every_range_len
    idx_k   = find_prefixsum_idx(mass_k)  (smallest i with Σ_{j<=i} p_j > mass_k)
    p_min   = min_tree.min() / sum_tree.sum();  max_w = (p_min * n) ** -beta
    w_k     = (p[idx_k] / sum_tree.sum() * n) ** -beta / max_w
    update: p[idx] = priority ** alpha;  max_priority = max(max_priority, priority)

with u_k = U(seed, k, counter) of the counter-based stream (oracle/ref_mac.py),
seed keyed by STREAM_PER.
Parity unpinned against the absent module; pinned to PyMARL2's published code.

RefBuffer is the whole buffer as a host model (ring, p, max_priority, draws)
built from sample / update; sample_margin says how far a case's strata are from
a prefix-sum boundary, the precondition of an exact index comparison.
"""
import numpy as np

from oracle.ref_mac import STREAM_PER, _uniform


def sample(p, batch, beta, seed, counter):
    p = np.asarray(p, np.float64)
    n = len(p)
    cum = np.cumsum(p)
    total = cum[-1]
    rng = total / batch
    idx = np.empty(batch, np.int64)
    w = np.empty(batch, np.float64)
    max_w = (p.min() / total * n) ** (-beta)
    for k in range(batch):
        mass = _uniform(seed, k, counter, STREAM_PER) * rng + k * rng
        i = int(np.searchsorted(cum, mass, side="right"))
        idx[k] = min(i, n - 1)
        w[k] = (p[idx[k]] / total * n) ** (-beta) / max_w
    return idx, w


def update(p, max_priority, idx, priorities, alpha):
    p = np.array(p, np.float64)
    for i, pr in zip(idx, priorities):
        if not (pr > 0 and np.isfinite(pr)):  # PyMARL2 asserts priority > 0: such values are dropped
            continue
        p[i] = pr ** alpha
        max_priority = max(max_priority, pr)
    return p, max_priority


def sample_margin(p, batch, seed, counter):
    """min over the strata of |cum_i - mass_k| / total: how far the nearest
    prefix-sum boundary is from any stratum's mass.  An exact-index comparison
    with an implementation that sums in another fp64 order (reordering noise
    ~1e-13 of the total) is sound only where this is well above that noise."""
    p = np.asarray(p, np.float64)
    cum = np.cumsum(p)
    total = cum[-1]
    rng = total / batch
    mass = np.array([_uniform(seed, k, counter, STREAM_PER) * rng + k * rng for k in range(batch)])
    i = np.searchsorted(cum, mass, side="right")
    above = np.abs(cum[np.minimum(i, len(p) - 1)] - mass)
    below = np.where(i > 0, np.abs(mass - cum[np.maximum(i - 1, 0)]), np.inf)
    return float(np.minimum(above, below).min() / total)


class RefBuffer:
    """Host model of the whole device buffer (t2omca_amd/replay.py): ring arrays,
    p = priority ** alpha in fp64, max_priority, the ring position and the draw
    counter, with the buffer's four operations built from sample / update above.

    scheme: {key: (per-episode shape, dtype)}."""

    def __init__(self, scheme, capacity, alpha, beta, t_max, seed=0):
        self.capacity, self.alpha, self.beta_original = int(capacity), float(alpha), float(beta)
        self.beta = self.beta_original
        self.beta_increment = (1.0 - self.beta_original) / float(t_max)
        self.seed = int(seed)
        self.data = {k: np.zeros((self.capacity,) + tuple(shape), dtype) for k, (shape, dtype) in scheme.items()}
        self.p = np.zeros(self.capacity, np.float64)
        self.max_priority = 1.0  # always an fp32-representable value
        self.buffer_index = 0
        self.episodes_in_buffer = 0
        self.draws = 0

    def insert(self, batch):
        """New episodes at max_priority ** alpha; wraps (also a batch larger than the
        free tail or than the capacity: the ring keeps the last `capacity` of them)."""
        n = len(next(iter(batch.values())))
        done = 0
        while done < n:
            m = min(n - done, self.capacity - self.buffer_index)
            sl = slice(self.buffer_index, self.buffer_index + m)
            for k, v in batch.items():
                self.data[k][sl] = np.asarray(v)[done:done + m]
            self.p[sl] = self.max_priority ** self.alpha
            self.buffer_index = (self.buffer_index + m) % self.capacity
            self.episodes_in_buffer = min(self.capacity, self.episodes_in_buffer + m)
            done += m

    def can_sample(self, batch_size):
        return self.episodes_in_buffer >= batch_size

    def sample(self, batch_size, t):
        """(idx, weights fp64); beta annealed to t (beyond t_max it keeps growing, as
        the buffer's does); one draw of the stream consumed."""
        self.beta = self.beta_original + t * self.beta_increment
        idx, w = sample(self.p[:self.episodes_in_buffer], batch_size, self.beta, self.seed, self.draws)
        self.draws += 1
        return idx, w

    def gather(self, idx):
        return {k: v[np.asarray(idx)] for k, v in self.data.items()}

    def update(self, idx, priorities, add=0.0):
        """v = float32(priority) + float32(add) in fp32, as the kernel adds it; v not > 0
        or not finite is skipped; of duplicates the last valid one wins.  Returns the
        mask of the entries that were valid."""
        with np.errstate(invalid="ignore", over="ignore"):
            v = (np.asarray(priorities, np.float32) + np.float32(add)).astype(np.float32)
        self.p, mx = update(self.p, self.max_priority, np.asarray(idx, np.int64), v.astype(np.float64), self.alpha)
        self.max_priority = float(mx)
        return (v > 0) & np.isfinite(v)
