"""The prioritized-replay sampling cases shared by the CPU margin test
(tests/test_replay_oracle.py) and the GPU kernel tests
(tests/test_gpu_replay_kernels.py): the same fp32 priorities, seed and counter,
so the margin the CPU test asserts is the margin of what the GPU test compares."""
import numpy as np

SEED, COUNTER = 7, 3
SIZES = (1, 2, 1023, 1024, 1025, 2047, 5000)  # around the 1024-thread chunking; the reference's 5000
BATCHES = (1, 32, 1024, 1500)  # one wave, the bench's batch, past the 1024-thread stride
SHAPES = ("uniform", "heavy", "dominant", "equal")
# noise of another fp64 summation order is ~1e-13 of the total; every stratum of
# every case keeps this distance from the nearest prefix-sum boundary
MIN_MARGIN = 1e-10


def priorities(shape, n, rng):
    """fp32 stored priorities (p = priority ** alpha) of one case."""
    if shape == "uniform":
        p = rng.uniform(0.01, 5.0, n)
    elif shape == "heavy":
        p = np.exp(rng.normal(0.0, 3.0, n))
    elif shape == "dominant":  # most strata land in one slot
        p = 10.0 ** rng.uniform(-6.0, -3.0, n)
        p[int(rng.integers(n))] = 1e4
    elif shape == "equal":
        p = np.full(n, 0.75)
    else:
        raise ValueError(shape)
    return p.astype(np.float32)


def sample_cases():
    """[(n, batch, shape, beta, p fp32 [n])]: the full grid at beta 0.7, plus beta 0 and
    beta 1.3 (past t_max) at the reference's size."""
    rng = np.random.default_rng(0)
    out = []
    for n in SIZES:
        for batch in BATCHES:
            for shape in SHAPES:
                out.append((n, batch, shape, 0.7, priorities(shape, n, rng)))
    for beta in (0.0, 1.3):
        out.append((5000, 1024, "heavy", beta, priorities("heavy", 5000, rng)))
    return out


# ---- the state-machine test's schedule (tests/test_gpu_replay_kernels.py) ---------
SM_CAPACITY, SM_ROUNDS, SM_T1, SM_AGENTS = 1100, 30, 3, 2
SM_ALPHA, SM_BETA, SM_T_MAX, SM_SEED = 0.6, 0.4, 20, 11
SM_COUNTS = (1, 7, 64, 300, 1200)


def sm_schedule():
    """[(insert count, sample batch, t)] per round, from a fixed generator."""
    rng = np.random.default_rng(5)
    return [(int(rng.choice(SM_COUNTS)), 32 if r % 2 == 0 else 257, r) for r in range(SM_ROUNDS)]


def sm_episodes(first, count):
    """Episodes number first .. first+count-1 as a batch: every field encodes the global
    episode number, so a gather is checkable against the number alone."""
    e = np.arange(first, first + count, dtype=np.int64)
    T1, A = SM_T1, SM_AGENTS
    t = np.arange(T1, dtype=np.int64)
    obs = (e[:, None, None, None] * 1.0 + t[None, :, None, None] * 0.25 +
           np.arange(A)[None, None, :, None] * 0.0625 + np.arange(9 * A)[None, None, None, :] * 1e-3)
    return {
        "obs": obs.astype(np.float32),
        "actions": (e[:, None, None, None] * 8 + t[None, :, None, None] * 2 +
                    np.arange(A)[None, None, :, None]).astype(np.int64),
        "terminated": ((e[:, None, None] + t[None, :, None]) % 251).astype(np.uint8),
        "filled": np.broadcast_to(((e[:, None, None] % 3) >= t[None, :, None]).astype(np.float32),
                                  (count, T1, 1)).copy(),
        "obs_nrm_n": (e * 1000003).astype(np.int64),
        "obs_nrm": (e[:, None, None] + np.arange(2)[None, :, None] * 0.5 +
                    np.arange(9 * A)[None, None, :] * 2.0 ** -20).astype(np.float64),
    }


def sm_priorities(episode, rnd):
    """New priorities as a fixed function of (global episode number, round): about
    one in ten is 0, negative, NaN or +Inf (the buffer must leave those slots as
    they were)."""
    episode = np.asarray(episode, np.int64)
    h = (episode * 2654435761 + rnd * 40503) % 1000
    pr = (0.001 + (h / 1000.0) ** 3 * 20.0).astype(np.float32)
    bad = (episode * 7 + rnd * 3) % 40
    pr = np.where(bad == 0, np.float32(0.0), pr)
    pr = np.where(bad == 1, np.float32(-1.5), pr)
    pr = np.where(bad == 2, np.float32(np.nan), pr)
    pr = np.where(bad == 3, np.float32(np.inf), pr)
    return pr.astype(np.float32)
