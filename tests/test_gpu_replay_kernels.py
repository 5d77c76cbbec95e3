"""GPU: the replay kernels (csrc/t2o_replay.hip) at the sizes where their code
paths change, against oracle/ref_replay.py:

  * t2o_per_sample through the raw C-ABI on a grid of n (around the 1024-thread
    chunking, the reference's 5000) x batch (up to the stride loop) x priority
    shapes: indices exactly, weights to one fp32 rounding, workspace bounds,
    poison past n, determinism of the draw stream;
  * t2o_gather_rows by alignment class (copy units 16 / 8 / 4 / 1 bytes), padded
    strides and rows past the grid cap, against host indexing;
  * the buffer as a state machine over 30 rounds against the host model
    (ref_replay.RefBuffer);
  * t2o_per_update's duplicate rule: the last valid entry of a slot stays.

The oracle always samples from the fp32 p the device holds; the fp32 powf is
judged separately (rtol 1e-6 against fp64), in the state-machine test.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ref_replay
from tests import replay_cases as rc
from tests.gpu_util import require_gpu

pytestmark = pytest.mark.gpu

EINVAL = -1  # include/t2omca.h T2O_EINVAL
W_RTOL = 2.0 ** -23  # the kernel computes the weight in fp64 and rounds once to fp32
GUARD = 64


def _lib():
    from t2omca_amd._lib import lib
    return lib()


def _stream():
    from t2omca_amd._lib import stream_ptr
    return stream_ptr(torch.device("cuda"))


def _vp(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


# ---- t2o_per_sample --------------------------------------------------------------

def _per_sample(p32, n, batch, beta, seed, counter):
    """Raw t2o_per_sample on p32[:n] (p32 may be longer: poison).  Returns (idx, w) as
    numpy after checking the workspace guard and the output guards."""
    L = _lib()
    p = torch.from_numpy(p32).cuda()
    ws_n = int(L.t2o_per_workspace_doubles(n))
    ws = torch.full((ws_n + GUARD,), -7.25, dtype=torch.float64, device="cuda")
    idx = torch.full((batch + GUARD,), -3, dtype=torch.int64, device="cuda")
    w = torch.full((batch + GUARD,), -5.0, dtype=torch.float32, device="cuda")
    rc_ = L.t2o_per_sample(_vp(p), n, batch, ctypes.c_double(beta), ctypes.c_uint64(seed), counter, _vp(ws), _vp(idx),
                           _vp(w), _stream())
    assert rc_ == 0
    torch.cuda.synchronize()
    assert bool((ws[ws_n:] == -7.25).all()), "workspace written past t2o_per_workspace_doubles(n)"
    assert bool((idx[batch:] == -3).all()) and bool((w[batch:] == -5.0).all())
    assert np.array_equal(p.cpu().numpy().view(np.uint32), p32.view(np.uint32))  # p is read-only
    return idx[:batch].cpu().numpy(), w[:batch].cpu().numpy()


def _poisoned(p32):
    """p followed by values that must never be read: huge, NaN, negative, zero."""
    return np.concatenate([p32, np.array([3e38, np.nan, -1e30, 0.0, np.inf] * 8, np.float32)])


@pytest.fixture(scope="module")
def sample_cases():
    """The grid with the oracle's answer per case, computed once."""
    out = []
    for n, batch, shape, beta, p in rc.sample_cases():
        ref_idx, ref_w = ref_replay.sample(p, batch, beta, rc.SEED, rc.COUNTER)
        out.append((n, batch, shape, beta, p, ref_idx, ref_w))
    return out


def test_per_sample_grid_matches_oracle(sample_cases):
    require_gpu()
    bad = []
    worst_w = 0.0
    for n, batch, shape, beta, p, ref_idx, ref_w in sample_cases:
        idx, w = _per_sample(_poisoned(p), n, batch, beta, rc.SEED, rc.COUNTER)
        assert idx.min() >= 0 and idx.max() < n, (n, batch, shape)
        err = float(np.max(np.abs(w.astype(np.float64) - ref_w) / ref_w))
        worst_w = max(worst_w, err)
        if not np.array_equal(idx, ref_idx) or not err <= W_RTOL:
            bad.append((n, batch, shape, beta, int((idx != ref_idx).sum()), err))
    print(f"per_sample: {len(sample_cases)} cases, worst weight error {worst_w:.3e} (bar {W_RTOL:.3e})")
    assert not bad, bad


def test_per_sample_draw_stream():
    """Same (seed, counter): the same draw; another counter or seed: another one."""
    require_gpu()
    p = rc.priorities("uniform", 5000, np.random.default_rng(1))
    a = _per_sample(p, 5000, 1024, 0.7, 7, 3)
    b = _per_sample(p, 5000, 1024, 0.7, 7, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = _per_sample(p, 5000, 1024, 0.7, 7, 4)
    d = _per_sample(p, 5000, 1024, 0.7, 8, 3)
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[0], d[0]) and not np.array_equal(c[0], d[0])


# ---- t2o_gather_rows -------------------------------------------------------------

def _carve(nbytes, offset, fill):
    """A uint8 device tensor whose byte `offset` past a 16-byte-aligned address starts
    a region of nbytes; returns (tensor, start index of the region)."""
    t = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
    start = (-t.data_ptr()) % 16 + offset
    t.copy_(fill(nbytes + 64))
    return t, start


def _pattern(seed):
    def fill(n):
        g = torch.Generator().manual_seed(seed)
        return torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    return fill


def _gather_case(row_bytes, src_pad, dst_pad, src_off, dst_off, rows, n_src, seed):
    """Runs t2o_gather_rows on carved buffers; returns the copy unit the entry chooses
    for this case after asserting the result byte for byte."""
    L = _lib()
    src_stride, dst_stride = row_bytes + src_pad, row_bytes + dst_pad
    g = np.random.default_rng(seed)
    idx = g.integers(0, n_src, rows)
    # duplicates, a descending run and the last slot
    idx[0] = n_src - 1
    if rows >= 3:
        idx[1] = idx[2] = min(1, n_src - 1)
    if rows >= 12:
        idx[4:12] = np.arange(n_src - 1, n_src - 9, -1) % n_src
    src, s0 = _carve(n_src * src_stride, src_off, _pattern(seed))
    dst, d0 = _carve(rows * dst_stride, dst_off, _pattern(seed + 1))
    before = dst.cpu().clone()
    src_h = src.cpu()
    idx_d = torch.from_numpy(idx).cuda()
    rc_ = L.t2o_gather_rows(_vp(src, s0), src_stride, _vp(idx_d), rows, _vp(dst, d0), dst_stride, row_bytes, _stream())
    assert rc_ == 0
    torch.cuda.synchronize()
    expect = before.clone()
    rows_src = src_h[s0:s0 + n_src * src_stride].view(n_src, src_stride)[:, :row_bytes]
    region = expect[d0:d0 + rows * dst_stride].view(rows, dst_stride)
    region[:, :row_bytes] = rows_src[torch.from_numpy(idx)]  # padding, head and the guard after the last row stay
    got = dst.cpu()
    assert torch.equal(got[:d0], expect[:d0]), "bytes before the destination changed"
    end = d0 + rows * dst_stride
    assert torch.equal(got[end:], expect[end:]), "guard after the last row changed"
    assert torch.equal(got, expect), (row_bytes, src_off, dst_off, src_pad, dst_pad)
    assert torch.equal(src.cpu(), src_h)
    al = (src.data_ptr() + s0) | (dst.data_ptr() + d0) | src_stride | dst_stride | row_bytes
    return 16 if al % 16 == 0 else 8 if al % 8 == 0 else 4 if al % 4 == 0 else 1


# (row_bytes, src_pad, dst_pad, src_off, dst_off, rows, n_src)
_GATHER_SMALL = [
    (5, 3, 7, 0, 0, 1500, 97),       # unit 1 from the size
    (5, 11, 27, 1, 4, 1500, 97),
    (12, 4, 20, 0, 0, 1500, 97),     # unit 4
    (12, 4, 20, 4, 8, 1500, 97),
    (12, 4, 20, 1, 0, 1500, 97),     # odd base: unit 1
    (24, 8, 24, 0, 0, 1500, 97),     # unit 8
    (24, 8, 24, 8, 8, 1500, 97),
    (24, 8, 24, 4, 0, 1500, 97),     # unit 4 from the base
    (24, 4, 8, 0, 0, 1500, 97),      # unit 4 from the source stride
    (48, 16, 32, 0, 0, 1500, 97),    # unit 16
    (48, 16, 32, 8, 0, 1500, 97),    # unit 8 from the base
    (48, 16, 8, 0, 0, 1500, 97),     # unit 8 from the destination stride
    (48, 16, 32, 0, 1, 1500, 97),    # unit 1 from the destination base
    (1620, 12, 28, 0, 0, 1500, 41),  # unit 4: the small obs row
    (1620, 12, 28, 4, 4, 1500, 41),
    (1620, 13, 28, 0, 8, 1500, 41),  # odd source stride: unit 1, one block past 256 units
]
_GATHER_LARGE = [
    (16389, 3, 7, 1, 0, 3, 5),         # unit 1, 16389 units > 64 * 256
    (16389, 11, 27, 1, 1, 3, 5),
    (300000, 16, 48, 0, 0, 3, 5),      # unit 16, 18750 units > 64 * 256
    (300000, 8, 8, 8, 8, 3, 5),        # unit 8 past the cap
    (300004, 4, 12, 0, 0, 3, 5),       # unit 4 past the cap
    (300004, 4, 12, 4, 8, 3, 5),
]


def test_gather_rows_alignment_classes_small_rows():
    require_gpu()
    units = [_gather_case(*c, seed=10 + i) for i, c in enumerate(_GATHER_SMALL)]
    assert set(units) == {16, 8, 4, 1}, units
    assert units == [1, 1, 4, 4, 1, 8, 8, 4, 4, 16, 8, 8, 1, 4, 4, 1]


def test_gather_rows_past_the_grid_cap():
    require_gpu()
    units = [_gather_case(*c, seed=40 + i) for i, c in enumerate(_GATHER_LARGE)]
    assert units == [1, 1, 16, 8, 4, 4]
    for (row_bytes, *_), u in zip(_GATHER_LARGE, units):
        assert row_bytes // u > 64 * 256  # the stride loop runs


def test_gather_rows_empty_and_too_many_rows():
    require_gpu()
    L = _lib()
    src = torch.arange(256, dtype=torch.uint8, device="cuda")
    dst = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert L.t2o_gather_rows(_vp(src), 16, _vp(idx), 0, _vp(dst), 16, 16, _stream()) == 0
    assert L.t2o_gather_rows(_vp(src), 16, _vp(idx), 8, _vp(dst), 16, 0, _stream()) == 0
    # the row-count check is on the host: nothing is launched, idx is not read
    assert L.t2o_gather_rows(_vp(src), 16, _vp(idx), 65536, _vp(dst), 16, 16, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())


def test_buffer_gather_reference_obs_row():
    """PrioritizedReplayBuffer.gather on the reference's obs row (151 x 16 x 144 fp32,
    1.39 MB: 16-byte units, past the grid cap) beside small fields."""
    require_gpu()
    from t2omca_amd.replay import PrioritizedReplayBuffer
    A, T1, cap = 16, 151, 8
    g = torch.Generator().manual_seed(3)
    batch = {"obs": torch.randn(cap, T1, A, 9 * A, generator=g).cuda(),
             "actions": torch.randint(0, 5, (cap, T1, A, 1), generator=g).cuda(),
             "terminated": torch.randint(0, 2, (cap, T1, 1), generator=g).to(torch.uint8).cuda()}
    buf = PrioritizedReplayBuffer(batch, cap, T1, 0.6, 0.4, 1000)
    buf.insert_episode_batch(batch)
    assert buf.data["obs"][0].numel() * 4 // 16 > 64 * 256
    idx = torch.tensor([7, 2, 2, 0, 7], device="cuda")
    got = buf.gather(idx)
    torch.cuda.synchronize()
    for k in batch:
        assert torch.equal(got[k].cpu(), batch[k].cpu()[idx.cpu()]), k


# ---- t2o_per_update: duplicates ---------------------------------------------------

def _per_update(p0, idx, prio, alpha, add, max0=1.0):
    L = _lib()
    p = torch.from_numpy(p0.astype(np.float32)).cuda()
    mx = torch.tensor([max0], dtype=torch.float32, device="cuda")
    idx_d = torch.from_numpy(np.asarray(idx, np.int64)).cuda()
    pr_d = torch.from_numpy(np.asarray(prio, np.float32)).cuda()
    assert L.t2o_per_update(_vp(p), _vp(idx_d), _vp(pr_d), len(idx), ctypes.c_float(alpha), ctypes.c_float(add),
                            _vp(mx), _stream()) == 0
    torch.cuda.synchronize()
    return p.cpu().numpy(), float(mx)


def _check_update(cap, idx, prio, add=0.0, alpha=0.6):
    """One t2o_per_update call against the sequential rule.  Every slot holds exactly
    the fp32 power of the priority the rule picks (the kernel's own powf of that one
    value: the winner is identified bit for bit), which is within rtol 1e-6 of fp64."""
    g = np.random.default_rng(cap)
    p0 = g.uniform(0.5, 2.0, cap).astype(np.float32)
    idx, prio = np.asarray(idx, np.int64), np.asarray(prio, np.float32)
    assert idx.min() >= 0 and idx.max() < cap
    got, mx = _per_update(p0, idx, prio, alpha, add)
    with np.errstate(invalid="ignore"):
        v = prio + np.float32(add)
    ref_p, ref_max = ref_replay.update(p0, 1.0, idx, v.astype(np.float64), alpha)
    valid = (v > 0) & np.isfinite(v)
    winner = {}
    for k in range(len(idx)):
        if valid[k]:
            winner[int(idx[k])] = k
    # each winner alone through the kernel: its bit pattern, free of any duplicate
    wk = np.array(sorted(winner.values()), np.int64)
    alone, _ = _per_update(p0, idx[wk], prio[wk], alpha, add)
    assert len(set(idx[wk].tolist())) == len(wk)
    untouched = np.ones(cap, bool)
    untouched[list(winner)] = False
    assert np.array_equal(got[untouched].view(np.uint32), p0[untouched].view(np.uint32))
    assert np.array_equal(got.view(np.uint32), alone.view(np.uint32)), \
        np.flatnonzero(got.view(np.uint32) != alone.view(np.uint32))[:16]
    assert np.allclose(got, ref_p, rtol=1e-6, atol=0.0)
    assert mx == ref_max
    return got


def test_per_update_duplicates_same_wave_other_wave_other_block():
    require_gpu()
    n, cap = 700, 900  # 3 blocks of 256 threads
    g = np.random.default_rng(0)
    idx = g.permutation(cap)[:n]  # distinct to begin with
    prio = g.uniform(0.01, 9.0, n).astype(np.float32)
    groups = {
        "same wave": [3, 17, 40, 63],
        "waves of one block": [70, 130, 200, 255],
        "blocks": [100, 300, 600],
        "wave, block and grid": [256, 257, 400, 511, 512, 699],
        "last invalid": [10, 330, 650],       # k = 650 is NaN: 330 must win
        "last two invalid": [20, 21, 22],     # 21, 22 invalid in one wave: 20 wins
        "all invalid": [30, 290, 580],        # the slot stays as it was
    }
    for name, ks in groups.items():
        for k in ks[1:]:
            idx[k] = idx[ks[0]]
    prio[650] = np.nan
    prio[21], prio[22] = -1.0, np.inf
    prio[30], prio[290], prio[580] = 0.0, np.nan, -np.inf
    assert len(set(idx.tolist())) == n - sum(len(ks) - 1 for ks in groups.values())
    got = _check_update(cap, idx, prio)
    winners = {"same wave": 63, "waves of one block": 255, "blocks": 600, "wave, block and grid": 699,
               "last invalid": 330, "last two invalid": 20}
    for name, win in winners.items():
        assert np.isclose(got[idx[win]], float(prio[win]) ** 0.6, rtol=1e-6, atol=0.0), name


def test_per_update_stratified_duplicates_at_the_bench_batch():
    """What sampling really produces: 1024 stratified draws from 1023 episodes repeat
    a few hundred indices, and each repeat carries its own priority."""
    require_gpu()
    p = rc.priorities("uniform", 1023, np.random.default_rng(4))
    idx, _ = ref_replay.sample(p, 1024, 0.7, 7, 3)
    assert 100 < 1024 - len(set(idx.tolist()))
    prio = rc.sm_priorities(np.arange(1024) * 13 + 5, 1)
    _check_update(1023, idx, prio, add=1e-6)
    # one slot named by every entry, across five blocks
    prio = np.random.default_rng(6).uniform(0.1, 3.0, 1200).astype(np.float32)
    prio[-1] = np.nan
    _check_update(8, np.full(1200, 5), prio)
    # fewer entries than one wave, and exactly one block
    _check_update(16, [3, 3, 4, 3], [1.0, 2.0, 3.0, 4.0])
    _check_update(300, np.arange(256) % 100, np.random.default_rng(7).uniform(0.1, 3.0, 256))


# ---- the buffer as a state machine -------------------------------------------------

def test_buffer_state_machine_matches_model():
    require_gpu()
    from t2omca_amd.replay import PrioritizedReplayBuffer
    cap, T1 = rc.SM_CAPACITY, rc.SM_T1
    example = {k: torch.from_numpy(v).cuda() for k, v in rc.sm_episodes(0, 2).items()}
    buf = PrioritizedReplayBuffer(example, cap, T1, rc.SM_ALPHA, rc.SM_BETA, rc.SM_T_MAX, seed=rc.SM_SEED)
    scheme = {k: (tuple(v.shape[1:]), v.dtype) for k, v in rc.sm_episodes(0, 1).items()}
    assert set(PrioritizedReplayBuffer.EPISODE_KEYS) <= set(scheme)
    model = ref_replay.RefBuffer(scheme, cap, rc.SM_ALPHA, rc.SM_BETA, rc.SM_T_MAX, seed=buf.seed)
    slot_episode = np.full(cap, -1, np.int64)  # global episode number in each slot

    def adopt_p(what):
        """p[:episodes] against the model's fp64 v ** alpha (the one place the fp32 pow is
        judged), then the model continues from the device's fp32 values."""
        k = model.episodes_in_buffer
        dev = buf.p.cpu().numpy()
        assert np.allclose(dev[:k], model.p[:k], rtol=1e-6, atol=0.0), what
        assert not dev[k:].any(), what
        model.p[:k] = dev[:k].astype(np.float64)
        return dev

    made, sampled, wraps, skipped_total = 0, 0, 0, 0
    for rnd, (count, b, t) in enumerate(rc.sm_schedule()):
        # ---- insert ------------------------------------------------------------
        eps = rc.sm_episodes(made, count)
        first_slot = model.buffer_index
        buf.insert_episode_batch({k: torch.from_numpy(v).cuda() for k, v in eps.items()})
        model.insert(eps)
        slot_episode[(first_slot + np.arange(count)) % cap] = made + np.arange(count)
        wraps += (first_slot + count) // cap
        made += count
        assert (buf.buffer_index, buf.episodes_in_buffer) == (model.buffer_index, model.episodes_in_buffer)
        assert float(buf.max_priority) == model.max_priority
        adopt_p(("insert", rnd))
        k = model.episodes_in_buffer
        assert np.array_equal(model.data["obs_nrm_n"][:k], slot_episode[:k] * 1000003)
        if not buf.can_sample(b):
            assert not model.can_sample(b)
            continue
        # ---- sample ------------------------------------------------------------
        assert buf._draws == model.draws == sampled
        batch, idx, w = buf.sample(b, t)
        ref_idx, ref_w = model.sample(b, t)
        sampled += 1
        assert buf._draws == model.draws == sampled and buf.beta == model.beta
        assert ref_replay.sample_margin(model.p[:k], b, model.seed, sampled - 1) >= rc.MIN_MARGIN, rnd
        idx_h = idx.cpu().numpy()
        assert np.array_equal(idx_h, ref_idx), rnd
        w_h = w.cpu().numpy().astype(np.float64)
        assert np.max(np.abs(w_h - ref_w) / ref_w) <= W_RTOL, rnd
        ref_rows = model.gather(ref_idx)
        assert set(batch.keys()) == set(ref_rows)
        for key, v in ref_rows.items():
            got = batch[key].cpu().numpy()
            assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, v), (rnd, key)
        # ---- update priorities -------------------------------------------------------
        pr = rc.sm_priorities(slot_episode[idx_h], rnd)
        p_before = buf.p.cpu().numpy()
        if rnd % 2 == 0:  # device tensors, the add inside the kernel
            buf.update_priorities(idx, torch.from_numpy(pr).cuda(), add=1e-6)
            valid = model.update(idx_h, pr, add=1e-6)
        else:  # host lists of td + 1e-6, the reference driver's call
            host = (torch.from_numpy(pr) + 1e-6).numpy().tolist()
            buf.update_priorities(idx_h.tolist(), host)
            valid = model.update(idx_h, host)
        assert float(buf.max_priority) == model.max_priority, rnd
        p_after = adopt_p(("update", rnd))
        untouched = np.ones(cap, bool)
        untouched[idx_h[valid]] = False
        skipped_total += int((~valid).sum())
        assert np.array_equal(p_after[untouched].view(np.uint32), p_before[untouched].view(np.uint32)), rnd
    assert made > 2 * cap and wraps >= 2 and sampled >= 20 and skipped_total > 50
    assert model.beta > 1.0  # annealed past t_max
