"""GPU: the two statistics entry points (csrc/t2o_stats.hip) against math.fsum.

Both sides sum identical doubles, so the only error is the kernel's own fp64
rounding: any fixed-order sum of n terms differs from the exact one by at most
n * 2^-52 * Σ|x_i| — that is the tolerance, nothing is measured.  (For
t2o_episode_stats, which adds its total to the accumulator, the pre-loaded value
is one more term.)  Repeated calls must agree bit for bit: the summation order
is a function of the element count alone.
"""
import ctypes
import math

import pytest
import torch

from tests.gpu_util import require_gpu

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
EINVAL = -1


def _wide(shape, g):
    """fp64 values of both signs spanning 12 orders of magnitude."""
    mag = 10.0 ** (12.0 * torch.rand(shape, generator=g, dtype=torch.float64) - 6.0)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()
    return mag * sign


def _bound(terms):
    return len(terms) * EPS * math.fsum(abs(x) for x in terms)


def _episode_inputs(n, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    reward, returns, info = _wide((n,), g), _wide((n,), g), _wide((n, 6), g)
    term = torch.ones(n, dtype=torch.uint8)
    term[1::3] = 0  # a third of the rows unterminated (n = 1: the one row terminated)
    info[term == 0, 4:] = float("nan")
    acc0 = _wide((10,), g)
    return reward, info, term, returns, acc0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 8195])
def test_episode_stats_against_fsum(n):
    require_gpu()
    from t2omca_amd import ops
    reward, info, term, returns, acc0 = _episode_inputs(n)
    dev = [t.cuda() for t in (reward, info, term, returns)]
    acc = acc0.cuda()
    ops.episode_stats(*dev, acc)
    again = acc0.cuda()
    ops.episode_stats(*dev, again)
    assert torch.equal(acc, again), "two calls on the same inputs must be bit-identical"
    got = acc.cpu().tolist()
    on = [i for i in range(n) if term[i]]
    assert n < 3 or len(on) < n
    cols = {1: returns.tolist(), 2: [reward[i].item() for i in on], 7: [1.0] * len(on)}
    for k, c in ((3, 0), (4, 1), (5, 2), (6, 3), (8, 4), (9, 5)):
        cols[k] = [info[i, c].item() for i in on]
    assert got[0] == acc0[0].item() + n  # counts every row, terminated or not
    for k, terms in cols.items():
        terms = terms + [acc0[k].item()]
        want = math.fsum(terms)
        err, bar = abs(got[k] - want), _bound(terms)
        print(f"n={n} acc[{k}]: |err| {err:.3e} bound {bar:.3e}")
        assert not math.isnan(got[k]) and err <= bar, (k, got[k], want)
    assert got[7] == acc0[7].item() + len(on)


def test_episode_stats_rejects_bad_arguments():
    require_gpu()
    from t2omca_amd import _lib
    reward, info, term, returns, acc0 = _episode_inputs(5)
    r, i, t, ret = (x.cuda() for x in (reward, info, term, returns))
    acc = acc0.cuda()
    lib, p, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    assert lib.t2o_episode_stats(p(r), p(i), p(t), p(ret), 0, p(acc), s) == EINVAL
    assert lib.t2o_episode_stats(p(r), p(i), p(t), p(ret), -3, p(acc), s) == EINVAL
    for hole in range(4):
        args = [p(r), p(i), p(t), p(ret)]
        args[hole] = None
        assert lib.t2o_episode_stats(*args, 5, p(acc), s) == EINVAL
    assert lib.t2o_episode_stats(p(r), p(i), p(t), p(ret), 5, None, s) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), acc0), "a refused call must not touch the accumulator"


# ---- t2o_td_stats -------------------------------------------------------------------
def _td_inputs(B, T, seed=0):
    g = torch.Generator().manual_seed(100 * B + T + seed)
    q = torch.randn(B, T, generator=g) * 3.0
    tgt = torch.randn(B, T, generator=g) * 3.0 + 0.5
    # [B, T+1, 1] as EpisodeBatch stores them; the kernels take the [:, :, 0] views
    term = torch.zeros(B, T + 1, 1, dtype=torch.uint8)
    filled = torch.ones(B, T + 1, 1, dtype=torch.int64)
    if B >= 3:
        term[0, T // 2, 0] = 1              # terminated mid-way: later steps masked
        filled[0, T // 2 + 1:, 0] = 0
        filled[1, max(1, T - 2):, 0] = 0    # an unfilled tail
        filled[2, :, 0] = 0                 # fully masked
    return q, tgt, term, filled


def _td_expected(q, tgt, term, filled):
    """[Σm, Σ|q-tgt|m, Σq m, Σtgt m]: fsum of the fp64 formula, and the bound of each."""
    B, T = q.shape
    q, tgt = q.double().tolist(), tgt.double().tolist()
    cols = [[], [], [], []]
    for b in range(B):
        for t in range(T):
            f = 1.0 if filled is None else float(filled[b, t])
            m = f * ((1.0 - (0.0 if term is None else float(term[b, t - 1]))) if t > 0 else 1.0)
            for c, x in zip(cols, (m, abs(q[b][t] - tgt[b][t]) * m, q[b][t] * m, tgt[b][t] * m)):
                c.append(x)
    return [math.fsum(c) for c in cols], [_bound(c) for c in cols]


def _check_td(q, tgt, term, filled, tag):
    from t2omca_amd import ops
    dq, dt = q.cuda(), tgt.cuda()
    dterm = None if term is None else term.cuda()
    dfill = None if filled is None else filled.cuda()
    vt = None if dterm is None else (dterm[:, :, 0] if dterm.dim() == 3 else dterm)
    vf = None if dfill is None else (dfill[:, :, 0] if dfill.dim() == 3 else dfill)
    out = ops.td_stats(dq, dt, vt, vf)
    again = ops.td_stats(dq, dt, vt, vf, out=torch.full((4,), 7.0, dtype=torch.float64, device="cuda"))
    assert torch.equal(out, again), "a repeated call must be bit-identical (and overwrite out)"
    ht = None if term is None else term.reshape(term.shape[0], -1)
    hf = None if filled is None else filled.reshape(filled.shape[0], -1)
    want, bars = _td_expected(q, tgt, ht, hf)
    got = out.cpu().tolist()
    for k in range(4):
        print(f"{tag} out[{k}]: |err| {abs(got[k] - want[k]):.3e} bound {bars[k]:.3e}")
        assert abs(got[k] - want[k]) <= bars[k], (tag, k, got[k], want[k])
    assert got[0] == want[0]  # a sum of 0/1 values is exact
    return dq, vt, vf, got


@pytest.mark.parametrize("B,T", [(1, 1), (3, 7), (5, 64), (33, 65)])
def test_td_stats_against_fsum(B, T):
    """uint8 terminated / int64 filled read in place as strided views, as the learner passes them."""
    require_gpu()
    from t2omca_amd import ops
    q, tgt, term, filled = _td_inputs(B, T)
    dq, vt, vf, got = _check_td(q, tgt, term, filled, f"({B},{T}) u8/i64 strided")
    assert vt.stride(0) == T + 1 and vf.stride(0) == T + 1  # rows T+1 apart, T of them read
    # Σm is td_loss's Σ mask on the same masks, exactly (both sum 0/1 values < 2^24)
    reward = torch.zeros(B, T + 1, 1, device="cuda")
    qt = torch.zeros(B, T + 1, device="cuda")
    for algo in ("wave", "sequential"):
        td = ops.td_loss(dq, qt, reward[:, :, 0], vt, vf, algo=algo)
        assert float(td["loss"][1]) == got[0], algo


@pytest.mark.parametrize("B,T", [(3, 7), (33, 65)])
def test_td_stats_float_masks_and_null_masks(B, T):
    require_gpu()
    q, tgt, term, filled = _td_inputs(B, T)
    _check_td(q, tgt, term[:, :T, 0].float().contiguous(), filled[:, :T, 0].float().contiguous(),
              f"({B},{T}) f32 dense")
    _, _, _, got = _check_td(q, tgt, None, None, f"({B},{T}) null masks")
    assert got[0] == B * T


def test_td_stats_rejects_bad_arguments():
    require_gpu()
    from t2omca_amd import _lib
    lib = _lib.lib()
    q = torch.randn(3, 4, device="cuda")
    out0 = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    out = out0.cuda()
    s = _lib.stream_ptr()

    def call(**kw):
        kw = {**dict(qtot=q.data_ptr(), targets=q.data_ptr(), B=3, T=4, out=out.data_ptr()), **kw}
        return lib.t2o_td_stats(ctypes.byref(_lib.TDStatsArgs(**kw)), s)

    assert lib.t2o_td_stats(None, s) == EINVAL
    assert call(qtot=None) == EINVAL and call(targets=None) == EINVAL and call(out=None) == EINVAL
    assert call(B=0) == EINVAL and call(T=0) == EINVAL and call(B=-1) == EINVAL
    assert call(term=q.data_ptr(), term_dtype=9) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), out0)
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(out.cpu(), out0)
