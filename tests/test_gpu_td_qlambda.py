"""GPU: t2o_td_qlambda (ops.td_qlambda) — t2o_td_loss with Peng's Q(λ) targets —
against the fp64 formula (tests/qlambda_model.build_q_lambda_targets) on the ragged
cases of test_gpu_td_loss._case plus an independent qtot_taken, for both kernels
(sequential / wave scan), both mask normalisations and mask_sum_acc.  fp32, bars
as test_gpu_td_loss.py: targets, gq, priorities 1e-5 normwise, loss 1e-5 relative,
Σ mask exact.

Beside the parity: the row stride of qtot_taken ([B, T] and a [B, T+1] buffer viewed)
does not change a bit; with qtot_taken := qtot_tgt[:, :T] the correction is an exact
zero and gq / targets / prio are torch.equal to ops.td_loss's; native mask dtypes give
the float-mask bits; an all-masked episode has priority 0, a zero gq row and finite
targets; T = 6000 runs on the wave scan and is a RuntimeError (T2O_EUNSUPPORTED: one
more staged row than TD(λ), T <= 4095) on the sequential kernel.
"""
import pytest
import torch

from tests.qlambda_model import build_q_lambda_targets
from tests.test_gpu_td_loss import _case, _nw

pytestmark = pytest.mark.gpu

ALGOS = ["sequential", "wave"]


def _taken(B, T, seed, cols=None):
    g = torch.Generator().manual_seed(seed + 9000)
    return torch.randn(B, cols or T, generator=g)


def _ref(qtot, qtgt, qk, reward, term, filled, w, gamma, lam):
    mask = filled.clone()
    mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
    tg = build_q_lambda_targets(reward, term, mask, qtgt, qk, gamma, lam)
    td = qtot - tg
    msum = mask.sum()
    loss = (w[:, None] * 0.5 * td ** 2 * mask).sum() / msum
    gq = w[:, None] * mask * td / msum
    prio = (td.abs() * mask).sum(1) / mask.sum(1).sqrt()
    return tg, gq, prio, loss, msum


def _c(t):
    return t.cuda().contiguous()


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("B,T", [(1, 1), (7, 5), (5, 64), (3, 127), (300, 60)])
def test_td_qlambda_matches_formula(B, T, algo):
    from t2omca_amd import ops
    qtot, qtgt, reward, term, filled, w = _case(B, T, B * 31 + T)
    qk = _taken(B, T, B * 31 + T)
    tg, gq, prio, loss, msum = _ref(*(x.double() for x in (qtot, qtgt, qk, reward, term, filled, w)), 0.99, 0.6)
    acc = torch.full((1,), 3.0, device="cuda")
    out = ops.td_qlambda(_c(qtot), _c(qtgt), _c(qk), _c(reward), _c(term), _c(filled), _c(w), gamma=0.99,
                         td_lambda=0.6, mask_sum=0.0, algo=algo, mask_sum_acc=acc)
    errs = dict(targets=_nw(out["targets"].cpu().double(), tg), gq=_nw(out["gq"].cpu().double(), gq),
                prio=_nw(out["prio"].cpu().double(), prio),
                loss=abs(float(out["loss"][0]) - float(loss)) / max(1.0, abs(float(loss))))
    print(f"B={B} T={T} {algo}:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert float(acc) == 3.0 + float(msum)  # Σ mask added into the caller's slot
    assert errs["targets"] < 1e-5 and errs["gq"] < 1e-5 and errs["prio"] < 1e-5, errs
    assert errs["loss"] <= 1e-5, errs
    assert float(out["loss"][1]) == float(msum)
    # externally supplied normaliser (data parallel): gq and loss scale by 1/mask_sum
    out2 = ops.td_qlambda(_c(qtot), _c(qtgt), _c(qk), _c(reward), _c(term), _c(filled), _c(w), gamma=0.99,
                          td_lambda=0.6, mask_sum=2.0 * float(msum), algo=algo)
    assert _nw(out2["gq"].cpu().double(), gq / 2) < 1e-5
    assert abs(float(out2["loss"][0]) - float(loss) / 2) <= 1e-5 * max(1.0, abs(float(loss)))
    assert float(out2["loss"][1]) == float(msum)
    assert torch.equal(out2["targets"], out["targets"]) and torch.equal(out2["prio"], out["prio"])
    # and the correction is in there: the TD(λ) targets are far away
    td = ops.td_loss(_c(qtot), _c(qtgt), _c(reward), _c(term), _c(filled), _c(w), gamma=0.99, td_lambda=0.6,
                     mask_sum=0.0, algo=algo)
    assert _nw(td["targets"].cpu().double(), tg) > 1e-2


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("B,T", [(1, 1), (7, 5), (37, 23)])
def test_td_qlambda_row_stride(B, T, algo):
    """qk_sb = T and qk_sb = T + 1 (a [B, T+1] buffer, whole or viewed [:, :T]): equal bits."""
    from t2omca_amd import ops
    qtot, qtgt, reward, term, filled, w = _case(B, T, 5)
    wide = _c(_taken(B, T, 5, cols=T + 1))
    dense = wide[:, :T].contiguous()
    assert B == 1 or (dense.stride(0) == T and wide.stride(0) == T + 1)
    args = (_c(reward), _c(term), _c(filled), _c(w))
    ref = ops.td_qlambda(_c(qtot), _c(qtgt), dense, *args, mask_sum=1.0, algo=algo)
    for qk in (wide, wide[:, :T]):
        out = ops.td_qlambda(_c(qtot), _c(qtgt), qk, *args, mask_sum=1.0, algo=algo)
        for k in ("gq", "targets", "prio"):
            assert torch.equal(out[k], ref[k]), k


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("B,T", [(1, 1), (7, 5), (5, 64), (3, 127), (300, 60)])
def test_td_qlambda_reduces_to_td_lambda(B, T, algo):
    """qtot_taken := qtot_tgt[:, :T]: the correction Q'_t - Qk_t is an exact zero, formed
    before r_t is added, so gq, targets and prio are t2o_td_loss's bit for bit."""
    from t2omca_amd import ops
    qtot, qtgt, reward, term, filled, w = _case(B, T, B * 31 + T)
    qt = _c(qtgt)
    args = (_c(reward), _c(term), _c(filled), _c(w))
    ref = ops.td_loss(_c(qtot), qt, *args, gamma=0.99, td_lambda=0.6, mask_sum=1.0, algo=algo)
    for qk in (qt[:, :T], qt[:, :T].contiguous()):
        out = ops.td_qlambda(_c(qtot), qt, qk, *args, gamma=0.99, td_lambda=0.6, mask_sum=1.0, algo=algo)
        for k in ("gq", "targets", "prio"):
            assert torch.equal(out[k], ref[k]), (k, int((out[k] != ref[k]).sum()))
        assert torch.equal(out["loss"][1:], ref["loss"][1:])


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("tdt,fdt", [(torch.uint8, torch.int64), (torch.bool, torch.int32)])
def test_td_qlambda_native_mask_dtypes(tdt, fdt, algo):
    from t2omca_amd import ops
    qtot, qtgt, reward, term, filled, w = _case(37, 23, 5)
    qk = _c(_taken(37, 23, 5))
    ref = ops.td_qlambda(_c(qtot), _c(qtgt), qk, _c(reward), _c(term), _c(filled), _c(w), mask_sum=0.0, algo=algo)
    # [B, T, 1] replay-style tensors viewed as [B, T] (non-unit outer strides)
    t3, f3 = _c(term.to(tdt)[..., None]), _c(filled.to(fdt)[..., None])
    out = ops.td_qlambda(_c(qtot), _c(qtgt), qk, _c(reward), t3[:, :, 0], f3[:, :, 0], _c(w), mask_sum=0.0,
                         algo=algo)
    for k in ("gq", "targets", "prio"):
        assert torch.equal(out[k], ref[k]), k
    # loss sums workgroup partials with float atomics (order varies); Σ mask is integral
    assert torch.allclose(out["loss"][:1], ref["loss"][:1], rtol=1e-6, atol=0.0)
    assert torch.equal(out["loss"][1:], ref["loss"][1:])


@pytest.mark.parametrize("algo", ALGOS)
def test_td_qlambda_all_masked_episode(algo):
    from t2omca_amd import ops
    B, T, dead, first = 9, 7, 2, 5
    qtot, qtgt, reward, term, filled, w = _case(B, T, 77)
    qk = _taken(B, T, 77)
    filled[dead], term[dead] = 0.0, 0.0
    filled[first], term[first] = 0.0, 0.0
    filled[first, 0] = term[first, 0] = 1.0
    tg, gq, prio, loss, msum = _ref(*(x.double() for x in (qtot, qtgt, qk, reward, term, filled, w)), 0.99, 0.6)
    live = torch.arange(B) != dead
    assert torch.isnan(prio[dead]) and torch.isfinite(prio[live]).all()
    acc = torch.zeros(1, device="cuda")
    out = ops.td_qlambda(_c(qtot), _c(qtgt), _c(qk), _c(reward), _c(term), _c(filled), _c(w), gamma=0.99,
                         td_lambda=0.6, mask_sum=0.0, algo=algo, mask_sum_acc=acc)
    o = {k: out[k].cpu().double() for k in ("gq", "targets", "prio", "loss")}
    assert float(o["prio"][dead]) == 0.0
    assert torch.equal(o["gq"][dead], torch.zeros(T, dtype=torch.float64))
    assert torch.isfinite(o["targets"]).all() and torch.isfinite(o["gq"]).all()
    assert float(o["loss"][1]) == float(msum) == float(acc)
    assert _nw(o["targets"][live], tg[live]) < 1e-5
    assert _nw(o["gq"][live], gq[live]) < 1e-5
    assert _nw(o["prio"][live], prio[live]) < 1e-5
    assert abs(float(o["loss"][0]) - float(loss)) <= 1e-5 * max(1.0, abs(float(loss)))
    # the episode that ends at step 0: one masked step, its target r_0 + Q'_0 - Qk_0
    want0 = (reward[first, :1] .double() + (qtgt[first, :1].double() - qk[first, :1].double()))
    assert _nw(o["targets"][first, :1], want0) < 1e-6


def test_td_qlambda_long_horizon():
    """T = 6000: the wave scan takes any T; the sequential kernel's LDS staging does not."""
    from t2omca_amd import ops
    B, T = 3, 6000
    qtot, qtgt, reward, term, filled, w = _case(B, T, 11)
    qk = _taken(B, T, 11)
    tg, gq, prio, loss, msum = _ref(*(x.double() for x in (qtot, qtgt, qk, reward, term, filled, w)), 0.99, 0.6)
    args = (_c(qtot), _c(qtgt), _c(qk), _c(reward), _c(term), _c(filled), _c(w))
    out = ops.td_qlambda(*args, mask_sum=0.0, algo="wave")
    assert _nw(out["targets"].cpu().double(), tg) < 1e-5 and _nw(out["prio"].cpu().double(), prio) < 1e-5
    assert _nw(out["gq"].cpu().double(), gq) < 1e-5
    with pytest.raises(RuntimeError):
        ops.td_qlambda(*args, mask_sum=0.0, algo="sequential")


def test_td_qlambda_rejects_bad_qtot_taken():
    from t2omca_amd import _lib, ops
    qtot, qtgt, reward, term, filled, w = _case(4, 6, 1)
    args = (_c(reward), _c(term), _c(filled), _c(w))
    for bad in (torch.zeros(4, 5), torch.zeros(3, 6), torch.zeros(4, 8), torch.zeros(4, 6, 1)):
        with pytest.raises(ValueError, match="qtot_taken"):
            ops.td_qlambda(_c(qtot), _c(qtgt), bad.cuda(), *args)
    with pytest.raises(ValueError, match="stride"):
        ops.td_qlambda(_c(qtot), _c(qtgt), torch.zeros(4, 12, device="cuda")[:, ::2], *args)
    # the C entry: T2O_EINVAL before any launch
    lib = _lib.lib()
    assert lib.t2o_td_qlambda(None, None) == -1
    assert lib.t2o_td_qlambda(_lib.ctypes.byref(_lib.TDQLambdaArgs(B=4, T=6)), None) == -1
