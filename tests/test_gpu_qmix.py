"""GPU: the QMIX / VDN kernels alone (csrc/t2o_qmix.hip) against the fp64 restatement
(tests/qmix_model.py) and autograd on it.

Inputs: seeded N(0, 1) states and q, modules drawn with torch.manual_seed(0).  Bars
are the project's: forward 1e-5 normwise, gradients 3e-5 flat and 3e-5 per parameter
block on the block's own maximum (test_gpu_learner_masks.TOL, grad_blocks.FP32_BLOCK_BAR).
Shapes (A, B, T, M, H): one agent in one partial tile; a partial second 16-row tile;
S = 40 (no multiple of 16); the headline 8 agents; 16; 64 agents (S = 512, A·M = 2048:
the weights exceed LDS); M = 16, H = 32; and 280 rows, where the backward writes two
slabs (asserted through the slab-count function)."""
import functools
import types

import pytest
import torch

from tests import qmix_model
from tests.arena import Arena
from tests.gpu_util import argmax_preconditions, masked_avail, normwise, require_gpu

pytestmark = pytest.mark.gpu

FWD_BAR, GRAD_BAR, BLOCK_BAR = 1e-5, 3e-5, 3e-5
SHAPES = [(1, 2, 3, 32, 64), (3, 5, 4, 32, 64), (5, 4, 6, 32, 64), (8, 6, 5, 32, 64), (16, 3, 4, 32, 64),
          (64, 2, 3, 32, 64), (6, 3, 5, 16, 32), (8, 40, 7, 32, 64)]
POS = [("abs", 1.0), ("softplus", 0.5), ("quadratic", 1.0), ("identity", 1.0)]


def _args(A, M=32, H=64, **kw):
    from t2omca_amd.synthetic import make_args
    return types.SimpleNamespace(**{**vars(make_args(A, device="cpu", mixer="qmix", mixing_embed_dim=M,
                                                     hypernet_embed=H)), **kw})


@functools.lru_cache(maxsize=None)
def case(A, B, T, M, H, pos_func="abs", beta=1.0, gy_pos=False):
    """Two networks (different parameters), inputs and the fp64 reference, computed once."""
    from t2omca_amd.modules import QMixer
    torch.manual_seed(0)
    on = QMixer(_args(A, M, H, qmix_pos_func=pos_func, qmix_pos_func_beta=beta))
    tg = QMixer(_args(A, M, H, qmix_pos_func=pos_func, qmix_pos_func_beta=beta))
    g = torch.Generator().manual_seed(7)
    S = 8 * A
    states = torch.randn(B, T + 1, S, generator=g)
    q_on, q_tg = torch.randn(B, T, A, generator=g), torch.randn(B, T + 1, A, generator=g)
    gy = torch.randn(B, T, generator=g)
    if gy_pos:
        gy = gy.abs()
    p_on, p_tg = qmix_model.param_dict(on), qmix_model.param_dict(tg)
    pg = {k: v.clone().requires_grad_(True) for k, v in p_on.items()}
    q64 = q_on.double().requires_grad_(True)
    y_on = qmix_model.qmix_forward(pg, q64, states[:, :T].double(), pos_func, beta)
    y_tg = qmix_model.qmix_forward(p_tg, q_tg.double(), states.double(), pos_func, beta)
    grads = torch.autograd.grad((y_on * gy.double()).sum(), [q64] + list(pg.values()))
    flat = lambda m: torch.cat([p.detach().reshape(-1) for p in m.parameters()])  # noqa: E731
    return dict(shape=on.shape, flat_on=flat(on), flat_tg=flat(tg), states=states, q_on=q_on, q_tg=q_tg, gy=gy,
                y_on=y_on.detach(), y_tg=y_tg, gq=grads[0], gp=[g_.reshape(-1) for g_ in grads[1:]], on=on)


def run(c, dev="cuda"):
    from t2omca_amd import ops
    d = {k: c[k].to(dev) for k in ("flat_on", "flat_tg", "states", "q_on", "q_tg", "gy")}
    T = c["q_on"].shape[1]
    y_on, y_tg = ops.qmix_fwd(c["shape"], d["flat_on"], d["states"], d["q_on"], params_tg=d["flat_tg"],
                              qv_tg=d["q_tg"])
    gqv, slabs, nslab = ops.qmix_bwd(c["shape"], d["flat_on"], d["states"][:, :T], d["q_on"], d["gy"])
    gflat = ops.reduce_slabs(slabs, nslab, torch.empty_like(d["flat_on"]))
    torch.cuda.synchronize()
    return y_on, y_tg, gqv, gflat, nslab


@pytest.mark.parametrize("A,B,T,M,H", SHAPES)
def test_forward_backward(A, B, T, M, H):
    require_gpu()
    from t2omca_amd import ops
    c = case(A, B, T, M, H)
    y_on, y_tg, gqv, gflat, nslab = run(c)
    assert nslab == ops.qmix_slab_count(B, T)
    if B * T >= 280:
        assert nslab >= 2
    errs = dict(y_on=normwise(y_on, c["y_on"]), y_tg=normwise(y_tg, c["y_tg"]), gqv=normwise(gqv, c["gq"]),
                gflat=normwise(gflat, torch.cat(c["gp"])))
    blocks, off = {}, 0
    for (name, _), ref in zip(ops.qmix_param_blocks(A, 8 * A, M, H), c["gp"]):
        blocks[name] = normwise(gflat[off:off + ref.numel()], ref)
        off += ref.numel()
    assert off == gflat.numel() == c["shape"].n_params
    print(f"qmix {(A, B, T, M, H)}: {errs} worst block {max(blocks.items(), key=lambda kv: kv[1])}")
    assert errs["y_on"] <= FWD_BAR and errs["y_tg"] <= FWD_BAR, errs
    assert errs["gqv"] <= GRAD_BAR and errs["gflat"] <= GRAD_BAR, errs
    assert all(float(ref.abs().max()) > 0 for ref in c["gp"])  # no block identically zero
    assert max(blocks.values()) <= BLOCK_BAR, blocks
    again = run(c)
    assert all(torch.equal(a, b) for a, b in zip((y_on, y_tg, gqv, gflat), again[:4]))


@pytest.mark.parametrize("pos_func,beta", POS)
def test_pos_funcs(pos_func, beta):
    require_gpu()
    c = case(8, 6, 5, 32, 64, pos_func, beta)
    y_on, y_tg, gqv, gflat, _ = run(c)
    errs = dict(y_on=normwise(y_on, c["y_on"]), y_tg=normwise(y_tg, c["y_tg"]), gqv=normwise(gqv, c["gq"]),
                gflat=normwise(gflat, torch.cat(c["gp"])))
    print(f"qmix pos {pos_func}: {errs}")
    assert errs["y_on"] <= FWD_BAR and errs["y_tg"] <= FWD_BAR, errs
    assert errs["gqv"] <= GRAD_BAR and errs["gflat"] <= GRAD_BAR, errs


def test_monotone_gradient():
    require_gpu()
    c = case(8, 6, 5, 32, 64, "abs", 1.0, True)
    gqv = run(c)[2]
    assert bool((gqv >= 0).all()) and bool((gqv > 0).any())


# ---- the select kernel -------------------------------------------------------
def _select_inputs(B, T, A, NA=5, seed=11):
    g = torch.Generator().manual_seed(seed)
    T1 = T + 1
    q_on, q_tg = torch.randn(B, T1, A, NA, generator=g), torch.randn(B, T1, A, NA, generator=g)
    avail = masked_avail(B, T1, A, NA, seed=103)
    acts = torch.randint(0, NA, (B, T1, A, 1), generator=g)
    return q_on, q_tg, avail, acts


def _select_ref(q_on, q_tg, avail, acts, T):
    chosen = torch.gather(q_on[:, :T], 3, acts[:, :T]).squeeze(3)
    qm = q_on.clone()
    if avail is not None:
        qm[avail == 0] = -9999999
    tmax = torch.gather(q_tg, 3, qm.max(dim=3, keepdim=True)[1]).squeeze(3)
    return chosen, tmax


@pytest.mark.parametrize("A,B,T", [(3, 5, 4), (8, 6, 5), (64, 2, 3)])
@pytest.mark.parametrize("with_avail", [True, False])
def test_q_select(A, B, T, with_avail):
    require_gpu()
    from t2omca_amd import ops
    q_on, q_tg, avail, acts = _select_inputs(B, T, A)
    moved, gap = argmax_preconditions(q_on, avail)
    assert moved >= 0.25 and gap >= 1e-4, (moved, gap)
    # one constructed row with an exact tie: the lower index must win
    q_on[0, 1, A - 1, :] = torch.tensor([0.5, 2.0, 2.0, -1.0, 2.0])
    avail[0, 1, A - 1, :] = torch.tensor([1, 1, 1, 1, 1], dtype=torch.int32)
    av = avail if with_avail else None
    chosen, tmax = _select_ref(q_on, q_tg, av, acts, T)
    act_view = acts.cuda()[..., 0]  # the [B, T+1, A] view of the learner's [B, T+1, A, 1] actions
    (qv_on, y_on), (qv_tg, y_tg) = ops.q_select(q_on.cuda(), actions=act_view, avail=None if av is None else av.cuda(),
                                                T_on=T, q_tg=q_tg.cuda(), T_tg=T + 1, want_y=True)
    assert torch.equal(qv_on.cpu(), chosen) and torch.equal(qv_tg.cpu(), tmax)
    assert float(qv_tg[0, 1, A - 1]) == float(q_tg[0, 1, A - 1, 1])
    assert normwise(y_on, chosen.double().sum(2)) <= 1e-6 and normwise(y_tg, tmax.double().sum(2)) <= 1e-6
    # one network, qmode 1 on the target's Q (the Q(λ) taken values)
    qv_tk, none = ops.q_select(q_tg.cuda(), actions=act_view, T_on=T)
    assert none is None and torch.equal(qv_tk.cpu(), torch.gather(q_tg[:, :T], 3, acts[:, :T]).squeeze(3))
    assert torch.equal(ops.vdn_bwd(y_on, A=A), y_on.unsqueeze(2).expand(B, T, A))


# ---- memory contract -----------------------------------------------------------
@pytest.mark.parametrize("A,B,T", [(3, 5, 4), (16, 3, 4)])
def test_memory_contract(A, B, T):
    """States, actions and avail as strided views of [B, T+1, ...] parents carved from
    a poisoned arena (the q arrays and every output dense, as the header states): finite
    outputs, bit-equal to a run on dense tensors, and nothing written outside them."""
    require_gpu()
    from t2omca_amd import ops
    c = case(A, B, T, 32, 64)
    sh, S, NA, T1 = c["shape"], 8 * A, 5, T + 1
    q_on, q_tg, avail, acts = _select_inputs(B, T, A)
    dense = dict(states=c["states"].cuda(), q_on=q_on.cuda(), q_tg=q_tg.cuda(), avail=avail.cuda(),
                 acts=acts.cuda()[..., 0], gy=c["gy"].cuda(), p_on=c["flat_on"].cuda(), p_tg=c["flat_tg"].cuda())

    def go(t, outs=None):
        o = outs or {}
        sel = ops.q_select(t["q_on"], actions=t["acts"], avail=t["avail"], T_on=T, q_tg=t["q_tg"], T_tg=T1,
                           want_y=True, outs=o.get("sel"))
        (qv_on, _), (qv_tg, _) = sel
        ys = ops.qmix_fwd(sh, t["p_on"], t["states"], qv_on, params_tg=t["p_tg"], qv_tg=qv_tg, outs=o.get("ys"))
        gqv, slabs, nslab = ops.qmix_bwd(sh, t["p_on"], t["states"], qv_on, t["gy"], gqv=o.get("gqv"),
                                         slabs=o.get("slabs"), work=o.get("work"))
        gv = ops.vdn_bwd(t["gy"], gqv=o.get("gv"), A=A)
        return [sel[0][0], sel[0][1], sel[1][0], sel[1][1], ys[0], ys[1], gqv, slabs[:nslab * sh.n_params], gv]

    ref = go(dense)
    ar = Arena(8 << 20, "cuda")
    pad = 3  # steps of padding behind each episode of the parents
    t = dict(dense)
    t["states"] = ar.place(dense["states"], ((T1 + pad) * (S + 4), S + 4, 1), name="states")
    t["acts"] = ar.place(dense["acts"], ((T1 + pad) * (A + 1), A + 1, 1), name="actions")
    t["avail"] = ar.place(dense["avail"], ((T1 + pad) * A * NA + 7, A * NA, NA, 1), name="avail")
    for k in ("q_on", "q_tg", "gy", "p_on", "p_tg"):
        t[k] = ar.place(dense[k], name=k)
    nslab = ops.qmix_slab_count(B, T)
    outs = dict(sel=((ar.carve((B, T, A), name="qv_on"), ar.carve((B, T), name="ysel_on")),
                     (ar.carve((B, T1, A), name="qv_tg"), ar.carve((B, T1), name="ysel_tg"))),
                ys=(ar.carve((B, T), name="y_on"), ar.carve((B, T1), name="y_tg")),
                gqv=ar.carve((B, T, A), name="gqv"), slabs=ar.carve((nslab * sh.n_params,), name="slabs"),
                work=ar.carve((ops.qmix_work_floats(sh, B, T),), name="work"), gv=ar.carve((B, T, A), name="gv"))
    got = go(t, outs)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, ref)):
        assert bool(torch.isfinite(a).all()), i
        assert torch.equal(a, b), i
    assert bool(torch.isfinite(outs["work"]).all())  # every element of the work buffer written
    ar.check("qmix kernels")


# ---- the modules ---------------------------------------------------------------
def test_modules_autograd():
    require_gpu()
    from t2omca_amd.modules import VDNMixer
    c = case(8, 6, 5, 32, 64)
    m = c["on"].cuda()
    try:
        q = c["q_on"].cuda().requires_grad_(True)
        y = m(q, c["states"][:, :5].cuda())
        assert y.shape == (6, 5, 1)
        (y[..., 0] * c["gy"].cuda()).sum().backward()
        assert normwise(y[..., 0], c["y_on"]) <= FWD_BAR and normwise(q.grad, c["gq"]) <= GRAD_BAR
        for p, ref in zip(m.parameters(), c["gp"]):
            assert normwise(p.grad.reshape(-1), ref) <= BLOCK_BAR
        q2 = c["q_on"].cuda().requires_grad_(True)
        yv = VDNMixer()(q2, None)
        (yv[..., 0] * c["gy"].cuda()).sum().backward()
        assert yv.shape == (6, 5, 1) and normwise(yv[..., 0], c["q_on"].double().sum(2)) <= 1e-6
        assert torch.equal(q2.grad, c["gy"].cuda().unsqueeze(2).expand(6, 5, 8))
    finally:
        m.cpu()
