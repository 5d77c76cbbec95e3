"""GPU: the QPLEX kernels alone (csrc/t2o_qplex.hip) against the fp64 restatement
(tests/qplex_model.py) and autograd on it.

Inputs: seeded N(0, 1) states, q and m and uniform joint actions u, drawn independently
(q − m takes both signs: asserted), modules drawn with torch.manual_seed(0).  Bars are the
project's: forward 1e-5 normwise, gradients 3e-5 flat and per parameter block
(test_gpu_learner_masks.TOL, grad_blocks.assert_blocks_fp32 with its fitness condition).
Shapes (A, B, T, NA, S, K): 20 rows with A below the MFMA K (a padded second tile); the
headline 8 agents; S = 50 (no multiple of 4), NA = 16 and one kernel; 16 agents; 64
agents with S = 512 (the largest weights).  At every shape: y for parts 1, 2, 3 of the
online rows, two networks in one launch (T and T + 1 steps), dL/dq, the flat parameter
gradient and every block, two runs bit-equal, and the same from a parameter buffer
offset by one float (the 4-byte-load instances).

MEASURED on an MI355X (normwise; the offset-by-one-float runs gave the same figures):

  (A, B, T, NA, S, K)      y1      y2      y3      y_tg    dL/dq   grad    worst block (smallest share)
  (3, 5, 4, 5, 24, 4)      1.1e-7  2.3e-7  1.9e-7  1.7e-7  1.9e-7  9.7e-8  2.4e-6 key_extractors.3.2.bias (8.9e-4)
  (8, 6, 5, 5, 64, 4)      1.4e-7  1.8e-7  1.8e-7  2.5e-7  2.4e-7  1.2e-7  7.1e-7 V.2.bias (1.1e-3)
  (5, 4, 6, 16, 50, 1)     1.1e-7  2.3e-7  2.3e-7  1.7e-7  1.9e-7  1.1e-7  4.3e-7 action_extractors.0.2.weight (2.7e-3)
  (16, 3, 4, 5, 128, 4)    1.6e-7  4.0e-7  3.0e-7  4.5e-7  2.9e-7  2.2e-7  2.4e-6 key_extractors.3.2.bias (1.1e-3)
  (64, 2, 3, 5, 512, 2)    2.6e-7  3.6e-7  3.4e-7  3.6e-7  3.1e-7  4.8e-7  2.1e-6 key_extractors.0.2.bias (1.8e-3)
  one part alone at (8, 6, 5): y_v grad 1.2e-7, dL/dq 2.4e-7; y_adv grad 2.8e-7, dL/dq exactly 0, the other
  part's parameters exactly 0.  QPlexMixer autograd: y 1.4e-7 / 1.8e-7, the same gradients.
"""
import functools
import types

import pytest
import torch

from tests import qplex_model
from tests.arena import Arena
from tests.gpu_util import argmax_preconditions, masked_avail, normwise, require_gpu
from tests.grad_blocks import assert_blocks_fp32

pytestmark = pytest.mark.gpu

FWD_BAR, GRAD_BAR = 1e-5, 3e-5
SHAPES = [(3, 5, 4, 5, 24, 4), (8, 6, 5, 5, 64, 4), (5, 4, 6, 16, 50, 1), (16, 3, 4, 5, 128, 4), (64, 2, 3, 5, 512, 2)]


def _args(A, NA, S, K, **kw):
    from t2omca_amd.synthetic import make_args
    return types.SimpleNamespace(**{**vars(make_args(A, device="cpu", mixer="dmaq")), "n_actions": NA,
                                    "state_shape": S, "num_kernel": K, **kw})


@functools.lru_cache(maxsize=None)
def case(A, B, T, NA, S, K):
    """Two networks (different parameters), inputs and the fp64 reference, computed once."""
    from t2omca_amd.modules import QPlexMixer
    torch.manual_seed(0)
    on, tg = QPlexMixer(_args(A, NA, S, K)), QPlexMixer(_args(A, NA, S, K))
    g = torch.Generator().manual_seed(7)
    states = torch.randn(B, T + 1, S, generator=g)
    rows = {}
    for n, Tn in (("on", T), ("tg", T + 1)):
        rows[n] = (torch.randn(B, Tn, A, generator=g), torch.randn(B, Tn, A, generator=g),
                   torch.randint(0, NA, (B, Tn, A), generator=g, dtype=torch.int32))
    gy = torch.randn(B, T, generator=g)
    d = rows["on"][0] - rows["on"][1]
    assert float((d > 0).float().mean()) > 0.2 and float((d < 0).float().mean()) > 0.2  # both signs of q − m
    p_on, p_tg = qplex_model.param_dict(on), qplex_model.param_dict(tg)
    pg = {k: v.clone().requires_grad_(True) for k, v in p_on.items()}
    q, m, u = rows["on"]
    q64 = q.double().requires_grad_(True)
    y_v, y_adv = qplex_model.qplex_parts(pg, q64, m.double(), u, states[:, :T].double(), NA)
    qt, mt, ut = rows["tg"]
    y_tg = qplex_model.qplex_forward(p_tg, qt.double(), mt.double(), ut, states.double(), NA)
    grads = {}
    for parts, y in ((1, y_v), (2, y_adv), (3, y_v + y_adv)):
        gs = torch.autograd.grad((y * gy.double()).sum(), [q64] + list(pg.values()), retain_graph=True,
                                 allow_unused=True)
        gs = [torch.zeros_like(x) if g_ is None else g_ for g_, x in zip(gs, [q64] + list(pg.values()))]
        grads[parts] = (gs[0], torch.cat([g_.reshape(-1) for g_ in gs[1:]]))
    flat = lambda mod: torch.cat([p.detach().reshape(-1) for p in mod.parameters()])  # noqa: E731
    return dict(shape=on.shape, flat_on=flat(on), flat_tg=flat(tg), states=states, rows=rows, gy=gy,
                y={1: y_v.detach(), 2: y_adv.detach(), 3: (y_v + y_adv).detach()}, y_tg=y_tg, grads=grads, p_on=p_on,
                on=on)


def _dev(c, offset=0):
    """The case's tensors on the device; offset: the parameter buffers start `offset` floats into an allocation."""
    d = dict(states=c["states"].cuda(), gy=c["gy"].cuda(), on=tuple(t.cuda() for t in c["rows"]["on"]),
             tg=tuple(t.cuda() for t in c["rows"]["tg"]))
    for k in ("flat_on", "flat_tg"):
        buf = torch.zeros(c[k].numel() + offset, device="cuda")
        buf[offset:].copy_(c[k])
        d[k] = buf[offset:]
        assert d[k].data_ptr() % 16 == 4 * offset
    return d


def run(c, offset=0):
    from t2omca_amd import ops
    d, sh = _dev(c, offset), c["shape"]
    T = c["gy"].shape[1]
    ys = {parts: ops.qplex_fwd(sh, d["flat_on"], d["states"], *d["on"], parts=parts) for parts in (1, 2)}
    ys[3], y_tg = ops.qplex_fwd(sh, d["flat_on"], d["states"], *d["on"], params_tg=d["flat_tg"], qv_tg=d["tg"][0],
                                qmax_tg=d["tg"][1], act_tg=d["tg"][2], parts=3)
    gqv, slabs, nslab = ops.qplex_bwd(sh, d["flat_on"], d["states"][:, :T], *d["on"], d["gy"], parts=3)
    gflat = ops.reduce_slabs(slabs, nslab, torch.empty_like(d["flat_on"]))
    torch.cuda.synchronize()
    return ys[1], ys[2], ys[3], y_tg, gqv, gflat


@pytest.mark.parametrize("A,B,T,NA,S,K", SHAPES)
def test_forward_backward(A, B, T, NA, S, K):
    require_gpu()
    from t2omca_amd import ops
    c = case(A, B, T, NA, S, K)
    out = run(c)
    y1, y2, y3, y_tg, gqv, gflat = out
    gq_ref, gp_ref = c["grads"][3]
    errs = dict(y1=normwise(y1, c["y"][1]), y2=normwise(y2, c["y"][2]), y3=normwise(y3, c["y"][3]),
                y_tg=normwise(y_tg, c["y_tg"]), gqv=normwise(gqv, gq_ref), gflat=normwise(gflat, gp_ref))
    print(f"qplex {(A, B, T, NA, S, K)}:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(errs[k] <= FWD_BAR for k in ("y1", "y2", "y3", "y_tg")), errs
    assert errs["gqv"] <= GRAD_BAR and errs["gflat"] <= GRAD_BAR, errs
    assert gflat.numel() == c["shape"].n_params == sum(v.numel() for v in c["p_on"].values())
    assert [k for k, _ in ops.qplex_param_blocks(A, S, NA, K=K)] == list(c["p_on"])
    assert_blocks_fp32(gflat, gp_ref, {}, c["p_on"], tag=f"qplex {(A, B, T, NA, S, K)}")
    # bit-reproducible, and the 4-byte-load instances (a buffer offset by one float) agree with the fp64 model too
    assert all(torch.equal(a, b) for a, b in zip(out, run(c)))
    o1 = run(c, offset=1)
    e1 = dict(y3=normwise(o1[2], c["y"][3]), y_tg=normwise(o1[3], c["y_tg"]), gqv=normwise(o1[4], gq_ref),
              gflat=normwise(o1[5], gp_ref))
    print(f"qplex {(A, B, T, NA, S, K)} offset by one float:", {k: f"{v:.2e}" for k, v in e1.items()})
    assert e1["y3"] <= FWD_BAR and e1["y_tg"] <= FWD_BAR and e1["gqv"] <= GRAD_BAR and e1["gflat"] <= GRAD_BAR, e1
    assert_blocks_fp32(o1[5], gp_ref, {}, c["p_on"], tag=f"qplex offset {(A, B, T, NA, S, K)}")


@pytest.mark.parametrize("parts", [1, 2])
def test_backward_of_one_part(parts):
    """The gradients of y_v alone and of y_adv alone (what QPlexMixer.forward's two modes
    differentiate): dL/dq = gy · w, or zero; the other part's parameters get exact zeros."""
    require_gpu()
    from t2omca_amd import ops
    A, B, T, NA, S, K = 8, 6, 5, 5, 64, 4
    c = case(A, B, T, NA, S, K)
    d, sh = _dev(c), c["shape"]
    gqv, slabs, nslab = ops.qplex_bwd(sh, d["flat_on"], d["states"][:, :T], *d["on"], d["gy"], parts=parts)
    gflat = ops.reduce_slabs(slabs, nslab, torch.empty_like(d["flat_on"])).cpu()
    gq_ref, gp_ref = c["grads"][parts]
    n_v = sum(v.numel() for k, v in c["p_on"].items() if not k.startswith("si_weight."))
    lo, hi = (0, n_v) if parts == 1 else (n_v, gflat.numel())
    eg, eq = normwise(gflat[lo:hi], gp_ref[lo:hi]), normwise(gqv, gq_ref) if parts == 1 else float(gqv.abs().max())
    print(f"qplex parts {parts}: grad {eg:.2e} dL/dq {eq:.2e}")
    assert eg <= GRAD_BAR and eq <= GRAD_BAR
    other = torch.cat([gflat[:lo], gflat[hi:]])
    assert not other.any() and not gp_ref[:lo].any() and not gp_ref[hi:].any()


# ---- the select kernel -------------------------------------------------------
def _select_inputs(B, T, A, NA=5, seed=11):
    g = torch.Generator().manual_seed(seed)
    T1 = T + 1
    q_on, q_tg = torch.randn(B, T1, A, NA, generator=g), torch.randn(B, T1, A, NA, generator=g)
    avail = masked_avail(B, T1, A, NA, seed=103)
    acts = torch.randint(0, NA, (B, T1, A, 1), generator=g)
    return q_on, q_tg, avail, acts


def _masked(q, avail):
    qm = q.clone()
    if avail is not None:
        qm[avail == 0] = -9999999
    return qm.max(dim=3)


@pytest.mark.parametrize("A,B,T", [(3, 5, 4), (8, 6, 5), (64, 2, 3)])
@pytest.mark.parametrize("with_avail", [True, False])
def test_select(A, B, T, with_avail):
    require_gpu()
    from t2omca_amd import ops
    q_on, q_tg, avail, acts = _select_inputs(B, T, A)
    moved, gap = argmax_preconditions(q_on, avail)
    assert moved >= 0.25 and gap >= 1e-4, (moved, gap)
    # one constructed row with an exact tie (the lower index must win), one with every action but one masked
    q_on[0, 1, A - 1, :] = torch.tensor([0.5, 2.0, 2.0, -1.0, 2.0])
    avail[0, 1, A - 1, :] = 1
    q_on[1, 2, 0, :] = torch.tensor([-3.0, 4.0, 5.0, 6.0, 7.0])
    q_tg[1, 2, 0, :] = torch.tensor([-2.0, 1.0, 2.0, 3.0, 4.0])
    avail[1, 2, 0, :] = torch.tensor([1, 0, 0, 0, 0], dtype=torch.int32)
    acts[1, 2, 0, 0] = 3  # (an unavailable action taken: the chosen Q exceeds the masked maximum)
    av = avail if with_avail else None
    (m_on, _), (m_tg, _) = _masked(q_on, av), _masked(q_tg, av)
    a_star = _masked(q_on, av)[1]
    chosen = torch.gather(q_on[:, :T], 3, acts[:, :T]).squeeze(3)
    tq = torch.gather(q_tg, 3, a_star.unsqueeze(3)).squeeze(3)
    act_view = acts.cuda()[..., 0]  # the [B, T+1, A] view of the learner's [B, T+1, A, 1] actions
    on, tg = ops.qplex_select(q_on.cuda(), actions=act_view, avail=None if av is None else av.cuda(), T_on=T,
                              q_tg=q_tg.cuda(), T_tg=T + 1)
    assert torch.equal(on[0].cpu(), chosen) and torch.equal(on[1].cpu(), m_on[:, :T])
    assert torch.equal(on[2].cpu().long(), acts[:, :T, :, 0]) and on[2].dtype == torch.int32
    assert torch.equal(tg[0].cpu(), tq) and torch.equal(tg[1].cpu(), m_tg) and torch.equal(tg[2].cpu().long(), a_star)
    assert int(tg[2][0, 1, A - 1]) == 1
    if with_avail:
        assert float(on[0][1, 2, 0]) == 6.0 and float(on[1][1, 2, 0]) == -3.0  # q > m
        assert int(tg[2][1, 2, 0]) == 0 and float(tg[0][1, 2, 0]) == -2.0 == float(tg[1][1, 2, 0])
    # one network, qmode 1 on the target's Q (the Q(λ) taken rows): its own maxima
    tk = ops.qplex_select(q_tg.cuda(), actions=act_view, avail=None if av is None else av.cuda(), T_on=T)
    assert torch.equal(tk[0].cpu(), torch.gather(q_tg[:, :T], 3, acts[:, :T]).squeeze(3))
    assert torch.equal(tk[1].cpu(), m_tg[:, :T]) and torch.equal(tk[2].cpu().long(), acts[:, :T, :, 0])


# ---- memory contract -----------------------------------------------------------
@pytest.mark.parametrize("A,B,T,NA,S,K", [SHAPES[0], SHAPES[2], SHAPES[3]])
def test_memory_contract(A, B, T, NA, S, K):
    """States, actions and avail as strided views of [B, T+1, ...] parents carved from a
    poisoned arena (everything else dense, as the header states): finite outputs,
    bit-equal to a run on dense tensors, and nothing written outside them."""
    require_gpu()
    from t2omca_amd import ops
    c = case(A, B, T, NA, S, K)
    sh, T1 = c["shape"], T + 1
    q_on, q_tg, avail, acts = _select_inputs(B, T, A, NA)
    dense = dict(states=c["states"].cuda(), q_on=q_on.cuda(), q_tg=q_tg.cuda(), avail=avail.cuda(),
                 acts=acts.cuda()[..., 0], gy=c["gy"].cuda(), p_on=c["flat_on"].cuda(), p_tg=c["flat_tg"].cuda())

    def go(t, outs=None):
        o = outs or {}
        on, tg = ops.qplex_select(t["q_on"], actions=t["acts"], avail=t["avail"], T_on=T, q_tg=t["q_tg"], T_tg=T1,
                                  outs=o.get("sel"))
        ys = ops.qplex_fwd(sh, t["p_on"], t["states"], *on, params_tg=t["p_tg"], qv_tg=tg[0], qmax_tg=tg[1],
                           act_tg=tg[2], outs=o.get("ys"))
        gqv, slabs, nslab = ops.qplex_bwd(sh, t["p_on"], t["states"], *on, t["gy"], gqv=o.get("gqv"),
                                          slabs=o.get("slabs"), work=o.get("work"))
        return [*on, *tg, ys[0], ys[1], gqv, slabs[:nslab * sh.n_params]]

    ref = go(dense)
    ar = Arena(16 << 20, "cuda")
    pad = 3  # steps of padding behind each episode of the parents
    t = dict(dense)
    sp = (S + 3) // 4 * 4 + 4
    t["states"] = ar.place(dense["states"], ((T1 + pad) * sp, sp, 1), name="states")
    t["acts"] = ar.place(dense["acts"], ((T1 + pad) * (A + 1), A + 1, 1), name="actions")
    t["avail"] = ar.place(dense["avail"], ((T1 + pad) * A * NA + 7, A * NA, NA, 1), name="avail")
    for k in ("q_on", "q_tg", "gy", "p_on", "p_tg"):
        t[k] = ar.place(dense[k], name=k)
    nslab = ops.qplex_slab_count(B, T)

    def sel(Tn, n):
        return (ar.carve((B, Tn, A), name="qv_" + n), ar.carve((B, Tn, A), name="qmax_" + n),
                ar.carve((B, Tn, A), torch.int32, name="act_" + n))
    outs = dict(sel=(sel(T, "on"), sel(T1, "tg")), ys=(ar.carve((B, T), name="y_on"), ar.carve((B, T1), name="y_tg")),
                gqv=ar.carve((B, T, A), name="gqv"), slabs=ar.carve((nslab * sh.n_params,), name="slabs"),
                work=ar.carve((ops.qplex_work_floats(sh, B, T),), name="work"))
    got = go(t, outs)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, ref)):
        assert bool(torch.isfinite(a.float()).all()), i
        assert torch.equal(a, b), i
    assert bool(torch.isfinite(outs["work"]).all())  # every element of the work buffer written
    ar.check("qplex kernels")


# ---- the module ----------------------------------------------------------------
def test_module_autograd():
    require_gpu()
    A, B, T, NA, S, K = 8, 6, 5, 5, 64, 4
    c = case(A, B, T, NA, S, K)
    m = c["on"].cuda()
    try:
        q0, mx, u = (t.cuda() for t in c["rows"]["on"])
        st, gy = c["states"][:, :T].cuda(), c["gy"].cuda()
        onehot = torch.nn.functional.one_hot(u.long(), NA).float()
        for parts, kw in ((1, dict(is_v=True)), (2, dict(actions=onehot, max_q_i=mx)), (2, dict(actions=u, max_q_i=mx))):
            m.zero_grad()
            q = q0.clone().requires_grad_(True)
            y = m(q, st, **kw)
            assert y.shape == (B, T, 1)
            (y[..., 0] * gy).sum().backward()
            gq_ref, gp_ref = c["grads"][parts]
            got = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
            ey, eq, eg = normwise(y[..., 0], c["y"][parts]), float((q.grad.cpu() - gq_ref).abs().max()), \
                normwise(got, gp_ref)
            print(f"QPlexMixer parts {parts}: y {ey:.2e} dL/dq (abs) {eq:.2e} grad {eg:.2e}")
            assert ey <= FWD_BAR and eg <= GRAD_BAR and eq <= GRAD_BAR * float(c["grads"][1][0].abs().max())
    finally:
        m.cpu()
