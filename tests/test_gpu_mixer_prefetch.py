"""GPU: the mixer unroll at the shapes where fetching weight fragments one product
ahead of their MFMA (mixer_block_fwd_pf, csrc/t2o_mixer_block.hpp) can go wrong,
against the CPU oracle (oracle/ref_model) and against a second run of itself.

The forward of the bf16 single-query-tile 8-agent instances (exact, runtime capacity,
run-time head) carries the head fragments of the next product across products, blocks
and the step boundary: the last LN2 of step t covers the fetch of the state embedding's
fragments and block 0's M for step t + 1, and the fetch after a network's last step
reads the same LDS image.  Every case runs both networks in one launch, as the TD
update does — online: chosen-action gather, T steps; target: double-Q argmax under an
avail mask, T + 1 steps — both from non-zero hyper tokens.  Shapes (A, B, T): (8, 1, 1)
no step boundary; (8, 3, 2) one boundary, fewer episodes than a workgroup's 8 waves;
(8, 9, 5) two workgroups, the second with one live wave; (5, 7, 2) / (5, 7, 5) the
runtime-agent instance; (3, 6, 2) an exact instance that keeps the reads at their use;
(16, 5, 4) multi-tile, unchanged.  At 8 agents also the softplus and identity mixing
heads (qmix_pos_func), which run the exact instance with the head as a run-time
parameter.

Checked: y, hw and qv of both networks, xout and xmid of the online one (the target
network stores neither), against ref_model.mixer_unroll / ref_model.block in fp64; one
(8, 3, 2) case per precision goes on through the BPTT (mixer_unroll_bwd, unpack_grads),
which reads the stored xmid / hw.  Every case runs twice and the runs must be bit-equal.

Bars (normwise max|Δ| / max|ref|): fp32 TOL_F32 of tests/test_gpu_mixer.py (1e-5),
gradients 2e-5.  The suite had no bf16 bar for the mixer's own outputs, so the bf16
bars are twice the largest error the parent commit (reads at their use) gave on these
same inputs, per quantity (BF16_BARS; measured values beside them).  The margin only
separates rounding from a wrong fragment: the change is bit-identical to the parent."""
import dataclasses
import functools

import pytest
import torch

from oracle import ref_model
from tests.gpu_util import flat_from_dict, normwise, require_gpu
from tests.test_gpu_mixer import TOL_F32, _shape

pytestmark = pytest.mark.gpu

SHAPES = [(8, 1, 1), (8, 3, 2), (8, 9, 5), (5, 7, 2), (5, 7, 5), (3, 6, 2), (16, 5, 4)]
CASES = [(A, B, T, "abs") for A, B, T in SHAPES] + [(8, B, T, head) for head in ("softplus", "identity")
                                                     for A, B, T in SHAPES if A == 8]
TOL_GRAD_F32 = 2e-5
# bf16: 2 x the parent commit's largest error over CASES (forward) / on the BPTT case.
# Measured on an MI355X, parent: y 2.33e-3, hw 4.88e-3, xout 3.63e-3, xmid 3.10e-3;
# grad 5.60e-2, gqv 7.96e-4, ghid 1.19e-2, ghw0 3.38e-3 — and this change the same to
# the last digit in every case (fp32, both: forward <= 4.3e-7, gradients <= 3.3e-7).
BF16_BARS = dict(y=4.66e-3, hw=9.76e-3, xout=7.26e-3, xmid=6.20e-3, grad=1.12e-1, gqv=1.59e-3, ghid=2.38e-2,
                 ghw0=6.76e-3)


def _cfg(A, head):
    return dict(n_agents=A, n_entities=A, state_entity_feats=8, mixer_emb=32, mixer_heads=3, mixer_depth=2,
                ff_hidden_mult=4, qmix_pos_func=head, qmix_pos_func_beta=0.5)


def _gpu_shape(cfg, prec):
    from t2omca_amd._lib import POS_FUNCS
    return dataclasses.replace(_shape(cfg), prec=1 if prec == "bf16" else 0,
                               pos_func=POS_FUNCS.get(cfg["qmix_pos_func"], 3), pos_beta=cfg["qmix_pos_func_beta"])


def _query_rows(p, cfg, hidden, states, hw0, hw):
    """The oracle's query rows (the last A + 3 tokens) after block 0 and after block 1,
    per step: xmid [B, T, 1, A + 3, E] and xout [B, T, A + 3, E].  hw: mixer_unroll's."""
    A, B, T = cfg["n_agents"], hidden.shape[0], hidden.shape[1]
    mids, outs = [], []
    for t in range(T):
        embs = ref_model._lin(states[:, t].reshape(B, A, 8), p, "feat_embedding")
        x0 = torch.cat((embs, hidden[:, t], hw0 if t == 0 else hw[:, t - 1]), 1)
        x1 = ref_model.block(p, "transformer.tblocks.0.", x0, x0, cfg["mixer_heads"])
        x2 = ref_model.block(p, "transformer.tblocks.1.", x1, x0, cfg["mixer_heads"])
        mids.append(x1[:, -A - 3:])
        outs.append(x2[:, -A - 3:])
    return torch.stack(mids, 1).unsqueeze(2), torch.stack(outs, 1)


@functools.lru_cache(maxsize=None)
def _case(A, B, T, head):
    """Inputs and the fp64 oracle's outputs (and the online network's gradients),
    computed once per case and left unchanged."""
    cfg = _cfg(A, head)
    g = torch.Generator().manual_seed(1000 * A + 10 * B + T)
    Tq = T + 1
    p_on = ref_model.init_params("mixer", cfg, 41 + A)
    p_tg = ref_model.init_params("mixer", cfg, 42 + A)
    c = dict(cfg=cfg, p_on=p_on, p_tg=p_tg,
             states=torch.randn(B, Tq, A * 8, generator=g), h_on=torch.randn(B, Tq, A, 32, generator=g),
             h_tg=torch.randn(B, Tq, A, 32, generator=g), q_on=torch.randn(B, Tq, A, 5, generator=g),
             q_tg=torch.randn(B, Tq, A, 5, generator=g), actions=torch.randint(0, 5, (B, Tq, A, 1), generator=g),
             hw0_on=torch.randn(B, 3, 32, generator=g), hw0_tg=torch.randn(B, 3, 32, generator=g),
             gy=torch.randn(B, T, generator=g), ghw=torch.randn(B, T, 3, 32, generator=g))
    avail = (torch.rand(B, Tq, A, 5, generator=g) > 0.3).int()
    avail[..., 0] = 1
    c["avail"] = avail
    c["chosen"] = torch.gather(c["q_on"][:, :T], 3, c["actions"][:, :T]).squeeze(3)
    qd = c["q_on"].clone()
    qd[avail == 0] = -9999999
    c["tmax"] = torch.gather(c["q_tg"], 3, qd.max(dim=3, keepdim=True)[1]).squeeze(3)
    # online network, with gradients (the BPTT cases)
    pd = {k: v.double().requires_grad_(True) for k, v in p_on.items()}
    qv = c["chosen"].double().requires_grad_(True)
    hid = c["h_on"][:, :T].double().requires_grad_(True)
    hw0 = c["hw0_on"].double().requires_grad_(True)
    y, hw = ref_model.mixer_unroll(pd, qv, hid, c["states"][:, :T].double(), hw0, cfg=cfg)
    ((y * c["gy"].double()).sum() + (hw * c["ghw"].double()).sum()).backward()
    with torch.no_grad():
        xmid, xout = _query_rows(pd, cfg, hid, c["states"][:, :T].double(), hw0, hw)
    c["on"] = dict(y=y.detach(), hw=hw.detach(), xmid=xmid, xout=xout,
                   grad=torch.cat([v.grad.reshape(-1) for v in pd.values()]), gqv=qv.grad, ghid=hid.grad,
                   ghw0=hw0.grad)
    with torch.no_grad():
        y, hw = ref_model.mixer_unroll({k: v.double() for k, v in p_tg.items()}, c["tmax"].double(),
                                       c["h_tg"].double(), c["states"].double(), c["hw0_tg"].double(), cfg=cfg)
    c["tg"] = dict(y=y, hw=hw)
    return c


def _forward(c, shape, T):
    from t2omca_amd import ops
    packs = [ops.pack_params(shape, flat_from_dict(p).cuda()) for p in (c["p_on"], c["p_tg"])]
    o_on, o_tg = ops.mixer_unroll_fwd(shape, packs[0], c["states"].cuda(), c["h_on"].cuda(), qmode_on=1,
                                      q_on=c["q_on"].cuda(), actions=c["actions"].cuda()[..., 0],
                                      avail=c["avail"].cuda(), hw0_on=c["hw0_on"].cuda(), T_on=T, pack_tg=packs[1],
                                      hid_tg=c["h_tg"].cuda(), qmode_tg=2, q_tg=c["q_tg"].cuda(),
                                      hw0_tg=c["hw0_tg"].cuda(), T_tg=T + 1)
    torch.cuda.synchronize()
    return packs, o_on, o_tg


def _bar(prec, k):
    if prec == "fp32":
        return TOL_F32 if k in ("y", "hw", "xout", "xmid") else TOL_GRAD_F32
    return BF16_BARS[k]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("A,B,T,head", CASES)
def test_mixer_fwd_prefetch_vs_oracle(A, B, T, head, prec):
    require_gpu()
    c = _case(A, B, T, head)
    shape = _gpu_shape(c["cfg"], prec)
    _, o_on, o_tg = _forward(c, shape, T)
    _, r_on, r_tg = _forward(c, shape, T)
    assert torch.equal(o_on["qv"].cpu(), c["chosen"])
    assert torch.equal(o_tg["qv"].cpu(), c["tmax"])
    errs = {f"on.{k}": (k, normwise(o_on[k], c["on"][k])) for k in ("y", "hw", "xout", "xmid")}
    errs.update({f"tg.{k}": (k, normwise(o_tg[k], c["tg"][k])) for k in ("y", "hw")})
    print(f"mixer fwd A={A} B={B} T={T} {head} {prec}: " + " ".join(f"{n} {e:.2e}" for n, (_, e) in errs.items()))
    for n, (k, e) in errs.items():
        assert e < _bar(prec, k), (n, e)
    for o, r in ((o_on, r_on), (o_tg, r_tg)):
        for k in ("y", "hw", "qv", "xout", "xmid"):
            assert (o[k] is None and r[k] is None) or torch.equal(o[k], r[k]), f"mixer forward not reproducible: {k}"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_mixer_bptt_from_prefetched_forward(prec):
    """The BPTT reads the forward's stored xmid / hw / xout / qv."""
    require_gpu()
    from t2omca_amd import ops
    A, B, T = 8, 3, 2
    c = _case(A, B, T, "abs")
    shape = _gpu_shape(c["cfg"], prec)
    params = flat_from_dict(c["p_on"]).cuda()
    runs = []
    for _ in range(2):
        packs, o_on, _ = _forward(c, shape, T)
        gpack, gqv, ghid, ghw0 = ops.mixer_unroll_bwd(shape, packs[0], c["states"].cuda(), c["h_on"].cuda(), o_on,
                                                      c["gy"].cuda(), hw0=c["hw0_on"].cuda(),
                                                      ghw_ext=c["ghw"].cuda(), want_ghw0=True)
        grad = torch.zeros_like(params)
        ops.unpack_grads(shape, params, gpack, grad)
        torch.cuda.synchronize()
        runs.append(dict(grad=grad, gqv=gqv, ghid=ghid, ghw0=ghw0))
    errs = {k: normwise(runs[0][k], c["on"][k]) for k in ("grad", "gqv", "ghid", "ghw0")}
    print(f"mixer bptt A={A} B={B} T={T} {prec}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < _bar(prec, k), (k, e)
    for k in errs:
        assert torch.equal(runs[0][k], runs[1][k]), f"mixer BPTT not reproducible: {k}"
