"""GPU: the agent unroll at the shapes where fetching weight fragments one product
ahead of their MFMA (wfrag_load, csrc/t2o_common.hpp) can go wrong, against the
CPU oracle (oracle/ref_model) and against a second run of itself.

The forward of the bf16 8-entity instances carries the head fragments of the next
product across products, blocks and the step boundary (the last product of step t
fetches the first of step t + 1, and the fetch after the last step reads the same
LDS image).  So the cases are: T = 1 and T = 2 (no boundary / one boundary, and
the resident-workgroup LOOP instance, which a range of <= 4 steps selects), T = 5
(the long-unroll instance the TD update runs), row counts that are no multiple of
the 16-row tile (A=8 B=3, A=3 B=6), more than one workgroup (A=8 B=9: five tiles),
an exact (8, 3) and a runtime-entity (5) instance, fp32 and bf16, and the BPTT on
both kernels (pipelined, T2O_AGENT_BWD=single), whose recompute is the same block.

Tolerances (normwise max|Δ| / max|ref|) are those of tests/test_gpu_agent.py and
tests/test_gpu_bf16.py: fp32 1e-5, bf16 2e-2 for Q / h and 6e-2 for the flat
gradient.  Every case runs twice and the two runs must agree bit for bit.

The bf16 BPTT cases take inputs on which the bar is meaningful (SEEDS below): with
the first inputs tried, (8, 3, 1) gave 8.76e-2 on both BPTT kernels, on the parent
commit as well, where the fp64 oracle with bf16 operands is itself 8.79e-2 off."""
import dataclasses
import functools

import pytest
import torch

from oracle import ref_model
from tests.gpu_util import flat_from_dict, normwise, require_gpu
from tests.test_gpu_agent import TOL_F32, _shape
from tests.test_gpu_bf16 import TOL_G, TOL_Q

pytestmark = pytest.mark.gpu

SHAPES = [(8, 3, 1), (8, 3, 2), (8, 3, 5), (8, 9, 5), (3, 6, 1), (3, 6, 2), (3, 6, 5), (5, 7, 2), (5, 7, 5)]
BWD_SHAPES = [(8, 3, 1), (8, 3, 2), (8, 9, 5), (3, 6, 2), (5, 7, 2), (5, 7, 5)]


def _cfg(A):
    return dict(n_agents=A, n_entities=A, obs_entity_feats=9, emb=32, heads=3, depth=2, ff_hidden_mult=4,
                n_actions=5)


# Input seed per shape (default 0).  The bf16 flat-gradient bar can tell a kernel
# error from rounding only where an exact computation with bf16 matmul operands
# sits clearly below it.  With few records (A·B·T = 24 at (8, 3, 1)) one FFN
# pre-activation that bf16 rounding moves across 0 changes a whole record's
# gradient: with seed 0 the fp64 oracle with bf16 operands (tests/grad_blocks.py
# Bf16Operands, CPU only) is itself 8.79e-2 off at (8, 3, 1), in
# tblocks.1.ff.0.weight, and the kernels give 8.76e-2 — before and after the
# fragment prefetch, on both BPTT kernels.  Such an input is unfit for the bar, not
# a kernel failure (the same stance as grad_blocks.assert_fit), so each BPTT shape
# takes the first seed whose emulation error is below half the bar, found on the
# CPU with the oracle alone, and the test asserts that condition on its input.
SEEDS = {(8, 3, 1): 3, (8, 3, 2): 2, (3, 6, 2): 7, (5, 7, 2): 1, (5, 7, 5): 2}


@functools.lru_cache(maxsize=None)
def _fit_for_bf16_bar(A, B, T):
    eg, e0 = _emulated_bf16_errors(_case(A, B, T))
    return eg < TOL_G / 2 and e0 < TOL_G / 2, (eg, e0)


def _emulated_bf16_errors(c):
    """Flat normwise errors (grad, gh0) of the fp64 oracle with bf16 matmul operands
    in the kernels' folded association, against the plain fp64 oracle."""
    from tests.grad_blocks import Bf16Operands
    pd = {k: v.double().requires_grad_(True) for k, v in c["p"].items()}
    h0d = c["h0"].double().requires_grad_(True)
    with Bf16Operands(fold=True):
        q, h = ref_model.agent_unroll(pd, c["obs"].double(), h0d, cfg=c["cfg"])
        gs = torch.autograd.grad((q * c["gq"].double()).sum() + (h * c["gh"].double()).sum(),
                                 list(pd.values()) + [h0d])
    return normwise(torch.cat([x.reshape(-1) for x in gs[:-1]]), c["grad"]), normwise(gs[-1], c["gh0"])


@functools.lru_cache(maxsize=None)
def _case(A, B, T):
    """Inputs and the fp64 oracle's outputs and gradients, computed once per shape."""
    cfg = _cfg(A)
    g = torch.Generator().manual_seed(100 * A + 10 * B + T + 1000 * SEEDS.get((A, B, T), 0))
    p = ref_model.init_params("agent", cfg, 7 + A)
    obs = torch.randn(B, T, A, A * 9, generator=g)
    h0 = torch.randn(B, A, 32, generator=g)
    gq = torch.randn(B, T, A, 5, generator=g)
    gh = torch.randn(B, T, A, 32, generator=g)
    pd = {k: v.double().requires_grad_(True) for k, v in p.items()}
    h0d = h0.double().requires_grad_(True)
    q, h = ref_model.agent_unroll(pd, obs.double(), h0d, cfg=cfg)
    ((q * gq.double()).sum() + (h * gh.double()).sum()).backward()
    grad = torch.cat([v.grad.reshape(-1) for v in pd.values()])
    return dict(cfg=cfg, p=p, obs=obs, h0=h0, gq=gq, gh=gh, q=q.detach(), h=h.detach(), grad=grad,
                gh0=h0d.grad.clone())


def _gpu_shape(cfg, prec):
    return dataclasses.replace(_shape(cfg), prec=1 if prec == "bf16" else 0)


def _forward(c, shape, hmid=False):
    from t2omca_amd import ops
    A, (B, T) = c["cfg"]["n_agents"], c["obs"].shape[:2]
    pack = ops.pack_params(shape, flat_from_dict(c["p"]).cuda())
    hm = torch.zeros(B, T, shape.D - 1, A, shape.E, device="cuda") if hmid else None
    q, h = ops.agent_unroll_fwd(shape, pack, c["obs"].cuda(), h0_on=c["h0"].cuda().contiguous(), hmid_on=hm)
    torch.cuda.synchronize()
    return pack, q, h, hm


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("A,B,T", SHAPES)
def test_agent_fwd_prefetch_vs_oracle(A, B, T, prec):
    require_gpu()
    c = _case(A, B, T)
    shape = _gpu_shape(c["cfg"], prec)
    _, q, h, _ = _forward(c, shape)
    _, q2, h2, _ = _forward(c, shape)
    eq, eh = normwise(q, c["q"]), normwise(h, c["h"])
    print(f"agent fwd A={A} B={B} T={T} {prec}: q {eq:.2e} h {eh:.2e}")
    tol = TOL_F32 if prec == "fp32" else TOL_Q
    assert eq < tol and eh < tol, (eq, eh)
    assert torch.equal(q, q2) and torch.equal(h, h2), "agent forward not reproducible"


@pytest.mark.parametrize("mode", ["pipe", "single"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("A,B,T", BWD_SHAPES)
def test_agent_bptt_prefetch_vs_oracle(A, B, T, prec, mode, monkeypatch):
    """BPTT from the forward's h / hmid.  pipe: the two-wave pipelined kernel (the
    forward stored hmid); single: the one-wave kernel (T2O_AGENT_BWD=single)."""
    require_gpu()
    from t2omca_amd import ops
    c = _case(A, B, T)
    if prec == "bf16":
        fit, emu = _fit_for_bf16_bar(A, B, T)
        assert fit, f"unfit input: the oracle with bf16 operands is itself {emu} off (SEEDS)"
    shape = _gpu_shape(c["cfg"], prec)
    if mode == "single":
        monkeypatch.setenv("T2O_AGENT_BWD", "single")
    else:
        monkeypatch.delenv("T2O_AGENT_BWD", raising=False)
    assert int(ops.lib().t2o_agent_bwd_ranges(ops.ctypes.byref(shape.layout()), 1)) == (1 if mode == "pipe" else 0)
    params = flat_from_dict(c["p"]).cuda()
    runs = []
    for _ in range(2):
        pack, q, h, hm = _forward(c, shape, hmid=True)
        gpack, gh0 = ops.agent_unroll_bwd(shape, pack, c["obs"].cuda(), h, h0=c["h0"].cuda().contiguous(),
                                          gq=c["gq"].cuda(), gh=c["gh"].cuda(), want_gh0=True, hmid=hm)
        grad = torch.zeros_like(params)
        ops.unpack_grads(shape, params, gpack, grad)
        torch.cuda.synchronize()
        runs.append((grad, gh0))
    (grad, gh0), (grad2, gh02) = runs
    eg, e0 = normwise(grad, c["grad"]), normwise(gh0, c["gh0"])
    print(f"agent bptt A={A} B={B} T={T} {prec} {mode}: grad {eg:.2e} gh0 {e0:.2e}")
    tol = TOL_F32 if prec == "fp32" else TOL_G
    assert eg < tol and e0 < tol, (eg, e0)
    assert torch.equal(grad, grad2) and torch.equal(gh0, gh02), "agent BPTT not reproducible"
