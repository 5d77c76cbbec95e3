"""GPU: the agent kernels (t2o_agent_unroll_fwd / _bwd, tuned and runtime-shaped) at action
counts other than five.

The Q head is one 16-column MFMA tile: lane group g holds columns 4g .. 4g + 3, guarded by
4g + r < NA in the forward, the BPTT and the range BPTT (t2o_agent.hip).  Five actions
cross the first group boundary by one column and nothing else; here the last group is
exactly full (4, 8, 16), one column wide (1, 9, 13), or the head ends inside the first
group (2, 3).  The runtime-shaped kernels (t2o_generic.hip) have their own GMAXNA = 16 loops.

Reference cases: the reference TransformerAgent's own outputs and autograd at (5 AGVs, 3
actions) and (8 AGVs, 8 actions) — tests/golden/agent_a5_na3.npz, agent_a8_na8.npz — through
the drop-in module (test_gpu_generic.agent_module_check) and through tests/test_gpu_agent.py's
forward and backward golden tests.

fp64 model cases: oracle/ref_model at random inputs, in tests/test_gpu_agent.py's form: two
networks' Q and h; the gradient of L = sum(gchosen * Q[actions]) + sum(gh * h) with respect
to every parameter tensor and h0 (the chosen-action gradient is scattered into the head's
columns at the recorded actions, among which 0 and NA - 1 both occur in every case).  The
BPTT runs from the forward's hmid: the two-wave pipelined kernel where the layout has one
(t2o_agent_bwd_ranges), and once the one-wave kernel (T2O_AGENT_BWD=single; the switch is
read at every call — t2o_agent.hip agent_bwd_single_wave — and t2o_agent_bwd_ranges == 0
is asserted to show that it took).

Bars (tests/test_gpu_runtime_shapes.py's): fp32 forward 1e-5, every parameter tensor's
gradient and dL/dh0 3e-5 normwise; bf16 forward 2e-2, the flat gradient and dL/dh0 6e-2,
on inputs for which the fp64 oracle with bf16 matmul operands (grad_blocks.Bf16Operands,
folded) is itself within half that bar (asserted; computed without a device).

MEASURED on an MI355X (every test prints its own figures; none of the reference cases and
none of these needed a second look):
  fp32 forward (q, h of either network)  <= 5.0e-7  (h at (5, 4, 5, 2))
  fp32 gradient per tensor               <= 6.2e-7 on the MFMA instances (the embedding weight at
                                         (8, 4, 5, 4)), 7.4e-7 on the runtime-shaped kernels (13 actions);
                                         the head's weight / bias <= 2.9e-7 / 1.8e-7 everywhere
  fp32 dL/dh0                            <= 3.1e-7, generic 8.9e-7
  one-wave BPTT at nine actions          per tensor 5.0e-7, dL/dh0 3.0e-7
  bf16 (8, 4, 5, 8) / (16, 3, 4, 3)      forward 4.1e-3 / 4.3e-3, flat gradient 2.0e-2 / 1.9e-2,
                                         dL/dh0 1.8e-2 / 2.3e-2 (the emulation's own: 1.4e-2 / 1.4e-2
                                         and 1.8e-2 / 2.1e-2)
"""
import ctypes
import dataclasses
import functools
import os

import pytest
import torch

from oracle import ref_model
from tests import test_gpu_agent as golden_tests
from tests.gpu_util import GOLD, flat_from_dict, normwise, require_gpu
from tests.test_gpu_agent import _shape
from tests.test_gpu_generic import agent_module_check

pytestmark = pytest.mark.gpu

TOL = {"fp32": (1e-5, 3e-5), "bf16": (2e-2, 6e-2)}
E = 32
# input draws other than the first, where the first is unfit for the bf16 bar (run_case): at
# (8, 4, 5, 8) the fp64 model with bf16 operands is itself 3.3e-2 off on dL/dh0 with draw 0
DRAWS = {(8, 4, 5, 8): 1}


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_AGENT_BWD", raising=False)


@pytest.mark.parametrize("name,instance", [("agent_a5_na3", "runtime"), ("agent_a8_na8", "exact")])
def test_reference_fixtures(name, instance):
    """Three actions on the padded runtime instance, eight (two full column groups) on the
    exact one, against the reference module's own outputs and autograd."""
    require_gpu()
    path = os.path.join(GOLD, name + ".npz")
    assert agent_module_check(path) == instance
    golden_tests.test_agent_fwd_matches_reference_golden(path)
    golden_tests.test_agent_bwd_matches_reference_autograd(path)


def _cfg(A, NA):
    return dict(n_agents=A, n_entities=A, obs_entity_feats=9, emb=E, heads=3, depth=2, ff_hidden_mult=4, n_actions=NA)


@functools.lru_cache(maxsize=None)
def case(A, B, T, NA):
    """Two networks, inputs and the fp64 model's outputs and gradients, computed once."""
    cfg = _cfg(A, NA)
    p_on = ref_model.init_params("agent", cfg, 40 + NA)
    p_tg = ref_model.init_params("agent", cfg, 60 + NA)
    g = torch.Generator().manual_seed(1000 * A + 100 * B + 10 * T + NA + 100000 * DRAWS.get((A, B, T, NA), 0))
    obs = torch.randn(B, T + 1, A, A * 9, generator=g)
    actions = torch.randint(0, NA, (B, T + 1, A, 1), generator=g)
    actions[0, 0, 0, 0], actions[B - 1, T - 1, A - 1, 0] = NA - 1, 0
    assert int(actions[:, :T].min()) == 0 and int(actions[:, :T].max()) == NA - 1
    h0 = 0.5 * torch.randn(B, A, E, generator=g)
    gch = torch.randn(B, T, A, generator=g)
    gh = torch.randn(B, T, A, E, generator=g)
    c = dict(cfg=cfg, p_on=p_on, p_tg=p_tg, obs=obs, actions=actions, h0=h0, gch=gch, gh=gh)
    c["q_tg"], c["h_tg"] = ref_model.agent_unroll({k: v.double() for k, v in p_tg.items()}, obs.double(),
                                                  h0.double(), cfg=cfg)
    c["q_on"], c["h_on"], c["gp"], c["gh0"] = _model_grads(c)
    return c


def _model_grads(c):
    T = c["gch"].shape[1]
    pd = {k: v.double().requires_grad_(True) for k, v in c["p_on"].items()}
    h0d = c["h0"].double().requires_grad_(True)
    q, h = ref_model.agent_unroll(pd, c["obs"].double(), h0d, cfg=c["cfg"])
    chosen = torch.gather(q[:, :T], 3, c["actions"][:, :T]).squeeze(3)
    loss = (chosen * c["gch"].double()).sum() + (h[:, :T] * c["gh"].double()).sum()
    gs = torch.autograd.grad(loss, list(pd.values()) + [h0d])
    return q.detach(), h.detach(), dict(zip(pd, gs[:-1])), gs[-1]


def emulated_bf16_errors(c):
    """(flat gradient, dL/dh0) normwise errors of the fp64 model with bf16 matmul operands in
    the kernels' folded association, against the plain fp64 model."""
    from tests.grad_blocks import Bf16Operands
    with Bf16Operands(fold=True):
        _, _, gp, gh0 = _model_grads(c)
    flat = lambda d: torch.cat([d[k].reshape(-1) for k in c["gp"]])  # noqa: E731
    return normwise(flat(gp), flat(c["gp"])), normwise(gh0, c["gh0"])


def run_case(A, B, T, NA, prec="fp32", instance=None, single=False):
    require_gpu()
    from t2omca_amd import ops
    c = case(A, B, T, NA)
    shape = dataclasses.replace(_shape(c["cfg"]), prec=1 if prec == "bf16" else 0)
    assert shape.NA == NA and (instance is None or shape.instance == instance)
    tf, tg = TOL[prec]
    if prec == "bf16":
        emu = emulated_bf16_errors(c)
        assert max(emu) < tg / 2, f"unfit input: the model with bf16 operands is itself {emu} off"
    ranges = int(ops.lib().t2o_agent_bwd_ranges(ctypes.byref(shape.layout()), 1))
    assert not single or ranges == 0
    dev = {k: c[k].cuda() for k in ("obs", "h0", "gch", "gh")}
    act = c["actions"].cuda()[..., 0]
    params = flat_from_dict(c["p_on"]).cuda()
    packs = [ops.pack_params(shape, flat_from_dict(p).cuda()) for p in (c["p_on"], c["p_tg"])]
    hm = torch.zeros(B, T + 1, shape.D - 1, A, E, device="cuda")
    q_on, h_on, q_tg, h_tg = ops.agent_unroll_fwd(shape, packs[0], dev["obs"], h0_on=dev["h0"], pack_tg=packs[1],
                                                  h0_tg=dev["h0"], hmid_on=hm)
    torch.cuda.synchronize()
    assert q_on.shape == (B, T + 1, A, NA)
    fwd = {k: normwise(v, c[k]) for k, v in (("q_on", q_on), ("h_on", h_on), ("q_tg", q_tg), ("h_tg", h_tg))}
    gpack, gh0 = ops.agent_unroll_bwd(shape, packs[0], dev["obs"], h_on, h0=dev["h0"], gchosen=dev["gch"], actions=act,
                                      gh=dev["gh"], want_gh0=True, hmid=hm)
    grad = torch.zeros_like(params)
    ops.unpack_grads(shape, params, gpack, grad)
    torch.cuda.synchronize()
    grad = grad.cpu()
    assert bool(torch.isfinite(grad).all())
    gerr, off = {}, 0
    for k, ref in c["gp"].items():
        gerr[k] = normwise(grad[off:off + ref.numel()].view_as(ref), ref)
        off += ref.numel()
    assert off == grad.numel()
    flat = normwise(grad, torch.cat([v.reshape(-1) for v in c["gp"].values()]))
    e0 = normwise(gh0, c["gh0"])
    worst = max(gerr.items(), key=lambda kv: kv[1])
    print(f"agent {(A, B, T, NA)} {prec} {shape.instance} bptt ranges {ranges}{' single' if single else ''}: fwd "
          f"{ {k: f'{v:.1e}' for k, v in fwd.items()} } grad flat {flat:.2e} worst tensor {worst[0]} {worst[1]:.2e} "
          f"head {gerr['q_basic.weight']:.2e} / {gerr['q_basic.bias']:.2e} gh0 {e0:.2e}")
    assert max(fwd.values()) < tf, fwd
    if prec == "fp32":
        assert max(gerr.values()) < tg, gerr
    assert flat < tg and e0 < tg, (flat, e0)
    return ranges


@pytest.mark.parametrize("A,B,T,NA,instance", [(8, 4, 5, 1, "exact"), (8, 4, 5, 4, "exact"), (8, 4, 5, 8, "exact"),
                                               (8, 3, 4, 16, "exact"), (5, 4, 5, 2, "runtime"),
                                               (12, 3, 4, 9, "runtime"), (20, 2, 4, 16, "runtime")])
def test_agent_action_counts_fp32(A, B, T, NA, instance):
    """8 AGVs: the exact instance at 1 (one column), 4 and 8 (a last group exactly full) and 16
    (the whole tile); 5 and 12: the runtime-entity instances of capacity 8 and 16; 20: the
    agent that streams its entities in 8-entity chunks, at 16 actions."""
    ranges = run_case(A, B, T, NA, instance=instance)
    if A == 8:
        assert ranges == 1  # the two-wave pipelined BPTT ran


def test_agent_action_counts_generic(monkeypatch):
    """T2O_GENERIC=1 at 13 actions: the runtime-shaped kernels' GMAXNA loops."""
    monkeypatch.setenv("T2O_GENERIC", "1")
    run_case(5, 4, 5, 13, instance="generic")


@pytest.mark.parametrize("A,B,T,NA", [(8, 4, 5, 8), (16, 3, 4, 3)])
def test_agent_action_counts_bf16(A, B, T, NA):
    run_case(A, B, T, NA, prec="bf16", instance="exact")


def test_agent_one_wave_bptt_nine_actions(monkeypatch):
    """T2O_AGENT_BWD=single: the one-wave BPTT's own head backward, at nine actions (the
    third column group one column wide)."""
    monkeypatch.setenv("T2O_AGENT_BWD", "single")
    run_case(8, 4, 5, 9, instance="exact", single=True)
