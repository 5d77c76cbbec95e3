"""GPU: the whole TD update (both agents, both mixers, double-Q, TD(λ), BPTT of both,
gradient) with SHARP attention: every tokeys / toqueries weight of the agent and the
mixer multiplied by 4 (tests/sharp.py: scores x 16), through tests/test_gpu_generic._td
with its own assertions — qtot / targets / priorities at 1e-5, the gradient at 3e-5 flat
and per parameter block against the tie-aware fp64 oracle; bf16 at (2e-2, 6e-2) and per
block through grad_blocks.assert_blocks_bf16, whose bar is calibrated by the bf16-operand
emulation of the same case.

Cases (A, B, T): (8, 4, 6) fp32 and bf16 (exact), (13, 3, 5) fp32 (runtime), (16, 3, 4)
fp32 and bf16 (multi-tile mixer, decoupled and pipelined by default), (64, 2, 3) fp32
(chunked agent, five-tile mixer), (5, 4, 6) under T2O_GENERIC=1, and pipeline=True / False
at (16, 3, 4).  The learner refuses pipeline=True wherever the mixer does not run
decoupled (one query tile: 8 AGVs; tests/test_gpu_mixer_split.py), so the forced
pipelined / sequential pair sits at the smallest shape that pipelines.

Asserted without a device (tests/test_sharp_inputs.py), from the oracle alone, for every
case: score spread >= 20 and mean max-probability >= 0.3 in both networks; at 64 the
agent's argmax falls on the hidden token and in the first and the last chunk, at 16 / 64
the mixer's in the first and the last key tile; float32 in the kernels' folded association
is within 1/3 of every fp32 bar (flat and per block), the bf16-operand emulation within
1/2 of the flat bf16 bars; the double-Q argmax's smallest top-two gap is >= 1e-4 max|Q|
(tests/gpu_util.argmax_preconditions, as tests/test_gpu_learner_masks.py asserts it).
For bf16 also: a second bf16 emulation (module-level association) stays within half of
every block's bar, so that the bar does not rest on a lucky emulation (SEEDS below).
Here the GPU case is tied to that CPU case: the modules' parameters must equal it bit
for bit.

MEASURED on an MI355X (in brackets: CPU float32 in the kernels' association / the bf16 emulation):

  case (A,B,T)        spread agent / mixer  max-prob      qtot             flat gradient     worst block
  A8 (8,4,6)          23 / 30               0.64 / 0.51   4.9e-7 (8.7e-7)  2.6e-7 (2.9e-7)   2.8e-6 (2.2e-6)
  A13 (13,3,5)        26 / 34               0.59 / 0.51   5.1e-7 (4.6e-7)  2.7e-7 (3.9e-7)   1.6e-6 (1.4e-6)
  A16 (16,3,4)        25 / 33               0.55 / 0.49   6.3e-7 (9.6e-7)  5.5e-7 (5.4e-7)   5.6e-6 (2.3e-6)
  A16 pipelined / sequential: the same figures to every digit printed
  A64 (64,2,3)        27 / 31               0.43 / 0.34   1.2e-7 (1.2e-7)  5.2e-7 (7.1e-7)   1.5e-6 (1.6e-6)
  A5 generic (5,4,6)  24 / 27               0.69 / 0.56   2.8e-7 (2.6e-7)  4.3e-7 (5.0e-7)   1.4e-6 (3.6e-6)
  A8 bf16, seed 1                                         9.6e-3 (4.7e-3)  1.3e-2 (1.5e-2)   GPU / emulation <= 1.06
  A16 bf16, seed 2                                        8.3e-3 (8.8e-3)  2.0e-2 (1.2e-2)   GPU / emul. <= 3.43 of 4
"""
import functools

import pytest
import torch

from tests.gpu_util import argmax_preconditions, require_gpu
from tests.grad_blocks import module_seed, oracle_grad
from tests.sharp import sharpen_
from tests.test_gpu_bf16 import TOL_G, TOL_Q
from tests.test_gpu_generic import _args, _cfg_of, _td

pytestmark = pytest.mark.gpu

S_UPDATE = 4
BATCH_SEED = 3
GAP = 1e-4
# (tag, A, B, T, precision, forced generic, pipeline, agent / mixer instance)
CASES = [("A8", 8, 4, 6, "fp32", False, None, "exact"), ("A8-bf16", 8, 4, 6, "bf16", False, None, "exact"),
         ("A13", 13, 3, 5, "fp32", False, None, "runtime"), ("A16", 16, 3, 4, "fp32", False, None, "exact"),
         ("A16-bf16", 16, 3, 4, "bf16", False, None, "exact"), ("A64", 64, 2, 3, "fp32", False, None, "exact"),
         ("A5-generic", 5, 4, 6, "fp32", True, None, "generic"),
         ("A16-pipelined", 16, 3, 4, "fp32", False, True, "exact"),
         ("A16-sequential", 16, 3, 4, "fp32", False, False, "exact")]
TOL = {"fp32": (1e-5, 3e-5), "bf16": (TOL_Q, TOL_G)}
# Batch seed per (A, B, T, precision) where _td's default 3 is unfit: the first seed from
# 0 upward that meets every condition of tests/test_sharp_inputs.py, found on the CPU from
# the oracle alone.  With seed 3 the bf16-operand emulation is itself 1.94e-2 off in qtot
# at (8, 4, 6) and 1.63e-2 at (16, 3, 4), against the 2e-2 bar (it must stay below half);
# seed 0 gives 2.50e-2 at (8, 4, 6) and an argmax gap of 6.0e-5 at (16, 3, 4).  At (16, 3, 4)
# seed 1 the per-block bar (4 x the folded emulation) is unfit: the folded emulation lands
# low in the mixer's blocks, where the module-level emulation, equally legitimate, is
# 4.1 - 4.3 x it (1.08 of the bar in mixer tblocks.1.norm2.weight) — and so were the
# kernels, MEASURED on an MI355X: 3 of 60 blocks at 4.06 - 4.32 x, with the same figures
# on the one-wave and on the decoupled mixer.  Seed 2 leaves the module-level emulation
# at 0.43 of the nearest bar, seed 1 at (8, 4, 6) at 0.32.
SEEDS = {(8, 4, 6, "bf16"): 1, (16, 3, 4, "bf16"): 2}


def batch_seed(A, B, T, precision):
    return SEEDS.get((A, B, T, precision), BATCH_SEED)


@functools.lru_cache(maxsize=None)
def update_case(A, B, T, seed=BATCH_SEED):
    """The modules _td draws (grad_blocks.module_seed, on the CPU) sharpened in place, the
    batch it draws, and the fp64 oracle's gradient, loss, priorities and extras."""
    from t2omca_amd.modules import TransformerAgent, TransformerMixer
    from t2omca_amd.synthetic import make_batch
    cfg = _cfg_of(A)
    state = torch.random.get_rng_state()
    try:
        torch.manual_seed(module_seed(A))
        args = _args(cfg, device="cpu")
        agent, mixer = TransformerAgent(None, args), TransformerMixer(args)
    finally:
        torch.random.set_rng_state(state)
    sharpen_(S_UPDATE)(agent, mixer)
    pa = {k: v.detach().double() for k, v in agent.state_dict().items()}
    pm = {k: v.detach().double() for k, v in mixer.state_dict().items()}
    batch, w = make_batch(B, T, A, seed=seed, obs_feats=9, state_feats=8, device="cpu")
    g, loss, prio, ex = oracle_grad(pa, pm, cfg, batch, w)
    ref = dict(grad=g, qtot=ex["qtot"], targets=ex["targets"], prio=prio)
    return dict(cfg=cfg, pa=pa, pm=pm, batch=batch, w=w, ref=ref, mac_out=ex["mac_out"])


@pytest.mark.parametrize("tag,A,B,T,precision,generic,pipeline,instance", CASES, ids=[c[0] for c in CASES])
def test_sharp_td_update_matches_oracle(tag, A, B, T, precision, generic, pipeline, instance, monkeypatch):
    require_gpu()
    monkeypatch.setenv("T2O_GENERIC", "1" if generic else "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)
    monkeypatch.delenv("T2O_AGENT_BWD", raising=False)
    seed = batch_seed(A, B, T, precision)
    c = update_case(A, B, T, seed)
    moved, gap = argmax_preconditions(c["mac_out"], c["batch"]["avail_actions"])
    print(f"{tag}: double-Q argmax top-two gap {gap:.2e} of max|Q|")
    assert gap >= GAP, gap

    def prepare(agent, mixer):
        """Sharpen in place, and tie this run to the case the CPU conditions were asserted on."""
        sharpen_(S_UPDATE)(agent, mixer)
        for mod, ref in ((agent, c["pa"]), (mixer, c["pm"])):
            sd = mod.state_dict()
            assert list(sd) == list(ref)
            assert all(torch.equal(v.detach().cpu().double(), ref[k]) for k, v in sd.items()), "not the CPU case"

    learner, errs = _td(dict(c["cfg"], tag=f"sharp-{tag}"), B, T, precision, seed=seed, tol=TOL[precision],
                        prepare=prepare, pipeline=pipeline)
    assert learner.sa.instance == instance and learner.sm.instance == instance
    if pipeline is not None:
        assert bool(learner._pipelined(B)) == pipeline
