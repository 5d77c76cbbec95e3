"""GPU: whole TD updates against the fp64 oracle at action counts other than five, and the
learner's refusal of an agent with more actions than the transformer mixer selects among.

Transformer agent + transformer mixer (test_gpu_generic._td, the bars of
tests/test_gpu_runtime_shapes.py: fp32 qtot / targets / priorities 1e-5, gradient 3e-5 flat
and per parameter block against the tie-aware oracle; bf16 2e-2 / 6e-2 and the per-block bar
against the bf16-operand emulation).  The batch is make_batch(seed 3, n_actions) drawn on the
CPU with tests/gpu_util.masked_avail(seed 103) as avail_actions; _td asserts the argmax
preconditions of tests/test_gpu_learner_masks.py on the oracle's own Q (the masked argmax
differs from the unmasked one in >= 25 % of (b, t, a); the smallest masked top-two gap is
>= 1e-4 max|Q|).  Their values at batch seed 3, computed from the oracle alone before any GPU
run.  The modules' seed is grad_blocks.module_seed(A) where that leaves every parameter block a
reference gradient to compare (grad_blocks.assert_fit); with another head width the same seed
draws another mixer, and at three shapes its hyper_b2 ReLU is off at every record (that block's
reference gradient identically zero).  There the seeds 0, 1, 2, ... were tried in order on the
CPU and the first that is fit and meets both preconditions taken (tried and rejected: (8, 4, 6, 2)
0 unfit, 1 moved 0.232, 2 unfit, 3 moved 0.009; (8, 4, 6, 8) 0 unfit; (20, 2, 5, 4) 4, 0, 1, 2
unfit, 3 moved 0.021, 5 unfit, 6 moved 0.013 and gap 6.3e-5):

  (A, B, T, NA)     seed  moved   gap        what the shape reaches
  (8, 4, 6, 2)      4     0.554   5.45e-03   head inside one column group; six padded Q slots in the mixer
  (8, 4, 6, 8)      1     0.290   1.80e-03   two full column groups; the mixer's Q row at its full width
  (5, 4, 6, 3)      0     0.586   2.65e-03   the runtime-entity instances (agent 8, mixer 8)
  (16, 4, 5, 8)     4     0.562   9.09e-04   the decoupled two-tile mixer beside the agent's step ranges (pipelined)
  (20, 2, 5, 4)     7     0.454   1.96e-03   the chunked agent, the 32-agent mixer class; one column group exactly full
  (8, 4, 6, 8) bf16 as the fp32 case, targets equal to online

Flat mixers with the transformer agent at 16 actions (the agent head's whole tile; t2o_q_select
and t2o_qplex_select at their widest row), (A, B, T) = (8, 6, 5), each through its own file's
_update (oracle, perturbed targets, bars, preconditions): qmix / vdn moved 0.545 gap 1.72e-3;
dmaq the same, share of q != m 0.917 online / 0.590 target.

The GRU agent under qmix with obs_last_action (its kernels build the one-hot, NA wide, inside
their input rows) at 2 and at 16 actions, (8, 6, 5), through tests/test_gpu_learner_rnn._update.
At 16 actions the file's module seed (1 at 8 AGVs) gives moved 0.608 gap 4.13e-4.  At two
actions seeds 0 and 1 give an agent whose Q favours action 0 almost everywhere (moved 0.003
and 0.038: under the 0.25 asked); seed 2 is the first that meets the preconditions (moved
0.517, gap 2.85e-3), chosen on the CPU from the oracle alone.

The refusal: TDLearner with a transformer mixer on MFMA kernels and a 9-action agent raises
ValueError at construction (t2o_mixer_unroll_fwd would return T2O_EUNSUPPORTED inside the
first train(), after the side stream has started); the same agent trains under qmix.

MEASURED on an MI355X (qtot / targets / priorities / flat gradient; worst block on its own maximum):
  (8, 4, 6, 2)              7.4e-7  2.1e-7  3.0e-7  8.6e-7   1.4e-6
  (8, 4, 6, 8)              4.5e-7  1.4e-7  2.1e-7  1.4e-7   1.2e-6   (one ReLU tie within the margin, not overridden)
  (5, 4, 6, 3)              6.3e-7  5.2e-7  6.2e-7  7.4e-7   1.3e-6
  (16, 4, 5, 8) pipelined   2.9e-7  1.2e-7  1.1e-7  1.8e-7   8.6e-7
  (20, 2, 5, 4)             8.8e-8  6.6e-8  5.5e-8  1.6e-7   9.9e-7
  (8, 4, 6, 8) bf16         4.8e-3  2.5e-3  2.5e-3  6.3e-3   relative L2 7.0e-2 against 3.5e-2 emulated (bar 1.4e-1)
  16 actions qmix/vdn/dmaq  2.1e-7 2.1e-7 3.3e-7 / 1.1e-7 8.7e-8 1.8e-7 / 1.9e-7 3.5e-8 1.9e-7 / 1.2e-7 7.7e-8 3.4e-7
                            (worst blocks 6.0e-7 2.7e-7 9.1e-7)
  rnn + qmix, 2 / 16        1.1e-7 / 1.8e-7   1.5e-7 / 9.5e-8   1.0e-7 / 1.7e-7   7.2e-8 / 3.0e-7   (3.0e-7 / 5.8e-7)
The only failures any of these cases showed were unfit inputs (the reference gradient of the
mixer's hyper_b2 identically zero under grad_blocks.module_seed at three shapes), before the
seeds above were chosen; no kernel missed a bar.
"""
import pytest
import torch

from tests.gpu_util import require_gpu
from tests.test_gpu_generic import _cfg_of, _td

pytestmark = pytest.mark.gpu

SEED = 3  # batch seed; the masks are drawn under SEED + 100, as tests/test_gpu_learner_masks.py's
MODEL_SEEDS = {(8, 2): 4, (8, 8): 1, (20, 4): 7}  # (A, NA): module docstring


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)


def _update(A, B, T, NA, **kw):
    cfg = dict(_cfg_of(A, n_actions=NA), tag=f"A{A}-NA{NA}")
    return _td(cfg, B, T, seed=SEED, avail_seed=SEED + 100, model_seed=MODEL_SEEDS.get((A, NA)), **kw)


@pytest.mark.parametrize("A,B,T,NA,instance", [(8, 4, 6, 2, "exact"), (8, 4, 6, 8, "exact"), (5, 4, 6, 3, "runtime"),
                                               (20, 2, 5, 4, "runtime")])
def test_td_update_action_counts_fp32(A, B, T, NA, instance):
    require_gpu()
    learner, _ = _update(A, B, T, NA)
    assert learner.sa.NA == NA and learner.sa.instance == instance and learner.sm.instance == instance


def test_td_update_eight_actions_pipelined():
    """16 AGVs at batch 4: the update runs in step ranges on two streams, the decoupled mixer's
    recurrence kernel selecting among eight actions."""
    require_gpu()
    learner, _ = _update(16, 4, 5, 8)
    assert learner._pipelined(4)


def test_td_update_eight_actions_bf16():
    require_gpu()
    learner, _ = _update(8, 4, 6, 8, precision="bf16", tol=(2e-2, 6e-2))
    assert learner.sa.NA == 8 and learner.precision == "bf16"


@pytest.mark.parametrize("kind", ["qmix", "vdn"])
def test_flat_mixer_update_sixteen_actions(monkeypatch, kind):
    require_gpu()
    from tests.test_gpu_learner_mixers import _update as flat_update
    learner = flat_update(monkeypatch, "NA16 (8,6,5)", kind, 8, 6, 5, n_actions=16)[0]
    assert learner.sa.NA == 16


def test_qplex_update_sixteen_actions(monkeypatch):
    require_gpu()
    from tests.test_gpu_learner_qplex import _update as qplex_update
    learner = qplex_update(monkeypatch, "NA16 (8,6,5)", 8, 6, 5, n_actions=16)[0]
    assert learner.sa.NA == 16


@pytest.mark.parametrize("NA,seed", [(2, 2), (16, None)])
def test_rnn_qmix_update_action_counts(monkeypatch, NA, seed):
    """(seed: the modules' torch.manual_seed where the file's own does not meet the
    preconditions — module docstring.)"""
    require_gpu()
    from tests.test_gpu_learner_rnn import _update as rnn_update
    learner = rnn_update(monkeypatch, f"NA{NA} (8,6,5)", "qmix", 8, 6, 5, n_actions=NA, seed=seed)[0]
    assert learner.sa.NA == NA and learner.sa.last_action and learner.sa.IN == 9 * 8 + NA + 8


def test_learner_refuses_nine_actions_under_the_transformer_mixer():
    """Nine actions: refused at construction under the transformer mixer, naming the count and
    the limit; the same agent trains under qmix (finite update, parameters moved)."""
    require_gpu()
    from t2omca_amd import _lib
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.modules import TransformerAgent, TransformerMixer, make_mixer
    from t2omca_amd.synthetic import make_args, make_batch
    A, B, T, NA = 8, 4, 5, 9
    limit = int(_lib.lib().t2o_mixer_max_actions())
    assert NA == limit + 1
    torch.manual_seed(0)
    args = make_args(A, n_actions=NA, mixer="qmix")
    agent = TransformerAgent(None, args).cuda()
    with pytest.raises(ValueError, match=rf"(?s)at most {limit} actions.*has {NA}.*qmix, vdn and dmaq"):
        TDLearner(agent, TransformerMixer(args).cuda())
    learner = TDLearner(agent, make_mixer(args).cuda())
    before = learner.params.clone()
    batch, w = make_batch(B, T, A, n_actions=NA, seed=SEED)
    info = learner.train(batch, 0, 0, per_weight=w)
    torch.cuda.synchronize()
    assert learner.step_count == 1 and bool(torch.isfinite(learner.grad).all())
    assert bool(torch.isfinite(info["qtot"]).all()) and not torch.equal(learner.params, before)
