"""GPU: TD updates 2..K against the fp64 oracle, following the learner's own trajectory.

Every other whole-update oracle test stops after one update from zero Adam moments,
where β1, β2 and the bias corrections cancel, the clip coefficient is 1, weight
decay is 0, the targets have never been swapped and every workspace buffer is fresh.
Here K = 4 updates run at (A, T) = (8, 5) and (16, 4) (the pipelined update), fp32,
each on another batch (make_batch seeds 3..6 drawn on the CPU, the masked
avail_actions of tests/test_gpu_learner_masks.py, ragged filled / terminated as
test_gpu_fullgrid._ragged draws them) of 6 -> 3 -> 6 -> 5 episodes, so
TDLearner._buf / _slab hand out prefixes of larger, dirty buffers; with
target_update_interval = 2 and episode_num = 0, 1, 2, 3 the PyMARL rule
(oracle/ref_learner.RefLearner.train) swaps the targets after the update with
episode_num = 2 and at no other.  One learner clips (grad_norm_clip = half the
oracle's gradient norm at update 0), one has weight_decay = 1e-2.  The weight-decay
learner first takes one unchecked warm-up update (seed 2, 6 episodes, episode_num 0:
no swap), so its checked Adam steps are 2..5: at step 1 from zero moments the update
is lr·g/(|g|+eps) with g = grad + weight_decay·p, where an element whose two terms
cancel to ~eps turns the fp32 rounding of that sum into ~6e-6 of p in any fp32 Adam
(tests/test_gpu_adam.py's docstring), far above the bar on p; from non-zero second
moments the step is well conditioned.

A free-running trajectory cannot be held tight against a reference one (ReLU ties,
Adam's sign sensitivity: tests/test_gpu_dp_learner.py), so every update u is checked
by itself from a snapshot of the learner's state before it:

  (i)   the oracle at the snapshot, given the snapshot's parameters and TARGET
        parameters (learner.target_params, not the packs): qtot, targets, priorities
        <= 1e-5, gradient <= 3e-5 tie-aware, with the argmax preconditions of
        test_gpu_learner_masks.py asserted.  A stale target pack after the swap, or
        stale workspace after the batch shrinks, fails here (at update 3 / 1);
  (ii)  the Adam transition: tests/gpu_util.adam_ref applied to the learner's OWN
        gradient (grad[:-1] / grad[-1]) from the snapshot's moments and step_count + 1
        against the learner's new params / exp_avg / exp_avg_sq at the bars of
        tests/test_gpu_adam.py, info["grad_norm"] <= 1e-5 relative;
  (iii) target_params bit-equal to the new params exactly when the rule fires, to the
        snapshot otherwise;
  (iv)  step_count + 1, info["mask_sum"] equal to the oracle's Σ mask exactly.

Argmax preconditions along the trajectories (share of moved argmaxes, smallest
relative top-two gap, worst over the 4 updates): (8, 5) clip 0.528 / 1.48e-04 (update
3), weight decay 0.524 / 1.01e-03; (16, 4) clip 0.485 / 2.56e-03, weight decay
0.290 (update 3) / 5.01e-04.

Measured on an MI355X (worst over the 4 updates; p as a fraction of its bar, which
the fp32 rounding of the parameters at 1 + lr, the LayerNorm gains, fills to 0.85):
                        qtot    targets prio    grad    m       v       p     grad norm
  (8, 5)  clip          5.8e-7  5.9e-7  3.2e-7  3.5e-7  2.1e-7  4.4e-7  0.86  1.4e-7
  (8, 5)  weight decay  3.5e-7  7.9e-7  5.2e-7  4.8e-7  3.3e-7  2.5e-7  0.85  2.6e-7
  (16, 4) clip          5.8e-7  5.3e-7  3.2e-7  3.4e-7  4.4e-7  4.5e-7  0.85  2.5e-7
  (16, 4) weight decay  3.9e-7  4.2e-7  3.2e-7  1.4e-6  4.5e-7  1.4e-7  0.85  1.2e-7
The clipping learner's gradient norms: 6683, 19148, 13859 (clip 3341) and 2125 (below
it) at 8 AGVs; the weight-decay learner clips at 10 in every update.
"""
import pytest
import torch

from tests.gpu_util import adam_errors, adam_ref, oracle_td_tie_aware, require_gpu, split_flat
from tests.test_gpu_fullgrid import _ragged
from tests.test_gpu_generic import _cfg_of
from tests.test_gpu_learner_masks import Snapshot, check_update, make_learner, masked_batch, to_cuda, update

pytestmark = pytest.mark.gpu

SIZES = (6, 3, 6, 5)
SEEDS = (3, 4, 5, 6)
INTERVAL = 2


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)


def _swap_rule(episodes, interval):
    """Which updates swap the targets, by RefLearner.train's rule (PyMARL's)."""
    last, fires = 0, []
    for ep in episodes:
        fire = (ep - last) / interval >= 1.0
        if fire:
            last = ep
        fires.append(fire)
    return fires


def _batches(A, T):
    out = []
    for B, seed in zip(SIZES, SEEDS):
        cpu, w = masked_batch(A, B, T, seed)
        out.append((_ragged(cpu, seed + 200), w))
    return out


def split_flat_of(pa, pm):
    """The flat fp32 parameter vector of fp64 dicts (agent then mixer)."""
    return torch.cat([v.reshape(-1) for v in list(pa.values()) + list(pm.values())]).float()


def _mask_sum(cpu):
    """The oracle's Σ mask (ref_learner.td_forward)."""
    term = cpu["terminated"][:, :-1, 0].double()
    mask = cpu["filled"][:, :-1, 0].double()
    mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
    return float(mask.sum())


@pytest.mark.parametrize("variant", ["clip", "weight_decay"])
@pytest.mark.parametrize("A,T,piped", [(8, 5, False), (16, 4, True)])
def test_updates_follow_oracle_and_adam(A, T, piped, variant):
    require_gpu()
    cfg = _cfg_of(A)
    batches = _batches(A, T)
    kw = dict(target_update_interval=INTERVAL)
    if variant == "clip":
        # half the oracle's gradient norm at update 0, so the clip engages there
        _, pa, pm = make_learner(cfg, model_seed=0)
        ref_g = oracle_td_tie_aware(pa, pm, cfg, batches[0][0], batches[0][1])[2]
        kw["grad_norm_clip"] = 0.5 * float(ref_g.norm())
    else:
        kw["weight_decay"] = 1e-2
    learner, pa, pm = make_learner(cfg, model_seed=0, **kw)
    first_step = 1
    if variant == "weight_decay":  # (module docstring: no checked step from zero moments)
        cpu, w = masked_batch(A, max(SIZES), T, 2)
        update(learner, to_cuda(_ragged(cpu, 202)), w.cuda(), episode_num=0)
        assert learner.step_count == 1 and torch.equal(learner.target_params, split_flat_of(pa, pm).cuda())
        first_step = 2
    fires = _swap_rule(range(len(SIZES)), INTERVAL)
    assert fires == [False, False, True, False]
    clipped, worst = 0, dict(qtot=0.0, targets=0.0, prio=0.0, grad=0.0, m=0.0, v=0.0, p=0.0, norm=0.0)
    for u, (cpu, w) in enumerate(batches):
        assert bool(learner._pipelined(cpu["obs"].shape[0])) == piped
        snap = Snapshot(learner)
        out, info = update(learner, to_cuda(cpu), w.cuda(), episode_num=u)
        # (i) the oracle at the snapshot, targets from learner.target_params
        pa_s, pm_s = split_flat(snap.params, pa, pm)
        pa_t, pm_t = split_flat(snap.targets, pa, pm)
        errs, _, _ = check_update(f"A={A} {variant} update {u}", learner, pa_s, pm_s, cfg, cpu, w, out,
                                  pa_tgt=pa_t, pm_tgt=pm_t, blocks=False)  # (flat only: the ragged batches'
        # fitness for a per-block comparison is not established; the first update's shapes have it in
        # test_gpu_learner_masks.py)
        # (ii) the Adam transition on the learner's own gradient
        graw = out[0]
        ref = adam_ref(snap.params, graw[:-1], snap.m, snap.v, snap.step + 1, lr=learner.lr, betas=learner.betas,
                       eps=learner.eps, weight_decay=learner.wd, max_norm=learner.clip, grad_div=float(graw[-1]))
        em, ev, ep, bar_p = adam_errors(learner.params, learner.exp_avg, learner.exp_avg_sq, ref, snap.params)
        gn = float(info["grad_norm"])
        en = abs(gn - ref[3]) / ref[3]
        clipped += gn > learner.clip
        print(f"  Adam step {snap.step + 1}: m {em:.2e} v {ev:.2e} p {ep:.2e} (bar {bar_p:.2e}) "
              f"grad norm {gn:.4f} (clip {learner.clip:.4f}) err {en:.2e}; swap {fires[u]}")
        assert em <= 1e-6 and ev <= 1e-6, (u, em, ev)
        assert ep <= bar_p, (u, ep, bar_p)
        assert en <= 1e-5, (u, en)
        # (iii) the target swap, on the PyMARL rule
        if fires[u]:
            assert torch.equal(learner.target_params, learner.params), u
            assert not torch.equal(learner.target_params, snap.targets)
        else:
            assert torch.equal(learner.target_params, snap.targets), u
        # (iv)
        assert learner.step_count == snap.step + 1 == u + first_step
        assert float(info["mask_sum"]) == _mask_sum(cpu) == float(graw[-1])
        for k, e in dict(errs, m=em, v=ev, p=ep / bar_p, norm=en).items():
            worst[k] = max(worst[k], e)
    print(f"A={A} {variant}: worst over the updates", {k: f"{v:.2e}" for k, v in worst.items()})
    if variant == "clip":
        assert clipped >= 1
