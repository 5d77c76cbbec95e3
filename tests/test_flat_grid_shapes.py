"""No device: every case of tests/test_gpu_flat_grids.py is what that file says it is.

A GPU comparison on a grid that "fills the slabs" proves something only if (a) the grid
does fill them — the slab arithmetic restated in tests/flat_grids.partition gives each
shape the partition its table claims, and the library's own host-side counts
(ops.*_slab_count, ops.*_work_floats: they need no device) agree with it — and (b) float32
arithmetic itself, summing 9 000 rows, stays clear of the bars — else a failure would say
nothing about the kernel.  Both are conditions here:

  shapes    capped: 64 slabs, tps >= 9, an empty slab, a partial last tile; middle:
            2..63 slabs, tps >= 9, a short last slab, a partial last tile.
  counts    the library's slab counts equal partition(R)[1]; the work buffers are the
            documented ones (QMIX, QPLEX: the rows padded to whole tiles times a row width
            that does not depend on the grid; the agent: R·5·H).
  fitness   no parameter tensor's reference gradient is under grad_blocks.FIT_SHARE of the
            largest; the same model in torch float32 on the CPU (one thread) stays under a
            third of every bar of flat_grids.bars against the fp64 reference.

MEASURED here (float32 on the CPU against fp64, normwise, the worst quantity of each case):
  qmix   capped abs 1.6e-6, softplus 1.6e-6, middle 4.6e-7 (hyper_b2.2.weight's gradient each time);
         forward outputs <= 1.6e-7, dL/dq <= 2.1e-7, flat gradient <= 8.8e-7
  qplex  capped 2.1e-6 (si_weight.key_extractors.2.2.weight), middle 1.3e-6
         (si_weight.agents_extractors.0.2.bias); forward <= 3.5e-7, dL/dq 2.1e-7, flat 2.9e-7
  rnn    capped 3.2e-7 (fc1.weight; q_tg 3.2e-7), middle 2.9e-7 (fc2.weight); dL/dh0 <= 1.4e-7
  learner (8, 165, 7) at batch seed 18: argmax moved 0.432, gap 1.46e-4; float32 oracle qtot <= 2.7e-7,
         targets <= 1.3e-7, priorities <= 1.7e-7, gradient <= 3.1e-7, worst block 7.7e-7 (qplex)
so every case is under a third of the project's bars (1e-5 forward, 3e-5 gradients) by a factor
of four or more, the bars stay as they are and none is replaced.
"""
import pytest

from tests import flat_grids as fg

CASES = pytest.mark.parametrize("kernel,grid,key", fg.CASES, ids=fg.CASE_IDS)


def test_partition_is_the_rule():
    """partition() on sizes worked out by hand (the issue's table and the edges of the rule)."""
    assert fg.partition(1) == (1, 1, 1, 1, 0, 1)
    assert fg.partition(16) == (1, 1, 1, 1, 0, 16)
    assert fg.partition(280) == (18, 2, 9, 2, 0, 8)          # the largest grid of the earlier kernel tests
    assert fg.partition(9233) == (578, 64, 10, 58, 6, 1)
    assert fg.partition(9240) == (578, 64, 10, 58, 6, 8)
    assert fg.partition(1300) == (82, 10, 9, 10, 0, 4) and fg.last_slab_tiles(1300) == 1
    assert fg.partition(1260) == (79, 9, 9, 9, 0, 12) and fg.last_slab_tiles(1260) == 7
    assert fg.partition(165 * 7) == (73, 9, 9, 9, 0, 3) and fg.last_slab_tiles(165 * 7) == 1
    assert fg.partition(576 * 16) == (576, 64, 9, 64, 0, 16)  # the cap with every slab used
    assert fg.partition(1024 * 60) == (3840, 64, 60, 64, 0, 16)  # the headline grid
    for R in range(1, 12000, 7):  # the slabs cover every tile once
        ntiles, nslab, tps, used, empty, last = fg.partition(R)
        assert (used - 1) * tps < ntiles <= used * tps <= nslab * tps and used + empty == nslab
        assert (ntiles - 1) * 16 + last == R and 1 <= last <= 16


@CASES
def test_shape_meets_its_conditions(kernel, grid, key):
    R = fg.rows(kernel, key)
    print(f"{kernel} {grid} {key}: R {R} partition {fg.partition(R)} last slab {fg.last_slab_tiles(R)} tiles")
    fg.assert_grid(grid, R)


def test_learner_shapes():
    A, B, T = fg.LEARNER_SHAPE
    fg.assert_grid("capped", B * T * A)  # the agent's rows
    fg.assert_grid("middle", B * T)      # the mixers'
    assert fg.REUSE_BATCHES[1] == B and max(fg.REUSE_BATCHES) == B
    # the reused workspaces shrink, stay and grow again below the largest
    assert fg.REUSE_BATCHES[0] == fg.REUSE_BATCHES[2] < fg.REUSE_BATCHES[3] < B
    slabs = [fg.partition(b * T * A)[1] for b in fg.REUSE_BATCHES]
    assert slabs == [2, 64, 2, 17], slabs


@pytest.mark.parametrize("kind", ["qmix", "vdn", "qplex"])
def test_learner_case_is_fit(kind):
    """check_update's preconditions (argmax moved >= 0.25, top-two gap >= 1e-4) and fitness at
    the batch seed flat_grids.LEARNER_BATCH_SEED, and the float32 oracle under a third of the
    whole-update bars (test_gpu_learner_masks.TOL, grad_blocks.FP32_BLOCK_BAR)."""
    from tests.grad_blocks import FP32_BLOCK_BAR
    from tests.test_gpu_learner_masks import TOL
    moved, gap, share, errs = fg.learner_case_cpu(kind)
    print(f"learner {kind} {fg.LEARNER_SHAPE} seed {fg.LEARNER_BATCH_SEED}: moved {moved:.3f} gap {gap:.2e} smallest "
          f"share {share:.1e}; cpu float32 " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert moved >= 0.25 and gap >= 1e-4, (moved, gap)
    tf, tg = TOL["fp32"]
    for k, bar in dict(qtot=tf, targets=tf, prio=tf, grad=tg, block=FP32_BLOCK_BAR).items():
        assert errs[k] <= bar / 3.0, (kind, k, errs[k], bar)


@CASES
def test_library_counts_agree(kernel, grid, key):
    from t2omca_amd import ops
    R = fg.rows(kernel, key)
    ntiles, nslab = fg.partition(R)[:2]
    if kernel == "qmix":
        c = fg.qmix_case(key)
        A, B, T, M, H = key[:5]
        assert ops.qmix_slab_count(B, T) == nslab
        work = ops.qmix_work_floats(c["shape"], B, T)
        assert work == ntiles * 16 * (ops.qmix_work_floats(c["shape"], 1, 1) // 16)
    elif kernel == "qplex":
        c = fg.qplex_case(key)
        A, B, T = key[:3]
        assert ops.qplex_slab_count(B, T) == nslab
        work = ops.qplex_work_floats(c["shape"], B, T)
        assert work == ntiles * 16 * (ops.qplex_work_floats(c["shape"], 1, 1) // 16)
    else:
        c = fg.rnn_case(key)
        A, B, T1, H = key[:4]
        assert ops.rnn_slab_count(B, c["T"], A) == nslab
        assert ops.rnn_work_floats(c["shape"], B, c["T"]) == R * 5 * H


@CASES
def test_reference_is_fit(kernel, grid, key):
    ref = fg.reference(kernel, key)
    assert not fg.unfit_blocks(kernel, key), fg.unfit_blocks(kernel, key)
    errs, bars = fg.fp32_errors(kernel, key), fg.bars(kernel, key)
    assert set(errs) == set(bars) == set(ref)
    worst = max(errs, key=lambda k: errs[k] / bars[k])
    block = max((k for k in errs if k.startswith("block.")), key=lambda k: errs[k])
    print(f"{kernel} {grid} {key} cpu float32: nearest its bar {worst} {errs[worst]:.2e} (bar {bars[worst]:g}); "
          f"worst tensor {block} {errs[block]:.2e}; "
          + " ".join(f"{k} {v:.2e}" for k, v in errs.items() if not k.startswith("block.")))
    for k, bar in bars.items():
        assert errs[k] <= bar / 3.0, (
            f"{kernel} {grid}: unfit input, float32 rounding alone gives {k} {errs[k]:.2e} (bar {bar:g})")
