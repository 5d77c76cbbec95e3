"""GPU: the flat mixers (csrc/t2o_qmix.hip, t2o_qplex.hip) and the GRU agent (t2o_rnn.hip)
on grids that fill their weight-gradient slabs, against the fp64 models of the WHOLE grid.

The earlier kernel tests stop at R = 280 rows: 18 tiles, two slabs, three trips through a
slab's tile loop.  The shapes of tests/flat_grids.py (its docstring has the slab rule and
the table) reach what those never ran: 64 slabs (the cap), 10 tiles per slab, 6 empty
slabs that must be written as zeros, a last tile of 1, 4, 8 or 12 rows, a last slab of 1
or 7 tiles, and reduce_slabs adding 4 slabs per lane over parameter totals of every
alignment.  tests/test_flat_grid_shapes.py proves on the CPU that the shapes are what this
says and that float32 alone stays under a third of every bar; the bars are the project's
(flat_grids.bars: 1e-5 normwise on every forward output, 3e-5 on dL/dq, dL/dh0, the flat
gradient and every parameter tensor on its own maximum).

  kernel level   forward of both networks and the backward at every shape, QMIX's softplus
                 head at the capped one; two runs of every backward bit-equal.
  poison         at the capped shapes the slab buffer (one slab longer than needed) and the
                 work buffer arrive filled with NaN: the 64 slabs come back finite, the 6
                 empty ones exactly zero, the extra slab still NaN, the reduced gradient
                 bit-equal to the run on fresh buffers.
  reduce_slabs   1, 15, 16, 17, 64 seeded normal slabs of n = 4096, 4100 (n % 64 = 4) and
                 30789 floats (the capped agent's parameter total, n % 4 = 1: the scalar path)
                 against the float64 sum at 1e-6 normwise; two runs bit-equal.
  learner        TDLearner with the GRU agent under qmix, vdn and qplex at (8, 165, 7)
                 through test_gpu_learner_rnn._update, unchanged: the agent's 9240 rows
                 fill 64 slabs, the mixers' 1155 rows nine slabs of nine tiles.
  reuse          one learner of each kind takes updates at B = 6, 165, 6, 40 from the same
                 state (its workspaces grow once and are then reused oversized, with the
                 larger batch's content): each update bit-equal to a fresh learner's.

MEASURED on an MI355X (normwise; each test prints its own figures; the poisoned runs are bit-equal):
  case                  forward (worst)   dL/dq    dL/dh0   flat grad  worst tensor
  qmix capped abs       1.6e-7 (y_tg)     1.8e-7            2.7e-7     5.0e-7 hyper_w1.0.bias
  qmix capped softplus  2.1e-7 (y_on)     1.8e-7            2.7e-7     7.1e-7 hyper_b1.0.bias
  qmix middle           1.9e-7 (y_tg)     1.3e-7            1.8e-7     2.6e-7 hyper_b2.2.bias
  qplex capped          2.2e-7 (y3)       1.9e-7            1.3e-7     5.9e-7 si_weight.action_extractors.1.2.bias
  qplex middle          2.6e-7 (y_tg)     1.9e-7            1.9e-7     1.9e-6 si_weight.agents_extractors.0.2.bias
  rnn capped            3.5e-7 (q_tg)              8.3e-7   2.0e-7     3.1e-7 rnn.weight_hh
  rnn middle            2.1e-7 (q_on)              4.1e-7   2.1e-7     4.2e-7 rnn.weight_hh
  reduce_slabs: exact at one slab, else 1.0e-7 - 1.7e-7.
  learner (8, 165, 7), qmix / vdn / qplex: qtot 2.1e-7 2.2e-7 2.2e-7, targets 1.4e-7 9.8e-8 1.1e-7, priorities
  1.8e-7 1.1e-7 1.2e-7, gradient 1.8e-7 1.1e-7 1.5e-7, worst block 3.9e-7 1.7e-7 7.8e-7; no ReLU tie.
  Reuse: every update of 6 -> 165 -> 6 -> 40 episodes bit-equal to a fresh learner's (the agent's slab buffer grows
  from 61 578 to 1 970 496 floats at the second update and stays).  The 32 tests take 3.7 s.

That these tests can fail (two defects planted in a scratch build, DESIGN.md section 5 "Slab grids"): with every
slab's tile loop cut at eight tiles 14 of them fail (and 24 of the 224 earlier tests of these kernels, none of
QPLEX's); with the write of an empty slab skipped 12 fail and all 224 earlier tests pass.
"""
import pytest
import torch

import tests.test_gpu_learner_rnn as lr
import tests.test_gpu_qmix as tq
import tests.test_gpu_qplex as tp
import tests.test_gpu_rnn_agent as tr
from tests import flat_grids as fg
from tests.gpu_util import normwise, require_gpu
from tests.test_gpu_learner_masks import SEED, Snapshot, masked_batch, perturb_targets, to_cuda, update

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("kernel,grid,key", fg.CASES, ids=fg.CASE_IDS)
CAPPED = pytest.mark.parametrize("kernel,grid,key", [c for c in fg.CASES if c[1] == "capped"],
                                 ids=[i for c, i in zip(fg.CASES, fg.CASE_IDS) if c[1] == "capped"])


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)


def _poison(n):
    return torch.full((n,), float("nan"), device="cuda")


def run_kernels(kernel, key, poison=False):
    """Forward of both networks and the backward of one case on the device.  Returns
    (the checked quantities by flat_grids' names, the slab buffer, nslab); poison: the
    slab buffer one slab longer than needed and the work buffer, both filled with NaN."""
    from t2omca_amd import ops
    if kernel == "qmix":
        c = fg.qmix_case(key)
        sh, T = c["shape"], key[2]
        d = {k: c[k].cuda() for k in ("flat_on", "flat_tg", "states", "q_on", "q_tg", "gy")}
        y_on, y_tg = ops.qmix_fwd(sh, d["flat_on"], d["states"], d["q_on"], params_tg=d["flat_tg"], qv_tg=d["q_tg"])
        kw = {}
        if poison:
            kw = dict(slabs=_poison((ops.qmix_slab_count(key[1], T) + 1) * sh.n_params),
                      work=_poison(ops.qmix_work_floats(sh, key[1], T)))
        gqv, slabs, nslab = ops.qmix_bwd(sh, d["flat_on"], d["states"][:, :T], d["q_on"], d["gy"], **kw)
        got = dict(y_on=y_on, y_tg=y_tg, gqv=gqv)
    elif kernel == "qplex":
        c = fg.qplex_case(key)
        sh, T = c["shape"], key[2]
        d = tp._dev(c)
        got = {f"y{parts}": ops.qplex_fwd(sh, d["flat_on"], d["states"], *d["on"], parts=parts) for parts in (1, 2)}
        got["y3"], got["y_tg"] = ops.qplex_fwd(sh, d["flat_on"], d["states"], *d["on"], params_tg=d["flat_tg"],
                                               qv_tg=d["tg"][0], qmax_tg=d["tg"][1], act_tg=d["tg"][2], parts=3)
        kw = {}
        if poison:
            kw = dict(slabs=_poison((ops.qplex_slab_count(key[1], T) + 1) * sh.n_params),
                      work=_poison(ops.qplex_work_floats(sh, key[1], T)))
        got["gqv"], slabs, nslab = ops.qplex_bwd(sh, d["flat_on"], d["states"][:, :T], *d["on"], d["gy"], parts=3, **kw)
    else:
        c = fg.rnn_case(key)
        sh = c["shape"]
        d = tr.to_dev(c)
        f = tr.forward(c, d)
        got = {k: f[k] for k in ("q_on", "h_on", "q_tg", "h_tg")}
        kw = {}
        if poison:
            kw = dict(slabs=_poison((ops.rnn_slab_count(key[1], c["T"], key[0]) + 1) * sh.n_params),
                      work=_poison(ops.rnn_work_floats(sh, key[1], c["T"])))
        slabs, nslab, got["gh0"] = ops.rnn_agent_bwd(sh, d["flat_on"], d["obs"], f, T=c["T"], actions=d["actions"],
                                                     gchosen=d["gch"], gh=d["gh"], h0=d["h0"], want_gh0=True, **kw)
    got["gflat"] = ops.reduce_slabs(slabs, nslab, torch.empty_like(d["flat_on"]))
    torch.cuda.synchronize()
    assert got["gflat"].numel() == sh.n_params
    return got, slabs, nslab


def check(tag, kernel, key, got):
    """Every quantity, and every parameter tensor of the flat gradient on its own maximum,
    against the fp64 reference of the whole grid at flat_grids.bars."""
    ref, bars = fg.reference(kernel, key), fg.bars(kernel, key)
    got = dict(got, **fg.split_blocks(got["gflat"], ref))
    assert set(got) == set(ref) == set(bars)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (tag, k)
    errs = fg.errors(got, ref)
    block = max((k for k in errs if k.startswith("block.")), key=lambda k: errs[k])
    print(f"{tag}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items() if not k.startswith("block."))
          + f" worst tensor {block[6:]} {errs[block]:.2e}")
    assert not fg.unfit_blocks(kernel, key)
    bad = {k: (e, bars[k]) for k, e in errs.items() if not e <= bars[k]}
    assert not bad, (tag, bad)
    return errs


@CASES
def test_forward_backward(kernel, grid, key):
    require_gpu()
    got, _, nslab = run_kernels(kernel, key)
    assert nslab == fg.partition(fg.rows(kernel, key))[1]
    check(f"flat grid {kernel} {grid} {key}", kernel, key, got)
    again, _, _ = run_kernels(kernel, key)
    for k, v in got.items():
        assert torch.equal(v, again[k]), f"not reproducible: {k}"


@CAPPED
def test_empty_slabs_and_poisoned_workspaces(kernel, grid, key):
    require_gpu()
    _, nslab, _, used, empty, _ = fg.partition(fg.rows(kernel, key))
    clean, _, _ = run_kernels(kernel, key)
    got, slabs, n = run_kernels(kernel, key, poison=True)
    assert n == nslab == 64 and empty >= 1
    slabs = slabs.view(nslab + 1, -1)
    assert bool(torch.isfinite(slabs[:nslab]).all()), "a slab the reduction reads was left unwritten"
    assert bool(slabs[:used].abs().amax(1).gt(0).all()), "a used slab is all zeros"
    assert not bool(slabs[used:nslab].any()), "an empty slab is not exactly zero"
    assert bool(torch.isnan(slabs[nslab]).all()), "written past the last slab"
    check(f"flat grid {kernel} {grid} {key} poisoned", kernel, key, got)
    for k, v in got.items():
        assert torch.equal(v, clean[k]), f"the workspace's content shows in {k}"


REDUCE_N = [4096, 4100, 30789]
assert REDUCE_N[0] % 64 == 0 and REDUCE_N[1] % 4 == 0 and REDUCE_N[1] % 64 and REDUCE_N[2] % 4


@pytest.mark.parametrize("n", REDUCE_N)
@pytest.mark.parametrize("nslab", [1, 15, 16, 17, 64])
def test_reduce_slabs(nslab, n):
    require_gpu()
    from t2omca_amd import ops
    if n == REDUCE_N[2]:
        assert n == fg.rnn_case(fg.RNN_CAPPED)["shape"].n_params
    g = torch.Generator().manual_seed(1000 * nslab + n)
    slabs = torch.randn(nslab + 1, n, generator=g)
    slabs[nslab] = float("nan")  # (one slab past the count: never read)
    dev = slabs.cuda()
    out = ops.reduce_slabs(dev, nslab, _poison(n))
    again = ops.reduce_slabs(dev, nslab, _poison(n))
    torch.cuda.synchronize()
    err = normwise(out, slabs[:nslab].double().sum(0))
    print(f"reduce_slabs nslab={nslab} n={n}: {err:.2e}")
    assert bool(torch.isfinite(out).all()) and err <= 1e-6, err
    assert torch.equal(out, again)


# ---- the learner ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", lr.KINDS)
def test_update_fills_the_slabs(monkeypatch, kind):
    """One whole update at (8, 165, 7) against the fp64 oracle, per block (_update's checks)."""
    require_gpu()
    A, B, T = fg.LEARNER_SHAPE
    monkeypatch.setattr(lr, "SEED", fg.LEARNER_BATCH_SEED)  # (the batch _update draws: flat_grids.LEARNER_BATCH_SEED)
    learner, *_ = lr._update(monkeypatch, f"flat grid ({A},{B},{T})", kind, A, B, T)
    from t2omca_amd import ops
    assert ops.rnn_slab_count(B, T, A) == 64 and learner._slabs["rnn"].numel() == 64 * learner.na


def _reuse_update(learner, B):
    A, _, T = fg.LEARNER_SHAPE
    cpu, w = masked_batch(A, B, T, SEED)
    return update(learner, to_cuda(cpu), w.cuda())[0]


@pytest.mark.parametrize("kind", lr.KINDS)
def test_workspace_reuse(kind):
    """B = 6, 165, 6, 40 through one learner, its state restored between the updates: each
    update's Q_tot, targets, priorities and raw gradient equal, bit for bit, those of a
    freshly constructed learner (fresh workspaces of that batch's own size) on the same batch."""
    require_gpu()
    A = fg.LEARNER_SHAPE[0]
    learner, _, _ = lr.make_learner(A, kind)
    perturb_targets(learner)
    snap = Snapshot(learner)
    sizes = []
    for B in fg.REUSE_BATCHES:
        got = _reuse_update(learner, B)
        snap.restore()
        sizes.append({k: v.numel() for k, v in learner._slabs.items()})
        fresh, _, _ = lr.make_learner(A, kind)
        perturb_targets(fresh)
        assert torch.equal(fresh.params, snap.params) and torch.equal(fresh.target_params, snap.targets)
        ref = _reuse_update(fresh, B)
        for name, a, b in zip(("grad", "qtot", "targets", "td_errors_abs"), got, ref):
            assert a.shape == b.shape and bool(torch.isfinite(a).all()), (kind, B, name)
            assert torch.equal(a, b), (f"{kind} B={B}: {name} differs from a fresh learner's in "
                                       f"{int((a != b).sum())} of {a.numel()} elements, normwise {normwise(a, b):.2e}")
    # the workspaces grew at the large batch and were kept for the smaller ones after it
    assert sizes[1] == sizes[2] == sizes[3] and all(sizes[1][k] > n for k, n in sizes[0].items() if "rnn" in k)
    print(f"reuse {kind}: workspaces {sizes[0]} -> {sizes[1]}")
