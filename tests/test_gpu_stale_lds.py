"""GPU: no kernel's result depends on what LDS held before it ran.

A kernel that reads an LDS word it did not write gets whatever the previous workgroup
on that CU left there.  The oracle tests cannot see such a read: in a test process the
leftovers are small finite numbers from the same kernels, multiplied by masked zeros.
Here every LDS word of every CU is set to a chosen 32-bit word first
(ops.lds_fill, t2o_probe.hip: one 160 KB workgroup per CU), then the launch under test
runs, where the case can arrange it, on fewer workgroups than the device has CUs, so that
each is the first on its CU after the fill (the exceptions are listed below), and its
outputs must be finite and THE SAME BITS whatever the word was
(tests/lds_fill.py: 0, 0xFFFFFFFF = NaN, 0x7F7F7F7F = 3.4e38 in fp32 and both bf16
halves; the huge finite word passes through the fmaxf / ReLU that swallow a NaN).

The premise (test_fill_reaches_every_workgroup, test_census_reads_the_fill): LDS keeps
its contents from one dispatch to the next and the fill reaches every CU.  Measured on
an MI355X (256 CUs; census = ops.lds_census, one 160 KB workgroup per CU, 40 960 words
each, counting the words that differ from the word asked for):

  fill grid 1x, 2x, 4x, 8x, 16x the CU count, each of the three words, twice over:
      0 differing words in every one of 256 census workgroups, and in every one of 1024
      (a census grid of 4x).  The smallest grid already reaches every CU; ops.lds_fill
      keeps the 4x default, which costs 9 us.
  fill 0xFFFFFFFF, census asked for 0x7F7F7F7F: 40 960 of 40 960 words differ in all 256.
  fill, synchronise, one torch reduction (x.sum()), census: 128 of 256 workgroups see
      up to 513 differing words: another kernel's LDS writes do survive into the next
      dispatch, which is the hazard this module is about.

Bit equality leans on the kernels being bit-reproducible run to run (README;
tests/test_gpu_reproducibility.py pins the whole update, test_gpu_noisy_head.py the
noisy head, test_gpu_stats_kernels.py the statistics).  On the summation-order bar
instead (1e-6 normwise, tests/test_gpu_fullgrid.py GRAD_SUM_BAR; float atomics in
varying order), plus finiteness:
  * the loss scalar of t2o_td_loss / t2o_td_qlambda (out["loss"]);
  * the T2O_GENERIC=1 update's raw gradient (its post-step parameters are checked
    exactly against the Adam step of that gradient, test_whole_update_generic says why).

Where a wrapper exposes the launches of one call, each gets its own fill: the BPTTs and
their contractions, the decoupled mixer's recurrence and rows kernels (phase 1 / 2,
forward and backward), qmix_bwd's and qplex_bwd's rows and weight-gradient kernels.
Where it does not, the later kernel of the call runs straight after the earlier one and
sees the fill only on CUs, and in LDS, the earlier one left alone:
  * rnn_agent_bwd: the BPTT kernel, then the weight-gradient kernel (`red[]`);
  * tape_contract: the contraction, then t2o_reduce_slabs (which has a case of its own);
  * TDLearner.train: one fill before the whole update.
Outside "fewer workgroups than CUs": t2o_reduce_slabs runs n / 64 workgroups (about 660
for a 42k-float gradient) inside every tape_contract and in the qmix / qplex / rnn cases
— its own case runs it at n = 255·64; the optimisers' norm partials run a fixed 256
workgroups, the CU count, and their update kernels 329 at n = 84 007 without using LDS.
These are small workgroups: several share a CU on disjoint LDS, so the first generation
still starts from the fill, but workgroups past it may start from a predecessor's words.

In the sweep: agent_unroll_fwd, agent_unroll_bwd + tape_contract, mixer_unroll_fwd,
mixer_unroll_bwd + its contraction (one-wave and decoupled), TDLearner.train (sequential,
pipelined, q_lambda, noisy agent, generic), qmix / qplex fwd + bwd, the GRU agent fwd +
bwd, the noisy head fwd / bwd / wgrad, td_loss, td_qlambda, adam_step, rmsprop_step,
reduce_slabs, pack_params / unpack_grads, td_stats, episode_stats.  Their LDS
(`smem`, `sm`, `red`, `lw`, `lf`, `Ws`, `Bs`, `part`, `noisy_smem`) holds fp32 / bf16 /
fp64 values only.  The one exception read and kept: the pair-barrier counters of the
pipelined BPTT kernels (t2o_common.hpp PairBarrier, 16 ints behind the float buffers),
which every such kernel zeroes and fences with __syncthreads() before any wave polls
them; they are counters, never addresses.

Left out on purpose: kernels that keep integers used as addresses, indices or loop
bounds in LDS — env_kernel (EnvLds), obs_expand_kernel (rows[]), the replay kernels
(key[], t2o_replay.hip).  A stale word there would be used as an index, and the fills
would make a wild access certain where today it is only possible.  select_actions_kernel
uses no LDS.
"""
import functools

import pytest
import torch

from tests import flat_grids
from tests.gpu_util import require_gpu
from tests.grad_blocks import module_seed
from tests.lds_fill import HUGE, NAN, PATTERNS, refill, under_each_fill
from tests.test_gpu_generic import _cfg_of
from tests.test_gpu_learner_masks import SEED, Snapshot, make_learner, masked_batch, to_cuda, update

pytestmark = pytest.mark.gpu

LDS_WORDS = 160 * 1024 // 4
PRECISIONS = ["fp32", "bf16"]


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    """The tuned instances and the default kernel choices unless a case says otherwise."""
    monkeypatch.setenv("T2O_GENERIC", "0")
    for k in ("T2O_MIXER_SPLIT", "T2O_MIXS_REC", "T2O_AGENT_BWD"):
        monkeypatch.delenv(k, raising=False)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the premise ---------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", PATTERNS, ids=[f"{p:#010x}" for p in PATTERNS])
def test_fill_reaches_every_workgroup(pattern):
    require_gpu()
    from t2omca_amd import ops
    torch.cuda.synchronize()
    ops.lds_fill(NAN if pattern != NAN else HUGE)  # whatever was there, it is not `pattern`
    ops.lds_fill(pattern)
    census = ops.lds_census(pattern).cpu()
    assert census.numel() == _cus()
    dirty = census[census != 0]
    print(f"fill {pattern:#010x}: {dirty.numel()} of {census.numel()} workgroups see other words "
          f"(most {int(census.max())} of {LDS_WORDS})")
    assert dirty.numel() == 0, dirty.tolist()


def test_census_reads_the_fill():
    """The census after a fill of one pattern, asked for another: every word of every
    workgroup differs.  The census reads LDS, not a constant."""
    require_gpu()
    from t2omca_amd import ops
    torch.cuda.synchronize()
    ops.lds_fill(NAN)
    other = ops.lds_census(HUGE).cpu()
    same = ops.lds_census(NAN).cpu()
    assert bool((other == LDS_WORDS).all()), other.tolist()
    assert bool((same == 0).all()), same.tolist()


# ---- transformer agent and mixer -----------------------------------------------------------

AGENT_B = {3: 5, 8: 6, 5: 3, 16: 2, 40: 2, 63: 2, 64: 2}
MIXER_B = {3: 4, 5: 4, 8: 4, 13: 3, 16: 3, 40: 2, 63: 2, 64: 2}
T_BWD = 4


@functools.lru_cache(maxsize=None)
def _nets(A, precision):
    """The learner's shapes and packs at A AGVs (its own, and a perturbed target pack)."""
    from t2omca_amd import ops
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.modules import TransformerAgent, TransformerMixer
    from t2omca_amd.synthetic import make_args
    torch.manual_seed(module_seed(A))
    args = make_args(A, device="cuda")
    agent, mixer = TransformerAgent(None, args).cuda(), TransformerMixer(args).cuda()
    ln = TDLearner(agent, mixer, precision=precision, priorities_to_cpu=False)
    g = torch.Generator().manual_seed(1)
    tgt = ln.params + (0.01 * torch.randn(ln.params.numel(), generator=g)).cuda()
    packs = dict(a_on=ops.pack_params(ln.sa, ln.params[:ln.na].contiguous()),
                 m_on=ops.pack_params(ln.sm, ln.params[ln.na:].contiguous()),
                 a_tg=ops.pack_params(ln.sa, tgt[:ln.na].contiguous()),
                 m_tg=ops.pack_params(ln.sm, tgt[ln.na:].contiguous()))
    torch.cuda.synchronize()
    return ln.sa, ln.sm, packs


@functools.lru_cache(maxsize=None)
def _inputs(A, B, T):
    """masked_batch on the device (T + 1 steps) and the random cotangents of the BPTT cases."""
    cpu, _ = masked_batch(A, B, T, SEED)
    d = to_cuda(cpu)
    g = torch.Generator().manual_seed(SEED + 1)
    d["act"] = d["actions"][..., 0].contiguous()
    d["avail32"] = d["avail_actions"].int().contiguous()
    d["h0"] = (0.5 * torch.randn(B, A, 32, generator=g)).cuda()
    d["gch"] = torch.randn(B, T, A, generator=g).cuda()
    d["gh"] = torch.randn(B, T, A, 32, generator=g).cuda()
    d["gy"] = torch.randn(B, T, generator=g).cuda()
    d["qv"] = torch.randn(B, T, A, generator=g).cuda()
    return d


def _contract(dc):
    """A deferred tape contraction on the BPTT's own slabs: not widened to
    ops.CONTRACT_MIN_WG workgroups (which is the CU count), so that each of its workgroups
    is the first on its CU after the fill.  (tape_contract sums the slabs in the same call,
    with no fill between: t2o_reduce_slabs has a case of its own.)"""
    from t2omca_amd import ops
    assert 0 < dc.nslab < _cus()
    return ops.tape_contract(dc.shape, dc.pack, dc.tape, dc.tiles, dc.slabs, dc.nslab, fmt=dc.fmt)


def _instance_of(A):
    return "exact" if A in (3, 8, 16, 64) else "runtime"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("A", sorted(AGENT_B))
def test_agent_forward(A, T, precision):
    """ops.agent_unroll_fwd, online and target in one launch (T = 1: the tile-loop variant)."""
    require_gpu()
    from t2omca_amd import ops
    sa, _, packs = _nets(A, precision)
    assert sa.instance == _instance_of(A)
    d = _inputs(A, AGENT_B[A], 5)
    obs = d["obs"][:, :T]

    def fn():
        return ops.agent_unroll_fwd(sa, packs["a_on"], obs, h0_on=d["h0"], pack_tg=packs["a_tg"], h0_tg=d["h0"])

    under_each_fill(fn, tag=f"agent fwd A={A} T={T} {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("block_inputs", [True, False], ids=["hmid", "no-hmid"])
@pytest.mark.parametrize("A", sorted(AGENT_B))
def test_agent_bptt(A, block_inputs, precision):
    """ops.agent_unroll_bwd then its tape contraction, LDS filled before each; with and
    without the forward's block inputs (which select the BPTT kernel)."""
    require_gpu()
    from t2omca_amd import ops
    sa, _, packs = _nets(A, precision)
    B, T = AGENT_B[A], T_BWD
    d = _inputs(A, B, T)
    obs = d["obs"]
    hmid = torch.empty(B, T + 1, sa.D - 1, A, sa.E, device="cuda") if block_inputs else None
    q, h = ops.agent_unroll_fwd(sa, packs["a_on"], obs, h0_on=d["h0"], hmid_on=hmid)
    L = sa.layout()
    slabs = torch.empty(int(ops.lib().t2o_agent_bwd_max_slabs(B, A)) * L.grad_total, device="cuda")

    def fn():
        dc, gh0 = ops.agent_unroll_bwd(sa, packs["a_on"], obs, h, h0=d["h0"], gchosen=d["gch"], actions=d["act"],
                                       gh=d["gh"], want_gh0=True, slabs=slabs, hmid=hmid, defer_contract=True)
        refill()
        return dict(gpack=_contract(dc), gh0=gh0)

    under_each_fill(fn, tag=f"agent bptt A={A} {precision}")


SPLITS = {A: ((None,) if A < 16 else ("0", "1")) for A in MIXER_B}
MIXER_CASES = [(A, s) for A in (40, 63, 3, 5, 8, 13, 16, 64) for s in SPLITS[A]]  # (the round-6 failure's first)
MIXER_IDS = [f"A{A}" + ("" if s is None else "-one-wave" if s == "0" else "-decoupled") for A, s in MIXER_CASES]


def _mixer_forward(ops, sm, packs, d, h_on, h_tg, q_on, q_tg, T):
    return ops.mixer_unroll_fwd(sm, packs["m_on"], d["state"], h_on, qmode_on=1, q_on=q_on, actions=d["act"],
                                avail=d["avail32"], T_on=T, pack_tg=packs["m_tg"], hid_tg=h_tg, qmode_tg=2,
                                q_tg=q_tg, T_tg=T + 1)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("A,split", MIXER_CASES, ids=MIXER_IDS)
def test_mixer_forward(monkeypatch, A, split, precision):
    """ops.mixer_unroll_fwd in the learner's Q-selection modes: chosen actions (1) and
    the avail-masked double-Q argmax (2) in one two-network launch, the q_lambda update's
    one-network launch on the target Q at the taken actions, and given qvals (0).  A
    decoupled forward is two kernels in one C call (mixs_fwd_rec_kernel, then
    mixs_fwd_rows_kernel on the same CUs): it runs as the wrapper's phase 1 and phase 2,
    LDS filled before each."""
    require_gpu()
    from t2omca_amd import ops
    if split is not None:
        monkeypatch.setenv("T2O_MIXER_SPLIT", split)
    sa, sm, packs = _nets(A, precision)
    assert sm.instance == _instance_of(A)
    B, T = MIXER_B[A], T_BWD
    d = _inputs(A, B, T)
    q_on, h_on, q_tg, h_tg = ops.agent_unroll_fwd(sa, packs["a_on"], d["obs"], pack_tg=packs["a_tg"])

    decoupled = split == "1"
    if decoupled:
        assert int(ops.lib().t2o_mixer_split(ops.ctypes.byref(sm.layout()), B)) == 1
    E, bufs = sm.E, {}

    def alloc(Tn):
        return dict(y=torch.zeros(B, Tn, device="cuda"), hw=torch.zeros(B, Tn, 3, E, device="cuda"),
                    qv=torch.zeros(B, Tn, A, device="cuda"), xout=torch.zeros(B, Tn, A + 3, E, device="cuda"),
                    xmid=torch.zeros(B, Tn, sm.D - 1, A + 3, E, device="cuda"))

    def before():  # (the decoupled launches write into buffers made before the fill)
        if decoupled:
            bufs.update(on=alloc(T), tg=dict(alloc(T + 1), xmid=None))

    def phased(T1, outs, *args, **kw):
        """A decoupled forward as its two launches, LDS filled before each: the recurrence
        over every step (phase 1), then the parallel rows (phase 2)."""
        ops.mixer_unroll_fwd(*args, outs=outs, phase=1, steps=(0, T1), **kw)
        refill()
        ops.mixer_unroll_fwd(*args, outs=outs, phase=2, **kw)

    def two():
        if decoupled:
            o_on, o_tg = bufs["on"], bufs["tg"]
            phased(T + 1, (o_on, o_tg), sm, packs["m_on"], d["state"], h_on, qmode_on=1, q_on=q_on, actions=d["act"],
                   avail=d["avail32"], T_on=T, pack_tg=packs["m_tg"], hid_tg=h_tg, qmode_tg=2, q_tg=q_tg, T_tg=T + 1)
        else:
            o_on, o_tg = _mixer_forward(ops, sm, packs, d, h_on, h_tg, q_on, q_tg, T)
        out = {"on." + k: v for k, v in o_on.items()}
        out.update({"tg." + k: v for k, v in o_tg.items() if k != "xout"})  # (the target's xout: decoupled scratch)
        return out

    def taken():
        if decoupled:
            phased(T, (bufs["on"], None), sm, packs["m_tg"], d["state"], h_tg, qmode_on=1, q_on=q_tg,
                   actions=d["act"], T_on=T)
            return bufs["on"]
        return ops.mixer_unroll_fwd(sm, packs["m_tg"], d["state"], h_tg, qmode_on=1, q_on=q_tg, actions=d["act"],
                                    T_on=T, want_xout=False)

    def given():
        if decoupled:
            phased(T, (bufs["on"], None), sm, packs["m_on"], d["state"], h_on, qmode_on=0, qv_on=d["qv"], T_on=T)
            return bufs["on"]
        return ops.mixer_unroll_fwd(sm, packs["m_on"], d["state"], h_on, qmode_on=0, qv_on=d["qv"], T_on=T)

    tag = f"mixer fwd A={A} split={split} {precision}"
    under_each_fill(two, before=before, tag=tag + " modes 1+2")
    base = under_each_fill(taken, before=before, tag=tag + " taken")
    under_each_fill(given, before=before, tag=tag + " given qvals")
    assert base["y"].shape == (B, T)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("A,split", MIXER_CASES, ids=MIXER_IDS)
def test_mixer_bptt(monkeypatch, A, split, precision):
    """ops.mixer_unroll_bwd then its tape contraction, LDS filled before each (the
    padding key rows in [Lk, 16·KT) of the runtime instances at 40 and 63 AGVs are where
    an fp32 flat key mask once gave run-dependent gradients).  A decoupled BPTT is two
    kernels in one C call (mixs_bwd_rows_kernel, then the recurrence, mixs_bwd_rec_pipe_kernel
    or mixs_bwd_rec_kernel, on the same CUs): it runs as the wrapper's phase 1 and phase 2
    over every step, LDS filled before each."""
    require_gpu()
    from t2omca_amd import ops
    if split is not None:
        monkeypatch.setenv("T2O_MIXER_SPLIT", split)
    sa, sm, packs = _nets(A, precision)
    B, T = MIXER_B[A], T_BWD
    d = _inputs(A, B, T)
    q_on, h_on = ops.agent_unroll_fwd(sa, packs["a_on"], d["obs"])[:2]
    o_on = ops.mixer_unroll_fwd(sm, packs["m_on"], d["state"], h_on, qmode_on=1, q_on=q_on, actions=d["act"], T_on=T)
    L = sm.layout()
    slabs = torch.empty(int(ops.lib().t2o_mixer_bwd_max_slabs(B)) * L.grad_total, device="cuda")

    decoupled = split == "1"
    bufs = {}

    def before():  # (the decoupled launches share buffers made before the fill)
        if decoupled:
            assert int(ops.lib().t2o_mixer_split(ops.ctypes.byref(L), B)) == 1
            bufs.update(outs=(torch.zeros(B, T, A, device="cuda"), torch.zeros(B, T, A, sm.E, device="cuda")),
                        carry=torch.zeros(B, 3, sm.E, device="cuda"),
                        tape=torch.empty(ops.tape_floats(sm, ops.mixer_tape_tiles(B, T, A, sm)), device="cuda"),
                        work=torch.empty(ops.mixer_work_floats(sm, B, T), device="cuda"))

    def fn():
        if decoupled:
            kw = dict(want_ghw0=True, slabs=slabs, **bufs)
            ops.mixer_unroll_bwd(sm, packs["m_on"], d["state"], h_on, o_on, d["gy"], phase=1, **kw)
            refill()
            contract, gqv, ghid, ghw0 = ops.mixer_unroll_bwd(sm, packs["m_on"], d["state"], h_on, o_on, d["gy"],
                                                             phase=2, steps=(0, T), **kw)
        else:
            contract, gqv, ghid, ghw0 = ops.mixer_unroll_bwd(sm, packs["m_on"], d["state"], h_on, o_on, d["gy"],
                                                             want_ghw0=True, slabs=slabs, defer_contract=True)
        refill()
        return dict(gpack=_contract(contract), gqv=gqv, ghid=ghid, ghw0=ghw0)

    under_each_fill(fn, before=before, tag=f"mixer bptt A={A} split={split} {precision}")


# ---- the whole update ----------------------------------------------------------------------

def _update_case(tag, learner, A, B, T):
    cpu, w = masked_batch(A, B, T, SEED)
    batch, w = to_cuda(cpu), w.cuda()
    snap = Snapshot(learner)

    def fn():
        (graw, qtot, targets, prio), _ = update(learner, batch, w)
        return dict(grad=graw, qtot=qtot, targets=targets, prio=prio.cuda(), params=learner.params.clone())

    under_each_fill(fn, before=snap.restore, tag=tag)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("A,B,T,piped", [(8, 6, 5, False), (16, 3, 4, True)], ids=["A8-sequential", "A16-pipelined"])
def test_whole_update(A, B, T, piped, precision):
    """TDLearner.train from a restored Snapshot, LDS filled once before it: the first
    kernels see the fill itself, every later kernel whose allocation is larger than its
    predecessors' sees it in the remainder (mixer_bwd_pipe_kernel and the step-range
    kernels are reachable only here)."""
    require_gpu()
    learner, _, _ = make_learner(_cfg_of(A), precision=precision, priorities_to_cpu=False)
    assert bool(learner._pipelined(B)) == piped
    _update_case(f"update A={A} {precision}", learner, A, B, T)


def test_whole_update_q_lambda():
    require_gpu()
    learner, _, _ = make_learner(_cfg_of(8), q_lambda=True, priorities_to_cpu=False)
    _update_case("update A=8 q_lambda", learner, 8, 6, 5)


def test_whole_update_noisy_agent():
    require_gpu()
    from tests.test_gpu_learner_noisy import make_noisy_learner
    learner, _, _ = make_noisy_learner(_cfg_of(8), priorities_to_cpu=False)
    _update_case("update A=8 noisy", learner, 8, 6, 5)


def test_whole_update_generic(monkeypatch):
    """T2O_GENERIC=1 at emb 64 / 4 heads: the runtime-shaped kernels sum their gradients
    with float atomics, so the raw gradient is on the 1e-6 summation-order bar; qtot,
    targets and priorities are the same bits.  The parameters after the step cannot be
    compared across fills on that bar: from the restored (zero) Adam state an element's
    step is lr·g / (|g| + eps), which turns a change of 1e-6·max|g| in a gradient element
    near zero into a change of up to lr (measured: 4.7e-6 / 5.7e-6 normwise between fills).
    They are checked exactly instead: under each fill, the parameters the update left must
    be the bits that t2o_adam_step gives from the restored state and that run's own raw
    gradient, replayed after a zero fill (the step is bit-reproducible, tests/test_gpu_adam.py)."""
    require_gpu()
    from t2omca_amd import ops
    monkeypatch.setenv("T2O_GENERIC", "1")
    learner, _, _ = make_learner(_cfg_of(8, E=64, H=4), priorities_to_cpu=False)
    assert learner.sa.instance == "generic" and learner.sm.instance == "generic"
    assert learner.optimizer == "adam"
    A, B, T = 8, 3, 5
    cpu, w = masked_batch(A, B, T, SEED)
    batch, w = to_cuda(cpu), w.cuda()
    snap = Snapshot(learner)
    replay = {}

    def before():
        snap.restore()
        replay.update(p=snap.params.clone(), m=snap.m.clone(), v=snap.v.clone(),
                      ws=torch.empty(int(ops.lib().t2o_adam_workspace_floats()), device="cuda"))

    def fn():
        (graw, qtot, targets, prio), _ = update(learner, batch, w)
        torch.cuda.synchronize()
        ops.lds_fill(0)
        ops.adam_step(replay["p"], graw[:-1], replay["m"], replay["v"], snap.step + 1, lr=learner.lr,
                      betas=learner.betas, eps=learner.eps, weight_decay=learner.wd, max_grad_norm=learner.clip,
                      workspace=replay["ws"], grad_div=graw[-1:])
        assert bool(torch.isfinite(learner.params).all())
        ndiff = int((learner.params != replay["p"]).sum())
        assert ndiff == 0, f"{ndiff} parameters are not the Adam step of the run's own gradient"
        assert not torch.equal(learner.params, snap.params), "the step moved nothing"
        return dict(grad=graw, qtot=qtot, targets=targets, prio=prio.cuda())

    under_each_fill(fn, before=before, sum_order=("grad",), tag="update generic E64H4")


# ---- flat mixers and the GRU agent ---------------------------------------------------------

@pytest.mark.parametrize("key", [flat_grids.QMIX_MIDDLE + ("abs", 1.0), (3, 5, 4, 32, 64, "abs", 1.0)],
                         ids=["middle-M16-H32", "M32-H64"])
def test_qmix(key):
    require_gpu()
    from t2omca_amd import ops
    c = flat_grids.qmix_case(key)
    d = {k: c[k].cuda() for k in ("flat_on", "flat_tg", "states", "q_on", "q_tg", "gy")}
    T = c["q_on"].shape[1]
    st = d["states"][:, :T]

    def fn():
        y_on, y_tg = ops.qmix_fwd(c["shape"], d["flat_on"], d["states"], d["q_on"], params_tg=d["flat_tg"],
                                  qv_tg=d["q_tg"])
        refill()
        go, gqv, slabs, nslab = ops.qmix_bwd(c["shape"], d["flat_on"], st, d["q_on"], d["gy"], launcher=True)
        go(1)
        refill()
        go(2)
        refill()
        gflat = ops.reduce_slabs(slabs, nslab, torch.empty_like(d["flat_on"]))
        return dict(y_on=y_on, y_tg=y_tg, gqv=gqv, gflat=gflat)

    under_each_fill(fn, tag=f"qmix {key}")


def test_qplex():
    require_gpu()
    from t2omca_amd import ops
    from tests.test_gpu_qplex import _dev
    c = flat_grids.qplex_case(flat_grids.QPLEX_MIDDLE)
    d, sh = _dev(c), c["shape"]
    T = c["gy"].shape[1]
    st = d["states"][:, :T]

    def fn():
        y3, y_tg = ops.qplex_fwd(sh, d["flat_on"], d["states"], *d["on"], params_tg=d["flat_tg"], qv_tg=d["tg"][0],
                                 qmax_tg=d["tg"][1], act_tg=d["tg"][2], parts=3)
        refill()
        go, gqv, slabs, nslab = ops.qplex_bwd(sh, d["flat_on"], st, *d["on"], d["gy"], parts=3, launcher=True)
        go(1)
        refill()
        go(2)
        refill()
        gflat = ops.reduce_slabs(slabs, nslab, torch.empty_like(d["flat_on"]))
        return dict(y3=y3, y_tg=y_tg, gqv=gqv, gflat=gflat)

    under_each_fill(fn, tag="qplex middle")


@pytest.mark.parametrize("key", [flat_grids.RNN_MIDDLE, (3, 5, 5, 64, "entity_both")], ids=["middle-H32", "H64"])
def test_rnn_agent(key):
    """rnn_agent_fwd, rnn_agent_bwd, the slab sum.  rnn_agent_bwd launches its BPTT kernel
    and its weight-gradient kernel in one call and exposes no way to split it: the second
    sees the fill only where the first left it (module docstring)."""
    require_gpu()
    from t2omca_amd import ops
    from tests import test_gpu_rnn_agent as tr
    c = flat_grids.rnn_case(key)
    d = tr.to_dev(c)

    def fn():
        fwd = tr.forward(c, d)
        refill()
        slabs, nslab, gh0 = ops.rnn_agent_bwd(c["shape"], d["flat_on"], d["obs"], fwd, T=c["T"], actions=d["actions"],
                                              gchosen=d["gch"], gh=d["gh"], h0=d["h0"], want_gh0=True)
        refill()
        gflat = ops.reduce_slabs(slabs, nslab, torch.empty_like(d["flat_on"]))
        return dict(q_on=fwd["q_on"], h_on=fwd["h_on"], q_tg=fwd["q_tg"], h_tg=fwd["h_tg"], gh0=gh0, gflat=gflat)

    under_each_fill(fn, tag=f"rnn {key}")


# ---- the noisy head ------------------------------------------------------------------------

@pytest.mark.parametrize("B,A,T,E,NA", [(3, 5, 4, 32, 5), (4, 16, 3, 64, 16)], ids=["NA5", "NA16"])
def test_noisy_head(B, A, T, E, NA):
    require_gpu()
    from t2omca_amd import ops
    from tests.test_gpu_noisy_head import _case
    c = _case(B, A, T, E, NA)
    bufs = {}

    def before():
        bufs["q"] = c["q_f"].clone()
        bufs["g"] = [torch.zeros(NA, E, device="cuda"), torch.zeros(NA, device="cuda"),
                     torch.zeros(NA, E, device="cuda"), torch.zeros(NA, device="cuda")]

    def fn():
        ops.noisy_head_fwd(c["h"], bufs["q"], c["u_w"], c["u_b"], c["s_w"], c["s_b"], eps=c["eps"])
        refill()
        gh, gpart = ops.noisy_head_bwd(c["gch"], c["act"], c["h"], c["u_w"], c["s_w"], c["eps"][0], gh_in=c["gh_in"])
        refill()
        ops.noisy_head_wgrad(gpart, B, A, *bufs["g"], eps=c["eps"])
        du_w, du_b, ds_w, ds_b = bufs["g"]
        return dict(q=bufs["q"], gh=gh, du_w=du_w, du_b=du_b, ds_w=ds_w, ds_b=ds_b)

    under_each_fill(fn, before=before, tag=f"noisy head NA={NA}")


# ---- the remaining float kernels -----------------------------------------------------------

@pytest.mark.parametrize("algo", ["sequential", "wave"])
def test_td_loss_and_qlambda(algo):
    """t2o_td_loss and t2o_td_qlambda at B = 7, T = 5; the loss scalar (out["loss"], float
    atomics) on the 1e-6 bar, targets / dL/dQtot / priorities the same bits."""
    require_gpu()
    from t2omca_amd import ops
    from tests.test_gpu_td_loss import _case
    B, T = 7, 5
    qtot, qtgt, reward, term, filled, w = (t.cuda().contiguous() for t in _case(B, T, B * 31 + T))
    taken = torch.randn(B, T, generator=torch.Generator().manual_seed(9)).cuda()

    def loss():
        out = ops.td_loss(qtot, qtgt, reward, term, filled, w, gamma=0.99, td_lambda=0.6, algo=algo)
        return dict(out)

    def qlambda():
        out = ops.td_qlambda(qtot, qtgt, taken, reward, term, filled, w, gamma=0.99, td_lambda=0.6, algo=algo)
        return dict(out)

    under_each_fill(loss, sum_order=("loss",), tag=f"td_loss {algo}")
    under_each_fill(qlambda, sum_order=("loss",), tag=f"td_qlambda {algo}")


@pytest.mark.parametrize("opt", ["adam", "rmsprop"])
def test_optimizer_steps(opt):
    """adam_step / rmsprop_step with clipping on (gradient norm well past max_grad_norm),
    so the norm partials run; n is no multiple of any block size."""
    require_gpu()
    from t2omca_amd import ops
    n = 84007
    g = torch.Generator().manual_seed(4)
    p0, gr = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    m0, v0 = (0.1 * torch.randn(n, generator=g)).cuda(), (0.01 * torch.rand(n, generator=g)).cuda()
    div = torch.full((1,), 3.0, device="cuda")
    assert float(gr.norm()) / 3.0 > 10.0
    bufs = {}

    def before():
        bufs.update(p=p0.clone(), m=m0.clone(), v=v0.clone(), norm=torch.zeros(1, device="cuda"),
                    ws=torch.empty(int(ops.lib().t2o_adam_workspace_floats()), device="cuda"))

    def fn():
        if opt == "adam":
            ops.adam_step(bufs["p"], gr, bufs["m"], bufs["v"], 3, max_grad_norm=10.0, workspace=bufs["ws"],
                          grad_div=div, grad_norm_out=bufs["norm"])
        else:
            ops.rmsprop_step(bufs["p"], gr, bufs["v"], max_grad_norm=10.0, workspace=bufs["ws"], grad_div=div,
                             grad_norm_out=bufs["norm"])
        return dict(p=bufs["p"], m=bufs["m"], v=bufs["v"], norm=bufs["norm"])

    under_each_fill(fn, before=before, tag=opt)


def test_reduce_slabs_and_pack():
    """pack_params / unpack_grads / reduce_slabs of the agent and the mixer, fp32 and bf16.
    The pack is written into a zeroed buffer made before the fill: a bf16 pack's image
    holds matrices only, and the image's vector slots (be, bo and each block's bu, g1, n1,
    c1, c2, g2, n2: 688 bf16 = 344 words at the default network) are written by no kernel
    and read by none (vectors are read from the fp32 pack), so in a fresh torch.empty
    buffer they hold whatever the allocation held."""
    require_gpu()
    from t2omca_amd import ops
    for precision in PRECISIONS:
        for which in ("a", "m"):
            sa, sm, _ = _nets(8, precision)
            shape = sa if which == "a" else sm
            g = torch.Generator().manual_seed(6)
            params = torch.randn(shape.n_params, generator=g).cuda()
            L = shape.layout()
            gpack = torch.randn(L.grad_total, generator=g).cuda()
            n_red = 255 * 64  # t2o_reduce_slabs runs n / 64 workgroups: one fewer than the CUs
            slabs = torch.randn(37 * n_red, generator=g).cuda()
            bufs = {}

            def before():
                bufs["grad"] = torch.zeros(shape.n_params, device="cuda")
                bufs["pack"] = torch.zeros(L.pack_floats, device="cuda")

            def fn():
                pack = ops.pack_params(shape, params, bufs["pack"])
                refill()
                ops.unpack_grads(shape, params, gpack, bufs["grad"])
                refill()
                total = ops.reduce_slabs(slabs, 37, torch.empty(n_red, device="cuda"))
                return dict(pack=pack, grad=bufs["grad"], total=total)

            under_each_fill(fn, before=before, tag=f"pack / unpack / reduce {which} {precision}")


def test_statistics_kernels():
    """t2o_td_stats and t2o_episode_stats: fp64 partial sums through LDS."""
    require_gpu()
    from t2omca_amd import ops
    from tests.test_gpu_stats_kernels import _episode_inputs, _td_inputs
    q, tgt, term, filled = (t.cuda() for t in _td_inputs(7, 5))
    term, filled = term[:, :, 0], filled[:, :, 0]
    under_each_fill(lambda: dict(out=ops.td_stats(q, tgt, term, filled)), tag="td_stats")
    reward, info, done, returns, acc0 = _episode_inputs(257)
    dev = [t.cuda() for t in (reward, info, done, returns)]
    bufs = {}

    def before():
        bufs["acc"] = acc0.cuda()

    under_each_fill(lambda: dict(acc=ops.episode_stats(*dev, bufs["acc"])), before=before, tag="episode_stats")
