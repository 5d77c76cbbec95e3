"""GPU: the mixing heads, the flat mixers and the GRU agent at LARGE magnitudes.

The suite's Q values are O(1): the ELU of the transformer mixer's head (elu1's
exp_fast(x) − 1 branch) sees arguments in about [−10, 12] at 8 AGVs and [−26, 25] at 64,
expm1f / expf of t2o_qmix.hip nothing deeper, and the GRU's gates never saturate.  With
rewards of task-offloading size |Q| is tens to hundreds.  Here, against the same fp64
references at the project's fp32 bars:

  transformer mixer   the cases of tests/test_gpu_sharp_attention.py at (8, 3, 2) and
                      (16, 5, 4), attention as initialised, q_on / q_tg x 50; heads abs,
                      softplus β 0.5 and β 2.0, quadratic, identity; forward (both
                      networks, one launch) 1e-5 and BPTT 2e-5.  At β 2.0 the last norm2
                      gain is x 4, so that softplus's threshold x·β > 20 is crossed in
                      both directions (HEADS below; β 0.5 stays on the soft branch)
  QMIX, QPLEX         ops.qmix_* / ops.qplex_* at the two smallest shapes of
                      tests/test_gpu_qmix.py / test_gpu_qplex.py with Q (and QPLEX's
                      maxima) x Q_SCALE; their bars: forward 1e-5, gradients 3e-5 flat and
                      per block
  GRU agent           tests/test_gpu_rnn_agent.case at (3, 5, 5) and (16, 3, 5), H = 64,
                      rnn.weight_ih / rnn.weight_hh x 8 (RNN_CASES, and why); forward 1e-5,
                      gradients per tensor
                      and dL/dh0 3e-5, a tensor excused only under grad_blocks.FIT_SHARE

Asserted without a device (tests/test_sharp_inputs.py): the oracle's ELU pre-activation
reaches below −100 and above +100 in every transformer-mixer case, some GRU gate
pre-activation exceeds |x| = 15, and each model's own float32 evaluation is within 1/3
of every bar (Q_SCALE: the largest of 50 / 20 / 10 at which that holds: 50).

MEASURED on an MI355X (worst quantity per case; in brackets the model's own float32 figure):

  transformer mixer (8,3,2), ELU pre-activation -1376 .. 1016:  abs 3.8e-7 (1.1e-6)  softplus 0.5 3.4e-6 (2.1e-6)
      softplus 2.0, x·β -28 .. 34: 3.0e-7 (6.8e-7)  quadratic 3.1e-7 (4.3e-7)  identity 4.5e-7 (3.0e-7)
  transformer mixer (16,5,4), ELU pre-activation -2506 .. 2485: abs 3.5e-7 (4.3e-7)  softplus 0.5 8.0e-7 (8.9e-7)
      softplus 2.0, x·β -31 .. 28: 4.6e-7 (7.4e-7)  quadratic 1.3e-6 (7.7e-7)  identity 3.8e-7 (3.0e-7)
  QMIX x50   (1,2,3) worst block 2.3e-6 (5.3e-7)    (3,5,4) flat gradient 9.7e-7 (7.8e-7)
  QPLEX x50  (3,5,4) worst block 2.1e-6 (3.3e-7)    (8,6,5) worst block 7.1e-7 (1.8e-6)
  GRU agent x8  (3,5,5) seed 1, gates up to 15.3: h of the target network 2.8e-6 (1.8e-6)
                (16,3,5) seed 0, gates up to 16.1: h of the target network 5.4e-6 (2.2e-6)
"""
import functools

import pytest
import torch

import tests.test_gpu_qmix as tq
import tests.test_gpu_qplex as tp
import tests.test_gpu_rnn_agent as tr
import tests.test_gpu_sharp_attention as sa
from tests import qmix_model, qplex_model, rnn_model
from tests.gpu_util import flat_from_dict, normwise, require_gpu
from tests.grad_blocks import FIT_SHARE, assert_blocks_fp32
from tests.sharp import fp32_fit, one_thread

pytestmark = pytest.mark.gpu

Q_SCALE = 50.0
HEADS = [("abs", 0.5), ("softplus", 0.5), ("softplus", 2.0), ("quadratic", 0.5), ("identity", 0.5)]
# Softplus is linear past x·β > 20 (nn.Softplus's threshold; posf / dposf in t2o_common.hpp), and
# its argument here is a LayerNorm output, |x| < 6.5 as initialised.  The β 2.0 cases therefore
# multiply the last block's norm2.weight of both networks by NORM2_GAIN: x·β then spans about
# [-31, 33] with 0.6 % of the w1 elements past the threshold (asserted on the CPU), float32 at
# 0.12 of a third of the worst bar.  β 0.5 would need a gain of 12 - 16, where float32 itself is
# at 1.0 - 1.8 of the third: those cases stay on the soft branch only.
NORM2_KEY, NORM2_GAIN, SOFTPLUS_THRESHOLD = "transformer.tblocks.1.norm2.weight", 4.0, 20.0


def crosses_threshold(head, beta):
    return head == "softplus" and beta == 2.0
MIXER_CASES = [(A, B, T, head, beta) for A, B, T in ((8, 3, 2), (16, 5, 4)) for head, beta in HEADS]
ELU_REACH = 100.0


# ---- the transformer mixer's heads ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mixer_case(A, B, T, head, beta):
    c = sa.mixer_inputs(A, B, T, head, 0, q_scale=Q_SCALE)
    c["cfg"] = dict(c["cfg"], qmix_pos_func_beta=beta)
    if crosses_threshold(head, beta):
        for p in (c["p_on"], c["p_tg"]):
            p[NORM2_KEY] = p[NORM2_KEY] * NORM2_GAIN
    c["ref"] = sa.mixer_eval(c)
    return c


@functools.lru_cache(maxsize=None)
def mixer_fit(A, B, T, head, beta):
    c = mixer_case(A, B, T, head, beta)
    return fp32_fit(lambda dtype: sa.mixer_eval(c, dtype), c["ref"], "fp32")


def elu_preactivation(c):
    """qvals · pos(w1) + b1 of the online network per (b, t), from the oracle's final
    query rows (oracle/ref_model.mixer_forward: w1 = the A agent rows, b1 = the next)."""
    A = c["cfg"]["n_agents"]
    x = c["ref"]["on.xout"]
    w1 = qmix_model.pos(x[:, :, :A], c["cfg"]["qmix_pos_func"], c["cfg"]["qmix_pos_func_beta"])
    return torch.einsum("bta,btae->bte", c["chosen"].double(), w1) + x[:, :, A]


@pytest.mark.parametrize("A,B,T,head,beta", MIXER_CASES)
def test_mixer_heads_large_q(A, B, T, head, beta, monkeypatch):
    require_gpu()
    from t2omca_amd import ops
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)
    c = mixer_case(A, B, T, head, beta)
    shape = sa._mixer_shape(c["cfg"], "fp32")
    assert shape.instance in ("exact", "runtime")  # (16 agents with a run-time head: the capacity class)
    params = flat_from_dict(c["p_on"]).cuda()
    runs = []
    for _ in range(2):
        packs, o_on, o_tg = sa._mixer_forward(c, shape, T)
        gpack, gqv, ghid, ghw0 = ops.mixer_unroll_bwd(shape, packs[0], c["states"].cuda(), c["h_on"].cuda(), o_on,
                                                      c["gy"].cuda(), hw0=c["hw0_on"].cuda(),
                                                      ghw_ext=c["ghw"].cuda(), want_ghw0=True)
        grad = torch.zeros_like(params)
        ops.unpack_grads(shape, params, gpack, grad)
        torch.cuda.synchronize()
        runs.append(dict(sa._mixer_fwd_outputs(o_on, o_tg), grad=grad, gqv=gqv, ghid=ghid, ghw0=ghw0))
    assert torch.equal(o_on["qv"].cpu(), c["chosen"]) and torch.equal(o_tg["qv"].cpu(), c["tmax"])
    sa._finite(**runs[0])
    cpu = mixer_fit(A, B, T, head, beta)
    errs = {k: normwise(runs[0][k], c["ref"][k]) for k in sa.FWD_KEYS + sa.BWD_KEYS}
    print(f"large-Q mixer A={A} B={B} T={T} {head} beta={beta}: "
          + " ".join(f"{k} {e:.2e} (cpu {cpu[k]:.2e})" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < sa.mixer_bar("fp32", k), (k, e)
    for k in errs:
        assert torch.equal(runs[0][k], runs[1][k]), f"not reproducible: {k}"


# ---- QMIX -------------------------------------------------------------------------------

QMIX_SHAPES = tq.SHAPES[:2]
FLAT_BARS = dict(y_on=tq.FWD_BAR, y_tg=tq.FWD_BAR, gqv=tq.GRAD_BAR, gflat=tq.GRAD_BAR, block=tq.BLOCK_BAR)


def qmix_eval(c, dtype=torch.float64):
    T = c["q_on"].shape[1]
    pg = {k: v.to(dtype).requires_grad_(True) for k, v in c["p_on"].items()}
    q = c["q_on"].to(dtype).requires_grad_(True)
    y_on = qmix_model.qmix_forward(pg, q, c["states"][:, :T].to(dtype))
    y_tg = qmix_model.qmix_forward({k: v.to(dtype) for k, v in c["p_tg"].items()}, c["q_tg"].to(dtype),
                                   c["states"].to(dtype))
    gs = torch.autograd.grad((y_on * c["gy"].to(dtype)).sum(), [q] + list(pg.values()))
    out = dict(y_on=y_on.detach(), y_tg=y_tg.detach(), gqv=gs[0], gflat=torch.cat([g.reshape(-1) for g in gs[1:]]))
    out.update({"block." + k: g for k, g in zip(pg, gs[1:])})
    return out


@functools.lru_cache(maxsize=None)
def qmix_case(A, B, T, M, H):
    """tests/test_gpu_qmix.case with both networks' Q x Q_SCALE and the fp64 reference of that."""
    base = tq.case(A, B, T, M, H)
    c = dict(base, q_on=base["q_on"] * Q_SCALE, q_tg=base["q_tg"] * Q_SCALE, p_on=qmix_model.param_dict(base["on"]))
    tg_flat, p_tg, off = base["flat_tg"].double(), {}, 0
    for k, v in c["p_on"].items():
        p_tg[k] = tg_flat[off:off + v.numel()].view_as(v)
        off += v.numel()
    c["p_tg"] = p_tg
    c["ref"] = qmix_eval(c)
    return c


def flat_errors(got, ref):
    """Normwise errors of the quantities in `got`, the per-block ones folded into their worst."""
    errs = {k: normwise(v, ref[k]) for k, v in got.items() if not k.startswith("block.")}
    errs["block"] = max(normwise(v, ref[k]) for k, v in got.items() if k.startswith("block."))
    return errs


@functools.lru_cache(maxsize=None)
def qmix_fit(A, B, T, M, H):
    c = qmix_case(A, B, T, M, H)
    with one_thread():
        return flat_errors(qmix_eval(c, torch.float32), c["ref"])


def _split_blocks(gflat, ref):
    out, off = {}, 0
    for k, v in ref.items():
        if k.startswith("block."):
            out[k] = gflat[off:off + v.numel()].view(v.shape)
            off += v.numel()
    assert off == gflat.numel()
    return out


@pytest.mark.parametrize("A,B,T,M,H", QMIX_SHAPES)
def test_qmix_large_q(A, B, T, M, H):
    require_gpu()
    c = qmix_case(A, B, T, M, H)
    y_on, y_tg, gqv, gflat, _ = tq.run(c)
    got = dict(y_on=y_on, y_tg=y_tg, gqv=gqv, gflat=gflat, **_split_blocks(gflat, c["ref"]))
    sa._finite(y_on=y_on, y_tg=y_tg, gqv=gqv, gflat=gflat)
    errs, cpu = flat_errors(got, c["ref"]), qmix_fit(A, B, T, M, H)
    print(f"large-Q qmix {(A, B, T, M, H)} x{Q_SCALE:g}: " + " ".join(f"{k} {e:.2e} (cpu {cpu[k]:.2e})"
                                                                     for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= FLAT_BARS[k], (k, e)
    assert all(torch.equal(a, b) for a, b in zip((y_on, y_tg, gqv, gflat), tq.run(c)[:4]))


# ---- QPLEX ------------------------------------------------------------------------------

QPLEX_SHAPES = tp.SHAPES[:2]
QPLEX_BARS = dict(y1=tp.FWD_BAR, y2=tp.FWD_BAR, y3=tp.FWD_BAR, y_tg=tp.FWD_BAR, gqv=tp.GRAD_BAR, gflat=tp.GRAD_BAR,
                  block=tp.GRAD_BAR)


def qplex_eval(c, dtype=torch.float64):
    NA, T = c["NA"], c["gy"].shape[1]
    pg = {k: v.to(dtype).requires_grad_(True) for k, v in c["p_on"].items()}
    q, m, u = c["rows"]["on"]
    q = q.to(dtype).requires_grad_(True)
    y_v, y_adv = qplex_model.qplex_parts(pg, q, m.to(dtype), u, c["states"][:, :T].to(dtype), NA)
    qt, mt, ut = c["rows"]["tg"]
    y_tg = qplex_model.qplex_forward({k: v.to(dtype) for k, v in c["p_tg"].items()}, qt.to(dtype), mt.to(dtype), ut,
                                     c["states"].to(dtype), NA)
    gs = torch.autograd.grad(((y_v + y_adv) * c["gy"].to(dtype)).sum(), [q] + list(pg.values()))
    out = dict(y1=y_v.detach(), y2=y_adv.detach(), y3=(y_v + y_adv).detach(), y_tg=y_tg.detach(), gqv=gs[0],
               gflat=torch.cat([g.reshape(-1) for g in gs[1:]]))
    out.update({"block." + k: g for k, g in zip(pg, gs[1:])})
    return out


@functools.lru_cache(maxsize=None)
def qplex_case(A, B, T, NA, S, K):
    """tests/test_gpu_qplex.case with Q and the maxima of both networks x Q_SCALE."""
    base = tp.case(A, B, T, NA, S, K)
    rows = {n: (q * Q_SCALE, m * Q_SCALE, u) for n, (q, m, u) in base["rows"].items()}
    c = dict(base, rows=rows, NA=NA)
    tg_flat, p_tg, off = base["flat_tg"].double(), {}, 0
    for k, v in base["p_on"].items():
        p_tg[k] = tg_flat[off:off + v.numel()].view_as(v)
        off += v.numel()
    c["p_tg"] = p_tg
    c["ref"] = qplex_eval(c)
    return c


@functools.lru_cache(maxsize=None)
def qplex_fit(A, B, T, NA, S, K):
    c = qplex_case(A, B, T, NA, S, K)
    with one_thread():
        return flat_errors(qplex_eval(c, torch.float32), c["ref"])


@pytest.mark.parametrize("A,B,T,NA,S,K", QPLEX_SHAPES)
def test_qplex_large_q(A, B, T, NA, S, K):
    require_gpu()
    c = qplex_case(A, B, T, NA, S, K)
    out = tp.run(c)
    y1, y2, y3, y_tg, gqv, gflat = out
    got = dict(y1=y1, y2=y2, y3=y3, y_tg=y_tg, gqv=gqv, gflat=gflat, **_split_blocks(gflat, c["ref"]))
    sa._finite(y1=y1, y2=y2, y3=y3, y_tg=y_tg, gqv=gqv, gflat=gflat)
    errs, cpu = flat_errors(got, c["ref"]), qplex_fit(A, B, T, NA, S, K)
    print(f"large-Q qplex {(A, B, T, NA, S, K)} x{Q_SCALE:g}: " + " ".join(f"{k} {e:.2e} (cpu {cpu[k]:.2e})"
                                                                          for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= QPLEX_BARS[k], (k, e)
    assert_blocks_fp32(gflat, c["ref"]["gflat"], {}, c["p_on"], tag=f"large-Q qplex {(A, B, T, NA, S, K)}")
    assert all(torch.equal(a, b) for a, b in zip(out, tp.run(c)))


# ---- the GRU agent --------------------------------------------------------------------------

GATE_REACH = 15.0
# (A, B, T1, H, input kind, with h0, gain on rnn.weight_ih / rnn.weight_hh, input seed).
# With the gain of 4 first meant for these cases no gate pre-activation of the fp64 model
# exceeds 7.4, in any input kind, with or without h0, so a gain of 4 saturates nothing.
# The cases are the learner's form (entity observations with both one-hots, h0 given); the
# gain is the smallest of 4, 6, 8, 10 and the input seed the first of 0..9 (0: the draw of
# tests/test_gpu_rnn_agent.case; n > 0: observations and h0 redrawn) at which some gate
# exceeds GATE_REACH while the model's own float32 evaluation stays within 1/3 of every
# bar; both conditions are asserted in tests/test_sharp_inputs.py.  The float32 forward
# error grows quickly with the gain (this recurrence amplifies a summation-order change):
# at a gain of 10 every seed of either shape is above the third, at 6 none reaches 15.
# (3, 5, 5): seed 0 reaches 13.0; seed 1 reaches 15.3 with float32 at 0.53 of the third.
# (16, 3, 5): seed 0 reaches 16.1 with float32 at 0.76 of the third.
RNN_CASES = [(3, 5, 5, 64, "entity_both", True, 8.0, 1), (16, 3, 5, 64, "entity_both", True, 8.0, 0)]
RNN_SCALED = ("rnn.weight_ih", "rnn.weight_hh")


def rnn_eval(c, dtype=torch.float64, gates=None):
    """q, h of both networks, the online one's gradient per tensor and dL/dh0, in dtype.
    gates: a list that receives the r / z / n gate pre-activations of the online network."""
    both = c["kind"].endswith("both")
    B, T1, A = c["actions"].shape
    H = c["H"]
    pg = {k: v.to(dtype).requires_grad_(True) for k, v in c["p_on"].items()}
    inputs = rnn_model.build_inputs(c["obs"].to(dtype), c["actions"], tr.NA, both, both)
    h0 = (torch.zeros(B, A, H) if c["h0"] is None else c["h0"]).to(dtype).requires_grad_(True)
    q_on, h_on = rnn_model.unroll(pg, inputs, h0)
    q_tg, h_tg = rnn_model.unroll({k: v.to(dtype) for k, v in c["p_tg"].items()}, inputs, h0.detach())
    if gates is not None:
        with torch.no_grad():
            hp = torch.cat([h0[:, None], h_on[:, :-1]], 1)
            x = torch.relu(inputs @ pg["fc1.weight"].T + pg["fc1.bias"])
            gi = x @ pg["rnn.weight_ih"].T + pg["rnn.bias_ih"]
            gh = hp @ pg["rnn.weight_hh"].T + pg["rnn.bias_hh"]
            r = torch.sigmoid(gi[..., :H] + gh[..., :H])
            gates.append(torch.cat([gi[..., :2 * H] + gh[..., :2 * H], gi[..., 2 * H:] + r * gh[..., 2 * H:]], -1))
    T = c["T"]
    loss = (torch.gather(q_on[:, :T], 3, c["actions"][:, :T].unsqueeze(3)).squeeze(3) * c["gch"].to(dtype)).sum()
    if c["gh"] is not None:
        loss = loss + (h_on[:, :T] * c["gh"].to(dtype)).sum()
    gs = torch.autograd.grad(loss, list(pg.values()) + [h0])
    out = dict(q_on=q_on.detach(), h_on=h_on.detach(), q_tg=q_tg.detach(), h_tg=h_tg.detach(), gh0=gs[-1])
    out.update({"grad." + k: g for k, g in zip(pg, gs[:-1])})
    return out


@functools.lru_cache(maxsize=None)
def rnn_case(A, B, T1, H, kind, with_h0, gain, seed=0):
    """tests/test_gpu_rnn_agent.case with both networks' GRU weights x gain; seed > 0
    redraws the observations and h0 (the same distributions) from their own generator."""
    base = tr.case(A, B, T1, H, kind, with_h0)
    if seed:
        g = torch.Generator().manual_seed(1000 + seed)
        base = dict(base, obs=torch.randn(B, T1, A, tr.obs_width(A, kind), generator=g),
                    h0=0.5 * torch.randn(B, A, H, generator=g) if with_h0 else None)
    assert list(dict(base["on"].named_parameters())) == list(rnn_model.KEYS)
    p_on = rnn_model.param_dict(base["on"])
    tg_flat, p_tg, off = base["flat_tg"].double(), {}, 0
    for k, v in p_on.items():
        p_tg[k] = tg_flat[off:off + v.numel()].view_as(v).clone()
        off += v.numel()
    for p in (p_on, p_tg):
        for k in RNN_SCALED:
            p[k] = p[k] * gain
    c = dict(base, p_on=p_on, p_tg=p_tg, flat_on=flat_from_dict(p_on), flat_tg=flat_from_dict(p_tg), kind=kind, H=H)
    gates = []
    c["ref"] = rnn_eval(c, gates=gates)
    c["gates"] = gates[0]
    c["gp"] = {k[5:]: v for k, v in c["ref"].items() if k.startswith("grad.")}  # (what tr.excused reads)
    return c


@functools.lru_cache(maxsize=None)
def rnn_fit(*case):
    c = rnn_case(*case)
    return fp32_fit(lambda dtype: rnn_eval(c, dtype), c["ref"], attention=False)


def rnn_bars(c):
    """Bar per checked quantity; a tensor under FIT_SHARE is excused (None), at most one."""
    ex = tr.excused(c)
    assert len(ex) <= 1, ex
    bars = {k: tr.FWD_BAR for k in ("q_on", "h_on", "q_tg", "h_tg")}
    bars.update({"grad." + k: (None if k in ex else tr.GRAD_BAR) for k in c["gp"]})
    bars["gh0"] = tr.GRAD_BAR
    return bars


@pytest.mark.parametrize("A,B,T1,H,kind,with_h0,gain,seed", RNN_CASES)
def test_rnn_agent_saturated_gates(A, B, T1, H, kind, with_h0, gain, seed):
    require_gpu()
    from t2omca_amd import ops
    c = rnn_case(A, B, T1, H, kind, with_h0, gain, seed)
    d = tr.to_dev(c)
    f = tr.forward(c, d)
    gflat, gh0, _ = tr.backward(c, d, f)
    got = {k: f[k] for k in ("q_on", "h_on", "q_tg", "h_tg")}
    got["gh0"] = gh0
    off = 0
    for name, shp in ops.rnn_param_blocks(c["shape"].IN, H, tr.NA):
        n = c["gp"][name].numel()
        got["grad." + name] = gflat[off:off + n].view(shp)
        off += n
    assert off == gflat.numel()
    sa._finite(**got)
    bars, cpu = rnn_bars(c), rnn_fit(A, B, T1, H, kind, with_h0, gain, seed)
    gmax = max(float(g.abs().max()) for g in c["gp"].values())
    errs = {}
    for k, bar in bars.items():
        if bar is None:
            assert float(got[k].abs().max()) <= FIT_SHARE * gmax, k
            continue
        errs[k] = normwise(got[k], c["ref"][k])
    reach = float(c["gates"].abs().max())
    print(f"saturated rnn {(A, B, T1, H, kind, with_h0)} x{gain:g} seed {seed}: max |gate pre-activation| {reach:.1f}; "
          + " ".join(f"{k} {e:.2e} (cpu {cpu[k]:.2e})" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= bars[k], (k, e)
    f2 = tr.forward(c, d)
    gflat2, gh02, _ = tr.backward(c, d, f2)
    assert all(torch.equal(f2[k], f[k]) for k in f) and torch.equal(gflat2, gflat) and torch.equal(gh02, gh0)
