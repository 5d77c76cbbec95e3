"""GPU: the agent and mixer unrolls at SHARP attention, against the fp64 oracle.

Everywhere else in the suite the attention scores stay within |s| < 2 (default
initialisation, N(0, 1) inputs: DESIGN.md §6), where exp(s) can neither overflow nor
underflow and the softmax is near uniform: the max subtraction, the chunked agent's
running-max rescale, the -inf padding masks, the BPTT's recomputed probabilities and
the cancellation in p·(gp − dot) are numerically idle.  Here every tokeys / toqueries
weight is multiplied by s (tests/sharp.py: the scores scale by s², the oracle stays
exact): s = 8 for the fp32 forward (score spread > 100, and a score above 88.7 where expf
overflows, so a missing or wrong maximum gives inf / NaN; S_OVERFLOW for the register
agents), s = 6 for the fp32 BPTT, s = 4 for bf16.

Agent (built on tests/test_gpu_agent_prefetch.py): the instance classes of
tests/test_gpu_memory_contract.SHAPES — 5 (runtime, padded entities), 8 (exact), 13
(runtime, 16 class), 16 (exact), 20 (streamed in 8-entity chunks, partial last chunk),
64 (streamed) — and 5 forced generic; q / h, flat gradient and dL/dh0; the BPTT from
the forward's h / hmid on both kernels where t2o_agent_bwd_ranges offers both.
Mixer (built on tests/test_gpu_mixer_prefetch.py): both networks in one launch (online:
chosen-action gather, T steps; target: double-Q argmax under avail, T + 1 steps; non-zero
hyper tokens) at 3, 8 (exact), 5 (runtime), 13 (one full tile), 16 / 20 / 64 (multi-tile,
padding keys, five query tiles), head abs, at 8 agents also softplus (β 0.5) and identity;
the multi-tile shapes under T2O_MIXER_SPLIT=0 and =1, the BPTT under =1 also with
T2O_MIXS_REC=single.  Every case: finite outputs, a second run bit-equal (the generic
BPTT, which sums with float atomics, to test_gpu_memory_contract.REORDER_BAR).

Bars are the project's: fp32 TOL_F32 = 1e-5 (agent forward and BPTT, mixer forward),
TOL_GRAD_F32 = 2e-5 (mixer BPTT); bf16 TOL_Q = 2e-2 / TOL_G = 6e-2 (agent) and BF16_BARS
(mixer), the latter raised for a quantity of a case to 2 x the error of the CPU
bf16-operand emulation of that case where that emulation exceeds half the bar.  That
each case is sharp (and where: hidden token, first and last chunk / key tile) and that
float32 / bf16-operand rounding alone stays below 1/3 / 1/2 of every bar is asserted
without a device in tests/test_sharp_inputs.py; SEEDS holds the input seeds that rule
selected.

MEASURED on an MI355X (normwise; in brackets the CPU figure of the same case: float32 in
the kernels' association, for bf16 the bf16-operand emulation; spread = largest row max −
row min of the scores, top = largest score, p = mean max-probability):

  agent (A,B,T)   s   spread  top    p     worst of q, h          s  spread  p     BPTT: worst of grad, dL/dh0
  (5,3,4)         8   130    77.7  0.95   3.7e-7 (4.7e-7)        6   62    0.88   1.8e-6 (1.6e-6), both kernels
  (5,3,4)        10   172   103.5  0.95   9.8e-7 (1.3e-6)
  (5,3,4) generic 8 / 10 / 6              3.4e-7 / 5.0e-7                          4.0e-6 (1.6e-6)
  (8,3,5)         8   117    79.9  0.92   6.8e-7 (8.5e-7)        6   66    0.86   2.1e-6 (1.5e-6)
  (8,3,5)        10   226   106.7  0.94   1.8e-6 (1.5e-6)
  (13,3,4)        8   133   100.4  0.90   1.0e-6 (6.2e-7)        6   71    0.84   2.2e-6 (1.5e-6)
  (16,3,4)        8   111    71.1  0.89   1.2e-6 (1.1e-6)        6   68    0.81   1.2e-6 (1.5e-6)
  (16,3,4)       10   170   111.4  0.93   9.8e-7 (1.0e-6)
  (20,2,4)        8   161    98.2  0.89   7.0e-7 (9.9e-7)        6   59    0.80   2.8e-6 (1.5e-6)
  (64,2,3)        8   146    95.2  0.86   9.7e-7 (1.3e-6)        6   81    0.74   3.7e-6 (1.7e-6)
  bf16, s = 4 (spread 28 - 36, p 0.48 - 0.74): q, h 3.2e-3 - 7.8e-3 (3.8e-3 - 8.6e-3);
  BPTT (8,3,5) grad 2.9e-2 (2.9e-2) dL/dh0 1.8e-2 (2.1e-2); (64,2,3) 2.1e-2 (2.3e-2), 2.6e-2 (2.7e-2).

  mixer (A,B,T)   s=8: spread  top    p    worst forward quantity      s=6: spread  p     worst BPTT quantity
  (3,6,2)              140   104.2  0.94  tg.hw 2.8e-6 (8.6e-7)            80    0.90   ghw0 2.7e-6 (1.5e-6)
  (8,3,2)              179   124.0  0.94  xout 2.3e-6 (1.1e-6)            100    0.89   ghw0 1.8e-6 (2.8e-6)
  (8,3,2) softplus / identity             xout 2.3e-6 (1.1e-6)                          2.3e-6 / 2.2e-6
  (5,7,2)              183   105.2  0.94  xout 1.9e-6 (8.8e-7)            103    0.89   ghw0 4.4e-6 (2.4e-6)
  (13,3,4)             187   102.6  0.93  tg.hw 3.8e-6 (3.1e-6)           100    0.88   grad 3.9e-6 (2.1e-6)
  (16,5,4)             173   111.2  0.92  tg.hw 6.1e-6 (2.6e-6)            98    0.86   grad 3.7e-6 (5.7e-6)
  (20,2,4)             194   120.6  0.93  xout 1.7e-6 (1.7e-6)            106    0.87   ghid 4.0e-6 (3.4e-6)
  (64,2,3)             264   135.0  0.92  on.hw 3.0e-6 (1.6e-6)           123    0.85   ghid 3.7e-6 (2.9e-6)
  The multi-tile families agree: forward bit for bit, BPTT to the third digit.
  bf16, s = 4 (spread 35 - 56, p 0.66 - 0.79): worst forward quantity 4.5e-3 - 8.0e-3
  (4.5e-3 - 9.4e-3), hw / xout / xmid equal to the emulation's figure to three digits in
  most cases; BPTT (8,3,2) grad 4.8e-2 (4.3e-2), gqv 1.2e-3, ghid 1.0e-2, ghw0 2.3e-2.

With the maximum removed from mixer_block_fwd and agent_block_fwd_ch in a scratch build
(arithmetic only; never committed) the 86 tests of test_gpu_agent / _mixer / _agent_prefetch
/ _mixer_prefetch still pass, and the twelve fp32 mixer forwards and the two chunked-agent
fp32 forwards here fail with non-finite outputs.
"""
import functools

import pytest
import torch

from oracle import ref_model
from tests.gpu_util import flat_from_dict, normwise, require_gpu
from tests.sharp import fp32_fit, sharpen
from tests.test_gpu_agent import TOL_F32
from tests.test_gpu_agent_prefetch import _cfg as _agent_cfg
from tests.test_gpu_agent_prefetch import _forward as _agent_forward
from tests.test_gpu_agent_prefetch import _gpu_shape as _agent_shape
from tests.test_gpu_bf16 import TOL_G, TOL_Q
from tests.test_gpu_memory_contract import EXACT, REORDER_BAR
from tests.test_gpu_memory_contract import SHAPES as CONTRACT_SHAPES
from tests.test_gpu_mixer_prefetch import BF16_BARS, TOL_GRAD_F32
from tests.test_gpu_mixer_prefetch import _cfg as _mixer_cfg
from tests.test_gpu_mixer_prefetch import _forward as _mixer_forward
from tests.test_gpu_mixer_prefetch import _gpu_shape as _mixer_shape
from tests.test_gpu_mixer_prefetch import _query_rows

pytestmark = pytest.mark.gpu

S_FWD, S_BWD, S_BF16 = 8, 6, 4
# A score spread above 100 does not by itself put a score above ln(FLT_MAX) = 88.73, where
# expf without the maximum is inf: the register agents' (5, 8, 16 entities) largest score at
# s = 8 is 61 - 86 at every input seed 0..9, and a forward without the max subtraction
# would pass them.  They run the fp32 forward at s = 10 as well (largest score 104 - 110);
# the 13-entity agent, the chunked agents and every mixer case overflow at s = 8 (asserted in
# tests/test_sharp_inputs.py).
S_OVERFLOW = 10
AGENT_REGISTER = (5, 8, 16)

# ---- the cases ----------------------------------------------------------------------

# (A, B, T, forced generic); the instance class each must run is CONTRACT_SHAPES'
AGENT_CASES = [(5, 3, 4, False), (8, 3, 5, False), (13, 3, 4, False), (16, 3, 4, False), (20, 2, 4, False),
               (64, 2, 3, False), (5, 3, 4, True)]
AGENT_BF16_BWD = [(8, 3, 5), (64, 2, 3)]
AGENT_INSTANCE = {s[0]: "exact" if s[3] == EXACT else "runtime" for s in CONTRACT_SHAPES}
AGENT_CHUNKED = (20, 64)
AGENT_OVERFLOW_AT_S_FWD = (13, 20, 64)  # a score above ln(FLT_MAX) at s = 8 (the register agents: at S_OVERFLOW)

MIXER_SHAPES = [(3, 6, 2), (8, 3, 2), (5, 7, 2), (13, 3, 4), (16, 5, 4), (20, 2, 4), (64, 2, 3)]
MIXER_MULTI_TILE = (16, 20, 64)
MIXER_CASES = [(A, B, T, "abs") for A, B, T in MIXER_SHAPES] + [(8, 3, 2, "softplus"), (8, 3, 2, "identity")]
MIXER_BF16_BWD = (8, 3, 2, "abs")
MIXER_INSTANCE = {3: "exact", 8: "exact", 5: "runtime", 13: "runtime", 16: "exact", 20: "runtime", 64: "exact"}
# kernel families of the multi-tile mixers: (T2O_MIXER_SPLIT, T2O_MIXS_REC)
FWD_FAMILIES = {"one-wave": ("0", None), "split": ("1", None)}
BWD_FAMILIES = dict(FWD_FAMILIES, **{"split-single": ("1", "single")})

# Input seed per case (default 0): the first seed from 0 upward at which the case is sharp
# enough (the fp32 forward cases of the chunked agents and of every mixer: with a score above
# ln(FLT_MAX) too) and float32 / bf16-operand rounding alone stays below 1/3 / 1/2 of every
# bar the case is held to — found on the CPU from the oracle alone, and asserted there
# (tests/test_sharp_inputs.py).  Keys: ("agent" | "mixer", A, B, T[, head], s).  float32
# itself sits at 2e-6 - 6e-6 in these cases, close to a third of the 1e-5 bars, and its
# figure moves by tens of percent with the order of the float32 sums; so the search asked for
# 0.6 of the asserted share, except at mixer (13,3,4) s=8 and (16,5,4) s=8 and s=6, where no
# seed in 0..9 leaves that headroom and the first seed within the plain third stands.
# Examples of what the skipped seeds gave: agent (13,3,4) s=6 seed 0 dL/dh0 1.2e-5 of 1e-5;
# mixer (8,3,2) s=8 seed 0 the target network's hw 6.7e-6 of 1e-5; mixer (20,2,4) s=6 ghid
# 1.2e-5 / 2.4e-5 of 2e-5 at seeds 0 / 1; the chunked agents' largest score at s=8 is 67.8 /
# 76.0 (20) and 84.4 / 87.1 (64) at seeds 0 / 1: no overflow.  No case needed a lower scale.
# Agent (5,3,4) s=6: at seed 0 dL/dh0 is sensitive to the float32 summation order (9.4e-7 and
# 3.5e-6 of 1e-5 with two orders of the same sums); seed 3 is the first that keeps the headroom
# under both (1.9e-6 / 1.6e-6).
SEEDS = {("agent", 5, 3, 4, 8): 2, ("agent", 8, 3, 5, 8): 1, ("agent", 20, 2, 4, 8): 2, ("agent", 64, 2, 3, 8): 2,
         ("agent", 16, 3, 4, 10): 1, ("agent", 5, 3, 4, 6): 3, ("agent", 8, 3, 5, 6): 1,
         ("agent", 13, 3, 4, 6): 8, ("agent", 16, 3, 4, 6): 3,
         ("agent", 20, 2, 4, 6): 3, ("agent", 64, 2, 3, 6): 1, ("agent", 64, 2, 3, 4): 1,
         ("mixer", 3, 6, 2, "abs", 8): 3, ("mixer", 8, 3, 2, "abs", 8): 1, ("mixer", 13, 3, 4, "abs", 8): 1,
         ("mixer", 20, 2, 4, "abs", 8): 1, ("mixer", 64, 2, 3, "abs", 8): 1, ("mixer", 8, 3, 2, "softplus", 8): 1,
         ("mixer", 8, 3, 2, "identity", 8): 1, ("mixer", 3, 6, 2, "abs", 6): 2, ("mixer", 8, 3, 2, "abs", 6): 1,
         ("mixer", 13, 3, 4, "abs", 6): 3, ("mixer", 20, 2, 4, "abs", 6): 9, ("mixer", 64, 2, 3, "abs", 6): 2,
         ("mixer", 8, 3, 2, "softplus", 6): 1, ("mixer", 8, 3, 2, "identity", 6): 3}


def _seed(*key):
    return SEEDS.get(key, 0)


# ---- agent ------------------------------------------------------------------------------

def agent_eval(c, dtype=torch.float64):
    """The oracle's q, h, flat gradient and dL/dh0 of an agent case, in dtype."""
    pd = {k: v.to(dtype).requires_grad_(True) for k, v in c["p"].items()}
    h0 = c["h0"].to(dtype).requires_grad_(True)
    q, h = ref_model.agent_unroll(pd, c["obs"].to(dtype), h0, cfg=c["cfg"])
    gs = torch.autograd.grad((q * c["gq"].to(dtype)).sum() + (h * c["gh"].to(dtype)).sum(), list(pd.values()) + [h0])
    return dict(q=q.detach(), h=h.detach(), grad=torch.cat([x.reshape(-1) for x in gs[:-1]]), gh0=gs[-1])


@functools.lru_cache(maxsize=None)
def agent_case(A, B, T, s):
    """Inputs (as tests/test_gpu_agent_prefetch._case draws them), the parameters
    sharpened by s, and the fp64 oracle's outputs and gradients; computed once."""
    cfg = _agent_cfg(A)
    g = torch.Generator().manual_seed(100 * A + 10 * B + T + 1000 * _seed("agent", A, B, T, s))
    c = dict(cfg=cfg, s=s, p=sharpen(ref_model.init_params("agent", cfg, 7 + A), s),
             obs=torch.randn(B, T, A, A * 9, generator=g), h0=torch.randn(B, A, 32, generator=g),
             gq=torch.randn(B, T, A, 5, generator=g), gh=torch.randn(B, T, A, 32, generator=g))
    c.update(agent_eval(c))
    return c


@functools.lru_cache(maxsize=None)
def agent_fit(A, B, T, s, prec):
    """Errors of float32 (prec fp32) / bf16-operand (bf16) rounding alone on the case."""
    c = agent_case(A, B, T, s)
    return fp32_fit(lambda dtype: agent_eval(c, dtype), c, prec)


def _agent_setup(A, generic, prec, monkeypatch):
    monkeypatch.setenv("T2O_GENERIC", "1" if generic else "0")
    shape = _agent_shape(_agent_cfg(A), prec)
    want = "generic" if generic else AGENT_INSTANCE[A]
    assert shape.instance == want, f"agent of {A} entities runs {shape.instance}, this case is meant to run {want}"
    return shape


def _finite(**ts):
    for k, t in ts.items():
        assert bool(torch.isfinite(t).all()), f"{k}: non-finite values"


AGENT_FWD_RUNS = ([c + (prec, s) for c in AGENT_CASES for prec, s in (("fp32", S_FWD), ("bf16", S_BF16))]
                  + [c + ("fp32", S_OVERFLOW) for c in AGENT_CASES if c[0] in AGENT_REGISTER])


@pytest.mark.parametrize("A,B,T,generic,prec,s", AGENT_FWD_RUNS)
def test_agent_fwd_sharp(A, B, T, generic, prec, s, monkeypatch):
    require_gpu()
    shape = _agent_setup(A, generic, prec, monkeypatch)
    c = agent_case(A, B, T, s)
    _, q, h, _ = _agent_forward(c, shape)
    _, q2, h2, _ = _agent_forward(c, shape)
    _finite(q=q, h=h)
    eq, eh = normwise(q, c["q"]), normwise(h, c["h"])
    cpu = agent_fit(A, B, T, s, prec)
    print(f"sharp agent fwd A={A} B={B} T={T} s={s} {prec}{' generic' if generic else ''}: q {eq:.2e} h {eh:.2e}"
          f" (cpu {prec}: q {cpu['q']:.2e} h {cpu['h']:.2e})")
    tol = TOL_F32 if prec == "fp32" else TOL_Q
    assert eq < tol and eh < tol, (eq, eh)
    assert torch.equal(q, q2) and torch.equal(h, h2), "agent forward not reproducible"


def _agent_bptt(A, B, T, generic, prec, s, monkeypatch):
    from t2omca_amd import ops
    shape = _agent_setup(A, generic, prec, monkeypatch)
    c = agent_case(A, B, T, s)
    monkeypatch.delenv("T2O_AGENT_BWD", raising=False)
    both = int(ops.lib().t2o_agent_bwd_ranges(ops.ctypes.byref(shape.layout()), 1)) == 1
    params = flat_from_dict(c["p"]).cuda()
    cpu = agent_fit(A, B, T, s, prec)
    tol = TOL_F32 if prec == "fp32" else TOL_G
    for mode in ("pipe", "single") if both else ("default",):
        if mode == "single":
            monkeypatch.setenv("T2O_AGENT_BWD", "single")
            assert int(ops.lib().t2o_agent_bwd_ranges(ops.ctypes.byref(shape.layout()), 1)) == 0
        runs = []
        for _ in range(2):
            pack, q, h, hm = _agent_forward(c, shape, hmid=True)
            gpack, gh0 = ops.agent_unroll_bwd(shape, pack, c["obs"].cuda(), h, h0=c["h0"].cuda().contiguous(),
                                              gq=c["gq"].cuda(), gh=c["gh"].cuda(), want_gh0=True, hmid=hm)
            grad = torch.zeros_like(params)
            ops.unpack_grads(shape, params, gpack, grad)
            torch.cuda.synchronize()
            runs.append((grad, gh0))
        (grad, gh0), (grad2, gh02) = runs
        _finite(grad=grad, gh0=gh0)
        eg, e0 = normwise(grad, c["grad"]), normwise(gh0, c["gh0"])
        print(f"sharp agent bptt A={A} B={B} T={T} s={s} {prec}{' generic' if generic else ''} {mode}: grad {eg:.2e}"
              f" gh0 {e0:.2e} (cpu {prec}: grad {cpu['grad']:.2e} gh0 {cpu['gh0']:.2e})")
        assert eg < tol and e0 < tol, (mode, eg, e0)
        if generic:  # float atomics: the same terms in an order that varies run to run
            assert normwise(grad2, grad) < REORDER_BAR and normwise(gh02, gh0) < REORDER_BAR
        else:
            assert torch.equal(grad, grad2) and torch.equal(gh0, gh02), "agent BPTT not reproducible"


@pytest.mark.parametrize("A,B,T,generic", AGENT_CASES)
def test_agent_bptt_sharp_fp32(A, B, T, generic, monkeypatch):
    """BPTT from the forward's h / hmid at s = 6: the pipelined and the one-wave kernel
    (T2O_AGENT_BWD=single) where t2o_agent_bwd_ranges offers both, else the one there is."""
    require_gpu()
    _agent_bptt(A, B, T, generic, "fp32", S_BWD, monkeypatch)


@pytest.mark.parametrize("A,B,T", AGENT_BF16_BWD)
def test_agent_bptt_sharp_bf16(A, B, T, monkeypatch):
    require_gpu()
    _agent_bptt(A, B, T, False, "bf16", S_BF16, monkeypatch)


# ---- mixer ------------------------------------------------------------------------------

FWD_KEYS = ("on.y", "on.hw", "on.xout", "on.xmid", "tg.y", "tg.hw")
BWD_KEYS = ("grad", "gqv", "ghid", "ghw0")


def mixer_eval(c, dtype=torch.float64):
    """The oracle's checked quantities of a mixer case in dtype: the online network's
    y, hw, query rows after each block and gradients, the target network's y and hw."""
    cfg, T = c["cfg"], c["T"]
    pd = {k: v.to(dtype).requires_grad_(True) for k, v in c["p_on"].items()}
    qv = c["chosen"].to(dtype).requires_grad_(True)
    hid = c["h_on"][:, :T].to(dtype).requires_grad_(True)
    hw0 = c["hw0_on"].to(dtype).requires_grad_(True)
    st = c["states"].to(dtype)
    y, hw = ref_model.mixer_unroll(pd, qv, hid, st[:, :T], hw0, cfg=cfg)
    gs = torch.autograd.grad((y * c["gy"].to(dtype)).sum() + (hw * c["ghw"].to(dtype)).sum(),
                             list(pd.values()) + [qv, hid, hw0])
    with torch.no_grad():
        xmid, xout = _query_rows(pd, cfg, hid, st[:, :T], hw0, hw)
        yt, hwt = ref_model.mixer_unroll({k: v.to(dtype) for k, v in c["p_tg"].items()}, c["tmax"].to(dtype),
                                         c["h_tg"].to(dtype), st, c["hw0_tg"].to(dtype), cfg=cfg)
    return {"on.y": y.detach(), "on.hw": hw.detach(), "on.xout": xout, "on.xmid": xmid, "tg.y": yt, "tg.hw": hwt,
            "grad": torch.cat([x.reshape(-1) for x in gs[:-3]]), "gqv": gs[-3], "ghid": gs[-2], "ghw0": gs[-1]}


def mixer_inputs(A, B, T, head, seed, q_scale=1.0):
    """Parameters and inputs as tests/test_gpu_mixer_prefetch._case draws them."""
    cfg = _mixer_cfg(A, head)
    g = torch.Generator().manual_seed(1000 * A + 10 * B + T + 100000 * seed)
    Tq = T + 1
    c = dict(cfg=cfg, T=T, p_on=ref_model.init_params("mixer", cfg, 41 + A),
             p_tg=ref_model.init_params("mixer", cfg, 42 + A),
             states=torch.randn(B, Tq, A * 8, generator=g), h_on=torch.randn(B, Tq, A, 32, generator=g),
             h_tg=torch.randn(B, Tq, A, 32, generator=g), q_on=q_scale * torch.randn(B, Tq, A, 5, generator=g),
             q_tg=q_scale * torch.randn(B, Tq, A, 5, generator=g),
             actions=torch.randint(0, 5, (B, Tq, A, 1), generator=g),
             hw0_on=torch.randn(B, 3, 32, generator=g), hw0_tg=torch.randn(B, 3, 32, generator=g),
             gy=torch.randn(B, T, generator=g), ghw=torch.randn(B, T, 3, 32, generator=g))
    avail = (torch.rand(B, Tq, A, 5, generator=g) > 0.3).int()
    avail[..., 0] = 1
    c["avail"] = avail
    c["chosen"] = torch.gather(c["q_on"][:, :T], 3, c["actions"][:, :T]).squeeze(3)
    qd = c["q_on"].clone()
    qd[avail == 0] = -9999999
    c["tmax"] = torch.gather(c["q_tg"], 3, qd.max(dim=3, keepdim=True)[1]).squeeze(3)
    return c


@functools.lru_cache(maxsize=None)
def mixer_case(A, B, T, head, s):
    """Both networks sharpened by s, and the fp64 oracle's outputs and gradients."""
    c = mixer_inputs(A, B, T, head, _seed("mixer", A, B, T, head, s))
    c["s"] = s
    c["p_on"], c["p_tg"] = sharpen(c["p_on"], s), sharpen(c["p_tg"], s)
    c["ref"] = mixer_eval(c)
    return c


@functools.lru_cache(maxsize=None)
def mixer_fit(A, B, T, head, s, prec):
    c = mixer_case(A, B, T, head, s)
    return fp32_fit(lambda dtype: mixer_eval(c, dtype), c["ref"], prec)


def mixer_bar(prec, k, emu=None):
    """The bar of quantity k ("on.y", "grad", ...).  bf16: BF16_BARS, or 2 x the CPU
    emulation's error of the same case where that exceeds half of it."""
    k = k.split(".")[-1]
    if prec == "fp32":
        return TOL_F32 if k in ("y", "hw", "xout", "xmid") else TOL_GRAD_F32
    return BF16_BARS[k] if emu is None else max(BF16_BARS[k], 2.0 * emu)


def _mixer_setup(A, head, prec, family, families, monkeypatch):
    monkeypatch.setenv("T2O_GENERIC", "0")
    split, rec = families.get(family, (None, None))
    for name, val in (("T2O_MIXER_SPLIT", split), ("T2O_MIXS_REC", rec)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    shape = _mixer_shape(_mixer_cfg(A, head), prec)
    assert shape.instance == MIXER_INSTANCE[A], (shape.instance, MIXER_INSTANCE[A])
    return shape


def _mixer_fwd_outputs(o_on, o_tg):
    return {"on.y": o_on["y"], "on.hw": o_on["hw"], "on.xout": o_on["xout"], "on.xmid": o_on["xmid"],
            "tg.y": o_tg["y"], "tg.hw": o_tg["hw"]}


def _families(cases, families):
    return [pytest.param(*c, fam, id="-".join(str(x) for x in c) + "-" + fam) for c in cases
            for fam in (families if c[0] in MIXER_MULTI_TILE else ("default",))]


def _mixer_fwd(A, B, T, head, family, prec, s, monkeypatch):
    shape = _mixer_setup(A, head, prec, family, FWD_FAMILIES, monkeypatch)
    c = mixer_case(A, B, T, head, s)
    _, o_on, o_tg = _mixer_forward(c, shape, T)
    _, r_on, r_tg = _mixer_forward(c, shape, T)
    assert torch.equal(o_on["qv"].cpu(), c["chosen"])
    assert torch.equal(o_tg["qv"].cpu(), c["tmax"])
    got = _mixer_fwd_outputs(o_on, o_tg)
    _finite(**got)
    cpu = mixer_fit(A, B, T, head, s, prec)
    errs = {k: normwise(got[k], c["ref"][k]) for k in FWD_KEYS}
    print(f"sharp mixer fwd A={A} B={B} T={T} {head} s={s} {prec} {family}: "
          + " ".join(f"{k} {e:.2e} (cpu {cpu[k]:.2e})" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < mixer_bar(prec, k, cpu[k]), (k, e, mixer_bar(prec, k, cpu[k]))
    for o, r in ((o_on, r_on), (o_tg, r_tg)):
        for k in ("y", "hw", "qv", "xout", "xmid"):
            assert (o[k] is None and r[k] is None) or torch.equal(o[k], r[k]), f"mixer forward not reproducible: {k}"


@pytest.mark.parametrize("A,B,T,head,family", _families(MIXER_CASES, FWD_FAMILIES))
def test_mixer_fwd_sharp_fp32(A, B, T, head, family, monkeypatch):
    require_gpu()
    _mixer_fwd(A, B, T, head, family, "fp32", S_FWD, monkeypatch)


@pytest.mark.parametrize("A,B,T,head,family", _families(MIXER_CASES, FWD_FAMILIES))
def test_mixer_fwd_sharp_bf16(A, B, T, head, family, monkeypatch):
    require_gpu()
    _mixer_fwd(A, B, T, head, family, "bf16", S_BF16, monkeypatch)


def _mixer_bptt(A, B, T, head, family, prec, s, monkeypatch):
    from t2omca_amd import ops
    shape = _mixer_setup(A, head, prec, family, BWD_FAMILIES, monkeypatch)
    c = mixer_case(A, B, T, head, s)
    params = flat_from_dict(c["p_on"]).cuda()
    runs = []
    for _ in range(2):
        packs, o_on, _ = _mixer_forward(c, shape, T)
        gpack, gqv, ghid, ghw0 = ops.mixer_unroll_bwd(shape, packs[0], c["states"].cuda(), c["h_on"].cuda(), o_on,
                                                      c["gy"].cuda(), hw0=c["hw0_on"].cuda(),
                                                      ghw_ext=c["ghw"].cuda(), want_ghw0=True)
        grad = torch.zeros_like(params)
        ops.unpack_grads(shape, params, gpack, grad)
        torch.cuda.synchronize()
        runs.append(dict(grad=grad, gqv=gqv, ghid=ghid, ghw0=ghw0))
    _finite(**runs[0])
    cpu = mixer_fit(A, B, T, head, s, prec)
    errs = {k: normwise(runs[0][k], c["ref"][k]) for k in BWD_KEYS}
    print(f"sharp mixer bptt A={A} B={B} T={T} {head} s={s} {prec} {family}: "
          + " ".join(f"{k} {e:.2e} (cpu {cpu[k]:.2e})" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < mixer_bar(prec, k, cpu[k]), (k, e, mixer_bar(prec, k, cpu[k]))
    for k in errs:
        assert torch.equal(runs[0][k], runs[1][k]), f"mixer BPTT not reproducible: {k}"


@pytest.mark.parametrize("A,B,T,head,family", _families(MIXER_CASES, BWD_FAMILIES))
def test_mixer_bptt_sharp_fp32(A, B, T, head, family, monkeypatch):
    """The BPTT from the forward's stored xmid / hw / xout / qv at s = 6; the multi-tile
    shapes on the one-wave kernels, decoupled, and decoupled with the one-wave recurrence."""
    require_gpu()
    _mixer_bptt(A, B, T, head, family, "fp32", S_BWD, monkeypatch)


def test_mixer_bptt_sharp_bf16(monkeypatch):
    require_gpu()
    _mixer_bptt(*MIXER_BF16_BWD, "default", "bf16", S_BF16, monkeypatch)
