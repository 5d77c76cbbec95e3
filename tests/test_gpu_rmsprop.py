"""GPU: ops.rmsprop_step (t2o_rmsprop_step: clip_grad_norm_ + RMSprop on flat fp32
buffers) against an fp64 restatement of clip_grad_norm_ + torch.optim.RMSprop
(momentum 0, not centered; tests/qlambda_model.rmsprop_ref, itself checked against
torch.optim.RMSprop in tests/test_qlambda_model.py) applied to the fp32 inputs upcast.

Modelled on tests/test_gpu_adam.py, whose conventions (clip, grad_div,
grad_norm_out, workspace) the entry point shares: a chain of 4 consecutive calls
from a zero square_avg (carried over, a fresh gradient each call) and one call
from a non-zero random square_avg ("warm"), with the clip active (‖g‖ ≈
5·max_grad_norm), inactive, and off (max_grad_norm = 0 with workspace=None:
grad_norm_out must stay untouched), weight_decay 0 and 1e-2, grad_div a device scalar
(37) and None, at n = 1, 255, 257 and 1024·256 + 3.  The same pruned product of 20,
for the same reason: at the first call from a zero square_avg the update is
lr·g/(√(1-α)·|g| + eps) with g = grad + weight_decay·p, and an element where the two
cancel to |g| ~ eps/√(1-α) = 1e-7 turns the fp32 rounding of that sum
(2^-24·|weight_decay·p| ~ 6e-11) into lr·6e-11/eps ~ 6e-6 of p, far past the bar on
the step, in any fp32 RMSprop; among 2.6e5 elements one such is near certain, among
257 it is not.  So weight decay stays out of the chains at the largest n, which takes
it from a non-zero square_avg instead.

Inputs as test_gpu_adam.py: parameters ~ U(-0.1, 0.1), gradients ~ N(0, σ = 1e-2)
after the division by grad_div, the first five gradient elements exactly 0, 1e-9,
1e-8, 1e-7, -1e-8 (times grad_div) where n >= 5; at n = 1 the parameter and the
gradient are non-negative (no cancelling sum in a one-element normwise error).

In a chain every call is checked from the reference's previous state rounded to
fp32, so errors do not compound; a second set of buffers runs the chain freely and
is compared at its end with the pure fp64 chain against the same bars x 4.

Bars (derived, not measured; tests/qlambda_model.rmsprop_errors):
  square_avg      normwise <= 1e-6 (three fp32 roundings plus the norm reduction's
                  ~1e-7 through the squared clip coefficient)
  p               max|p_gpu - p_ref| <= 2^-24·max|p_ref| + 1e-5·max|p_ref - p_before|
  grad_norm_out   relative <= 1e-5
"""
import pytest
import torch

from tests.gpu_util import require_gpu
from tests.qlambda_model import rmsprop_errors, rmsprop_ref
from tests.test_gpu_adam import BIG, MAX_NORM, _grad

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-3, alpha=0.99, eps=1e-8)

# (n, mode, clip, weight_decay, grad_div)
CASES = [
    (1, "chain", "inactive", 0.0, None),
    (1, "chain", "active", 1e-2, 37.0),
    (255, "chain", "active", 0.0, None),
    (255, "chain", "inactive", 1e-2, 37.0),
    (255, "chain", "off", 0.0, 37.0),
    (257, "chain", "active", 1e-2, None),
    (257, "chain", "inactive", 0.0, 37.0),
    (257, "chain", "off", 0.0, None),
    (BIG, "chain", "active", 0.0, 37.0),
    (BIG, "chain", "inactive", 0.0, None),
    (BIG, "chain", "off", 0.0, 37.0),
    (1, "warm", "active", 0.0, None),
    (1, "warm", "off", 1e-2, 37.0),
    (255, "warm", "inactive", 0.0, 37.0),
    (255, "warm", "off", 1e-2, None),
    (257, "warm", "active", 1e-2, 37.0),
    (257, "warm", "inactive", 0.0, None),
    (BIG, "warm", "active", 1e-2, None),
    (BIG, "warm", "inactive", 1e-2, 37.0),
    (BIG, "warm", "off", 0.0, None),
]


def _call(ops, p, g, sq, clip, wd, gdiv, norm_out):
    kw = dict(HYPER, weight_decay=wd, grad_div=gdiv, grad_norm_out=norm_out)
    if clip == "off":
        ops.rmsprop_step(p, g, sq, max_grad_norm=0.0, workspace=None, **kw)
    else:
        ws = torch.empty(int(ops.lib().t2o_adam_workspace_floats()), device="cuda")
        ops.rmsprop_step(p, g, sq, max_grad_norm=MAX_NORM, workspace=ws, **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,mode,clip,wd,grad_div", CASES)
def test_rmsprop_step_matches_fp64(n, mode, clip, wd, grad_div):
    require_gpu()
    from t2omca_amd import ops
    gen = torch.Generator().manual_seed(n % 1000 + 7 * len(mode) + int(wd * 1e3))
    max_norm = 0.0 if clip == "off" else MAX_NORM
    ref_kw = dict(HYPER, weight_decay=wd, max_norm=max_norm, grad_div=grad_div)
    gdiv = None if grad_div is None else torch.full((1,), grad_div, device="cuda")
    p32 = (0.2 * torch.rand(n, generator=gen) - 0.1).float()
    if mode == "chain":
        calls, s32 = 4, torch.zeros(n)
    else:
        calls, s32 = 1, (1e-4 * torch.rand(n, generator=gen)).float()
    if n == 1:  # (module docstring: no cancelling sums in a one-element normwise error)
        p32 = p32.abs()
    # the free-running chain: device buffers only the kernel writes, and pure fp64
    fp, fs = p32.cuda(), s32.cuda()
    free = (p32.double(), s32.double())
    dp, ds = (torch.empty(n, device="cuda") for _ in range(2))
    worst = dict(sq=0.0, p=0.0, norm=0.0)
    for call in range(calls):
        g32 = _grad(n, gen, clip, grad_div)
        g = g32.cuda()
        # one call from the reference's previous state (rounded to fp32)
        dp.copy_(p32), ds.copy_(s32)
        norm_out = torch.full((1,), 123.0, device="cuda")
        _call(ops, dp, g, ds, clip, wd, gdiv, norm_out)
        ref = rmsprop_ref(p32, g32, s32, **ref_kw)
        es, ep, bar_p = rmsprop_errors(dp, ds, ref, p32)
        if clip == "off":
            en = 0.0
            assert float(norm_out) == 123.0  # no clipping: grad_norm_out left untouched
        else:
            en = abs(float(norm_out) - ref[2]) / ref[2]
            assert (ref[2] > MAX_NORM) == (clip == "active")
        print(f"n={n} {mode} {clip} wd={wd} div={grad_div} call {call}: sq {es:.2e} p {ep:.2e} (bar {bar_p:.2e}) "
              f"norm {en:.2e}")
        assert torch.equal(g.cpu(), g32)  # the gradient is read only
        assert es <= 1e-6, (call, es)
        assert ep <= bar_p, (call, ep, bar_p)
        assert en <= 1e-5, (call, en)
        for k, e in (("sq", es), ("p", ep / bar_p), ("norm", en)):
            worst[k] = max(worst[k], e)
        # free-running
        before = free[0]
        _call(ops, fp, g, fs, clip, wd, gdiv, None)
        free = rmsprop_ref(free[0], g32, free[1], **ref_kw)[:2]
        p32, s32 = (x.float() for x in ref[:2])
    print(f"  worst per call: sq {worst['sq']:.2e} p {worst['p']:.2f} of its bar norm {worst['norm']:.2e}")
    if mode == "chain":
        es, ep, bar_p = rmsprop_errors(fp, fs, free, before)
        print(f"  free-running chain after {calls} calls: sq {es:.2e} p {ep:.2e} (bar {4 * bar_p:.2e})")
        assert es <= 4e-6, es
        assert ep <= 4 * bar_p, (ep, 4 * bar_p)


def test_rmsprop_step_rejects_bad_arguments():
    """T2O_EINVAL before any launch: a null required pointer, n < 1, a clip without its workspace."""
    require_gpu()
    from t2omca_amd import _lib
    lib = _lib.lib()
    x = torch.zeros(4, device="cuda")
    P = _lib.ptr

    def rc(p, g, sq, ws, n, clip=0.0):
        return lib.t2o_rmsprop_step(P(p), P(g), P(sq), P(ws), n, 1e-3, 0.99, 1e-8, 0.0, clip, None, None, None)
    assert rc(None, x, x, None, 4) == rc(x, None, x, None, 4) == rc(x, x, None, None, 4) == -1
    assert rc(x, x, x, None, 0) == -1
    assert rc(x, x, x, None, 4, clip=10.0) == -1
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0
