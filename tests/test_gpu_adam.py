"""GPU: ops.adam_step (t2o_adam_step: clip_grad_norm_ + Adam on flat fp32 buffers)
against an fp64 restatement of clip_grad_norm_ + torch.optim.Adam (non-amsgrad, L2
weight decay, the lerp form; tests/gpu_util.adam_ref) applied to the fp32 inputs
upcast.

At step 1 from zero moments the update is lr·g/(|g|+eps): β1, β2 and both bias
corrections cancel.  So the cases here run a chain of 4 consecutive calls (step
1..4, moments carried over, a fresh gradient each call) and one call at step 1000
from non-zero random moments, with the clip active (‖g‖ ≈ 5·max_grad_norm),
inactive, and off (max_grad_norm = 0 with workspace=None: grad_norm_out must stay
untouched), weight_decay 0 and 1e-2, grad_div a device scalar (37) and None, at
n = 1, 255, 257 (one block, not full / one element into the second) and
1024·256 + 3 (the grid-stride loop).  A pruned product of 20.  The pruning keeps
weight decay out of the chains at the largest n: at step 1 from zero moments the
update is lr·g/(|g|+eps) with g = grad + weight_decay·p, and an element where the
two cancel to |g| ~ eps turns the fp32 rounding of that sum (2^-24·|weight_decay·p|
~ 6e-11) into lr·6e-11/eps ~ 6e-6 of p, 600 times the bar on the step, in any fp32
Adam; among 2.6e5 elements one such is near certain (|g| < 2.4e-7 has probability
2e-5 per element), among 257 it is not (and the seeds here have none).  The largest
n takes its weight decay at step 1000 from non-zero moments instead.

Inputs: parameters ~ U(-0.1, 0.1), gradients ~ N(0, σ = 1e-2) after the division
by grad_div; where n >= 5 the first five gradient elements are exactly 0, 1e-9,
1e-8, 1e-7 and -1e-8 (times grad_div), so eps and its place matter.  At n = 1 the
lone element stays random (a zero gradient would make the case vacuous) and the
parameter, the gradient and the first moment are drawn non-negative: normwise over
one element is that element's relative error, and a cancelling sum (the lerp of m
towards a gradient of the other sign, g + weight_decay·p) carries its rounding
error in ulps of its operands, not of its result, which the bars below, derived
for the largest element of a vector, do not cover.

In a chain every call is checked from the reference's previous state: the
reference's p, m, v rounded to fp32 are copied into the device buffers before the
call, so errors do not compound.  A second set of buffers runs the chain freely
and is compared at its end with the pure fp64 chain against the same bars x 4.

Bars (derived, not measured; tests/gpu_util.adam_errors):
  m, v            normwise <= 1e-6
  p               max|p_gpu - p_ref| <= 2^-24·max|p_ref| + 1e-5·max|p_ref - p_before|
  grad_norm_out   relative <= 1e-5
A semantic error in β1, β2, a bias correction, the weight-decay place or the clip
coefficient moves p by >= 1e-3 of the step at step >= 2.

Measured on an MI355X (worst over the 20 cases; p as a fraction of its bar):
  per call     m 2.9e-7   v 5.3e-7   p 0.25 of the bar   grad norm 2.6e-7
  free chain   m 3.0e-7   v 4.0e-7   p 0.22 of the x4 bar
"""
import pytest
import torch

from tests.gpu_util import adam_errors, adam_ref, require_gpu

pytestmark = pytest.mark.gpu

BIG = 1024 * 256 + 3
MAX_NORM = 10.0
SPECIAL = (0.0, 1e-9, 1e-8, 1e-7, -1e-8)
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)

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
    (1, "step1000", "active", 0.0, None),
    (1, "step1000", "off", 1e-2, 37.0),
    (255, "step1000", "inactive", 0.0, 37.0),
    (255, "step1000", "off", 1e-2, None),
    (257, "step1000", "active", 1e-2, 37.0),
    (257, "step1000", "inactive", 0.0, None),
    (BIG, "step1000", "active", 1e-2, None),
    (BIG, "step1000", "inactive", 1e-2, 37.0),
    (BIG, "step1000", "off", 0.0, None),
]


def _grad(n, gen, clip, grad_div):
    """A fresh fp32 gradient: N(0, 1e-2) after the division by grad_div, scaled to a
    norm of 5·MAX_NORM where the clip is to engage, the special values first."""
    g = 1e-2 * torch.randn(n, generator=gen, dtype=torch.float64)
    if n == 1:
        g = g.abs()
    if clip == "active":
        g = g * (5 * MAX_NORM / float(g.norm()))
    if n >= len(SPECIAL):
        g[:len(SPECIAL)] = torch.tensor(SPECIAL, dtype=torch.float64)
    return (g * (grad_div or 1.0)).float()


def _call(ops, p, g, m, v, step, clip, wd, gdiv, norm_out):
    kw = dict(HYPER, weight_decay=wd, grad_div=gdiv, grad_norm_out=norm_out)
    if clip == "off":
        ops.adam_step(p, g, m, v, step, max_grad_norm=0.0, workspace=None, **kw)
    else:
        ws = torch.empty(int(ops.lib().t2o_adam_workspace_floats()), device="cuda")
        ops.adam_step(p, g, m, v, step, max_grad_norm=MAX_NORM, workspace=ws, **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,mode,clip,wd,grad_div", CASES)
def test_adam_step_matches_fp64(n, mode, clip, wd, grad_div):
    require_gpu()
    from t2omca_amd import ops
    gen = torch.Generator().manual_seed(n % 1000 + 7 * len(mode) + int(wd * 1e3))
    max_norm = 0.0 if clip == "off" else MAX_NORM
    ref_kw = dict(HYPER, weight_decay=wd, max_norm=max_norm, grad_div=grad_div)
    gdiv = None if grad_div is None else torch.full((1,), grad_div, device="cuda")
    p32 = (0.2 * torch.rand(n, generator=gen) - 0.1).float()
    if mode == "chain":
        steps = [1, 2, 3, 4]
        m32, v32 = torch.zeros(n), torch.zeros(n)
    else:
        steps = [1000]
        m32 = (1e-2 * torch.randn(n, generator=gen)).float()
        v32 = (1e-4 * torch.rand(n, generator=gen)).float()
    if n == 1:  # (module docstring: no cancelling sums in a one-element normwise error)
        p32, m32 = p32.abs(), m32.abs()
    # the free-running chain: device buffers only the kernel writes, and pure fp64
    fp, fm, fv = p32.cuda(), m32.cuda(), v32.cuda()
    free = (p32.double(), m32.double(), v32.double())
    dp, dm, dv = (torch.empty(n, device="cuda") for _ in range(3))
    worst = dict(m=0.0, v=0.0, p=0.0, norm=0.0)
    for step in steps:
        g32 = _grad(n, gen, clip, grad_div)
        g = g32.cuda()
        # one call from the reference's previous state (rounded to fp32)
        dp.copy_(p32), dm.copy_(m32), dv.copy_(v32)
        norm_out = torch.full((1,), 123.0, device="cuda")
        _call(ops, dp, g, dm, dv, step, clip, wd, gdiv, norm_out)
        ref = adam_ref(p32, g32, m32, v32, step, **ref_kw)
        em, ev, ep, bar_p = adam_errors(dp, dm, dv, ref, p32)
        if clip == "off":
            en = 0.0
            assert float(norm_out) == 123.0  # no clipping: grad_norm_out left untouched
        else:
            en = abs(float(norm_out) - ref[3]) / ref[3]
            assert (ref[3] > MAX_NORM) == (clip == "active")
        print(f"n={n} {mode} {clip} wd={wd} div={grad_div} step {step}: m {em:.2e} v {ev:.2e} "
              f"p {ep:.2e} (bar {bar_p:.2e}) norm {en:.2e}")
        assert torch.equal(g.cpu(), g32)  # the gradient is read only
        assert em <= 1e-6 and ev <= 1e-6, (step, em, ev)
        assert ep <= bar_p, (step, ep, bar_p)
        assert en <= 1e-5, (step, en)
        for k, e in (("m", em), ("v", ev), ("p", ep / bar_p), ("norm", en)):
            worst[k] = max(worst[k], e)
        # free-running
        before = free[0]
        _call(ops, fp, g, fm, fv, step, clip, wd, gdiv, None)
        free = adam_ref(free[0], g32, free[1], free[2], step, **ref_kw)[:3]
        p32, m32, v32 = (x.float() for x in ref[:3])
    print(f"  worst per call: m {worst['m']:.2e} v {worst['v']:.2e} p {worst['p']:.2f} of its bar "
          f"norm {worst['norm']:.2e}")
    if mode == "chain":
        em, ev, ep, bar_p = adam_errors(fp, fm, fv, free, before)
        print(f"  free-running chain after {len(steps)} calls: m {em:.2e} v {ev:.2e} p {ep:.2e} (bar {4 * bar_p:.2e})")
        assert em <= 4e-6 and ev <= 4e-6, (em, ev)
        assert ep <= 4 * bar_p, (ep, 4 * bar_p)
