"""GPU: the NoisyNet head kernels alone (t2o_noise_normal, t2o_noisy_head_fwd / _bwd /
_wgrad through t2omca_amd.ops) against the fp64 restatement tests/noisy_model.py, and
the drop-in agent's training-mode forward / autograd through them.

Shapes (B, A, T, E, NA): row counts B·A below (6, 15), at (64) and across (72) a
wave's 64 rows, E and NA at the kernels' limits (64, 16), and E = 16 / 32 / 64 for
the 4 / 8 / 16 lanes that share a row.  h is what the agent unroll of a seeded module
produced (so the mean head can be held against the fused kernel's own q); the means are
the module's, the sigmas 0.3·N(0, 1): every element distinct, a dropped or transposed ε
shows.  Bars: noise within one fp32 ulp of the numpy value (both evaluate Box–Muller in
fp64 from identical uniforms and can differ only in the final rounding); forward and
gh_out 1e-5 normwise, weight gradients 3e-5 (the learner tests' fp32 bars) on the
device's own ε; the mean head 1e-6 from the fused q (two fp32 summation orders of one
dot product).  The weight gradients are bit-identical over three runs and between the
whole unroll and the ranges (0,1), (1,3), (3,4) cut to T.  Precondition, from the
restatement alone: the noisy q is >= 1e-2 normwise away from the mean-head q
(measured 3.0 - 4.4 at these seeds).

Measured on an MI355X: every ε element bit-equal to numpy; forward 0.9 - 1.3e-7, the
mean head 1.6 - 4.0e-7 from the fused q; gh_out 4e-8, weight gradients 0.2 - 1.4e-7.
"""
import numpy as np
import pytest
import torch

from tests import noisy_model as nm
from tests.gpu_util import normwise, require_gpu

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 4, 32, 5), (9, 8, 1, 32, 5), (2, 3, 3, 16, 5), (4, 16, 3, 64, 16)]
IDS = ["rows15-E32", "rows72-E32", "rows6-E16", "rows64-E64-NA16"]
NET = {32: dict(heads=3, depth=2), 16: dict(heads=2, depth=1), 64: dict(heads=4, depth=2)}
SEED, COUNTER = 5, 3


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    monkeypatch.setenv("T2O_GENERIC", "0")


_CASES = {}


def _case(B, A, T, E, NA):
    """Computed once per shape and left unchanged: the module's fused (q, h) over T + 1
    steps, the head's parameters, the device ε and everything as fp64 CPU copies."""
    key = (B, A, T, E, NA)
    if key in _CASES:
        return _CASES[key]
    from t2omca_amd import ops
    from t2omca_amd.modules import TransformerAgent
    from t2omca_amd.synthetic import make_args
    torch.manual_seed(0)
    agent = TransformerAgent(None, make_args(A, emb=E, n_actions=NA, **NET[E])).cuda()
    flat = torch.cat([p.detach().reshape(-1) for p in agent.parameters()])
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(B, T + 1, A, 9 * A, generator=g).cuda()
    q_f, h = ops.agent_unroll_fwd(agent.shape, ops.pack_params(agent.shape, flat), obs)
    u_w = flat[-NA * (E + 1):-NA].view(NA, E).contiguous()
    u_b = flat[-NA:].contiguous()
    s_w = (0.3 * torch.randn(NA, E, generator=g)).cuda()
    s_b = (0.3 * torch.randn(NA, generator=g)).cuda()
    eps = ops.noise_normal(E, NA, T + 1, SEED, "learner_online", COUNTER, device="cuda")
    act = torch.randint(0, NA, (B, T + 1, A), generator=g).cuda()
    gch = torch.randn(B, T, A, generator=g).cuda()
    gh_in = torch.randn(B, T, A, E, generator=g).cuda()
    torch.cuda.synchronize()
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    c = dict(q_f=q_f, h=h, u_w=u_w, u_b=u_b, s_w=s_w, s_b=s_b, eps=eps, act=act, gch=gch, gh_in=gh_in,
             cpu={k: d(v) for k, v in dict(h=h, u_w=u_w, u_b=u_b, s_w=s_w, s_b=s_b, eps_w=eps[0], eps_b=eps[1],
                                           gch=gch, gh_in=gh_in).items()})
    _CASES[key] = c
    return c


def _ulp_ok(dev, ref):
    dev, ref = np.asarray(dev, np.float32), np.asarray(ref, np.float32)
    return np.abs(dev.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)


@pytest.mark.parametrize("B,A,T,E,NA", SHAPES, ids=IDS)
def test_noise_matches_numpy(B, A, T, E, NA):
    require_gpu()
    from t2omca_amd import ops
    c = _case(B, A, T, E, NA)
    ref_w, ref_b = nm.noise_normal(E, NA, T + 1, SEED, "learner_online", COUNTER)
    dev_w, dev_b = c["eps"][0].cpu().numpy(), c["eps"][1].cpu().numpy()
    ok_w, ok_b = _ulp_ok(dev_w, ref_w), _ulp_ok(dev_b, ref_b)
    exact = float((dev_w == ref_w).mean())
    print(f"E{E} NA{NA}: {exact:.4f} of eps_w bit-equal to numpy, the rest within 1 ulp: {bool(ok_w.all())}")
    assert ok_w.all() and ok_b.all()
    assert exact > 0.9
    # the other kinds and counters are other streams, and a step range writes only its rows
    for kind, counter in (("learner_target", COUNTER), ("runner", COUNTER), ("module", COUNTER),
                          ("learner_online", COUNTER + 1)):
        w, b = ops.noise_normal(E, NA, T + 1, SEED, kind, counter, device="cuda")
        rw, rb = nm.noise_normal(E, NA, T + 1, SEED, kind, counter)
        assert _ulp_ok(w.cpu().numpy(), rw).all() and _ulp_ok(b.cpu().numpy(), rb).all()
        assert not torch.equal(w, c["eps"][0])
    out = (torch.full((T + 1, NA, E), 7.0, device="cuda"), torch.full((T + 1, NA), 7.0, device="cuda"))
    ops.noise_normal(E, NA, T + 1, SEED, "learner_online", COUNTER, out=out, steps=(T, T + 1))
    assert bool((out[0][:T] == 7.0).all()) and bool((out[1][:T] == 7.0).all())
    assert torch.equal(out[0][T], c["eps"][0][T]) and torch.equal(out[1][T], c["eps"][1][T])


@pytest.mark.parametrize("B,A,T,E,NA", SHAPES, ids=IDS)
def test_forward(B, A, T, E, NA):
    require_gpu()
    from t2omca_amd import ops
    c, cpu = _case(B, A, T, E, NA), _case(B, A, T, E, NA)["cpu"]
    want = nm.noisy_head(cpu["h"], cpu["u_w"], cpu["u_b"], cpu["s_w"], cpu["s_b"], cpu["eps_w"], cpu["eps_b"])
    mean = nm.noisy_head(cpu["h"], cpu["u_w"], cpu["u_b"], cpu["s_w"], cpu["s_b"])
    away = normwise(want, mean)
    print(f"precondition: noisy q vs mean-head q {away:.2e} normwise")
    assert away >= 1e-2, away
    q = torch.full_like(c["q_f"], float("nan"))
    ops.noisy_head_fwd(c["h"], q, c["u_w"], c["u_b"], c["s_w"], c["s_b"], eps=c["eps"])
    err = normwise(q, want)
    # in step ranges, into the same buffer: the same bits
    q2 = torch.full_like(q, float("nan"))
    for t0, t1 in ((0, 1), (1, T + 1)):
        ops.noisy_head_fwd(c["h"], q2, c["u_w"], c["u_b"], c["s_w"], c["s_b"], eps=c["eps"], steps=(t0, t1))
    # the mean head against the fused kernel's own q
    qm = torch.full_like(q, float("nan"))
    ops.noisy_head_fwd(c["h"], qm, c["u_w"], c["u_b"])
    err_mean, err_fused = normwise(qm, mean), normwise(qm, c["q_f"])
    print(f"forward {err:.2e}; mean head vs restatement {err_mean:.2e}, vs the fused q {err_fused:.2e}")
    assert err < 1e-5, err
    assert torch.equal(q, q2)
    assert err_mean < 1e-5 and err_fused < 1e-6, (err_mean, err_fused)


def _backward(c, T, ranges, gh_in=True, eps=True):
    from t2omca_amd import ops
    NA, E = c["u_w"].shape
    B, _, A = c["gch"].shape
    gh = gpart = None
    for lo, hi in ranges:
        gh, gpart = ops.noisy_head_bwd(c["gch"], c["act"], c["h"], c["u_w"], c["s_w"] if eps else None,
                                       c["eps"][0] if eps else None, gh_in=c["gh_in"] if gh_in else None, gh_out=gh,
                                       gpart=gpart, steps=(lo, hi))
    g = [torch.zeros(NA, E, device="cuda"), torch.zeros(NA, device="cuda"), torch.zeros(NA, E, device="cuda"),
         torch.zeros(NA, device="cuda")]
    if eps:
        ops.noisy_head_wgrad(gpart, B, A, *g, eps=c["eps"])
    else:
        ops.noisy_head_wgrad(gpart, B, A, g[0], g[1])
    torch.cuda.synchronize()
    return gh, g


@pytest.mark.parametrize("B,A,T,E,NA", SHAPES, ids=IDS)
def test_backward(B, A, T, E, NA):
    require_gpu()
    c, cpu = _case(B, A, T, E, NA), _case(B, A, T, E, NA)["cpu"]
    act = c["act"].cpu()[:, :T]
    want = nm.noisy_head_grads(cpu["h"][:, :T], cpu["u_w"], cpu["s_w"], cpu["eps_w"], cpu["eps_b"], cpu["gch"], act,
                               cpu["gh_in"])
    gh, g = _backward(c, T, [(0, T)])
    errs = [normwise(gh, want[0])] + [normwise(a, b) for a, b in zip(g, want[1:])]
    print("gh_out, du_w, du_b, ds_w, ds_b:", " ".join(f"{e:.2e}" for e in errs))
    assert errs[0] < 1e-5, errs
    assert max(errs[1:]) < 3e-5, errs
    # run to run, and whatever step ranges the backward ran in (from the last down, as the
    # pipelined learner issues them): the same bits
    for _ in range(2):
        gh2, g2 = _backward(c, T, [(0, T)])
        assert torch.equal(gh, gh2) and all(torch.equal(a, b) for a, b in zip(g, g2))
    ranges = [(lo, min(hi, T)) for lo, hi in ((0, 1), (1, 3), (3, 4)) if lo < T]
    gh3, g3 = _backward(c, T, list(reversed(ranges)))
    assert torch.equal(gh, gh3) and all(torch.equal(a, b) for a, b in zip(g, g3))
    # += into the caller's slots
    from t2omca_amd import ops
    _, gpart = ops.noisy_head_bwd(c["gch"], c["act"], c["h"], c["u_w"], c["s_w"], c["eps"][0])
    acc = [x.clone() for x in g]
    ops.noisy_head_wgrad(gpart, B, A, *acc, eps=c["eps"])
    assert all(torch.equal(a, 2 * b) for a, b in zip(acc, g))
    # without gh_in, and the mean head (eps NULL: W_t = u_w, no sigma gradient)
    gh4, _ = _backward(c, T, [(0, T)], gh_in=False)
    assert normwise(gh4, want[0] - cpu["gh_in"]) < 1e-5
    zero = torch.zeros_like(cpu["eps_w"]), torch.zeros_like(cpu["eps_b"])
    want0 = nm.noisy_head_grads(cpu["h"][:, :T], cpu["u_w"], cpu["s_w"], zero[0], zero[1], cpu["gch"], act,
                                cpu["gh_in"])
    gh5, g5 = _backward(c, T, [(0, T)], eps=False)
    assert normwise(gh5, want0[0]) < 1e-5 and normwise(g5[0], want0[1]) < 3e-5 and normwise(g5[1], want0[2]) < 3e-5
    assert not g5[2].any() and not g5[3].any()


def test_actions_with_strides_and_unaligned_rows():
    """Actions read through their strides (a [T+1, B, A] buffer viewed [B, T+1, A], as the
    runner's batches are), and E = 30 (rows that are no multiple of 16 bytes: the scalar
    load path)."""
    require_gpu()
    from t2omca_amd import ops
    B, A, T, E, NA = 3, 5, 4, 30, 5
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
    h, u_w, u_b, s_w, s_b = r(B, T + 1, A, E), r(NA, E), r(NA), 0.3 * r(NA, E), 0.3 * r(NA)
    gch, gh_in = r(B, T, A), r(B, T, A, E)
    act = torch.randint(0, NA, (T + 1, B, A), generator=g).cuda().transpose(0, 1)
    assert not act.is_contiguous()
    eps = ops.noise_normal(E, NA, T + 1, 1, "runner", 0, device="cuda")
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    q = torch.empty(B, T + 1, A, NA, device="cuda")
    ops.noisy_head_fwd(h, q, u_w, u_b, s_w, s_b, eps=eps)
    assert normwise(q, nm.noisy_head(d(h), d(u_w), d(u_b), d(s_w), d(s_b), d(eps[0]), d(eps[1]))) < 1e-5
    gh, gpart = ops.noisy_head_bwd(gch, act, h, u_w, s_w, eps[0], gh_in=gh_in)
    gr = [torch.zeros(NA, E, device="cuda"), torch.zeros(NA, device="cuda"), torch.zeros(NA, E, device="cuda"),
          torch.zeros(NA, device="cuda")]
    ops.noisy_head_wgrad(gpart, B, A, *gr, eps=eps)
    want = nm.noisy_head_grads(d(h)[:, :T], d(u_w), d(s_w), d(eps[0]), d(eps[1]), d(gch), act.cpu()[:, :T], d(gh_in))
    assert normwise(gh, want[0]) < 1e-5
    assert max(normwise(a, b) for a, b in zip(gr, want[1:])) < 3e-5


def test_many_rows_use_row_parts():
    """B·A = 2304 rows: three row parts per step in the backward, 64 workgroups striding
    the rows in the forward."""
    require_gpu()
    from t2omca_amd import ops
    B, A, T, E, NA = 288, 8, 2, 32, 5
    assert ops.noisy_head_parts(B, A) == 3
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
    h, u_w, u_b, s_w, s_b = r(B, T, A, E), r(NA, E), r(NA), 0.3 * r(NA, E), 0.3 * r(NA)
    gch = r(B, T, A)
    act = torch.randint(0, NA, (B, T, A), generator=g).cuda()
    eps = ops.noise_normal(E, NA, T, 2, "learner_online", 1, device="cuda")
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    q = torch.empty(B, T, A, NA, device="cuda")
    ops.noisy_head_fwd(h, q, u_w, u_b, s_w, s_b, eps=eps)
    assert normwise(q, nm.noisy_head(d(h), d(u_w), d(u_b), d(s_w), d(s_b), d(eps[0]), d(eps[1]))) < 1e-5
    runs = []
    for _ in range(2):
        gh, gpart = ops.noisy_head_bwd(gch, act, h, u_w, s_w, eps[0])
        gr = [torch.zeros(NA, E, device="cuda"), torch.zeros(NA, device="cuda"), torch.zeros(NA, E, device="cuda"),
              torch.zeros(NA, device="cuda")]
        ops.noisy_head_wgrad(gpart, B, A, *gr, eps=eps)
        runs.append([gh] + gr)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    want = nm.noisy_head_grads(d(h), d(u_w), d(s_w), d(eps[0]), d(eps[1]), d(gch), act.cpu())
    assert normwise(runs[0][0], want[0]) < 1e-5
    assert max(normwise(a, b) for a, b in zip(runs[0][1:], want[1:])) < 3e-5


def test_module_training_forward_and_autograd():
    """modules.TransformerAgent with action_selector "noisy-new": eval mode is the plain
    agent's fused step bit for bit and draws nothing; a training-mode forward draws kind
    "module" noise at its call counter, its q is the restated head on its own h, and
    autograd reaches u_w, u_b, s_w, s_b (and h: the transformer's parameters)."""
    require_gpu()
    import types
    from t2omca_amd.modules import TransformerAgent
    from t2omca_amd.synthetic import make_args
    A, b, E, NA = 8, 3, 32, 5
    args = make_args(A)
    torch.manual_seed(0)
    noisy = TransformerAgent(None, types.SimpleNamespace(**{**vars(args), "action_selector": "noisy-new",
                                                            "noise_seed": 4})).cuda()
    torch.manual_seed(0)
    plain = TransformerAgent(None, args).cuda()
    with torch.no_grad():
        noisy.q_basic.s_w.copy_(0.3 * torch.randn(NA, E))
        noisy.q_basic.s_b.copy_(0.3 * torch.randn(NA))
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(b, A, 9 * A, generator=g).cuda()
    h0 = torch.randn(b, A, E, generator=g).cuda()
    noisy.eval()
    q_e, h_e = noisy(obs, h0)
    q_p, h_p = plain(obs, h0)
    assert torch.equal(q_e, q_p) and torch.equal(h_e, h_p) and noisy.noise_calls == 0
    noisy.train()
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    nl = noisy.q_basic
    qs = []
    for call in range(2):
        q, h = noisy(obs, h0)
        assert noisy.noise_calls == call + 1 and torch.equal(h, h_e)
        ew, eb = (torch.from_numpy(x).double() for x in nm.noise_normal(E, NA, 1, 4, "module", call))
        want = nm.noisy_head(d(h).unsqueeze(1), d(nl.u_w), d(nl.u_b), d(nl.s_w), d(nl.s_b), ew, eb)[:, 0]
        assert normwise(q, want) < 1e-5
        qs.append(q)
    assert normwise(qs[1], qs[0]) > 1e-2  # fresh noise every call
    G = torch.randn(b, A, NA, generator=g).cuda()
    noisy.zero_grad()
    (q * G).sum().backward()
    leaves = [d(p).requires_grad_(True) for p in (nl.u_w, nl.u_b, nl.s_w, nl.s_b)]
    hh = d(h).unsqueeze(1).requires_grad_(True)
    (nm.noisy_head(hh, *leaves, ew, eb)[:, 0] * d(G)).sum().backward()
    for p, ref in zip((nl.u_w, nl.u_b, nl.s_w, nl.s_b), leaves):
        assert normwise(p.grad, ref.grad) < 3e-5
    # dL/dh reached the fused BPTT: the plain agent given that dL/dh gets the same
    # transformer gradients
    plain.zero_grad()
    _, h_pl = plain(obs, h0)
    (h_pl * hh.grad[:, 0].float().cuda()).sum().backward()
    for (n1, p1), (_, p2) in zip(list(noisy.named_parameters())[:-4], list(plain.named_parameters())[:-2]):
        assert normwise(p1.grad, p2.grad) < 3e-5, n1
