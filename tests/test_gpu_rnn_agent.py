"""GPU: the GRU agent's kernels alone (csrc/t2o_rnn.hip) against the fp64 restatement
(tests/rnn_model.py) and autograd on it.

Inputs: seeded N(0, 1) observations, uniform actions, h0 ~ 0.5 N(0, 1) where given;
the two networks are drawn with torch.manual_seed(SEED = 0) through modules.make_agent.
Bars are the project's fp32 bars (test_gpu_learner_masks.TOL["fp32"]): forward 1e-5
normwise, every parameter tensor's gradient and dL/dh0 3e-5 normwise per tensor.  A
tensor is excused only under grad_blocks.FIT_SHARE (its reference gradient carries
less than that share of the whole), at most one per case: with seed 0 the fp64 model
alone excuses exactly one tensor in the whole grid, rnn.weight_hh wherever T = 1 and
h0 is zero (its gradient Σ dghᵀ h_{t-1} is then identically zero), checked on the CPU
by test_reference_is_fit below.

Shapes (A, B, T1): one row; 15 rows (a partial tile); 16 rows (a whole tile); 17
sequences (a second, partial tile); 16 agents; 64 agents.  Input kinds: the flat
observation (6 wide) with both one-hots (IN = 14 at 3 agents: no multiple of 4), the
entity observation (9·A wide) without and with them.  The backward runs over
T = T1 - 1 steps of the T1-step forward where T1 >= 3 (the learner's form), else over
all of them.

MEASURED on an MI355X over the whole grid (every test prints its own figures):
  forward  q, h of either network   worst 6.7e-7  ((64, 2, 3), H = 64, entity obs without one-hots, no h0)
  backward per tensor and dL/dh0    worst 1.3e-6  (dL/dh0 at (1, 17, 2), H = 64, entity obs without one-hots, with gh)
  the worst tensor is dL/dh0 in most cases, else rnn.weight_hh or rnn.weight_ih at <= 7.4e-7.
Two runs of the forward and of the backward, the one-network call against the two-network
call, and the split step ranges are bit-equal everywhere.
"""
import functools
import types

import pytest
import torch

from tests import rnn_model
from tests.arena import Arena
from tests.gpu_util import normwise, require_gpu
from tests.grad_blocks import FIT_SHARE

pytestmark = pytest.mark.gpu

FWD_BAR, GRAD_BAR = 1e-5, 3e-5
SEED = 0
SHAPES = [(1, 1, 1), (3, 5, 5), (8, 2, 3), (1, 17, 2), (16, 3, 5), (64, 2, 3)]
KINDS = ["flat_both", "entity_none", "entity_both"]
NA = 5  # the action count of every case that does not name one
# (A, B, T1, NA): the narrowest one-hot and head (two actions) and the widest the kernels take (16)
NA_SHAPES = [(3, 5, 5, 2), (8, 2, 3, 16)]


def agent_args(A, H=64, kind="flat_both", na=NA, **kw):
    both = kind.endswith("both")
    return types.SimpleNamespace(n_agents=A, n_actions=na, rnn_hidden_dim=H, obs_last_action=both, obs_agent_id=both,
                                 agent="rnn", device="cpu", **kw)


def obs_width(A, kind):
    return 6 if kind.startswith("flat") else 9 * A


def input_width(A, kind, na=NA):
    return obs_width(A, kind) + ((na + A) if kind.endswith("both") else 0)


def bwd_steps(T1):
    return T1 - 1 if T1 >= 3 else T1


@functools.lru_cache(maxsize=None)
def case(A, B, T1, H, kind, with_h0, na=NA):
    """Two networks, inputs and the fp64 reference (forward of both, gradients of the
    online one), computed once.  With na != 5 the actions 0 and na - 1 both occur."""
    from t2omca_amd.modules import make_agent
    torch.manual_seed(SEED)
    on = make_agent(input_width(A, kind, na), agent_args(A, H, kind, na))
    tg = make_agent(input_width(A, kind, na), agent_args(A, H, kind, na))
    g = torch.Generator().manual_seed(7 + A + 3 * B + 5 * T1)
    obs = torch.randn(B, T1 + 1, A, obs_width(A, kind), generator=g)[:, :T1]  # (a strided view's parent)
    actions = torch.randint(0, na, (B, T1, A), generator=g)
    assert na == NA or (int(actions.min()) == 0 and int(actions.max()) == na - 1)
    h0 = 0.5 * torch.randn(B, A, H, generator=g) if with_h0 else None
    T = bwd_steps(T1)
    gch = torch.randn(B, T, A, generator=g)
    zeroed = torch.rand(B, T, generator=g) < 0.3  # steps a mask would zero (never the first episode's first)
    zeroed[0, 0] = False
    gch[zeroed] = 0.0
    use_gh = (A + B + T1 + H // 32 + int(with_h0)) % 2 == 0
    gh = torch.randn(B, T, A, H, generator=g) if use_gh else None
    p_on, p_tg = rnn_model.param_dict(on), rnn_model.param_dict(tg)
    pg = {k: v.clone().requires_grad_(True) for k, v in p_on.items()}
    both = kind.endswith("both")
    inputs = rnn_model.build_inputs(obs.double(), actions, na, both, both)
    h0d = (h0.double() if with_h0 else torch.zeros(B, A, H, dtype=torch.float64)).requires_grad_(True)
    q_on, h_on = rnn_model.unroll(pg, inputs, h0d)
    q_tg, h_tg = rnn_model.unroll(p_tg, inputs, h0d.detach())
    loss = (torch.gather(q_on[:, :T], 3, actions[:, :T].unsqueeze(3)).squeeze(3) * gch.double()).sum()
    if use_gh:
        loss = loss + (h_on[:, :T] * gh.double()).sum()
    grads = torch.autograd.grad(loss, list(pg.values()) + [h0d])
    flat = lambda m: torch.cat([p.detach().reshape(-1) for p in m.parameters()])  # noqa: E731
    return dict(shape=on.shape, flat_on=flat(on), flat_tg=flat(tg), obs=obs, actions=actions, h0=h0, gch=gch, gh=gh,
                q_on=q_on.detach(), h_on=h_on.detach(), q_tg=q_tg, h_tg=h_tg, gp=dict(zip(pg, grads[:-1])),
                gh0=grads[-1], on=on, T=T, na=na)


def excused(c):
    """The tensors grad_blocks.FIT_SHARE excuses: less than that share of the whole gradient."""
    gmax = max(float(g.abs().max()) for g in c["gp"].values())
    assert gmax > 0
    return [k for k, g in c["gp"].items() if float(g.abs().max()) < FIT_SHARE * gmax]


def to_dev(c):
    d = {k: c[k].cuda() for k in ("flat_on", "flat_tg", "actions", "gch")}
    d["obs"] = c["obs"].cuda()
    d["h0"] = None if c["h0"] is None else c["h0"].cuda()
    d["gh"] = None if c["gh"] is None else c["gh"].cuda()
    return d


def forward(c, d, two=True, **kw):
    from t2omca_amd import ops
    return ops.rnn_agent_fwd(c["shape"], d["flat_on"], d["obs"], actions=d["actions"], h0_on=d["h0"],
                             params_tg=d["flat_tg"] if two else None, h0_tg=d["h0"] if two else None, **kw)


def backward(c, d, fwd, **kw):
    from t2omca_amd import ops
    slabs, nslab, gh0 = ops.rnn_agent_bwd(c["shape"], d["flat_on"], d["obs"], fwd, T=c["T"], actions=d["actions"],
                                          gchosen=d["gch"], gh=d["gh"], h0=d["h0"], want_gh0=True, **kw)
    return ops.reduce_slabs(slabs, nslab, torch.empty_like(d["flat_on"])), gh0, nslab


GRID = [(A, B, T1, H, kind) for (A, B, T1) in SHAPES for H in (32, 64) for kind in KINDS]


@pytest.mark.parametrize("A,B,T1,H,kind", GRID)
def test_reference_is_fit(A, B, T1, H, kind):
    """(No device: the fp64 model alone.)  At most one tensor per case is excused."""
    for with_h0 in (False, True):
        ex = excused(case(A, B, T1, H, kind, with_h0))
        assert len(ex) <= 1, ex
        assert ex in ([], ["rnn.weight_hh"]) and (not ex or (T1 == 1 and not with_h0)), ex


@pytest.mark.parametrize("A,B,T1,na", NA_SHAPES)
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("kind", ["flat_both", "entity_both"])
def test_reference_is_fit_action_counts(A, B, T1, na, H, kind):
    """(No device.)  The fp64 model at 2 and 16 actions excuses no tensor."""
    for with_h0 in (False, True):
        assert excused(case(A, B, T1, H, kind, with_h0, na)) == []


@pytest.mark.parametrize("A,B,T1,H,kind", GRID)
def test_forward_backward(A, B, T1, H, kind):
    forward_backward(A, B, T1, H, kind)


@pytest.mark.parametrize("A,B,T1,na", NA_SHAPES)
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("kind", ["flat_both", "entity_both"])
def test_forward_backward_action_counts(A, B, T1, na, H, kind):
    """The last-action one-hot the kernels build inside their input rows (width NA, at columns
    OBS .. OBS + NA) and the Q head (NA rows of fc2) at two actions and at 16, the most the
    kernels take; IN = 6 + 2 + 3 = 11 (flat, 3 agents) is no multiple of 4.  MEASURED on an
    MI355X over these eight cases: forward <= 3.7e-7, backward per tensor and dL/dh0 <= 1.0e-6."""
    forward_backward(A, B, T1, H, kind, na)


def forward_backward(A, B, T1, H, kind, na=NA):
    require_gpu()
    from t2omca_amd import ops
    worst = {}
    for with_h0 in (False, True):
        c = case(A, B, T1, H, kind, with_h0, na)
        d = to_dev(c)
        f = forward(c, d)
        errs = {k: normwise(f[k], c[k]) for k in ("q_on", "h_on", "q_tg", "h_tg")}
        print(f"rnn fwd {(A, B, T1, H, kind, with_h0)}: {errs}")
        assert max(errs.values()) <= FWD_BAR, errs
        # one network alone, and a second run: bit-equal
        f1 = forward(c, d, two=False)
        f2 = forward(c, d)
        assert all(torch.equal(f1[k], f[k]) for k in ("q_on", "h_on", "gi_on", "x_on"))
        assert all(torch.equal(f2[k], f[k]) for k in f)
        gflat, gh0, nslab = backward(c, d, f)
        assert nslab == ops.rnn_slab_count(B, c["T"], A)
        ex = excused(c)
        assert len(ex) <= 1, ex
        gerr, off = {}, 0
        for name, shp in ops.rnn_param_blocks(c["shape"].IN, H, na):
            ref = c["gp"][name]
            assert tuple(ref.shape) == tuple(shp)
            got = gflat[off:off + ref.numel()].view(shp)
            off += ref.numel()
            assert bool(torch.isfinite(got).all()), name
            if name in ex:
                assert float(got.abs().max()) <= FIT_SHARE * max(float(g.abs().max()) for g in c["gp"].values()), name
                continue
            gerr[name] = normwise(got, ref)
        assert off == gflat.numel() == c["shape"].n_params
        gerr["h0"] = normwise(gh0, c["gh0"])
        print(f"rnn bwd {(A, B, T1, H, kind, with_h0)} gh={c['gh'] is not None}: worst "
              f"{max(gerr.items(), key=lambda kv: kv[1])}")
        assert max(gerr.values()) <= GRAD_BAR, gerr
        gflat2, gh02, _ = backward(c, d, f)
        assert torch.equal(gflat2, gflat) and torch.equal(gh02, gh0)
        worst[with_h0] = (max(errs.values()), max(gerr.values()))
    print(f"rnn worst {(A, B, T1, H, kind)}: {worst}")


@pytest.mark.parametrize("A,B,T1,H,kind", [(3, 5, 5, 64, "flat_both"), (16, 3, 5, 32, "entity_both"),
                                           (8, 2, 3, 64, "entity_none")])
@pytest.mark.parametrize("with_h0", [False, True])
def test_step_ranges(A, B, T1, H, kind, with_h0):
    """[0, T1) in one call == [0, k) then [k, T1) from the carried h, bit for bit."""
    require_gpu()
    c = case(A, B, T1, H, kind, with_h0)
    d = to_dev(c)
    from t2omca_amd import ops
    whole = forward(c, d)
    for k in range(1, T1):
        outs = {n: torch.full_like(v, float("nan")) for n, v in whole.items()}
        forward(c, d, steps=(0, k), outs=outs)
        ops.rnn_agent_fwd(c["shape"], d["flat_on"], d["obs"], actions=d["actions"], h0_on=outs["h_on"][:, k - 1],
                          params_tg=d["flat_tg"], h0_tg=outs["h_tg"][:, k - 1], steps=(k, T1), outs=outs)
        for n in whole:
            assert torch.equal(outs[n], whole[n]), (k, n)


@pytest.mark.parametrize("A,B,T1", [(3, 5, 1), (8, 2, 1), (17, 1, 1), (3, 5, 3), (1, 17, 2)])
def test_memory_contract(A, B, T1):
    """15, 16 and 17 rows (and sequences): observations, actions and h0 as strided views
    carved from a poisoned arena (parameters, outputs and workspaces dense, as the header
    states): finite outputs, bit-equal to a run on dense tensors, nothing written outside
    them, and every element of the outputs and of the work buffer written."""
    require_gpu()
    from t2omca_amd import ops
    H, kind = 64, "flat_both"
    c = case(A, B, T1, H, kind, True)
    sh, T, OBS = c["shape"], c["T"], obs_width(A, kind)
    d = to_dev(c)
    dense = dict(d, obs=d["obs"].contiguous())
    f_ref = forward(c, dense)
    g_ref, gh0_ref, nslab = backward(c, dense, f_ref)
    ar = Arena(16 << 20, "cuda")
    t = dict(d)
    pad = 2
    t["obs"] = ar.place(dense["obs"], ((T1 + pad) * A * OBS + 4, A * OBS, OBS, 1), name="obs", stride_multiple=1)
    t["actions"] = ar.place(d["actions"], ((T1 + pad) * (A + 1), A + 1, 1), name="actions")
    t["h0"] = ar.place(d["h0"], (A * H + 8, H, 1), name="h0")
    for k in ("flat_on", "flat_tg", "gch"):
        t[k] = ar.place(d[k], name=k)
    if d["gh"] is not None:
        t["gh"] = ar.place(d["gh"], name="gh")
    outs = {k: ar.carve((B, T1, A, w), name=k) for k, w in (("q_on", NA), ("h_on", H), ("gi_on", 3 * H), ("x_on", H),
                                                            ("q_tg", NA), ("h_tg", H), ("gi_tg", 3 * H))}
    f = forward(c, t, outs=outs)
    slabs = ar.carve((nslab * sh.n_params,), name="slabs")
    work = ar.carve((ops.rnn_work_floats(sh, B, T),), name="work")
    gh0 = ar.carve((B, A, H), name="gh0")
    g, gh0, _ = backward(c, t, f, slabs=slabs, work=work, gh0=gh0)
    torch.cuda.synchronize()
    for k in f_ref:
        assert bool(torch.isfinite(f[k]).all()), k
        assert torch.equal(f[k], f_ref[k]), k
    assert bool(torch.isfinite(slabs).all()) and bool(torch.isfinite(work).all())
    assert torch.equal(g, g_ref) and torch.equal(gh0, gh0_ref)
    ar.check("rnn kernels")


@pytest.mark.parametrize("A,B,H,kind", [(3, 5, 64, "flat_both"), (8, 2, 32, "entity_both")])
def test_module_autograd(A, B, H, kind):
    """RNNAgent.forward and loss.backward() against torch's own Linear / GRUCell / Linear
    carrying the same parameters."""
    require_gpu()
    c = case(A, B, 1, H, kind, True)
    m = c["on"]
    IN = input_width(A, kind)
    ref = torch.nn.ModuleDict(dict(fc1=torch.nn.Linear(IN, H), rnn=torch.nn.GRUCell(H, H), fc2=torch.nn.Linear(H, NA)))
    ref.load_state_dict(m.state_dict())
    ref = ref.double()
    g = torch.Generator().manual_seed(3)
    inputs = torch.randn(B, A, IN, generator=g)
    hid = (0.5 * torch.randn(B, A, H, generator=g)).requires_grad_(True)
    wq, wh = torch.randn(B, A, NA, generator=g), torch.randn(B, A, H, generator=g)
    hd = hid.detach().double().requires_grad_(True)
    hr = ref["rnn"](torch.relu(ref["fc1"](inputs.double().view(-1, IN))), hd.view(-1, H))
    qr = ref["fc2"](hr)
    ((qr.view(B, A, NA) * wq.double()).sum() + (hr.view(B, A, H) * wh.double()).sum()).backward()
    m.cuda()
    try:
        hc = hid.detach().cuda().requires_grad_(True)
        q, h = m(inputs.cuda(), hc)
        assert q.shape == (B, A, NA) and h.shape == (B, A, H)
        ((q * wq.cuda()).sum() + (h * wh.cuda()).sum()).backward()
        assert normwise(q, qr.view(B, A, NA)) <= FWD_BAR and normwise(h, hr.view(B, A, H)) <= FWD_BAR
        assert normwise(hc.grad, hd.grad) <= GRAD_BAR
        for (name, p), pr in zip(m.named_parameters(), ref.parameters()):
            assert normwise(p.grad, pr.grad) <= GRAD_BAR, name
        # the step without a carried state: init_hidden's zeros, expanded
        m.args.device = "cuda"
        q0, _ = m(inputs.cuda(), m.init_hidden())
        hz = ref["rnn"](torch.relu(ref["fc1"](inputs.double().view(-1, IN))), torch.zeros(B * A, H, dtype=torch.float64))
        assert normwise(q0, ref["fc2"](hz).view(B, A, NA)) <= FWD_BAR
    finally:
        m.cpu()
        m.args.device = "cpu"
        m.zero_grad()
