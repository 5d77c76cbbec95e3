"""CPU: the restatement of the QPLEX mixer (tests/qplex_model.py) checked against itself
(y_adv = 0 at q = m, ∂y/∂q = w, the stop-gradient, λ > 0) and against a plain nn.Module
written as PyMARL2's dmaq_general.py / dmaq_si_weight.py read, and the module's
parameter tree, limits and dispatch (t2omca_amd.modules, learner._mixer_kind_of)."""
import types

import pytest
import torch
import torch.nn as nn

from tests import qplex_model

COUNTS = {3: 28450, 8: 73940, 16: 146724, 64: 583428}


class PlainSIWeight(nn.Module):
    """dmaq_si_weight.DMAQ_SI_Weight at adv_hypernet_layers 2, as it reads."""

    def __init__(self, A, S, NA, HA, K):
        super().__init__()
        self.A, self.K = A, K
        def net(n_in, n_out):
            return nn.Sequential(nn.Linear(n_in, HA), nn.ReLU(), nn.Linear(HA, n_out))
        self.key_extractors = nn.ModuleList([net(S, 1) for _ in range(K)])
        self.agents_extractors = nn.ModuleList([net(S, A) for _ in range(K)])
        self.action_extractors = nn.ModuleList([net(S + A * NA, A) for _ in range(K)])

    def forward(self, states, actions):
        data = torch.cat([states, actions], dim=1)
        heads = []
        for key, ag, ac in zip(self.key_extractors, self.agents_extractors, self.action_extractors):
            x_key = torch.abs(key(states)).repeat(1, self.A) + 1e-10
            heads.append(x_key * torch.sigmoid(ag(states)) * torch.sigmoid(ac(data)))
        return torch.stack(heads, dim=1).sum(dim=1)


class PlainQPlex(nn.Module):
    """dmaq_general.DMAQer with weighted_head and is_minus_one, as it reads."""

    def __init__(self, A, S, NA, H=64, HA=64, K=4):
        super().__init__()
        self.A, self.S, self.NA = A, S, NA
        self.hyper_w_final = nn.Sequential(nn.Linear(S, H), nn.ReLU(), nn.Linear(H, A))
        self.V = nn.Sequential(nn.Linear(S, H), nn.ReLU(), nn.Linear(H, A))
        self.si_weight = PlainSIWeight(A, S, NA, HA, K)

    def forward(self, agent_qs, states, actions=None, max_q_i=None, is_v=False):
        bs = agent_qs.size(0)
        states = states.reshape(-1, self.S)
        agent_qs = agent_qs.reshape(-1, self.A)
        w_final = torch.abs(self.hyper_w_final(states)).view(-1, self.A) + 1e-10
        v = self.V(states).view(-1, self.A)
        agent_qs = w_final * agent_qs + v
        if is_v:
            return torch.sum(agent_qs, dim=-1).view(bs, -1, 1)
        max_q_i = w_final * max_q_i.reshape(-1, self.A) + v
        adv_q = (agent_qs - max_q_i).detach()
        adv_w = self.si_weight(states, actions.reshape(-1, self.A * self.NA))
        return torch.sum(adv_q * (adv_w - 1.0), dim=1).view(bs, -1, 1)


def _args(A, **kw):
    from t2omca_amd.synthetic import make_args
    return types.SimpleNamespace(**{**vars(make_args(A, device="cpu", mixer="dmaq")), **kw})


def _draw(A, S, NA, b=3, T=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    q, m = torch.randn(b, T, A, generator=g).double(), torch.randn(b, T, A, generator=g).double()
    u = torch.randint(0, NA, (b, T, A), generator=g)
    s = torch.randn(b, T, S, generator=g).double()
    return q, m, u, s


@pytest.mark.parametrize("A,NA,H,HA,K", [(1, 5, 64, 64, 4), (3, 5, 64, 64, 4), (8, 5, 64, 64, 4), (5, 16, 32, 64, 1)])
def test_restatement_equals_the_plain_module(A, NA, H, HA, K):
    torch.manual_seed(0)
    S = 8 * A + 2
    net = PlainQPlex(A, S, NA, H, HA, K).double()
    q, m, u, s = _draw(A, S, NA)
    p = qplex_model.param_dict(net)
    assert list(p) == qplex_model.keys(K) and {k: tuple(v.shape) for k, v in p.items()} == \
        qplex_model.shapes(A, S, NA, H, HA, K)
    onehot = torch.nn.functional.one_hot(u, NA).double()
    y_v, y_adv = qplex_model.qplex_parts(p, q, m, u, s, NA)
    for got, ref in ((y_v, net(q, s, is_v=True)[..., 0]), (y_adv, net(q, s, onehot, m)[..., 0])):
        assert float((got - ref).detach().abs().max()) <= 1e-14 * max(1.0, float(ref.detach().abs().max()))
    assert torch.equal(qplex_model.qplex_forward(p, q, m, u, s, NA), y_v + y_adv)


def test_model_against_itself():
    torch.manual_seed(1)
    A, S, NA = 5, 42, 5
    p = {k: torch.randn(sh, dtype=torch.float64).requires_grad_(True) * 0.3 for k, sh in
         qplex_model.shapes(A, S, NA).items()}
    p = {k: v.detach().requires_grad_(True) for k, v in p.items()}
    q, m, u, s = _draw(A, S, NA, seed=2)
    assert bool(((q - m) > 0).any()) and bool(((q - m) < 0).any())  # any sign of q − m
    w, v, lam = qplex_model.weights(p, s, u, NA)
    assert bool((lam > 0).all()) and bool((w > 0).all())
    # y_adv = 0 where q = m
    assert float(qplex_model.qplex_parts(p, q, q.clone(), u, s, NA)[1].detach().abs().max()) == 0.0
    # ∂y/∂q = w, and no gradient reaches m
    q_, m_ = q.clone().requires_grad_(True), m.clone().requires_grad_(True)
    y = qplex_model.qplex_forward(p, q_, m_, u, s, NA)
    gq, gm = torch.autograd.grad(y.sum(), (q_, m_), allow_unused=True)
    assert torch.equal(gq, w.detach()) and (gm is None or not gm.any())
    # the stop-gradient: hyper_w_final's gradient is that of y_v alone; si_weight's that of y_adv alone
    names = list(p)
    g_all = torch.autograd.grad(qplex_model.qplex_forward(p, q, m, u, s, NA).sum(), list(p.values()))
    y_v, y_adv = qplex_model.qplex_parts(p, q, m, u, s, NA)
    g_v = torch.autograd.grad(y_v.sum(), list(p.values()), allow_unused=True)
    g_a = torch.autograd.grad(y_adv.sum(), list(p.values()), allow_unused=True)
    for n, ga, gv, gd in zip(names, g_all, g_v, g_a):
        if n.startswith("si_weight."):
            assert gv is None and torch.equal(ga, gd) and bool(gd.any()), n
        else:
            assert gd is None and torch.equal(ga, gv) and bool(gv.any()), n
    # ... which a port without the detach gets wrong
    y_leak = ((w * (q - m)) * (lam - 1.0)).sum()
    g_leak, = torch.autograd.grad(y_leak, p["hyper_w_final.2.weight"])
    assert bool(g_leak.any())


def test_gradcheck():
    torch.manual_seed(1)
    A, S, NA = 3, 10, 4
    p = {k: (0.3 * torch.randn(sh, dtype=torch.float64)).requires_grad_(True) for k, sh in
         qplex_model.shapes(A, S, NA, 32, 32, 2).items()}
    q, m, u, s = _draw(A, S, NA, b=2, T=2)
    q.requires_grad_(True)
    keys = list(p)

    # gradcheck perturbs what the stop-gradient freezes, so it checks the differentiable factorisation
    # with c = w (q − m) held at this point; the model's own gradients must equal that function's
    c = (qplex_model.weights(p, s, u, NA)[0] * (q - m)).detach()

    def f(q, *vals):
        w, v, lam = qplex_model.weights(dict(zip(keys, vals)), s, u, NA)
        return (w * q + v).sum(2) + (c * (lam - 1.0)).sum(2)
    assert torch.autograd.gradcheck(f, (q, *p.values()), eps=1e-6, atol=1e-6)
    g_f = torch.autograd.grad(f(q, *p.values()).sum(), (q, *p.values()))
    g_m = torch.autograd.grad(qplex_model.qplex_forward(p, q, m, u, s, NA).sum(), (q, *p.values()))
    assert all(torch.equal(a, b) for a, b in zip(g_f, g_m))


def test_modules_build_on_the_cpu():
    from t2omca_amd import ops
    from t2omca_amd.learner import MIXERS, _mixer_kind_of
    from t2omca_amd.modules import QPlexMixer, make_mixer
    torch.manual_seed(0)
    m = make_mixer(_args(8))
    assert type(m) is QPlexMixer and m.kind == "qplex" and m.custom_space is True and "qplex" in MIXERS
    assert type(make_mixer(_args(8, mixer="qplex"))) is QPlexMixer
    sd = m.state_dict()
    assert len(sd) == 56 and list(sd) == qplex_model.keys(4)
    assert [k for k, _ in m.named_parameters()] == qplex_model.keys(4)  # registration order = opt.th order
    assert {k: tuple(v.shape) for k, v in sd.items()} == qplex_model.shapes(8, 64, 5)
    assert [(k, tuple(sh)) for k, sh in ops.qplex_param_blocks(8, 64, 5)] == [(k, tuple(v.shape)) for k, v in sd.items()]
    assert _mixer_kind_of(sd) == "qplex"
    assert m.shape == ops.QplexShape(8, 64, 5, 64, 64, 4)
    # torch's default initialisation: the same draws as the plain module under one seed
    torch.manual_seed(0)
    plain = PlainQPlex(8, 64, 5)
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), plain.state_dict().values()))
    for A, n in COUNTS.items():
        mm = QPlexMixer(_args(A))
        assert sum(p.numel() for p in mm.parameters()) == n == mm.shape.n_params
    small = QPlexMixer(_args(6, hypernet_embed=32, adv_hypernet_embed=64, num_kernel=1, state_shape=(5, 10),
                             n_actions=16))
    assert small.shape == ops.QplexShape(6, 50, 16, 32, 64, 1)
    for A in range(1, 65):  # qplex.yaml's defaults at every AGV count
        assert QPlexMixer(_args(A)).shape.n_params > 0


@pytest.mark.parametrize("kw,limit", [(dict(hypernet_embed=128), "hypernet_embed"),
                                      (dict(adv_hypernet_embed=48), "adv_hypernet_embed"),
                                      (dict(state_shape=2048), "state width"), (dict(n_agents=65), "n_agents"),
                                      (dict(n_actions=17), "n_actions"), (dict(num_kernel=11), "num_kernel"),
                                      (dict(adv_hypernet_layers=1), "adv_hypernet_layers"),
                                      (dict(adv_hypernet_layers=3), "adv_hypernet_layers"),
                                      (dict(weighted_head=False), "weighted_head"),
                                      (dict(is_minus_one=False), "is_minus_one")])
def test_unsupported_settings_fail_at_construction(kw, limit):
    from t2omca_amd.modules import QPlexMixer
    with pytest.raises(ValueError, match=limit):
        QPlexMixer(_args(8, **kw))


def test_other_mixers_dispatch_as_before():
    from t2omca_amd.learner import _mixer_kind_of
    from t2omca_amd.modules import QMixer, TransformerMixer, VDNMixer, make_mixer
    assert type(make_mixer(_args(3, mixer="qmix"))) is QMixer
    assert type(make_mixer(_args(3, mixer="vdn"))) is VDNMixer
    assert type(make_mixer(_args(3, mixer="transformer"))) is TransformerMixer
    assert type(make_mixer(_args(3, mixer="qatten"))) is TransformerMixer
    assert _mixer_kind_of(make_mixer(_args(3, mixer="qmix")).state_dict()) == "qmix"
    assert _mixer_kind_of({}) == "vdn"
    assert _mixer_kind_of(make_mixer(_args(3, mixer="transformer")).state_dict()) == "transformer"


def test_mixer_refuses_cpu_tensors():
    from t2omca_amd.modules import QPlexMixer
    m = QPlexMixer(_args(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 2, 3), torch.zeros(2, 2, 24), is_v=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 2, 3), torch.zeros(2, 2, 24), torch.zeros(2, 2, 3, dtype=torch.int64), torch.zeros(2, 2, 3))
