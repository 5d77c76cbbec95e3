"""CPU: the restatement of the QMIX / VDN mixers (tests/qmix_model.py) against a plain
nn.Module written as the definition reads, its gradients, its
monotonicity, and the modules' parameter trees and dispatch (t2omca_amd.modules)."""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import qmix_model


class PlainQMixer(nn.Module):
    """PyMARL2's nmix.Mixer, as the definition reads."""

    def __init__(self, A, S, M=32, H=64):
        super().__init__()
        self.A, self.M = A, M
        self.hyper_w1 = nn.Sequential(nn.Linear(S, H), nn.ReLU(), nn.Linear(H, A * M))
        self.hyper_b1 = nn.Sequential(nn.Linear(S, M))
        self.hyper_w2 = nn.Sequential(nn.Linear(S, H), nn.ReLU(), nn.Linear(H, M))
        self.hyper_b2 = nn.Sequential(nn.Linear(S, M), nn.ReLU(), nn.Linear(M, 1))

    def forward(self, qvals, states):
        b, T, A = qvals.shape
        s = states.reshape(-1, states.shape[-1])
        q = qvals.reshape(b * T, 1, A)
        w1 = self.hyper_w1(s).abs().view(-1, A, self.M)
        b1 = self.hyper_b1(s).view(-1, 1, self.M)
        w2 = self.hyper_w2(s).abs().view(-1, self.M, 1)
        b2 = self.hyper_b2(s).view(-1, 1, 1)
        hidden = F.elu(torch.matmul(q, w1) + b1)
        return (torch.matmul(hidden, w2) + b2).view(b, T, 1)


def _args(A, **kw):
    from t2omca_amd.synthetic import make_args
    return types.SimpleNamespace(**{**vars(make_args(A, device="cpu")), **kw})


@pytest.mark.parametrize("A,M,H", [(1, 32, 64), (3, 32, 64), (8, 32, 64), (6, 16, 32)])
def test_restatement_equals_the_plain_module(A, M, H):
    torch.manual_seed(0)
    S = 8 * A
    net = PlainQMixer(A, S, M, H).double()
    q, s = torch.randn(3, 4, A, dtype=torch.float64), torch.randn(3, 4, S, dtype=torch.float64)
    ref = net(q, s)[..., 0]
    got = qmix_model.qmix_forward(qmix_model.param_dict(net), q, s)
    assert float((got - ref).detach().abs().max()) <= 1e-15 * max(1.0, float(ref.detach().abs().max()))
    assert list(net.state_dict()) == list(qmix_model.KEYS)


@pytest.mark.parametrize("pos_func,beta", [("abs", 1.0), ("softplus", 0.5), ("quadratic", 1.0), ("identity", 1.0)])
def test_gradcheck(pos_func, beta):
    torch.manual_seed(1)
    A, S = 3, 24
    # (weights of 0.3·N(0, 1): O(1) pre-activations, so that central differences with eps 1e-6 resolve atol)
    p = {k: (0.3 * torch.randn(sh, dtype=torch.float64)).requires_grad_(True) for k, sh in
         qmix_model.shapes(A, S, 16, 32).items()}
    q = torch.randn(2, 2, A, dtype=torch.float64, requires_grad=True)
    s = torch.randn(2, 2, S, dtype=torch.float64)
    keys = list(p)

    def f(q, *vals):
        return qmix_model.qmix_forward(dict(zip(keys, vals)), q, s, pos_func, beta)
    assert torch.autograd.gradcheck(f, (q, *p.values()), eps=1e-6, atol=1e-6)


def test_monotone_in_q_with_abs():
    torch.manual_seed(2)
    A, S = 5, 40
    p = {k: torch.randn(sh, dtype=torch.float64) for k, sh in qmix_model.shapes(A, S).items()}
    q = torch.randn(4, 6, A, dtype=torch.float64, requires_grad=True)
    s = torch.randn(4, 6, S, dtype=torch.float64)
    g, = torch.autograd.grad(qmix_model.qmix_forward(p, q, s).sum(), q)
    assert bool((g >= 0).all()) and bool((g > 0).any())


def test_vdn_is_the_sum():
    q = torch.randn(3, 4, 5, dtype=torch.float64)
    assert torch.equal(qmix_model.vdn_forward(q), q.sum(2))
    assert torch.equal(qmix_model.mix("vdn", {}, q, None), q.sum(2))


def test_modules_build_on_the_cpu():
    from t2omca_amd import ops
    from t2omca_amd.modules import QMixer, TransformerMixer, VDNMixer, make_mixer
    torch.manual_seed(0)
    m = QMixer(_args(8))
    sd = m.state_dict()
    assert list(sd) == list(qmix_model.KEYS)
    assert {k: tuple(v.shape) for k, v in sd.items()} == qmix_model.shapes(8, 64)
    assert [k for k, _ in m.named_parameters()] == list(qmix_model.KEYS)  # registration order = opt.th order
    assert sum(p.numel() for p in m.parameters()) == 31233 == m.shape.n_params
    assert [(k, tuple(sh)) for k, sh in ops.qmix_param_blocks(8, 64)] == [(k, tuple(v.shape)) for k, v in sd.items()]
    assert m.kind == "qmix" and VDNMixer.kind == "vdn" and TransformerMixer.kind == "transformer"
    assert (m.n_agents, m.embed_dim, m.hypernet_embed, m.state_dim) == (8, 32, 64, 64)
    # torch's default initialisation: the same draws as the plain module under one seed
    torch.manual_seed(0)
    plain = PlainQMixer(8, 64)
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), plain.state_dict().values()))
    small = QMixer(_args(6, mixing_embed_dim=16, hypernet_embed=32, state_shape=(6, 8)))
    assert small.shape == ops.QmixShape(6, 48, 16, 32, 0, 1.0)
    assert QMixer(_args(4, qmix_pos_func="softplus", qmix_pos_func_beta=0.5)).shape.pos_beta == 0.5
    assert QMixer(_args(4), abs=False).shape.pos_func == 3
    assert list(VDNMixer().parameters()) == [] and VDNMixer().state_dict() == {}
    for A in range(1, 65):  # PyMARL2's defaults at every AGV count
        assert QMixer(_args(A)).shape.n_params > 0


@pytest.mark.parametrize("kw,limit", [(dict(mixing_embed_dim=48), "mixing_embed_dim"), (dict(hypernet_embed=128),
                                                                                      "hypernet_embed"),
                                      (dict(state_shape=2048), "state width"), (dict(n_agents=65), "n_agents")])
def test_unsupported_sizes_fail_at_construction(kw, limit):
    from t2omca_amd.modules import QMixer
    with pytest.raises(ValueError, match=limit):
        QMixer(_args(8, **kw))


def test_make_mixer_dispatch():
    from t2omca_amd.modules import QMixer, TransformerMixer, VDNMixer, make_mixer
    from t2omca_amd.synthetic import make_args
    assert type(make_mixer(_args(3, mixer="qmix"))) is QMixer
    assert type(make_mixer(_args(3, mixer="vdn"))) is VDNMixer
    assert type(make_mixer(_args(3))) is TransformerMixer
    assert type(make_mixer(_args(3, mixer="transformer"))) is TransformerMixer
    # make_args: the new fields only with mixer=, its present output otherwise unchanged
    base = vars(make_args(3, device="cpu"))
    assert "mixer" not in base and "state_shape" not in base and "mixing_embed_dim" not in base
    with_q = vars(make_args(3, device="cpu", mixer="qmix"))
    assert {k: v for k, v in with_q.items() if k in base} == base
    assert (with_q["mixer"], with_q["mixing_embed_dim"], with_q["hypernet_embed"], with_q["state_shape"]) == \
        ("qmix", 32, 64, 24)


def test_mixers_refuse_cpu_tensors():
    from t2omca_amd.modules import QMixer, VDNMixer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        QMixer(_args(3))(torch.zeros(2, 2, 3), torch.zeros(2, 2, 24))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VDNMixer()(torch.zeros(2, 2, 3), None)
