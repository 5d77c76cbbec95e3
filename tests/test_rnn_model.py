"""CPU: the GRU agent's restatement (tests/rnn_model.py) pinned to torch itself, the
input builder, the RNNAgent parameter tree and the argument validation that runs
without a device."""
import types

import pytest
import torch

from tests import rnn_model

NA = 5


def _args(A, H=64, **kw):
    return types.SimpleNamespace(**{**dict(n_agents=A, n_actions=NA, rnn_hidden_dim=H, agent="rnn", device="cpu"),
                                    **kw})


def _torch_agent(IN, H):
    return torch.nn.ModuleDict(dict(fc1=torch.nn.Linear(IN, H), rnn=torch.nn.GRUCell(H, H),
                                    fc2=torch.nn.Linear(H, NA)))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("H", [32, 64])
def test_unroll_against_torch_modules(H):
    """Outputs and the autograd gradients of a random scalar loss to 1e-12 normwise: the
    restatement, gate order included, is torch.nn.GRUCell's."""
    torch.manual_seed(1)
    B, T1, A, IN = 3, 4, 2, 14
    ref = _torch_agent(IN, H).double()
    p = {k: v.detach().clone().requires_grad_(True) for k, v in ref.state_dict().items()}
    assert tuple(p) == rnn_model.KEYS and {k: tuple(v.shape) for k, v in p.items()} == rnn_model.shapes(IN, H, NA)
    x = torch.randn(B, T1, A, IN, dtype=torch.float64)
    h0 = torch.randn(B, A, H, dtype=torch.float64).requires_grad_(True)
    wq, wh = torch.randn(B, T1, A, NA, dtype=torch.float64), torch.randn(B, T1, A, H, dtype=torch.float64)
    q, h = rnn_model.unroll(p, x, h0)
    g = torch.autograd.grad((q * wq).sum() + (h * wh).sum(), list(p.values()) + [h0])
    h0r = h0.detach().clone().requires_grad_(True)
    hr, qs, hs = h0r.view(-1, H), [], []
    for t in range(T1):
        hr = ref["rnn"](torch.relu(ref["fc1"](x[:, t].reshape(-1, IN))), hr)
        hs.append(hr.view(B, A, H))
        qs.append(ref["fc2"](hr).view(B, A, NA))
    qr, hrs = torch.stack(qs, 1), torch.stack(hs, 1)
    gr = torch.autograd.grad((qr * wq).sum() + (hrs * wh).sum(), list(ref.parameters()) + [h0r])
    assert _rel(q, qr) <= 1e-12 and _rel(h, hrs) <= 1e-12
    for name, a, b in zip(list(p) + ["h0"], g, gr):
        assert _rel(a, b) <= 1e-12, name


def test_build_inputs():
    B, T1, A, OBS = 2, 4, 3, 6
    g = torch.Generator().manual_seed(0)
    obs = torch.randn(B, T1, A, OBS, generator=g, dtype=torch.float64)
    acts = torch.randint(0, NA, (B, T1, A, 1), generator=g)
    x = rnn_model.build_inputs(obs, acts, NA, True, True)
    assert x.shape == (B, T1, A, OBS + NA + A) and x.dtype == obs.dtype
    assert torch.equal(x[..., :OBS], obs)
    last = x[..., OBS:OBS + NA]
    assert not bool(last[:, 0].any())  # zero at t = 0
    assert torch.equal(last[:, 1:].argmax(3), acts[:, :-1, :, 0]) and bool((last[:, 1:].sum(3) == 1).all())
    assert torch.equal(x[..., OBS + NA:], torch.eye(A, dtype=obs.dtype).expand(B, T1, A, A))
    assert torch.equal(rnn_model.build_inputs(obs, None, NA, False, False), obs)
    assert rnn_model.build_inputs(obs, acts[..., 0], NA, True, False).shape[3] == OBS + NA
    assert torch.equal(rnn_model.build_inputs(obs, None, NA, False, True)[..., OBS:],
                       torch.eye(A, dtype=obs.dtype).expand(B, T1, A, A))


@pytest.mark.parametrize("entity", [False, True])
@pytest.mark.parametrize("flags", [False, True])
@pytest.mark.parametrize("H", [32, 64])
def test_make_agent_parameter_tree(entity, flags, H):
    from t2omca_amd import modules
    A = 3
    obs_dim = 9 * A if entity else 6
    IN = obs_dim + ((NA + A) if flags else 0)
    agent = modules.make_agent(IN, _args(A, H, obs_last_action=flags, obs_agent_id=flags))
    assert isinstance(agent, modules.RNNAgent) and agent.kind == "rnn"
    sd = agent.state_dict()
    assert tuple(sd) == rnn_model.KEYS
    assert {k: tuple(v.shape) for k, v in sd.items()} == rnn_model.shapes(IN, H, NA)
    sh = agent.shape
    assert (sh.A, sh.OBS, sh.NA, sh.H, sh.last_action, sh.agent_id, sh.IN) == (A, obs_dim, NA, H, flags, flags, IN)
    assert sh.n_params == sum(v.numel() for v in sd.values())
    assert tuple(agent.init_hidden().shape) == (1, H) and not bool(agent.init_hidden().any())
    ref = _torch_agent(IN, H)
    agent.load_state_dict(ref.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(agent.parameters(), ref.parameters()))
    other = _torch_agent(IN, H)
    other.load_state_dict(agent.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(other.parameters(), ref.parameters()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        agent(torch.zeros(2, A, IN), agent.init_hidden())


def test_make_agent_default_is_the_transformer():
    from t2omca_amd import modules
    from t2omca_amd.synthetic import make_args
    args = make_args(3, device="cpu")
    t = modules.make_agent(27, args)
    assert isinstance(t, modules.TransformerAgent) and t.kind == "transformer"
    assert isinstance(modules.make_agent(14, types.SimpleNamespace(**{**vars(args), "agent": "n_rnn"})),
                      modules.RNNAgent)
    # the defaults are PyMARL's: both one-hots on, 64 hidden units
    a = modules.make_agent(14, types.SimpleNamespace(n_agents=3, n_actions=NA, agent="rnn", device="cpu"))
    assert a.shape.OBS == 6 and a.shape.H == 64 and a.shape.last_action and a.shape.agent_id


def test_use_orthogonal():
    from t2omca_amd import modules
    torch.manual_seed(0)
    a = modules.make_agent(14, _args(3, use_orthogonal=True, gain=0.5))
    w = a.fc1.weight.detach().double()
    assert torch.allclose(w.T @ w, torch.eye(14, dtype=torch.float64), atol=1e-5)  # orthonormal columns
    assert not bool(a.fc1.bias.any()) and not bool(a.fc2.bias.any())
    w2 = a.fc2.weight.detach().double()
    assert torch.allclose(w2 @ w2.T, 0.25 * torch.eye(NA, dtype=torch.float64), atol=1e-5)


def test_unsupported_arguments_raise():
    from t2omca_amd import modules
    with pytest.raises(ValueError, match="use_layer_norm"):
        modules.make_agent(14, _args(3, use_layer_norm=True))
    with pytest.raises(ValueError, match=r"rnn_hidden_dim=48.*rnn_hidden_dim in \{32, 64\}"):
        modules.make_agent(14, _args(3, 48))
    with pytest.raises(ValueError, match="GRU kernels take"):
        modules.make_agent(14, _args(65))
    with pytest.raises(ValueError, match="GRU kernels take"):
        modules.make_agent(4, _args(3))  # no room for the observation


def test_learner_refuses_what_the_rnn_agent_does_not_run():
    """(The checks come before the learner asks for a device.)"""
    from t2omca_amd import modules
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.synthetic import make_args
    A = 3
    args = types.SimpleNamespace(**{**vars(make_args(A, device="cpu", mixer="qmix")), "agent": "rnn"})
    agent, mixer = modules.make_agent(9 * A + NA + A, args), modules.make_mixer(args)
    with pytest.raises(ValueError, match="flat mixers.*supported"):
        TDLearner(agent, modules.TransformerMixer(args))
    with pytest.raises(ValueError, match="pipeline=True"):
        TDLearner(agent, mixer, pipeline=True)
    noisy = types.SimpleNamespace(**{**vars(args), "action_selector": "noisy-new"})
    with pytest.raises(ValueError, match="noisy"):
        TDLearner(modules.make_agent(9 * A + NA + A, noisy), mixer)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # what is left is the device
        TDLearner(agent, mixer)
