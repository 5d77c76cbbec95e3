"""CPU: the fp64 restatement of the NoisyNet head (tests/noisy_model.py) checks
itself — the written-out backward against torch autograd of the written-out
forward, and the counter-based Box–Muller noise: deterministic, a function of every
argument, and standard normal over 2^16 draws (|mean| < 4/√n, |var − 1| < 4·√(2/n):
four standard errors of the mean and of the variance of n N(0, 1) draws)."""
import numpy as np
import pytest
import torch

from tests import noisy_model as nm


def _case(B, T, A, E, NA, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    return dict(h=r(B, T, A, E), u_w=r(NA, E), u_b=r(NA), s_w=0.3 * r(NA, E), s_b=0.3 * r(NA),
                eps_w=r(T, NA, E), eps_b=r(T, NA), g=r(B, T, A), gh_in=r(B, T, A, E),
                act=torch.randint(0, NA, (B, T, A), generator=g))


@pytest.mark.parametrize("B,T,A,E,NA", [(3, 4, 5, 32, 5), (2, 3, 3, 16, 5), (2, 2, 4, 64, 16)])
def test_head_backward_matches_autograd(B, T, A, E, NA):
    c = _case(B, T, A, E, NA, 0)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("h", "u_w", "u_b", "s_w", "s_b")}
    # the written-out expression, step by step and row by row
    q = torch.stack([torch.stack([
        (leaves["u_w"] + leaves["s_w"] * c["eps_w"][t]) @ leaves["h"][b, t].T
        + (leaves["u_b"] + leaves["s_b"] * c["eps_b"][t])[:, None] for t in range(T)]) for b in range(B)])
    q = q.permute(0, 1, 3, 2)  # [B, T, A, NA]
    assert torch.allclose(q, nm.noisy_head(c["h"], c["u_w"], c["u_b"], c["s_w"], c["s_b"], c["eps_w"], c["eps_b"]),
                          rtol=1e-12, atol=1e-12)
    chosen = torch.gather(q, 3, c["act"].unsqueeze(-1)).squeeze(-1)
    loss = (chosen * c["g"]).sum() + (leaves["h"] * c["gh_in"]).sum()
    gh, gu_w, gu_b, gs_w, gs_b = torch.autograd.grad(loss, [leaves[k] for k in ("h", "u_w", "u_b", "s_w", "s_b")])
    out = nm.noisy_head_grads(c["h"], c["u_w"], c["s_w"], c["eps_w"], c["eps_b"], c["g"], c["act"], c["gh_in"])
    for name, want, got in zip(("gh", "du_w", "du_b", "ds_w", "ds_b"), (gh, gu_w, gu_b, gs_w, gs_b), out):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-11), name


def test_mean_head_is_the_plain_linear():
    c = _case(2, 3, 4, 32, 5, 1)
    q = nm.noisy_head(c["h"], c["u_w"], c["u_b"], c["s_w"], c["s_b"])
    assert torch.allclose(q, torch.nn.functional.linear(c["h"], c["u_w"], c["u_b"]), rtol=1e-13, atol=1e-13)
    zero = nm.noisy_head(c["h"], c["u_w"], c["u_b"], c["s_w"], c["s_b"], 0 * c["eps_w"], 0 * c["eps_b"])
    assert torch.equal(q, zero)


def test_noise_is_a_function_of_its_arguments():
    E, NA, T = 32, 5, 3
    a = nm.noise_normal(E, NA, T, 7, "learner_online", 11)
    b = nm.noise_normal(E, NA, T, 7, "learner_online", 11)
    assert a[0].dtype == np.float32 and a[0].shape == (T, NA, E) and a[1].shape == (T, NA)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for seed, kind, counter in ((8, "learner_online", 11), (7, "learner_target", 11), (7, "learner_online", 12),
                                (7, "runner", 11)):
        other = nm.noise_normal(E, NA, T, seed, kind, counter)
        assert not np.array_equal(a[0], other[0]) and not np.array_equal(a[1], other[1])
    # step t's block depends on t only: a longer unroll extends a shorter one
    longer = nm.noise_normal(E, NA, T + 2, 7, "learner_online", 11)
    assert np.array_equal(longer[0][:T], a[0]) and np.array_equal(longer[1][:T], a[1])
    assert not np.array_equal(a[0][0], a[0][1])
    # seed' = 4·seed + kind: (seed 1, kind 0) is not (seed 0, any kind)
    s1 = nm.noise_normal(E, NA, 1, 1, 0, 0)[0]
    assert all(not np.array_equal(s1, nm.noise_normal(E, NA, 1, 0, k, 0)[0]) for k in range(4))
    w64, b64 = nm.noise64(E, NA, 0, T, 7, 0, 11)
    assert np.isfinite(w64).all() and np.isfinite(b64).all()


def test_noise_is_standard_normal():
    E, NA = 63, 16                      # NA·(E+1) = 1024 draws per step
    w, b = nm.noise64(E, NA, 0, 64, 3, "runner", 5)
    z = np.concatenate([w.reshape(-1), b.reshape(-1)])
    n = z.size
    assert n == 1 << 16
    mean, var = z.mean(), z.var()
    print(f"n = {n}: mean {mean:+.4e} (bar {4 / np.sqrt(n):.4e}), "
          f"var - 1 {var - 1:+.4e} (bar {4 * np.sqrt(2 / n):.4e})")
    assert abs(mean) < 4 / np.sqrt(n)
    assert abs(var - 1) < 4 * np.sqrt(2 / n)


def test_noise_limits_are_checked():
    with pytest.raises(AssertionError):
        nm.noise64(64, 32, 0, 1, 0, 0, 0)        # NA·(E+1) > 2048
    with pytest.raises(AssertionError):
        nm.noise64(32, 5, 0, 1, 0, 0, 1 << 28)   # counter
