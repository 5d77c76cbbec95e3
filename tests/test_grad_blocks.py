"""CPU: the per-block gradient comparator (tests/grad_blocks.py) sees what the flat
normwise metric misses, and the bf16-operand emulation of the oracle engages.

Everything here is the fp64 oracle's TD update at (A, B, T) = (8, 6, 5), the model
torch.manual_seed(0) and batch seed 3 of tests/test_gpu_generic._td; no kernel runs.
"""
import pytest
import torch

from tests import grad_blocks as gb
from tests.gpu_util import normwise

QUERY = "mixer.transformer.tblocks.1.attention.toqueries.weight"


def cpu_case(A, B, T, seed=3, **cfg_kw):
    """(pa, pm, cfg, batch, w) of a case of tests/test_gpu_generic._td, all on the CPU."""
    from t2omca_amd.modules import TransformerAgent, TransformerMixer
    from t2omca_amd.synthetic import make_batch
    from tests.test_gpu_generic import _args, _cfg_of
    cfg = _cfg_of(A, **cfg_kw)
    torch.manual_seed(gb.module_seed(A))
    args = _args(cfg, device="cpu")
    agent, mixer = TransformerAgent(None, args), TransformerMixer(args)
    pa = {k: v.detach().double() for k, v in agent.state_dict().items()}
    pm = {k: v.detach().double() for k, v in mixer.state_dict().items()}
    batch, w = make_batch(B, T, A, seed=seed, obs_feats=9, state_feats=8, device="cpu")
    return pa, pm, cfg, batch, w


@pytest.fixture(scope="module")
def case():
    pa, pm, cfg, batch, w = cpu_case(8, 6, 5)
    ref = gb.oracle_grad(pa, pm, cfg, batch, w)[0]
    emu = gb.emulated_bf16_grad(pa, pm, cfg, batch, w)
    return dict(pa=pa, pm=pm, cfg=cfg, batch=batch, w=w, ref=ref, emu=emu)


def _damaged(case):
    ref, bl = case["ref"], {n: (a, b) for n, a, b in gb.blocks(case["pa"], case["pm"])}
    a, b = bl[QUERY]
    zeroed, scaled, no_mixer = ref.clone(), ref.clone(), ref.clone()
    zeroed[a:b] = 0
    scaled[a:b] *= 0.9
    no_mixer[min(s for n, (s, _) in bl.items() if n.startswith("mixer.")):] = 0
    small = ref.clone()
    gmax = float(ref.abs().max())
    hidden = [n for n, (s, e) in bl.items() if float(ref[s:e].abs().max()) < 6e-2 * gmax]
    for n in hidden:
        small[bl[n][0]:bl[n][1]] = 0
    return dict(zeroed=zeroed, scaled=scaled, no_mixer=no_mixer, small=small), hidden


def test_blocks_catch_what_the_flat_metric_passes(case):
    """Damaged copies of the oracle gradient: (a) the mixer's second toqueries gradient
    zeroed, (b) that block scaled by 0.9, (c) every mixer block zeroed, (d) every block
    whose own maximum is below 6e-2 of the global one zeroed: 34 of the 60, 57,505 of
    84,006 elements, 28 of the mixer's 30 among them.
    Flat normwise error against the undamaged gradient, measured: (a) 3.0e-3,
    (b) 3.0e-4, (c) 9.1e-2, (d) 5.2e-2.  (a), (b) and (d) pass bf16's flat 6e-2, and
    (a), (b) are 100x / 10x the fp32 bar 3e-5 although the block is wholly wrong (its
    own scale is 3.0e-3 of the global maximum).  (c) does not pass the flat bar at this
    case: two mixer blocks, tblocks.0.attention.unifyheads.bias (9.1e-2) and
    tblocks.1.norm2.weight (6.8e-2), lie above it, so what the flat metric sees of a
    missing mixer is exactly the larger of the two; (d) is the hole it cannot see.
    Per block all four fail at both precisions' bars."""
    pa, pm, ref, emu = case["pa"], case["pm"], case["ref"], case["emu"]
    damaged, hidden = _damaged(case)
    flat = {k: normwise(g, ref) for k, g in damaged.items()}
    print({k: f"{v:.2e}" for k, v in flat.items()}, len(hidden), "blocks below 6e-2")
    assert flat["zeroed"] < 6e-2 and flat["scaled"] < 6e-2 and flat["small"] < 6e-2, flat
    assert flat["zeroed"] <= 100 * 3e-5 and flat["scaled"] <= 10 * 3e-5, flat
    rows = gb.block_errors(ref, ref, pa, pm)
    assert len(hidden) == 34 and sum(r["size"] for r in rows if r["name"] in hidden) == 57505
    assert sum(n.startswith("mixer.") for n in hidden) == 28
    assert flat["no_mixer"] == max(r["share"] for r in rows if r["name"].startswith("mixer.")) < 0.1
    for k, g in damaged.items():
        with pytest.raises(AssertionError, match="blocks at or above"):
            gb.assert_blocks_fp32(g, ref, pa, pm, tag=k)
        with pytest.raises(AssertionError, match="blocks above"):
            gb.assert_blocks_bf16(g, ref, emu, pa, pm, tag=k)
    # the failure names the damaged block first
    rows = sorted(gb.block_errors(damaged["scaled"], ref, pa, pm), key=lambda r: -r["emax"])
    assert rows[0]["name"] == QUERY and abs(rows[0]["emax"] - 0.1) < 1e-12 and abs(rows[0]["el2"] - 0.1) < 1e-12
    assert all(r["emax"] == 0 for r in rows[1:])


def test_undamaged_gradients_pass(case):
    """The oracle against itself, and the oracle in float32 against fp64 (<= 5.9e-7 per
    block, 50x under the fp32 bar); the emulation against its own bar."""
    pa, pm, ref = case["pa"], case["pm"], case["ref"]
    gb.assert_blocks_fp32(ref, ref, pa, pm, tag="self")
    f32 = gb.oracle_grad(pa, pm, case["cfg"], case["batch"], case["w"], dtype=torch.float32)[0]
    rows = gb.assert_blocks_fp32(f32, ref, pa, pm, tag="float32 oracle")
    assert max(r["emax"] for r in rows) < 3e-6
    gb.assert_blocks_bf16(case["emu"], ref, case["emu"], pa, pm, tag="emulation")


def test_unfit_reference_is_refused(case):
    """A reference with an all-zero block, or one below 1e-5 of the global maximum,
    is an unfit input: the comparator raises even when the gradients are equal."""
    pa, pm = case["pa"], case["pm"]
    a, b = next((a, b) for n, a, b in gb.blocks(pa, pm) if n == "mixer.hyper_b2.bias")
    for scale in (0.0, 1e-4):
        ref = case["ref"].clone()
        ref[a:b] *= scale
        with pytest.raises(AssertionError, match="unfit input"):
            gb.assert_blocks_fp32(ref, ref, pa, pm)
        with pytest.raises(AssertionError, match="unfit input"):
            gb.assert_blocks_bf16(ref, ref, ref, pa, pm)
    assert gb.assert_fit(case["ref"], pa, pm) >= 1e-3


def test_block_names_follow_the_reference_order(case):
    names = [n for n, _, _ in gb.blocks(case["pa"], case["pm"])]
    assert len(names) == 60 and names[0] == "agent.feat_embedding.weight" and names[-1] == "mixer.hyper_b2.bias"
    assert gb.blocks(case["pa"], case["pm"])[-1][2] == case["ref"].numel() == 84006
    assert {gb.block_class(n) for n in names} == set(gb.CLASSES)
    assert gb.block_class("agent.q_basic.s_w") == "agent FFN/LN"


def test_round_bf16_is_round_to_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, -3.3, 1e-20, 0.0],
                     dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.296875, 0.0, 0.0], dtype=torch.float64)
    got = gb.round_bf16(x)
    assert torch.equal(got[:5], want[:5]) and got[6] == 0
    assert torch.equal(got, got.float().bfloat16().double())  # representable in bf16
    y = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).float().double()
    assert torch.equal(gb.round_bf16(y), y.float().bfloat16().double())


def test_emulation_without_rounding_is_the_oracle_bit_for_bit(case):
    mode = gb.Bf16Operands(rounding=False)
    g, loss, prio, _ = gb.oracle_grad(case["pa"], case["pm"], case["cfg"], case["batch"], case["w"], mode=mode)
    _, loss0, prio0, _ = gb.oracle_grad(case["pa"], case["pm"], case["cfg"], case["batch"], case["w"])
    assert mode.calls > 100
    assert torch.equal(loss, loss0) and torch.equal(prio, prio0)
    assert torch.equal(g, case["ref"])


def test_folded_attention_is_the_oracles_attention(case):
    """The kernels' association of the attention (grad_blocks.folded_mha), with no
    rounding: the oracle's gradient to fp64 rounding in every block."""
    mode = gb.Bf16Operands(rounding=False, fold=True)
    g = gb.oracle_grad(case["pa"], case["pm"], case["cfg"], case["batch"], case["w"], mode=mode)[0]
    from oracle import ref_model
    assert ref_model.mha is not gb.folded_mha  # (restored on exit)
    rows = gb.block_errors(g, case["ref"], case["pa"], case["pm"])
    assert max(r["emax"] for r in rows) < 1e-12, max(r["emax"] for r in rows)
    plain = gb.oracle_grad(case["pa"], case["pm"], case["cfg"], case["batch"], case["w"], mode=gb.Bf16Operands())[0]
    assert not torch.equal(plain, case["emu"])  # the emulation the tests use is the folded one


def test_emulation_error_is_of_bf16_size(case):
    """The mode engages: flat normwise error of the emulation at (8, 6, 5) within
    [1e-3, 2e-2] (measured 8.6e-3; 8.8e-3 unfolded); per block in relative L2 at most a few percent."""
    err = normwise(case["emu"], case["ref"])
    rows = gb.block_errors(case["emu"], case["ref"], case["pa"], case["pm"])
    print(f"emulation flat {err:.2e}, worst block el2 {max(r['el2'] for r in rows):.2e} "
          f"emax {max(r['emax'] for r in rows):.2e}")
    assert 1e-3 <= err <= 2e-2, err
    assert all(2.0 ** -12 < r["el2"] < 0.1 for r in rows), sorted((r["el2"], r["name"]) for r in rows)
