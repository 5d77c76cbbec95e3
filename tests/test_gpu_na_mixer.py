"""GPU: the transformer mixer's Q selection (t2o_mixer_unroll_fwd, qmode 1 and 2) at action
counts other than five.

mix_load (t2o_mixer_parts.hpp) prefetches MIX_MAXNA = 8 action slots per lane whatever the
action count, the slots past NA as clamped duplicates of slot NA - 1, and mix_qv masks
them with -inf before its first-maximum scan.  Five actions leave three such slots; here
run eight (none: the full width), seven (one), three and two (most of the row padding) and
one (every slot a duplicate of slot 0, the selection always 0), on the one-tile exact and
runtime instances (8 and 5 agents), the two-tile 16-agent mixer decoupled and one-wave
(T2O_MIXER_SPLIT=1 / 0), and the runtime-shaped kernels' own selection (T2O_GENERIC=1).

Inputs of qselect_case: the online Q is integer-valued in -3..3 (ties in most rows, which
the first-maximum rule decides), the target Q N(0, 1); avail is Bernoulli(0.6) with no
action forced on, so rows with nothing available occur, and (b, t, a) = (1, 0, 0) is made
one (the reference's -9999999 masking then selects action 0); agent 1 of episode 0 has
only action NA - 1 at every step; the actions are uniform with 0 and NA - 1 both present.

The selected values must EQUAL a torch gather of the given Q bit for bit: the online
network's at the recorded actions, the target network's at the avail-masked first-maximum
argmax of the online Q.  y and hw of both networks are held to the fp32 forward bar 1e-5
against oracle/ref_model on the gathered values, as tests/test_gpu_mixer.py does.

The C ABI: with a selection mode on, more than t2o_mixer_max_actions() = 8 actions are
T2O_EUNSUPPORTED on the MFMA instances; qmode 0 (the drop-in module's path) reads no Q
row and runs at any count.

MEASURED on an MI355X: the selected values bit-equal in every case (rows with a tied maximum:
0.17 - 0.30 of them from two actions up); y <= 2.1e-7, hw <= 6.9e-7 normwise.
"""
import pytest
import torch

from oracle import ref_model
from tests.gpu_util import flat_from_dict, normwise, require_gpu
from tests.test_gpu_mixer import TOL_F32, _shape

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _kernel_family(monkeypatch):
    monkeypatch.setenv("T2O_GENERIC", "0")
    monkeypatch.delenv("T2O_MIXER_SPLIT", raising=False)


def qselect_inputs(A, B, T, NA, seed=33):
    g = torch.Generator().manual_seed(seed + NA)
    Tq = T + 1
    d = dict(states=torch.randn(B, Tq, A * 8, generator=g), h_on=torch.randn(B, Tq, A, 32, generator=g),
             h_tg=torch.randn(B, Tq, A, 32, generator=g),
             q_on=torch.randint(-3, 4, (B, Tq, A, NA), generator=g).float(),
             q_tg=torch.randn(B, Tq, A, NA, generator=g))
    actions = torch.randint(0, NA, (B, Tq, A, 1), generator=g)
    actions[0, 0, 0, 0], actions[0, 0, 1, 0] = 0, NA - 1
    avail = (torch.rand(B, Tq, A, NA, generator=g) < 0.6).int()
    avail[0, :, 1] = 0
    avail[0, :, 1, NA - 1] = 1  # only the last action
    avail[1, 0, 0] = 0          # nothing available
    d.update(actions=actions, avail=avail)
    return d


def qselect_case(A, B, T, NA, instance):
    require_gpu()
    from t2omca_amd import ops
    cfg = dict(n_agents=A, n_entities=A, state_entity_feats=8, mixer_emb=32, mixer_heads=3,
               mixer_depth=2, ff_hidden_mult=4)
    shape = _shape(cfg)
    assert shape.instance == instance
    p_on = ref_model.init_params("mixer", cfg, 31)
    p_tg = ref_model.init_params("mixer", cfg, 32)
    d = qselect_inputs(A, B, T, NA)
    Tq = T + 1
    q_on, q_tg, actions, avail = d["q_on"], d["q_tg"], d["actions"], d["avail"]
    packs = [ops.pack_params(shape, flat_from_dict(p).cuda()) for p in (p_on, p_tg)]
    o_on, o_tg = ops.mixer_unroll_fwd(shape, packs[0], d["states"].cuda(), d["h_on"].cuda(), qmode_on=1,
                                      q_on=q_on.cuda(), actions=actions.cuda()[..., 0], avail=avail.cuda(), T_on=T,
                                      pack_tg=packs[1], hid_tg=d["h_tg"].cuda(), qmode_tg=2, q_tg=q_tg.cuda(),
                                      T_tg=Tq)
    torch.cuda.synchronize()
    chosen = torch.gather(q_on[:, :T], 3, actions[:, :T]).squeeze(3)
    qd = q_on.clone()
    qd[avail == 0] = -9999999
    sel = qd.argmax(dim=3, keepdim=True)  # (the first maximum)
    assert int(sel[1, 0, 0]) == 0 and bool((sel[0, :, 1] == NA - 1).all())
    ties = float(((qd == qd.max(dim=3, keepdim=True).values).sum(3) > 1).double().mean())
    tmax = torch.gather(q_tg, 3, sel).squeeze(3)
    assert torch.equal(o_on["qv"].cpu(), chosen)
    assert torch.equal(o_tg["qv"].cpu(), tmax)
    errs = {}
    for name, p, qv, h, T_, o in (("on", p_on, chosen, d["h_on"], T, o_on), ("tg", p_tg, tmax, d["h_tg"], Tq, o_tg)):
        pd = {k: v.double() for k, v in p.items()}
        y, hw = ref_model.mixer_unroll(pd, qv.double(), h[:, :T_].double(), d["states"][:, :T_].double(),
                                       torch.zeros(B, 3, 32, dtype=torch.float64), cfg=cfg)
        errs[name] = (normwise(o["y"], y), normwise(o["hw"], hw))
    print(f"mixer qselect {(A, B, T, NA)} {instance}: rows with a tied maximum {ties:.2f}; y / hw {errs}")
    assert max(max(e) for e in errs.values()) < TOL_F32, errs


@pytest.mark.parametrize("A,B,T,NA,instance", [(8, 4, 5, 1, "exact"), (8, 4, 5, 2, "exact"), (8, 4, 5, 8, "exact"),
                                               (5, 3, 4, 7, "runtime")])
def test_qselect_one_tile(A, B, T, NA, instance):
    qselect_case(A, B, T, NA, instance)


@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("A,B,T,NA", [(16, 3, 4, 3), (16, 3, 4, 8)])
def test_qselect_two_tiles(monkeypatch, A, B, T, NA, split):
    """16 agents: the decoupled mixer (t2o_mixer_split.hip: T2O_MIXER_SPLIT=1) and the
    one-wave multi-tile kernel (=0) each run mix_load / mix_qv in their own step loop."""
    require_gpu()
    import ctypes

    from t2omca_amd import _lib
    monkeypatch.setenv("T2O_MIXER_SPLIT", split)
    L = _lib.make_layout(1, 32, 3, 2, 8, 1, 128, A)
    assert _lib.lib().t2o_mixer_split(ctypes.byref(L), B) == int(split)
    qselect_case(A, B, T, NA, "exact")


def test_qselect_generic(monkeypatch):
    """T2O_GENERIC=1: the runtime-shaped mixer's own selection loop (t2o_generic.hip)."""
    monkeypatch.setenv("T2O_GENERIC", "1")
    qselect_case(4, 3, 5, 6, "generic")


def test_nine_actions_abi_limit():
    """Nine actions: a selection mode on either network is T2O_EUNSUPPORTED (-2) on the MFMA
    instance, with no launch; qmode 0 with one network runs and gives the oracle's y."""
    require_gpu()
    from t2omca_amd import _lib, ops
    A, B, T, NA = 8, 3, 4, 9
    assert NA == _lib.lib().t2o_mixer_max_actions() + 1
    cfg = dict(n_agents=A, n_entities=A, state_entity_feats=8, mixer_emb=32, mixer_heads=3,
               mixer_depth=2, ff_hidden_mult=4)
    shape = _shape(cfg)
    p = ref_model.init_params("mixer", cfg, 31)
    pack = ops.pack_params(shape, flat_from_dict(p).cuda())
    d = qselect_inputs(A, B, T - 1, NA)
    dev = {k: v.cuda() for k, v in d.items()}
    act = dev["actions"][..., 0]
    for kw in (dict(qmode_on=1, q_on=dev["q_on"], actions=act),
               dict(qmode_on=2, q_on=dev["q_on"], avail=dev["avail"]),
               dict(qmode_on=0, qv_on=dev["q_tg"][..., 0].contiguous(), q_on=dev["q_on"], pack_tg=pack,
                    hid_tg=dev["h_tg"], qmode_tg=2, q_tg=dev["q_tg"], avail=dev["avail"])):
        with pytest.raises(RuntimeError, match="mixer_unroll_fwd failed with status -2"):
            ops.mixer_unroll_fwd(shape, pack, dev["states"], dev["h_on"], **kw)
    qv = d["q_tg"][..., 0].contiguous()
    out = ops.mixer_unroll_fwd(shape, pack, dev["states"], dev["h_on"], qmode_on=0, qv_on=qv.cuda(), q_on=dev["q_on"])
    torch.cuda.synchronize()
    y, hw = ref_model.mixer_unroll({k: v.double() for k, v in p.items()}, qv.double(), d["h_on"].double(),
                                   d["states"].double(), torch.zeros(B, 3, 32, dtype=torch.float64), cfg=cfg)
    assert torch.equal(out["qv"].cpu(), qv)
    assert normwise(out["y"], y) < TOL_F32 and normwise(out["hw"], hw) < TOL_F32
