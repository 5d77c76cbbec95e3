"""Per-parameter-block comparison of TD-update gradients, and a bf16-operand
emulation of the fp64 oracle (test helpers; CPU code only).

The flat metric normwise(g, ref) = max|Δ| / max|ref| over all parameters is set by
the block that holds the largest gradient (the agent's first unifyheads.bias); a
block whose own maximum is 1e-3 of that is checked to 3 % by a 3e-5 bar and not at
all by bf16's 6e-2.  Here every block (one parameter tensor, in the reference
order: agent then mixer, a noisy agent's u_w / u_b / s_w / s_b included) is
compared on its own scale:

    emax = max|Δ_block| / max|ref_block|        el2 = ‖Δ_block‖₂ / ‖ref_block‖₂

fp32  (assert_blocks_fp32): emax < 3e-5 in every block, the project's fp32 gradient
      bar.  The fp64 oracle evaluated in float32 stays <= 5.9e-7 in every block.
bf16  (assert_blocks_bf16): el2 <= max(2^-8, 4·e_emu) in every block, e_emu the el2
      error of emulated_bf16_grad for that same case: the oracle in fp64 with the
      operands of every matmul (F.linear, torch.bmm, torch.matmul: all it uses)
      rounded to bf16, round to nearest even, in the forward and in the backward
      (incoming gradient and saved operands), and with one rounding site of the kernels
      that the module-level form does not have, added after the first measurement: the
      MFMA kernels evaluate the attention with folded weights M_h = Wk_hᵀ Wq_h / √E and
      N_h = U_h Wv_h (t2o_pack.hip:5-9), whose bf16 images (t2o_pack.hip:114-115,
      129-130) are what a product rounds, and sum the p-weighted RAW keys before N_h
      (folded_mha below; without rounding it equals the oracle to 1e-15).  With the
      unfolded emulation the 5-AGV runtime case (5,4,6) exceeded the bar in four mixer
      blocks, the value path and the embedding that feeds it as keys (embedding weight
      1.28e-1 against 4 x 2.06e-2); folded, the emulation's own error there is 5.3e-2.
      2^-8 is two bf16 unit roundoffs, a
      floor where the emulation happens to land close.  The factor 4: the kernels
      round at more sites than the module-level emulation (folded projection weights,
      the bf16 tape, the recompute in the BPTT), about three per matmul adding
      linearly, plus one for the spread of a maximum over 60 blocks.

Fitness (assert_fit, part of both): a reference gradient with an all-zero block, or
a block whose maximum is below 1e-5 of the global one, cannot carry a block-relative
check: such a case is an unfit input, not a pass.
"""
import torch
import torch.nn.functional as F
from torch.overrides import TorchFunctionMode

FP32_BLOCK_BAR = 3e-5
BF16_FLOOR = 2.0 ** -8
BF16_MARGIN = 4.0
FIT_SHARE = 1e-5


def module_seed(A):
    """The torch.manual_seed the agent and mixer of a whole-update case are drawn with.
    With seed 0 the mixer's hyper_b2 ReLU (n_transf_mixer.py:82) is off at every record
    of the short unrolls (T <= 4) the cases with 13 AGVs and more use, at every batch
    seed 3..39: hyper_b2's reference gradient is then identically zero and the case
    unfit.  Seed 4 leaves no block below 5e-4 of the global maximum at any of them
    (computed on the CPU at batch seed 3)."""
    return 0 if A <= 12 else 4


CLASSES = ("agent attention", "agent FFN/LN", "mixer attention", "mixer FFN/LN", "hyper heads")


def block_class(name):
    """The kernel family a block's gradient comes from (DESIGN.md §5's table rows)."""
    net = name.split(".", 1)[0]
    if net == "mixer" and ".hyper_" in "." + name.split(".", 1)[1]:
        return "hyper heads"
    return f"{net} attention" if ".attention." in name else f"{net} FFN/LN"


def blocks(pa, pm):
    """[(name, start, stop)] of the flat vector: 'agent.<key>' then 'mixer.<key>'."""
    out, off = [], 0
    for net, src in (("agent", pa), ("mixer", pm)):
        for k, v in src.items():
            out.append((f"{net}.{k}", off, off + v.numel()))
            off += v.numel()
    return out


def _flat64(x):
    return x.detach().cpu().double().reshape(-1)


def block_errors(g, ref, pa, pm):
    """One dict per block: name, size, ref_max, share (ref_max / the global max), emax, el2."""
    g, ref = _flat64(g), _flat64(ref)
    bl = blocks(pa, pm)
    assert g.numel() == ref.numel() == bl[-1][2], (g.numel(), ref.numel(), bl[-1][2])
    gmax = float(ref.abs().max())
    rows = []
    for name, a, b in bl:
        r, d = ref[a:b], g[a:b] - ref[a:b]
        rmax, rl2 = float(r.abs().max()), float(r.norm())
        rows.append(dict(name=name, size=b - a, ref_max=rmax, share=rmax / gmax if gmax > 0 else 0.0,
                         emax=float(d.abs().max()) / rmax if rmax > 0 else float("inf"),
                         el2=float(d.norm()) / rl2 if rl2 > 0 else float("inf")))
    return rows


def assert_fit(ref, pa, pm, tag=""):
    """The fitness condition on a reference gradient; returns the smallest share."""
    ref = _flat64(ref)
    gmax = float(ref.abs().max())
    assert gmax > 0 and bool(torch.isfinite(ref).all()), f"{tag}: unfit reference gradient"
    unfit = [(n, float(ref[a:b].abs().max()) / gmax) for n, a, b in blocks(pa, pm)
             if float(ref[a:b].abs().max()) < FIT_SHARE * gmax]
    assert not unfit, f"{tag}: unfit input, blocks below {FIT_SHARE:g} of the global max|ref| (or zero): {unfit}"
    return min(float(ref[a:b].abs().max()) / gmax for _, a, b in blocks(pa, pm))


def _table(rows, key, extra=()):
    rows = sorted(rows, key=lambda r: -r[key])
    cols = ("emax", "el2", "share") + tuple(extra)
    head = "  " + " ".join(f"{c:>9}" for c in cols) + "  block"
    return "\n".join([head] + ["  " + " ".join(f"{r[c]:9.2e}" for c in cols) + f"  {r['name']} [{r['size']}]"
                               for r in rows])


def assert_blocks_fp32(g, ref, pa, pm, tag="", bar=FP32_BLOCK_BAR):
    """Every block's max|Δ| / max|ref_block| < bar against `ref`; prints the worst
    block, and on failure every block sorted by error.  Returns the rows."""
    assert_fit(ref, pa, pm, tag)
    rows = block_errors(g, ref, pa, pm)
    worst = max(rows, key=lambda r: r["emax"])
    print(f"BLOCKS {tag} fp32: worst block {worst['name']} emax {worst['emax']:.2e} el2 {worst['el2']:.2e} "
          f"(share {worst['share']:.1e}); smallest share {min(r['share'] for r in rows):.1e}")
    bad = [r for r in rows if not r["emax"] < bar]
    assert not bad, (f"{tag}: {len(bad)} of {len(rows)} blocks at or above {bar:g} of their own max|ref|:\n"
                     + _table(rows, "emax"))
    return rows


def assert_blocks_bf16(g, ref, emu, pa, pm, tag=""):
    """Every block's ‖Δ‖₂ / ‖ref_block‖₂ <= max(2^-8, 4·e_emu_block), e_emu the same
    figure of the bf16-operand emulation `emu` of this case; prints the worst block
    and the largest GPU / emulation ratio per block class.  Returns the rows."""
    assert_fit(ref, pa, pm, tag)
    rows = block_errors(g, ref, pa, pm)
    for r, e in zip(rows, block_errors(emu, ref, pa, pm)):
        r["e_emu"] = e["el2"]
        r["bar"] = max(BF16_FLOOR, BF16_MARGIN * e["el2"])
        r["ratio"] = r["el2"] / e["el2"] if e["el2"] > 0 else float("inf")
        r["of_bar"] = r["el2"] / r["bar"]
    worst = max(rows, key=lambda r: r["of_bar"])
    by_class = {c: max((r["ratio"] for r in rows if block_class(r["name"]) == c), default=float("nan"))
                for c in CLASSES}
    print(f"BLOCKS {tag} bf16: worst block {worst['name']} el2 {worst['el2']:.2e} emu {worst['e_emu']:.2e} "
          f"bar {worst['bar']:.2e}; largest el2 {max(r['el2'] for r in rows):.2e}; GPU/emulation by class "
          + ", ".join(f"{c} {v:.2f}" for c, v in by_class.items()))
    bad = [r for r in rows if not r["el2"] <= r["bar"]]
    assert not bad, (f"{tag}: {len(bad)} of {len(rows)} blocks above max(2^-8, 4 x emulation) in relative L2:\n"
                     + _table(rows, "of_bar", ("e_emu", "bar", "ratio")))
    return rows


# ---- the oracle with bf16 matmul operands ---------------------------------------

def round_bf16(x):
    """fp64 -> nearest bf16 value (8 significant bits, ties to even), kept in fp64;
    done on the fp64 value itself, not through float32 (no double rounding)."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


class _RoundedOperands(torch.autograd.Function):
    """func(a, b[, bias]) with a and b rounded by `rnd`; the backward is func's own
    autograd formula on the saved rounded operands and the rounded incoming gradient
    (the bias gradient takes the unrounded one: it is a sum, not a matmul)."""

    @staticmethod
    def forward(ctx, func, rnd, a, b, bias):
        ctx.func, ctx.rnd = func, rnd
        a, b = rnd(a), rnd(b)
        ctx.save_for_backward(a, b, bias)
        return func(a, b) if bias is None else func(a, b, bias)

    @staticmethod
    def backward(ctx, g):
        a, b, bias = ctx.saved_tensors
        need = ctx.needs_input_grad[2:]
        with torch.enable_grad(), torch._C.DisableTorchFunction():
            leaves = [t.detach().requires_grad_(True) if t is not None and n else t
                      for t, n in zip((a, b, bias), need)]
            out = ctx.func(*leaves[:2]) if bias is None else ctx.func(*leaves)
            ops = [t for t, n in zip(leaves[:2], need[:2]) if n]
            got = list(torch.autograd.grad(out, ops, ctx.rnd(g), retain_graph=need[2])) if ops else []
            gbias = torch.autograd.grad(out, leaves[2], g)[0] if need[2] else None
        ga = got.pop(0) if need[0] else None
        gb = got.pop(0) if need[1] else None
        return None, None, ga, gb, gbias


def folded_mha(p, pre, q, k, heads):
    """oracle/ref_model.mha in the association the MFMA kernels compute
    (t2omca_amd/csrc/t2o_pack.hip:5-9): per head M_h = Wk_hᵀ Wq_h / √E and
    N_h = U_h Wv_h are folded from the fp32 parameters, scores = (M_h x) · key,
    z_h = Σ_j p_j key_j over the RAW keys, attended = Σ_h N_h z_h + b_U.  The same
    bilinear forms as mha, but what a bf16 product rounds is M_h and N_h (their bf16
    images, t2o_pack.hip:114-115 and 129-130), M_h x (t2o_mixer_block.hpp:258) and
    z_h, not Wq / Wk / Wv / U and the projected queries, keys and values.  The fold
    itself (einsum) is no rounded product: the pack kernel folds in fp32."""
    b, t_q, e = q.shape
    wq, wk, wv = (p[pre + n + ".weight"].view(heads, e, e) for n in ("toqueries", "tokeys", "tovalues"))
    u = p[pre + "unifyheads.weight"].view(e, heads, e)
    m_fold = torch.einsum("hmi,hmk->hik", wk, wq) / e ** 0.5      # M[h, i, k]
    n_fold = torch.einsum("ohm,hmk->ohk", u, wv).reshape(e, heads * e)  # N[o, h·E + k]
    mx = torch.matmul(q[:, None], m_fold.transpose(-1, -2)[None])  # [b, h, t_q, e]
    prob = F.softmax(torch.matmul(mx, k[:, None].transpose(-1, -2)), dim=-1)
    z = torch.matmul(prob, k[:, None])                            # [b, h, t_q, e]
    z = z.transpose(1, 2).reshape(b, t_q, heads * e)
    return F.linear(z, n_fold, p[pre + "unifyheads.bias"])


class Bf16Operands(TorchFunctionMode):
    """Inside this mode F.linear, torch.bmm and torch.matmul run with both operands
    rounded to bf16 (forward and backward); rounding=False swaps the same calls but
    rounds nothing, which must reproduce plain autograd bit for bit.  `calls` counts
    the swapped calls.  fold=True also evaluates the attention as the kernels do, with
    folded projection weights (folded_mha, installed as oracle.ref_model.mha while the
    mode is entered): the extra rounding sites are the folded matrices' bf16 images."""

    def __init__(self, rounding=True, fold=False):
        super().__init__()
        self.rnd = round_bf16 if rounding else (lambda x: x)
        self.calls = 0
        self.fold, self._mha = fold, None

    def __enter__(self):
        if self.fold:
            from oracle import ref_model
            self._mha, ref_model.mha = ref_model.mha, folded_mha
        return super().__enter__()

    def __exit__(self, *exc):
        if self.fold:
            from oracle import ref_model
            ref_model.mha = self._mha
        return super().__exit__(*exc)

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is F.linear or func is torch.bmm or func is torch.matmul:
            args = list(args) + ([kwargs.pop("bias")] if "bias" in kwargs else [])
            assert not kwargs and 2 <= len(args) <= 3, (func, kwargs)
            self.calls += 1
            return _RoundedOperands.apply(func, self.rnd, args[0], args[1], args[2] if len(args) > 2 else None)
        return func(*args, **kwargs)


def oracle_grad(pa, pm, cfg, batch, w, *, pa_tgt=None, pm_tgt=None, mode=None, dtype=torch.float64, **kw):
    """(flat gradient, loss, priorities, extras) of oracle/ref_learner.td_forward (looked
    up when called) in `dtype`, inside `mode` if one is given (forward and backward)."""
    import contextlib

    from oracle import ref_learner

    def cast(d):
        return {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in d.items()}

    pa, pm = cast(pa), cast(pm)
    pat, pmt = (pa if pa_tgt is None else cast(pa_tgt)), (pm if pm_tgt is None else cast(pm_tgt))
    pa_g = {k: v.clone().requires_grad_(True) for k, v in pa.items()}
    pm_g = {k: v.clone().requires_grad_(True) for k, v in pm.items()}
    with (mode if mode is not None else contextlib.nullcontext()):
        loss, prio, ex = ref_learner.td_forward(pa_g, pm_g, pat, pmt, cast(batch), cfg,
                                                per_weight=w.detach().cpu().to(dtype), **kw)
        gs = torch.autograd.grad(loss, list(pa_g.values()) + list(pm_g.values()))
    return torch.cat([g.reshape(-1) for g in gs]), loss.detach(), prio.detach(), ex


def emulated_bf16_grad(pa, pm, cfg, batch, w, **kw):
    """The fp64 oracle's flat gradient with bf16 matmul operands and the attention in
    the kernels' folded association (Bf16Operands(fold=True))."""
    mode = Bf16Operands(fold=True)
    g = oracle_grad(pa, pm, cfg, batch, w, mode=mode, **kw)[0]
    assert mode.calls > 0
    return g
