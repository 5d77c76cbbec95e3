"""GPU: WHERE the kernels read and write (the memory contract of include/t2omca.h).

The rest of the suite checks what every kernel computes; here every entry point is
called straight through the C ABI (argument structs of t2omca_amd/_lib.py, no ops.*
wrapper, so the test owns every buffer) twice:

  dense run   ordinary contiguous tensors; the unrolls' forward outputs are held
              against the fp64 oracle (oracle/ref_model.agent_unroll / mixer_unroll)
              at the project's bars (normwise 1e-5 fp32, 2e-2 bf16), so "equal to the
              dense run" cannot mean "equally wrong";
  arena run   every input that has strides in the ABI is a strided view, and every
              output and workspace has EXACTLY the size the header states, all carved
              from one poisoned allocation with guard bands (tests/arena.py: NaN /
              -1 between the rows of a view, past its last step, around every tensor).

Asserted: every return code 0; every output of the arena run finite and torch.equal
to the dense run's (the same kernel on the same values at other addresses gives the
same bits; the one documented exception is t2o_td_loss's loss scalar, summed with
float atomics: rtol 1e-6, Σ mask exact); arena.check() after each launch and after
the synchronise (no byte outside a tensor's logical elements changed).

Input layouts (`_LAYOUTS`; a case's inputs take different ones, rotated by the case's
position in `SHAPES`, so every strided input of every family sees each of them):
  tm       time-major storage viewed [B, T, ...] (sb < st), as runner.py produces;
  slice    a [:, :T] slice of a buffer two steps longer (sb > T·st), the steps past T
           poisoned: a used read of step t + 1 past the end turns an output NaN;
  padded   a padded step stride and a padded episode stride at once;
plus q_ts > T for the mixer's Q arrays, h_ts > T for the BPTT's h_seq / hmid (steps
>= T poisoned), actions as [B, T, A, 1] int64 storage viewed [B, T, A], avail as
int32 with padded strides.

Shapes: the default network (emb 32, 3 heads, depth 2, ff x 4) at the smallest
(A, B, T) that reach each instance class and a partial 16-row tile (`SHAPES`), fp32
and bf16, plus one forced-generic case; the instance class is asserted per case.  The
generic BPTT sums with float atomics in an order that varies run to run, dense or not:
its summed outputs are compared at REORDER_BAR (see there), everything else bit for bit.
"""
import ctypes
import functools

import pytest
import torch

from oracle import ref_model
from tests.arena import Arena
from tests.gpu_util import flat_from_dict, normwise, require_gpu

pytestmark = pytest.mark.gpu

E, H, D, FF, NA, FO, FS = 32, 3, 2, 128, 5, 9, 8
EXACT, RUNTIME, GENERIC = 0, 1, 2
# (A, B, T, agent instance, mixer instance): tests' docstrings say what each reaches
SHAPES = [(5, 3, 4, RUNTIME, RUNTIME), (8, 3, 5, EXACT, EXACT), (13, 3, 4, RUNTIME, RUNTIME),
          (16, 3, 4, EXACT, EXACT), (20, 2, 4, RUNTIME, RUNTIME), (64, 2, 3, EXACT, EXACT)]
CASES = [pytest.param(i, prec, False, id=f"A{s[0]}-{'bf16' if prec else 'fp32'}")
         for i, s in enumerate(SHAPES) for prec in (0, 1)] + [pytest.param(0, 0, True, id="A5-generic")]
BAR = {0: 1e-5, 1: 2e-2}
_LAYOUTS = ("tm", "slice", "padded")
T2O_EINVAL = -1  # include/t2omca.h


def _cfg(A):
    return dict(n_agents=A, n_entities=A, obs_entity_feats=FO, emb=E, heads=H, depth=D, ff_hidden_mult=4,
                n_actions=NA, state_entity_feats=FS, mixer_emb=E, mixer_heads=H, mixer_depth=D)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- the two memory providers ---------------------------------------------------

class Dense:
    """Ordinary contiguous device tensors."""
    arena = None

    def inp(self, name, src, how=None, valid=None):
        return src.cuda().contiguous()

    def out(self, name, shape, dtype=torch.float32):
        return torch.empty(tuple(int(s) for s in shape), dtype=dtype, device="cuda")

    def check(self, what):
        pass


class Carved:
    """Tensors carved from one poisoned arena: strided inputs, exact-size outputs."""

    def __init__(self, nbytes):
        self.arena = Arena(nbytes, "cuda")

    def inp(self, name, src, how=None, valid=None):
        """how: None dense, or a layout of `_LAYOUTS` over the two leading axes of src
        [B, T, ...].  valid: only steps [:, :valid] are copied, the rest keep the poison."""
        src = src.cuda()
        if how is None:
            t = self.arena.carve(src.shape, src.dtype, name=name)
        else:
            B, T = src.shape[:2]
            row = 1
            for n in src.shape[2:]:
                row *= n
            flt = src.dtype.is_floating_point
            pad = 4 if flt else 3
            if how == "tm":
                sb, st = row, B * row
            elif how == "slice":
                sb, st = (T + 2) * row, row
            else:
                st = (row + 3) // 4 * 4 + pad if flt else row + pad
                sb = (T + 1) * st + 2 * pad
            inner, n = [], 1
            for s in reversed(src.shape[2:]):
                inner.append(n)
                n *= s
            # rows the kernels load 4 floats at a time (hidden states) keep 16-byte alignment;
            # obs at an odd entity count has rows of 9·A·A floats, read element-wise
            mult = 4 if flt and row % 4 == 0 else 1
            t = self.arena.carve_view(src.shape, src.dtype, (sb, st) + tuple(reversed(inner)), name=name,
                                      stride_multiple=mult)
        if valid is None:
            t.copy_(src)
        else:
            t[:, :valid].copy_(src[:, :valid])
        return t

    def out(self, name, shape, dtype=torch.float32):
        return self.arena.carve(shape, dtype, name=name)

    def check(self, what):
        self.arena.check(what)


def _both(run, nbytes=64 << 20):
    """run(mem) -> dict of outputs, on dense tensors and on the arena; returns both."""
    dense = run(Dense())
    torch.cuda.synchronize()
    mem = Carved(nbytes)
    carved = run(mem)
    torch.cuda.synchronize()
    mem.check("after the synchronise")
    return dense, carved


# The runtime-shaped (generic) BPTT kernels add their gradients with float atomics — the
# vector / embedding / head gradients once per wave into the slab, the mixer's key-token
# gradients into LDS rows its waves share (t2o_generic.hip) — so those outputs are the same
# terms summed in an order that varies run to run, dense or not.  They are held to the
# project's bar for "same terms, other order" (tests/test_gpu_fullgrid.py GRAD_SUM_BAR: 1e-6
# normwise; fp32 sums of a few thousand O(1) terms differ by ~sqrt(n)·2^-24 ≈ 4e-6 of ONE
# term, far less of the tensor's largest element).  The tuned kernels flush in wave order
#  and stay bit-exact.
REORDER_BAR = 1e-6


def _assert_same(dense, carved, loose=(), reordered=()):
    assert dense.keys() == carved.keys()
    for k, v in dense.items():
        if v is None:
            assert carved[k] is None
            continue
        assert torch.isfinite(carved[k].double()).all(), f"{k}: the arena run left or produced a non-finite value"
        if k in loose:
            assert torch.allclose(carved[k], v, rtol=1e-6, atol=0.0), k
        elif any(k.endswith(r) for r in reordered):
            assert normwise(carved[k], v) < REORDER_BAR, (k, normwise(carved[k], v))
        else:
            assert torch.equal(carved[k], v), (k, int((carved[k] != v).sum()), "elements differ from the dense run")


def _lay(i, k):
    return _LAYOUTS[(i + k) % 3]


# ---- layouts, parameters, packs ---------------------------------------------------

def _layout(kind, A, prec, generic):
    from t2omca_amd import _lib
    F, na = (FO, NA) if kind == 0 else (FS, 1)
    return _lib.make_layout(kind, E, H, D, F, na, FF, A, prec, flags=_lib.LAYOUT_FORCE_GENERIC if generic else 0)


def _instance(L, want):
    from t2omca_amd import _lib
    got = _lib.lib().t2o_layout_instance(ctypes.byref(L))
    assert got == want, f"layout instance {got}, this case is meant to run {want} (0 exact, 1 runtime, 2 generic)"


@functools.lru_cache(maxsize=None)
def _params(kind, A, seed):
    return ref_model.init_params("agent" if kind == 0 else "mixer", _cfg(A), seed)


def _pack(mem, L, p, name):
    """t2o_pack_params into a buffer of exactly pack_floats floats."""
    from t2omca_amd import _lib
    params = mem.inp(name + ".params", flat_from_dict(p))
    pack = mem.out(name + ".pack", (L.pack_floats,))
    assert _lib.lib().t2o_pack_params(ctypes.byref(L), _vp(params), _vp(pack), _stream()) == 0
    mem.check("t2o_pack_params " + name)
    return params, pack


def _contract(mem, pend, tag, out):
    """t2o_bwd_tape_contract (one tape), t2o_reduce_slabs, t2o_unpack_grads."""
    from t2omca_amd import _lib
    lib = _lib.lib()
    ta = _lib.TapeArgs(L=ctypes.pointer(pend["L"]), pack=_ptr(pend["pack"]), tape=_ptr(pend["tape"]),
                       tiles=pend["tiles"], gslabs=_ptr(pend["slabs"]), nslab=pend["nslab"], rec_format=pend["fmt"])
    assert lib.t2o_bwd_tape_contract(ctypes.byref(ta), None, _stream()) == 0
    mem.check("t2o_bwd_tape_contract " + tag)
    _reduce_unpack(mem, pend, tag, out)


def _reduce_unpack(mem, pend, tag, out):
    from t2omca_amd import _lib
    lib = _lib.lib()
    L = pend["L"]
    gpack = mem.out(tag + ".gpack", (L.grad_total,))
    assert lib.t2o_reduce_slabs(_vp(pend["slabs"]), pend["nslab"], L.grad_total, _vp(gpack), _stream()) == 0
    mem.check("t2o_reduce_slabs " + tag)
    grad = mem.out(tag + ".grad", (pend["params"].numel(),))
    grad.zero_()  # (t2o_unpack_grads accumulates)
    assert lib.t2o_unpack_grads(ctypes.byref(L), _vp(pend["params"]), _vp(gpack), _vp(grad), _stream()) == 0
    mem.check("t2o_unpack_grads " + tag)
    out[tag + ".gpack"], out[tag + ".grad"] = gpack, grad


# ---- the agent -----------------------------------------------------------------------

def _agent_inputs(A, B, T1, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(obs=torch.randn(B, T1, A, A * FO, generator=g), h0_on=0.5 * torch.randn(B, A, E, generator=g),
                h0_tg=0.5 * torch.randn(B, A, E, generator=g))


def _agent_fwd(mem, i, prec, generic, two_nets=True, k_split=None, steps=None):
    """Online + target network with hmid_on and nonzero h0; whole, then (k_split) in the
    step ranges (0, k), (k, T) into a second set of outputs.  steps: T, if not the case's."""
    from t2omca_amd import _lib
    lib = _lib.lib()
    A, B, T = SHAPES[i][:3]
    T = steps or T
    L = _layout(0, A, prec, generic)
    _instance(L, GENERIC if generic else SHAPES[i][3])
    x = _agent_inputs(A, B, T, 100 + A)
    _, pack_on = _pack(mem, L, _params(0, A, 11), "agent_on")
    pack_tg = _pack(mem, L, _params(0, A, 12), "agent_tg")[1] if two_nets else None
    obs = mem.inp("obs", x["obs"], _lay(i, 0))
    h0_on, h0_tg = mem.inp("h0_on", x["h0_on"]), mem.inp("h0_tg", x["h0_tg"]) if two_nets else None
    out = {}
    for tag, ranges in (("", [(0, T)]),) + ((("r.", [(0, k_split), (k_split, T)]),) if k_split else ()):
        o = dict(q_on=mem.out(tag + "q_on", (B, T, A, NA)), h_on=mem.out(tag + "h_on", (B, T, A, E)),
                 hmid_on=mem.out(tag + "hmid_on", (B, T, D - 1, A, E)))
        if two_nets:
            o.update(q_tg=mem.out(tag + "q_tg", (B, T, A, NA)), h_tg=mem.out(tag + "h_tg", (B, T, A, E)))
        a = _lib.AgentFwdArgs(L=ctypes.pointer(L), pack_on=_ptr(pack_on), pack_tg=_ptr(pack_tg), obs=_ptr(obs),
                              obs_sb=obs.stride(0), obs_st=obs.stride(1), h0_on=_ptr(h0_on), h0_tg=_ptr(h0_tg),
                              q_on=_ptr(o["q_on"]), h_on=_ptr(o["h_on"]), hmid_on=_ptr(o["hmid_on"]),
                              q_tg=_ptr(o.get("q_tg")), h_tg=_ptr(o.get("h_tg")), B=B, T=T, A=A)
        for t0, t1 in ranges:
            a.t0, a.t1 = t0, t1
            assert lib.t2o_agent_unroll_fwd(ctypes.byref(a), _stream()) == 0
            mem.check(f"t2o_agent_unroll_fwd steps [{t0}, {t1})")
        out.update({tag + k: v for k, v in o.items()})
    return out


@pytest.mark.parametrize("i,prec,generic", CASES)
def test_agent_unroll_fwd(i, prec, generic):
    """t2o_agent_unroll_fwd (and t2o_pack_params into pack_floats floats): two networks,
    hmid_on, nonzero h0; whole and in two step ranges.  Instances: runtime capacity 8
    (A 5, 15 rows: a partial tile), exact (8: 1.5 tiles; 16), runtime 16 (13), chunked
    (20 runtime, 64 exact), generic.  obs saw tm / slice / padded (rotated over the
    shapes); the dense q / h are held against the fp64 oracle."""
    require_gpu()
    A, B, T = SHAPES[i][:3]
    # (the generic kernels take the whole unroll only: a step range is T2O_EUNSUPPORTED)
    dense, carved = _both(lambda mem: _agent_fwd(mem, i, prec, generic, k_split=None if generic else T // 2))
    x = _agent_inputs(A, B, T, 100 + A)
    for net, seed in (("on", 11), ("tg", 12)):
        p64 = {k: v.double() for k, v in _params(0, A, seed).items()}
        q, h = ref_model.agent_unroll(p64, x["obs"].double(), x["h0_" + net].double(), cfg=_cfg(A))
        for tag in ("",) if generic else ("", "r."):
            errs = normwise(dense[tag + "q_" + net], q), normwise(dense[tag + "h_" + net], h)
            assert max(errs) < BAR[0 if generic else prec], (net, tag, errs)
    _assert_same(dense, carved)


def _agent_bwd(mem, i, prec, generic, fwd, has_hmid, ranges, out, tag):
    """One BPTT over T of the T + 1 forward steps (h_ts = T + 1, the last step poisoned on
    the arena) from gchosen + actions + gh, gh0 wanted; returns the pending contraction."""
    from t2omca_amd import _lib
    lib = _lib.lib()
    A, B, T = SHAPES[i][:3]
    T1 = T + 1
    L = _layout(0, A, prec, generic)
    x = _agent_inputs(A, B, T1, 100 + A)
    g = torch.Generator().manual_seed(200 + A)
    gchosen = mem.inp("gchosen", torch.randn(B, T, A, generator=g))
    gh = mem.inp("gh", 0.1 * torch.randn(B, T, A, E, generator=g))
    actions = mem.inp("actions", torch.randint(0, NA, (B, T1, A, 1), generator=g), _lay(i, 1), valid=T)[..., 0]
    params, pack = _pack(mem, L, _params(0, A, 11), tag + "agent")
    obs = mem.inp("obs", x["obs"], _lay(i, 2), valid=T)
    h0 = mem.inp("h0", x["h0_on"])
    h_seq = mem.inp("h_seq", fwd["h_on"], None, valid=T)
    hmid = mem.inp("hmid", fwd["hmid_on"], None, valid=T) if has_hmid else None
    tiles = lib.t2o_bwd_tape_tiles(ctypes.byref(L), B, T, A)
    assert tiles == T * ((B * A + 15) // 16) or generic
    nmax = lib.t2o_agent_bwd_max_slabs(B, A)
    tape = mem.out(tag + "tape", (lib.t2o_bwd_tape_floats(ctypes.byref(L), tiles),))
    slabs = mem.out(tag + "slabs", (nmax * L.grad_total,))
    gh0 = mem.out(tag + "gh0", (B, A, E))
    gcarry = mem.out(tag + "gcarry", (B * A, E)) if len(ranges) > 1 else None
    nslab = ctypes.c_int32(0)
    a = _lib.AgentBwdArgs(L=ctypes.pointer(L), pack=_ptr(pack), obs=_ptr(obs), obs_sb=obs.stride(0),
                          obs_st=obs.stride(1), h0=_ptr(h0), h_seq=_ptr(h_seq), hmid=_ptr(hmid), h_ts=T1,
                          gchosen=_ptr(gchosen), actions=_ptr(actions), act_sb=actions.stride(0),
                          act_st=actions.stride(1), gh=_ptr(gh), gslabs=_ptr(slabs), max_slabs=nmax,
                          nslab=ctypes.pointer(nslab), tape=_ptr(tape), gh0=_ptr(gh0), gcarry=_ptr(gcarry), B=B, T=T,
                          A=A)
    for t_lo, t_hi in ranges:
        a.t_lo, a.t_hi = t_lo, t_hi
        assert lib.t2o_agent_unroll_bwd(ctypes.byref(a), _stream()) == 0
        mem.check(f"t2o_agent_unroll_bwd {tag} steps [{t_lo}, {t_hi})")
        assert 1 <= nslab.value <= nmax
    out[tag + "gh0"] = gh0
    return dict(L=L, pack=pack, tape=tape, tiles=tiles, slabs=slabs, nslab=nslab.value, params=params,
                fmt=lib.t2o_agent_bwd_tape_format(ctypes.byref(L), int(has_hmid)))


@functools.lru_cache(maxsize=None)
def _agent_fwd_dense(i, prec, generic):
    """The forward a BPTT case differentiates: T + 1 steps of one network, dense (kept on the host)."""
    o = _agent_fwd(Dense(), i, prec, generic, two_nets=False, steps=SHAPES[i][2] + 1)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize("i,prec,generic", CASES)
def test_agent_unroll_bwd_and_contraction(i, prec, generic):
    """t2o_agent_unroll_bwd, then t2o_bwd_tape_contract, t2o_reduce_slabs, t2o_unpack_grads:
    gchosen + actions + gh with gh0 wanted; with hmid and without; whole, and (where
    t2o_agent_bwd_ranges says 1) in two step ranges with gcarry.  The tape has
    t2o_bwd_tape_floats(t2o_bwd_tape_tiles) floats, the slabs t2o_agent_bwd_max_slabs x
    grad_total; bf16 at <= 8 entities writes the lean record (t2o_agent_bwd_tape_format).
    obs and the [B, T, A, 1] int64 actions saw tm / slice / padded; h_ts = T + 1 > T with
    step T of h_seq / hmid poisoned."""
    require_gpu()
    from t2omca_amd import _lib
    lib = _lib.lib()
    A, B, T = SHAPES[i][:3]
    L = _layout(0, A, prec, generic)
    fwd = _agent_fwd_dense(i, prec, generic)
    if prec == 1 and A == 8 and not generic:
        assert lib.t2o_agent_bwd_tape_format(ctypes.byref(L), 1) == 1  # the lean record
    k = T // 2

    def run(mem):
        out = {}
        for has_hmid in (True, False):
            tag = "hmid." if has_hmid else "nohmid."
            _contract(mem, _agent_bwd(mem, i, prec, generic, fwd, has_hmid, [(0, T)], out, tag), tag + "agent", out)
            if lib.t2o_agent_bwd_ranges(ctypes.byref(L), int(has_hmid)) == 1:
                tag += "r."
                pend = _agent_bwd(mem, i, prec, generic, fwd, has_hmid, [(k, T), (0, k)], out, tag)
                _contract(mem, pend, tag + "agent", out)
        return out

    dense, carved = _both(run)
    if not generic and A in (8, 16):
        assert any(key.startswith("hmid.r.") for key in dense), "the pipelined BPTT no longer takes step ranges here"
    _assert_same(dense, carved, reordered=(".gpack", ".grad") if generic else ())


# ---- the mixer -----------------------------------------------------------------------

def _mixer_inputs(A, B, T1, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(states=torch.randn(B, T1, A * FS, generator=g), hid_on=torch.randn(B, T1, A, E, generator=g),
                hid_tg=torch.randn(B, T1, A, E, generator=g), hw0_on=0.5 * torch.randn(B, 3, E, generator=g),
                hw0_tg=0.5 * torch.randn(B, 3, E, generator=g), q_on=torch.randn(B, T1, A, NA, generator=g),
                q_tg=torch.randn(B, T1, A, NA, generator=g), actions=torch.randint(0, NA, (B, T1, A, 1), generator=g),
                avail=_avail(B, T1, A, g), qv=torch.randn(B, T1, A, generator=g))


def _avail(B, T1, A, g):
    av = (torch.rand(B, T1, A, NA, generator=g) < 0.5).to(torch.int32)
    av[..., 0] = 1
    return av


def _mixer_fwd(mem, i, prec, generic):
    """Online (qmode 1: chosen-action gather, T steps) + target (qmode 2: double-Q with
    avail, T + 1 steps) in one launch, q_ts = T + 3; where t2o_mixer_split is 1 also in the
    decoupled phases (1 over two step ranges, then 2) into a second set of outputs."""
    from t2omca_amd import _lib
    lib = _lib.lib()
    A, B, T = SHAPES[i][:3]
    T1, q_ts = T + 1, T + 3
    L = _layout(1, A, prec, generic)
    _instance(L, GENERIC if generic else SHAPES[i][4])
    x = _mixer_inputs(A, B, T1, 300 + A)
    _, pack_on = _pack(mem, L, _params(1, A, 21), "mixer_on")
    _, pack_tg = _pack(mem, L, _params(1, A, 22), "mixer_tg")
    states = mem.inp("states", x["states"], _lay(i, 0))
    # (one pair of strides serves both networks' hidden states; the online network runs T
    # of the T + 1 steps, its last step stays poisoned on the arena)
    hid_on = mem.inp("hid_on", x["hid_on"], _lay(i, 1), valid=T)
    hid_tg = mem.inp("hid_tg", x["hid_tg"], _lay(i, 1))
    assert hid_on.stride() == hid_tg.stride()
    hw0_on, hw0_tg = mem.inp("hw0_on", x["hw0_on"]), mem.inp("hw0_tg", x["hw0_tg"])

    def q_array(name):  # [B, q_ts, A, NA], steps >= T + 1 poisoned on the arena
        pad = torch.zeros(B, q_ts, A, NA)
        pad[:, :T1] = x[name]
        return mem.inp(name, pad, None, valid=T1)
    q_on, q_tg = q_array("q_on"), q_array("q_tg")
    actions = mem.inp("actions", x["actions"], _lay(i, 2), valid=T)[..., 0]
    avail = mem.inp("avail", x["avail"], "padded")
    split = lib.t2o_mixer_split(ctypes.byref(L), B) == 1
    out = {}
    phases = (("ph.", [(1, 0, T1 // 2), (1, T1 // 2, T1), (2, 0, 0)]),) if split else ()
    for tag, calls in (("", [(0, 0, 0)]),) + phases:
        o = {}
        for n, Tn in (("on", T), ("tg", T1)):
            o.update({f"y_{n}": mem.out(f"{tag}y_{n}", (B, Tn)), f"hw_{n}": mem.out(f"{tag}hw_{n}", (B, Tn, 3, E)),
                      f"qvo_{n}": mem.out(f"{tag}qvo_{n}", (B, Tn, A)),
                      f"xout_{n}": mem.out(f"{tag}xout_{n}", (B, Tn, A + 3, E))})
        o["xmid_on"] = mem.out(tag + "xmid_on", (B, T, D - 1, A + 3, E))
        a = _lib.MixerFwdArgs(L=ctypes.pointer(L), pack_on=_ptr(pack_on), pack_tg=_ptr(pack_tg), states=_ptr(states),
                              st_sb=states.stride(0), st_st=states.stride(1), hid_on=_ptr(hid_on),
                              hid_tg=_ptr(hid_tg), hid_sb=hid_on.stride(0), hid_st=hid_on.stride(1),
                              hw0_on=_ptr(hw0_on), hw0_tg=_ptr(hw0_tg), qmode_on=1, qmode_tg=2, q_on=_ptr(q_on),
                              q_tg=_ptr(q_tg), q_ts=q_ts, n_actions=NA, actions=_ptr(actions),
                              act_sb=actions.stride(0), act_st=actions.stride(1), avail=_ptr(avail),
                              av_sb=avail.stride(0), av_st=avail.stride(1), B=B, T_on=T, T_tg=T1,
                              **{k: _ptr(v) for k, v in o.items()})
        for phase, t0, t1 in calls:
            a.phase, a.t0, a.t1 = phase, t0, t1
            assert lib.t2o_mixer_unroll_fwd(ctypes.byref(a), _stream()) == 0
            mem.check(f"t2o_mixer_unroll_fwd phase {phase} steps [{t0}, {t1})")
        out.update({tag + k: v for k, v in o.items()})
    return out


@pytest.mark.parametrize("i,prec,generic", CASES)
def test_mixer_unroll_fwd(i, prec, generic):
    """t2o_mixer_unroll_fwd: online qmode 1 + target qmode 2 with actions and avail in one
    launch (T and T + 1 steps), xout / xmid kept; where t2o_mixer_split is 1 (the multi-tile
    mixers at these batches: 16 agents with 19 query rows, 20, 64) also phases 1 (two step
    ranges) and 2.  Instances: one tile (A 5 partial,
    8 exact, 13 full), multi-tile (16, 20 in capacity 32, 64 five tiles), generic.
    states, hid_on / hid_tg and the [B, T, A, 1] int64 actions saw tm / slice / padded,
    avail int32 padded strides, q_ts = T + 3 with the Q arrays' tail poisoned, hid_on's
    unused step T poisoned; the dense y / hw are held against the fp64 oracle, qvo is exact."""
    require_gpu()
    from t2omca_amd import _lib
    A, B, T = SHAPES[i][:3]
    T1 = T + 1
    dense, carved = _both(lambda mem: _mixer_fwd(mem, i, prec, generic))
    if A == 16 and not generic:
        assert "ph.y_on" in dense, "the 16-agent mixer no longer runs decoupled at this batch"
    x = _mixer_inputs(A, B, T1, 300 + A)
    qv_on = x["q_on"].gather(3, x["actions"]).squeeze(3)[:, :T]
    best = x["q_on"].masked_fill(x["avail"] == 0, -9999999.0).argmax(3, keepdim=True)
    qv_tg = x["q_tg"].gather(3, best).squeeze(3)
    for n, qv, Tn, seed in (("on", qv_on, T, 21), ("tg", qv_tg, T1, 22)):
        p64 = {k: v.double() for k, v in _params(1, A, seed).items()}
        y, hw = ref_model.mixer_unroll(p64, qv.double(), x["hid_" + n][:, :Tn].double(), x["states"][:, :Tn].double(),
                                       x["hw0_" + n].double(), cfg=_cfg(A))
        for tag in ("", "ph.") if "ph.y_on" in dense else ("",):
            assert torch.equal(dense[f"{tag}qvo_{n}"].cpu(), qv), (n, tag)
            errs = normwise(dense[f"{tag}y_{n}"], y), normwise(dense[f"{tag}hw_{n}"], hw)
            assert max(errs) < BAR[0 if generic else prec], (n, tag, errs)
    _assert_same(dense, carved)


@functools.lru_cache(maxsize=None)
def _mixer_fwd_dense(i, prec, generic):
    """The forward a mixer BPTT case differentiates: one network on given qvals, T steps."""
    from t2omca_amd import _lib
    lib = _lib.lib()
    A, B, T = SHAPES[i][:3]
    L = _layout(1, A, prec, generic)
    mem = Dense()
    x = _mixer_inputs(A, B, T + 1, 300 + A)
    _, pack = _pack(mem, L, _params(1, A, 21), "mixer")
    st, hid, qv = (x[k][:, :T].contiguous().cuda() for k in ("states", "hid_on", "qv"))
    hw0 = x["hw0_on"].cuda()
    o = dict(y=mem.out("y", (B, T)), hw=mem.out("hw", (B, T, 3, E)), qvo=mem.out("qvo", (B, T, A)),
             xout=mem.out("xout", (B, T, A + 3, E)), xmid=mem.out("xmid", (B, T, D - 1, A + 3, E)))
    a = _lib.MixerFwdArgs(L=ctypes.pointer(L), pack_on=_ptr(pack), states=_ptr(st), st_sb=st.stride(0),
                          st_st=st.stride(1), hid_on=_ptr(hid), hid_sb=hid.stride(0), hid_st=hid.stride(1),
                          hw0_on=_ptr(hw0), qmode_on=0, qv_on=_ptr(qv), y_on=_ptr(o["y"]), hw_on=_ptr(o["hw"]),
                          qvo_on=_ptr(o["qvo"]), xout_on=_ptr(o["xout"]), xmid_on=_ptr(o["xmid"]), B=B, T_on=T)
    assert lib.t2o_mixer_unroll_fwd(ctypes.byref(a), _stream()) == 0
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _mixer_bwd(mem, i, prec, generic, fwd, calls, out, tag):
    """One mixer BPTT (calls: (phase, t_lo, t_hi) in order) from gy and an extra dL/dhw,
    ghw0 wanted; the workspace has t2o_mixer_bwd_work_floats floats where the mixer runs
    decoupled (else NULL).  Returns the pending contraction."""
    from t2omca_amd import _lib
    lib = _lib.lib()
    A, B, T = SHAPES[i][:3]
    L = _layout(1, A, prec, generic)
    x = _mixer_inputs(A, B, T + 1, 300 + A)
    g = torch.Generator().manual_seed(400 + A)
    gy = mem.inp("gy", torch.randn(B, T, generator=g))
    ghw_ext = mem.inp("ghw_ext", 0.1 * torch.randn(B, T, 3, E, generator=g))
    params, pack = _pack(mem, L, _params(1, A, 21), tag + "mixer")
    states = mem.inp("states", x["states"], _lay(i, 1), valid=T)
    hid = mem.inp("hid", x["hid_on"], _lay(i, 2), valid=T)
    hw0 = mem.inp("hw0", x["hw0_on"])
    qv, hw, xout, xmid = (mem.inp(k, fwd[k]) for k in ("qvo", "hw", "xout", "xmid"))
    tiles = lib.t2o_bwd_tape_tiles(ctypes.byref(L), B, T, A)
    assert tiles > 0
    nmax = lib.t2o_mixer_bwd_max_slabs(B)
    tape = mem.out(tag + "tape", (lib.t2o_bwd_tape_floats(ctypes.byref(L), tiles),))
    slabs = mem.out(tag + "slabs", (nmax * L.grad_total,))
    split = lib.t2o_mixer_split(ctypes.byref(L), B) == 1
    nwork = lib.t2o_mixer_bwd_work_floats(ctypes.byref(L), B, T) if split else 0
    assert nwork >= 0 and (nwork > 0 or not split)
    work = mem.out(tag + "work", (nwork,)) if nwork else None
    carry = mem.out(tag + "ghw_carry", (B, 3, E)) if len(calls) > 1 else None
    o = dict(gqv=mem.out(tag + "gqv", (B, T, A)), ghid=mem.out(tag + "ghid", (B, T, A, E)),
             ghw0=mem.out(tag + "ghw0", (B, 3, E)))
    nslab = ctypes.c_int32(0)
    a = _lib.MixerBwdArgs(L=ctypes.pointer(L), pack=_ptr(pack), states=_ptr(states), st_sb=states.stride(0),
                          st_st=states.stride(1), hid=_ptr(hid), hid_sb=hid.stride(0), hid_st=hid.stride(1),
                          hw0=_ptr(hw0), qv=_ptr(qv), hw=_ptr(hw), xout=_ptr(xout), xmid=_ptr(xmid), gy=_ptr(gy),
                          ghw_ext=_ptr(ghw_ext), gslabs=_ptr(slabs), max_slabs=nmax, nslab=ctypes.pointer(nslab),
                          tape=_ptr(tape), work=_ptr(work), work_floats=nwork, ghw_carry=_ptr(carry), B=B, T=T,
                          **{k: _ptr(v) for k, v in o.items()})
    for phase, t_lo, t_hi in calls:
        a.phase, a.t_lo, a.t_hi = phase, t_lo, t_hi
        assert lib.t2o_mixer_unroll_bwd(ctypes.byref(a), _stream()) == 0
        mem.check(f"t2o_mixer_unroll_bwd {tag} phase {phase} steps [{t_lo}, {t_hi})")
        assert 1 <= nslab.value <= nmax
    out.update({tag + k: v for k, v in o.items()})
    return dict(L=L, pack=pack, tape=tape, tiles=tiles, slabs=slabs, nslab=nslab.value, params=params, fmt=0)


@pytest.mark.parametrize("i,prec,generic", CASES)
def test_mixer_unroll_bwd_and_contraction(i, prec, generic):
    """t2o_mixer_unroll_bwd phase 0, and where t2o_mixer_split is 1 (16, 20 and 64 agents
    at these batches) also the decoupled phases — 1, then 2 over two step ranges with ghw_carry — with
    `work` of t2o_mixer_bwd_work_floats floats; then t2o_bwd_tape_contract, t2o_reduce_slabs,
    t2o_unpack_grads.  Tape of t2o_bwd_tape_floats(t2o_bwd_tape_tiles) floats (the compact
    stream of a multi-tile mixer), slabs of t2o_mixer_bwd_max_slabs x grad_total.  states
    and hid saw tm / slice / padded, step T of both poisoned."""
    require_gpu()
    from t2omca_amd import _lib
    lib = _lib.lib()
    A, B, T = SHAPES[i][:3]
    L = _layout(1, A, prec, generic)
    fwd = _mixer_fwd_dense(i, prec, generic)
    split = lib.t2o_mixer_split(ctypes.byref(L), B) == 1
    assert split or A != 16 or generic, "the 16-agent mixer no longer runs decoupled at this batch"
    k = T // 2

    def run(mem):
        out = {}
        _contract(mem, _mixer_bwd(mem, i, prec, generic, fwd, [(0, 0, 0)], out, ""), "mixer", out)
        if split:
            pend = _mixer_bwd(mem, i, prec, generic, fwd, [(1, 0, 0), (2, k, T), (2, 0, k)], out, "ph.")
            _contract(mem, pend, "ph.mixer", out)
        return out

    nmax = lib.t2o_mixer_bwd_max_slabs(B)
    dense, carved = _both(run, nbytes=(64 << 20) + 2 * 4 * nmax * L.grad_total)
    _assert_same(dense, carved, reordered=(".gpack", ".grad", "ghid", "ghw0") if generic else ())


@pytest.mark.parametrize("i,prec", [pytest.param(i, prec, id=f"A{SHAPES[i][0]}-{'bf16' if prec else 'fp32'}")
                                    for i in (1, 3) for prec in (0, 1)])
def test_paired_contraction(i, prec):
    """t2o_bwd_tape_contract with two tapes (the mixer's first, the agent's second: at 8
    AGVs bf16 the agent's is the lean record) after both BPTTs, then each slab sum and
    unfold: equal to the dense run, and nothing outside the two slab buffers changes."""
    require_gpu()
    from t2omca_amd import _lib
    lib = _lib.lib()
    A, B, T = SHAPES[i][:3]
    fa, fm = _agent_fwd_dense(i, prec, False), _mixer_fwd_dense(i, prec, False)

    def run(mem):
        out = {}
        pm = _mixer_bwd(mem, i, prec, False, fm, [(0, 0, 0)], out, "m.")
        pa = _agent_bwd(mem, i, prec, False, fa, True, [(0, T)], out, "a.")
        tas = [_lib.TapeArgs(L=ctypes.pointer(p["L"]), pack=_ptr(p["pack"]), tape=_ptr(p["tape"]), tiles=p["tiles"],
                             gslabs=_ptr(p["slabs"]), nslab=p["nslab"], rec_format=p["fmt"]) for p in (pm, pa)]
        assert lib.t2o_bwd_tape_contract(ctypes.byref(tas[0]), ctypes.byref(tas[1]), _stream()) == 0
        mem.check("t2o_bwd_tape_contract (two tapes)")
        _reduce_unpack(mem, pm, "m.mixer", out)
        _reduce_unpack(mem, pa, "a.agent", out)
        return out

    nmax = lib.t2o_mixer_bwd_max_slabs(B)
    dense, carved = _both(run, nbytes=(64 << 20) + 4 * nmax * _layout(1, A, prec, False).grad_total)
    _assert_same(dense, carved)


# ---- the TD loss, Q(λ) and the logged sums ---------------------------------------------

def _td_inputs(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    T1 = T + 1
    term = torch.zeros(B, T1, 1, dtype=torch.uint8)
    filled = torch.ones(B, T1, 1, dtype=torch.int64)
    ends = torch.randint(T // 3, T, (B,), generator=g)
    for b in range(0, B, 2):  # every other episode ends early
        term[b, int(ends[b]), 0] = 1
        filled[b, int(ends[b]) + 1:, 0] = 0
    return dict(qtot=torch.randn(B, T, generator=g), qtot_tgt=torch.randn(B, T1, generator=g),
                qtot_taken=torch.randn(B, T, generator=g), reward=torch.randn(B, T1, 1, generator=g), term=term,
                filled=filled, w=0.5 + 0.5 * torch.rand(B, generator=g))


def _td(mem, B, T, lay):
    from t2omca_amd import _lib
    lib = _lib.lib()
    x = _td_inputs(B, T, 500 + B)
    qtot, qtgt, w = mem.inp("qtot", x["qtot"]), mem.inp("qtot_tgt", x["qtot_tgt"]), mem.inp("w", x["w"])
    reward = mem.inp("reward", x["reward"], lay[0], valid=T)[:, :, 0]
    term = mem.inp("terminated", x["term"], lay[1], valid=T)[:, :, 0]
    filled = mem.inp("filled", x["filled"], lay[2], valid=T)[:, :, 0]
    # qtot_taken: rows of T values qk_sb > T apart (the producer may unroll more steps)
    taken = mem.inp("qtot_taken", x["qtot_taken"][:, None, :], "padded")[:, 0]
    out = {}
    for what, algo in (("td_loss", 1), ("td_loss", 2), ("td_qlambda", 1), ("td_qlambda", 2)):
        tag = f"{what}.{algo}."
        o = dict(gq=mem.out(tag + "gq", (B, T)), targets=mem.out(tag + "targets", (B, T)),
                 prio=mem.out(tag + "prio", (B,)), loss=mem.out(tag + "loss", (2,)))
        acc = mem.out(tag + "mask_sum_acc", (1,))
        acc.zero_()
        kw = dict(qtot=_ptr(qtot), qtot_tgt=_ptr(qtgt), reward=_ptr(reward), rw_sb=reward.stride(0),
                  rw_st=reward.stride(1), term=_ptr(term), tm_sb=term.stride(0), tm_st=term.stride(1),
                  filled=_ptr(filled), fl_sb=filled.stride(0), fl_st=filled.stride(1), per_weight=_ptr(w),
                  mask_sum_acc=_ptr(acc), gamma=0.99, td_lambda=0.6, mask_sum=0.0, term_dtype=1, filled_dtype=3,
                  algo=algo, B=B, T=T, **{k: _ptr(v) for k, v in o.items()})
        if what == "td_loss":
            rc = lib.t2o_td_loss(ctypes.byref(_lib.TDArgs(**kw)), _stream())
        else:
            qa = _lib.TDQLambdaArgs(qtot_taken=_ptr(taken), qk_sb=taken.stride(0) if B > 1 else T, **kw)
            rc = lib.t2o_td_qlambda(ctypes.byref(qa), _stream())
        assert rc == 0, what
        mem.check(f"t2o_{what} algo {algo}")
        out.update({tag + k: v for k, v in o.items()})
        out[tag + "loss0"], out[tag + "mask_sum"] = o["loss"][:1], o["loss"][1:]
        del out[tag + "loss"]
        out[tag + "mask_sum_acc"] = acc
    stats = mem.out("stats", (4,), torch.float64)
    a = _lib.TDStatsArgs(qtot=_ptr(qtot), targets=_ptr(out["td_loss.1.targets"]), term=_ptr(term), tm_sb=term.stride(0),
                         tm_st=term.stride(1), filled=_ptr(filled), fl_sb=filled.stride(0), fl_st=filled.stride(1),
                         term_dtype=1, filled_dtype=3, B=B, T=T, out=_ptr(stats))
    assert lib.t2o_td_stats(ctypes.byref(a), _stream()) == 0
    mem.check("t2o_td_stats")
    out["stats"] = stats
    return out


@pytest.mark.parametrize("B,T,lay", [(3, 5, ("tm", "slice", "padded")), (5, 70, ("padded", "tm", "slice")),
                                     (2, 4, ("slice", "padded", "tm"))])
def test_td_loss_qlambda_and_stats(B, T, lay):
    """t2o_td_loss and t2o_td_qlambda (sequential and wave scan), t2o_td_stats: reward
    float, terminated uint8 and filled int64 in [B, T + 1, 1] storage, each tm / slice /
    padded over the cases, step T poisoned; qtot_taken with a padded row stride qk_sb > T.  T = 70
    spans more than one wave of steps.  The loss scalar sums workgroup partials with float
    atomics (rtol 1e-6, as test_td_loss_native_mask_dtypes); Σ mask and the rest are exact."""
    require_gpu()
    dense, carved = _both(lambda mem: _td(mem, B, T, lay), nbytes=8 << 20)
    x = _td_inputs(B, T, 500 + B)
    m = x["filled"][:, :T, 0].double()
    m[:, 1:] *= 1 - x["term"][:, :T - 1, 0].double()
    assert float(dense["td_loss.1.mask_sum"]) == float(m.sum()) == float(dense["stats"][0])
    _assert_same(dense, carved, loose=[k for k in dense if k.endswith("loss0")])


# ---- the noisy head -------------------------------------------------------------------

def _noisy(mem, A, B, T, lay):
    from t2omca_amd import _lib
    lib = _lib.lib()
    g = torch.Generator().manual_seed(600 + A)
    T1 = T + 1
    eps_w, eps_b = mem.out("eps_w", (T, NA, E)), mem.out("eps_b", (T, NA))
    for t0, t1 in ((T // 2, T), (0, T // 2)):
        a = _lib.NoiseArgs(eps_w=_ptr(eps_w), eps_b=_ptr(eps_b), seed=7, counter=3, kind=0, E=E, NA=NA, T=T, t0=t0,
                           t1=t1)
        assert lib.t2o_noise_normal(ctypes.byref(a), _stream()) == 0
        mem.check(f"t2o_noise_normal rows [{t0}, {t1})")
    u_w, u_b, s_w, s_b = (mem.inp(n, 0.3 * torch.randn(*s, generator=g))
                          for n, s in (("u_w", (NA, E)), ("u_b", (NA,)), ("s_w", (NA, E)), ("s_b", (NA,))))
    h = mem.inp("h", torch.randn(B, T1, A, E, generator=g), None, valid=T)  # h_ts = T + 1, step T poisoned
    q = mem.out("q", (B, T, A, NA))
    a = _lib.NoisyFwdArgs(h=_ptr(h), u_w=_ptr(u_w), u_b=_ptr(u_b), s_w=_ptr(s_w), s_b=_ptr(s_b), eps_w=_ptr(eps_w),
                          eps_b=_ptr(eps_b), q=_ptr(q), h_ts=T1, q_ts=T, B=B, A=A, E=E, NA=NA)
    for a.t0, a.t1 in ((0, T // 2), (T // 2, T)):
        assert lib.t2o_noisy_head_fwd(ctypes.byref(a), _stream()) == 0
        mem.check("t2o_noisy_head_fwd")
    gchosen = mem.inp("gchosen", torch.randn(B, T, A, generator=g))
    gh_in = mem.inp("gh_in", torch.randn(B, T, A, E, generator=g))
    actions = mem.inp("actions", torch.randint(0, NA, (B, T1, A, 1), generator=g), lay, valid=T)[..., 0]
    P = lib.t2o_noisy_head_parts(B, A)
    assert P >= 1
    gh_out, gpart = mem.out("gh_out", (B, T, A, E)), mem.out("gpart", (T, P, NA, E + 1))
    b = _lib.NoisyBwdArgs(gchosen=_ptr(gchosen), actions=_ptr(actions), act_sb=actions.stride(0),
                          act_st=actions.stride(1), h=_ptr(h), u_w=_ptr(u_w), s_w=_ptr(s_w), eps_w=_ptr(eps_w),
                          gh_in=_ptr(gh_in), gh_out=_ptr(gh_out), gpart=_ptr(gpart), h_ts=T1, B=B, T=T, A=A, E=E, NA=NA)
    for b.t_lo, b.t_hi in ((T // 2, T), (0, T // 2)):
        assert lib.t2o_noisy_head_bwd(ctypes.byref(b), _stream()) == 0
        mem.check("t2o_noisy_head_bwd")
    du = [mem.out(n, s) for n, s in (("du_w", (NA, E)), ("du_b", (NA,)), ("ds_w", (NA, E)), ("ds_b", (NA,)))]
    for t in du:
        t.zero_()  # (accumulated)
    w = _lib.NoisyWgradArgs(gpart=_ptr(gpart), eps_w=_ptr(eps_w), eps_b=_ptr(eps_b), du_w=_ptr(du[0]), du_b=_ptr(du[1]),
                            ds_w=_ptr(du[2]), ds_b=_ptr(du[3]), B=B, T=T, A=A, E=E, NA=NA)
    assert lib.t2o_noisy_head_wgrad(ctypes.byref(w), _stream()) == 0
    mem.check("t2o_noisy_head_wgrad")
    return dict(eps_w=eps_w, eps_b=eps_b, q=q, gh_out=gh_out, gpart=gpart, du_w=du[0], du_b=du[1], ds_w=du[2],
                ds_b=du[3])


@pytest.mark.parametrize("A,B,T,lay", [(5, 3, 4, "tm"), (16, 3, 4, "padded"), (64, 2, 3, "slice")])
def test_noisy_head(A, B, T, lay):
    """t2o_noise_normal, t2o_noisy_head_fwd / _bwd (each in two step ranges), _wgrad: gpart
    of t2o_noisy_head_parts(B, A) parts; the [B, T, A, 1] int64 actions tm / padded / slice,
    h_ts = T + 1 with step T poisoned.  The dense q is held against W_t h + b_t in fp64."""
    require_gpu()
    dense, carved = _both(lambda mem: _noisy(mem, A, B, T, lay), nbytes=16 << 20)
    g = torch.Generator().manual_seed(600 + A)
    u_w, u_b, s_w, s_b = (0.3 * torch.randn(*s, generator=g).double() for s in ((NA, E), (NA,), (NA, E), (NA,)))
    h = torch.randn(B, T + 1, A, E, generator=g).double()[:, :T]
    W = u_w + s_w * dense["eps_w"].cpu().double()
    q = torch.einsum("tne,btae->btan", W, h) + (u_b + s_b * dense["eps_b"].cpu().double())[None, :, None, :]
    assert normwise(dense["q"], q) < 1e-5
    _assert_same(dense, carved)


# ---- the optimisers, action selection ----------------------------------------------------

def _optim(mem, n, which):
    from t2omca_amd import _lib
    lib = _lib.lib()
    g = torch.Generator().manual_seed(700 + n)
    p, gr = mem.inp("params", torch.randn(n, generator=g)), mem.inp("grads", 3.0 * torch.randn(n, generator=g))
    m, v = mem.inp("exp_avg", 0.1 * torch.randn(n, generator=g)), mem.inp("exp_avg_sq", torch.rand(n, generator=g))
    ws = mem.out("workspace", (lib.t2o_adam_workspace_floats(),))
    div = mem.inp("grad_div", torch.tensor([7.0]))
    norm = mem.out("grad_norm", (1,))
    if which == "adam":
        rc = lib.t2o_adam_step(_vp(p), _vp(gr), _vp(m), _vp(v), _vp(ws), n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 10.0, 3,
                               _vp(div), _vp(norm), _stream())
    else:
        rc = lib.t2o_rmsprop_step(_vp(p), _vp(gr), _vp(v), _vp(ws), n, 1e-3, 0.99, 1e-8, 1e-4, 10.0, _vp(div),
                                  _vp(norm), _stream())
    assert rc == 0
    mem.check("t2o_%s_step" % which)
    return dict(params=p, exp_avg=m, exp_avg_sq=v, grad_norm=norm, grads=gr)


@pytest.mark.parametrize("which", ["adam", "rmsprop"])
@pytest.mark.parametrize("n", [1037, 83191])
def test_optimiser_steps(which, n):
    """t2o_adam_step / t2o_rmsprop_step in place on buffers of exactly n floats, n no
    multiple of a workgroup or of 4 (1037: under one reduction block; 83191: about the
    default networks' parameter count), the workspace t2o_adam_workspace_floats floats."""
    require_gpu()
    dense, carved = _both(lambda mem: _optim(mem, n, which), nbytes=8 << 20)
    assert abs(float(dense["grad_norm"]) / float((dense["grads"].double() / 7.0).norm()) - 1) < 1e-5
    _assert_same(dense, carved)


def _select(mem, rows, eps):
    from t2omca_amd import _lib
    g = torch.Generator().manual_seed(800 + rows)
    q = mem.inp("q", torch.randn(rows, NA, generator=g))
    avail = mem.inp("avail", _avail(1, 1, rows, g)[0, 0])
    act = mem.out("actions", (rows,), torch.int64)
    assert _lib.lib().t2o_select_actions(_vp(q), _vp(avail), _vp(act), rows, NA, eps, ctypes.c_uint64(5), 9,
                                         _stream()) == 0
    mem.check("t2o_select_actions")
    return dict(actions=act, avail=avail)


@pytest.mark.parametrize("rows,eps", [(15, 0.0), (24 * 8 + 3, 0.3)])
def test_select_actions(rows, eps):
    """t2o_select_actions on exactly `rows` rows (15: under a wave; 195: several workgroups'
    worth, odd): actions in range, available, equal to the dense run."""
    require_gpu()
    dense, carved = _both(lambda mem: _select(mem, rows, eps), nbytes=4 << 20)
    a = dense["actions"]
    assert ((a >= 0) & (a < NA)).all() and (dense["avail"].gather(1, a[:, None]) == 1).all()
    _assert_same(dense, carved)


# ---- the alignment rule of the mixers' hidden states --------------------------------------

@pytest.mark.parametrize("bad", ["base", "hid_st", "hid_sb"])
def test_mixer_rejects_misaligned_hidden_states(bad):
    """include/t2omca.h: hid_on / hid_tg / hid are 16-byte aligned with hid_sb / hid_st in
    multiples of 4 floats (the tuned kernels load 4 floats at a time); anything else is
    T2O_EINVAL before any launch, forward and backward."""
    require_gpu()
    from t2omca_amd import _lib
    lib = _lib.lib()
    A, B, T = 8, 3, 5
    L = _layout(1, A, 0, False)
    # every buffer has its real size (zeros), so the calls are harmless whatever they return
    z = lambda *shape: torch.zeros(*(int(n) for n in shape), device="cuda")  # noqa: E731
    row = A * E
    buf = z(B * (T + 1) * (row + 4) + 8)
    off, st, sb = ((1, row, T * row) if bad == "base" else (0, row + 2, T * (row + 2)) if bad == "hid_st"
                   else (0, row, T * row + 2))
    hid = buf.data_ptr() + 4 * off
    pack, states, qv, y, hw = z(L.pack_floats), z(B, T, A * FS), z(B, T, A), z(B, T), z(B, T, 3, E)
    fa = _lib.MixerFwdArgs(L=ctypes.pointer(L), pack_on=_ptr(pack), states=_ptr(states), st_sb=T * A * FS,
                           st_st=A * FS, hid_on=hid, hid_sb=sb, hid_st=st, qmode_on=0, qv_on=_ptr(qv), y_on=_ptr(y),
                           hw_on=_ptr(hw), B=B, T_on=T)
    assert lib.t2o_mixer_unroll_fwd(ctypes.byref(fa), _stream()) == T2O_EINVAL
    tiles = lib.t2o_bwd_tape_tiles(ctypes.byref(L), B, T, A)
    nmax = lib.t2o_mixer_bwd_max_slabs(B)
    xout, gqv, ghid = z(B, T, A + 3, E), z(B, T, A), z(B, T, A, E)
    slabs, tape = z(nmax * L.grad_total), z(lib.t2o_bwd_tape_floats(ctypes.byref(L), tiles))
    nslab = ctypes.c_int32(0)
    ba = _lib.MixerBwdArgs(L=ctypes.pointer(L), pack=_ptr(pack), states=_ptr(states), st_sb=T * A * FS, st_st=A * FS,
                           hid=hid, hid_sb=sb, hid_st=st, qv=_ptr(qv), hw=_ptr(hw), xout=_ptr(xout), gy=_ptr(y),
                           gqv=_ptr(gqv), ghid=_ptr(ghid), gslabs=_ptr(slabs), max_slabs=nmax,
                           nslab=ctypes.pointer(nslab), tape=_ptr(tape), B=B, T=T)
    assert lib.t2o_mixer_unroll_bwd(ctypes.byref(ba), _stream()) == T2O_EINVAL
    torch.cuda.synchronize()
