"""Thin torch-tensor wrappers over the C-ABI entry points (include/t2omca.h).

Every function checks device/dtype/contiguity on the host, then launches on
the current HIP stream.  There is no CPU path: CPU tensors raise.
"""
import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import (AgentBwdArgs, AgentFwdArgs, MixerBwdArgs, MixerFwdArgs, TapeArgs, TDArgs, TDQLambdaArgs, check, lib,
                   ptr, stream_ptr)

AGENT, MIXER = 0, 1


def _dev(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback); "
                               "the CPU restatement lives in oracle/ and is test-only")
        if t.dtype not in (torch.float32, torch.int64):
            raise TypeError(f"t2omca_amd: unsupported dtype {t.dtype}")


@dataclass(frozen=True)
class NetShape:
    kind: int
    E: int
    H: int
    D: int
    F: int
    NA: int
    FF: int
    n_ent: int
    prec: int = 0   # 0 fp32, 1 bf16 MFMA operands (fp32 accumulate / LayerNorm / softmax / state)
    n_agents: int = 0  # mixer: agents (hidden tokens / qvals); 0 = n_ent (its state tokens)
    pos_func: int = 0  # mixer head positivity (_lib.POS_FUNCS; 3 = identity)
    pos_beta: float = 1.0

    def layout(self):
        return _layout_cached(self)

    @property
    def generic(self):
        """True when no tuned kernel instance exists: the runtime-shaped kernels run."""
        return bool(self.layout().generic)

    @property
    def instance(self):
        """Which kernels run this network: "exact" (MFMA instance compiled for its entity
        count), "runtime" (MFMA instance of a capacity class, entity count read at run
        time) or "generic" (runtime-shaped fp32 kernels) — include/t2omca.h."""
        if not hasattr(lib(), "t2o_layout_instance"):  # an older build under A/B timing (T2O_LIB)
            return "generic" if self.generic else "exact"
        return ("exact", "runtime", "generic")[int(lib().t2o_layout_instance(ctypes.byref(self.layout())))]

    @property
    def agents(self):
        return self.n_agents or self.n_ent

    @property
    def n_params(self):
        return int(lib().t2o_param_count(self.kind, self.E, self.H, self.D, self.F, self.NA, self.FF))


_LAYOUTS = {}


def _layout_cached(s):
    key = (s, _lib.force_generic())
    L = _LAYOUTS.get(key)
    if L is None:
        L = _lib.make_layout(s.kind, s.E, s.H, s.D, s.F, s.NA, s.FF, s.n_ent, s.prec, s.n_agents, s.pos_func,
                             s.pos_beta)
        _LAYOUTS[key] = L
    return L


def pack_params(shape: NetShape, params: torch.Tensor, out: torch.Tensor = None):
    """params (flat, reference state_dict order) -> folded kernel pack."""
    _dev(params)
    L = shape.layout()
    assert params.numel() == shape.n_params and params.is_contiguous()
    if out is None:
        out = torch.empty(L.pack_floats, device=params.device, dtype=torch.float32)
    check(lib().t2o_pack_params(ctypes.byref(L), ptr(params), ptr(out), stream_ptr()), "pack_params")
    return out


def unpack_grads(shape: NetShape, params, gpack, grad):
    """grad += unfold(gpack)   (grad in reference parameter order)."""
    _dev(params, gpack, grad)
    L = shape.layout()
    check(lib().t2o_unpack_grads(ctypes.byref(L), ptr(params), ptr(gpack), ptr(grad), stream_ptr()),
          "unpack_grads")
    return grad


def reduce_slabs(slabs, nslab, out):
    _dev(slabs, out)
    check(lib().t2o_reduce_slabs(ptr(slabs), int(nslab), out.numel(), ptr(out), stream_ptr()),
          "reduce_slabs")
    return out


def _p(t):
    """Device address of a tensor for an argument struct's pointer field (None -> NULL)."""
    return None if t is None else t.data_ptr()


def _mark(timer, tag):
    if timer is not None:
        timer(tag)


def agent_unroll_fwd(shape: NetShape, pack_on, obs, h0_on=None, pack_tg=None, h0_tg=None, timer=None,
                     hmid_on=None, steps=None, outs=None, launcher=False):
    """Unroll the agent over obs [B, T, A, n_ent*F] (any stride over B, T; inner
    [A, n_ent*F] contiguous).  Returns (q_on, h_on[, q_tg, h_tg]) with
    q [B, T, A, NA], h [B, T, A, E].  hmid_on: optional [B, T, D-1, A, E]
    output buffer for the inter-block activations (used by the backward).
    steps=(t0, t1): only those steps (t2o_agent_fwd_args.t0 / t1: t0 > 0 continues
    from h[t0 - 1]) into the given outs=(q_on, h_on, q_tg, h_tg)."""
    _dev(pack_on, obs, h0_on, pack_tg, h0_tg)
    B, T, A, nf = obs.shape
    assert obs.dtype == torch.float32 and nf == shape.n_ent * shape.F
    assert obs.stride(3) == 1 and obs.stride(2) == nf, "obs rows must be contiguous per timestep"
    L = shape.layout()
    dev = obs.device
    if outs is not None:
        q_on, h_on, q_tg, h_tg = outs
    else:
        q_on = torch.empty(B, T, A, shape.NA, device=dev)
        h_on = torch.empty(B, T, A, shape.E, device=dev)
        q_tg = h_tg = None
        if pack_tg is not None:
            q_tg = torch.empty_like(q_on)
            h_tg = torch.empty_like(h_on)
    for h0 in (h0_on, h0_tg):
        if h0 is not None:
            assert h0.is_contiguous() and h0.numel() == B * A * shape.E
    a = AgentFwdArgs(L=ctypes.pointer(L), pack_on=_p(pack_on), pack_tg=_p(pack_tg), obs=_p(obs),
                     obs_sb=obs.stride(0), obs_st=obs.stride(1), h0_on=_p(h0_on), h0_tg=_p(h0_tg), q_on=_p(q_on),
                     h_on=_p(h_on), hmid_on=_p(hmid_on), q_tg=_p(q_tg), h_tg=_p(h_tg), B=B, T=T, A=A)
    fn = lib().t2o_agent_unroll_fwd

    def go(t0, t1):
        a.t0, a.t1 = int(t0), int(t1)
        _mark(timer, "begin:agent_fwd")
        check(fn(ctypes.byref(a), stream_ptr()), "agent_unroll_fwd")
        _mark(timer, "end:agent_fwd")
    if launcher:  # go(t0, t1) per step range, the arguments converted once (pipelined learner)
        return go
    go(*(steps if steps is not None else (0, T)))
    if pack_tg is not None:
        return q_on, h_on, q_tg, h_tg
    return q_on, h_on


def tape_floats(shape: NetShape, tiles):
    """Backward tape workspace (floats) for `tiles` tiles of weight-gradient records
    (16 per tile; a one-tile mixer stores just its A+3 query rows)."""
    return int(lib().t2o_bwd_tape_floats(ctypes.byref(shape.layout()), int(tiles)))


def agent_tape_tiles(B, T, A, shape: NetShape = None):
    return T * ((B * A + 15) // 16)


def mixer_tape_tiles(B, T, A, shape: NetShape):
    """Weight-gradient tape tiles per block of a mixer BPTT over B episodes x T
    steps (include/t2omca.h t2o_bwd_tape_tiles: one tile of the A+3 query rows
    per (episode, step) when they fit 16 records; tuned multi-tile mixers store
    each block's query-row records as one compact stream cut into 16-record
    tiles, t2o_mixer.hip)."""
    n = int(lib().t2o_bwd_tape_tiles(ctypes.byref(shape.layout()), int(B), int(T), int(A)))
    if n < 0:
        raise ValueError(f"mixer_tape_tiles: bad shape B={B} T={T} A={A} for a mixer of {shape.agents} agents")
    return n


def _tape(shape, tiles, tape, device):
    n = tape_floats(shape, tiles)
    if tape is None or tape.numel() < n:
        tape = torch.empty(n, device=device)
    return tape


# The tape contraction runs one workgroup per slab (split-K over the tape's
# tiles).  A backward over a small replay batch fills few slabs (the mixer BPTT
# one per 1-4 episodes, the agent BPTT one per two 16-row tiles: 8 and 16 at
# configs[0]'s 32 episodes), so its contraction would stream the whole tape
# through those few workgroups; it gets at least CONTRACT_MIN_WG instead, the
# extra slabs zeroed first (they receive no BPTT flush; the contraction writes
# everything else of a slab itself).
CONTRACT_MIN_WG = 256


def mixer_work_floats(shape: NetShape, B, T):
    """Workspace floats of a decoupled multi-tile mixer backward (0 when it does not
    run decoupled at this batch: t2o_mixer_split)."""
    L = shape.layout()
    if int(lib().t2o_mixer_split(ctypes.byref(L), int(B))) != 1:
        return 0
    return max(0, int(lib().t2o_mixer_bwd_work_floats(ctypes.byref(L), int(B), int(T))))


def mixer_slab_count(B):
    """Slabs a mixer backward over B episodes needs (its BPTT's + the widened contraction's)."""
    return max(int(lib().t2o_mixer_bwd_max_slabs(B)), CONTRACT_MIN_WG)


def agent_slab_count(B, A):
    """Slabs an agent backward over B episodes of A agents needs."""
    return max(int(lib().t2o_agent_bwd_max_slabs(B, A)), CONTRACT_MIN_WG)


class DeferredContraction:
    """A backward call's weight-gradient tape, not yet contracted: call it (on the
    stream that should run the contraction + slab sum) for the compact gradient
    block, or hand two of them to tape_contract_pair."""

    def __init__(self, shape, pack, tape, tiles, slabs, nslab, timer, tag, fmt):
        self.shape, self.pack, self.tape, self.tiles = shape, pack, tape, tiles
        self.slabs, self.nslab, self.timer, self.tag, self.fmt = slabs, nslab, timer, tag, fmt

    def widen(self):
        """Raise the contraction's workgroup count to CONTRACT_MIN_WG where the slab
        buffer holds them (tuned layouts): zero the slabs past the BPTT's on the
        current stream.  Idempotent."""
        L = self.shape.layout()
        cap = self.slabs.numel() // L.grad_total
        nc = min(max(self.nslab, CONTRACT_MIN_WG), cap)
        if L.generic or nc <= self.nslab:
            return
        self.slabs[self.nslab * L.grad_total:nc * L.grad_total].zero_()
        self.nslab = nc

    def __call__(self):
        self.widen()
        return tape_contract(self.shape, self.pack, self.tape, self.tiles, self.slabs, self.nslab, self.timer,
                             self.tag, self.fmt)


def agent_unroll_bwd(shape: NetShape, pack, obs, h_seq, h0=None, gq=None, gchosen=None, actions=None,
                     gh=None, want_gh0=False, slabs=None, timer=None, hmid=None, tape=None, defer_contract=False,
                     steps=None, gcarry=None, launcher=False):
    """BPTT of agent_unroll_fwd over the first T = len(grads) steps.

    obs [B, >=T, A, nF]; h_seq [B, Ts>=T, A, E] (forward output); gq [B,T,A,NA],
    gchosen [B,T,A] + actions (int64 [B, >=T, A], a-stride 1), gh [B,T,A,E].
    Returns (gpack, gh0) with gpack the compact weight-gradient block (with
    defer_contract, a DeferredContraction instead).  steps=(t_lo, t_hi): only
    steps t_hi - 1 .. t_lo (t2o_agent_bwd_args.t_lo / t_hi; ranges from the last down
    on the same slabs / tape, gcarry [B*A, E] between them); the contraction is
    then always deferred (call it after the range that ends at step 0)."""
    _dev(pack, obs, h_seq, h0, gq, gchosen, actions, gh)
    B, _, A, _ = obs.shape
    T = next(t.shape[1] for t in (gq, gchosen, gh) if t is not None)
    L = shape.layout()
    for t in (gq, gchosen, gh):
        assert t is None or t.is_contiguous()
    assert h_seq.is_contiguous() and h_seq.shape[1] >= T
    act_sb = act_st = 0
    if gchosen is not None:
        assert actions is not None and actions.dtype == torch.int64 and actions.stride(2) == 1
        act_sb, act_st = actions.stride(0), actions.stride(1)
    nmax = int(lib().t2o_agent_bwd_max_slabs(B, A))
    if slabs is None or slabs.numel() < nmax * L.grad_total:
        nmax = agent_slab_count(B, A)
        slabs = torch.empty(nmax * L.grad_total, device=obs.device)
    gh0 = torch.empty(B, A, shape.E, device=obs.device) if want_gh0 else None
    tiles = agent_tape_tiles(B, T, A)
    tape = _tape(shape, tiles, tape, obs.device)
    nslab = ctypes.c_int32(0)
    a = AgentBwdArgs(L=ctypes.pointer(L), pack=_p(pack), obs=_p(obs), obs_sb=obs.stride(0), obs_st=obs.stride(1),
                     h0=_p(h0), h_seq=_p(h_seq), hmid=_p(hmid), h_ts=h_seq.shape[1], gq=_p(gq), gchosen=_p(gchosen),
                     actions=_p(actions), act_sb=act_sb, act_st=act_st, gh=_p(gh), gslabs=_p(slabs), max_slabs=nmax,
                     nslab=ctypes.pointer(nslab), tape=_p(tape), gh0=_p(gh0), gcarry=_p(gcarry), B=B, T=T, A=A)
    fn = lib().t2o_agent_unroll_bwd
    fmt = int(lib().t2o_agent_bwd_tape_format(ctypes.byref(L), int(hmid is not None)))

    def go(t_lo, t_hi):
        a.t_lo, a.t_hi = int(t_lo), int(t_hi)
        _mark(timer, "begin:agent_bwd")
        check(fn(ctypes.byref(a), stream_ptr()), "agent_unroll_bwd")
        _mark(timer, "end:agent_bwd")
        return DeferredContraction(shape, pack, tape, tiles, slabs, nslab.value, timer, "agent_dw", fmt)
    if launcher:  # go(t_lo, t_hi) per step range -> the (deferred) contraction
        return go, gh0
    dc = go(*(steps if steps is not None else (0, T)))
    return (dc if defer_contract or steps is not None else dc()), gh0


def _mstrides(t):
    return (t.stride(0), t.stride(1)) if t is not None else (0, 0)


def _hid_aligned(hid):
    """include/t2omca.h (t2o_mixer_fwd_args.hid_on): the mixer kernels read a step's hidden
    tokens with 16-byte loads, so the base and every (episode, step) row are 16-byte
    aligned: episode / step strides in multiples of 4 floats."""
    return (hid.data_ptr() % 16 == 0 and (hid.shape[0] < 2 or hid.stride(0) % 4 == 0) and
            (hid.shape[1] < 2 or hid.stride(1) % 4 == 0))


def mixer_unroll_fwd(shape: NetShape, pack_on, states, hid_on, *, qmode_on=0, qv_on=None, q_on=None,
                     actions=None, avail=None, hw0_on=None, T_on=None,
                     pack_tg=None, hid_tg=None, qmode_tg=2, qv_tg=None, q_tg=None, hw0_tg=None,
                     T_tg=None, want_xout=True, timer=None, phase=0, steps=None, outs=None, launcher=False):
    """Mixer unroll (see include/t2omca.h).  states [B, >=T, n_ent*F];
    hid_* [B, >=T, A, E] (contiguous inner [A, E]); q_on/q_tg [B, q_ts, A, NA]
    contiguous; actions int64 [B, >=T, A]; avail int32 [B, >=T, A, NA].
    Returns dict of outputs per network: y [B,T], hw [B,T,3,E], qv [B,T,A], xout.
    phase 1 / 2 (a decoupled mixer, t2o_mixer_fwd_args.phase): the recurrence
    over steps=(t0, t1) / the parallel rows, into the given outs=(o_on, o_tg)."""
    _dev(pack_on, states, hid_on, qv_on, q_on, hw0_on, pack_tg, hid_tg, qv_tg, q_tg, hw0_tg)
    B = states.shape[0]
    A, E = hid_on.shape[2], shape.E
    if A != shape.agents:
        raise ValueError(f"mixer_unroll_fwd: hidden states carry {A} agents, the mixer was built for {shape.agents}")
    L = shape.layout()
    dev = states.device
    T_on = T_on or (qv_on.shape[1] if qv_on is not None else hid_on.shape[1])
    assert hid_on.stride(3) == 1 and hid_on.stride(2) == E and states.stride(2) == 1
    assert _hid_aligned(hid_on), "mixer_unroll_fwd: hidden-state rows must be 16-byte aligned"
    if hid_tg is not None:
        assert hid_tg.stride(0) == hid_on.stride(0) and hid_tg.stride(1) == hid_on.stride(1)
        assert _hid_aligned(hid_tg), "mixer_unroll_fwd: hidden-state rows must be 16-byte aligned"
    q_ts = q_on.shape[1] if q_on is not None else 0
    for q in (q_on, q_tg):
        assert q is None or (q.is_contiguous() and q.shape[1] == q_ts)
    if actions is not None:
        assert actions.dtype == torch.int64 and actions.stride(2) == 1
    if avail is not None:
        assert avail.dtype == torch.int32 and avail.stride(3) == 1 and avail.stride(2) == avail.shape[3]

    def alloc(T, bwd):
        # xout / xmid only feed the backward: the target network skips them
        return dict(y=torch.empty(B, T, device=dev), hw=torch.empty(B, T, 3, E, device=dev),
                    qv=torch.empty(B, T, A, device=dev),
                    xout=torch.empty(B, T, A + 3, E, device=dev) if bwd else None,
                    xmid=torch.empty(B, T, shape.D - 1, A + 3, E, device=dev) if (bwd and shape.D > 1) else None)

    # a multi-tile mixer at a small batch runs decoupled (t2o_mixer_split.hip): its
    # parallel kernel reads the recurrent kernel's window rows back from xout
    split = bool(lib().t2o_mixer_split(ctypes.byref(L), B) == 1)
    given = outs
    if given is not None:
        o_on, o_tg = given
        T_tg = T_tg or (hid_tg.shape[1] if hid_tg is not None else None)
    else:
        o_on = alloc(T_on, want_xout or split)
        o_tg = None
        if pack_tg is not None:
            T_tg = T_tg or hid_tg.shape[1]
            o_tg = alloc(T_tg, False)
            if split:
                o_tg["xout"] = torch.empty(B, T_tg, A + 3, E, device=dev)
    n_actions = q_on.shape[3] if q_on is not None else 0
    act_sb, act_st = _mstrides(actions)
    av_sb, av_st = _mstrides(avail)
    g = lambda d, k: _p(d[k]) if d is not None else None  # noqa: E731
    a = MixerFwdArgs(L=ctypes.pointer(L), pack_on=_p(pack_on), pack_tg=_p(pack_tg), states=_p(states),
                     st_sb=states.stride(0), st_st=states.stride(1), hid_on=_p(hid_on), hid_tg=_p(hid_tg),
                     hid_sb=hid_on.stride(0), hid_st=hid_on.stride(1), hw0_on=_p(hw0_on), hw0_tg=_p(hw0_tg),
                     qmode_on=qmode_on, qmode_tg=qmode_tg, qv_on=_p(qv_on), qv_tg=_p(qv_tg), q_on=_p(q_on),
                     q_tg=_p(q_tg), q_ts=q_ts, n_actions=n_actions, actions=_p(actions), act_sb=act_sb,
                     act_st=act_st, avail=_p(avail), av_sb=av_sb, av_st=av_st,
                     y_on=g(o_on, "y"), hw_on=g(o_on, "hw"), qvo_on=g(o_on, "qv"), xout_on=g(o_on, "xout"),
                     xmid_on=g(o_on, "xmid"), y_tg=g(o_tg, "y"), hw_tg=g(o_tg, "hw"), qvo_tg=g(o_tg, "qv"),
                     xout_tg=g(o_tg, "xout"), xmid_tg=g(o_tg, "xmid"), B=B, T_on=T_on, T_tg=T_tg or 0)
    fn = lib().t2o_mixer_unroll_fwd

    def go(phase, t0=0, t1=0):
        a.phase, a.t0, a.t1 = int(phase), int(t0), int(t1)
        _mark(timer, "begin:mixer_fwd")
        check(fn(ctypes.byref(a), stream_ptr()), "mixer_unroll_fwd")
        _mark(timer, "end:mixer_fwd")
    if launcher:  # go(phase, t0, t1) per phase / step range (pipelined learner)
        return go
    go(int(phase), *(steps if steps is not None else (0, 0)))
    return (o_on, o_tg) if pack_tg is not None else o_on


def tape_contract(shape: NetShape, pack, tape, tiles, slabs, nslab, timer=None, tag="dw", fmt=0):
    """Fill the M/N/W1/W2 regions of the backward's slabs from its tape (pack =
    the pack the backward used; fmt = the tape's record format,
    t2o_agent_bwd_tape_format), then sum the slabs.  Returns the compact
    gradient block (on the current stream)."""
    L = shape.layout()
    _mark(timer, "begin:" + tag)
    a = TapeArgs(L=ctypes.pointer(L), pack=_p(pack), tape=_p(tape), tiles=int(tiles), gslabs=_p(slabs),
                 nslab=int(nslab), rec_format=int(fmt))
    check(lib().t2o_bwd_tape_contract(ctypes.byref(a), None, stream_ptr()), "bwd_tape_contract")
    _mark(timer, "end:" + tag)
    gpack = torch.empty(L.grad_total, device=slabs.device)
    reduce_slabs(slabs, nslab, gpack)
    return gpack


def tape_contract_pair(dm: DeferredContraction, da: DeferredContraction, timer=None):
    """Both backwards' tape contractions in one launch (t2o_bwd_tape_contract with two tapes;
    dm the mixer's, da the agent's), then each slab sum.  Returns (gpack_m, gpack_a)."""
    Lm, La = dm.shape.layout(), da.shape.layout()
    dm.widen()
    da.widen()
    _mark(timer, "begin:dw_pair")
    am = TapeArgs(L=ctypes.pointer(Lm), pack=_p(dm.pack), tape=_p(dm.tape), tiles=int(dm.tiles), gslabs=_p(dm.slabs),
                  nslab=int(dm.nslab), rec_format=0)
    aa = TapeArgs(L=ctypes.pointer(La), pack=_p(da.pack), tape=_p(da.tape), tiles=int(da.tiles), gslabs=_p(da.slabs),
                  nslab=int(da.nslab), rec_format=int(da.fmt))
    check(lib().t2o_bwd_tape_contract(ctypes.byref(am), ctypes.byref(aa), stream_ptr()), "bwd_tape_contract (pair)")
    _mark(timer, "end:dw_pair")
    out = []
    for d, L in ((dm, Lm), (da, La)):
        g = torch.empty(L.grad_total, device=d.slabs.device)
        reduce_slabs(d.slabs, d.nslab, g)
        out.append(g)
    return out[0], out[1]


def mixer_unroll_bwd(shape: NetShape, pack, states, hid, fwd, gy, hw0=None, ghw_ext=None,
                     want_ghw0=False, slabs=None, timer=None, tape=None, defer_contract=False, work=None,
                     phase=0, steps=None, carry=None, outs=None, launcher=False):
    """BPTT of mixer_unroll_fwd (one network, `fwd` = its output dict).
    Returns (gpack, gqv [B,T,A], ghid [B,T,A,E], ghw0 or None).  With
    defer_contract the first item is instead a zero-argument callable that runs
    the tape contraction + slab sum (on whatever stream is current when called)
    and returns gpack.  work: optional float buffer for the decoupled multi-tile
    mixer (t2o_mixer_bwd_work_floats; allocated here when needed and not given).
    phase 1 / 2 (a decoupled mixer, t2o_mixer_bwd_args.phase): the parallel
    part / the recurrence over steps=(t_lo, t_hi) (ranges from the last down,
    carry [B, 3, E] between them) into outs=(gqv, ghid), with the same slabs,
    tape and work every call; the contraction is then always deferred."""
    _dev(pack, states, hid, gy, hw0, ghw_ext)
    B, T = gy.shape
    A, E = hid.shape[2], shape.E
    if A != shape.agents:
        raise ValueError(f"mixer_unroll_bwd: hidden states carry {A} agents, the mixer was built for {shape.agents}")
    L = shape.layout()
    dev = gy.device
    assert gy.is_contiguous() and fwd["xout"] is not None
    assert _hid_aligned(hid), "mixer_unroll_bwd: hidden-state rows must be 16-byte aligned"
    nmax = int(lib().t2o_mixer_bwd_max_slabs(B))
    if slabs is None or slabs.numel() < nmax * L.grad_total:
        nmax = mixer_slab_count(B)
        slabs = torch.empty(nmax * L.grad_total, device=dev)
    if outs is not None:
        gqv, ghid = outs
    else:
        gqv = torch.empty(B, T, A, device=dev)
        ghid = torch.empty(B, T, A, E, device=dev)
    ghw0 = torch.empty(B, 3, E, device=dev) if want_ghw0 else None
    tiles = mixer_tape_tiles(B, T, A, shape)
    tape = _tape(shape, tiles, tape, dev)
    nslab = ctypes.c_int32(0)
    nwork = mixer_work_floats(shape, B, T)
    if nwork and (work is None or work.numel() < nwork):
        work = torch.empty(nwork, device=dev)
    a = MixerBwdArgs(L=ctypes.pointer(L), pack=_p(pack), states=_p(states), st_sb=states.stride(0),
                     st_st=states.stride(1), hid=_p(hid), hid_sb=hid.stride(0), hid_st=hid.stride(1), hw0=_p(hw0),
                     qv=_p(fwd["qv"]), hw=_p(fwd["hw"]), xout=_p(fwd["xout"]), xmid=_p(fwd.get("xmid")), gy=_p(gy),
                     ghw_ext=_p(ghw_ext), gqv=_p(gqv), ghid=_p(ghid), ghw0=_p(ghw0), gslabs=_p(slabs), max_slabs=nmax,
                     nslab=ctypes.pointer(nslab), tape=_p(tape), work=_p(work) if nwork else None, work_floats=nwork,
                     ghw_carry=_p(carry), B=B, T=T)
    fn = lib().t2o_mixer_unroll_bwd

    def go(phase, t_lo=0, t_hi=0):
        a.phase, a.t_lo, a.t_hi = int(phase), int(t_lo), int(t_hi)
        _mark(timer, "begin:mixer_bwd")
        check(fn(ctypes.byref(a), stream_ptr()), "mixer_unroll_bwd")
        _mark(timer, "end:mixer_bwd")
        return DeferredContraction(shape, pack, tape, tiles, slabs, nslab.value, timer, "mixer_dw", 0)
    if launcher:  # go(phase, t_lo, t_hi) per phase / step range -> the (deferred) contraction
        return go
    contract = go(int(phase), *(steps if steps is not None else (0, 0)))
    return (contract if defer_contract or phase else contract()), gqv, ghid, ghw0


# TD loss mask element types (include/t2omca.h T2O_DT_*)
_MASK_DT = {torch.float32: 0, torch.uint8: 1, torch.bool: 1, torch.int32: 2, torch.int64: 3}


def _mask_dtype(t):
    if t is None:
        return 0
    if t.dtype not in _MASK_DT:
        raise TypeError(f"td_loss: unsupported mask dtype {t.dtype}")
    return _MASK_DT[t.dtype]


TD_ALGOS = {"auto": 0, "sequential": 1, "wave": 2}  # include/t2omca.h T2O_TD_*


def _td_call(what, args_cls, qtot, qtot_tgt, reward, terminated, filled, per_weight, gamma, td_lambda, mask_sum,
             algo, mask_sum_acc, **extra):
    """The host checks, outputs and argument struct td_loss and td_qlambda share."""
    _dev(qtot, qtot_tgt, reward, per_weight, mask_sum_acc)
    for m in (terminated, filled):  # any mask dtype of _MASK_DT, device-resident
        if m is not None and not m.is_cuda:
            raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
        _mask_dtype(m)
    B, T = qtot.shape
    dev = qtot.device
    assert qtot.is_contiguous() and qtot_tgt.is_contiguous() and qtot_tgt.shape[1] == T + 1
    out = dict(gq=torch.empty(B, T, device=dev), targets=torch.empty(B, T, device=dev),
               prio=torch.empty(B, device=dev), loss=torch.empty(2, device=dev))
    rs, ts, fs = _mstrides(reward), _mstrides(terminated), _mstrides(filled)
    a = args_cls(qtot=_p(qtot), qtot_tgt=_p(qtot_tgt), reward=_p(reward), rw_sb=rs[0], rw_st=rs[1],
                 term=_p(terminated), tm_sb=ts[0], tm_st=ts[1], filled=_p(filled), fl_sb=fs[0], fl_st=fs[1],
                 per_weight=_p(per_weight), gq=_p(out["gq"]), targets=_p(out["targets"]), prio=_p(out["prio"]),
                 loss=_p(out["loss"]), mask_sum_acc=_p(mask_sum_acc), gamma=float(gamma), td_lambda=float(td_lambda),
                 mask_sum=float(mask_sum), term_dtype=_mask_dtype(terminated), filled_dtype=_mask_dtype(filled),
                 algo=TD_ALGOS[algo], B=B, T=T, **extra)
    check(getattr(lib(), "t2o_" + what)(ctypes.byref(a), stream_ptr()), what)
    return out


def td_loss(qtot, qtot_tgt, reward, terminated=None, filled=None, per_weight=None, gamma=0.99,
            td_lambda=0.6, mask_sum=0.0, algo="auto", mask_sum_acc=None):
    """TD(λ) targets / loss / grads / priorities (PyMARL2 NQLearner contract).
    qtot [B,T], qtot_tgt [B,T+1]; reward [B, >=T] float view; terminated / filled
    [B, >=T] views in float32, uint8/bool, int32 or int64 (read in place).
    algo: "sequential" (the reference's backward order, one thread per episode),
    "wave" (one wave per episode, suffix scan) or "auto" (the library default).
    mask_sum_acc: optional 1-float device tensor that receives += Σ mask.
    Returns dict(gq [B,T], targets [B,T], prio [B], loss [2])."""
    return _td_call("td_loss", TDArgs, qtot, qtot_tgt, reward, terminated, filled, per_weight, gamma, td_lambda,
                    mask_sum, algo, mask_sum_acc)


def td_qlambda(qtot, qtot_tgt, qtot_taken, reward, terminated=None, filled=None, per_weight=None, gamma=0.99,
               td_lambda=0.6, mask_sum=0.0, algo="auto", mask_sum_acc=None):
    """td_loss with Peng's Q(λ) targets (include/t2omca.h t2o_td_qlambda; PyMARL2
    NQLearner with q_lambda: True): qtot_taken [B, T] or [B, T+1] (a view with any
    row stride, unit inner stride; steps 0..T-1 are read) is the target mixer's
    output on the target Q of the taken actions, and each step's reward gains
    qtot_tgt[t] - qtot_taken[t].  Everything else, the returned dict included, as
    td_loss; the sequential kernel takes T <= 4095."""
    _dev(qtot_taken)
    B, T = qtot.shape
    if qtot_taken.dim() != 2 or qtot_taken.shape[0] != B or qtot_taken.shape[1] not in (T, T + 1):
        raise ValueError(f"td_qlambda: qtot_taken must be [{B}, {T}] or [{B}, {T + 1}], got {tuple(qtot_taken.shape)}")
    if qtot_taken.dtype != torch.float32:
        raise TypeError(f"td_qlambda: qtot_taken must be float32, got {qtot_taken.dtype}")
    if qtot_taken.stride(1) != 1 or (B > 1 and qtot_taken.stride(0) < T):
        raise ValueError(f"td_qlambda: qtot_taken needs a unit inner stride and rows that do not overlap, got "
                         f"strides {tuple(qtot_taken.stride())}")
    qk_sb = qtot_taken.stride(0) if B > 1 else max(qtot_taken.stride(0), T)
    return _td_call("td_qlambda", TDQLambdaArgs, qtot, qtot_tgt, reward, terminated, filled, per_weight, gamma,
                    td_lambda, mask_sum, algo, mask_sum_acc, qtot_taken=_p(qtot_taken), qk_sb=qk_sb)


def adam_step(params, grads, exp_avg, exp_avg_sq, step, *, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
              weight_decay=0.0, max_grad_norm=10.0, workspace=None, grad_div=None, grad_norm_out=None):
    """In-place clip_grad_norm_ + Adam on flat fp32 buffers (grads divided by the
    device scalar grad_div first, if given)."""
    _dev(params, grads, exp_avg, exp_avg_sq, workspace, grad_div, grad_norm_out)
    n = params.numel()
    if workspace is None:
        workspace = torch.empty(int(lib().t2o_adam_workspace_floats()), device=params.device)
    check(lib().t2o_adam_step(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), ptr(workspace), n,
                              float(lr), float(betas[0]), float(betas[1]), float(eps),
                              float(weight_decay), float(max_grad_norm), int(step), ptr(grad_div),
                              ptr(grad_norm_out),
                              stream_ptr()), "adam_step")


def rmsprop_step(params, grads, square_avg, *, lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=0.0, max_grad_norm=10.0,
                 workspace=None, grad_div=None, grad_norm_out=None):
    """In-place clip_grad_norm_ + RMSprop (torch.optim.RMSprop, momentum 0, not
    centered) on flat fp32 buffers; clip, grad_div and grad_norm_out as adam_step."""
    _dev(params, grads, square_avg, workspace, grad_div, grad_norm_out)
    n = params.numel()
    if workspace is None:
        workspace = torch.empty(int(lib().t2o_adam_workspace_floats()), device=params.device)
    check(lib().t2o_rmsprop_step(ptr(params), ptr(grads), ptr(square_avg), ptr(workspace), n, float(lr),
                                 float(alpha), float(eps), float(weight_decay), float(max_grad_norm), ptr(grad_div),
                                 ptr(grad_norm_out), stream_ptr()), "rmsprop_step")


# ---- the NoisyNet Q head (include/t2omca.h t2o_noise_normal / t2o_noisy_head_*) ----

def _f32c(name, t, shape=None):
    if not t.is_cuda:
        raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise TypeError(f"{name}: expected a dense float32 tensor" + (f" of shape {tuple(shape)}" if shape else "") +
                        f", got {tuple(t.shape)} {t.dtype}")
    return t


def noise_normal(E, NA, T, seed, kind, counter, device=None, out=None, steps=None):
    """The ε block of a noisy head (t2o_noise_normal): eps_w [T, NA, E], eps_b [T, NA],
    one launch; kind one of _lib.NOISE_KINDS (or its number), counter the caller's
    call count.  steps=(t0, t1) writes only those rows of `out`=(eps_w, eps_b)."""
    if out is None:
        out = (torch.empty(T, NA, E, device=device), torch.empty(T, NA, device=device))
    eps_w, eps_b = out
    _f32c("noise_normal: eps_w", eps_w, (T, NA, E))
    _f32c("noise_normal: eps_b", eps_b, (T, NA))
    t0, t1 = steps if steps is not None else (0, T)
    a = _lib.NoiseArgs(eps_w=_p(eps_w), eps_b=_p(eps_b), seed=int(seed) & ((1 << 64) - 1), counter=int(counter),
                       kind=_lib.NOISE_KINDS.get(kind, kind), E=E, NA=NA, T=T, t0=int(t0), t1=int(t1))
    check(lib().t2o_noise_normal(ctypes.byref(a), stream_ptr(eps_w.device)), "noise_normal")
    return eps_w, eps_b


def noisy_head_fwd(h, q, u_w, u_b, s_w=None, s_b=None, eps=None, steps=None, timer=None, launcher=False):
    """q[b, t] = (u_w + s_w ⊙ eps_w[t]) h[b, t] + (u_b + s_b ⊙ eps_b[t]) over steps
    [t0, t1) (default: every step of q), written into q [B, q_ts, A, NA] over what the
    agent unroll left there; h [B, h_ts, A, E] its hidden states.  eps=(eps_w, eps_b)
    (noise_normal's) or None: the mean head."""
    B, h_ts, A, E = h.shape
    q_ts, NA = q.shape[1], q.shape[3]
    _f32c("noisy_head_fwd: h", h)
    _f32c("noisy_head_fwd: q", q, (B, q_ts, A, NA))
    _f32c("noisy_head_fwd: u_w", u_w, (NA, E))
    _f32c("noisy_head_fwd: u_b", u_b, (NA,))
    eps_w = eps_b = None
    if eps is not None:
        eps_w, eps_b = eps
        _f32c("noisy_head_fwd: s_w", s_w, (NA, E))
        _f32c("noisy_head_fwd: s_b", s_b, (NA,))
        _f32c("noisy_head_fwd: eps_w", eps_w, (eps_w.shape[0], NA, E))
        _f32c("noisy_head_fwd: eps_b", eps_b, (eps_w.shape[0], NA))
    a = _lib.NoisyFwdArgs(h=_p(h), u_w=_p(u_w), u_b=_p(u_b), s_w=_p(s_w), s_b=_p(s_b), eps_w=_p(eps_w),
                          eps_b=_p(eps_b), q=_p(q), h_ts=h_ts, q_ts=q_ts, B=B, A=A, E=E, NA=NA)
    fn = lib().t2o_noisy_head_fwd
    n_eps = eps_w.shape[0] if eps_w is not None else None

    def go(t0, t1):
        if n_eps is not None and t1 > n_eps:
            raise ValueError(f"noisy_head_fwd: steps up to {t1}, the noise covers {n_eps}")
        a.t0, a.t1 = int(t0), int(t1)
        _mark(timer, "begin:noisy_fwd")
        check(fn(ctypes.byref(a), stream_ptr(h.device)), "noisy_head_fwd")
        _mark(timer, "end:noisy_fwd")
    if launcher:
        return go
    go(*(steps if steps is not None else (0, min(h_ts, q_ts))))
    return q


def noisy_head_parts(B, A):
    """Row parts per step of the head backward's weight-gradient partials."""
    n = int(lib().t2o_noisy_head_parts(int(B), int(A)))
    if n < 1:
        raise ValueError(f"noisy_head_parts: bad shape B={B} A={A}")
    return n


def noisy_head_bwd(gchosen, actions, h, u_w, s_w=None, eps_w=None, gh_in=None, gh_out=None, gpart=None, steps=None,
                   timer=None, launcher=False):
    """Backward of the head at the taken actions over steps [t_lo, t_hi) (default all T):
    gh_out [B, T, A, E] = gh_in + gchosen · W_t[action] and the weight-gradient
    partials gpart [T, P, NA, E+1] of those steps (noisy_head_wgrad sums them once
    every step is in).  gchosen [B, T, A]; actions int64 [B, >= T, A]; h [B, >= T, A, E].
    Returns (gh_out, gpart)."""
    B, T, A = gchosen.shape
    E, NA = h.shape[3], u_w.shape[0]
    _f32c("noisy_head_bwd: gchosen", gchosen)
    _f32c("noisy_head_bwd: h", h, (B, h.shape[1], A, E))
    _f32c("noisy_head_bwd: u_w", u_w, (NA, E))
    if not actions.is_cuda or actions.dtype != torch.int64 or actions.stride(2) != 1 or actions.shape[1] < T:
        raise TypeError("noisy_head_bwd: actions must be an int64 HIP tensor [B, >= T, A] with unit agent stride")
    if eps_w is not None:
        _f32c("noisy_head_bwd: s_w", s_w, (NA, E))
        _f32c("noisy_head_bwd: eps_w", eps_w, (eps_w.shape[0], NA, E))
        if eps_w.shape[0] < T:
            raise ValueError(f"noisy_head_bwd: {T} steps, the noise covers {eps_w.shape[0]}")
    P = noisy_head_parts(B, A)
    if gh_out is None:
        gh_out = torch.empty(B, T, A, E, device=h.device)
    if gpart is None:
        gpart = torch.empty(T, P, NA, E + 1, device=h.device)
    _f32c("noisy_head_bwd: gh_out", gh_out, (B, T, A, E))
    _f32c("noisy_head_bwd: gpart", gpart, (T, P, NA, E + 1))
    if gh_in is not None:
        _f32c("noisy_head_bwd: gh_in", gh_in, (B, T, A, E))
    a = _lib.NoisyBwdArgs(gchosen=_p(gchosen), actions=_p(actions), act_sb=actions.stride(0), act_st=actions.stride(1),
                          h=_p(h), u_w=_p(u_w), s_w=_p(s_w), eps_w=_p(eps_w), gh_in=_p(gh_in), gh_out=_p(gh_out),
                          gpart=_p(gpart), h_ts=h.shape[1], B=B, T=T, A=A, E=E, NA=NA)
    fn = lib().t2o_noisy_head_bwd

    def go(t_lo, t_hi):
        a.t_lo, a.t_hi = int(t_lo), int(t_hi)
        _mark(timer, "begin:noisy_bwd")
        check(fn(ctypes.byref(a), stream_ptr(h.device)), "noisy_head_bwd")
        _mark(timer, "end:noisy_bwd")
    if launcher:
        return go, gh_out, gpart
    go(*(steps if steps is not None else (0, T)))
    return gh_out, gpart


def noisy_head_wgrad(gpart, B, A, du_w, du_b, ds_w=None, ds_b=None, eps=None, timer=None):
    """du_w, du_b += Σ_t gpart[t];  ds_w, ds_b += Σ_t eps[t] ⊙ gpart[t]  (fixed order;
    the slots are views of the caller's flat gradient).  eps None: the mean head."""
    T, P, NA, E1 = gpart.shape
    E = E1 - 1
    _f32c("noisy_head_wgrad: gpart", gpart, (T, noisy_head_parts(B, A), NA, E1))
    _f32c("noisy_head_wgrad: du_w", du_w)
    _f32c("noisy_head_wgrad: du_b", du_b)
    assert du_w.numel() == NA * E and du_b.numel() == NA
    eps_w = eps_b = None
    if eps is not None:
        eps_w, eps_b = eps
        _f32c("noisy_head_wgrad: eps_w", eps_w, (eps_w.shape[0], NA, E))
        _f32c("noisy_head_wgrad: eps_b", eps_b, (eps_w.shape[0], NA))
        _f32c("noisy_head_wgrad: ds_w", ds_w)
        _f32c("noisy_head_wgrad: ds_b", ds_b)
        assert eps_w.shape[0] >= T and ds_w.numel() == NA * E and ds_b.numel() == NA
    a = _lib.NoisyWgradArgs(gpart=_p(gpart), eps_w=_p(eps_w), eps_b=_p(eps_b), du_w=_p(du_w), du_b=_p(du_b),
                            ds_w=_p(ds_w), ds_b=_p(ds_b), B=int(B), T=T, A=int(A), E=E, NA=NA)
    _mark(timer, "begin:noisy_wgrad")
    check(lib().t2o_noisy_head_wgrad(ctypes.byref(a), stream_ptr(gpart.device)), "noisy_head_wgrad")
    _mark(timer, "end:noisy_wgrad")


def select_actions(q, avail, epsilon=0.0, seed=0, counter=0, out=None):
    """ε-greedy actions (include/t2omca.h t2o_select_actions): q f32 [..., NA] and
    avail i32 [..., NA], dense; returns int64 [...] (or writes `out`)."""
    _dev(q)
    if avail.dtype != torch.int32 or not avail.is_cuda:
        raise TypeError("avail must be an int32 HIP-device tensor")
    NA = q.shape[-1]
    assert q.is_contiguous() and avail.is_contiguous() and avail.shape == q.shape
    rows = q.numel() // NA
    if out is None:
        out = torch.empty(q.shape[:-1], dtype=torch.int64, device=q.device)
    assert out.is_contiguous() and out.numel() == rows and out.dtype == torch.int64
    check(lib().t2o_select_actions(ptr(q), ptr(avail), ptr(out), rows, NA, float(epsilon),
                                   ctypes.c_uint64(int(seed) & ((1 << 64) - 1)), int(counter), stream_ptr()),
          "select_actions")
    return out


def _cu_count():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def lds_fill(word, workgroups=None):
    """Diagnostic (include/t2omca.h t2o_probe_lds_fill): `workgroups` workgroups of one
    per CU (160 KB of dynamic LDS each; default 4x the CU count) store the 32-bit
    `word` into every word of their LDS, on the current stream."""
    n = 4 * _cu_count() if workgroups is None else int(workgroups)
    check(lib().t2o_probe_lds_fill(int(word) & 0xFFFFFFFF, n, stream_ptr()), "probe_lds_fill")


def lds_census(word, workgroups=None):
    """Diagnostic (t2o_probe_lds_census): int32 [workgroups] (default the CU count),
    per workgroup the number of words of its 160 KB of LDS that differ from `word`;
    the kernel writes nothing to LDS."""
    n = _cu_count() if workgroups is None else int(workgroups)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    check(lib().t2o_probe_lds_census(int(word) & 0xFFFFFFFF, n, ptr(out), stream_ptr()), "probe_lds_census")
    return out


def obs_expand(wire, snap_n, snap, out=None, out64=None):
    """Dense normalised obs from the compact wire format (SURVEY.md §8 f3,
    include/t2omca.h t2o_obs_expand).  wire int32 [B, T1, A, 4] (episode / step
    strides free, agent rows dense), snap_n int64 [B], snap f64 [B, 2, 9A];
    returns f32 [B, T1, A, 9A] (or writes `out`, any episode / step strides with
    dense steps); out64 optionally receives the fp64 values (dense)."""
    for t in (wire, snap_n, snap, out, out64):
        if t is not None and not t.is_cuda:
            raise RuntimeError("obs_expand needs HIP-device tensors (no CPU fallback)")
    if wire.dtype != torch.int32 or snap_n.dtype != torch.int64 or snap.dtype != torch.float64:
        raise TypeError("obs_expand: wire int32, snap_n int64, snap float64")
    B, T1, A, four = wire.shape
    assert four == 4 and wire.stride(3) == 1 and wire.stride(2) == 4
    assert snap_n.shape == (B,) and snap.shape == (B, 2, 9 * A) and snap.is_contiguous() and snap_n.is_contiguous()
    if out is None:
        out = torch.empty(B, T1, A, 9 * A, device=wire.device)
    assert out.dtype == torch.float32 and out.shape == (B, T1, A, 9 * A)
    assert out.stride(3) == 1 and out.stride(2) == 9 * A
    if out64 is not None:
        assert out64.dtype == torch.float64 and out64.shape == out.shape and out64.is_contiguous()
    check(lib().t2o_obs_expand(ptr(wire), wire.stride(0), wire.stride(1), ptr(snap_n), ptr(snap), ptr(out),
                               out.stride(0), out.stride(1), ptr(out64), B, T1, A, stream_ptr(wire.device)),
          "obs_expand")
    return out


def td_stats(qtot, targets, terminated=None, filled=None, out=None):
    """The masked sums the learner logs from (include/t2omca.h t2o_td_stats): qtot /
    targets f32 [B,T] dense, terminated / filled [B, >=T] views as td_loss takes
    them (read in place; None: none terminated / all filled).  Returns `out`, f64
    [4] = [Σm, Σ|q-tgt|m, Σq·m, Σtgt·m] (overwritten), summed in fp64 in an order
    fixed by (B, T).  One launch, no host read."""
    _dev(qtot, targets)
    for m in (terminated, filled):
        if m is not None and not m.is_cuda:
            raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
    B, T = qtot.shape
    assert qtot.is_contiguous() and targets.is_contiguous() and targets.shape == qtot.shape
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=qtot.device)
    assert out.dtype == torch.float64 and out.numel() == 4 and out.is_contiguous() and out.is_cuda
    ts, fs = _mstrides(terminated), _mstrides(filled)
    a = _lib.TDStatsArgs(qtot=_p(qtot), targets=_p(targets), term=_p(terminated), tm_sb=ts[0], tm_st=ts[1],
                         filled=_p(filled), fl_sb=fs[0], fl_st=fs[1], term_dtype=_mask_dtype(terminated),
                         filled_dtype=_mask_dtype(filled), B=B, T=T, out=_p(out))
    check(lib().t2o_td_stats(ctypes.byref(a), stream_ptr(qtot.device)), "td_stats")
    return out


def episode_stats(reward, info, terminated, returns, acc):
    """acc += the runner's statistics of one finished run (include/t2omca.h
    t2o_episode_stats): reward f64 [n], info f64 [n, 6] (env.INFO_KEYS columns),
    terminated uint8 [n], returns f64 [n], acc f64 [EP_STATS], all dense on the
    device.  One launch, no host read."""
    n = returns.numel()
    for t, dt, shape in ((reward, torch.float64, (n,)), (info, torch.float64, (n, 6)),
                         (terminated, torch.uint8, (n,)), (returns, torch.float64, (n,)),
                         (acc, torch.float64, (_lib.EP_STATS,))):
        if not t.is_cuda:
            raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise TypeError(f"episode_stats: expected a dense {shape} {dt} tensor, got {tuple(t.shape)} {t.dtype}")
    check(lib().t2o_episode_stats(ptr(reward), ptr(info), ptr(terminated), ptr(returns), n, ptr(acc),
                                  stream_ptr(acc.device)), "episode_stats")
    return acc


# ---- the QMIX and VDN mixers (include/t2omca.h t2o_q_select / t2o_qmix_* / t2o_vdn_bwd) ----

@dataclass(frozen=True)
class QmixShape:
    """Sizes of a QMixer (modules.QMixer): agents, state width, mixing_embed_dim M,
    hypernet_embed H, and the positivity function of the hypernetwork weights."""
    A: int
    S: int
    M: int = 32
    H: int = 64
    pos_func: int = 0
    pos_beta: float = 1.0

    @property
    def n_params(self):
        return int(lib().t2o_qmix_param_count(self.A, self.S, self.M, self.H))

    @property
    def agents(self):
        return self.A


QMIX_LIMITS = "1 <= n_agents <= 64, 1 <= state width <= 1024, mixing_embed_dim in {16, 32}, hypernet_embed in {32, 64}"


def qmix_param_blocks(A, S, M=32, H=64):
    """(state_dict key, shape) of a QMixer's parameters in their flat order."""
    return [("hyper_w1.0.weight", (H, S)), ("hyper_w1.0.bias", (H,)), ("hyper_w1.2.weight", (A * M, H)),
            ("hyper_w1.2.bias", (A * M,)), ("hyper_b1.0.weight", (M, S)), ("hyper_b1.0.bias", (M,)),
            ("hyper_w2.0.weight", (H, S)), ("hyper_w2.0.bias", (H,)), ("hyper_w2.2.weight", (M, H)),
            ("hyper_w2.2.bias", (M,)), ("hyper_b2.0.weight", (M, S)), ("hyper_b2.0.bias", (M,)),
            ("hyper_b2.2.weight", (1, M)), ("hyper_b2.2.bias", (1,))]


def _i64c(name, t):
    if not t.is_cuda:
        raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
    if t.dtype != torch.int64 or t.dim() != 3 or t.stride(2) != 1:
        raise TypeError(f"{name}: expected an int64 tensor [B, >= T, A] with unit agent stride")
    return t


def q_select(q_on, *, qmode_on=1, actions=None, avail=None, T_on=None, q_tg=None, qmode_tg=2, T_tg=None,
             want_y=False, outs=None, timer=None):
    """The learner's chosen-Q gather / double-Q selection (t2o_q_select).  q_on / q_tg
    [B, q_ts, A, NA] dense float32; actions int64 [B, >= T, A] (any episode / step
    strides); avail int32 [B, >= T, A, NA] or None.  qmode 1: the network's Q at the
    actions; 2: at the argmax of q_on masked by avail (ties: the lowest index).  The
    first network covers t < T_on, the second (q_tg given) t < T_tg.  Returns
    (qv_on, y_on) or ((qv_on, y_on), (qv_tg, y_tg)); y = Σ_a qv when want_y, else None.
    outs: the same structure of preallocated dense tensors."""
    _f32c("q_select: q_on", q_on)
    B, q_ts, A, NA = q_on.shape
    T_on = int(T_on or q_ts)
    two = q_tg is not None
    if two:
        _f32c("q_select: q_tg", q_tg, (B, q_ts, A, NA))
        T_tg = int(T_tg or q_ts)
    if qmode_on not in (1, 2) or (two and qmode_tg not in (1, 2)):
        raise ValueError("q_select: qmode must be 1 (gather at the actions) or 2 (double-Q argmax)")
    if actions is not None:
        _i64c("q_select: actions", actions)
    elif qmode_on == 1 or (two and qmode_tg == 1):
        raise ValueError("q_select: qmode 1 needs the actions")
    if avail is not None:
        if not avail.is_cuda:
            raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
        if avail.dtype != torch.int32 or avail.stride(3) != 1 or avail.stride(2) != NA:
            raise TypeError("q_select: avail must be int32 [B, >= T, A, NA] with dense [A, NA] rows")
    dev = q_on.device

    def alloc(T):
        return (torch.empty(B, T, A, device=dev), torch.empty(B, T, device=dev) if want_y else None)
    if outs is None:
        outs = (alloc(T_on), alloc(T_tg)) if two else alloc(T_on)
    (qv_on, y_on), (qv_tg, y_tg) = (outs if two else (outs, (None, None)))
    _f32c("q_select: qv_on", qv_on, (B, T_on, A))
    if y_on is not None:
        _f32c("q_select: y_on", y_on, (B, T_on))
    if two:
        _f32c("q_select: qv_tg", qv_tg, (B, T_tg, A))
        if y_tg is not None:
            _f32c("q_select: y_tg", y_tg, (B, T_tg))
    act_sb, act_st = _mstrides(actions)
    av_sb, av_st = _mstrides(avail)
    a = _lib.QSelectArgs(q_on=_p(q_on), q_tg=_p(q_tg), q_ts=q_ts, n_actions=NA, actions=_p(actions), act_sb=act_sb,
                         act_st=act_st, avail=_p(avail), av_sb=av_sb, av_st=av_st, qmode_on=qmode_on,
                         qmode_tg=qmode_tg if two else 0, qv_on=_p(qv_on), qv_tg=_p(qv_tg), y_on=_p(y_on),
                         y_tg=_p(y_tg), B=B, T_on=T_on, T_tg=T_tg if two else 0, A=A)
    _mark(timer, "begin:q_select")
    check(lib().t2o_q_select(ctypes.byref(a), stream_ptr(dev)), "q_select")
    _mark(timer, "end:q_select")
    return outs


def _qmix_states(name, states, B, S):
    if not states.is_cuda:
        raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
    if states.dtype != torch.float32 or states.dim() != 3 or states.shape[0] != B or states.shape[2] != S or \
            states.stride(2) != 1:
        raise TypeError(f"{name}: states must be float32 [B, >= T, {S}] with unit feature stride")
    return states


def qmix_fwd(shape: QmixShape, params_on, states, qv_on, *, params_tg=None, qv_tg=None, outs=None, timer=None):
    """QMIX forward (t2o_qmix_fwd) of one or two networks in one launch.  params_*:
    the mixer's flat parameters (dense float32, shape.n_params); states [B, >= T, S]
    (any episode / step strides); qv_* [B, T_*, A] dense.  Returns y_on [B, T_on], or
    (y_on, y_tg)."""
    B, T_on, A = qv_on.shape
    _f32c("qmix_fwd: params_on", params_on, (shape.n_params,))
    _f32c("qmix_fwd: qv_on", qv_on, (B, T_on, shape.A))
    _qmix_states("qmix_fwd", states, B, shape.S)
    two = params_tg is not None
    T_tg = 0
    if two:
        T_tg = qv_tg.shape[1]
        _f32c("qmix_fwd: params_tg", params_tg, (shape.n_params,))
        _f32c("qmix_fwd: qv_tg", qv_tg, (B, T_tg, shape.A))
    if states.shape[1] < max(T_on, T_tg):
        raise ValueError(f"qmix_fwd: {max(T_on, T_tg)} steps, the states cover {states.shape[1]}")
    dev = qv_on.device
    if outs is None:
        outs = (torch.empty(B, T_on, device=dev), torch.empty(B, T_tg, device=dev)) if two else \
            torch.empty(B, T_on, device=dev)
    y_on, y_tg = outs if two else (outs, None)
    _f32c("qmix_fwd: y_on", y_on, (B, T_on))
    if two:
        _f32c("qmix_fwd: y_tg", y_tg, (B, T_tg))
    a = _lib.QmixFwdArgs(params_on=_p(params_on), params_tg=_p(params_tg), states=_p(states), st_sb=states.stride(0),
                         st_st=states.stride(1), qv_on=_p(qv_on), qv_tg=_p(qv_tg), y_on=_p(y_on), y_tg=_p(y_tg),
                         B=B, T_on=T_on, T_tg=T_tg, A=shape.A, S=shape.S, M=shape.M, H=shape.H,
                         pos_func=shape.pos_func, pos_beta=float(shape.pos_beta))
    _mark(timer, "begin:qmix_fwd")
    check(lib().t2o_qmix_fwd(ctypes.byref(a), stream_ptr(dev)), "qmix_fwd")
    _mark(timer, "end:qmix_fwd")
    return outs


def qmix_slab_count(B, T):
    n = int(lib().t2o_qmix_bwd_slabs(int(B), int(T)))
    if n < 1:
        raise ValueError(f"qmix_slab_count: bad shape B={B} T={T}")
    return n


def qmix_work_floats(shape: QmixShape, B, T):
    n = int(lib().t2o_qmix_bwd_work_floats(int(B), int(T), shape.M, shape.H))
    if n < 1:
        raise ValueError(f"qmix_work_floats: bad shape B={B} T={T} M={shape.M} H={shape.H}")
    return n


def qmix_bwd(shape: QmixShape, params, states, qv, gy, *, gqv=None, slabs=None, work=None, timer=None,
             launcher=False):
    """QMIX backward (t2o_qmix_bwd) of one network: dL/dqv [B, T, A] and the partial
    weight-gradient slabs [qmix_slab_count(B, T), n_params] (sum them with
    reduce_slabs).  Returns (gqv, slabs, nslab); launcher: (go, gqv, slabs, nslab) with
    go(phase) — 1 the rows (gqv and the work buffer), 2 the weight gradients."""
    B, T, A = qv.shape
    _f32c("qmix_bwd: params", params, (shape.n_params,))
    _f32c("qmix_bwd: qv", qv, (B, T, shape.A))
    _f32c("qmix_bwd: gy", gy, (B, T))
    _qmix_states("qmix_bwd", states, B, shape.S)
    if states.shape[1] < T:
        raise ValueError(f"qmix_bwd: {T} steps, the states cover {states.shape[1]}")
    dev = qv.device
    nslab, nwork = qmix_slab_count(B, T), qmix_work_floats(shape, B, T)
    if gqv is None:
        gqv = torch.empty(B, T, A, device=dev)
    if slabs is None:
        slabs = torch.empty(nslab * shape.n_params, device=dev)
    if work is None:
        work = torch.empty(nwork, device=dev)
    _f32c("qmix_bwd: gqv", gqv, (B, T, A))
    _f32c("qmix_bwd: slabs", slabs)
    _f32c("qmix_bwd: work", work)
    if slabs.numel() < nslab * shape.n_params or work.numel() < nwork:
        raise ValueError("qmix_bwd: the slab or work buffer is too small")
    a = _lib.QmixBwdArgs(params=_p(params), states=_p(states), st_sb=states.stride(0), st_st=states.stride(1),
                         qv=_p(qv), gy=_p(gy), gqv=_p(gqv), gslabs=_p(slabs), work=_p(work), work_floats=work.numel(),
                         max_slabs=slabs.numel() // shape.n_params, B=B, T=T, A=shape.A, S=shape.S, M=shape.M,
                         H=shape.H, pos_func=shape.pos_func, pos_beta=float(shape.pos_beta))
    fn = lib().t2o_qmix_bwd

    def go(phase=0):
        a.phase = int(phase)
        _mark(timer, "begin:qmix_bwd")
        check(fn(ctypes.byref(a), stream_ptr(dev)), "qmix_bwd")
        _mark(timer, "end:qmix_bwd")
    if launcher:
        return go, gqv, slabs, nslab
    go(0)
    return gqv, slabs, nslab


def vdn_fwd(qv, timer=None):
    """VDN forward y [B, T] = Σ_a qv[B, T, A], in agent order: the select kernel's row
    sum (qv as a one-action Q array, whose argmax is that action)."""
    _f32c("vdn_fwd: qv", qv)
    return q_select(qv.unsqueeze(3), qmode_on=2, want_y=True, timer=timer)[1]


def vdn_bwd(gy, gqv=None, A=None, timer=None):
    """VDN backward (t2o_vdn_bwd): gqv[b, t, a] = gy[b, t]."""
    _f32c("vdn_bwd: gy", gy)
    B, T = gy.shape
    if gqv is None:
        gqv = torch.empty(B, T, int(A), device=gy.device)
    _f32c("vdn_bwd: gqv", gqv, (B, T, gqv.shape[2]))
    _mark(timer, "begin:vdn_bwd")
    check(lib().t2o_vdn_bwd(_p(gy), _p(gqv), B, T, gqv.shape[2], stream_ptr(gy.device)), "vdn_bwd")
    _mark(timer, "end:vdn_bwd")
    return gqv


# ---- the QPLEX duelling mixer (include/t2omca.h t2o_qplex_*) ----

@dataclass(frozen=True)
class QplexShape:
    """Sizes of a QPlexMixer (modules.QPlexMixer): agents, state width, actions,
    hypernet_embed H, adv_hypernet_embed HA and num_kernel K."""
    A: int
    S: int
    NA: int
    H: int = 64
    HA: int = 64
    K: int = 4

    @property
    def n_params(self):
        return int(lib().t2o_qplex_param_count(self.A, self.S, self.NA, self.H, self.HA, self.K))

    @property
    def agents(self):
        return self.A


QPLEX_LIMITS = ("1 <= n_agents <= 64, 1 <= state width <= 1024, 1 <= n_actions <= 16, hypernet_embed and "
                "adv_hypernet_embed in {32, 64}, 1 <= num_kernel <= 10, adv_hypernet_layers == 2, weighted_head and "
                "is_minus_one True")


def qplex_param_blocks(A, S, NA, H=64, HA=64, K=4):
    """(state_dict key, shape) of a QPlexMixer's parameters in their flat order."""
    def net(name, n_in, hid, n_out):
        return [(f"{name}.0.weight", (hid, n_in)), (f"{name}.0.bias", (hid,)), (f"{name}.2.weight", (n_out, hid)),
                (f"{name}.2.bias", (n_out,))]
    out = net("hyper_w_final", S, H, A) + net("V", S, H, A)
    for name, n_in, n_out in (("key_extractors", S, 1), ("agents_extractors", S, A),
                              ("action_extractors", S + A * NA, A)):
        for k in range(K):
            out += net(f"si_weight.{name}.{k}", n_in, HA, n_out)
    return out


def _i32c(name, t, shape):
    if not t.is_cuda:
        raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
    if t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise TypeError(f"{name}: expected a dense int32 tensor of shape {tuple(shape)}, got {tuple(t.shape)} {t.dtype}")
    return t


def qplex_select(q_on, *, qmode_on=1, actions=None, avail=None, T_on=None, q_tg=None, qmode_tg=2, T_tg=None,
                 outs=None, timer=None):
    """q_select for the QPLEX mixer (t2o_qplex_select): per network the selected Q, the
    avail-masked maximum of the network's own Q and the action index used (int32), each
    [B, T_*, A].  Arguments as q_select.  Returns (qv, qmax, act), or a pair of them with
    two networks; outs: the same structure of preallocated dense tensors."""
    _f32c("qplex_select: q_on", q_on)
    B, q_ts, A, NA = q_on.shape
    T_on = int(T_on or q_ts)
    two = q_tg is not None
    if two:
        _f32c("qplex_select: q_tg", q_tg, (B, q_ts, A, NA))
        T_tg = int(T_tg or q_ts)
    if qmode_on not in (1, 2) or (two and qmode_tg not in (1, 2)):
        raise ValueError("qplex_select: qmode must be 1 (gather at the actions) or 2 (double-Q argmax)")
    if actions is not None:
        _i64c("qplex_select: actions", actions)
    elif qmode_on == 1 or (two and qmode_tg == 1):
        raise ValueError("qplex_select: qmode 1 needs the actions")
    if avail is not None:
        if not avail.is_cuda:
            raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
        if avail.dtype != torch.int32 or avail.stride(3) != 1 or avail.stride(2) != NA:
            raise TypeError("qplex_select: avail must be int32 [B, >= T, A, NA] with dense [A, NA] rows")
    dev = q_on.device

    def alloc(T):
        return (torch.empty(B, T, A, device=dev), torch.empty(B, T, A, device=dev),
                torch.empty(B, T, A, device=dev, dtype=torch.int32))
    if outs is None:
        outs = (alloc(T_on), alloc(T_tg)) if two else alloc(T_on)
    o_on, o_tg = outs if two else (outs, (None, None, None))
    for o, T in ((o_on, T_on),) + (((o_tg, T_tg),) if two else ()):
        _f32c("qplex_select: qv", o[0], (B, T, A))
        _f32c("qplex_select: qmax", o[1], (B, T, A))
        _i32c("qplex_select: act", o[2], (B, T, A))
    act_sb, act_st = _mstrides(actions)
    av_sb, av_st = _mstrides(avail)
    a = _lib.QplexSelectArgs(q_on=_p(q_on), q_tg=_p(q_tg), q_ts=q_ts, n_actions=NA, actions=_p(actions),
                             act_sb=act_sb, act_st=act_st, avail=_p(avail), av_sb=av_sb, av_st=av_st,
                             qmode_on=qmode_on, qmode_tg=qmode_tg if two else 0, qv_on=_p(o_on[0]), qv_tg=_p(o_tg[0]),
                             qmax_on=_p(o_on[1]), qmax_tg=_p(o_tg[1]), act_on=_p(o_on[2]), act_tg=_p(o_tg[2]),
                             B=B, T_on=T_on, T_tg=T_tg if two else 0, A=A)
    _mark(timer, "begin:qplex_select")
    check(lib().t2o_qplex_select(ctypes.byref(a), stream_ptr(dev)), "qplex_select")
    _mark(timer, "end:qplex_select")
    return outs


def _qplex_rows(name, shape, qv, qmax, act, need_adv=True):
    B, T, A = qv.shape
    _f32c(f"{name}: qv", qv, (B, T, shape.A))
    if qmax is None or act is None:
        if need_adv:
            raise ValueError(f"{name}: the advantage part needs qmax and act")
        return
    _f32c(f"{name}: qmax", qmax, (B, T, A))
    _i32c(f"{name}: act", act, (B, T, A))


def qplex_fwd(shape: QplexShape, params_on, states, qv_on, qmax_on=None, act_on=None, *, params_tg=None, qv_tg=None,
              qmax_tg=None, act_tg=None, parts=3, outs=None, timer=None):
    """QPLEX forward (t2o_qplex_fwd) of one or two networks in one launch.  params_*:
    the mixer's flat parameters (dense float32, shape.n_params, any 4-byte alignment);
    states [B, >= T, S] (any episode / step strides); qv_*, qmax_* float32 and act_*
    int32, [B, T_*, A] dense.  parts: 1 = y_v, 2 = y_adv, 3 = their sum.  Returns y_on
    [B, T_on], or (y_on, y_tg)."""
    if parts not in (1, 2, 3):
        raise ValueError("qplex_fwd: parts must be 1 (y_v), 2 (y_adv) or 3 (both)")
    B, T_on, A = qv_on.shape
    _f32c("qplex_fwd: params_on", params_on, (shape.n_params,))
    _qplex_rows("qplex_fwd", shape, qv_on, qmax_on, act_on, parts & 2)
    _qmix_states("qplex_fwd", states, B, shape.S)
    two = params_tg is not None
    T_tg = 0
    if two:
        T_tg = qv_tg.shape[1]
        _f32c("qplex_fwd: params_tg", params_tg, (shape.n_params,))
        _qplex_rows("qplex_fwd", shape, qv_tg, qmax_tg, act_tg, parts & 2)
    if states.shape[1] < max(T_on, T_tg):
        raise ValueError(f"qplex_fwd: {max(T_on, T_tg)} steps, the states cover {states.shape[1]}")
    dev = qv_on.device
    if outs is None:
        outs = (torch.empty(B, T_on, device=dev), torch.empty(B, T_tg, device=dev)) if two else \
            torch.empty(B, T_on, device=dev)
    y_on, y_tg = outs if two else (outs, None)
    _f32c("qplex_fwd: y_on", y_on, (B, T_on))
    if two:
        _f32c("qplex_fwd: y_tg", y_tg, (B, T_tg))
    a = _lib.QplexFwdArgs(params_on=_p(params_on), params_tg=_p(params_tg), states=_p(states), st_sb=states.stride(0),
                          st_st=states.stride(1), qv_on=_p(qv_on), qv_tg=_p(qv_tg), qmax_on=_p(qmax_on),
                          qmax_tg=_p(qmax_tg), act_on=_p(act_on), act_tg=_p(act_tg), y_on=_p(y_on), y_tg=_p(y_tg),
                          B=B, T_on=T_on, T_tg=T_tg, parts=parts, A=shape.A, S=shape.S, NA=shape.NA, H=shape.H,
                          HA=shape.HA, K=shape.K)
    _mark(timer, "begin:qplex_fwd")
    check(lib().t2o_qplex_fwd(ctypes.byref(a), stream_ptr(dev)), "qplex_fwd")
    _mark(timer, "end:qplex_fwd")
    return outs


def qplex_slab_count(B, T):
    n = int(lib().t2o_qplex_bwd_slabs(int(B), int(T)))
    if n < 1:
        raise ValueError(f"qplex_slab_count: bad shape B={B} T={T}")
    return n


def qplex_work_floats(shape: QplexShape, B, T):
    n = int(lib().t2o_qplex_bwd_work_floats(int(B), int(T), shape.A, shape.H, shape.HA, shape.K))
    if n < 1:
        raise ValueError(f"qplex_work_floats: bad shape B={B} T={T} {shape}")
    return n


def qplex_bwd(shape: QplexShape, params, states, qv, qmax, act, gy, *, parts=3, gqv=None, slabs=None, work=None,
              timer=None, launcher=False):
    """QPLEX backward (t2o_qplex_bwd) of one network, of Σ gy · y(parts): dL/dqv
    [B, T, A] (= gy · w; zeros without part 1) and the partial weight-gradient slabs
    [qplex_slab_count(B, T), n_params] (sum them with reduce_slabs).  Returns (gqv, slabs,
    nslab); launcher: (go, gqv, slabs, nslab) with go(phase) — 1 the rows (gqv and the
    work buffer), 2 the weight gradients."""
    if parts not in (1, 2, 3):
        raise ValueError("qplex_bwd: parts must be 1 (y_v), 2 (y_adv) or 3 (both)")
    B, T, A = qv.shape
    _f32c("qplex_bwd: params", params, (shape.n_params,))
    _qplex_rows("qplex_bwd", shape, qv, qmax, act)
    _f32c("qplex_bwd: gy", gy, (B, T))
    _qmix_states("qplex_bwd", states, B, shape.S)
    if states.shape[1] < T:
        raise ValueError(f"qplex_bwd: {T} steps, the states cover {states.shape[1]}")
    dev = qv.device
    nslab, nwork = qplex_slab_count(B, T), qplex_work_floats(shape, B, T)
    if gqv is None:
        gqv = torch.empty(B, T, A, device=dev)
    if slabs is None:
        slabs = torch.empty(nslab * shape.n_params, device=dev)
    if work is None:
        work = torch.empty(nwork, device=dev)
    _f32c("qplex_bwd: gqv", gqv, (B, T, A))
    _f32c("qplex_bwd: slabs", slabs)
    _f32c("qplex_bwd: work", work)
    if slabs.numel() < nslab * shape.n_params or work.numel() < nwork:
        raise ValueError("qplex_bwd: the slab or work buffer is too small")
    a = _lib.QplexBwdArgs(params=_p(params), states=_p(states), st_sb=states.stride(0), st_st=states.stride(1),
                          qv=_p(qv), qmax=_p(qmax), act=_p(act), gy=_p(gy), gqv=_p(gqv), gslabs=_p(slabs),
                          work=_p(work), work_floats=work.numel(), max_slabs=slabs.numel() // shape.n_params,
                          parts=parts, B=B, T=T, A=shape.A, S=shape.S, NA=shape.NA, H=shape.H, HA=shape.HA, K=shape.K)
    fn = lib().t2o_qplex_bwd

    def go(phase=0):
        a.phase = int(phase)
        _mark(timer, "begin:qplex_bwd")
        check(fn(ctypes.byref(a), stream_ptr(dev)), "qplex_bwd")
        _mark(timer, "end:qplex_bwd")
    if launcher:
        return go, gqv, slabs, nslab
    go(0)
    return gqv, slabs, nslab


# ---- the GRU agent of the QMIX baselines (include/t2omca.h t2o_rnn_*) ----

RNN_HIDDEN = (32, 64)
RNN_LIMITS = "1 <= n_agents <= 64, 1 <= input width <= 656, 1 <= n_actions <= 16, rnn_hidden_dim in {32, 64}"


@dataclass(frozen=True)
class RnnShape:
    """Sizes of an RNNAgent (modules.RNNAgent): agents, the flattened observation's
    width, actions, rnn_hidden_dim H, and which one-hots the input carries."""
    A: int
    OBS: int
    NA: int
    H: int = 64
    last_action: bool = True
    agent_id: bool = True

    @property
    def IN(self):
        return self.OBS + (self.NA if self.last_action else 0) + (self.A if self.agent_id else 0)

    @property
    def E(self):
        """The hidden state's width (what NetShape calls E)."""
        return self.H

    @property
    def n_params(self):
        return int(lib().t2o_rnn_param_count(self.IN, self.H, self.NA))

    @property
    def agents(self):
        return self.A


def rnn_param_blocks(IN, H, NA):
    """(state_dict key, shape) of an RNNAgent's parameters in their flat order."""
    return [("fc1.weight", (H, IN)), ("fc1.bias", (H,)), ("rnn.weight_ih", (3 * H, H)), ("rnn.weight_hh", (3 * H, H)),
            ("rnn.bias_ih", (3 * H,)), ("rnn.bias_hh", (3 * H,)), ("fc2.weight", (NA, H)), ("fc2.bias", (NA,))]


def _rnn_obs(name, shape, obs):
    if not obs.is_cuda:
        raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
    if obs.dtype != torch.float32 or obs.dim() != 4 or obs.shape[2] != shape.A or obs.shape[3] != shape.OBS or \
            obs.stride(3) != 1 or obs.stride(2) != shape.OBS:
        raise TypeError(f"{name}: obs must be float32 [B, T, {shape.A}, {shape.OBS}] with dense [A, obs] rows")
    return obs


def _rnn_h0(name, shape, h0, B):
    if h0 is None:
        return None
    if not h0.is_cuda:
        raise RuntimeError("t2omca_amd ops need HIP-device tensors (no CPU fallback)")
    if h0.dtype != torch.float32 or tuple(h0.shape) != (B, shape.A, shape.H) or h0.stride(2) != 1 or \
            h0.stride(1) != shape.H or (B > 1 and h0.stride(0) % 4) or h0.data_ptr() % 16:
        raise TypeError(f"{name}: expected float32 [{B}, {shape.A}, {shape.H}] with dense [A, H] rows, 16-byte "
                        "aligned (any episode stride that is a multiple of 4)")
    return h0


def _rnn_actions(name, shape, actions, B, steps, need):
    if actions is None:
        if need:
            raise ValueError(f"{name}: the actions are needed")
        return None
    _i64c(f"{name}: actions", actions)
    if actions.shape[0] != B or actions.shape[2] != shape.A or actions.shape[1] < steps:
        raise ValueError(f"{name}: actions must cover [{B}, >= {steps}, {shape.A}], got {tuple(actions.shape)}")
    return actions


def rnn_agent_fwd(shape: RnnShape, params_on, obs, *, actions=None, act_shift=0, h0_on=None, params_tg=None,
                  h0_tg=None, steps=None, outs=None, want_x=True, timer=None):
    """GRU agent forward (t2o_rnn_fwd) of one or two networks sharing the inputs.
    params_*: flat parameters (dense float32, shape.n_params); obs [B, T1, A, OBS] (any
    episode / step strides, dense [A, OBS] rows); actions int64 [B, >= T1 - 1 + act_shift,
    A] (any episode / step strides) or None: the last-action one-hot of step t is that of
    actions[:, t - 1 + act_shift], zero where that index is negative or actions is None.
    h0_*: [B, A, H] (the state before the first step run) or None for zeros.
    steps=(t0, t1): only those steps, into the given outs.  Returns a dict: q_on
    [B, T1, A, NA], h_on [B, T1, A, H], gi_on [B, T1, A, 3H], x_on [B, T1, A, H] (want_x;
    both kept for the backward) and q_tg, h_tg, gi_tg with two networks; outs: such a dict
    of preallocated dense tensors."""
    _rnn_obs("rnn_agent_fwd", shape, obs)
    B, T1, A, _ = obs.shape
    H, NA = shape.H, shape.NA
    _f32c("rnn_agent_fwd: params_on", params_on, (shape.n_params,))
    two = params_tg is not None
    if two:
        _f32c("rnn_agent_fwd: params_tg", params_tg, (shape.n_params,))
    t0, t1 = (0, T1) if steps is None else (int(steps[0]), int(steps[1]))
    if not 0 <= t0 < t1 <= T1:
        raise ValueError(f"rnn_agent_fwd: steps {(t0, t1)} outside [0, {T1}]")
    if shape.last_action:
        _rnn_actions("rnn_agent_fwd", shape, actions, B, max(t1 - 1 + int(act_shift), 0), False)
    else:
        actions = None
    _rnn_h0("rnn_agent_fwd: h0_on", shape, h0_on, B)
    _rnn_h0("rnn_agent_fwd: h0_tg", shape, h0_tg, B)
    if h0_on is not None and h0_tg is not None and B > 1 and h0_on.stride(0) != h0_tg.stride(0):
        raise TypeError("rnn_agent_fwd: h0_on and h0_tg must share their episode stride")
    dev = obs.device
    if outs is None:
        outs = {}
    want = [("q_on", NA), ("h_on", H), ("gi_on", 3 * H)] + ([("x_on", H)] if want_x else []) + \
        ([("q_tg", NA), ("h_tg", H), ("gi_tg", 3 * H)] if two else [])
    for k, w in want:
        if k not in outs:
            outs[k] = torch.empty(B, T1, A, w, device=dev)
        _f32c(f"rnn_agent_fwd: {k}", outs[k], (B, T1, A, w))
    h0 = h0_on if h0_on is not None else h0_tg
    act_sb, act_st = _mstrides(actions)
    a = _lib.RnnFwdArgs(params_on=_p(params_on), params_tg=_p(params_tg), obs=_p(obs), obs_sb=obs.stride(0),
                        obs_st=obs.stride(1), actions=_p(actions), act_sb=act_sb, act_st=act_st, h0_on=_p(h0_on),
                        h0_tg=_p(h0_tg), h0_sb=h0.stride(0) if h0 is not None and B > 1 else 0,
                        x_on=_p(outs.get("x_on") if want_x else None), gi_on=_p(outs["gi_on"]),
                        gi_tg=_p(outs.get("gi_tg") if two else None), q_on=_p(outs["q_on"]), h_on=_p(outs["h_on"]),
                        q_tg=_p(outs.get("q_tg") if two else None), h_tg=_p(outs.get("h_tg") if two else None),
                        B=B, T1=T1, A=A, OBS=shape.OBS, NA=NA, H=H, last_action=int(shape.last_action),
                        agent_id=int(shape.agent_id), act_shift=int(act_shift), t0=t0, t1=t1)
    _mark(timer, "begin:rnn_fwd")
    check(lib().t2o_rnn_fwd(ctypes.byref(a), stream_ptr(dev)), "rnn_agent_fwd")
    _mark(timer, "end:rnn_fwd")
    return outs


def rnn_slab_count(B, T, A):
    n = int(lib().t2o_rnn_bwd_slabs(int(B), int(T), int(A)))
    if n < 1:
        raise ValueError(f"rnn_slab_count: bad shape B={B} T={T} A={A}")
    return n


def rnn_work_floats(shape: RnnShape, B, T):
    n = int(lib().t2o_rnn_bwd_work_floats(int(B), int(T), shape.A, shape.H))
    if n < 1:
        raise ValueError(f"rnn_work_floats: bad shape B={B} T={T} {shape}")
    return n


def rnn_agent_bwd(shape: RnnShape, params, obs, fwd, *, T=None, actions=None, act_shift=0, gchosen=None, gq=None,
                  gh=None, h0=None, want_gh0=False, gh0=None, slabs=None, work=None, timer=None):
    """GRU agent backward (t2o_rnn_bwd) of one network over the steps t < T (default:
    all) of the forward `fwd` (rnn_agent_fwd's dict: x_on, gi_on, h_on) on the same obs,
    actions, act_shift and h0.  dL/dq is either gchosen [B, T, A], the gradient at
    actions[:, t] (the learner's form), or gq [B, T, A, NA]; gh [B, T, A, H] (optional)
    adds dL/dh.  Returns (slabs, nslab, gh0): the partial weight-gradient slabs
    [rnn_slab_count(B, T, A), n_params] (sum them with reduce_slabs) and dL/dh0 [B, A, H]
    (want_gh0, else None)."""
    _rnn_obs("rnn_agent_bwd", shape, obs)
    B, Ts, A, _ = obs.shape
    H, NA = shape.H, shape.NA
    T = Ts if T is None else int(T)
    if not 1 <= T <= Ts:
        raise ValueError(f"rnn_agent_bwd: T={T} outside [1, {Ts}]")
    _f32c("rnn_agent_bwd: params", params, (shape.n_params,))
    for k, w in (("x_on", H), ("gi_on", 3 * H), ("h_on", H)):
        _f32c(f"rnn_agent_bwd: fwd[{k!r}]", fwd[k], (B, Ts, A, w))
    if (gchosen is None) == (gq is None):
        raise ValueError("rnn_agent_bwd: give exactly one of gchosen and gq")
    if gchosen is not None:
        _f32c("rnn_agent_bwd: gchosen", gchosen, (B, T, A))
    else:
        _f32c("rnn_agent_bwd: gq", gq, (B, T, A, NA))
    if gh is not None:
        _f32c("rnn_agent_bwd: gh", gh, (B, T, A, H))
    if shape.last_action or gchosen is not None:
        need = T if gchosen is not None else max(T - 1 + int(act_shift), 0)
        _rnn_actions("rnn_agent_bwd", shape, actions, B, need, gchosen is not None)
    else:
        actions = None
    _rnn_h0("rnn_agent_bwd: h0", shape, h0, B)
    dev = obs.device
    nslab, nwork = rnn_slab_count(B, T, A), rnn_work_floats(shape, B, T)
    if slabs is None:
        slabs = torch.empty(nslab * shape.n_params, device=dev)
    if work is None:
        work = torch.empty(nwork, device=dev)
    if want_gh0 and gh0 is None:
        gh0 = torch.empty(B, A, H, device=dev)
    _f32c("rnn_agent_bwd: slabs", slabs)
    _f32c("rnn_agent_bwd: work", work)
    if gh0 is not None:
        _f32c("rnn_agent_bwd: gh0", gh0, (B, A, H))
    if slabs.numel() < nslab * shape.n_params or work.numel() < nwork:
        raise ValueError("rnn_agent_bwd: the slab or work buffer is too small")
    act_sb, act_st = _mstrides(actions)
    a = _lib.RnnBwdArgs(params=_p(params), obs=_p(obs), obs_sb=obs.stride(0), obs_st=obs.stride(1),
                        actions=_p(actions), act_sb=act_sb, act_st=act_st, h0=_p(h0),
                        h0_sb=h0.stride(0) if h0 is not None and B > 1 else 0, x=_p(fwd["x_on"]), gi=_p(fwd["gi_on"]),
                        h=_p(fwd["h_on"]), gchosen=_p(gchosen), gq=_p(gq), gh=_p(gh), gh0=_p(gh0), gslabs=_p(slabs),
                        work=_p(work), work_floats=work.numel(), max_slabs=slabs.numel() // shape.n_params, B=B, T=T,
                        Ts=Ts, A=A, OBS=shape.OBS, NA=NA, H=H, last_action=int(shape.last_action),
                        agent_id=int(shape.agent_id), act_shift=int(act_shift))
    _mark(timer, "begin:rnn_bwd")
    check(lib().t2o_rnn_bwd(ctypes.byref(a), stream_ptr(dev)), "rnn_agent_bwd")
    _mark(timer, "end:rnn_bwd")
    return slabs, nslab, gh0
