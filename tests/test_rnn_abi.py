"""CPU: the C-ABI of the GRU agent (include/t2omca.h t2o_rnn_fwd / _bwd / _bwd_slabs /
_bwd_work_floats / _param_count): the library exports the symbols, the ctypes mirrors
of the two argument structs have the C sizes at ids 21-22 (12, 16 and 20 stay unknown,
ABI 6), every bad argument is T2O_EINVAL before any launch (host pointers, no device: a
launch would fault), and the ops wrappers refuse CPU tensors."""
import ctypes

import pytest
import torch

EINVAL = -1


def _lib():
    from t2omca_amd import _lib
    return _lib, _lib.lib()


def test_symbols_and_struct_sizes():
    _l, lib = _lib()
    for name in ("t2o_rnn_param_count", "t2o_rnn_fwd", "t2o_rnn_bwd", "t2o_rnn_bwd_slabs", "t2o_rnn_bwd_work_floats"):
        assert hasattr(lib, name) and name in _l.EXPORTS, name
    assert lib.t2o_abi_version() == 6 == _l.ABI_VERSION  # added within ABI 6: nothing existing moved
    for cls, which, size in ((_l.RnnFwdArgs, 21, 192), (_l.RnnBwdArgs, 22, 200)):
        assert cls.WHICH == which and cls in _l.ARGS_STRUCTS
        assert ctypes.sizeof(cls) == lib.t2o_args_sizeof(which) == size, cls.__name__
    for unassigned in (12, 16, 20):  # published as unknown: left unassigned
        assert lib.t2o_args_sizeof(unassigned) == -1
    assert lib.t2o_args_sizeof(23) == -1  # the next unused id
    # the earlier structs kept their ids and sizes
    assert [lib.t2o_args_sizeof(i) for i in range(12)] == [136, 192, 296, 224, 48, 168, 88, 184, 56, 96, 120, 80]
    assert [lib.t2o_args_sizeof(i) for i in (13, 14, 15)] == [128, 112, 120]
    assert [lib.t2o_args_sizeof(i) for i in (17, 18, 19)] == [144, 144, 144]
    with pytest.raises(AttributeError):
        _l.RnnFwdArgs(pack=1)


def test_sizes():
    _, lib = _lib()
    count = lambda IN, H, NA: H * IN + H + 2 * (3 * H * H + 3 * H) + NA * H + NA  # noqa: E731
    for IN, H, NA in ((14, 64, 5), (14, 32, 5), (1, 32, 1), (656, 64, 16), (9 * 8 + 5 + 8, 64, 5)):
        assert lib.t2o_rnn_param_count(IN, H, NA) == count(IN, H, NA), (IN, H, NA)
    for bad in ((0, 64, 5), (657, 64, 5), (14, 48, 5), (14, 128, 5), (14, 64, 0), (14, 64, 17)):
        assert lib.t2o_rnn_param_count(*bad) == EINVAL, bad
    assert lib.t2o_rnn_bwd_slabs(2, 3, 1) == 1 and lib.t2o_rnn_bwd_slabs(40, 7, 1) == 2
    assert lib.t2o_rnn_bwd_slabs(5, 7, 8) == 2 and lib.t2o_rnn_bwd_slabs(1024, 60, 8) == 64  # capped
    for bad in ((0, 3, 1), (3, 0, 1), (3, 3, 0), (1 << 14, 1 << 13, 1)):
        assert lib.t2o_rnn_bwd_slabs(*bad) == EINVAL, bad
    assert lib.t2o_rnn_bwd_work_floats(5, 4, 3, 64) == 60 * 5 * 64  # per row dgi [3H], dgh's n gate [H], dpre [H]
    assert lib.t2o_rnn_bwd_work_floats(5, 4, 3, 32) == 60 * 5 * 32
    assert lib.t2o_rnn_bwd_work_floats(5, 4, 3, 48) == EINVAL and lib.t2o_rnn_bwd_work_floats(0, 4, 3, 64) == EINVAL


def _aligned(n):
    buf = (ctypes.c_float * (n + 4))()
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_fwd_bwd_reject_bad_arguments_before_launch():
    _l, lib = _lib()
    keep, p = _aligned(64)
    dims = dict(B=2, A=3, OBS=6, NA=5, H=64, last_action=1, agent_id=1)
    bad_dims = (dict(A=0), dict(A=65), dict(OBS=0), dict(OBS=657), dict(OBS=650), dict(NA=0), dict(NA=17), dict(H=16),
                dict(H=48), dict(H=128), dict(B=0), dict(B=1 << 27))
    fwd = dict(params_on=p, params_tg=p, obs=p, obs_sb=90, obs_st=18, actions=p, act_sb=15, act_st=3, h0_on=p, h0_tg=p,
               h0_sb=192, x_on=p, gi_on=p, gi_tg=p, q_on=p, h_on=p, q_tg=p, h_tg=p, T1=5, t0=0, t1=5, **dims)
    assert lib.t2o_rnn_fwd(None, None) == EINVAL
    for bad in (dict(params_on=None), dict(obs=None), dict(gi_on=None), dict(q_on=None), dict(h_on=None),
                dict(gi_tg=None), dict(q_tg=None), dict(h_tg=None), dict(T1=0), dict(t0=-1), dict(t1=6), dict(t0=5),
                dict(t0=3, t1=3), dict(h_on=p + 4), dict(gi_on=p + 8), dict(x_on=p + 4), dict(h0_on=p + 4),
                dict(h0_sb=190)) + bad_dims:
        assert lib.t2o_rnn_fwd(ctypes.byref(_l.RnnFwdArgs(**dict(fwd, **bad))), None) == EINVAL, bad
    need = lib.t2o_rnn_bwd_work_floats(2, 4, 3, 64)
    bwd = dict(params=p, obs=p, obs_sb=90, obs_st=18, actions=p, act_sb=15, act_st=3, h0=p, h0_sb=192, x=p, gi=p, h=p,
               gchosen=p, gq=None, gh=p, gh0=p, gslabs=p, work=p, work_floats=need, max_slabs=1, T=4, Ts=5, **dims)
    assert lib.t2o_rnn_bwd(None, None) == EINVAL
    for bad in (dict(params=None), dict(obs=None), dict(x=None), dict(gi=None), dict(h=None), dict(gslabs=None),
                dict(work=None), dict(work=p + 4), dict(work_floats=need - 1), dict(max_slabs=0), dict(T=0), dict(T=6),
                dict(gchosen=None), dict(gq=p), dict(actions=None), dict(gh=p + 4), dict(gh0=p + 8), dict(h0=p + 4),
                dict(h0_sb=191)) + bad_dims:
        assert lib.t2o_rnn_bwd(ctypes.byref(_l.RnnBwdArgs(**dict(bwd, **bad))), None) == EINVAL, bad
    del keep


def test_ops_argument_checks():
    from t2omca_amd import ops
    sh = ops.RnnShape(3, 6, 5)
    assert sh.IN == 14 and sh.E == 64 and sh.agents == 3 and ops.RnnShape(3, 27, 5, 32, False, False).IN == 27
    n = sh.n_params
    assert n == sum(torch.Size(s).numel() for _, s in ops.rnn_param_blocks(14, 64, 5))
    assert [k for k, _ in ops.rnn_param_blocks(14, 64, 5)] == ["fc1.weight", "fc1.bias", "rnn.weight_ih",
                                                                "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh",
                                                                "fc2.weight", "fc2.bias"]
    obs, acts = torch.zeros(2, 4, 3, 6), torch.zeros(2, 4, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rnn_agent_fwd(sh, torch.zeros(n), obs, actions=acts)
    fwd = dict(x_on=torch.zeros(2, 4, 3, 64), gi_on=torch.zeros(2, 4, 3, 192), h_on=torch.zeros(2, 4, 3, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rnn_agent_bwd(sh, torch.zeros(n), obs, fwd, actions=acts, gchosen=torch.zeros(2, 4, 3))
