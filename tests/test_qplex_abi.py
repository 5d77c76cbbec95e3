"""CPU: the C-ABI of the QPLEX mixer (include/t2omca.h t2o_qplex_select / _fwd / _bwd /
_bwd_slabs / _bwd_work_floats / _param_count): the library exports the symbols, the
ctypes mirrors of the three argument structs have the C sizes at ids 17-19 (12 and 16
stay unknown, ABI 6), every bad argument is T2O_EINVAL before any launch (host pointers,
no device: a launch would fault), and the ops wrappers refuse CPU tensors."""
import ctypes

import pytest
import torch

EINVAL = -1
COUNTS = {3: 28450, 8: 73940, 16: 146724, 64: 583428}  # NA = 5, S = 8·A, K = 4, H = HA = 64


def _lib():
    from t2omca_amd import _lib
    return _lib, _lib.lib()


def test_symbols_and_struct_sizes():
    _l, lib = _lib()
    for name in ("t2o_qplex_param_count", "t2o_qplex_select", "t2o_qplex_fwd", "t2o_qplex_bwd", "t2o_qplex_bwd_slabs",
                 "t2o_qplex_bwd_work_floats"):
        assert hasattr(lib, name) and name in _l.EXPORTS, name
    assert lib.t2o_abi_version() == 6 == _l.ABI_VERSION  # added within ABI 6: nothing existing moved
    for cls, which, size in ((_l.QplexSelectArgs, 17, 144), (_l.QplexFwdArgs, 18, 144), (_l.QplexBwdArgs, 19, 144)):
        assert cls.WHICH == which and cls in _l.ARGS_STRUCTS
        assert ctypes.sizeof(cls) == lib.t2o_args_sizeof(which) == size, cls.__name__
    assert lib.t2o_args_sizeof(12) == -1 and lib.t2o_args_sizeof(16) == -1  # published as unknown: left unassigned
    assert lib.t2o_args_sizeof(20) == -1                                     # the next unused id
    # the earlier structs kept their ids and sizes
    assert [lib.t2o_args_sizeof(i) for i in range(12)] == [136, 192, 296, 224, 48, 168, 88, 184, 56, 96, 120, 80]
    assert [lib.t2o_args_sizeof(i) for i in (13, 14, 15)] == [ctypes.sizeof(c) for c in
                                                               (_l.QSelectArgs, _l.QmixFwdArgs, _l.QmixBwdArgs)]
    with pytest.raises(AttributeError):
        _l.QplexFwdArgs(pack=1)


def test_sizes():
    _, lib = _lib()
    for A, n in COUNTS.items():
        assert lib.t2o_qplex_param_count(A, 8 * A, 5, 64, 64, 4) == n, A
    # A = 6, S = 50, NA = 16, H = 32, HA = 64, K = 1, by hand
    assert lib.t2o_qplex_param_count(6, 50, 16, 32, 64, 1) == 2 * (32 * 50 + 32 + 6 * 32 + 6) + \
        (64 * 50 + 64 + 64 + 1) + (64 * 50 + 64 + 6 * 64 + 6) + (64 * (50 + 96) + 64 + 6 * 64 + 6)
    ok = (8, 64, 5, 64, 64, 4)
    for i, vals in enumerate(((0, 65), (0, 1025), (0, 17), (16, 48, 128), (16, 48, 128), (0, 11))):
        for v in vals:
            bad = ok[:i] + (v,) + ok[i + 1:]
            assert lib.t2o_qplex_param_count(*bad) == EINVAL, bad
    for edge in ((1, 1, 1, 32, 32, 1), (64, 1024, 16, 64, 64, 10)):
        assert lib.t2o_qplex_param_count(*edge) > 0, edge
    assert lib.t2o_qplex_bwd_slabs(2, 3) == 1 and lib.t2o_qplex_bwd_slabs(40, 7) == 2
    assert lib.t2o_qplex_bwd_slabs(1024, 60) == 64   # capped
    assert lib.t2o_qplex_bwd_slabs(0, 3) == EINVAL and lib.t2o_qplex_bwd_slabs(3, 0) == EINVAL
    assert lib.t2o_qplex_bwd_slabs(1 << 14, 1 << 13) == EINVAL
    # whole 16-row tiles; per block its hidden vector, its pre-activation gradient and its outputs' (A in 16s)
    assert lib.t2o_qplex_bwd_work_floats(40, 7, 8, 64, 64, 4) == 288 * 14 * (2 * 64 + 16)
    assert lib.t2o_qplex_bwd_work_floats(2, 3, 17, 32, 64, 1) == 16 * (2 * (64 + 32) + 3 * (128 + 32))
    assert lib.t2o_qplex_bwd_work_floats(2, 3, 8, 48, 64, 4) == EINVAL
    assert lib.t2o_qplex_bwd_work_floats(2, 3, 65, 64, 64, 4) == EINVAL
    assert lib.t2o_qplex_bwd_work_floats(2, 3, 8, 64, 64, 11) == EINVAL


def test_select_rejects_bad_arguments_before_launch():
    _l, lib = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = dict(q_on=p, q_tg=p, q_ts=5, n_actions=5, actions=p, act_sb=15, act_st=3, avail=p, av_sb=75, av_st=15,
              qmode_on=1, qmode_tg=2, qv_on=p, qv_tg=p, qmax_on=p, qmax_tg=p, act_on=p, act_tg=p, B=2, T_on=4, T_tg=5,
              A=3)
    assert lib.t2o_qplex_select(None, None) == EINVAL
    for bad in (dict(q_on=None), dict(qv_on=None), dict(qmax_on=None), dict(act_on=None), dict(qv_tg=None),
                dict(qmax_tg=None), dict(act_tg=None), dict(actions=None), dict(qmode_on=0), dict(qmode_on=3),
                dict(qmode_tg=0), dict(qmode_tg=3), dict(B=0), dict(T_on=0), dict(T_tg=0), dict(T_on=6),
                dict(T_tg=6), dict(A=0), dict(A=65), dict(n_actions=0), dict(n_actions=17),
                dict(B=1 << 14, q_ts=1 << 13)):
        assert lib.t2o_qplex_select(ctypes.byref(_l.QplexSelectArgs(**dict(ok, **bad))), None) == EINVAL, bad
    # the old select keeps refusing a third mode: the maxima come from the new entry point
    old = dict(q_on=p, q_tg=None, q_ts=5, n_actions=5, actions=p, act_sb=15, act_st=3, qmode_on=3, qv_on=p, B=2,
               T_on=4, A=3)
    assert lib.t2o_q_select(ctypes.byref(_l.QSelectArgs(**old)), None) == EINVAL


def test_fwd_bwd_reject_bad_arguments_before_launch():
    _l, lib = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    dims = dict(A=8, S=64, NA=5, H=64, HA=64, K=4)
    bad_dims = (dict(A=0), dict(A=65), dict(S=0), dict(S=1025), dict(NA=0), dict(NA=17), dict(H=16), dict(H=128),
                dict(HA=48), dict(HA=128), dict(K=0), dict(K=11))
    fwd = dict(params_on=p, params_tg=p, states=p, st_sb=320, st_st=64, qv_on=p, qv_tg=p, qmax_on=p, qmax_tg=p,
               act_on=p, act_tg=p, y_on=p, y_tg=p, B=2, T_on=4, T_tg=5, parts=3, **dims)
    assert lib.t2o_qplex_fwd(None, None) == EINVAL
    for bad in (dict(params_on=None), dict(states=None), dict(qv_on=None), dict(y_on=None), dict(qv_tg=None),
                dict(y_tg=None), dict(qmax_on=None), dict(act_on=None), dict(qmax_tg=None), dict(act_tg=None),
                dict(parts=0), dict(parts=4), dict(B=0), dict(T_on=0), dict(T_tg=0),
                dict(B=1 << 14, T_on=1 << 13)) + bad_dims:
        assert lib.t2o_qplex_fwd(ctypes.byref(_l.QplexFwdArgs(**dict(fwd, **bad))), None) == EINVAL, bad
    work = (ctypes.c_float * 8)()
    wp = (ctypes.addressof(work) + 15) // 16 * 16
    need = lib.t2o_qplex_bwd_work_floats(2, 4, 8, 64, 64, 4)
    bwd = dict(params=p, states=p, st_sb=320, st_st=64, qv=p, qmax=p, act=p, gy=p, gqv=p, gslabs=p, work=wp,
               work_floats=need, max_slabs=1, phase=0, parts=3, B=2, T=4, **dims)
    assert lib.t2o_qplex_bwd(None, None) == EINVAL
    for bad in (dict(params=None), dict(states=None), dict(qv=None), dict(qmax=None), dict(act=None), dict(gy=None),
                dict(gqv=None), dict(gslabs=None), dict(work=None), dict(work=wp + 4), dict(work_floats=need - 1),
                dict(max_slabs=0), dict(phase=3), dict(phase=-1), dict(parts=0), dict(parts=4), dict(B=0), dict(T=0),
                dict(phase=1, gy=None), dict(phase=2, gslabs=None)) + bad_dims:
        assert lib.t2o_qplex_bwd(ctypes.byref(_l.QplexBwdArgs(**dict(bwd, **bad))), None) == EINVAL, bad


def test_ops_refuse_cpu_tensors():
    from t2omca_amd import ops
    sh = ops.QplexShape(3, 24, 5)
    n = sh.n_params
    assert n == COUNTS[3]
    q, m, u = torch.zeros(2, 3, 3), torch.zeros(2, 3, 3), torch.zeros(2, 3, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.qplex_select(torch.zeros(2, 3, 3, 5), actions=torch.zeros(2, 3, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.qplex_fwd(sh, torch.zeros(n), torch.zeros(2, 3, 24), q, m, u)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.qplex_bwd(sh, torch.zeros(n), torch.zeros(2, 3, 24), q, m, u, torch.zeros(2, 3))
    assert [tuple(s) for _, s in ops.qplex_param_blocks(3, 24, 5)][:4] == [(64, 24), (64,), (3, 64), (3,)]
    assert sum(torch.Size(s).numel() for _, s in ops.qplex_param_blocks(3, 24, 5)) == n
