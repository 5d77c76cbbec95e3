"""CPU: the C-ABI of the QMIX / VDN mixers (include/t2omca.h t2o_q_select,
t2o_qmix_fwd / _bwd / _bwd_slabs / _bwd_work_floats / _param_count, t2o_vdn_bwd): the
library exports the symbols, the ctypes mirrors of the three argument structs have the
C sizes, every bad argument is T2O_EINVAL before any launch (host pointers, no device:
a launch would fault), and the ops wrappers refuse CPU tensors."""
import ctypes

import pytest
import torch

EINVAL = -1


def _lib():
    from t2omca_amd import _lib
    return _lib, _lib.lib()


def test_symbols_and_struct_sizes():
    _l, lib = _lib()
    for name in ("t2o_q_select", "t2o_qmix_param_count", "t2o_qmix_fwd", "t2o_qmix_bwd", "t2o_qmix_bwd_slabs",
                 "t2o_qmix_bwd_work_floats", "t2o_vdn_bwd"):
        assert hasattr(lib, name) and name in _l.EXPORTS, name
    assert lib.t2o_abi_version() == 6 == _l.ABI_VERSION  # added within ABI 6: nothing existing moved
    for cls, which in ((_l.QSelectArgs, 13), (_l.QmixFwdArgs, 14), (_l.QmixBwdArgs, 15)):
        assert cls.WHICH == which and cls in _l.ARGS_STRUCTS
        assert ctypes.sizeof(cls) == lib.t2o_args_sizeof(which), cls.__name__
    assert lib.t2o_args_sizeof(16) == -1   # the next unused id
    assert lib.t2o_args_sizeof(12) == -1   # published as unknown before these structs: left unassigned
    # the earlier structs kept their ids and sizes
    assert [c.WHICH for c in _l.ARGS_STRUCTS[:12]] == list(range(12))
    assert [lib.t2o_args_sizeof(i) for i in range(12)] == [136, 192, 296, 224, 48, 168, 88, 184, 56, 96, 120, 80]
    with pytest.raises(AttributeError):
        _l.QmixFwdArgs(pack=1)


def test_sizes():
    _, lib = _lib()
    assert lib.t2o_qmix_param_count(8, 64, 32, 64) == 31233
    assert lib.t2o_qmix_param_count(6, 48, 16, 32) == 2 * (48 * 32 + 32) + 96 * 32 + 96 + 2 * (16 * 48 + 16) + \
        16 * 32 + 16 + 16 + 1
    for bad in ((0, 8, 32, 64), (65, 8, 32, 64), (8, 0, 32, 64), (8, 1025, 32, 64), (8, 64, 48, 64), (8, 64, 32, 128)):
        assert lib.t2o_qmix_param_count(*bad) == EINVAL, bad
    assert lib.t2o_qmix_bwd_slabs(2, 3) == 1 and lib.t2o_qmix_bwd_slabs(40, 7) == 2
    assert lib.t2o_qmix_bwd_slabs(1024, 60) == 64   # capped
    assert lib.t2o_qmix_bwd_slabs(0, 3) == EINVAL and lib.t2o_qmix_bwd_slabs(3, 0) == EINVAL
    # whole 16-row tiles of 4H + 4M + 4 floats
    assert lib.t2o_qmix_bwd_work_floats(40, 7, 32, 64) == 288 * (4 * 64 + 4 * 32 + 4)
    assert lib.t2o_qmix_bwd_work_floats(2, 3, 16, 32) == 16 * (4 * 32 + 4 * 16 + 4)
    assert lib.t2o_qmix_bwd_work_floats(2, 3, 8, 32) == EINVAL


def test_q_select_rejects_bad_arguments_before_launch():
    _l, lib = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = dict(q_on=p, q_tg=p, q_ts=5, n_actions=5, actions=p, act_sb=15, act_st=3, avail=p, av_sb=75, av_st=15,
              qmode_on=1, qmode_tg=2, qv_on=p, qv_tg=p, y_on=None, y_tg=None, B=2, T_on=4, T_tg=5, A=3)
    assert lib.t2o_q_select(None, None) == EINVAL
    for bad in (dict(q_on=None), dict(qv_on=None), dict(qv_tg=None), dict(actions=None), dict(qmode_on=0),
                dict(qmode_on=3), dict(qmode_tg=0), dict(qmode_tg=3), dict(B=0), dict(T_on=0), dict(T_tg=0),
                dict(T_on=6), dict(T_tg=6), dict(A=0), dict(A=65), dict(n_actions=0),
                dict(q_tg=None, y_tg=p)):
        assert lib.t2o_q_select(ctypes.byref(_l.QSelectArgs(**dict(ok, **bad))), None) == EINVAL, bad


def test_qmix_entry_points_reject_bad_arguments_before_launch():
    _l, lib = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    fwd = dict(params_on=p, params_tg=p, states=p, st_sb=320, st_st=64, qv_on=p, qv_tg=p, y_on=p, y_tg=p, B=2, T_on=4,
               T_tg=5, A=8, S=64, M=32, H=64, pos_func=0, pos_beta=1.0)
    assert lib.t2o_qmix_fwd(None, None) == EINVAL
    for bad in (dict(params_on=None), dict(states=None), dict(qv_on=None), dict(y_on=None), dict(qv_tg=None),
                dict(y_tg=None), dict(B=0), dict(T_on=0), dict(T_tg=0), dict(A=0), dict(A=65), dict(S=0), dict(S=1025),
                dict(M=8), dict(M=48), dict(H=16), dict(H=128), dict(pos_func=-1), dict(pos_func=4),
                dict(B=1 << 14, T_on=1 << 13)):
        assert lib.t2o_qmix_fwd(ctypes.byref(_l.QmixFwdArgs(**dict(fwd, **bad))), None) == EINVAL, bad
    work = (ctypes.c_float * 8)()
    wp = (ctypes.addressof(work) + 15) // 16 * 16
    need = lib.t2o_qmix_bwd_work_floats(2, 4, 32, 64)
    bwd = dict(params=p, states=p, st_sb=320, st_st=64, qv=p, gy=p, gqv=p, gslabs=p, work=wp, work_floats=need,
               max_slabs=1, phase=0, B=2, T=4, A=8, S=64, M=32, H=64, pos_func=0, pos_beta=1.0)
    assert lib.t2o_qmix_bwd(None, None) == EINVAL
    for bad in (dict(params=None), dict(states=None), dict(qv=None), dict(gy=None), dict(gqv=None), dict(gslabs=None),
                dict(work=None), dict(work=wp + 4), dict(work_floats=need - 1), dict(max_slabs=0), dict(phase=3),
                dict(phase=-1), dict(B=0), dict(T=0), dict(A=65), dict(S=0), dict(M=48), dict(H=128),
                dict(pos_func=4), dict(phase=1, gy=None), dict(phase=2, gslabs=None)):
        assert lib.t2o_qmix_bwd(ctypes.byref(_l.QmixBwdArgs(**dict(bwd, **bad))), None) == EINVAL, bad
    assert lib.t2o_vdn_bwd(None, p, 2, 4, 3, None) == EINVAL and lib.t2o_vdn_bwd(p, None, 2, 4, 3, None) == EINVAL
    assert lib.t2o_vdn_bwd(p, p, 0, 4, 3, None) == EINVAL and lib.t2o_vdn_bwd(p, p, 2, 4, 65, None) == EINVAL


def test_ops_refuse_cpu_tensors():
    from t2omca_amd import ops
    sh = ops.QmixShape(3, 24)
    n = sh.n_params
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.q_select(torch.zeros(2, 3, 3, 5), actions=torch.zeros(2, 3, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.qmix_fwd(sh, torch.zeros(n), torch.zeros(2, 3, 24), torch.zeros(2, 3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.qmix_bwd(sh, torch.zeros(n), torch.zeros(2, 3, 24), torch.zeros(2, 3, 3), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vdn_bwd(torch.zeros(2, 3), A=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vdn_fwd(torch.zeros(2, 3, 3))
