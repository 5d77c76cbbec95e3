"""CPU: the C-ABI of the stale-LDS probes (include/t2omca.h t2o_probe_lds_fill /
t2o_probe_lds_census): the header declares them, the library exports them, the ctypes
binding lists them as diagnostics (an older build under T2O_LIB may lack them), and a bad
argument is T2O_EINVAL before any launch (no device here: a launch would fail)."""
import ctypes
import os
import re

EINVAL = -1
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("t2o_probe_lds_fill", "t2o_probe_lds_census")


def test_declared_exported_and_bound_as_diagnostics():
    from t2omca_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(REPO, "include", "t2omca.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(uint32_t word, int workgroups, ", header), name
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert name in _lib._DIAGNOSTIC and name in _lib._OPTIONAL, name
        assert _lib.EXPORTS[name][0] is ctypes.c_int and _lib.EXPORTS[name][1][0] is ctypes.c_uint32
    assert len(_lib.EXPORTS["t2o_probe_lds_fill"][1]) == 3
    assert len(_lib.EXPORTS["t2o_probe_lds_census"][1]) == 4
    assert lib.t2o_abi_version() == _lib.ABI_VERSION  # added within the ABI version: nothing existing moved


def test_bad_arguments_do_not_launch():
    from t2omca_amd import _lib
    lib = _lib.lib()
    for n in (0, -1):
        assert lib.t2o_probe_lds_fill(0xFFFFFFFF, n, None) == EINVAL
        assert lib.t2o_probe_lds_census(0, n, None, None) == EINVAL
    assert lib.t2o_probe_lds_census(0x7F7F7F7F, 4, None, None) == EINVAL  # no output buffer
