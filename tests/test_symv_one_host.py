"""The host-visible pieces of the decide-first x-update, without a GPU: the option SYMV_VERDICT accepts 0|1|2|3 and nothing else, and the
hook admm_hip_test_symv_one (tests/test_gpu_symv_one.py) is declared, exported, bound and listed, and refuses bad requests before it
looks for a device.  In the style of tests/test_symv_plan_host.py."""
import ctypes
import os
import re

import numpy as np
import pytest

INVALID_ARG, NO_DEVICE = 1, 2
_fp = ctypes.POINTER(ctypes.c_float)


def _L():
    from admm_amd import _lib
    return _lib


def test_the_option_takes_the_four_levels():
    L = _L()
    lib = L.load()
    L.options.reset()
    try:
        for v in (b"0", b"1", b"2", b"3"):
            L.check(lib.admm_hip_option_set(b"SYMV_VERDICT", v))
            assert lib.admm_hip_option_get(b"SYMV_VERDICT") == v
        for v in (b"4", b"-1", b"on"):
            assert lib.admm_hip_option_set(b"SYMV_VERDICT", v) == INVALID_ARG, v
            assert b"SYMV_VERDICT" in lib.admm_hip_last_error() and b"0|1|2|3" in lib.admm_hip_last_error()
            assert lib.admm_hip_option_get(b"SYMV_VERDICT") == b"3"      # a refusal leaves the setting as it was
    finally:
        L.check(lib.admm_hip_options_reset())
    assert lib.admm_hip_option_get(b"SYMV_VERDICT") is None              # unset: the default, level 3
    with L.options(SYMV_VERDICT=3):
        assert lib.admm_hip_option_get(b"SYMV_VERDICT") == b"3"


def _args(p=5, cap=4096):
    A = np.eye(p, dtype=np.float32, order="F")
    v = np.ones(p, dtype=np.float32)
    y = np.zeros((2, p), np.float32)
    dot, axp = np.zeros((2, cap), np.float32), np.zeros((2, cap), np.float32)
    return dict(A=A.ctypes.data_as(_fp), v0=v.ctypes.data_as(_fp), v1=v.ctypes.data_as(_fp), y=y.ctypes.data_as(_fp), dot=dot.ctypes.data_as(_fp),
                axp=axp.ctypes.data_as(_fp), cap=cap, info=(ctypes.c_longlong * 4)(), sched=(ctypes.c_int * 3)(), keep=(A, v, y, dot, axp))


def _one(lib, a, p=5, gate=0, nt=0, **ptr):
    g = dict(a, **ptr)
    return lib.admm_hip_test_symv_one(g["A"], p, g["v0"], g["v1"], gate, nt, 0x7FC00000, g["y"], g["dot"], g["axp"], g["cap"], g["info"], g["sched"])


def test_the_hook_refuses_bad_arguments_before_it_looks_for_a_device():
    lib = _L().load()
    a = _args()
    for spoil in (dict(A=None), dict(v0=None), dict(v1=None), dict(y=None), dict(info=None), dict(sched=None), dict(dot=None), dict(axp=None),
                  dict(p=0), dict(p=32769), dict(gate=-1), dict(gate=4), dict(nt=2), dict(nt=-1), dict(cap=-1)):
        assert _one(lib, a, **spoil) == INVALID_ARG, spoil
        assert "symv_one hook" in lib.admm_hip_last_error().decode()


def test_the_symbol_is_declared_exported_bound_and_listed():
    L = _L()
    lib = L.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "admm_hip.h")).read(), flags=re.S)
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    sym = "admm_hip_test_symv_one"
    assert re.search(r"\b%s\s*\(" % sym, hdr)
    assert hasattr(lib, sym) and sym in L.EXPORTS
    assert len(lib.admm_hip_test_symv_one.argtypes) == 13 and lib.admm_hip_test_symv_one.restype is ctypes.c_int
    assert "`%s`" % sym in doc
    assert "`ADMM_HIP_SYMV_VERDICT=0` / `1` / `2` / `3`" in doc


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a machine without a GPU")
def test_valid_requests_find_no_device():
    lib = _L().load()
    a = _args()
    for gate in (0, 1, 2, 3):
        assert _one(lib, a, gate=gate) == NO_DEVICE
    assert _one(lib, a, gate=2, nt=1, dot=None, axp=None, cap=0) == NO_DEVICE
