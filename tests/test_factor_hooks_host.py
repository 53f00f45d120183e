"""The test hooks of the factorisation chain (admm_hip_test_gemm_nt, admm_hip_test_cholesky_linvt, admm_hip_test_spd_inverse_shift),
everything that needs no GPU: declared, exported, bound with argument types, listed in INTEGRATION.md, and refusing bad or
inconsistent requests before they look for a device.  What they compute is tests/test_gpu_factor.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 2
HOOKS = ("admm_hip_test_gemm_nt", "admm_hip_test_cholesky_linvt", "admm_hip_test_spd_inverse_shift")


def _lib():
    from admm_amd import _lib
    return _lib.load()


def _gemm(is_double=0, lower=0, mirror=0, kstart_row=0, b_lower=0, in_place=0, M=4, N=3, K=16, alpha=1.0, beta=0.0, A="ok", B="ok", C="ok"):
    lib = _lib()
    dt = np.float64 if is_double else np.float32
    a = np.ones((max(M, 1), max(K, 1)), dtype=dt, order="F")
    b = np.ones((max(N, 1), max(K, 1)), dtype=dt, order="F")
    c = np.zeros((max(M, 1), max(N, 1)), dtype=dt, order="F")
    ptr = lambda x, how: ctypes.c_void_p(x.ctypes.data) if how == "ok" else None
    rc = lib.admm_hip_test_gemm_nt(is_double, lower, mirror, kstart_row, b_lower, in_place, M, N, K, alpha, beta, ptr(a, A), ptr(b, B), ptr(c, C))
    return rc, lib.admm_hip_last_error().decode()


GEMM_REFUSALS = [
    (dict(A=None), "must not be NULL"),
    (dict(B=None), "must not be NULL"),
    (dict(C=None), "must not be NULL"),
    (dict(M=0), "M, N in"),
    (dict(N=-1), "M, N in"),
    (dict(K=0), "M, N in"),
    (dict(M=16385), "M, N in"),
    (dict(alpha=float("nan")), "finite"),
    (dict(beta=float("inf")), "finite"),
    (dict(lower=1, M=4, N=3), "square"),
    (dict(mirror=1), "mirrored store belongs to lower"),
    (dict(b_lower=1, is_double=0), "b_lower"),
    (dict(b_lower=1, is_double=1, lower=1, M=4, N=4), "b_lower"),
    (dict(in_place=1, K=16), "in_place"),
    (dict(in_place=1, K=128, N=129), "in_place"),
    (dict(in_place=1, K=128, lower=1, M=4, N=4), "in_place"),
]


def test_symbols_are_declared_exported_and_listed():
    from admm_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "admm_hip.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in HOOKS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym) and sym in _lib.EXPORTS
        assert getattr(lib, sym).argtypes is not None and getattr(lib, sym).restype is ctypes.c_int
        assert "`%s`" % sym in doc, sym


def test_gemm_hook_refuses_inconsistent_requests_before_it_looks_for_a_device():
    for spoil, fragment in GEMM_REFUSALS:
        rc, msg = _gemm(**spoil)
        assert rc == INVALID_ARG and fragment in msg, (spoil, rc, msg)


def test_factor_and_shift_hooks_refuse_bad_arguments_before_they_look_for_a_device():
    lib = _lib()
    a = np.eye(3, dtype=np.float64, order="F")
    f = np.eye(3, dtype=np.float32, order="F")
    o1, o2 = np.zeros_like(a), np.zeros_like(a)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)
    for args in ((0, None, 3, p(o1), p(o2)), (1, p(a), 3, None, p(o2)), (1, p(a), 3, p(o1), None), (1, p(a), 0, p(o1), p(o2)), (0, p(a), -2, p(o1), p(o2))):
        assert lib.admm_hip_test_cholesky_linvt(*args) == INVALID_ARG, args
        assert "bad arguments" in lib.admm_hip_last_error().decode()
    for args in ((None, 3, 0.5, p(f)), (p(f), 3, 0.5, None), (p(f), 0, 0.5, p(f)), (p(f), 3, float("nan"), p(f)), (p(f), 3, float("inf"), p(f))):
        assert lib.admm_hip_test_spd_inverse_shift(*args) == INVALID_ARG, args
        assert "bad arguments" in lib.admm_hip_last_error().decode()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a machine without a GPU")
def test_valid_requests_find_no_device():
    lib = _lib()
    for kw in (dict(), dict(is_double=1, b_lower=1), dict(lower=1, mirror=1, kstart_row=1, M=5, N=5), dict(in_place=1, K=128, M=130, N=128)):
        rc, msg = _gemm(**kw)
        assert rc == NO_DEVICE, (kw, rc, msg)
    a = np.eye(3, dtype=np.float32, order="F")
    o1, o2 = np.zeros_like(a), np.zeros_like(a)
    assert lib.admm_hip_test_cholesky_linvt(0, a.ctypes.data, 3, o1.ctypes.data, o2.ctypes.data) == NO_DEVICE
    assert lib.admm_hip_test_spd_inverse_shift(a.ctypes.data, 3, 0.37, o1.ctypes.data) == NO_DEVICE
