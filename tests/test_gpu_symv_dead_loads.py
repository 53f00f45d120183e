"""GPU: symv2_lower_kernel no longer loads the float4s of a diagonal block that lie above the diagonal in full (symv_kernels.h:
`col <= last`).  Those entries were zeroed after the load before, so nothing may change by a bit: the kernel must still equal
symvn_lower_kernel at NR = 2 -- the restatement of the same arithmetic that still loads the whole rectangle -- and must not
notice what the strict upper triangle holds.

Sizes: 2048 (whole strips), 2049 (a last strip of one row), 2303 and 2563 (a diagonal block cut by p, rows that are no multiple
of 4 or 32), 4200 (another schedule: 64-column segments, more than one tile per diagonal block)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
_fp = ctypes.POINTER(ctypes.c_float)
_cache = {}


def _symv2(A, v0, v1):
    from admm_amd import _lib
    lib = _lib.load()
    p = A.shape[0]
    y0, y1 = np.empty(p, F), np.empty(p, F)
    _lib.check(lib.admm_hip_test_symv(A.ctypes.data_as(_fp), p, v0.ctypes.data_as(_fp), v1.ctypes.data_as(_fp),
                                      y0.ctypes.data_as(_fp), y1.ctypes.data_as(_fp)))
    return y0, y1


def _symvn2(A, v0, v1):
    from admm_amd import _lib
    lib = _lib.load()
    p = A.shape[0]
    V = np.ascontiguousarray(np.stack([v0, v1]), dtype=F)
    out = np.empty((2, p), F)
    _lib.check(lib.admm_hip_test_symv_multi(A.ctypes.data_as(_fp), p, V.ctypes.data_as(_fp), 2, 2, out.ctypes.data_as(_fp)))
    return out[0], out[1]


def _case(p):
    """A random symmetric matrix, a dense and a sparse vector, and what the kernel returns for them (computed once)."""
    if p not in _cache:
        rng = np.random.default_rng(p)
        B = rng.standard_normal((p, p)).astype(F)
        A = np.asfortranarray(np.tril(B) + np.tril(B, -1).T, dtype=F)
        v0 = rng.standard_normal(p).astype(F)
        v1 = (rng.standard_normal(p) * (rng.uniform(size=p) < 0.1)).astype(F)
        _cache[p] = (A, v0, v1, _symv2(A, v0, v1))
    return _cache[p]


SIZES = [2048, 2049, 2303, 2563, 4200]


@pytest.mark.parametrize("p", SIZES)
def test_equals_the_untouched_multi_vector_kernel_bit_for_bit(p):
    A, v0, v1, (y0, y1) = _case(p)
    r0, r1 = _symvn2(A, v0, v1)
    assert np.isfinite(y0).all() and np.isfinite(y1).all()
    assert np.array_equal(y0, r0), (p, int(np.argmax(y0 != r0)))
    assert np.array_equal(y1, r1), (p, int(np.argmax(y1 != r1)))


@pytest.mark.parametrize("p", SIZES)
def test_the_strict_upper_triangle_is_never_seen(p):
    A, v0, v1, (y0, y1) = _case(p)
    iu = np.triu_indices(p, 1)
    for poison in (np.nan, np.inf, -np.inf):
        Ap = A.copy(order="F")
        Ap[iu] = poison
        z0, z1 = _symv2(Ap, v0, v1)
        assert np.array_equal(y0, z0) and np.array_equal(y1, z1), (p, poison)
