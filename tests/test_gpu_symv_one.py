"""The one-vector kernel of the decide-first x-update (symv_kernels.h: symv1_lower_kernel) with its gate forced, through the hook
admm_hip_test_symv_one: gate 0 / 1 multiplies v0 / v1 into plane 0 of the partial arrays, gate 2 makes every tile leave, gate 3 runs
the two-vector kernel (symv2_lower_kernel) on the same storage.  The finished sums go through symv_sum_partials1, the one-plane sum of
the solver's TAIL_SYMV1 tails.

Exactness is the device of test_gpu_symv_variants.py: small integers (|a|, |v| <= 7 at p <= 2563: 49 p < 2^24; <= 3 at p = 4200), so
every fmaf and every partial sum is exact in fp32 in any order and the result has to EQUAL the int64 product; the strict upper triangle
is NaN, and so is every slot of the partial arrays before the launch (fill = a NaN pattern): an entry read from above the diagonal, a
slot summed that no tile wrote, or a slot summed twice shows as a wrong number."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_fp = ctypes.POINTER(ctypes.c_float)
POISON = 0x7FC0BEEF                      # a quiet NaN with a payload: equal to itself only as bits
CASES = [(2304, None, 7), (2563, None, 7), (4200, "32,32,0", 3)]      # whole grid resident | ragged: p no multiple of 32 or 256 | 1220 tiles > 1024 resident slots


def _ptr(a):
    return a.ctypes.data_as(_fp)


def _options(sched):
    from admm_amd import options
    return options(SYMV_SCHED=sched)


@functools.lru_cache(maxsize=None)
def _ints(p, lim):
    rng = np.random.default_rng(1000 * lim + p)
    B = rng.integers(-lim, lim + 1, size=(p, p), dtype=np.int32)
    Ai = np.tril(B) + np.tril(B, -1).T
    A = np.asfortranarray(np.where(np.tri(p, dtype=bool), Ai, np.nan).astype(np.float32))
    v0 = rng.integers(-lim, lim + 1, size=p, dtype=np.int64)
    v1 = rng.integers(-lim, lim + 1, size=p, dtype=np.int64) * (rng.uniform(size=p) < 0.1)
    Ai = Ai.astype(np.int64)
    out = (A, v0.astype(np.float32), v1.astype(np.float32), Ai @ v0, Ai @ v1)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _gauss(p):
    rng = np.random.default_rng(p)
    B = rng.standard_normal((p, p)).astype(np.float32)
    A = np.asfortranarray(np.tril(B) + np.tril(B, -1).T, dtype=np.float32)
    A[np.triu_indices(p, 1)] = np.nan
    v0 = rng.standard_normal(p).astype(np.float32)
    v1 = (rng.standard_normal(p) * (rng.uniform(size=p) < 0.1)).astype(np.float32)
    for a in (A, v0, v1):
        a.setflags(write=False)
    return A, v0, v1


def _one(A, v0, v1, gate, nt=0):
    """(y [2][p], dot planes [2][nd], axpy planes [2][na], tiles, tiles that left) of one launch.  The planes' sizes come back from the
    hook; the capacity offered holds any schedule: row strips and segments of a strip number at most ceil(p / 32) each."""
    from admm_amd import _lib
    p = A.shape[0]
    nrb = -(-p // 256)
    cap = max(nrb, -(-p // 32)) * nrb * 256
    y = np.full((2, p), np.nan, np.float32)
    dot, axp = np.zeros((2, cap), np.float32), np.zeros((2, cap), np.float32)
    so, info = (ctypes.c_int * 3)(), (ctypes.c_longlong * 4)()
    _lib.check(_lib.load().admm_hip_test_symv_one(_ptr(A), p, _ptr(v0), _ptr(v1), gate, nt, POISON, _ptr(y), _ptr(dot), _ptr(axp), cap, info, so))
    return y, dot[:, :int(info[2])], axp[:, :int(info[3])], int(info[0]), int(info[1])


def _poisoned(a):
    return bool((a.view(np.uint32) == POISON).all())


def _exact(y, ref):
    return np.array_equal(y.astype(np.float64), ref.astype(np.float64))


@pytest.mark.parametrize("p,sched,lim", CASES, ids=lambda v: str(v))
def test_the_picked_vector_exactly_into_plane_zero(p, sched, lim):
    A, v0, v1, r0, r1 = _ints(p, lim)
    with _options(sched):
        for nt in (0, 1):
            for gate, ref in ((0, r0), (1, r1)):
                y, dot, axp, tiles, left = _one(A, v0, v1, gate, nt)
                assert left == 0 and tiles > 0
                if sched is not None:
                    assert tiles == 1220                            # more tiles than the 1024 resident workgroups of a 256-CU device
                assert _exact(y[0], ref), (gate, nt, np.flatnonzero(y[0] != ref)[:8])
                assert _poisoned(dot[1]) and _poisoned(axp[1])       # plane 1 is nobody's on this path


@pytest.mark.parametrize("p,sched,lim", CASES, ids=lambda v: str(v))
def test_bit_identical_to_the_two_vector_kernels_planes(p, sched, lim):
    """Gaussian data: the partials written for pick = r, and their sum, have the bits symv2_lower_kernel leaves in plane r."""
    A, v0, v1 = _gauss(p)
    with _options(sched):
        y2, dot2, axp2, _, left2 = _one(A, v0, v1, 3)
        assert left2 == 0 and np.isfinite(y2).all()
        # every slot a tile owns was written by both kernels; the slots no tile owns keep the fill in both
        for r in (0, 1):
            y, dot, axp, _, left = _one(A, v0, v1, r)
            assert left == 0
            assert dot[0].tobytes() == dot2[r].tobytes() and axp[0].tobytes() == axp2[r].tobytes(), r
            assert y[0].tobytes() == y2[r].tobytes(), r
        # and the reference is admm_hip_test_symv_ex's (variant 0) on the same inputs
        from admm_amd import _lib
        e0, e1 = np.empty(p, np.float32), np.empty(p, np.float32)
        so = (ctypes.c_int * 3)()
        _lib.check(_lib.load().admm_hip_test_symv_ex(_ptr(A), p, _ptr(v0), _ptr(v1), 0, 0, 1, _ptr(e0), _ptr(e1), so))
        assert e0.tobytes() == y2[0].tobytes() and e1.tobytes() == y2[1].tobytes()


@pytest.mark.parametrize("p,sched,lim", CASES, ids=lambda v: str(v))
def test_a_forced_leave_writes_nothing_and_counts_every_tile(p, sched, lim):
    A, v0, v1, _, _ = _ints(p, lim)
    with _options(sched):
        for nt in (0, 1):
            _, dot, axp, tiles, left = _one(A, v0, v1, 2, nt)
            assert _poisoned(dot) and _poisoned(axp)
            assert left == tiles > 0
            if sched is not None:
                assert tiles == 1220
