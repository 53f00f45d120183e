"""Every instantiation of the symmetric x-update (symv_kernels.h) under every class of tile schedule, against an exact reference.

The kernels: symv2_lower_kernel plain / non-temporal / with the mid-tile verdict check (admm_hip_test_symv_ex, variants 0 / 1 / 2),
symvn_lower_kernel<2, 4, 8, 12> plain and non-temporal with both consumers (admm_hip_test_symv_multi_ex: finish 0 is
symv_sum_partials, 1 is symv_sum_partials_n walked as the multi-task tail walks it), symv2_lower_f64acc_kernel
(admm_hip_test_symv_f64acc), and the tile lists dealt out to the ranks of the row-sharded solver (part / nparts).  The schedules go
through the thread option SYMV_SCHED, so every width from 32 to 256 runs at orders of a few hundred; every hook reports the schedule
its plan used and every test asserts it.

Exactness: the matrix and the vectors hold small integers, |a| <= 7, |v| <= 7 (3 at p = 4200, 2 at p = 6001), so every product and
every partial sum of any subset of a row's terms is an integer of magnitude <= 49 p < 2^24 (9 * 4200, 4 * 6001 likewise): each fmaf,
shuffle add, cross-wave add and consumer add is exact in fp32 whatever the order, and the result has to EQUAL the int64 product, every
element, no tolerance.  The strict upper triangle handed to the kernels is NaN (they may read only the lower one): a single entry read
from above the diagonal, a slot read that no tile wrote into a poisoned value, or a slot summed twice shows as a wrong integer."""
import ctypes
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_fp = ctypes.POINTER(ctypes.c_float)
_dp = ctypes.POINTER(ctypes.c_double)

P = (3, 31, 33, 129, 255, 256, 257, 259, 260, 383, 385, 511, 513, 769, 1023, 1025, 1100)
S = (None, "32,32,0", "64,64,0", "128,128,0", "256,256,0", "192,64,500", "128,64,500", "256,32,500", "32,256,500", "96,160,333",
     "224,96,1000", "160,224,0")
DEFAULT_CLASSES = {(32, 32), (64, 64), (128, 64), (192, 64)}
NR = (2, 4, 8, 12)


def _ptr(a, t=_fp):
    return a.ctypes.data_as(t)


def _check_sched(sched_out, sched, p):
    """The plan ran the schedule the test set (or, without an override, one of the documented default classes)."""
    nrb = -(-p // 256)
    got = tuple(sched_out)
    if sched is None:
        assert got[:2] in DEFAULT_CLASSES and got[2] == (0 if got[0] == got[1] else nrb // 2), got
    else:
        wb, ws, permille = (int(x) for x in sched.split(","))
        assert got == (wb, ws, permille * nrb // 1000), (got, sched)
    return got


def _symv_ex(A, v0, v1, variant=0, part=0, nparts=1, sched=None):
    from admm_amd import _lib
    p = A.shape[0]
    y0, y1 = np.full(p, np.nan, np.float32), np.full(p, np.nan, np.float32)
    so = (ctypes.c_int * 3)()
    _lib.check(_lib.load().admm_hip_test_symv_ex(_ptr(A), p, _ptr(v0), _ptr(v1), variant, part, nparts, _ptr(y0), _ptr(y1), so))
    _check_sched(so, sched, p)
    return y0, y1


def _symv_multi_ex(A, V, rhs, nt, finish, sched=None):
    from admm_amd import _lib
    p, nr = A.shape[0], V.shape[0]
    out = np.full((nr, p), np.nan, np.float32)
    so = (ctypes.c_int * 3)()
    _lib.check(_lib.load().admm_hip_test_symv_multi_ex(_ptr(A), p, _ptr(V), nr, rhs, nt, finish, _ptr(out), so))
    _check_sched(so, sched, p)
    return out


def _symv_f64acc(A, v0, v1, sched=None):
    from admm_amd import _lib
    p = A.shape[0]
    y0, y1 = np.full(p, np.nan), np.full(p, np.nan)
    so = (ctypes.c_int * 3)()
    _lib.check(_lib.load().admm_hip_test_symv_f64acc(_ptr(A), p, _ptr(v0), _ptr(v1), _ptr(y0, _dp), _ptr(y1, _dp), so))
    _check_sched(so, sched, p)
    return y0, y1


def _ints(p, lim=7):
    """(A for the hooks: float32 column-major, lower triangle integers in [-lim, lim], strict upper triangle NaN; v0 dense; v1 ~90 % zeros;
    the int64 references A v0, A v1 with the lower triangle mirrored; that mirrored matrix).  The orders of P are computed once and
    shared, never written to; the few large ones are not kept."""
    return _ints_shared(p, lim) if p <= max(P) else _ints_build(p, lim)


@functools.lru_cache(maxsize=None)
def _ints_shared(p, lim):
    return _ints_build(p, lim)


def _ints_build(p, lim):
    rng = np.random.default_rng(1000 * lim + p)
    B = rng.integers(-lim, lim + 1, size=(p, p), dtype=np.int32)
    Ai = np.tril(B) + np.tril(B, -1).T
    A = np.asfortranarray(np.where(np.tri(p, dtype=bool), Ai, np.nan).astype(np.float32))
    v0 = rng.integers(-lim, lim + 1, size=p, dtype=np.int64)
    v1 = rng.integers(-lim, lim + 1, size=p, dtype=np.int64) * (rng.uniform(size=p) < 0.1)
    Ai = Ai.astype(np.int64)
    out = (A, v0.astype(np.float32), v1.astype(np.float32), Ai @ v0, Ai @ v1, Ai)
    for a in out:
        a.setflags(write=False)
    return out


def _exact(y, ref):
    """Equal as numbers, every element (a NaN or an infinity equals no integer)."""
    return np.array_equal(y.astype(np.float64), ref.astype(np.float64))


def _same_bits(a, b):
    return a.tobytes() == b.tobytes()


def _options(sched):
    from admm_amd import options
    return options(SYMV_SCHED=sched)


@pytest.mark.parametrize("sched", S, ids=lambda s: s or "default")
def test_two_vector_kernel_exact_all_variants(sched):
    """symv2_lower_kernel plain, NT and MID: equal to the int64 product and bit-identical to each other, 17 orders per schedule."""
    with _options(sched):
        for p in P:
            A, v0, v1, r0, r1, _ = _ints(p)
            ys = [_symv_ex(A, v0, v1, variant, sched=sched) for variant in (0, 1, 2)]
            for variant, (y0, y1) in enumerate(ys):
                assert _exact(y0, r0) and _exact(y1, r1), (p, variant, np.flatnonzero(y0 != r0)[:8], np.flatnonzero(y1 != r1)[:8])
                assert _same_bits(y0, ys[0][0]) and _same_bits(y1, ys[0][1]), (p, variant)


def _vectors(v0, v1, nr):
    """v0, v1 and cyclic shifts of them by whole positions (same values, same sparsity: the bound on the partial sums stands)."""
    return np.ascontiguousarray(np.stack([np.roll(v1 if r & 1 else v0, 37 * (r // 2)) for r in range(nr)]), dtype=np.float32)


@pytest.mark.parametrize("rhs", NR)
@pytest.mark.parametrize("sched", S, ids=lambda s: s or "default")
def test_multi_vector_kernel_exact(sched, rhs):
    """symvn_lower_kernel<rhs>, plain and NT, both consumers: odd counts, a partly filled last pass, a single vector."""
    with _options(sched):
        for p in (33, 257, 385, 1025):
            A, v0, v1, _, _, Ai = _ints(p)
            for nr in sorted({1, 2, 3, rhs, rhs + 1, 2 * rhs - 1}):
                V = _vectors(v0, v1, nr)
                ref = (Ai @ V.astype(np.int64).T).T
                for nt in (0, 1):
                    pair = _symv_multi_ex(A, V, rhs, nt, 0, sched)
                    chunk = _symv_multi_ex(A, V, rhs, nt, 1, sched)
                    for r in range(nr):
                        assert _exact(pair[r], ref[r]), (p, nr, nt, r, np.flatnonzero(pair[r] != ref[r])[:8])
                        assert _exact(chunk[r], ref[r]), (p, nr, nt, r, np.flatnonzero(chunk[r] != ref[r])[:8])
                    assert _same_bits(pair, chunk), (p, nr, nt)


@pytest.mark.parametrize("sched", S, ids=lambda s: s or "default")
def test_f64acc_exact(sched):
    """symv2_lower_f64acc_kernel and the double consumer: the double result equals the int64 product."""
    with _options(sched):
        for p in P:
            A, v0, v1, r0, r1, _ = _ints(p)
            y0, y1 = _symv_f64acc(A, v0, v1, sched)
            assert np.array_equal(y0, r0.astype(np.float64)) and np.array_equal(y1, r1.astype(np.float64)), p


@pytest.mark.parametrize("p", [257, 1100])
def test_f64acc_accuracy_gaussian(p):
    """Float data that rounds: every float x float product is exact in double (24 + 24 bits), so only the p - 1 additions of a row's p
    terms round, each by at most 2^-53 of a partial sum that |A||v| bounds, whatever the order; the reference (math.fsum of the exact
    products: correctly rounded) adds 2^-53 |ref|.  Hence |y - ref|_i <= p 2^-52 (|A||v|)_i -- derived, not measured."""
    rng = np.random.default_rng(p)
    B = rng.standard_normal((p, p)).astype(np.float32)
    A = np.asfortranarray(np.tril(B) + np.tril(B, -1).T, dtype=np.float32)
    v0 = rng.standard_normal(p).astype(np.float32)
    v1 = (rng.standard_normal(p) * (rng.uniform(size=p) < 0.1)).astype(np.float32)
    Ap = A.copy(order="F")
    Ap[np.triu_indices(p, 1)] = np.nan
    y0, y1 = _symv_f64acc(Ap, v0, v1)
    A64 = A.astype(np.float64)
    worst = 0.0
    for y, v in ((y0, v0), (y1, v1)):
        prod = A64 * v.astype(np.float64)[None, :]                       # exact
        ref = np.array([math.fsum(row) for row in prod])
        bound = p * 2.0 ** -52 * np.abs(prod).sum(axis=1)
        err = np.abs(y - ref)
        worst = max(worst, float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()))
        assert (err <= bound).all(), (p, float((err / bound).max()))
    print("f64acc p = %d: max |y - ref| / (p 2^-52 |A||v|) = %.3e" % (p, worst))


@pytest.mark.parametrize("sched", [None, "192,64,500", "96,160,333", "128,128,0"], ids=lambda s: s or "default")
def test_dealt_out_tile_lists_add_up(sched):
    """nparts > 1: every rank launches its share into zeroed partial arrays; the shares add up to the product and none holds a NaN."""
    with _options(sched):
        for p in (385, 1100):
            A, v0, v1, r0, r1, _ = _ints(p)
            for nparts in (2, 3, 4):
                s0, s1 = np.zeros(p, np.int64), np.zeros(p, np.int64)
                for part in range(nparts):
                    y0, y1 = _symv_ex(A, v0, v1, 0, part, nparts, sched)
                    assert np.isfinite(y0).all() and np.isfinite(y1).all(), (p, nparts, part)
                    s0 += y0.astype(np.int64); s1 += y1.astype(np.int64)
                assert np.array_equal(s0, r0) and np.array_equal(s1, r1), (p, nparts)


def test_consumer_second_pass():
    """p = 4200 in 32-column segments: an element of the last strip sums 1 dot + 132 axpy partials, of the one before 2 + 128 -- more
    than the 16 x 8 slots of one pass of symv_sum_partials (and the 8 x 8 of symv_sum_partials_n), so its k0 loop runs again."""
    sched, p = "32,32,0", 4200
    A, v0, v1, r0, r1, Ai = _ints(p, 3)
    with _options(sched):
        for variant in (0, 2):
            y0, y1 = _symv_ex(A, v0, v1, variant, sched=sched)
            assert _exact(y0, r0) and _exact(y1, r1), (variant, np.flatnonzero(y0 != r0)[:8], np.flatnonzero(y1 != r1)[:8])
        V = _vectors(v0, v1, 5)
        ref = (Ai @ V.astype(np.int64).T).T
        pair, chunk = _symv_multi_ex(A, V, 4, 0, 0, sched), _symv_multi_ex(A, V, 4, 0, 1, sched)
        assert _exact(pair, ref) and _exact(chunk, ref) and _same_bits(pair, chunk)


def _skip_unless_128_64(sched_out, p):
    got = tuple(sched_out)
    if got != (128, 64, -(-p // 256) // 2):
        pytest.skip("this device's compute-unit count cuts p = %d as %s, not as the 128|64 class of a 256-CU device" % (p, got))


def test_the_128_64_class_gaussian():
    """p = 6000 under the default schedule of a 256-CU device: 128-column segments for the long strips, 64 for the short ones -- the
    class no other test runs.  Gaussian data, held to the bounds of tests/test_gpu_symv.py: 1e-6 norm-wise against float64."""
    from admm_amd import _lib
    p = 6000
    rng = np.random.default_rng(p)
    B = rng.standard_normal((p, p)).astype(np.float32)
    A = np.asfortranarray(np.tril(B) + np.tril(B, -1).T, dtype=np.float32)
    del B
    v0 = rng.standard_normal(p).astype(np.float32)
    v1 = (rng.uniform(size=p) * (rng.uniform(size=p) < 0.1)).astype(np.float32)
    so = (ctypes.c_int * 3)()
    y0, y1 = np.empty(p, np.float32), np.empty(p, np.float32)
    _lib.check(_lib.load().admm_hip_test_symv_ex(_ptr(A), p, _ptr(v0), _ptr(v1), 0, 0, 1, _ptr(y0), _ptr(y1), so))
    _skip_unless_128_64(so, p)
    A64 = A.astype(np.float64)
    for name, y, v in (("v0", y0, v0), ("v1", y1, v1)):
        ref = A64 @ v.astype(np.float64)
        scale = np.abs(A64) @ np.abs(v.astype(np.float64))
        err = np.abs(y.astype(np.float64) - ref).max() / scale.max()
        rel = np.linalg.norm(y - ref) / np.linalg.norm(ref)
        print("128|64 p = %d %s: max |y - ref| / max |A||v| = %.3e, ||y - ref|| / ||ref|| = %.3e" % (p, name, err, rel))
        assert err <= 1e-6 and rel <= 1e-6, (name, err, rel)


def test_the_128_64_class_exact():
    """p = 6001 (ragged in every sense) in the same class, integers in [-2, 2]: 4 * 6001 < 2^24.  Plain and MID."""
    from admm_amd import _lib
    p = 6001
    A, v0, v1, r0, r1, _ = _ints(p, 2)
    so = (ctypes.c_int * 3)()
    for variant in (0, 2):
        y0, y1 = np.full(p, np.nan, np.float32), np.full(p, np.nan, np.float32)
        _lib.check(_lib.load().admm_hip_test_symv_ex(_ptr(A), p, _ptr(v0), _ptr(v1), variant, 0, 1, _ptr(y0), _ptr(y1), so))
        _skip_unless_128_64(so, p)
        assert _exact(y0, r0) and _exact(y1, r1), (variant, np.flatnonzero(y0 != r0)[:8], np.flatnonzero(y1 != r1)[:8])


@pytest.mark.parametrize("p,lim", [(2563, 7), (4200, 3)])
def test_ragged_non_temporal_at_the_default_schedule(p, lim):
    """The NT form where the solver's own schedules are cut ragged (the only NT launch of the other tests is p = 12800 = 50 x 256):
    exact, and bit-identical to the plain form."""
    A, v0, v1, r0, r1, _ = _ints(p, lim)
    plain = _symv_ex(A, v0, v1, 0)
    nt = _symv_ex(A, v0, v1, 1)
    for y, z, r in ((plain[0], nt[0], r0), (plain[1], nt[1], r1)):
        assert _exact(z, r), np.flatnonzero(z != r)[:8]
        assert _exact(y, r) and _same_bits(y, z)
