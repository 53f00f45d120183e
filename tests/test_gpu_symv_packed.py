"""The one-vector kernel on the exact 29-bit copy of the tiles (symv_kernels.h: symv1_packed_kernel, symv_pack_kernel; format in
symv_pack.h) through the hook admm_hip_test_symv_packed, against symv1_lower_kernel on the fp32 matrix through admm_hip_test_symv_one, on
the shapes and schedules of tests/test_gpu_symv_one.py.

The packing is exact, and everything behind the decode is the fp32 kernel's code, so the partial planes and their sum have to be the same
BYTES, whatever the data: inverse-like matrices, planted zeros / denormals / tiny entries (the escape list), small integers.  The number of
escapes the pack kernel reports is compared with a NumPy restatement of the format's rule over the plan's own tile list."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_fp = ctypes.POINTER(ctypes.c_float)
POISON = 0x7FC0BEEF
CASES = [(2304, None, 7), (2563, None, 7), (4200, "32,32,0", 3)]      # one resident round | ragged in 32 and 256 | 1220 tiles > the resident slots
WINDOW, CAP = 14, 32


def _ptr(a):
    return a.ctypes.data_as(_fp)


def _options(sched):
    from admm_amd import options
    return options(SYMV_SCHED=sched)


def _tiles(p, sched):
    """The plan's tile list (row strip, first column, width, segment), from the host hook."""
    from admm_amd import _lib
    cap = 4 * (-(-p // 32)) ** 2
    so, info, tl = (ctypes.c_int * 3)(), (ctypes.c_longlong * 6)(), (ctypes.c_int * (4 * cap))()
    with _options(sched):
        _lib.check(_lib.load().admm_hip_test_symv_plan(p, 256, 0, 1, so, info, tl, cap))
    return np.frombuffer(tl, dtype=np.int32)[:4 * int(info[5])].reshape(-1, 4).copy()


def _expected_escapes(A, tiles):
    """Per tile: entries the fp32 kernel uses (on or below the diagonal, columns < p; rows >= p are zero padding) that are not a zero and
    whose upper seven exponent bits lie outside [base - 13, base], base = the largest among the tile's finite non-zero used entries."""
    p = A.shape[0]
    bits = A.view(np.uint32)
    out = []
    for rb, c0, w, _ in tiles:
        r0, r1, c1 = rb * 256, min(rb * 256 + 256, p), min(c0 + w, p)
        if c0 >= c1:
            out.append(0)
            continue
        b = bits[r0:r1, c0:c1].astype(np.int64)
        used = (np.arange(r0, r1)[:, None] >= np.arange(c0, c1)[None, :])
        mag, e8, e7 = b & 0x7FFFFFFF, (b >> 23) & 0xFF, (b >> 24) & 0x7F
        counts = used & (mag != 0) & (e8 != 255)
        base = int(e7[counts].max()) if counts.any() else 0
        fits = (mag == 0) | ((e8 != 255) & (e7 <= base) & (e7 >= base - (WINDOW - 1)))
        out.append(int((used & ~fits).sum()))
    return np.asarray(out)


@functools.lru_cache(maxsize=None)
def _inverse_like(p):
    # An N(0, 1) draw within 2^-27 of zero (diagonal tiles, against the 1.0) is an escape: about every second matrix of these sizes has one.
    # The seeds are ones whose matrices have none (asserted below with the NumPy rule); escapes are the planted test's business.
    rng = np.random.default_rng({2304: 31000}.get(p, 29000) + p)
    B = (3e-3 * rng.standard_normal((p, p))).astype(np.float32)
    A = np.asfortranarray(np.tril(B, -1) + np.tril(B, -1).T + np.eye(p, dtype=np.float32), dtype=np.float32)
    A[np.triu_indices(p, 1)] = np.nan
    v0 = rng.standard_normal(p).astype(np.float32)
    v1 = (rng.standard_normal(p) * (rng.uniform(size=p) < 0.1)).astype(np.float32)
    for a in (A, v0, v1):
        a.setflags(write=False)
    return A, v0, v1


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


def _cap(p):
    nrb = -(-p // 256)
    return max(nrb, -(-p // 32)) * nrb * 256


def _fp32(A, v0, v1, gate):
    """symv1_lower_kernel: (y [p], dot planes [2][nd], axpy planes [2][na], tiles, tiles that left)."""
    from admm_amd import _lib
    p, cap = A.shape[0], _cap(A.shape[0])
    y = np.full((2, p), np.nan, np.float32)
    dot, axp = np.zeros((2, cap), np.float32), np.zeros((2, cap), np.float32)
    so, info = (ctypes.c_int * 3)(), (ctypes.c_longlong * 4)()
    _lib.check(_lib.load().admm_hip_test_symv_one(_ptr(A), p, _ptr(v0), _ptr(v1), gate, 0, POISON, _ptr(y), _ptr(dot), _ptr(axp), cap, info, so))
    return y[0], dot[:, :int(info[2])], axp[:, :int(info[3])], int(info[0]), int(info[1])


def _packed(A, v0, v1, gate, nt=0, esc_cap=CAP):
    """symv1_packed_kernel: the same, and (escapes met, tiles overflowed, bytes of the stream, 1 if the kernel ran)."""
    from admm_amd import _lib
    p, cap = A.shape[0], _cap(A.shape[0])
    y = np.full((2, p), np.nan, np.float32)
    dot, axp = np.zeros((2, cap), np.float32), np.zeros((2, cap), np.float32)
    so, info = (ctypes.c_int * 3)(), (ctypes.c_longlong * 8)()
    _lib.check(_lib.load().admm_hip_test_symv_packed(_ptr(A), p, _ptr(v0), _ptr(v1), gate, nt, POISON, esc_cap, _ptr(y), _ptr(dot), _ptr(axp), cap, info, so))
    return y[0], dot[:, :int(info[2])], axp[:, :int(info[3])], int(info[0]), int(info[1]), tuple(int(info[k]) for k in (4, 5, 6, 7))


def _poisoned(a):
    return bool((a.view(np.uint32) == POISON).all())


def _same_bytes(A, v0, v1, sched, escapes):
    with _options(sched):
        for gate in (0, 1):
            y, dot, axp, tiles, left = _fp32(A, v0, v1, gate)
            assert left == 0 and tiles > 0 and np.isfinite(y).all()
            for nt in (0, 1):
                yp, dotp, axpp, tilesp, leftp, (met, over, nbytes, ran) = _packed(A, v0, v1, gate, nt)
                assert (met, over, ran) == (escapes, 0, 1), (gate, nt, met, over, ran)
                assert tilesp == tiles and leftp == 0
                assert dotp[0].tobytes() == dot[0].tobytes() and axpp[0].tobytes() == axp[0].tobytes(), (gate, nt)      # unowned slots: the poison in both
                assert yp.tobytes() == y.tobytes(), (gate, nt)
                assert _poisoned(dotp[1]) and _poisoned(axpp[1])                                                         # plane 1 is nobody's on this path
                assert nbytes % 7424 == 0 and nbytes == 7424 * int((_tiles(A.shape[0], sched)[:, 2] // 8).sum())


@pytest.mark.parametrize("p,sched,lim", CASES, ids=lambda v: str(v))
def test_inverse_like_data_gives_the_fp32_kernels_bytes(p, sched, lim):
    A, v0, v1 = _inverse_like(p)
    want = int(_expected_escapes(A, _tiles(p, sched)).sum())
    assert want == 0                      # unit diagonal, off-diagonals 3e-3 N(0, 1): everything within 13 exponent pairs of its tile's largest
    _same_bytes(A, v0, v1, sched, 0)


def _plant(p, sched):
    """The inverse-like matrix with 20 entries replaced: an exact zero, -0.0, a denormal and a typical entry x 2^-40, one of each in a
    diagonal tile, an interior tile, the last (ragged) strip, the first and the last chunk of a wave."""
    A, v0, v1 = _inverse_like(p)
    A = A.copy(order="F")
    tiles = _tiles(p, sched)
    nrb = -(-p // 256)
    rb, c0, w, _ = tiles[(tiles[:, 1] + tiles[:, 2] > tiles[:, 0] * 256) & (tiles[:, 0] == nrb // 2)][0]
    spots = [[(rb * 256 + 255 - 7 * k, max(c0, rb * 256) + 2 * k) for k in range(4)]]                   # diagonal tile, below the diagonal
    rb, c0, w, _ = tiles[(tiles[:, 1] + tiles[:, 2] <= tiles[:, 0] * 256) & (tiles[:, 0] == nrb // 2)][-1]
    spots.append([(rb * 256 + 17 + 40 * k, c0 + 3 + 5 * k) for k in range(4)])                          # interior tile
    spots.append([(p - 1 - k, 11 + 300 * k) for k in range(4)])                                         # the last rows of the last strip
    rb, c0, w, _ = tiles[(tiles[:, 1] + tiles[:, 2] <= tiles[:, 0] * 256) & (tiles[:, 0] == nrb - 2)][0]
    cw = w // 4
    spots.append([(rb * 256 + 64 * k + k, c0 + k * cw + 2 * k) for k in range(4)])                      # first chunk of waves 0 .. 3
    spots.append([(rb * 256 + 61 * k + 3, c0 + k * cw + cw - 1 - k) for k in range(4)])                 # last chunk of waves 0 .. 3
    kinds = [np.float32(0.0), np.float32(-0.0), np.uint32(0x00012345).view(np.float32), None]
    outside = 0
    seen = set()
    for g, group in enumerate(spots):
        for k, (r, c) in enumerate(group):
            assert r >= c and r < p and (r, c) not in seen
            seen.add((r, c))
            val = kinds[(k + g) % 4]
            if val is None:
                val = np.float32(3e-3 * 2.0 ** -40) * (-1 if k % 2 else 1)
            A[r, c] = val
            outside += (k + g) % 4 >= 2
    return A, v0, v1, tiles, outside


@pytest.mark.parametrize("p,sched,lim", CASES, ids=lambda v: str(v))
def test_planted_zeros_denormals_and_tiny_entries(p, sched, lim):
    A, v0, v1, tiles, outside = _plant(p, sched)
    assert outside == 10
    per_tile = _expected_escapes(A, tiles)
    assert int(per_tile.sum()) == outside and per_tile.max() <= CAP      # the zeros have a code of their own; the denormals and the tiny entries do not fit
    _same_bytes(A, v0, v1, sched, outside)


@pytest.mark.parametrize("p,sched,lim", CASES[1:2], ids=lambda v: str(v))
def test_a_list_that_overflows_is_reported_and_nothing_is_streamed(p, sched, lim):
    A, v0, v1 = _inverse_like(p)
    A = A.copy(order="F")
    tiles = _tiles(p, sched)
    rb, c0, w, _ = tiles[(tiles[:, 1] + tiles[:, 2] <= tiles[:, 0] * 256) & (tiles[:, 0] == -(-p // 256) - 2)][0]
    for k in range(CAP + 1):                                            # one more than the list holds, in one tile
        A[rb * 256 + 3 * k, c0 + (5 * k) % w] = np.uint32(0x00000100 + k).view(np.float32)
    assert _expected_escapes(A, tiles).max() == CAP + 1
    with _options(sched):
        _, dot, axp, _, left, (met, over, _, ran) = _packed(A, v0, v1, 0)
        assert (met, over, ran, left) == (CAP + 1, 1, 0, 0)
        assert _poisoned(dot) and _poisoned(axp)
        _, _, _, _, _, (met, over, _, ran) = _packed(A, v0, v1, 0, esc_cap=CAP + 1)      # a list that holds them: streamed
        assert (met, over, ran) == (CAP + 1, 0, 1)
        _, _, _, _, _, (met, over, _, ran) = _packed(_inverse_like(p)[0], v0, v1, 0, esc_cap=0)      # no escapes: capacity 0 is enough
        assert (met, over, ran) == (0, 0, 1)


@pytest.mark.parametrize("p,sched,lim", CASES, ids=lambda v: str(v))
def test_a_forced_leave_writes_nothing_and_counts_every_tile(p, sched, lim):
    A, v0, v1 = _inverse_like(p)
    with _options(sched):
        for nt in (0, 1):
            _, dot, axp, tiles, left, (met, over, _, ran) = _packed(A, v0, v1, 2, nt)
            assert _poisoned(dot) and _poisoned(axp)
            assert left == tiles > 0 and (met, over, ran) == (0, 0, 1)
            if sched is not None:
                assert tiles == 1220


@pytest.mark.parametrize("p,sched,lim", CASES, ids=lambda v: str(v))
def test_small_integers_equal_the_int64_product(p, sched, lim):
    A, v0, v1, r0, r1 = _ints(p, lim)
    with _options(sched):
        for nt in (0, 1):
            for gate, ref in ((0, r0), (1, r1)):
                y, dot, axp, tiles, left, (met, over, _, ran) = _packed(A, v0, v1, gate, nt)
                assert (met, over, ran, left) == (0, 0, 1, 0) and tiles > 0      # |a| <= 7 spans two exponent pairs, the zeros have their code
                assert np.array_equal(y.astype(np.float64), ref.astype(np.float64)), (gate, nt, np.flatnonzero(y != ref)[:8])
                assert _poisoned(dot[1]) and _poisoned(axp[1])
