"""The chain under every tall, consensus and LAD solve, piece by piece against float64: the matrix-core NT-GEMM
(gemm_nt_mfma_kernel / gemm_nt_mfma_f64_kernel through their launchers, hook admm_hip_test_gemm_nt), the blocked Cholesky +
[L | I] elimination (cholesky_linvt_blocked over potf2_inv_kernel, hook admm_hip_test_cholesky_linvt), the inverse U U' in its
three precisions (admm_hip_test_spd_inverse) and with the tall path's float shift (admm_hip_test_spd_inverse_shift), the not-SPD
report, and the split-K forms of the Gram.  Orders are small on purpose: a single partial diagonal block, a last block of one
row (129, 257, 385), exact multiples of 128, and conditioning up to 1e5 under metrics that grow with it.

Bounds.  GEMM and Gram: the standard entrywise bound of a K-term inner product in any summation order plus the two roundings of
the alpha / beta epilogue, (K + 3) u (|alpha| |A| |B|' + |beta| |C0|), u = 2^-24 / 2^-53.  Factor and inverse: 5 x what LAPACK
achieves in the same precision on the same matrix (the factor tests/test_gpu_kernels.py gives itself); LAPACK is called through
scipy.linalg.lapack (potrf, trtri, potri) because numpy.linalg runs float32 input in DOUBLE and rounds the result -- its
"float32" inverse is the correctly rounded double one, no single-precision yardstick (cond 30, n = 129: residual 1.4e-7 where
spotrf + spotri reach 6.3e-7).  Via-double inverses: one float rounding of a double inverse, 2^-24 |exact| + 5 e64, e64 = the
largest entrywise error of LAPACK's float64 inverse of the same input against a refined reference (the residual formed in 80-bit
arithmetic, one Newton correction)."""
import functools

import numpy as np
import pytest
import scipy.linalg.lapack as lapack

pytestmark = pytest.mark.gpu

U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
DTYPES = [np.float32, np.float64]


def _lib():
    from admm_amd import _lib as L
    return L, L.load()


# ------------------------------------------------------------------------------------------------------------ GEMM
def _gemm(A, B, C0, alpha, beta, lower=0, mirror=0, kstart_row=0, b_lower=0, in_place=0):
    """C = alpha A B' + beta C0 through the project's launcher; A (M, K), B (N, K), C0 (M, N).  The hook itself fails (code 8)
    when the launch changed anything outside M x N of the padded device storage (a NaN guard band / the rest of A in place)."""
    L, lib = _lib()
    A, B = np.asfortranarray(A), np.asfortranarray(B)
    C = np.array(C0, dtype=A.dtype, order="F", copy=True)
    (M, K), N = A.shape, B.shape[0]
    assert B.shape == (N, K) and C.shape == (M, N) and B.dtype == A.dtype
    L.check(lib.admm_hip_test_gemm_nt(int(A.dtype == np.float64), lower, mirror, kstart_row, b_lower, in_place, M, N, K,
                                      float(alpha), float(beta), A.ctypes.data, B.ctypes.data, C.ctypes.data))
    return C


def _rand(rng, shape, dtype):
    return np.asfortranarray((rng.standard_normal(shape) * 2 + 0.3).astype(dtype))


def _ref_and_bound(A, B, C0, alpha, beta):
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    ref, mag = alpha * (A64 @ B64.T), abs(alpha) * (np.abs(A64) @ np.abs(B64).T)
    if beta != 0:
        ref, mag = ref + beta * C0.astype(np.float64), mag + abs(beta) * np.abs(C0.astype(np.float64))
    return ref, (A.shape[1] + 3) * U[A.dtype.type] * mag


def _lower_tiles(n):
    t = np.arange(n) // 128
    return t[:, None] >= t[None, :]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _worst(C, ref, bound, where=None):
    r = np.abs(C - ref) / np.where(bound > 0, bound, 1.0)
    return float(r[where].max() if where is not None else r.max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)])
@pytest.mark.parametrize("M,N,K", [(1, 1, 16), (127, 129, 16), (129, 127, 128), (200, 1, 128), (1, 200, 136), (257, 385, 24), (384, 384, 128)])
def test_gemm_full_launch_entrywise(M, N, K, alpha, beta, dtype):
    """The launch of the panel and U updates (not lower, no mirror: the epilogue through LDS, EPI = 1) against float64, entry by
    entry; with beta = 0 the output starts as NaN and must come back finite (beta C is never read)."""
    rng = np.random.default_rng(1000 * M + 10 * N + K)
    A, B, C0 = _rand(rng, (M, K), dtype), _rand(rng, (N, K), dtype), _rand(rng, (M, N), dtype)
    if beta == 0:
        C0[:] = np.nan
    C = _gemm(A, B, C0, alpha, beta)
    ref, bound = _ref_and_bound(A, B, C0, alpha, beta)
    assert np.all(np.isfinite(C))
    print(f"[gemm {dtype.__name__} {M}x{N}x{K} alpha={alpha} beta={beta}] worst |C - ref| / bound {_worst(C, ref, bound):.3f}")
    assert np.all(np.abs(C - ref) <= bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)])
@pytest.mark.parametrize("n,K", [(129, 40), (300, 128), (384, 24)])
def test_gemm_lower_leaves_the_upper_tiles_alone(n, K, alpha, beta, dtype):
    """LOWER without the mirrored store (the trailing update A_ij -= L_ik L_jk'; EPI = 1): tiles on or below the diagonal within
    the bound, tiles strictly above it bit for bit what they were."""
    rng = np.random.default_rng(n + K)
    A, B, C0 = _rand(rng, (n, K), dtype), _rand(rng, (n, K), dtype), _rand(rng, (n, n), dtype)
    low = _lower_tiles(n)
    if beta == 0:
        C0[low] = np.nan
    C = _gemm(A, B, C0, alpha, beta, lower=1)
    ref, bound = _ref_and_bound(A, B, C0, alpha, beta)
    assert np.array_equal(_bits(C)[~low], _bits(C0)[~low])
    assert np.all(np.isfinite(C[low]))
    print(f"[gemm lower {dtype.__name__} n={n} K={K} alpha={alpha} beta={beta}] worst |C - ref| / bound {_worst(C, ref, bound, low):.3f}")
    assert np.all((np.abs(C - ref) <= bound)[low])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.5, -2.0)])
@pytest.mark.parametrize("n,K", [(129, 40), (300, 128), (384, 24)])
def test_gemm_lower_mirrored_is_exactly_symmetric(n, K, alpha, beta, dtype):
    """LOWER with the mirrored store (the Gram Z Z' and the inverse U U'; direct stores, EPI = 0), as its callers use it: both
    operands the same matrix (and a symmetric C0 under beta).  C == C' exactly and both triangles within the bound."""
    rng = np.random.default_rng(2 * n + K)
    A = _rand(rng, (n, K), dtype)
    C0 = _rand(rng, (n, n), dtype)
    C0 = np.asfortranarray(np.tril(C0) + np.tril(C0, -1).T)
    if beta == 0:
        C0[:] = np.nan
    C = _gemm(A, A, C0, alpha, beta, lower=1, mirror=1)
    ref, bound = _ref_and_bound(A, A, C0, alpha, beta)
    assert np.all(np.isfinite(C)) and np.array_equal(C, C.T)
    print(f"[gemm lower + mirror {dtype.__name__} n={n} K={K} alpha={alpha} beta={beta}] worst |C - ref| / bound {_worst(C, ref, bound):.3f}")
    assert np.all(np.abs(C - ref) <= bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mirror", [1, 0])
@pytest.mark.parametrize("p", [129, 257, 385])
def test_gemm_kstart_row_skips_exact_zeros_only(p, mirror, dtype):
    """U U' with U upper triangular, as spd_inverse_blocked (mirror) and the distributed inverse (no mirror) launch it: starting
    a tile's K loop at its first row skips products that are exact zeros -- bit-identical to the launch that does not skip."""
    rng = np.random.default_rng(p)
    Uop = np.asfortranarray(np.triu(_rand(rng, (p, p), dtype)))
    C0 = np.zeros((p, p), dtype=dtype)
    full = _gemm(Uop, Uop, C0, 1.0, 0.0, lower=1, mirror=mirror)
    skip = _gemm(Uop, Uop, C0, 1.0, 0.0, lower=1, mirror=mirror, kstart_row=1)
    ref, bound = _ref_and_bound(Uop, Uop, C0, 1.0, 0.0)
    low = _lower_tiles(p) if not mirror else np.ones((p, p), dtype=bool)
    assert np.all((np.abs(full - ref) <= bound)[low])
    assert np.array_equal(_bits(skip), _bits(full))


@pytest.mark.parametrize("p", [129, 257, 385])
def test_gemm_b_lower_skips_exact_zeros_only(p):
    """The double launch with a lower-triangular B (gemm_nt_f64(..., b_lower): the K loop ends after the tile's last column)."""
    rng = np.random.default_rng(3 * p)
    A = _rand(rng, (200, p), np.float64)
    B = np.asfortranarray(np.tril(_rand(rng, (p, p), np.float64)))
    C0 = np.full((200, p), np.nan)
    full = _gemm(A, B, C0, 1.0, 0.0)
    skip = _gemm(A, B, C0, 1.0, 0.0, b_lower=1)
    ref, bound = _ref_and_bound(A, B, C0, 1.0, 0.0)
    assert np.all(np.abs(full - ref) <= bound)
    assert np.array_equal(_bits(skip), _bits(full))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 40, 128])
@pytest.mark.parametrize("M", [128, 129, 500])
def test_gemm_in_place_equals_out_of_place(M, N, dtype):
    """The factorisation's U[:, k] <- U[:, k] L_kk^-T and L_ik = A_ik L_kk^-T write their output over operand A (K = 128, N = the
    block's columns): bit for bit the out-of-place result; the columns of A behind N and its padding rows stay (the hook)."""
    rng = np.random.default_rng(M + N)
    A, B = _rand(rng, (M, 128), dtype), _rand(rng, (N, 128), dtype)
    C0 = np.full((M, N), np.nan, dtype=dtype)
    out = _gemm(A, B, C0, 1.0, 0.0)
    inp = _gemm(A, B, C0, 1.0, 0.0, in_place=1)
    ref, bound = _ref_and_bound(A, B, C0, 1.0, 0.0)
    assert np.all(np.abs(out - ref) <= bound)
    assert np.array_equal(_bits(inp), _bits(out))


# ------------------------------------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def spd(n, cond, seed=0):
    """Q diag(logspace(0, -log10 cond)) Q' in float64, symmetric to the bit."""
    rng = np.random.default_rng(7919 * n + seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0.0, -np.log10(cond), n)) @ Q.T
    A = 0.5 * (A + A.T)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def graded(n=300):
    """D A D with D = 10^U(-3, 3) on a cond-30 matrix: unstandardised columns."""
    d = 10.0 ** np.random.default_rng(n).uniform(-3, 3, n)
    A = spd(n, 30.0) * d[:, None] * d[None, :]
    A = 0.5 * (A + A.T)
    A.setflags(write=False)
    return A


def lapack_inverse(A):
    """LAPACK's SPD inverse in A's own precision: potrf + potri, mirrored."""
    potrf, potri = (lapack.spotrf, lapack.spotri) if A.dtype == np.float32 else (lapack.dpotrf, lapack.dpotri)
    c, info = potrf(A, lower=1)
    assert info == 0, f"potrf info {info}"
    X, info = potri(c, lower=1)
    assert info == 0, f"potri info {info}"
    return np.tril(X) + np.tril(X, -1).T


def refined_inverse(A64):
    """inv(A64) far below float64 rounding: LAPACK's float64 inverse X0 (dpotrf + dpotri) plus one Newton correction X0 (I - A X0) whose residual
    is formed in 80-bit arithmetic (its own rounding ~ 2^-11 of X0's error).  Returns (refined, X0)."""
    X0 = lapack_inverse(np.asfortranarray(A64))
    R = (np.eye(A64.shape[0], dtype=np.longdouble) - A64.astype(np.longdouble) @ X0.astype(np.longdouble)).astype(np.float64)
    X1 = X0 + X0 @ R
    return 0.5 * (X1 + X1.T), X0


_exact_cache = {}


def exact_of(key, A64):
    """(refined inverse, e64 = max entrywise error of LAPACK float64 on it), computed once per fixture."""
    if key not in _exact_cache:
        ex, X0 = refined_inverse(A64)
        _exact_cache[key] = (ex, float(np.abs(X0 - ex).max()))
    return _exact_cache[key]


def assert_float32_positive_definite(A32):
    """A bad fixture must not pass for a library error: LAPACK float32 potrf factorises the float32 matrix."""
    _, info = lapack.spotrf(A32, lower=1)
    assert info == 0, f"fixture is not positive definite in float32 (spotrf info {info})"


def residual(A64, X):
    return float(np.abs(A64 @ X.astype(np.float64) - np.eye(A64.shape[0])).max())


def _inverse(A, precision):
    L, lib = _lib()
    A = np.asfortranarray(A)
    out = np.zeros_like(A, order="F")
    L.check(lib.admm_hip_test_spd_inverse(A.ctypes.data, A.shape[0], precision, out.ctypes.data))
    return out


def _inverse_shift(A32, diag):
    L, lib = _lib()
    A32 = np.asfortranarray(A32, dtype=np.float32)
    out = np.zeros_like(A32, order="F")
    L.check(lib.admm_hip_test_spd_inverse_shift(A32.ctypes.data, A32.shape[0], float(diag), out.ctypes.data))
    return out


def _factor(A):
    L, lib = _lib()
    A = np.asfortranarray(A)
    Lf, Uf = np.zeros_like(A, order="F"), np.zeros_like(A, order="F")
    L.check(lib.admm_hip_test_cholesky_linvt(int(A.dtype == np.float64), A.ctypes.data, A.shape[0], Lf.ctypes.data, Uf.ctypes.data))
    return Lf, Uf


# ------------------------------------------------------------------------------------------------------------ factor and U
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cond", [30.0, 1e3])
@pytest.mark.parametrize("n", [1, 2, 5, 127, 128, 129, 257, 385])
def test_factor_and_linvt_against_lapack(n, cond, dtype):
    """L backward (||L L' - A||_max / ||A||_max) and U = L^-T (||U' L - I||_max), each within 5 x the figure LAPACK's potrf /
    trtri reach in the same precision on the same matrix; U exactly zero below its diagonal.  Above L's diagonal the input stays
    where no launch writes: the tiles strictly above the diagonal and the first diagonal tile (potf2_inv_kernel stores rows >=
    columns only).  The later diagonal tiles are whole output tiles of the LOWER trailing update (test_gemm_lower_leaves_the_upper
    _tiles_alone pins that granularity): their upper halves hold the Schur complement's mirror entries, which nothing reads."""
    A = np.asfortranarray(spd(n, cond).astype(dtype))
    A64 = A.astype(np.float64)
    if dtype == np.float32:
        assert_float32_positive_definite(A)
    Lf, Uf = _factor(A)
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    up &= ~_lower_tiles(n) | (np.arange(n)[None, :] < 128)
    assert np.array_equal(_bits(Lf)[up], _bits(A)[up])
    assert not Uf[np.tril(np.ones((n, n), dtype=bool), -1)].any()
    potrf, trtri = (lapack.spotrf, lapack.strtri) if dtype == np.float32 else (lapack.dpotrf, lapack.dtrtri)
    Ll, info = potrf(A, lower=1, clean=1)
    assert info == 0
    Li, info = trtri(Ll, lower=1)
    assert info == 0
    L64, Ll64 = np.tril(Lf).astype(np.float64), np.tril(Ll).astype(np.float64)
    back = lambda F: float(np.abs(F @ F.T - A64).max() / np.abs(A64).max())
    b_lib, b_lap = back(L64), back(Ll64)
    u_lib = float(np.abs(Uf.astype(np.float64).T @ L64 - np.eye(n)).max())
    u_lap = float(np.abs(np.tril(Li).astype(np.float64) @ Ll64 - np.eye(n)).max())
    print(f"[factor {dtype.__name__} n={n} cond={cond:g}] ||LL' - A|| / ||A||: {b_lib:.2e} (LAPACK potrf {b_lap:.2e})   "
          f"||U'L - I||: {u_lib:.2e} (LAPACK trtri {u_lap:.2e})")
    assert b_lib <= 5 * b_lap, (b_lib, b_lap)
    assert u_lib <= 5 * u_lap, (u_lib, u_lap)


# ------------------------------------------------------------------------------------------------------------ inverse
ORDERS = [1, 2, 3, 5, 127, 128, 129, 255, 257, 384, 385]
CONDS = [30.0, 1e3, 1e5]


def _check_inverse(tag, A64_full, precision, key, run=_inverse):
    """One inverse under its bound; returns (Ainv, A64 as the library saw it, bound description) for the callers that compare
    routes.  Precision 0 / 1: residual against 5 x LAPACK in the same precision.  Precision 2: one float rounding of a double
    inverse, entrywise."""
    dtype = np.float64 if precision == 1 else np.float32
    A = np.asfortranarray(A64_full.astype(dtype))
    A64 = A.astype(np.float64)
    if dtype == np.float32:
        assert_float32_positive_definite(A)
    Ainv = run(A, precision)
    assert np.array_equal(Ainv, Ainv.T)
    res = residual(A64, Ainv)
    if precision in (0, 1):
        res_lap = residual(A64, lapack_inverse(A))
        print(f"[inverse {tag} precision={precision}] ||A Ainv - I||_max {res:.2e} (LAPACK in the same precision: {res_lap:.2e})")
        assert res <= 5 * res_lap, (tag, precision, res, res_lap)
        return Ainv, A64, 5 * res_lap
    exact, e64 = exact_of(key, A64)
    bound = 2.0 ** -24 * np.abs(exact) + 5 * e64
    err = np.abs(Ainv.astype(np.float64) - exact)
    print(f"[inverse {tag} precision=2] worst |Ainv - exact| / (2^-24 |exact| + 5 e64) {float((err / bound).max()):.3f}  "
          f"(e64 = {e64:.2e}, max |exact| = {np.abs(exact).max():.2e}, ||A Ainv - I||_max {res:.2e})")
    assert np.all(err <= bound), (tag, float((err / bound).max()))
    return Ainv, A64, bound


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("cond", CONDS)
@pytest.mark.parametrize("n", ORDERS)
def test_inverse_small_orders_and_conditioning(n, cond, precision):
    """Every order at which the blocked driver takes another shape (one partial block; a last block of one row; whole blocks)
    at cond 30, 1e3 and 1e5, under a metric that grows with cond."""
    _check_inverse(f"n={n} cond={cond:g}", spd(n, cond), precision, ("spd", n, cond))


def _scaled_error(X, exact):
    d = np.sqrt(np.diag(exact))
    return np.abs(X.astype(np.float64) - exact) / (d[:, None] * d[None, :])


def _check_graded(precision, run=_inverse):
    """D A D, n = 300: errors scaled by sqrt(exact_ii exact_jj) (the inverse's entries span twelve orders of magnitude), 5 x
    LAPACK in the same precision on that figure; precision 2: half an ulp plus 5 x LAPACK float64's scaled figure."""
    dtype = np.float64 if precision == 1 else np.float32
    A = np.asfortranarray(graded().astype(dtype))
    A64 = A.astype(np.float64)
    if dtype == np.float32:
        assert_float32_positive_definite(A)
    exact, _ = exact_of(("graded", precision == 1), A64)
    Ainv = run(A, precision)
    assert np.array_equal(Ainv, Ainv.T)
    e_lib = _scaled_error(Ainv, exact)
    if precision in (0, 1):
        e_lap = float(_scaled_error(lapack_inverse(A), exact).max())
        print(f"[inverse graded n=300 precision={precision}] max |Ainv - exact| / sqrt(exact_ii exact_jj) {float(e_lib.max()):.2e} "
              f"(LAPACK in the same precision: {e_lap:.2e})")
        assert e_lib.max() <= 5 * e_lap, (precision, float(e_lib.max()), e_lap)
        return Ainv, exact, 5 * e_lap
    d = np.sqrt(np.diag(exact))
    e64s = float(_scaled_error(lapack_inverse(A64), exact).max())
    bound = 2.0 ** -24 * np.abs(exact) / (d[:, None] * d[None, :]) + 5 * e64s
    print(f"[inverse graded n=300 precision=2] worst scaled error / (2^-24 |exact| / sqrt(..) + 5 e64) {float((e_lib / bound).max()):.3f} (scaled e64 = {e64s:.2e})")
    assert np.all(e_lib <= bound)
    return Ainv, exact, bound


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_inverse_graded_scaling(precision):
    _check_graded(precision)


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("n,cond", [(5, 30.0), (5, 1e3), (5, 1e5), (129, 30.0), (129, 1e3), (129, 1e5)])
def test_inverse_rocsolver_route_same_bounds_and_agreement(n, cond, precision):
    """ADMM_HIP_FACTOR=rocsolver on the same inputs: the same bounds, and the two routes agree to the sum of their bounds
    (residual metric: A (X1 - X2) = (A X1 - I) - (A X2 - I))."""
    import admm_amd
    X1, A64, b1 = _check_inverse(f"n={n} cond={cond:g} mfma", spd(n, cond), precision, ("spd", n, cond))
    with admm_amd.options(FACTOR="rocsolver"):
        X2, _, b2 = _check_inverse(f"n={n} cond={cond:g} rocsolver", spd(n, cond), precision, ("spd", n, cond))
    if precision == 2:
        assert np.all(np.abs(X1.astype(np.float64) - X2.astype(np.float64)) <= b1 + b2)
    else:
        assert np.abs(A64 @ (X1.astype(np.float64) - X2.astype(np.float64))).max() <= b1 + b2


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_inverse_rocsolver_route_graded(precision):
    import admm_amd
    X1, exact, b1 = _check_graded(precision)
    with admm_amd.options(FACTOR="rocsolver"):
        X2, _, b2 = _check_graded(precision)
    d = np.sqrt(np.diag(exact))
    assert np.all(np.abs(X1.astype(np.float64) - X2.astype(np.float64)) / (d[:, None] * d[None, :]) <= b1 + b2)


# ------------------------------------------------------------------------------------------------------------ the float shift
def _shifted(A32, diag):
    """What the library must invert: A with the FLOAT sum A_ii + diag on its diagonal, everything else widened."""
    S = A32.astype(np.float64)
    S[np.diag_indices_from(S)] = (np.diag(A32) + np.float32(diag)).astype(np.float64)
    return S


def _check_shift(tag, A32, diag):
    A32 = np.asfortranarray(A32, dtype=np.float32)
    S = _shifted(A32, diag)
    in_double = np.diag(A32).astype(np.float64) + float(diag)
    assert np.any(np.diag(S) != in_double), "the float and the double sum coincide: this input cannot tell them apart"
    _, info = lapack.dpotrf(S, lower=1)
    assert info == 0
    exact, X0 = refined_inverse(S)
    e64 = float(np.abs(X0 - exact).max())
    Ainv = _inverse_shift(A32, diag)
    assert np.array_equal(Ainv, Ainv.T)
    bound = 2.0 ** -24 * np.abs(exact) + 5 * e64
    err = np.abs(Ainv.astype(np.float64) - exact)
    # the same figure for the inverse of the double sum: how far the wrong addition would be from the bound
    wrong = np.linalg.inv(S - np.diag(np.diag(S)) + np.diag(in_double))
    print(f"[shift {tag} diag={float(diag):.4g}] worst |Ainv - exact| / (2^-24 |exact| + 5 e64) {float((err / bound).max()):.3f}  (e64 = {e64:.2e}; "
          f"the inverse with diag added in double would score {float((np.abs(wrong - exact) / bound).max()):.2f} before its rounding)")
    assert np.all(err <= bound), (tag, float((err / bound).max()))


@pytest.mark.parametrize("which", ["0.37", "1e-3 mean"])
@pytest.mark.parametrize("n,cond", [(5, 1e3), (127, 1e3), (128, 30.0), (129, 1e3), (385, 1e3)])
def test_shifted_inverse_adds_rho_in_float(n, cond, which):
    """spd_inverse_f32_via_f64 with the rho shift: the inverse of the matrix whose diagonal is the float sum, rounded once."""
    A32 = spd(n, cond).astype(np.float32)
    assert_float32_positive_definite(A32)
    diag = 0.37 if which == "0.37" else 1e-3 * float(np.diag(A32).astype(np.float64).mean())
    _check_shift(f"n={n} cond={cond:g}", A32, diag)


@pytest.mark.parametrize("which", ["0.37", "1e-3 mean"])
def test_shifted_inverse_of_a_rank_deficient_gram(which):
    """X'X of 200 rows at order 300: positive definite only through the shift."""
    X = np.random.default_rng(300).standard_normal((200, 300))
    A32 = ((X.T @ X) / 200.0).astype(np.float32)
    assert np.linalg.eigvalsh(A32.astype(np.float64))[0] < 1e-6
    diag = 0.37 if which == "0.37" else 1e-3 * float(np.diag(A32).astype(np.float64).mean())
    _check_shift("rank-deficient Gram n=300", A32, diag)


# ------------------------------------------------------------------------------------------------------------ not SPD
def _dominant(n, seed=0):
    rng = np.random.default_rng(n + seed)
    A = rng.uniform(-1.0, 1.0, (n, n))
    A = 0.5 * (A + A.T)
    A[np.diag_indices(n)] = n + 1.0
    return A


def _refused(A, precision):
    from admm_amd._lib import AdmmHipError
    with pytest.raises(AdmmHipError) as e:
        _inverse(A.astype(np.float64 if precision == 1 else np.float32), precision)
    return e.value


def _good_inverse_still_passes(precision):
    """After a refusal the next inverse on the same thread, of a good matrix, passes its bound."""
    _check_inverse("after a refusal: n=129 cond=30", spd(129, 30.0), precision, ("spd", 129, 30.0))


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("n,k", [(5, 0), (100, 99), (129, 128), (300, 127), (300, 128), (385, 384)])
def test_not_spd_names_the_first_failing_pivot(n, k, precision):
    """A diagonally dominant matrix with A[k, k] = -5: the leading minors are untouched, so pivot k (reported 1-based) is the
    first to fail -- the last pivot of a block, the first of the next, a last block of one row."""
    A = _dominant(n)
    A[k, k] = -5.0
    err = _refused(A, precision)
    assert err.code == 5 and f"(pivot {k + 1})" in str(err), str(err)
    _good_inverse_still_passes(precision)


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("n", [5, 200])
def test_not_spd_all_ones(n, precision):
    """Integers: after the first step the second pivot is exactly zero in float and in double."""
    err = _refused(np.ones((n, n)), precision)
    assert err.code == 5 and "(pivot 2)" in str(err), str(err)
    _good_inverse_still_passes(precision)


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_not_spd_nan_on_the_diagonal(precision):
    """One NaN at (130, 130): no earlier pivot column reads it, pivot 131 is the first that is not a positive number."""
    A = _dominant(300)
    A[130, 130] = np.nan
    err = _refused(A, precision)
    assert err.code == 5 and "(pivot 131)" in str(err), str(err)
    _good_inverse_still_passes(precision)


# ------------------------------------------------------------------------------------------------------------ Gram split-K
def _gram(A, atA):
    L, lib = _lib()
    A = np.asfortranarray(A)
    k = A.shape[1] if atA else A.shape[0]
    G = np.zeros((k, k), dtype=A.dtype, order="F")
    L.check(lib.admm_hip_test_gram(A.ctypes.data, A.shape[0], A.shape[1], int(atA), int(A.dtype == np.float64), G.ctypes.data))
    return G


GRAM_CASES = [
    # float: split-K goes to 16 (gram_mfma_f32: fewer than 512 tiles, K / 2048 >= 16)
    (33001, 129, True, np.float32),       # 3 tiles, K = 33001 ragged against 16 x 16: ksplit = 16
    (300, 70000, False, np.float32),      # AA' of the wide solver: 6 tiles, ksplit = 16
    # double: gram_mfma_f64 picks S in 2 .. 4 while K / S >= 4096 and tiles x S fit the 2 x CUs resident workgroups (256 CUs: 512)
    (16400, 100, True, np.float64),       # 1 tile, 16400 / 4 = 4100: S = 4 (shares of 4104, 4104, 4104, 4088)
    (9000, 300, True, np.float64),        # 6 tiles, 9000 / 2 = 4500, 9000 / 3 < 4096: S = 2
] + [(r, c, atA, dt) for (r, c) in [(1, 1), (5, 3), (40, 1)] for atA in (True, False) for dt in DTYPES]


@pytest.mark.parametrize("rows,cols,atA,dtype", GRAM_CASES)
def test_gram_split_k_and_small_orders(rows, cols, atA, dtype):
    """The Gram where its K range is cut into shares summed in a fixed order (float: 16 shares; double: S = 4 and S = 2 with
    their own summing kernel, K >= 8192) and at orders below one tile: the tolerances of test_gram_vs_numpy, the entrywise
    (K + 3) u |A|'|A| bound, mirrored exactly."""
    rng = np.random.default_rng(rows + cols)
    A = (rng.standard_normal((rows, cols)) * 2 + 0.3).astype(dtype)
    G = _gram(A, atA)
    Z = A.astype(np.float64) if atA else A.astype(np.float64).T
    ref, mag = Z.T @ Z, np.abs(Z).T @ np.abs(Z)
    assert np.array_equal(G, G.T)
    rel = float(np.abs(G - ref).max() / np.abs(ref).max())
    bound = (Z.shape[0] + 3) * U[dtype] * mag
    print(f"[gram {dtype.__name__} {rows}x{cols} {'AtA' if atA else 'AAt'}] max error / max entry {rel:.2e}; worst |G - ref| / bound {_worst(G, ref, bound):.4f}")
    assert rel < (2e-5 if dtype == np.float32 else 1e-13)
    assert np.all(np.abs(G - ref) <= bound)
