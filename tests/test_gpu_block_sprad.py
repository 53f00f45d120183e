"""The spectral radii admm_hip_parbp takes for its column blocks (sharing_bp.hip: sbp_sprad_batch, Lanczos runs batched by block on
launch_gemv_t_batch<double>) through the hook admm_hip_test_block_sprad, block by block against numpy.linalg.norm(A_b, 2) ** 2 -- the
solver's tests see only their mean, through rho.

The bounds.  The run iterates on the fp64 Gram matrix G_b = fl(A_b A_b'), whose rounding dG_b is bounded from the data: every entry
is a sum of p_b products, |dG_b| <= p_b 2^-53 |A_b| |A_b|' entry by entry, so ||dG_b||_2 <= p_b 2^-53 || |A_b| ||_2^2.  Then
    out[b] >= lambda_b (1 - 1e-14) - ||dG_b||      the unsafe side: an under-estimate breaks the majorisation of the x-update
    out[b] <= lambda_b (1 + 1e-8) + ||dG_b||       1e-8 is what the code itself accepts on its 600-step exit.
Every test prints its figures ("block_sprad ..." lines, pytest -s): profiles/gemv_family_tests.md."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_EIGS = 6


def _sprad(A, nblocks):
    from admm_amd import _lib
    A = np.asfortranarray(A, dtype=np.float64)
    out, ns = np.full(nblocks, np.nan), np.full(nblocks, -1, np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.check(_lib.load().admm_hip_test_block_sprad(A.ctypes.data_as(dp), A.shape[0], A.shape[1], nblocks, out.ctypes.data_as(dp),
                                                     ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    return out, ns


def _partition(p, nblocks):
    """solve_parbp's: nblocks - 1 blocks of p div nblocks columns, the last takes the rest."""
    chunk = p // nblocks
    return [slice(b * chunk, p if b == nblocks - 1 else (b + 1) * chunk) for b in range(nblocks)]


def _bounds(Ab):
    lam = np.linalg.norm(Ab, 2) ** 2
    dG = Ab.shape[1] * 2.0 ** -53 * np.linalg.norm(np.abs(Ab), 2) ** 2
    return lam, lam * (1 - 1e-14) - dG, lam * (1 + 1e-8) + dG


def _check(A, nblocks, what):
    out, ns = _sprad(A, nblocks)
    for b, cols in enumerate(_partition(A.shape[1], nblocks)):
        lam, lo, hi = _bounds(A[:, cols])
        print("block_sprad %s: block %d of %d, %d x %d, steps %d, out / lambda - 1 = %.3g, slack below %.3g" %
              (what, b, nblocks, A.shape[0], A[:, cols].shape[1], ns[b], out[b] / lam - 1 if lam > 0 else out[b], (out[b] - lo) / max(lam, 1e-300)))
        assert lo <= out[b] <= hi, (what, b, out[b], lam, lo, hi)
    return out, ns


@pytest.mark.parametrize("n,nblocks,p", [(48, 64, 127), (48, 30, 89)])
def test_blocks_in_lockstep_finish_at_their_own_steps(n, nblocks, p):
    """Gaussian blocks of different widths in one batch.  The partition gives every block but the last p div nblocks columns, so the
    widths differ most where that is small: 63 blocks of ONE column and a last one of 64 (wider than n = 48); 29 blocks of two columns
    and a last one of 31 (narrower than n: rank 31, the Krylov space runs out before n steps).  They advance in lockstep and are judged
    at different steps; each value within the bounds, and bit for bit the value the hook returns for that block alone."""
    rng = np.random.default_rng(n + p)
    A = rng.standard_normal((n, p))
    parts = _partition(p, nblocks)
    widths = [c.stop - c.start for c in parts]
    assert widths == [p // nblocks] * (nblocks - 1) + [p - (nblocks - 1) * (p // nblocks)] and widths[0] in (1, 2) and widths[-1] in (64, 31)
    out, ns = _check(A, nblocks, "lockstep")
    assert ns[-1] > ns[:-1].max() and ns.min() >= 1 and ns.max() <= n
    for b in (0, 1, nblocks // 2, nblocks - 1):
        alone, ns1 = _sprad(A[:, parts[b]], 1)
        assert alone[0].tobytes() == out[b].tobytes() and ns1[0] == ns[b], (b, alone[0], out[b], ns1[0], ns[b])


def test_degenerate_orders_and_ranks():
    """n = 1 (the first step is the answer), n = 2 (two steps span the space), a rank-one block and a block of zeros (||w|| = 0 after
    the first step: the `bb <= 1e-300` exit, where the value is exactly 0) beside Gaussian blocks that keep stepping."""
    rng = np.random.default_rng(8)
    out, ns = _check(rng.standard_normal((1, 3)), 2, "n=1")
    assert ns.tolist() == [1, 1]
    out, ns = _check(rng.standard_normal((2, 5)), 2, "n=2")
    assert ns.max() <= 2
    n = 40
    A = rng.standard_normal((n, 35))                                          # 11 | 11 | 13 columns
    A[:, :11] = np.outer(rng.standard_normal(n), rng.standard_normal(11))
    out, ns = _check(A, 3, "rank one")
    assert ns[0] < ns[2]
    Z = rng.standard_normal((n, 17))                                          # 5 | 5 | 7 columns
    Z[:, :5] = 0.0
    out, ns = _check(Z, 3, "zero block")
    assert out[0] == 0.0 and ns[0] == 1 and np.isfinite(out).all()


def _clustered(rest):
    """n = 640, one block U diag(s) V' whose two largest squared singular values are 1 and 1 - 1e-9, the others rest(k), k = 1 .. n - 2."""
    n = 640
    rng = np.random.default_rng(640)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s2 = np.concatenate([[1.0, 1.0 - 1e-9], rest(np.arange(1, n - 1) / n)])
    A = (U * np.sqrt(s2)) @ V.T
    sv = np.linalg.svd(A, compute_uv=False) ** 2
    assert 0.5e-9 < (sv[0] - sv[1]) / sv[0] < 2e-9 and sv[2] < 1 - 5e-5
    return A


def test_clustered_top_eigenvalues_take_the_600_step_exit():
    """The two top eigenvalues 1e-9 apart and the others DENSE below them (1 - 1e-4 - (k / n)^2 / 4): the Krylov space needs more than 600
    of the 640 dimensions before the Ritz pair's residual passes 1e-14 (a float64 restatement of the loop on this spectrum: 3e-11 to
    5e-11 after 600 steps, 1e-12 and 7e-10 with the quarter replaced by 0.2 and 0.3), so the block leaves through the 600-step exit.
    Either the value comes back from there (theta + r) within both bounds -- never below the lower one -- or the call raises
    ADMM_ERR_EIGS.  Measured on an MI355X: see profiles/gemv_family_tests.md."""
    from admm_amd._lib import AdmmHipError
    A = _clustered(lambda t: 1.0 - 1e-4 - 0.25 * t ** 2)
    try:
        out, ns = _check(A, 1, "clustered, dense below")
    except AdmmHipError as e:
        assert e.code == ERR_EIGS
        print("block_sprad clustered, dense below: ADMM_ERR_EIGS")
        return
    assert ns[0] == 600


def test_clustered_top_eigenvalues_over_a_separated_rest():
    """The same pair over a rest that is far below (0.25 * 0.97^k): the pair's span converges within a dozen steps to a blend of the two
    (residual 5e-10, above the 1e-14 bound), rounding then brings the second direction in and the run ends well before 600 steps with
    the larger of the two -- within the bounds, in particular not the blend, which lies 2.4e-10 below."""
    A = _clustered(lambda t: 0.25 * 0.97 ** (640 * t - 1))
    out, ns = _check(A, 1, "clustered, separated rest")
    assert 12 <= ns[0] < 100
