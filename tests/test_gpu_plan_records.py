"""GPU: the decision trace and the iterate dump of a prepared plan (admm_hip_lasso_plan_trace_* / _state_*), for the three
solvers that record them -- what a reader gets when its capacity is below the number of decisions, and when one plan runs twice.
The smallest shapes at which each plan still takes all of its usual launches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (n, p, $parallel() blocks, solver branch in the stats, floats of one iterate record)
CASES = {
    "tall": (64, 16, 0, 0, lambda n, p: 5 * p),                    # x | z | y | adj_z | adj_y
    "wide": (16, 64, 0, 1, lambda n, p: p + 3 * n),                # x | A x | z | y; fused RT = 4, persistent stretch on
    "parallel2": (40, 24, 2, 2, lambda n, p: (1 + 2 * 2) * p),     # z | x_k, y_k of the two blocks
}


def _plan(n, p, nthread):
    from admm_amd import admm_lasso
    from admm_amd.api import LassoPlan
    rng = np.random.default_rng(20240 + n + p)
    x = rng.standard_normal((n, p))
    y = x[:, :3] @ np.array([1.5, -1.0, 0.5]) + 0.5 * rng.standard_normal(n)
    m = admm_lasso(x, y).penalty(nlambda=3)
    if nthread:
        m.nthread = nthread
    return LassoPlan(m)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", sorted(CASES))
def test_records_full_clipped_and_repeated(case):
    n, p, nthread, branch, rec_floats = CASES[case]
    rec = rec_floats(n, p)
    # 1. full records
    a = _plan(n, p, nthread)
    a.enable_trace(1 << 12)
    a.enable_state(1 << 12)
    fit = a.run()
    T, S = a.read_trace(), a.read_state().copy()
    N = len(T)
    assert fit.stats["branch"] == branch
    assert 8 < N < (1 << 12), N                                    # the capacities below really clip, those above do not
    assert S.shape == (N, rec), (S.shape, N, rec)
    # 2. clipped records: the first ones, bit for bit, and nothing else changes
    b = _plan(n, p, nthread)
    b.enable_trace(5)
    b.enable_state(3)
    fit_b = b.run()
    Tb, Sb = b.read_trace(), b.read_state().copy()
    b.close()
    assert Tb.shape == (5, T.shape[1]) and _same(Tb, T[:5])
    assert Sb.shape == (3, rec) and _same(Sb, S[:3])
    assert _same(fit_b.beta_dense, fit.beta_dense) and _same(fit_b.niter, fit.niter) and _same(fit_b.lambda_, fit.lambda_)
    # 3. a second run() of the same plan: the same records and results, byte for byte
    fit2 = a.run()
    T2, S2 = a.read_trace(), a.read_state().copy()
    a.close()
    assert _same(T2, T) and _same(S2, S)
    assert _same(fit2.beta_dense, fit.beta_dense) and _same(fit2.niter, fit.niter)
