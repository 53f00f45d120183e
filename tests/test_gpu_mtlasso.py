"""GPU: the multi-task lasso on the tall path (admm_hip_mtlasso: symvn_lower_kernel, tall_mt_tail_kernel) against the kernel and the
Lasso it must reduce to, and against the NumPy restatement (tests/mtlasso_oracle.py: tests/group_oracle.py on a Kronecker design).

Shapes -- the smallest at which the kernels can go wrong:
  (400, 70)     one row strip, p no multiple of 32, three workgroups of the tail;
  (600, 264)    two strips with a ragged last one (264 = 256 + 8): the smallest p at which a response's partial planes hold more than
                one row block, so that a wrong plane stride shows (the restatement at m = 5 takes ~3 s here, ~15 s at (1300, 600));
  (1100, 520)   three strips with a ragged last one (520 = 2 * 256 + 8);
  (2304, 2100)  diagonal and interior tiles under the default schedule (bit-level tests only: the restatement needs ~25 s there).
Response counts: the tail walks a row's responses in chunks of 4 (kMtChunk, lasso_tall.hip), so m <= 3 runs the first chunk only.  m = 5
and 6 reach the second chunk (with 1 and 2 live slots), m = 13 the last one with a single live slot, m = 16 = ADMM_HIP_MT_MAX fills
all four; with 2 m right-hand sides these also give x-update passes that are full, partly filled and (MT_RHS = 12, m = 5) a single one.
10 lambdas, lambda_min_ratio 0.01, eps 1e-5, fixed seeds."""
import ctypes

import numpy as np
import pytest

import group_oracle as go
import mtlasso_oracle as mo
from helpers import traced_fit

pytestmark = pytest.mark.gpu

F = np.float32
NLAM, LMR = 10, 0.01
_fp = ctypes.POINTER(ctypes.c_float)
_cache = {}


def _shared(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _data(n, p, m):
    return _shared(("data", n, p, m), lambda: mo.synth_mt(n, p, m, seed=n + p))


def _model(x, Y, weights=None, **kw):
    from admm_amd import admm_mtlasso
    return admm_mtlasso(x, Y, **kw).penalty(nlambda=NLAM, lambda_min_ratio=LMR, row_weights=weights)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _weights(p):
    w = np.ones(p)
    w[3], w[7] = 0.0, 0.5
    return w


def _rhs_values():
    from admm_amd import _lib
    return _lib.MT_RHS_BUILT


# ---- 1. the kernel against the existing kernel
def _sym(p, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((p, p)).astype(F)
    return np.asfortranarray(np.tril(B) + np.tril(B, -1).T, dtype=F)


def _symv2(A, v0, v1):
    from admm_amd import _lib
    lib = _lib.load()
    p = A.shape[0]
    A = np.asfortranarray(A, dtype=F)
    y0, y1 = np.empty(p, F), np.empty(p, F)
    _lib.check(lib.admm_hip_test_symv(A.ctypes.data_as(_fp), p, v0.ctypes.data_as(_fp), v1.ctypes.data_as(_fp), y0.ctypes.data_as(_fp), y1.ctypes.data_as(_fp)))
    return y0, y1


def _symvn(A, V, rhs):
    from admm_amd import _lib
    lib = _lib.load()
    nr, p = V.shape
    A = np.asfortranarray(A, dtype=F)
    out = np.empty((nr, p), F)
    _lib.check(lib.admm_hip_test_symv_multi(A.ctypes.data_as(_fp), p, np.ascontiguousarray(V).ctypes.data_as(_fp), nr, rhs, out.ctypes.data_as(_fp)))
    return out


def _kernel_case(p):
    """A, 32 vectors (dense, sparse and scaled ones) and what the EXISTING kernel returns for each of them (pairs (r, 31 - r))."""
    def make():
        A = _sym(p, p)
        rng = np.random.default_rng(p + 1)
        V = rng.standard_normal((32, p)).astype(F)
        V[1::3] *= (rng.uniform(size=(V[1::3].shape)) < 0.1)
        V[2::5] *= 100.0
        V = np.ascontiguousarray(V)
        ref = np.empty_like(V)
        for r in range(16):
            ref[r], ref[31 - r] = _symv2(A, V[r], V[31 - r])
        return A, V, ref
    return _shared(("kernel", p), make)


@pytest.mark.parametrize("p", [37, 520, 2100])
def test_multi_vector_kernel_is_the_two_vector_kernel_bit_for_bit(p):
    A, V, ref = _kernel_case(p)
    A64 = A.astype(np.float64)
    exact = V.astype(np.float64) @ A64                                        # row r = A v_r (A symmetric)
    scale = np.abs(V.astype(np.float64)) @ np.abs(A64)
    Ap = A.copy()
    Ap[np.triu_indices(p, 1)] = np.nan
    for rhs in _rhs_values():
        for nr in (2, 6, 10, 32):
            out = _symvn(A, V[:nr], rhs)
            assert _same(out, ref[:nr]), (p, rhs, nr, int(np.argmax(np.any(out != ref[:nr], axis=1))))
            for r in range(nr):                                               # the bound of tests/test_gpu_symv.py
                assert np.abs(out[r] - exact[r]).max() / scale[r].max() <= 1e-6, (p, rhs, nr, r)
                assert np.linalg.norm(out[r] - exact[r]) / np.linalg.norm(exact[r]) <= 1e-6, (p, rhs, nr, r)
        assert _same(_symvn(Ap, V[:6], rhs), ref[:6]), (p, rhs, "the strict upper triangle was read")


# ---- 2. m = 1 is the Lasso
@pytest.mark.parametrize("standardize,intercept", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("n,p", [(400, 70), (1100, 520), (2304, 2100)])
def test_one_response_is_the_lasso_bit_for_bit(n, p, standardize, intercept):
    from admm_amd import _lib, admm_lasso
    x, Y = _data(n, p, 3)
    y = np.ascontiguousarray(Y[:, 1])
    fit_m, tr_m = traced_fit(_model(x, y, intercept=intercept, standardize=standardize))
    lasso = admm_lasso(x, y, intercept=intercept, standardize=standardize).penalty(nlambda=NLAM, lambda_min_ratio=LMR)
    if p < 2048:
        with _lib.options(XUPDATE="sym"):
            fit_l, tr_l = traced_fit(lasso)
    else:
        fit_l, tr_l = traced_fit(lasso)
    assert fit_m.stats["branch"] == 0 and fit_m.stats["xupdate_variant"] == fit_l.stats["xupdate_variant"] == 1
    assert _same(fit_m.lambda_, fit_l.lambda_) and _same(fit_m.niter, fit_l.niter)
    assert fit_m.beta_dense.shape == (1, p + 1, NLAM) and _same(fit_m.beta_dense[0], fit_l.beta_dense)
    assert len(tr_m) == len(tr_l) > NLAM and _same(tr_m, tr_l)
    assert np.count_nonzero(fit_l.beta_dense[1:, -1]) > 0


# ---- 3. MT_RHS is invisible
@pytest.mark.parametrize("n,p,m", [(1100, 520, 3), (2304, 2100, 2), (1100, 520, 5), (400, 70, 16)])
def test_right_hand_sides_per_pass_are_invisible_and_runs_repeat(n, p, m):
    from admm_amd import _lib
    x, Y = _data(n, p, m)
    runs = {}
    for rhs in (0,) + tuple(_rhs_values()):
        with _lib.options(MT_RHS=rhs):
            runs[rhs] = traced_fit(_model(x, Y))
    with _lib.options(MT_RHS=8):
        again = traced_fit(_model(x, Y))
    f0, t0 = runs[0]
    assert f0.niter.max() <= 10000 and np.count_nonzero(f0.beta_dense[:, 1:, -1]) > 0
    for rhs, (f, t) in list(runs.items()) + [("8 again", again)]:
        assert _same(f.beta_dense, f0.beta_dense) and _same(f.niter, f0.niter) and _same(f.lambda_, f0.lambda_), rhs
        assert _same(t, t0), rhs


# ---- 4. every iteration applies the prox and the dual update
@pytest.mark.parametrize("n,p,m,rhs", [(400, 70, 3, 0), (2304, 2100, 2, 0), (400, 70, 6, 4), (400, 70, 16, 12), (600, 264, 5, 8)])
def test_every_iteration_applies_the_row_prox_and_the_dual_update(n, p, m, rhs):
    """Iterate dump ([5][m][p] per record): z is tests/group_oracle.py's group_prox of the record's own v = x + adj_y / rho with groups
    = rows, to one float ulp at |v| (the double norm differs from NumPy's only in summation order); a row may be zero on one side only
    within 1e-12 of its threshold; y = fl(adj_y + rho (x - z)) exactly.  The rules and constants of
    test_every_iteration_applies_the_group_prox_and_the_dual_update."""
    from admm_amd import _lib
    x, Y = _data(n, p, m)
    w = _weights(p)
    with _lib.options(MT_RHS=rhs):
        fit, tr, S = traced_fit(_model(x, Y, w), capacity=1 << 12, state=True)
    N = len(tr)
    assert tr[0, 8] == -1 and S.shape == (N, 5 * p * m) and NLAM < N < (1 << 12)
    assert fit.niter.max() <= 10000
    sizes = [m] * p
    starts = go.group_starts(sizes)[:-1]
    rows = lambda a: np.ascontiguousarray(a.T).reshape(-1)                      # [m][p] -> the Kronecker order j m + k
    worst = 0.0
    for s in range(1, N):
        xs, z, ys, adjz, adjy = (rows(a) for a in S[s].reshape(5, m, p))
        rho, lam = tr[s, 9], tr[s, 11]
        v = (xs + adjy / F(rho)).astype(F)
        z_ref, nrm, pen = go.group_prox(v, sizes, w, lam, rho, F)
        ulp = np.spacing(np.abs(v))
        err = np.abs(z.astype(np.float64) - z_ref.astype(np.float64))
        worst = max(worst, float(np.max(err / ulp)))
        assert np.all(err <= ulp), (s, int(np.argmax(err / ulp)))
        zero_lib = np.add.reduceat((z != 0).astype(np.int64), starts) == 0
        zero_ref = np.add.reduceat((z_ref != 0).astype(np.int64), starts) == 0
        flip = zero_lib != zero_ref
        assert np.all(np.abs(nrm[flip] - pen[flip]) <= 1e-12 * pen[flip]), (s, np.nonzero(flip)[0][:5])
        y_ref = (adjy + F(rho) * (xs - z).astype(F)).astype(F)
        assert np.array_equal(ys, y_ref), s
    print(f"[mtlasso stepwise ({n}, {p}, {m}) MT_RHS={rhs}] {N - 1} iterations, largest |z - z_ref| = {worst:.2f} ulp at |v|")


# ---- 5. against the restatement
def _kkt_against_the_restatement(n, p, m, w, standardize=True, intercept=True):
    """One library fit and one float32 restatement run of the same problem: the lambda grid, then the group KKT figures on the Kronecker
    design, each at most 3 x the restatement's figure from this same run (floor 1e-4): tests/test_gpu_grplasso.py's own bound."""
    x, Y = _data(n, p, m)
    tag = f"({n}, {p}, {m})" + ("" if standardize and intercept else f" standardize={standardize} intercept={intercept}")
    fit = _model(x, Y, w, standardize=standardize, intercept=intercept).fit()
    ref = mo.mt_path(x, Y, w, nlambda=NLAM, lmin_ratio=LMR, standardize=standardize, intercept=intercept)
    assert fit.niter.max() <= 10000 and ref["niter"].max() <= 10000
    assert np.allclose(fit.lambda_, ref["lam"], rtol=1e-5)
    b_lib = mo.to_standardised(fit.beta_dense, ref["std"])
    lam_int = fit.lambda_ * n / np.float64(ref["std"].scaleY)
    ww = np.ones(p) if w is None else w
    lib = go.kkt_maxima(*go.group_kkt(ref["K"], ref["yv"], b_lib, lam_int, ref["sizes"], ww), fit.lambda_)
    res = go.kkt_maxima(*go.group_kkt(ref["K"], ref["yv"], ref["beta_std"], ref["lam_int"], ref["sizes"], ww), ref["lam"])
    print(f"[mtlasso {tag}] library  (viol-1)*ratio {lib[0]:.3e}  on*ratio {lib[1]:.3e}  unp {lib[2]:.3e}  niter {fit.niter.tolist()}")
    print(f"[mtlasso {tag}] restated (viol-1)*ratio {res[0]:.3e}  on*ratio {res[1]:.3e}  unp {res[2]:.3e}  niter {ref['niter'].tolist()}")
    for name, a, b in zip(("(viol-1)*ratio", "on*ratio", "unp"), lib, res):
        assert a <= max(3.0 * b, 1e-4), (name, a, b)
    return x, Y, fit, ref


@pytest.mark.parametrize("n,p,m", [(400, 70, 3), (1100, 520, 3), (600, 264, 5), (400, 70, 13)])
def test_weighted_path_against_the_restatement(n, p, m):
    """Weights with a 0 and a 0.5.  Group KKT figures on the Kronecker design and the distance to the float64 optimum, each at most
    3 x the float32 restatement's figure from this same run (floors 1e-4 / 1e-6): tests/test_gpu_grplasso.py's own bounds."""
    w = _weights(p)
    x, Y, fit, ref = _kkt_against_the_restatement(n, p, m, w)
    assert np.all(np.all(fit.beta_dense[:, 1 + 3, :] != 0, axis=0))            # the unpenalised row, every response, every lambda
    opt = mo.mt_path(x, Y, w, lam=fit.lambda_, eps=1e-9, T=np.float64)
    r32 = mo.mt_path(x, Y, w, lam=fit.lambda_, eps=1e-5)
    assert opt["niter"].max() <= 10000
    d_lib = np.abs(mo.to_standardised(fit.beta_dense, opt["std"]) - opt["beta_std"]).max(axis=0)
    d_ref = np.abs(r32["beta_std"].astype(np.float64) - opt["beta_std"]).max(axis=0)
    print(f"[mtlasso distance ({n}, {p}, {m})] library ", " ".join(f"{v:.2e}" for v in d_lib))
    print(f"[mtlasso distance ({n}, {p}, {m})] restated", " ".join(f"{v:.2e}" for v in d_ref))
    assert np.all(d_lib <= np.maximum(3.0 * d_ref, 1e-6)), (d_lib, d_ref)


@pytest.mark.parametrize("standardize,intercept", [(True, False), (False, True), (False, False)])
def test_the_other_standardisation_rules_against_the_restatement(standardize, intercept):
    """Several responses under the three flag values the weighted test does not take, as tests/mtlasso_oracle.py's standardise states
    them: the common scale about the means without centring (standardize only), own means with the common scale and X unscaled
    (intercept only), nothing at all.  The lambda grid depends on scaleY and the KKT figures are taken in the restatement's units, so
    a wrong scale or a wrong centring misses the same bounds as above.  The intercepts: exactly 0 without `intercept`; with it, meanY_k - sum_j coef_jk meanX_j recomputed in double from the
    library's own coefficients, to the rounding of a float sum of p + 1 terms ((p + 2) float epsilons of the terms' absolute sum)."""
    n, p, m = 400, 70, 3
    x, Y, fit, ref = _kkt_against_the_restatement(n, p, m, None, standardize, intercept)
    assert np.count_nonzero(fit.beta_dense[:, 1:, -1]) > 0
    b0 = fit.beta_dense[:, 0, :].astype(np.float64)
    if not intercept:
        assert not b0.any()
        return
    coef = fit.beta_dense[:, 1:, :].astype(np.float64)                           # (m, p, nlambda)
    mx, my = x.mean(axis=0), Y.mean(axis=0)
    want = my[:, None] - np.einsum("kjl,j->kl", coef, mx)
    room = (p + 2) * np.finfo(F).eps * (np.abs(my)[:, None] + np.einsum("kjl,j->kl", np.abs(coef), np.abs(mx)))
    assert np.all(np.abs(b0 - want) <= room), float(np.max(np.abs(b0 - want) / room))


# ---- 6. identical responses stay identical
@pytest.mark.parametrize("m,rhs", [(3, 0), (6, 12), (16, 8)])
def test_identical_responses_get_identical_coefficients(m, rhs):
    from admm_amd import _lib
    x, Y = _data(400, 70, 3)
    y = Y[:, 0]
    with _lib.options(MT_RHS=rhs):
        fit = _model(x, np.column_stack([y] * m)).fit()
    assert fit.niter.max() <= 10000 and np.count_nonzero(fit.beta_dense[0, 1:, -1]) > 0
    for k in range(1, m):
        assert _same(fit.beta_dense[0], fit.beta_dense[k]), k


# ---- 7. plan lifecycle
def test_a_plan_runs_twice_like_the_one_shot_call():
    from admm_amd.api import LassoPlan
    x, Y = _data(400, 70, 3)
    one = _model(x, Y).fit()
    plan = LassoPlan(_model(x, Y))
    r1, r2 = plan.run(), plan.run()
    plan.close()
    assert one.beta_dense.shape == (3, 71, NLAM)
    for r in (r1, r2):
        assert _same(r.beta_dense, one.beta_dense) and _same(r.niter, one.niter) and _same(r.lambda_, one.lambda_)


# ---- 8. a single device only
def test_an_attached_communicator_is_refused():
    """A communicator cannot be attached without a device (admm_hip_comm_init looks for one first), so this refusal is checked here
    and not in tests/test_mtlasso_host.py."""
    from admm_amd import _lib, dist
    x, Y = _data(400, 70, 3)
    dist.init_comm(1, 0)
    try:
        with pytest.raises(_lib.AdmmHipError, match="single device") as e:
            _model(x, Y).fit()
        assert e.value.code == 1                                              # ADMM_ERR_INVALID_ARG
    finally:
        dist.finalize_comm()
    assert _model(x, Y).fit().niter.max() <= 10000                             # and runs again once it is detached
