"""GPU: the box-constrained, weighted elastic net on the tall path (admm_hip_boxenet, tall_box_tail_kernel) against the Lasso, the
elastic net and the sparse-group lasso it must reduce to, and against the NumPy restatement of its iteration (tests/box_oracle.py).

Shapes -- the group tests' own, the smallest at which either tail form can go wrong:
  B1  n = 600, p = 230 (gemv tail): p no multiple of 32, the last workgroup holds 6 of 32 coordinates;
  B2  n = 2304, p = 2100 (symv tail, p >= 2048).
10 lambdas, lambda_min_ratio 0.01, eps 1e-5, fixed seeds.  The pattern (box_oracle.box_pattern): a quarter of the columns non-negative,
a quarter capped at 0.25, a quarter in [-0.1, 0.1], a quarter free, every 37th excluded, factors in [0.5, 2] with two columns unpenalised."""
import numpy as np
import pytest

import box_oracle as bo
import group_oracle as go
from helpers import traced_fit

pytestmark = pytest.mark.gpu

F = np.float32
NLAM, LMR = 10, 0.01
SHAPES = {"B1": bo.B1, "B2": bo.B2}
_cache = {}


def _shared(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _data(shape):
    return _shared(("data", shape), lambda: bo.synth_box(*SHAPES[shape]))


def _pattern(shape):
    return bo.box_pattern(SHAPES[shape][1])


def _pen(**pen):
    return dict(dict(nlambda=NLAM, lambda_min_ratio=LMR), **pen)


def _box(x, y, lower=None, upper=None, u=None, alpha=None, standardize=True, intercept=True, **pen):
    from admm_amd import admm_boxenet
    return admm_boxenet(x, y, lower, upper, intercept=intercept, standardize=standardize).penalty(alpha=alpha, penalty_factor=u, **_pen(**pen))


def _plain(x, y, alpha=None, standardize=True, intercept=True, **pen):
    from admm_amd import admm_enet, admm_lasso
    if alpha is None:
        return admm_lasso(x, y, intercept, standardize).penalty(**_pen(**pen))
    return admm_enet(x, y, intercept, standardize).penalty(alpha=alpha, **_pen(**pen))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _plain_pair(shape, alpha):
    """(fit, trace) of admm_lasso / admm_enet on the shape (shared: the factor test takes its grid from here)."""
    x, y = _data(shape)
    return _shared(("plain", shape, alpha), lambda: traced_fit(_plain(x, y, alpha)))


def _pattern_fit(shape, alpha=None):
    """The library's fit of the shape with the test pattern (shared by the tests that only read it)."""
    x, y = _data(shape)
    lower, upper, u = _pattern(shape)
    return _shared(("pattern", shape, alpha), lambda: _box(x, y, lower, upper, u, alpha).fit())


# ---- 1. without bounds and factors it is the existing solver

@pytest.mark.parametrize("alpha", [None, 0.5])
@pytest.mark.parametrize("shape", ["B1", "B2"])
def test_without_bounds_and_factors_it_is_the_lasso_or_the_elastic_net_byte_for_byte(shape, alpha):
    """u = 1 gives lambda / rho exactly and a clamp to (-inf, inf) is the identity: grid, beta, niter and the decision trace of
    admm_lasso (alpha None) / admm_enet (0.5), on the x-update variant that p selects."""
    x, y = _data(shape)
    fit_p, tr_p = _plain_pair(shape, alpha)
    fit_b, tr_b = traced_fit(_box(x, y, alpha=alpha))
    assert fit_b.stats["branch"] == 0 and fit_b.stats["xupdate_variant"] == fit_p.stats["xupdate_variant"] == (1 if x.shape[1] >= 2048 else 0)
    assert fit_p.niter.max() <= 10000 and np.count_nonzero(fit_p.beta_dense[1:, -1]) > 0
    m = min(len(tr_b), len(tr_p))
    print(f"[box plain {shape} alpha={alpha}] trace records {len(tr_b)} / {len(tr_p)}, {int(np.sum(np.any(tr_b[:m] != tr_p[:m], axis=1)))} differ")
    assert _same(fit_b.lambda_, fit_p.lambda_) and _same(fit_b.niter, fit_p.niter)
    assert _same(fit_b.beta_dense, fit_p.beta_dense)
    assert len(tr_b) == len(tr_p) > NLAM and _same(tr_b, tr_p)


@pytest.mark.parametrize("alpha", [None, 0.5])
@pytest.mark.parametrize("standardize,intercept", [(True, True), (True, False), (False, True), (False, False)])
def test_infinite_bounds_and_unit_factors_given_as_arrays_change_nothing(standardize, intercept, alpha):
    """B1 under the four standardisations, the bounds passed as arrays of -+infinity and the factors as ones."""
    x, y = _data("B1")
    p = x.shape[1]
    fit_p, tr_p = traced_fit(_plain(x, y, alpha, standardize, intercept))
    fit_b, tr_b = traced_fit(_box(x, y, np.full(p, -np.inf), np.full(p, np.inf), np.ones(p), alpha, standardize, intercept))
    assert _same(fit_b.lambda_, fit_p.lambda_) and _same(fit_b.niter, fit_p.niter)
    assert _same(fit_b.beta_dense, fit_p.beta_dense)
    assert len(tr_b) == len(tr_p) > NLAM and _same(tr_b, tr_p)


# ---- 2. factors alone

@pytest.mark.parametrize("shape", ["B1", "B2"])
def test_factors_alone_are_the_sparse_group_lasso_at_alpha_one_on_singletons(shape):
    """Lasso prox, u from the pattern (two columns unpenalised), no bounds, on the Lasso's own grid passed as lambda_: beta, niter and
    the decision trace of admm_sgl(alpha = 1, l1_weights = u) with every column a group of its own."""
    from admm_amd import admm_sgl
    x, y = _data(shape)
    p = x.shape[1]
    u = _pattern(shape)[2]
    grid = [float(v) for v in _plain_pair(shape, None)[0].lambda_]
    fit_b, tr_b = traced_fit(_box(x, y, u=u, lambda_=grid))
    fit_s, tr_s = traced_fit(admm_sgl(x, y, np.arange(p), alpha=1.0).penalty(l1_weights=u, lambda_=grid))
    assert fit_b.lambda_.tolist() == grid == fit_s.lambda_.tolist()
    assert fit_s.niter.max() <= 10000 and np.all(np.any(fit_s.beta_dense[1:][u == 0] != 0, axis=1))
    assert _same(fit_b.niter, fit_s.niter) and _same(fit_b.beta_dense, fit_s.beta_dense)
    assert len(tr_b) == len(tr_s) > NLAM and _same(tr_b, tr_s)


# ---- 3. every iteration

@pytest.mark.parametrize("alpha", [None, 0.5])
@pytest.mark.parametrize("shape", ["B1", "B2"])
def test_every_iteration_applies_the_clamped_prox_and_the_dual_update(shape, alpha):
    """Iterate dump with the pattern: in every record z is box_prox of the record's own x, adj_y, rho and lambda EXACTLY (element-wise,
    no sums), and y = fl(adj_y + rho (x - z)) exactly.  The bounds in solver units are formed as the library forms them, from the
    standardisation's floats (box_oracle.library_scales).  Record 0 is the cold start."""
    x, y = _data(shape)
    p = x.shape[1]
    lower, upper, u = _pattern(shape)
    lo, hi = bo.std_bounds(lower, upper, *bo.library_scales(x, y), p)
    free_lo, free_hi = np.full(p, -np.inf, F), np.full(p, np.inf, F)
    fit, tr, S = traced_fit(_box(x, y, lower, upper, u, alpha), capacity=1 << 13, state=True)
    N = len(tr)
    assert tr[0, 8] == -1 and S.shape == (N, 5 * p) and NLAM < N < (1 << 13)
    assert fit.niter.max() <= 10000
    fixed = lo == hi
    n_lo = n_hi = bad_z = bad_y = 0
    for s in range(1, N):
        xs, z, ys, adjz, adjy = S[s].reshape(5, p)
        rho, lam = tr[s, 9], tr[s, 11]
        v = (xs + adjy / F(rho)).astype(F)
        z_ref = bo.box_prox(v, u, lo, hi, lam, rho, alpha)
        z_free = bo.box_prox(v, u, free_lo, free_hi, lam, rho, alpha)
        y_ref = (adjy + F(rho) * (xs - z).astype(F)).astype(F)
        bad_z += int(np.sum(z != z_ref))
        bad_y += int(np.sum(ys != y_ref))
        n_lo += int(np.sum((z_free < lo) & (z == lo) & ~fixed))
        n_hi += int(np.sum((z_free > hi) & (z == hi) & (hi != 0) & ~fixed))
        assert np.all(z[fixed] == 0), (shape, alpha, s)
    print(f"[box stepwise {shape} alpha={alpha}] {N - 1} iterations: {bad_z} z and {bad_y} y entries differ from the restatement; "
          f"clamped at a lower bound {n_lo} times, at a non-zero upper bound {n_hi} times; {int(fixed.sum())} excluded columns stayed 0")
    assert bad_z == 0 and bad_y == 0
    assert n_lo > 0 and n_hi > 0 and fixed.sum() > 0                  # the clamp was at work on both sides


# ---- 4. the output box

@pytest.mark.parametrize("shape", ["B1", "B2"])
def test_the_output_lies_in_the_callers_box(shape):
    """Every returned coefficient within the caller's bounds, compared in double; excluded columns exactly 0; at the last lambda some
    coefficient sits on a non-zero bound (within four float spacings: the recovery to the original scale rounds)."""
    lower, upper, u = _pattern(shape)
    fit = _pattern_fit(shape)
    b = fit.beta_dense[1:].astype(np.float64)
    assert fit.niter.max() <= 10000
    assert np.all(b >= lower[:, None]) and np.all(b <= upper[:, None])
    assert np.all(fit.beta_dense[1:][lower == upper] == 0)
    last = b[:, -1]
    near = lambda bound: np.isfinite(bound) & (bound != 0) & (np.abs(last - bound) <= 4.0 * np.spacing(np.abs(bound).astype(F)))
    at = near(lower) | near(upper)
    print(f"[box output {shape}] niter {fit.niter.tolist()}; at the last lambda {int(at.sum())} coefficients on a non-zero bound, "
          f"{int(np.sum((last == 0) & (lower == 0) & (upper != 0)))} held at a zero lower bound, {np.count_nonzero(last)} non-zero")
    assert at.sum() >= 1


# ---- 5. KKT

@pytest.mark.parametrize("alpha", [None, 0.5])
def test_the_pattern_meets_the_kkt_conditions_of_the_bounded_problem(alpha):
    """B1 with the pattern: the path maximum of box_kkt is at most 3 x the restatement's from this same run (floor 1e-4).  3: the
    figure at the stopping iteration varies with the trajectory by up to 10 x from lambda to lambda, the path maximum is stable
    (tests/test_gpu_grplasso.py, tests/test_gpu_sgl.py)."""
    x, y = _data("B1")
    lower, upper, u = _pattern("B1")
    fit = _pattern_fit("B1", alpha)
    ref = bo.box_path(x, y, lower, upper, u, alpha, nlambda=NLAM, lmin_ratio=LMR)
    assert np.allclose(fit.lambda_, ref["lam"], rtol=1e-5)
    b = go.to_standardised(fit.beta_dense, ref["std"])
    lam_int = fit.lambda_ * ref["Xs"].shape[0] / np.float64(ref["std"].scaleY)
    lib = float(bo.box_kkt(ref["Xs"], ref["Ys"], b, lam_int, u, ref["lo"], ref["hi"], alpha).max())
    res = float(bo.box_kkt(ref["Xs"], ref["Ys"], ref["beta_std"], ref["lam_int"], u, ref["lo"], ref["hi"], alpha).max())
    print(f"[box kkt B1 alpha={alpha}] library {lib:.3e} niter {fit.niter.tolist()}")
    print(f"[box kkt B1 alpha={alpha}] restated {res:.3e} niter {ref['niter'].tolist()}")
    assert fit.niter.max() <= 10000
    assert lib <= max(3.0 * res, 1e-4), (lib, res)


# ---- 6. distance to the optimum

@pytest.mark.parametrize("alpha", [None, 0.5])
def test_distance_to_the_optimum_is_the_float32_restatements(alpha):
    """Against the float64 restatement at eps 1e-9 as the optimum, on the library's own grid: the library's max |beta - beta_opt|
    (standardised units) per lambda is at most 3 x that of the float32 restatement at eps 1e-5, floor 1e-6."""
    x, y = _data("B1")
    lower, upper, u = _pattern("B1")
    fit = _pattern_fit("B1", alpha)
    opt = bo.box_path(x, y, lower, upper, u, alpha, lam=fit.lambda_, eps=1e-9, T=np.float64)
    r32 = bo.box_path(x, y, lower, upper, u, alpha, lam=fit.lambda_, eps=1e-5)
    assert opt["niter"].max() <= 10000
    d_lib = np.abs(go.to_standardised(fit.beta_dense, opt["std"]) - opt["beta_std"]).max(axis=0)
    d_ref = np.abs(r32["beta_std"].astype(np.float64) - opt["beta_std"]).max(axis=0)
    print(f"[box distance B1 alpha={alpha}] library ", " ".join(f"{v:.2e}" for v in d_lib))
    print(f"[box distance B1 alpha={alpha}] restated", " ".join(f"{v:.2e}" for v in d_ref))
    assert np.all(d_lib <= np.maximum(3.0 * d_ref, 1e-6)), (d_lib, d_ref)


# ---- 7. determinism and plumbing

def test_determinism_device_input_user_grid_maxit_and_plan_reruns():
    import torch
    from admm_amd import DevicePtr, admm_boxenet
    from admm_amd.api import LassoPlan
    x, y = _data("B1")
    n, p = x.shape
    lower, upper, u = _pattern("B1")
    a = _pattern_fit("B1")
    b = _box(x, y, lower, upper, u).fit()
    assert _same(a.beta_dense, b.beta_dense) and _same(a.niter, b.niter) and _same(a.lambda_, b.lambda_)
    # device-resident input
    xd = torch.tensor(np.asfortranarray(x).T.copy(), device="cuda")      # p x n row-major == n x p column-major
    yd = torch.tensor(y, device="cuda")
    torch.cuda.synchronize()
    d = admm_boxenet(DevicePtr(xd.data_ptr()), DevicePtr(yd.data_ptr()), lower, upper, n=n, p=p).penalty(penalty_factor=u, **_pen()).fit()
    assert _same(a.beta_dense, d.beta_dense) and _same(a.niter, d.niter)
    # a user grid is honoured
    grid = [float(a.lambda_[2]), float(a.lambda_[5])]
    g = _box(x, y, lower, upper, u, lambda_=grid).fit()
    assert g.lambda_.tolist() == grid and g.beta_dense.shape == (p + 1, 2) and g.niter.min() > 1
    assert np.count_nonzero(g.beta_dense[1:, 1]) >= np.count_nonzero(g.beta_dense[1:, 0]) > 0
    # maxit exhausted: niter = maxit + 1, finite coefficients inside the box
    m = _box(x, y, lower, upper, u).opts(maxit=3).fit()
    assert m.niter.tolist() == [4] * NLAM and np.all(np.isfinite(m.beta_dense))
    assert np.all(m.beta_dense[1:] >= lower[:, None]) and np.all(m.beta_dense[1:] <= upper[:, None])
    # one plan run twice
    plan = LassoPlan(_box(x, y, lower, upper, u))
    r1, r2 = plan.run(), plan.run()
    plan.close()
    assert _same(r1.beta_dense, r2.beta_dense) and _same(r1.niter, r2.niter) and _same(r1.beta_dense, a.beta_dense)


def test_an_attached_communicator_is_refused():
    """A communicator cannot be attached without a device, so this refusal is checked here and not in tests/test_boxenet_host.py."""
    from admm_amd import _lib, dist
    x, y = _data("B1")
    dist.init_comm(1, 0)
    try:
        with pytest.raises(_lib.AdmmHipError, match="single device") as e:
            _box(x, y, lower=0.0).fit()
        assert e.value.code == 1                                              # ADMM_ERR_INVALID_ARG
    finally:
        dist.finalize_comm()


# ---- 8. the early exit of discarded x-update launches

def test_the_early_exit_of_discarded_launches_is_invisible():
    """B2 (symv x-update), the pattern: SYMV_VERDICT=0 and the default give beta, niter and the decision trace identical to the bit."""
    from admm_amd import options
    x, y = _data("B2")
    lower, upper, u = _pattern("B2")
    with options(SYMV_VERDICT=0):
        fit_off, tr_off = traced_fit(_box(x, y, lower, upper, u))
    fit_on, tr_on = traced_fit(_box(x, y, lower, upper, u))
    assert int(fit_on.stats["xupdate_variant"]) == 1
    assert _same(fit_on.lambda_, fit_off.lambda_) and _same(fit_on.niter, fit_off.niter)
    assert _same(fit_on.beta_dense, fit_off.beta_dense) and _same(fit_on.beta_dense, _pattern_fit("B2").beta_dense)
    assert len(tr_on) == len(tr_off) > NLAM and _same(tr_on, tr_off)
