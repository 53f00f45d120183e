"""GPU: the sparse-group lasso on the tall path (admm_hip_sgl, tall_group_tail_kernel<., true>) against the group lasso and the Lasso
it must reduce to, and against the NumPy restatement of its iteration (tests/sgl_oracle.py).

Shapes -- the group tests' own, the smallest at which this tail can go wrong:
  S1  n = 600, p = 230 (gemv tail): groups that straddle the 32-coordinate tiles, of exactly 32, of 33 and of 70 (several passes),
      singletons between large groups, p no multiple of 32;
  S2  n = 2304, p = 2100 (symv tail, p >= 2048): the S1 pattern repeated, one group of 200, a tail of singletons.
10 lambdas, lambda_min_ratio 0.01, eps 1e-5, fixed seeds."""
import numpy as np
import pytest

import group_oracle as go
import sgl_oracle as so
from helpers import traced_fit

pytestmark = pytest.mark.gpu

F = np.float32
NLAM, LMR = 10, 0.01
SHAPES = {"S1": (600, go.S1_SIZES, 11), "S2": (2304, go.s2_sizes(), 12)}
_cache = {}


def _shared(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _data(shape):
    def make():
        n, sizes, seed = SHAPES[shape]
        return go.synth_groups(n, sizes, seed) + (np.asarray(sizes),)
    return _shared(("data", shape), make)


def _labels(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


def _pen(**pen):
    return dict(dict(nlambda=NLAM, lambda_min_ratio=LMR), **pen)


def _sgl(x, y, sizes, alpha, u=None, w=None, **pen):
    from admm_amd import admm_sgl
    return admm_sgl(x, y, _labels(sizes), alpha=alpha).penalty(group_weights=w, l1_weights=u, **_pen(**pen))


def _grp(x, y, sizes, w=None, **pen):
    from admm_amd import admm_grplasso
    return admm_grplasso(x, y, _labels(sizes)).penalty(group_weights=w, **_pen(**pen))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _weights(sizes):
    w = go.default_weights(sizes)
    w[3], w[9] = 0.0, 0.5
    return w


def _u(shape):
    """l1 weights that are not constant: uniform in [0.5, 2], fixed seed."""
    p = int(np.sum(SHAPES[shape][1]))
    return np.random.default_rng(31).uniform(0.5, 2.0, p)


def _lib_s1_half():
    """The library's fit of S1 at alpha = 0.5, default weights (shared by the tests that only read it)."""
    x, y, sizes = _data("S1")
    return _shared("lib_s1_half", lambda: _sgl(x, y, sizes, 0.5).fit())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_alpha_zero_is_the_group_lasso_byte_for_byte(shape, weighted):
    """soft(v, 0) = v and 0 u + 1 w = w exactly: grid, beta, niter and the decision trace of admm_grplasso, with default weights and
    with one group unpenalised and one at weight 0.5; the l1 weights play no part."""
    x, y, sizes = _data(shape)
    w = _weights(sizes) if weighted else None
    fit_s, tr_s = traced_fit(_sgl(x, y, sizes, 0.0, u=_u(shape), w=w))
    fit_g, tr_g = traced_fit(_grp(x, y, sizes, w))
    assert fit_s.stats["xupdate_variant"] == fit_g.stats["xupdate_variant"] == (1 if x.shape[1] >= 2048 else 0)
    assert _same(fit_s.lambda_, fit_g.lambda_) and _same(fit_s.niter, fit_g.niter)
    assert _same(fit_s.beta_dense, fit_g.beta_dense)
    assert len(tr_s) == len(tr_g) > NLAM and _same(tr_s, tr_g)
    assert fit_g.niter.max() <= 10000 and np.count_nonzero(fit_g.beta_dense[1:, -1]) > 0


def _alpha_one_pair(shape):
    def make():
        from admm_amd import admm_lasso
        x, y, sizes = _data(shape)
        return traced_fit(_sgl(x, y, sizes, 1.0)) + traced_fit(admm_lasso(x, y).penalty(**_pen()))
    return _shared(("alpha1", shape), make)


@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_alpha_one_with_unit_weights_is_the_lasso_byte_for_byte(shape):
    """pen_g = 0, so shrink is exactly 1 (or the group is all zero): with the S1 / S2 groupings the grid, beta, niter and the decision
    trace are admm_lasso's, on the x-update variant that p selects.  (The trace holds the residual norms, which are summed tile by
    tile: they are the Lasso's because a call without any block weight is packed on the Lasso tail's tiles.  Packed group by group
    they differed in the last bit -- S1: 95 of 573 records, 4.7e-16 relative; S2: 375 of 741, 5.6e-16 -- with grid, beta and niter equal.)"""
    fit_s, tr_s, fit_l, tr_l = _alpha_one_pair(shape)
    p = fit_l.beta_dense.shape[0] - 1
    assert fit_s.stats["branch"] == 0 and fit_s.stats["xupdate_variant"] == fit_l.stats["xupdate_variant"] == (1 if p >= 2048 else 0)
    assert fit_l.niter.max() <= 10000 and np.count_nonzero(fit_l.beta_dense[1:, -1]) > 0
    m = min(len(tr_s), len(tr_l))
    differ = int(np.sum(np.any(tr_s[:m] != tr_l[:m], axis=1)))
    print(f"[sgl alpha=1 {shape}] trace records {len(tr_s)} / {len(tr_l)}, {differ} differ")
    assert _same(fit_s.lambda_, fit_l.lambda_) and _same(fit_s.niter, fit_l.niter)
    assert _same(fit_s.beta_dense, fit_l.beta_dense)
    assert len(tr_s) == len(tr_l) > NLAM and _same(tr_s, tr_l)


def test_alpha_one_with_l1_weights_is_the_group_lasso_on_singletons():
    """alpha = 1 with u drawn from {0, 0.5, 1, 2} and the S1 grouping, on a user grid (u = 0 leaves coordinates unpenalised): beta and
    niter of admm_grplasso on one-column groups with weights u."""
    x, y, sizes = _data("S1")
    p = x.shape[1]
    u = np.random.default_rng(32).choice([0.0, 0.5, 1.0, 2.0], size=p)
    assert set(np.unique(u)) == {0.0, 0.5, 1.0, 2.0}
    lam = _alpha_one_pair("S1")[2].lambda_
    grid = [float(lam[1]), float(lam[4]), float(lam[7])]
    a = _sgl(x, y, sizes, 1.0, u=u, lambda_=grid).fit()
    b = _grp(x, y, np.ones(p, dtype=int), w=u, lambda_=grid).fit()
    assert a.lambda_.tolist() == grid == b.lambda_.tolist()
    assert _same(a.niter, b.niter) and _same(a.beta_dense, b.beta_dense)
    assert b.niter.max() <= 10000 and np.all(np.any(a.beta_dense[1:][u == 0] != 0, axis=1))
    # the same holds whenever no group carries a block weight: alpha = 0.5 with every w_g = 0 is the Lasso with penalty factors u / 2
    c = _sgl(x, y, sizes, 0.5, u=u, w=np.zeros(len(sizes)), lambda_=grid).fit()
    d = _grp(x, y, np.ones(p, dtype=int), w=0.5 * u, lambda_=grid).fit()
    assert _same(c.niter, d.niter) and _same(c.beta_dense, d.beta_dense)


@pytest.mark.parametrize("alpha", [0.5, 0.95])
@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_every_iteration_applies_the_two_level_prox_and_the_dual_update(shape, alpha):
    """Iterate dump: in every record z is the restatement's next_z of the record's own x, adj_y, rho and lambda to within one float ulp
    at |v_j| (s is the same float on both sides; only the summation order of the double norm differs, ~1e-13 relative: derived, not
    measured); one-column groups bit for bit; a group may be zero on one side only within 1e-12 of its threshold;
    y = fl(adj_y + rho (x - z)) exactly.  Record 0 is the cold start."""
    x, y, sizes = _data(shape)
    p = x.shape[1]
    u = _u(shape)
    l1, wg, _ = so.sgl_weights(sizes, alpha, u, None)
    fit, tr, S = traced_fit(_sgl(x, y, sizes, alpha, u=u), capacity=1 << 12, state=True)
    N = len(tr)
    assert tr[0, 8] == -1 and S.shape == (N, 5 * p) and NLAM < N < (1 << 12)
    assert fit.niter.max() <= 10000
    st = go.group_starts(sizes)
    single = (np.asarray(sizes) == 1)[_labels(sizes)]
    worst, nmixed = 0.0, 0
    for s in range(1, N):
        xs, z, ys, adjz, adjy = S[s].reshape(5, p)
        rho, lam = tr[s, 9], tr[s, 11]
        v = (xs + adjy / F(rho)).astype(F)
        z_ref, s_ref, nrm, pen = so.sgl_prox(v, sizes, l1, wg, lam, rho, F)
        ulp = np.spacing(np.abs(v))
        err = np.abs(z.astype(np.float64) - z_ref.astype(np.float64))
        worst = max(worst, float(np.max(err / ulp)))
        assert np.all(err <= ulp), (shape, alpha, s, int(np.argmax(err / ulp)))
        assert np.array_equal(z[single], z_ref[single]), (shape, alpha, s)
        zero_lib = np.add.reduceat((z != 0).astype(np.int64), st[:-1]) == 0
        zero_ref = np.add.reduceat((z_ref != 0).astype(np.int64), st[:-1]) == 0
        flip = zero_lib != zero_ref
        assert np.all(np.abs(nrm[flip] - pen[flip]) <= 1e-12 * pen[flip]), (shape, alpha, s, np.nonzero(flip)[0][:5])
        y_ref = (adjy + F(rho) * (xs - z).astype(F)).astype(F)
        assert np.array_equal(ys, y_ref), (shape, alpha, s)
        nz = np.add.reduceat((z != 0).astype(np.int64), st[:-1])
        nmixed += bool(np.any((nz > 0) & (nz < np.asarray(sizes))))
    assert nmixed > 0                                   # the element-wise threshold was at work inside surviving groups
    print(f"[sgl stepwise {shape} alpha={alpha}] {N - 1} iterations, largest |z - z_ref| = {worst:.2f} ulp at |v|, "
          f"{nmixed} iterations with zeros inside a surviving group")


@pytest.mark.parametrize("alpha", [0.5, 0.95])
def test_weights_zero_and_half_meet_the_kkt_conditions(alpha):
    """S1 with one group weight 0 and one 0.5: the path-wide maxima of off ratio, on ratio and unp are at most 3 x the restatement's
    from this same run (floor 1e-4).  3: the figure at the stopping iteration varies with the trajectory by up to 10 x from lambda to
    lambda, the path maximum is stable (tests/test_gpu_grplasso.py)."""
    x, y, sizes = _data("S1")
    w = _weights(sizes)
    l1, wg, _ = so.sgl_weights(sizes, alpha, None, w)
    fit = _sgl(x, y, sizes, alpha, w=w).fit()
    ref = so.sgl_path(x, y, sizes, alpha, None, w, nlambda=NLAM, lmin_ratio=LMR)
    assert np.allclose(fit.lambda_, ref["lam"], rtol=1e-5)
    b = go.to_standardised(fit.beta_dense, ref["std"])
    lam_int = fit.lambda_ * ref["Xs"].shape[0] / np.float64(ref["std"].scaleY)
    lib = so.sgl_kkt_maxima(*so.sgl_kkt(ref["Xs"], ref["Ys"], b, lam_int, sizes, l1, wg), fit.lambda_)
    res = so.sgl_kkt_maxima(*so.sgl_kkt(ref["Xs"], ref["Ys"], ref["beta_std"], ref["lam_int"], sizes, l1, wg), ref["lam"])
    print(f"[sgl weights S1 alpha={alpha}] library  off*ratio {lib[0]:.3e}  on*ratio {lib[1]:.3e}  unp {lib[2]:.3e}  niter {fit.niter.tolist()}")
    print(f"[sgl weights S1 alpha={alpha}] restated off*ratio {res[0]:.3e}  on*ratio {res[1]:.3e}  unp {res[2]:.3e}  niter {ref['niter'].tolist()}")
    assert fit.niter.max() <= 10000
    for name, a_, b_ in zip(("off*ratio", "on*ratio", "unp"), lib, res):
        assert a_ <= max(3.0 * b_, 1e-4), (name, a_, b_)


@pytest.mark.parametrize("alpha", [0.5, 0.95])
def test_distance_to_the_optimum_is_the_float32_restatements(alpha):
    """Against the float64 restatement at eps 1e-9 as the optimum, on the library's own grid: the library's max |beta - beta_opt|
    (standardised units) per lambda is at most 3 x that of the float32 restatement at eps 1e-5, floor 1e-6."""
    x, y, sizes = _data("S1")
    fit = _lib_s1_half() if alpha == 0.5 else _sgl(x, y, sizes, alpha).fit()
    opt = so.sgl_path(x, y, sizes, alpha, lam=fit.lambda_, eps=1e-9, T=np.float64)
    r32 = so.sgl_path(x, y, sizes, alpha, lam=fit.lambda_, eps=1e-5)
    assert opt["niter"].max() <= 10000
    d_lib = np.abs(go.to_standardised(fit.beta_dense, opt["std"]) - opt["beta_std"]).max(axis=0)
    d_ref = np.abs(r32["beta_std"].astype(np.float64) - opt["beta_std"]).max(axis=0)
    print(f"[sgl distance S1 alpha={alpha}] library ", " ".join(f"{v:.2e}" for v in d_lib))
    print(f"[sgl distance S1 alpha={alpha}] restated", " ".join(f"{v:.2e}" for v in d_ref))
    assert np.all(d_lib <= np.maximum(3.0 * d_ref, 1e-6)), (d_lib, d_ref)


def test_groups_enter_along_the_path_and_are_sparse_inside():
    """alpha = 0.5 on S1: at lambda[0] the model is empty or holds the one group sitting on the threshold; the number of active groups
    does not fall across lambda indices 2, 5 and 9; at index 5 a multi-column group holds zero and non-zero coefficients side by
    side -- which admm_grplasso cannot give (its test asserts that a group enters or leaves whole)."""
    x, y, sizes = _data("S1")
    fit = _lib_s1_half()
    nact = [so.active_groups(fit.beta_dense[1:, l], sizes) for l in range(NLAM)]
    mixed = so.mixed_groups(fit.beta_dense[1:, 5], sizes)
    print("[sgl active groups S1]", nact, " groups with zeros and non-zeros at index 5:", mixed)
    assert nact[0] <= 1
    assert 1 <= nact[2] <= nact[5] <= nact[9]
    assert len(mixed) >= 1


def test_determinism_device_input_user_grid_maxit_and_plan_reruns():
    import torch
    from admm_amd import DevicePtr, admm_sgl
    from admm_amd.api import LassoPlan
    x, y, sizes = _data("S1")
    n, p = x.shape
    a = _lib_s1_half()
    b = _sgl(x, y, sizes, 0.5).fit()
    assert _same(a.beta_dense, b.beta_dense) and _same(a.niter, b.niter) and _same(a.lambda_, b.lambda_)
    # device-resident input
    xd = torch.tensor(np.asfortranarray(x).T.copy(), device="cuda")      # p x n row-major == n x p column-major
    yd = torch.tensor(y, device="cuda")
    torch.cuda.synchronize()
    d = admm_sgl(DevicePtr(xd.data_ptr()), DevicePtr(yd.data_ptr()), _labels(sizes), alpha=0.5, n=n, p=p).penalty(**_pen()).fit()
    assert _same(a.beta_dense, d.beta_dense) and _same(a.niter, d.niter)
    # a user grid is honoured
    grid = [float(a.lambda_[2]), float(a.lambda_[5])]
    g = _sgl(x, y, sizes, 0.5, lambda_=grid).fit()
    assert g.lambda_.tolist() == grid and g.beta_dense.shape == (p + 1, 2) and g.niter.min() > 1
    assert np.count_nonzero(g.beta_dense[1:, 1]) >= np.count_nonzero(g.beta_dense[1:, 0]) > 0
    # maxit exhausted: niter = maxit + 1, finite coefficients
    m = _sgl(x, y, sizes, 0.5).opts(maxit=3).fit()
    assert m.niter.tolist() == [4] * NLAM and np.all(np.isfinite(m.beta_dense))
    # one plan run twice
    plan = LassoPlan(_sgl(x, y, sizes, 0.5))
    r1, r2 = plan.run(), plan.run()
    plan.close()
    assert _same(r1.beta_dense, r2.beta_dense) and _same(r1.niter, r2.niter) and _same(r1.beta_dense, a.beta_dense)


def test_scattered_groups_take_l1_weights_in_the_callers_order():
    from admm_amd import admm_sgl
    x, y, sizes = _data("S1")
    u = _u("S1")
    labels = _labels(sizes)
    perm = np.random.default_rng(4).permutation(x.shape[1])
    a = _sgl(x, y, sizes, 0.5, u=u).fit()
    # the same columns in scattered order with their labels and their l1 weights: the same model, coefficient j of the caller's column j
    s = admm_sgl(x[:, perm], y, labels[perm], alpha=0.5).penalty(l1_weights=u[perm], **_pen())
    w_by_label = go.default_weights(sizes)[s.group_labels]
    assert np.allclose(s.effective_weights(), w_by_label)
    fit = s.fit()
    assert np.allclose(fit.lambda_, a.lambda_, rtol=1e-5)
    # the groups arrive in another order, so sums run in another order: equal to solver tolerance, not bit for bit
    assert np.abs(fit.beta_dense[1:][np.argsort(perm)] - a.beta_dense[1:]).max() <= 2e-3 * np.abs(a.beta_dense[1:]).max()
