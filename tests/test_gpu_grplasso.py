"""GPU: the group lasso on the tall path (admm_hip_grplasso, tall_group_tail_kernel) against the Lasso it must reduce to and
against the NumPy restatement of its iteration (tests/group_oracle.py).

Shapes -- the smallest at which the tail can go wrong:
  S1  n = 600, p = 230 (gemv tail): groups that straddle the 32-coordinate tiles, of exactly 32, of 33 and of 70 (several passes),
      singletons between large groups, p no multiple of 32;
  S2  n = 2304, p = 2100 (symv tail, p >= 2048): the S1 pattern repeated, one group of 200, a tail of singletons.
10 lambdas, lambda_min_ratio 0.01, eps 1e-5, fixed seeds."""
import numpy as np
import pytest

import group_oracle as go
from helpers import traced_fit

pytestmark = pytest.mark.gpu

F = np.float32
NLAM, LMR = 10, 0.01
SHAPES = {"S1": (600, go.S1_SIZES, 11), "S2": (2304, go.s2_sizes(), 12)}
_cache = {}


def _data(shape):
    if shape not in _cache:
        n, sizes, seed = SHAPES[shape]
        _cache[shape] = go.synth_groups(n, sizes, seed) + (np.asarray(sizes),)
    return _cache[shape]


def _labels(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


def _model(x, y, sizes, weights=None, **pen):
    from admm_amd import admm_grplasso
    pen = dict(dict(nlambda=NLAM, lambda_min_ratio=LMR), **pen)
    return admm_grplasso(x, y, _labels(sizes)).penalty(group_weights=weights, **pen)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _weights_s1():
    w = go.default_weights(go.S1_SIZES)
    w[3], w[9] = 0.0, 0.5
    return w


def _shared(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _lib_s1():
    """The library's default-weight fit of S1 (shared by the tests that only read it)."""
    x, y, sizes = _data("S1")
    return _shared("lib_s1", lambda: _model(x, y, sizes).fit())


@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_singleton_groups_of_weight_one_are_the_lasso_bit_for_bit(shape):
    from admm_amd import admm_lasso
    x, y, _ = _data(shape)
    p = x.shape[1]
    fit_g, tr_g = traced_fit(_model(x, y, np.ones(p, dtype=int), weights=np.ones(p)))
    fit_l, tr_l = traced_fit(admm_lasso(x, y).penalty(nlambda=NLAM, lambda_min_ratio=LMR))
    assert fit_g.stats["branch"] == 0 and fit_g.stats["xupdate_variant"] == fit_l.stats["xupdate_variant"] == (1 if p >= 2048 else 0)
    assert _same(fit_g.lambda_, fit_l.lambda_) and _same(fit_g.niter, fit_l.niter)
    assert _same(fit_g.beta_dense, fit_l.beta_dense)
    assert len(tr_g) == len(tr_l) > NLAM and _same(tr_g, tr_l)
    assert fit_l.niter.max() <= 10000 and np.count_nonzero(fit_l.beta_dense[1:, -1]) > 0


@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_every_iteration_applies_the_group_prox_and_the_dual_update(shape):
    """Iterate dump: in every record z is the restatement's next_z of the record's own x and adj_y, to within one float ulp at |v_i|
    (the double norm differs from NumPy's only in summation order, ~1e-13 relative: derived, not measured); singleton groups bit
    for bit; a group may be zero on one side and not on the other only within 1e-12 of its threshold; y = fl(adj_y + rho (x - z))
    exactly.  Record 0 is the cold start (X'y in the x slot), as for the tall plan."""
    x, y, sizes = _data(shape)
    p = x.shape[1]
    w = go.default_weights(sizes)
    fit, tr, S = traced_fit(_model(x, y, sizes), capacity=1 << 12, state=True)
    N = len(tr)
    assert tr[0, 8] == -1 and S.shape == (N, 5 * p) and NLAM < N < (1 << 12)
    assert fit.niter.max() <= 10000
    gid = _labels(sizes)
    single = (np.asarray(sizes) == 1)[gid]
    worst = 0.0
    for s in range(1, N):
        xs, z, ys, adjz, adjy = S[s].reshape(5, p)
        rho, lam = tr[s, 9], tr[s, 11]
        v = (xs + adjy / F(rho)).astype(F)
        z_ref, nrm, pen = go.group_prox(v, sizes, w, lam, rho, F)
        ulp = np.spacing(np.abs(v))
        err = np.abs(z.astype(np.float64) - z_ref.astype(np.float64))
        worst = max(worst, float(np.max(err / ulp)))
        assert np.all(err <= ulp), (shape, s, int(np.argmax(err / ulp)))
        assert np.array_equal(z[single], z_ref[single]), (shape, s)
        zero_lib = np.add.reduceat((z != 0).astype(np.int64), go.group_starts(sizes)[:-1]) == 0
        zero_ref = np.add.reduceat((z_ref != 0).astype(np.int64), go.group_starts(sizes)[:-1]) == 0
        flip = zero_lib != zero_ref
        assert np.all(np.abs(nrm[flip] - pen[flip]) <= 1e-12 * pen[flip]), (shape, s, np.nonzero(flip)[0][:5])
        y_ref = (adjy + F(rho) * (xs - z).astype(F)).astype(F)
        assert np.array_equal(ys, y_ref), (shape, s)
    print(f"[grplasso stepwise {shape}] {N - 1} iterations, largest |z - z_ref| = {worst:.2f} ulp at |v|")


def _lib_kkt(fit, ref, sizes, w):
    b = go.to_standardised(fit.beta_dense, ref["std"])
    lam_int = fit.lambda_ * ref["Xs"].shape[0] / np.float64(ref["std"].scaleY)
    return go.group_kkt(ref["Xs"], ref["Ys"], b, lam_int, sizes, w), b


def test_weights_zero_and_half_meet_the_group_kkt_conditions():
    """One group unpenalised (weight 0), one at weight 0.5: the unpenalised group is in the model at every lambda, and the path-wide
    maxima of (viol - 1) ratio, on ratio and unp are at most 3 x the restatement's from this same run (floor 1e-4).  3: the figure
    at the stopping iteration varies with the trajectory by up to 10 x from lambda to lambda, the path maximum is stable."""
    x, y, sizes = _data("S1")
    w = _weights_s1()
    fit = _model(x, y, sizes, weights=w).fit()
    ref = go.grp_path(x, y, sizes, w, nlambda=NLAM, lmin_ratio=LMR)
    assert np.allclose(fit.lambda_, ref["lam"], rtol=1e-5)
    st = go.group_starts(sizes)
    assert np.all(np.any(fit.beta_dense[1 + st[3]:1 + st[4]] != 0, axis=0))
    (viol, on, unp), _ = _lib_kkt(fit, ref, sizes, w)
    lib = go.kkt_maxima(viol, on, unp, fit.lambda_)
    rv, ro, ru = go.group_kkt(ref["Xs"], ref["Ys"], ref["beta_std"], ref["lam_int"], sizes, w)
    res = go.kkt_maxima(rv, ro, ru, ref["lam"])
    print(f"[grplasso weights S1] library  (viol-1)*ratio {lib[0]:.3e}  on*ratio {lib[1]:.3e}  unp {lib[2]:.3e}  niter {fit.niter.tolist()}")
    print(f"[grplasso weights S1] restated (viol-1)*ratio {res[0]:.3e}  on*ratio {res[1]:.3e}  unp {res[2]:.3e}  niter {ref['niter'].tolist()}")
    for name, a, b in zip(("(viol-1)*ratio", "on*ratio", "unp"), lib, res):
        assert a <= max(3.0 * b, 1e-4), (name, a, b)


def test_distance_to_the_optimum_is_the_float32_restatements():
    """Against the float64 restatement at eps 1e-9 as the optimum, on the library's own grid: the library's max |beta - beta_opt|
    (standardised units) per lambda is at most 3 x that of the float32 restatement at eps 1e-5, floor 1e-6."""
    x, y, sizes = _data("S1")
    fit = _lib_s1()
    opt = go.grp_path(x, y, sizes, lam=fit.lambda_, eps=1e-9, T=np.float64)
    r32 = go.grp_path(x, y, sizes, lam=fit.lambda_, eps=1e-5)
    assert opt["niter"].max() <= 10000
    d_lib = np.abs(go.to_standardised(fit.beta_dense, opt["std"]) - opt["beta_std"]).max(axis=0)
    d_ref = np.abs(r32["beta_std"].astype(np.float64) - opt["beta_std"]).max(axis=0)
    print("[grplasso distance S1] library ", " ".join(f"{v:.2e}" for v in d_lib))
    print("[grplasso distance S1] restated", " ".join(f"{v:.2e}" for v in d_ref))
    assert np.all(d_lib <= np.maximum(3.0 * d_ref, 1e-6)), (d_lib, d_ref)


def test_determinism_device_input_user_grid_maxit_and_plan_reruns():
    import torch
    from admm_amd import DevicePtr, admm_grplasso
    from admm_amd.api import LassoPlan
    x, y, sizes = _data("S1")
    n, p = x.shape
    a = _lib_s1()
    b = _model(x, y, sizes).fit()
    assert _same(a.beta_dense, b.beta_dense) and _same(a.niter, b.niter) and _same(a.lambda_, b.lambda_)
    # device-resident input
    xd = torch.tensor(np.asfortranarray(x).T.copy(), device="cuda")      # p x n row-major == n x p column-major
    yd = torch.tensor(y, device="cuda")
    torch.cuda.synchronize()
    d = admm_grplasso(DevicePtr(xd.data_ptr()), DevicePtr(yd.data_ptr()), _labels(sizes), n=n, p=p).penalty(nlambda=NLAM, lambda_min_ratio=LMR).fit()
    assert _same(a.beta_dense, d.beta_dense) and _same(a.niter, d.niter)
    # a user grid is honoured, and equals the same values on the automatic grid's path where they coincide
    grid = [float(a.lambda_[2]), float(a.lambda_[5])]
    u = _model(x, y, sizes, lambda_=grid).fit()
    assert u.lambda_.tolist() == grid and u.beta_dense.shape == (p + 1, 2) and u.niter.min() > 1
    assert np.count_nonzero(u.beta_dense[1:, 1]) >= np.count_nonzero(u.beta_dense[1:, 0]) > 0
    # maxit exhausted: niter = maxit + 1, finite coefficients
    m = _model(x, y, sizes).opts(maxit=3).fit()
    assert m.niter.tolist() == [4] * NLAM and np.all(np.isfinite(m.beta_dense))
    # one plan run twice
    plan = LassoPlan(_model(x, y, sizes))
    r1, r2 = plan.run(), plan.run()
    plan.close()
    assert _same(r1.beta_dense, r2.beta_dense) and _same(r1.niter, r2.niter) and _same(r1.beta_dense, a.beta_dense)


def test_scattered_groups_are_reordered_and_put_back():
    x, y, sizes = _data("S1")
    from admm_amd import admm_grplasso
    perm = np.random.default_rng(4).permutation(x.shape[1])
    labels = _labels(sizes)
    a = _lib_s1()
    # the same columns in scattered order with their labels: the same model, coefficient j of the caller's column j
    s = admm_grplasso(x[:, perm], y, labels[perm]).penalty(nlambda=NLAM, lambda_min_ratio=LMR)
    w_by_label = go.default_weights(sizes)[s.group_labels]
    assert np.allclose(s.effective_weights(), w_by_label)
    fit = s.fit()
    assert np.allclose(fit.lambda_, a.lambda_, rtol=1e-5)
    # the groups arrive in another order, so sums run in another order: equal to solver tolerance, not bit for bit
    assert np.abs(fit.beta_dense[1:][np.argsort(perm)] - a.beta_dense[1:]).max() <= 2e-3 * np.abs(a.beta_dense[1:]).max()


def test_active_set_grows_along_the_path():
    """At lambda[0] the penalised model is empty or holds the one group sitting on the threshold (as the Lasso test allows); the
    number of active groups does not fall between lambda indices 2, 5 and 9."""
    x, y, sizes = _data("S1")
    fit = _lib_s1()
    st = go.group_starts(sizes)
    nact = [sum(bool(np.any(fit.beta_dense[1 + st[k]:1 + st[k + 1], l] != 0)) for k in range(len(sizes))) for l in range(NLAM)]
    print("[grplasso active groups S1]", nact)
    assert nact[0] <= 1
    assert 1 <= nact[2] <= nact[5] <= nact[9]
    # a group enters or leaves whole
    for l in range(NLAM):
        for k in range(len(sizes)):
            blk = fit.beta_dense[1 + st[k]:1 + st[k + 1], l] != 0
            assert blk.all() or not blk.any(), (l, k)
