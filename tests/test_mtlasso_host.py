"""Multi-task lasso (admm_hip_mtlasso), everything that needs no GPU: the declared / exported symbols, what the C ABI refuses before
it looks for a device, the Python builder, the MT_RHS option, and the NumPy restatement (tests/mtlasso_oracle.py), which at m = 1
with weight 1 must be tests/group_oracle.py with singleton groups -- already shown to restate the Lasso oracle exactly."""
import ctypes
import os
import re

import numpy as np
import pytest

import group_oracle as go
import mtlasso_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 2
MT_MAX = 16


def _call(entry="mtlasso", n=6, p=4, m=2, weights=None, x="ok", Y="ok", opts=(10, 1e-5, 1e-5, -1.0), nlambda_auto=5, lmin_ratio=0.01, mem=0):
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    mm = max(m, 1)
    rng = np.random.default_rng(11)                      # a well-posed problem: where there is a device, a valid call runs
    xa = np.asfortranarray(rng.standard_normal((max(n, 1), max(p, 1))))
    Ya = np.asfortranarray(rng.standard_normal((max(n, 1), mm)))
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    o = AdmmOpts(*opts)
    nl = nlambda_auto + 1
    lam_out, beta, nit = np.zeros(nl), np.zeros((max(p, 1) + 1) * mm * nl, dtype=np.float32), np.zeros(nl, dtype=np.int32)
    head = (ctypes.c_void_p(xa.ctypes.data) if x == "ok" else None, ctypes.c_void_p(Ya.ctypes.data) if Y == "ok" else None, n, p, m, mem,
            None if w is None else w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None, 0, nlambda_auto, lmin_ratio, 1, 1, ctypes.byref(o))
    if entry == "mtlasso":
        rc = lib.admm_hip_mtlasso(*head, lam_out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                  beta.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nit.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None)
    else:
        h = ctypes.c_void_p()
        rc = lib.admm_hip_mtlasso_plan_create(*head, ctypes.byref(h), None)
        assert h.value is None or rc == 0
        if rc == 0:
            lib.admm_hip_lasso_plan_destroy(h)
    return rc, lib.admm_hip_last_error().decode()


REFUSALS = [
    (dict(m=0), "number of responses"),
    (dict(m=-3), "number of responses"),
    (dict(n=40, p=4, m=MT_MAX + 1), "number of responses"),
    (dict(n=4, p=4), "built for n > p only"),
    (dict(n=3, p=4), "built for n > p only"),
    (dict(Y=None), "must not be NULL"),
    (dict(x=None), "must not be NULL"),
    (dict(weights=(1.0, -0.5, 1.0, 1.0)), "finite and non-negative"),
    (dict(weights=(1.0, np.nan, 1.0, 1.0)), "finite and non-negative"),
    (dict(weights=(1.0, np.inf, 1.0, 1.0)), "finite and non-negative"),
    (dict(weights=(0.0, 0.0, 0.0, 0.0)), "at least one row weight must be positive"),
    # what check_common / PathSpec::check() refuse for every path entry point
    (dict(n=0), "n and p must be positive"),
    (dict(mem=7), "mem must be"),
    (dict(opts=(0, 1e-5, 1e-5, -1.0)), "maxit should be positive"),
    (dict(nlambda_auto=0), "need a lambda grid"),
    (dict(lmin_ratio=1.0), "lambda_min_ratio"),
]
# An attached communicator is refused too, but none can be attached without a device (admm_hip_comm_init looks for one first): that
# refusal is tests/test_gpu_mtlasso.py's test_an_attached_communicator_is_refused.


def test_symbols_are_declared_and_exported():
    from admm_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "admm_hip.h")).read(), flags=re.S)
    for sym in ("admm_hip_mtlasso", "admm_hip_mtlasso_plan_create", "admm_hip_test_symv_multi"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym) and sym in _lib.EXPORTS
    assert re.search(r"#define\s+ADMM_HIP_MT_MAX\s+16\b", hdr) and _lib.MT_MAX == MT_MAX


@pytest.mark.parametrize("entry", ["mtlasso", "mtlasso_plan_create"])
def test_c_abi_refuses_bad_multi_task_calls_before_it_looks_for_a_device(entry):
    for spoil, fragment in REFUSALS:
        rc, msg = _call(entry, **spoil)
        assert rc == INVALID_ARG and fragment in msg, (entry, spoil, rc, msg)


def test_refine_is_refused_not_ignored():
    from admm_amd import _lib
    with _lib.options(REFINE="1"):
        for entry in ("mtlasso", "mtlasso_plan_create"):
            rc, msg = _call(entry)
            assert rc == INVALID_ARG and "REFINE" in msg, (entry, rc, msg)


def test_the_largest_response_count_passes_the_checks_and_one_more_does_not():
    # m = ADMM_HIP_MT_MAX gets as far as the device (or runs, where there is one); m + 1 is refused by the checks
    rc, msg = _call(n=40, p=4, m=MT_MAX, opts=(1, 1e-5, 1e-5, -1.0), nlambda_auto=1)
    assert rc in (0, NO_DEVICE), (rc, msg)
    rc, msg = _call(n=40, p=4, m=MT_MAX + 1, opts=(1, 1e-5, 1e-5, -1.0), nlambda_auto=1)
    assert rc == INVALID_ARG and "number of responses" in msg


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a machine without a GPU")
def test_valid_multi_task_calls_find_no_device():
    for entry in ("mtlasso", "mtlasso_plan_create"):
        for kw in (dict(), dict(m=1), dict(weights=(0.0, 2.0, 0.5, 1.0)), dict(m=MT_MAX, n=40)):
            rc, msg = _call(entry, **kw)
            assert rc == NO_DEVICE, (entry, kw, rc, msg)


def test_mt_rhs_is_checked_when_it_is_set():
    from admm_amd import _lib
    lib = _lib.load()
    _lib.options.reset()
    try:
        assert _lib.MT_RHS_BUILT == (2, 4, 8, 12)
        for v in (b"0",) + tuple(str(k).encode() for k in _lib.MT_RHS_BUILT):
            assert lib.admm_hip_option_set(b"MT_RHS", v) == 0
            assert lib.admm_hip_option_get(b"ADMM_HIP_MT_RHS") == v
        for bad in (b"1", b"3", b"6", b"16", b"-2", b"two", b""):
            assert lib.admm_hip_option_set(b"MT_RHS", bad) == INVALID_ARG, bad
            assert b"MT_RHS" in lib.admm_hip_last_error()
            assert lib.admm_hip_option_get(b"MT_RHS") == b"12"              # a refused value changes nothing
    finally:
        _lib.options.reset()
    assert lib.admm_hip_option_get(b"MT_RHS") is None


def test_builder_shapes_weights_and_refusals():
    from admm_amd import admm_mtlasso, ADMM_MTLasso, ADMM_Lasso, DevicePtr
    rng = np.random.default_rng(5)
    x = rng.standard_normal((20, 6))
    Y = rng.standard_normal((20, 3))
    mdl = admm_mtlasso(x, Y)
    assert isinstance(mdl, ADMM_MTLasso) and isinstance(mdl, ADMM_Lasso)
    assert (mdl.n, mdl.p, mdl.m) == (20, 6, 3) and mdl.row_weights is None and mdl.y.flags.f_contiguous
    assert admm_mtlasso(x, Y[:, 0]).m == 1                                     # a vector is one response
    mdl.penalty(nlambda=4, lambda_min_ratio=0.1, row_weights=[1.0, 0.0, 2.5, 1, 1, 1]).opts(maxit=50, eps_abs=1e-6)
    assert mdl.row_weights.tolist() == [1.0, 0.0, 2.5, 1, 1, 1] and mdl.nlambda == 4 and mdl.lambda_min_ratio == 0.1 and mdl.maxit == 50
    for bad, frag in (([1.0, 2.0], "one entry per column"), ([1.0, -1.0, 1, 1, 1, 1], "non-negative"), ([1.0, np.nan, 1, 1, 1, 1], "finite"),
                      ([0.0] * 6, "positive")):
        with pytest.raises(ValueError, match=frag):
            mdl.penalty(row_weights=bad)
    with pytest.raises(ValueError, match="n > p only"):
        admm_mtlasso(x[:6], Y[:6])
    with pytest.raises(ValueError, match="should be equal"):
        admm_mtlasso(x, Y[:19])
    with pytest.raises(ValueError, match="number of responses"):
        admm_mtlasso(rng.standard_normal((40, 3)), rng.standard_normal((40, MT_MAX + 1)))
    with pytest.raises(ValueError, match="is needed with a device pointer"):
        admm_mtlasso(DevicePtr(4096), DevicePtr(8192), n=20, p=6)
    d = admm_mtlasso(DevicePtr(4096), DevicePtr(8192), n=20, p=6, m=4)
    assert d.m == 4
    for call in (lambda: mdl.parallel(2), lambda: mdl.cv(3), lambda: mdl.fit_responses(np.zeros((20, 2)))):
        with pytest.raises(ValueError, match="not available for the multi-task lasso"):
            call()


def test_fit_object_has_one_coefficient_matrix_per_response():
    from admm_amd.api import ADMM_MTLasso_fit
    nl, m, p = 3, 2, 4
    raw = np.arange(nl * m * (p + 1), dtype=np.float32).reshape(nl, m, p + 1)      # what the library writes: [nlambda][m][p + 1]
    fit = ADMM_MTLasso_fit(np.array([3.0, 2.0, 1.0]), raw, np.array([5, 6, 7], dtype=np.int32), {})
    assert fit.beta_dense.shape == (m, p + 1, nl)
    for l in range(nl):
        for k in range(m):
            assert np.array_equal(fit.beta_dense[k, :, l], raw[l, k])
    assert len(fit.beta) == m and fit.beta[1].shape == (p + 1, nl)


@pytest.mark.parametrize("standardize,intercept", [(True, True), (True, False), (False, True), (False, False)])
def test_one_response_of_weight_one_is_the_group_oracle_with_singleton_groups(standardize, intercept):
    x, y = go.synth_groups(120, [1] * 17, seed=3)
    ref = go.grp_path(x, y, [1] * 17, np.ones(17), nlambda=6, lmin_ratio=0.05, standardize=standardize, intercept=intercept)
    r = mo.mt_path(x, y.reshape(-1, 1), None, nlambda=6, lmin_ratio=0.05, standardize=standardize, intercept=intercept)
    assert np.array_equal(ref["lam"], r["lam"]) and np.array_equal(ref["niter"], r["niter"])
    assert r["beta"].shape == (1, 18, 6) and ref["beta"].tobytes() == np.ascontiguousarray(r["beta"][0]).tobytes()
    assert ref["std"].scaleY == r["std"].scaleY and ref["std"].meanY == r["meanYs"][0]


def test_common_scale_and_own_means():
    """Every response is centred by its own mean and all are divided by sqrt(sum_k ||y_k - mean_k||^2 / (n m)); without the
    intercept the same norm about the means, nothing centred."""
    x, Y = mo.synth_mt(60, 5, 3, seed=2)
    Yc = Y - Y.mean(axis=0)
    want = np.sqrt((Yc ** 2).sum() / Y.size)
    for standardize, intercept in ((True, True), (False, True), (True, False)):
        Xs, Ys, std, means = mo.standardise(x, Y, standardize, intercept)
        assert abs(float(std.scaleY) - want) <= 4e-7 * want
        if intercept:
            assert np.allclose(means, Y.mean(axis=0), rtol=1e-6) and np.allclose(Ys, Yc / want, atol=1e-5)
        else:
            assert not means.any() and np.allclose(Ys, Y / want, rtol=1e-5)
    Xs, Ys, std, means = mo.standardise(x, Y, False, False)
    assert std.scaleY == 1 and not means.any() and np.array_equal(Ys, Y.astype(np.float32))


def test_restatement_meets_the_lasso_kkt_bounds_and_keeps_rows_whole():
    """The restatement on (400, 70, 3), 10 lambdas down to 0.01, eps 1e-5, weights with a 0 and a 0.5: group KKT figures within the
    bounds tests/test_grplasso_host.py holds the group restatement to; a row enters or leaves for all responses at once; the
    unpenalised row is in the model at every lambda."""
    n, p, m = 400, 70, 3
    x, Y = mo.synth_mt(n, p, m, seed=n + p)
    w = np.ones(p)
    w[3], w[7] = 0.0, 0.5
    r = mo.mt_path(x, Y, w)
    viol, on, unp = go.group_kkt(r["K"], r["yv"], r["beta_std"], r["lam_int"], r["sizes"], w)
    over, on_max, unp_max = go.kkt_maxima(viol, on, unp, r["lam"])
    print(f"[mtlasso restatement (400, 70, 3) weighted] (viol-1)*ratio {over:.3e}  on*ratio {on_max:.3e}  unp {unp_max:.3e}  niter {r['niter'].tolist()}")
    assert r["niter"].max() <= 10000
    assert over < 2e-3 and on_max < 2e-3 and unp_max < 2e-3 and viol.max() < 1.3
    B = r["beta_std"].reshape(p, m, -1)
    rows = B != 0
    assert np.all(rows.all(axis=1) | ~rows.any(axis=1))
    assert np.all(rows[3].all(axis=0))
