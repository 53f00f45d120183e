"""CPU: ridge logistic regression (admm_hip_logit_ridge) without a device -- the algebra of the ridge rows, the square loss's prox, the
restatement of the augmented loop (tests/logit_ridge_oracle.py) against a float64 ridge Newton optimum, the symbols through every
layer, what the C ABI refuses before it looks for a device, and the Python builders' argument checks.

Bound against the ridge IRLS optimum (eps_abs = eps_rel = 1e-4, rho = 1, both intercept settings; CELLS below: (400, 8, seed 1) and
(2100, 40, seed 2) with logit_data's labels at lambda 0.1, 1, 10, 100 and with separable labels at lambda 1; (150, 200, seed 3), n < p,
at lambda 1 and 10): the measured worst relative excess of the penalised objective, f / f_IRLS - 1, on exactly these 24 inputs is
1.15e-5 (2100 x 40, separable labels, lambda = 1: 1.149e-5 without the intercept, 1.143e-5 with it, 86 iterations; 400 x 8 separable:
3.5e-6; 150 x 200: 1.3e-6; every cell with logit_data's labels at n > p is below 4e-8).  Ten times that is 1.15e-4.  EXCESS_CAP is 1e-4:
the power of ten next to it and the figure the feature's specification names -- the tighter reading of "ten times the worst case,
as a power of ten" (tests/test_logit_host.py's rule), 8.7 times the measured worst case.  Iterations: 12 - 17 with logit_data's labels
at n > p, 32 - 68 at n < p, 66 - 86 with separable labels."""
import ctypes
import os
import re

import numpy as np
import pytest

import logit_multi_oracle as lm
import logit_oracle as lo
import logit_ridge_oracle as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
OPTS = {"maxit": 10000, "eps_abs": 1e-4, "eps_rel": 1e-4, "rho": 1.0}
MEASURED_WORST = 1.15e-5          # see the docstring
EXCESS_CAP = 1e-4                # tests/test_gpu_logit_ridge.py imports it
SYMBOLS = ("admm_hip_logit_ridge", "admm_hip_logit_ridge_state")
LAMBDAS = (0.1, 1.0, 10.0, 100.0)
# (n, p, seed, labels, lambda)
CELLS = ([(n, p, seed, "data", lam) for n, p, seed in ((400, 8, 1), (2100, 40, 2)) for lam in LAMBDAS]
         + [(400, 8, 1, "separable", 1.0), (2100, 40, 2, "separable", 1.0), (150, 200, 3, "data", 1.0), (150, 200, 3, "data", 10.0)])

_cache = {}


def cell_data(n, p, seed, labels):
    key = ("data", n, p, seed, labels)
    if key not in _cache:
        x, y = lo.logit_data(n, p, seed)
        if labels == "separable":
            y = lr.separable_labels(x, seed)
        assert 0.0 < y.mean() < 1.0
        _cache[key] = (x, y)
    return _cache[key]


def cell_irls(n, p, seed, labels, lam, intercept):
    """-> (b0, b, optimum) of the ridge Newton on the cell's standardised design"""
    key = ("irls", n, p, seed, labels, lam, intercept)
    if key not in _cache:
        x, y = cell_data(n, p, seed, labels)
        xs, _ = lr.standardized_design(x, intercept)
        _cache[key] = lr.ridge_irls(xs, y, lam, intercept)[:3]
    return _cache[key]


def cell_restatement(n, p, seed, labels, lam, intercept):
    key = ("restated", n, p, seed, labels, lam, intercept)
    if key not in _cache:
        x, y = cell_data(n, p, seed, labels)
        got = lr.logit_ridge(x, y, lam, intercept, OPTS)
        _cache[key] = (got["beta"][:, 0, 0], int(got["niter"][0, 0]))
    return _cache[key]


def test_symbols_are_declared_exported_bound_and_documented():
    from admm_amd import _lib
    header = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"ADMM_HIP_API int " + name + r"\(", header), name
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
        assert "`" + name + "`" in doc, name
    assert len(lib.admm_hip_logit_ridge.argtypes) == len(lib.admm_hip_logit_multi.argtypes) + 2
    assert len(lib.admm_hip_logit_ridge_state.argtypes) == len(lib.admm_hip_logit_state.argtypes) + 1
    shim = open(os.path.join(ROOT, "integration", "admm_shim.cpp")).read()
    assert "RcppExport SEXP admm_logit_ridge(" in shim and "admm_hip_logit_ridge(" in shim


@pytest.mark.parametrize("intercept", [True, False])
def test_the_gram_matrix_of_the_augmented_rows_is_the_ridge_shifted_one(intercept):
    x, _ = lo.logit_data(60, 7, 4)
    for lam in (0.1, 3.0, 100.0):
        A, _ = lr.augmented(x, lam, intercept)
        X, _ = lm.unfolded(x, intercept)
        assert A.shape == (60 + 7, 7 + int(intercept)) and np.array_equal(A[:60], X)
        D = np.zeros(A.shape[1])
        D[:7] = 1.0                                                # the intercept's entry is not shifted
        G, want = A.T @ A, X.T @ X + lam * np.diag(D)
        assert np.max(np.abs(G - want)) <= 1e-13 * np.max(np.abs(want))
        if intercept:
            assert G[7, 7] == (X.T @ X)[7, 7] == 60.0 and not np.any(A[60:, 7])


def test_the_square_prox_is_the_minimiser():
    """z = v rho / (1 + rho) minimises z^2 / 2 + rho / 2 (z - v)^2: the derivative z + rho (z - v) vanishes there and the objective is not
    lower anywhere on a fine grid."""
    rng = np.random.default_rng(12)
    for _ in range(200):
        rho = float(np.exp(rng.uniform(-5, 5)))
        v = float(rng.standard_normal() * 6)
        z = float(lr.square_prox(np.array([v]), rho)[0])
        assert abs(z + rho * (z - v)) <= 1e-14 * max(1.0, rho) * max(1.0, abs(v))
        grid = np.linspace(-abs(v) - 1.0, abs(v) + 1.0, 20001)
        obj = lambda u: 0.5 * u * u + 0.5 * rho * (u - v) ** 2      # noqa: E731
        assert obj(z) <= obj(grid).min() + 1e-12 * (1.0 + obj(z))


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("n,p,seed,labels,lam", CELLS)
def test_restatement_against_the_ridge_irls_optimum(n, p, seed, labels, lam, intercept):
    x, y = cell_data(n, p, seed, labels)
    beta, niter = cell_restatement(n, p, seed, labels, lam, intercept)
    assert niter <= OPTS["maxit"]
    _, _, best = cell_irls(n, p, seed, labels, lam, intercept)
    f = lr.objective_of(x, y, beta, lam, intercept)
    excess = f / best - 1.0
    print(f"[logit ridge restatement n={n} p={p} {labels} lambda={lam} icpt={int(intercept)}] niter {niter}, objective {f:.9e} vs IRLS {best:.9e} (+{excess:.2e})")
    assert -1e-9 <= excess <= EXCESS_CAP
    if not intercept:
        assert beta[0] == 0.0


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("n,p,seed", [(400, 8, 1), (2100, 40, 2)])
def test_the_coefficient_norm_does_not_grow_with_lambda(n, p, seed, intercept):
    """|b(lambda)|_2 over the user columns is non-increasing in lambda at the optimum: asserted on the ridge IRLS exactly, on the
    restatement with the slack of its measured distance |b - b*| (printed)."""
    x, y = cell_data(n, p, seed, "data")
    _, std = lr.standardized_design(x, intercept)
    star, got, dist = [], [], []
    for lam in LAMBDAS:
        _, b, _ = cell_irls(n, p, seed, "data", lam, intercept)
        _, br = lr.to_std(std, cell_restatement(n, p, seed, "data", lam, intercept)[0], intercept)
        star.append(float(np.linalg.norm(b)))
        got.append(float(np.linalg.norm(br)))
        dist.append(float(np.linalg.norm(br - b)))
    print(f"[logit ridge norms n={n} p={p} icpt={int(intercept)}] IRLS {star}, restatement {got}, |b - b*| {dist}")
    assert all(star[i + 1] < star[i] for i in range(len(LAMBDAS) - 1))
    assert all(got[i + 1] <= got[i] + dist[i] + dist[i + 1] for i in range(len(LAMBDAS) - 1))


def test_k_columns_and_a_grid_equal_the_single_fits():
    x, _ = lo.logit_data(400, 8, 1)
    Y = lm.label_matrix(x, 1)[:, :3]
    lam = (10.0, 0.1)
    both = lr.logit_ridge(x, Y, lam, True, OPTS)
    assert both["beta"].shape == (9, 3, 2) and both["niter"].shape == (3, 2)
    for l, lv in enumerate(lam):
        for c in range(3):
            one = lr.logit_ridge(x, Y[:, c], lv, True, OPTS)
            assert one["niter"][0, 0] == both["niter"][c, l] and np.array_equal(one["beta"][:, 0, 0], both["beta"][:, c, l])


def _call(lib, **over):
    from admm_amd._lib import AdmmOpts
    keep = dict(x=np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), y=np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0]),
                lam=np.array([1.0, 0.5]), beta=np.full(3 * 2 * 2, 7.0), niter=np.full(4, -5, np.int32))
    if "y_values" in over:
        keep["y"] = np.asarray(over.pop("y_values"), dtype=np.float64)
    if "lam_values" in over:
        keep["lam"] = np.asarray(over.pop("lam_values"), dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    v = dict(x=keep["x"].ctypes.data, y=keep["y"].ctypes.data, n=6, p=2, k=2, mem=0, intercept=1, lam=keep["lam"].ctypes.data_as(dp), nlam=2,
             opts=(10, 1e-4, 1e-4, 1.0), beta=keep["beta"].ctypes.data_as(dp), niter=keep["niter"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    v.update(over)
    o = AdmmOpts(*v["opts"]) if v["opts"] is not None else None
    rc = lib.admm_hip_logit_ridge(v["x"], v["y"], v["n"], v["p"], v["k"], v["mem"], v["intercept"], v["lam"], v["nlam"],
                                  ctypes.byref(o) if o is not None else None, v["beta"], v["niter"], None)
    if rc == INVALID_ARG:                                      # a refused call touches no output
        assert np.all(keep["beta"] == 7.0) and np.all(keep["niter"] == -5)
    return rc, lib.admm_hip_last_error().decode()


LAMBDA_MSG = "every lambda must be finite and positive (lambda = 0 is admm_hip_logit_multi)"
GOOD_Y = [0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 1, 0]
REFUSALS = [
    (dict(lam_values=[1.0, 0.0]), LAMBDA_MSG),
    (dict(lam_values=[-1.0, 1.0]), LAMBDA_MSG),
    (dict(lam_values=[1.0, float("nan")]), LAMBDA_MSG),
    (dict(lam_values=[float("inf"), 1.0]), LAMBDA_MSG),
    (dict(nlam=0), "lambda must have at least one value"),
    (dict(lam=None), "lambda must not be NULL"),
    (dict(k=0), "y must have at least one column"),
    (dict(y_values=GOOD_Y[:6] + [0, 1, 0.5, 0, 1, 0]), "column 1 of y: every label must be exactly 0 or 1"),
    (dict(y_values=[0, 1, float("nan"), 0, 1, 0] + GOOD_Y[6:]), "column 0 of y: every label must be exactly 0 or 1"),
    (dict(y_values=GOOD_Y[:6] + [1.0] * 6), "column 1 of y must hold both classes"),
    (dict(y_values=[0.0] * 6 + GOOD_Y[6:]), "column 0 of y must hold both classes"),
    (dict(n=1), "nrow(x) must be at least 2"),
    (dict(x=None), "x and y must not be NULL"),
    (dict(n=0), "n and p must be positive"),
    (dict(mem=7), "mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE"),
    (dict(opts=None), "opts must not be NULL"),
    (dict(opts=(0, 1e-4, 1e-4, 1.0)), "maxit should be positive"),
    (dict(opts=(10, 1e-4, 1e-4, 0.0)), "rho should be positive"),
    (dict(beta=None), "output pointers must not be NULL"),
    (dict(niter=None), "output pointers must not be NULL"),
]


@pytest.mark.parametrize("over,message", REFUSALS, ids=[f"{k}-" + m[:24] + "/" + ",".join(o) for k, (o, m) in enumerate(REFUSALS)])
def test_bad_calls_are_refused_before_any_device_is_touched(over, message):
    from admm_amd import _lib
    lib = _lib.load()
    assert _call(lib, **dict(over)) == (INVALID_ARG, message)


def test_there_is_no_shape_condition_and_the_state_form_refuses_like_lad_state():
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    # n = 2 rows against p = 2 columns and the intercept: passes every check (and then the call looks for a device)
    assert _call(lib, n=2, k=1, y_values=[0, 1])[0] != INVALID_ARG
    x, y = np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    beta, niter, o = np.zeros(3), np.zeros(1, np.int32), AdmmOpts(10, 1e-4, 1e-4, 1.0)
    st, nst = np.zeros(5 * 8 * 2), ctypes.c_longlong()
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.admm_hip_logit_ridge_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, 1.0, ctypes.byref(o), beta.ctypes.data_as(dp),
                                        niter.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None, 0, None, st.ctypes.data_as(dp), 2, ctypes.byref(nst))
    assert (rc, lib.admm_hip_last_error().decode()) == (INVALID_ARG, "bad state arguments (the iterate dump needs the trace)")
    rc = lib.admm_hip_logit_ridge_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, 0.0, ctypes.byref(o), beta.ctypes.data_as(dp),
                                        niter.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None, 0, None, None, 0, None)
    assert (rc, lib.admm_hip_last_error().decode()) == (INVALID_ARG, LAMBDA_MSG)


def test_python_builder_argument_checks():
    from admm_amd import ADMM_LogitRidge, ADMM_LogitRidgeOvR, admm_logit_ridge, admm_logit_ridge_ovr
    from admm_amd.api import ADMM_LogitRidge_fit
    rng = np.random.default_rng(3)
    x = rng.standard_normal((30, 40))                                # n < p is accepted
    Y = (rng.uniform(size=(30, 3)) < 0.4).astype(np.float64)
    m = admm_logit_ridge(x, Y, [10.0, 0.1, 1.0])
    assert isinstance(m, ADMM_LogitRidge) and m.intercept is True and (m.n, m.p, m.k) == (30, 40, 3)
    assert m.lam.tolist() == [10.0, 0.1, 1.0]                        # in the order given
    assert (m.maxit, m.eps_abs, m.eps_rel, m.rho) == (10000, 1e-4, 1e-4, 1.0)
    assert m.opts(maxit=7, rho=2.0).maxit == 7 and m.rho == 2.0
    assert admm_logit_ridge(x, Y[:, 0], 2.0).k == 1 and admm_logit_ridge(x, Y[:, 0], 2.0).lam.tolist() == [2.0]
    for bad in (0.0, -1.0, np.nan, np.inf, [1.0, 0.0]):
        with pytest.raises(ValueError, match="finite and positive"):
            admm_logit_ridge(x, Y, bad)
    with pytest.raises(ValueError, match="at least one value"):
        admm_logit_ridge(x, Y, [])
    Yb = Y.copy()
    Yb[3, 2] = 0.5
    with pytest.raises(ValueError, match="column 2 of y: every label must be exactly 0 or 1"):
        admm_logit_ridge(x, Yb, 1.0)
    Yb = Y.copy()
    Yb[:, 1] = 1.0
    with pytest.raises(ValueError, match="column 1 of y must hold both classes"):
        admm_logit_ridge(x, Yb, 1.0)
    with pytest.raises(ValueError, match="nrow\\(x\\) should be equal to nrow\\(Y\\)"):
        admm_logit_ridge(x, Y[:-1], 1.0)
    with pytest.raises(ValueError, match="single label column and a single lambda"):
        admm_logit_ridge(x, Y, 1.0).fit(trace=True)
    with pytest.raises(ValueError, match="single label column and a single lambda"):
        admm_logit_ridge(x, Y[:, 0], [1.0, 2.0]).fit(trace=True)
    labels = np.where(Y[:, 0] == 1.0, 5, np.where(Y[:, 1] == 1.0, 11, -3))
    o = admm_logit_ridge_ovr(x, labels, 1.0)
    assert isinstance(o, ADMM_LogitRidgeOvR) and o.classes.tolist() == [-3, 5, 11] and o.k == 3
    assert np.array_equal(o.y, (labels[:, None] == o.classes[None, :]).astype(np.float64))
    with pytest.raises(ValueError, match="at least two classes"):
        admm_logit_ridge_ovr(x, np.zeros(30, dtype=int), 1.0)
    assert "ridge" in repr(ADMM_LogitRidge_fit(np.ones(1), np.zeros((3, 2, 1)), np.zeros((2, 1)), {}))
