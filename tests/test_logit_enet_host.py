"""CPU: elastic-net logistic regression (admm_hip_logit_enet) without a device -- the algebra of the penalty rows, the elastic net's
prox, the restatement of the augmented loop (tests/logit_enet_oracle.py) against a float64 reference optimum that asserts its own KKT
conditions, the symbols through every layer, what the C ABI refuses before it looks for a device, and the Python builders' argument
checks.

CELLS: (400, 8, seed 1), (2100, 40, seed 2) and (150, 200, seed 3, n < p) of logit_oracle.logit_data, alpha in {1, 0.5}, lambda =
f lambda_1 / alpha with f in {0.5, 0.1}; eps_abs = eps_rel = 1e-4, rho = 1, both intercept settings: 24 inputs.

Bound against the reference optimum: the measured worst relative excess of the penalised objective, f / f_opt - 1, of the RETURNED
coefficients (the penalty rows of the last z over sqrt(n), the intercept from get_x) on exactly these 24 inputs is 2.33e-5 (150 x 200,
alpha = 1, f = 0.1, with the intercept, 66 iterations: the one cell whose zero pattern differs from the optimum's, 79 non-zeros against
80); the next are 1.6e-7 (the same cell without the intercept) and 9.1e-8 (150 x 200, alpha = 0.5, f = 0.1), and every cell with n > p
is below 1e-8.  Ten times the worst is 2.3e-4; EXCESS_CAP is 1e-4, the power of ten next to it on the tight side, 4.3 times the measured
worst case -- tests/test_logit_ridge_host.py's rule (1.15e-5 -> 1e-4).  The dense read-out (get_x for every coefficient, no zeros) is
printed beside it: 6e-8 ... 2.1e-4 above the optimum on the same inputs.  The alpha = 0 cells against the ridge IRLS: at most 1.6e-9.
The zero pattern of the returned coefficients differs from the optimum's in at most ONE coefficient per cell: a condition, not a
measurement.  Iterations: 17 - 36 at n > p, 41 - 72 at n < p; the empty model at 1.25 lambda_max takes 34 - 43."""
import ctypes
import os
import re

import numpy as np
import pytest

import logit_multi_oracle as lm
import logit_oracle as lo
import logit_enet_oracle as le
import logit_ridge_oracle as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
OPTS = {"maxit": 10000, "eps_abs": 1e-4, "eps_rel": 1e-4, "rho": 1.0}
MEASURED_WORST = 2.33e-5          # 150 x 200, alpha = 1, f = 0.1, with the intercept (66 iterations); see the docstring
EXCESS_CAP = 1e-4                 # tests/test_gpu_logit_enet.py imports it
SUPPORT_SLACK = 1                 # zeros that may differ from the optimum's, per cell
SYMBOLS = ("admm_hip_logit_enet", "admm_hip_logit_enet_lambda_max", "admm_hip_logit_enet_state")
SHAPES = ((400, 8, 1), (2100, 40, 2), (150, 200, 3))
# (n, p, seed, alpha, f): lambda = f lambda_1 / alpha
CELLS = [(n, p, seed, alpha, f) for n, p, seed in SHAPES for alpha in (1.0, 0.5) for f in (0.5, 0.1)]
RIDGE_CELLS = [(n, p, seed, lam) for n, p, seed in SHAPES[:2] for lam in (1.0, 10.0)]

_cache = {}


def cell_data(n, p, seed, labels="data"):
    key = ("data", n, p, seed, labels)
    if key not in _cache:
        x, y = lo.logit_data(n, p, seed)
        if labels == "separable":
            y = lr.separable_labels(x, seed)
        assert 0.0 < y.mean() < 1.0
        _cache[key] = (x, y)
    return _cache[key]


def cell_lambda_one(n, p, seed, intercept, labels="data"):
    key = ("lambda1", n, p, seed, intercept, labels)
    if key not in _cache:
        x, y = cell_data(n, p, seed, labels)
        _cache[key] = float(le.lambda_one(x, y, intercept)[0])
    return _cache[key]


def cell_lambda(n, p, seed, alpha, f, intercept, labels="data"):
    return f * cell_lambda_one(n, p, seed, intercept, labels) / alpha


def cell_optimum(n, p, seed, lam, alpha, intercept, labels="data"):
    """-> (b0, b, optimum) of the reference on the cell's standardised design"""
    key = ("optimum", n, p, seed, lam, alpha, intercept, labels)
    if key not in _cache:
        x, y = cell_data(n, p, seed, labels)
        xs, _ = lr.standardized_design(x, intercept)
        _cache[key] = le.enet_optimum(xs, y, lam, alpha, intercept)
    return _cache[key]


def cell_restatement(n, p, seed, lam, alpha, intercept):
    """-> (returned beta, niter, the dense get_x read-out on the standardised scale)"""
    key = ("restated", n, p, seed, lam, alpha, intercept)
    if key not in _cache:
        x, y = cell_data(n, p, seed)
        d = {}
        got = le.logit_enet(x, y, lam, alpha, intercept, OPTS, [[d]])
        _cache[key] = (got["beta"][:, 0, 0], int(got["niter"][0, 0]), d["dense"])
    return _cache[key]


def support_differences(beta, b_opt):
    """zeros of the returned penalised coefficients that the optimum does not have, plus the other way round"""
    return int(np.sum((np.asarray(beta)[1:] == 0.0) != (np.asarray(b_opt) == 0.0)))


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
    assert len(lib.admm_hip_logit_enet.argtypes) == len(lib.admm_hip_logit_ridge.argtypes) + 1
    assert len(lib.admm_hip_logit_enet_state.argtypes) == len(lib.admm_hip_logit_ridge_state.argtypes) + 1
    assert len(lib.admm_hip_logit_enet_lambda_max.argtypes) == 8
    shim = open(os.path.join(ROOT, "integration", "admm_shim.cpp")).read()
    for name in SYMBOLS:
        assert "RcppExport SEXP admm_" + name[len("admm_hip_"):] + "(" in shim and name + "(" in shim


@pytest.mark.parametrize("intercept", [True, False])
def test_one_gram_matrix_serves_every_cell(intercept):
    """The augmented matrix does not depend on (lambda, alpha): its Gram matrix is X'X + n D, D = 1 on the user columns."""
    x, _ = lo.logit_data(60, 7, 4)
    A, _ = le.augmented(x, intercept)
    X, _ = lm.unfolded(x, intercept)
    assert A.shape == (60 + 7, 7 + int(intercept)) and np.array_equal(A[:60], X)
    assert np.array_equal(A[60:, :7], np.sqrt(60.0) * np.eye(7)) and not np.any(A[60:, 7:])
    D = np.zeros(A.shape[1])
    D[:7] = 1.0
    G, want = A.T @ A, X.T @ X + 60.0 * np.diag(D)
    assert np.max(np.abs(G - want)) <= 1e-13 * np.max(np.abs(want))


def test_the_enet_prox_is_the_minimiser():
    """z = soft(v, c_hi / rho) / (1 + c_lo / rho) minimises c_hi |z| + c_lo z^2 / 2 + rho / 2 (z - v)^2: not lower anywhere on a fine
    grid, exactly 0.0 inside the threshold, and the stationarity condition holds outside it."""
    rng = np.random.default_rng(12)
    for _ in range(200):
        rho = float(np.exp(rng.uniform(-5, 5)))
        c_hi, c_lo = float(np.exp(rng.uniform(-4, 2))), float(rng.choice([0.0, np.exp(rng.uniform(-4, 2))]))
        v = float(rng.standard_normal() * 6)
        z = float(le.enet_prox(np.array([v]), rho, c_hi, c_lo)[0])
        if abs(v) <= c_hi / rho:
            assert z == 0.0
        else:
            assert np.sign(z) == np.sign(v)
            assert abs(c_hi * np.sign(z) + c_lo * z + rho * (z - v)) <= 1e-13 * max(1.0, rho, c_hi) * max(1.0, abs(v))
        grid = np.linspace(-abs(v) - 1.0, abs(v) + 1.0, 20001)
        obj = lambda u: c_hi * np.abs(u) + 0.5 * c_lo * u * u + 0.5 * rho * (u - v) ** 2      # noqa: E731
        assert obj(z) <= obj(grid).min() + 1e-12 * (1.0 + obj(z))
    # alpha = 0 (c_hi = 0): the ridge rows' prox with lambda / c^2 in place of 1
    v = rng.standard_normal(50)
    assert np.allclose(le.enet_prox(v, 2.0, 0.0, 1.0), lr.square_prox(v, 2.0), rtol=1e-15, atol=0)


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("n,p,seed,alpha,f", CELLS)
def test_restatement_against_the_reference_optimum(n, p, seed, alpha, f, intercept):
    x, y = cell_data(n, p, seed)
    lam = cell_lambda(n, p, seed, alpha, f, intercept)
    beta, niter, dense = cell_restatement(n, p, seed, lam, alpha, intercept)
    assert niter <= OPTS["maxit"]
    _, b_opt, best = cell_optimum(n, p, seed, lam, alpha, intercept)
    fval = le.objective_of(x, y, beta, lam, alpha, intercept)
    excess = fval / best - 1.0
    xs, _ = lr.standardized_design(x, intercept)
    dense_excess = le.objective(xs, y, dense[p] if intercept else 0.0, dense[:p], lam, alpha) / best - 1.0
    diff = support_differences(beta, b_opt)
    print(f"[logit enet restatement n={n} p={p} alpha={alpha} f={f} icpt={int(intercept)}] niter {niter}, objective {fval:.9e} vs optimum {best:.9e} "
          f"(+{excess:.2e}; the dense read-out +{dense_excess:.2e}); support {int(np.sum(beta[1:] != 0.0))} vs {int(np.sum(b_opt != 0.0))}, {diff} differ")
    assert -1e-9 <= excess <= EXCESS_CAP
    assert diff <= SUPPORT_SLACK
    assert np.any(beta[1:] != 0.0)
    if alpha == 1.0:
        assert np.any(beta[1:] == 0.0)
    if not intercept:
        assert beta[0] == 0.0


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("n,p,seed", SHAPES)
def test_above_lambda_max_the_model_is_empty(n, p, seed, alpha, intercept):
    x, y = cell_data(n, p, seed)
    lam = cell_lambda(n, p, seed, alpha, 1.25, intercept)
    got = le.logit_enet(x, y, lam, alpha, intercept, OPTS)
    beta, niter = got["beta"][:, 0, 0], int(got["niter"][0, 0])
    print(f"[logit enet empty n={n} p={p} alpha={alpha} icpt={int(intercept)}] niter {niter}, intercept {beta[0]:.6f}")
    assert niter <= OPTS["maxit"]
    assert np.all(beta[1:] == 0.0) and np.isfinite(beta[0])


def test_lambda_one_is_where_the_optimum_empties():
    """Just below lambda_1 / alpha the KKT conditions at b = 0 fail, at it they hold: lambda_one is the gradient's largest entry there."""
    for n, p, seed in SHAPES[:2]:
        x, y = cell_data(n, p, seed)
        for intercept in (True, False):
            xs, _ = lr.standardized_design(x, intercept)
            l1 = cell_lambda_one(n, p, seed, intercept)
            b0 = np.log(y.mean() / (1.0 - y.mean())) if intercept else 0.0
            g = xs.T @ (y - 1.0 / (1.0 + np.exp(-b0)))                # minus the likelihood's gradient at (b0, 0)
            assert abs(np.max(np.abs(g)) - l1) <= 1e-9 * l1


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("n,p,seed,lam", RIDGE_CELLS)
def test_alpha_zero_is_the_ridge_problem_on_the_shared_inverse(n, p, seed, lam, intercept):
    x, y = cell_data(n, p, seed)
    beta, niter, _ = cell_restatement(n, p, seed, lam, 0.0, intercept)
    xs, _ = lr.standardized_design(x, intercept)
    best = lr.ridge_irls(xs, y, lam, intercept)[2]
    excess = lr.objective_of(x, y, beta, lam, intercept) / best - 1.0
    print(f"[logit enet alpha=0 n={n} p={p} lambda={lam} icpt={int(intercept)}] niter {niter}, objective +{excess:.2e} over the ridge IRLS")
    assert niter <= OPTS["maxit"]
    assert -1e-9 <= excess <= EXCESS_CAP
    assert le.objective_of(x, y, beta, lam, 0.0, intercept) == pytest.approx(lr.objective_of(x, y, beta, lam, intercept), rel=1e-14)


def test_k_columns_and_a_grid_equal_the_single_fits():
    x, _ = lo.logit_data(400, 8, 1)
    Y = lm.label_matrix(x, 1)[:, :3]
    lam, alpha = (6.0, 20.0), (1.0, 0.5)
    both = le.logit_enet(x, Y, lam, alpha, True, OPTS)
    assert both["beta"].shape == (9, 3, 2) and both["niter"].shape == (3, 2)
    for l in range(2):
        for c in range(3):
            one = le.logit_enet(x, Y[:, c], lam[l], alpha[l], True, OPTS)
            assert one["niter"][0, 0] == both["niter"][c, l] and np.array_equal(one["beta"][:, 0, 0], both["beta"][:, c, l])


def _call(lib, **over):
    from admm_amd._lib import AdmmOpts
    keep = dict(x=np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), y=np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0]),
                lam=np.array([1.0, 0.5]), alpha=np.array([1.0, 0.5]), beta=np.full(3 * 2 * 2, 7.0), niter=np.full(4, -5, np.int32))
    for name in ("y", "lam", "alpha"):
        if name + "_values" in over:
            keep[name] = np.asarray(over.pop(name + "_values"), dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    v = dict(x=keep["x"].ctypes.data, y=keep["y"].ctypes.data, n=6, p=2, k=2, mem=0, intercept=1, lam=keep["lam"].ctypes.data_as(dp),
             alpha=keep["alpha"].ctypes.data_as(dp), ncell=2, opts=(10, 1e-4, 1e-4, 1.0), beta=keep["beta"].ctypes.data_as(dp),
             niter=keep["niter"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    v.update(over)
    o = AdmmOpts(*v["opts"]) if v["opts"] is not None else None
    rc = lib.admm_hip_logit_enet(v["x"], v["y"], v["n"], v["p"], v["k"], v["mem"], v["intercept"], v["lam"], v["alpha"], v["ncell"],
                                 ctypes.byref(o) if o is not None else None, v["beta"], v["niter"], None)
    if rc == INVALID_ARG:                                      # a refused call touches no output
        assert np.all(keep["beta"] == 7.0) and np.all(keep["niter"] == -5)
    return rc, lib.admm_hip_last_error().decode()


NULL_MSG = "lambda and alpha must not be NULL"
LAMBDA_MSG = "every lambda must be finite and positive"
ALPHA_MSG = "every alpha must lie in [0, 1]"
GOOD_Y = [0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 1, 0]
REFUSALS = [
    (dict(lam_values=[1.0, 0.0]), LAMBDA_MSG),
    (dict(lam_values=[-1.0, 1.0]), LAMBDA_MSG),
    (dict(lam_values=[1.0, float("nan")]), LAMBDA_MSG),
    (dict(lam_values=[float("inf"), 1.0]), LAMBDA_MSG),
    (dict(alpha_values=[1.0, -0.1]), ALPHA_MSG),
    (dict(alpha_values=[1.5, 0.5]), ALPHA_MSG),
    (dict(alpha_values=[1.0, float("nan")]), ALPHA_MSG),
    (dict(ncell=0), "lambda must have at least one value"),
    (dict(lam=None), NULL_MSG),
    (dict(alpha=None), NULL_MSG),
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


def test_lambda_max_and_the_state_form_refuse_before_any_device_is_touched():
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    # n = 2 rows against p = 2 columns and the intercept: passes every check (and then the call looks for a device)
    assert _call(lib, n=2, k=1, y_values=[0, 1])[0] != INVALID_ARG
    x, y = np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    out = np.full(1, 7.0)

    def lmax(xp, yp, n, k, outp):
        rc = lib.admm_hip_logit_enet_lambda_max(xp, yp, n, 2, k, 0, 1, outp)
        assert out[0] == 7.0
        return rc, lib.admm_hip_last_error().decode()

    assert lmax(x.ctypes.data, y.ctypes.data, 6, 0, out.ctypes.data_as(dp)) == (INVALID_ARG, "y must have at least one column")
    assert lmax(None, y.ctypes.data, 6, 1, out.ctypes.data_as(dp)) == (INVALID_ARG, "x and y must not be NULL")
    assert lmax(x.ctypes.data, y.ctypes.data, 6, 1, None) == (INVALID_ARG, "output pointers must not be NULL")
    assert lmax(x.ctypes.data, y.ctypes.data, 1, 1, out.ctypes.data_as(dp)) == (INVALID_ARG, "nrow(x) must be at least 2")
    half = np.array([0.0, 1.0, 0.5, 0.0, 1.0, 0.0])
    assert lmax(x.ctypes.data, half.ctypes.data, 6, 1, out.ctypes.data_as(dp)) == (INVALID_ARG, "column 0 of y: every label must be exactly 0 or 1")
    assert lmax(x.ctypes.data, np.ones(6).ctypes.data, 6, 1, out.ctypes.data_as(dp)) == (INVALID_ARG, "column 0 of y must hold both classes")
    beta, niter, o = np.zeros(3), np.zeros(1, np.int32), AdmmOpts(10, 1e-4, 1e-4, 1.0)
    st, nst = np.zeros(5 * 8 * 2), ctypes.c_longlong()
    rc = lib.admm_hip_logit_enet_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, 1.0, 1.0, ctypes.byref(o), beta.ctypes.data_as(dp), niter.ctypes.data_as(ip),
                                       None, None, 0, None, st.ctypes.data_as(dp), 2, ctypes.byref(nst))
    assert (rc, lib.admm_hip_last_error().decode()) == (INVALID_ARG, "bad state arguments (the iterate dump needs the trace)")
    rc = lib.admm_hip_logit_enet_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, 0.0, 1.0, ctypes.byref(o), beta.ctypes.data_as(dp), niter.ctypes.data_as(ip),
                                       None, None, 0, None, None, 0, None)
    assert (rc, lib.admm_hip_last_error().decode()) == (INVALID_ARG, LAMBDA_MSG)
    rc = lib.admm_hip_logit_enet_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, 1.0, 1.5, ctypes.byref(o), beta.ctypes.data_as(dp), niter.ctypes.data_as(ip),
                                       None, None, 0, None, None, 0, None)
    assert (rc, lib.admm_hip_last_error().decode()) == (INVALID_ARG, ALPHA_MSG)


def test_python_builder_argument_checks():
    from admm_amd import ADMM_LogitEnet, ADMM_LogitEnetOvR, admm_logit_enet, admm_logit_enet_ovr
    from admm_amd.api import ADMM_LogitEnet_fit
    rng = np.random.default_rng(3)
    x = rng.standard_normal((30, 40))                                # n < p is accepted
    Y = (rng.uniform(size=(30, 3)) < 0.4).astype(np.float64)
    m = admm_logit_enet(x, Y, [10.0, 0.1, 1.0], alpha=[1.0, 0.5, 0.0])
    assert isinstance(m, ADMM_LogitEnet) and m.intercept is True and (m.n, m.p, m.k) == (30, 40, 3)
    assert m.lam.tolist() == [10.0, 0.1, 1.0] and m.alpha.tolist() == [1.0, 0.5, 0.0]      # pairs, in the order given
    assert (m.maxit, m.eps_abs, m.eps_rel, m.rho) == (10000, 1e-4, 1e-4, 1.0)
    assert m.opts(maxit=7, rho=2.0).maxit == 7 and m.rho == 2.0
    one = admm_logit_enet(x, Y[:, 0], 2.0)
    assert one.k == 1 and one.lam.tolist() == [2.0] and one.alpha.tolist() == [1.0]
    assert admm_logit_enet(x, Y, [2.0, 3.0], alpha=0.25).alpha.tolist() == [0.25, 0.25]      # one alpha for every lambda
    auto = admm_logit_enet(x, Y, alpha=0.5)
    assert auto.lam is None and auto.nlambda == 100 and auto.lambda_min_ratio == 0.01 and auto.alpha.tolist() == [0.5] * 100
    assert admm_logit_enet(x[:, :5], Y, nlambda=7).lambda_min_ratio == 0.0001
    for bad in (0.0, -1.0, np.nan, np.inf, [1.0, 0.0]):
        with pytest.raises(ValueError, match="finite and positive"):
            admm_logit_enet(x, Y, bad)
    for bad in (-0.1, 1.5, np.nan, [1.0, 2.0]):
        with pytest.raises(ValueError, match="every alpha must lie in \\[0, 1\\]"):
            admm_logit_enet(x, Y, [1.0, 2.0], alpha=bad)
    with pytest.raises(ValueError, match="as long as lam"):
        admm_logit_enet(x, Y, [1.0, 2.0], alpha=[1.0, 0.5, 0.2])
    with pytest.raises(ValueError, match="at least one value"):
        admm_logit_enet(x, Y, [])
    with pytest.raises(ValueError, match="alpha = 0 has no lambda_max"):
        admm_logit_enet(x, Y, alpha=0.0)
    with pytest.raises(ValueError, match="needs one alpha"):
        admm_logit_enet(x, Y, alpha=[1.0, 0.5])
    Yb = Y.copy()
    Yb[3, 2] = 0.5
    with pytest.raises(ValueError, match="column 2 of y: every label must be exactly 0 or 1"):
        admm_logit_enet(x, Yb, 1.0)
    Yb = Y.copy()
    Yb[:, 1] = 1.0
    with pytest.raises(ValueError, match="column 1 of y must hold both classes"):
        admm_logit_enet(x, Yb, 1.0)
    with pytest.raises(ValueError, match="nrow\\(x\\) should be equal to nrow\\(Y\\)"):
        admm_logit_enet(x, Y[:-1], 1.0)
    with pytest.raises(ValueError, match="single label column and a single cell"):
        admm_logit_enet(x, Y, 1.0).fit(trace=True)
    with pytest.raises(ValueError, match="single label column and a single cell"):
        admm_logit_enet(x, Y[:, 0], [1.0, 2.0]).fit(trace=True)
    labels = np.where(Y[:, 0] == 1.0, 5, np.where(Y[:, 1] == 1.0, 11, -3))
    o = admm_logit_enet_ovr(x, labels, 1.0, alpha=0.5)
    assert isinstance(o, ADMM_LogitEnetOvR) and o.classes.tolist() == [-3, 5, 11] and o.k == 3 and o.alpha.tolist() == [0.5]
    assert np.array_equal(o.y, (labels[:, None] == o.classes[None, :]).astype(np.float64))
    with pytest.raises(ValueError, match="at least two classes"):
        admm_logit_enet_ovr(x, np.zeros(30, dtype=int), 1.0)
    assert "elastic-net" in repr(ADMM_LogitEnet_fit(np.ones(1), np.ones(1), np.zeros((3, 2, 1)), np.zeros((2, 1)), {}))
