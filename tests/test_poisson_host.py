"""CPU: Poisson regression with the elastic-net penalty (admm_hip_poisson) without a device -- the NumPy statement of the Newton prox
against bisection and against its equation, the restatement of the augmented loop (tests/poisson_oracle.py) against a float64 reference
optimum that asserts its own KKT conditions, the symbols through every layer, what the C ABI refuses before it looks for a device, and
the Python builder's argument checks.

Data: poisson_oracle.poisson_data -- x = N(0, 1), y = Poisson(exp(b0 + 0.5 x_0 - 0.4 x_1 + 0.3 x_2)), b0 = 0.7 unless said.
CELLS: (400, 8, seed 1), (2100, 40, seed 2) and (150, 200, seed 3, n < p), alpha in {1, 0.5}, lambda = f lambda_1 / alpha with f in
{0.5, 0.1}; a lambda = 0 cell on the two tall shapes; the b0 = 4.0 (mean count 68) and b0 = -2.0 (mean 0.18, 83 % zeros) responses on
(400, 8, 1) at the same four (alpha, f); eps_abs = eps_rel = 1e-4, rho = 1, both intercept settings: 44 inputs.

EXCESS = (objective - optimum) / (objective of the empty model - optimum): the Poisson objective can be negative or near zero, so a
ratio to the optimum itself is not usable.  The measured worst EXCESS of the RETURNED coefficients (the penalty rows of the last z over
sqrt(n), the intercept from get_x) on exactly these 44 inputs is 1.57e-6 (400 x 8, b0 = 4, alpha = 0.5, f = 0.5, with the intercept,
37 iterations); the next are 1.22e-6 and 9.2e-7 (b0 = -2 with the intercept), and every b0 = 0.7 cell is at or below 4.8e-7.
EXCESS_CAP is ten times the worst, 1.57e-5 (below the sibling tests' 1e-4).  The zero pattern of the returned coefficients equals the
optimum's at every one of the 44 inputs; SUPPORT_SLACK = 1 is the sibling tests' condition, not a measurement.  Iterations: 30 - 55 at
b0 = 0.7, 37 - 118 at b0 = 4, 11 - 26 at b0 = -2."""
import ctypes
import os
import re

import numpy as np
import pytest

import logit_enet_oracle as le
import logit_ridge_oracle as lr
import poisson_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
OPTS = {"maxit": 10000, "eps_abs": 1e-4, "eps_rel": 1e-4, "rho": 1.0}
MEASURED_WORST = 1.57e-6          # 400 x 8, b0 = 4, alpha = 0.5, f = 0.5, with the intercept (37 iterations); see the docstring
EXCESS_CAP = 10 * MEASURED_WORST  # tests/test_gpu_poisson.py imports it
assert EXCESS_CAP <= 1e-4
SUPPORT_SLACK = 1                 # zeros that may differ from the optimum's, per cell
SYMBOLS = ("admm_hip_poisson", "admm_hip_poisson_lambda_max", "admm_hip_poisson_state")
SHAPES = ((400, 8, 1), (2100, 40, 2), (150, 200, 3))
# (n, p, seed, b0, alpha, f): lambda = f lambda_1 / alpha
CELLS = ([(n, p, seed, 0.7, alpha, f) for n, p, seed in SHAPES for alpha in (1.0, 0.5) for f in (0.5, 0.1)]
         + [(n, p, seed, 0.7, 1.0, 0.0) for n, p, seed in SHAPES[:2]]
         + [(400, 8, 1, b0, alpha, f) for b0 in (4.0, -2.0) for alpha in (1.0, 0.5) for f in (0.5, 0.1)])
# the prox's inputs (the device hook is tested on the same set, tests/test_gpu_poisson.py)
PROX_T = (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3, 1e6, 1e12)
PROX_Y = (0.0, 1.0, 3.0, 1e4)
PROX_V = np.concatenate([np.linspace(-60.0, 60.0, 4001), [745.0, -745.0, 800.0, -800.0, 1e4, -1e4, 0.0, 1e-300, -1e-300]])

_cache = {}


def prox_inputs(t):
    """-> (v, y): PROX_V x PROX_Y, and for every y the v that put w = v + t y just below and just above t"""
    v = np.concatenate([PROX_V for _ in PROX_Y] + [np.array([t * (1.0 - y) * (1.0 - 1e-12) - 1e-15 * t, t * (1.0 - y) * (1.0 + 1e-12) + 1e-15 * t]) for y in PROX_Y])
    y = np.concatenate([np.full(PROX_V.size, y) for y in PROX_Y] + [np.full(2, y) for y in PROX_Y])
    return v, y


def cell_data(n, p, seed, b0=0.7):
    key = ("data", n, p, seed, b0)
    if key not in _cache:
        _cache[key] = po.poisson_data(n, p, seed, b0)
    return _cache[key]


def cell_lambda_one(n, p, seed, intercept, b0=0.7):
    key = ("lambda1", n, p, seed, intercept, b0)
    if key not in _cache:
        x, y = cell_data(n, p, seed, b0)
        _cache[key] = float(po.lambda_one(x, y, intercept)[0])
    return _cache[key]


def cell_lambda(n, p, seed, alpha, f, intercept, b0=0.7):
    return f * cell_lambda_one(n, p, seed, intercept, b0) / alpha


def cell_optimum(n, p, seed, lam, alpha, intercept, b0=0.7):
    """-> (b0, b, optimum) of the reference on the cell's standardised design"""
    key = ("optimum", n, p, seed, lam, alpha, intercept, b0)
    if key not in _cache:
        x, y = cell_data(n, p, seed, b0)
        xs, _ = lr.standardized_design(x, intercept)
        _cache[key] = po.poisson_optimum(xs, y, lam, alpha, intercept)
    return _cache[key]


def excess_of(x, y, beta, lam, alpha, intercept, best):
    """EXCESS of caller-scale coefficients (see the docstring)"""
    return (po.objective_of(x, y, beta, lam, alpha, intercept) - best) / (po.null_objective(y, intercept) - best)


def support_differences(beta, b_opt):
    """zeros of the returned penalised coefficients that the optimum does not have, plus the other way round"""
    return int(np.sum((np.asarray(beta)[1:] == 0.0) != (np.asarray(b_opt) == 0.0)))


def test_symbols_are_declared_exported_bound_and_documented():
    from admm_amd import _lib
    header = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in SYMBOLS + ("admm_hip_test_poisson_prox",):
        assert re.search(r"ADMM_HIP_API int " + name + r"\(", header), name
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
    for name in SYMBOLS:
        assert "`" + name + "`" in doc, name
    assert len(lib.admm_hip_poisson.argtypes) == len(lib.admm_hip_logit_enet.argtypes)
    assert len(lib.admm_hip_poisson_state.argtypes) == len(lib.admm_hip_logit_enet_state.argtypes)
    assert len(lib.admm_hip_poisson_lambda_max.argtypes) == 8 and len(lib.admm_hip_test_poisson_prox.argtypes) == 5
    shim = open(os.path.join(ROOT, "integration", "admm_shim.cpp")).read()
    for name in SYMBOLS:
        assert "RcppExport SEXP admm_" + name[len("admm_hip_"):] + "(" in shim and name + "(" in shim
    assert "Not offered: an exposure offset" in header


@pytest.mark.parametrize("t", PROX_T)
def test_prox_solves_its_equation(t):
    """Against bisection to a closed bracket, and against the equation itself: |h(z)| / h'(z), the Newton estimate of the distance to the
    root (h' >= 1), both within prox_tol; finite everywhere, never above w, non-decreasing in v."""
    rho = 1.0 / t
    v, y = prox_inputs(t)
    steps = []
    z = po.prox(v, y, rho, steps=steps)
    w = v + t * y
    assert np.all(np.isfinite(z)) and np.all(z <= w)
    tol = po.prox_tol(v, y, rho)
    rel = np.abs(z - po.prox_exact(v, y, rho)) / tol
    e = t * np.exp(z)
    res = np.abs(z + e - w) / (1.0 + e) / tol
    print(f"[poisson prox t={t}] {steps[0]} sweeps; worst |z - z*| = {float(rel.max()):.2e}, worst |h| / h' = {float(res.max()):.2e} of the tolerance")
    assert float(rel.max()) <= 1.0 and float(res.max()) <= 1.0
    assert steps[0] <= 64                                                       # the library's cap, kPoisMaxSteps
    for k in range(len(PROX_Y)):
        assert np.all(np.diff(z[k * PROX_V.size:k * PROX_V.size + 4001]) >= 0.0)
    # the start is right of the root (or within the tolerance of it) and exp never sees more than 4 max(w, t)
    z0 = po.prox_start(v, y, rho)[0]
    assert np.all(z0 >= po.prox_exact(v, y, rho) - tol) and np.all(t * np.exp(z0) <= 4.0 * np.maximum(w, t))


def test_the_trap_below_t():
    """ln(w / t) bounds the root only for w >= t: below it lies LEFT of the root, and a step clamped from above never moves from there."""
    t, w = 10.0, np.array([1.0, 5.0, 9.999])
    z = po.prox(w, 0.0, 1.0 / t)
    assert np.all(np.log(w / t) < z) and np.all(z < 0.0)
    assert np.array_equal(po.prox_start(w, 0.0, 1.0 / t)[0], np.zeros(3))


def test_the_prox_is_the_minimiser():
    rng = np.random.default_rng(7)
    for _ in range(200):
        rho = float(np.exp(rng.uniform(-5, 5)))
        y = float(rng.choice([0.0, 1.0, 2.0, 17.0, 0.5]))
        v = float(rng.standard_normal() * 6)
        z = float(po.prox(np.array([v]), y, rho)[0])
        grid = z + np.linspace(-3.0, 3.0, 6001)
        obj = lambda u: np.exp(u) - y * u + 0.5 * rho * (u - v) ** 2      # noqa: E731
        assert obj(z) <= obj(grid).min() + 1e-12 * (1.0 + abs(obj(z)))


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("n,p,seed,b0,alpha,f", CELLS)
def test_restatement_against_the_reference_optimum(n, p, seed, b0, alpha, f, intercept):
    x, y = cell_data(n, p, seed, b0)
    lam = cell_lambda(n, p, seed, alpha, f, intercept, b0)
    d = {}
    got = po.poisson(x, y, lam, alpha, intercept, OPTS, [[d]])
    beta, niter = got["beta"][:, 0, 0], int(got["niter"][0, 0])
    assert niter <= OPTS["maxit"]
    _, b_opt, best = cell_optimum(n, p, seed, lam, alpha, intercept, b0)
    excess = excess_of(x, y, beta, lam, alpha, intercept, best)
    diff = support_differences(beta, b_opt)
    print(f"[poisson restatement n={n} p={p} b0={b0} alpha={alpha} f={f} icpt={int(intercept)}] mean count {y.mean():.2f}, niter {niter}, EXCESS {excess:.2e}; "
          f"support {int(np.sum(beta[1:] != 0.0))} vs {int(np.sum(b_opt != 0.0))}, {diff} differ")
    assert -1e-9 <= excess <= EXCESS_CAP
    assert diff <= SUPPORT_SLACK
    assert np.any(beta[1:] != 0.0)
    if alpha == 1.0 and f > 0.0:
        assert np.any(beta[1:] == 0.0)
    if f == 0.0:
        assert np.all(beta[1:] != 0.0)
    if not intercept:
        assert beta[0] == 0.0


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("n,p,seed", SHAPES)
def test_above_lambda_max_the_model_is_empty(n, p, seed, alpha, intercept):
    """Empty-model cells are compared by coefficients: every penalised one exactly 0.0, the intercept log mean(y)."""
    x, y = cell_data(n, p, seed)
    lam = cell_lambda(n, p, seed, alpha, 1.5, intercept)
    got = po.poisson(x, y, lam, alpha, intercept, OPTS)
    beta, niter = got["beta"][:, 0, 0], int(got["niter"][0, 0])
    print(f"[poisson empty n={n} p={p} alpha={alpha} icpt={int(intercept)}] niter {niter}, intercept {beta[0]:.6f} (log mean {np.log(y.mean()):.6f})")
    assert niter <= OPTS["maxit"]
    assert np.all(beta[1:] == 0.0)
    assert abs(beta[0] - np.log(y.mean())) <= 1e-6 if intercept else beta[0] == 0.0      # (measured: 3.6e-10, 2.3e-8, 3.5e-8 at the three shapes)


def test_lambda_one_is_where_the_optimum_empties():
    """lambda_one is the largest entry of the likelihood's gradient at the empty model: mu = mean(y) with the intercept, 1 without."""
    for n, p, seed in SHAPES[:2]:
        x, y = cell_data(n, p, seed)
        for intercept in (True, False):
            xs, _ = lr.standardized_design(x, intercept)
            mu = y.mean() if intercept else 1.0
            assert abs(np.max(np.abs(xs.T @ (y - mu))) - cell_lambda_one(n, p, seed, intercept)) <= 1e-12 * cell_lambda_one(n, p, seed, intercept)
            # at lambda_1 the KKT conditions hold at b = 0, just below they fail
            b = np.zeros(p)
            A = np.hstack([np.ones((n, 1)), xs]) if intercept else xs
            D = np.concatenate([[0.0], np.ones(p)]) if intercept else np.ones(p)
            b_all = np.concatenate([[np.log(y.mean())], b]) if intercept else b
            l1 = cell_lambda_one(n, p, seed, intercept)
            assert po._kkt(A, y, D, b_all, l1 * (1.0 + 1e-9), 1.0)[0] <= 1e-9 * l1
            assert po._kkt(A, y, D, b_all, 0.9 * l1, 1.0)[0] >= 0.09 * l1


def test_k_columns_and_a_grid_equal_the_single_fits():
    x, y = cell_data(400, 8, 1)
    Y = np.column_stack([y, cell_data(400, 8, 1, -2.0)[1], 3.0 * y])
    lam, alpha = (60.0, 200.0, 0.0), (1.0, 0.5, 0.0)
    both = po.poisson(x, Y, lam, alpha, True, OPTS)
    assert both["beta"].shape == (9, 3, 3) and both["niter"].shape == (3, 3)
    for l in range(3):
        for c in range(3):
            one = po.poisson(x, Y[:, c], lam[l], alpha[l], True, OPTS)
            assert one["niter"][0, 0] == both["niter"][c, l] and np.array_equal(one["beta"][:, 0, 0], both["beta"][:, c, l])


def _call(lib, **over):
    from admm_amd._lib import AdmmOpts
    keep = dict(x=np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), y=np.array([0.0, 1.0, 3.0, 0.0, 2.5, 0.0, 1.0, 1.0, 0.0, 0.0, 7.0, 0.0]),
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
    rc = lib.admm_hip_poisson(v["x"], v["y"], v["n"], v["p"], v["k"], v["mem"], v["intercept"], v["lam"], v["alpha"], v["ncell"],
                              ctypes.byref(o) if o is not None else None, v["beta"], v["niter"], None)
    if rc == INVALID_ARG:                                      # a refused call touches no output
        assert np.all(keep["beta"] == 7.0) and np.all(keep["niter"] == -5)
    return rc, lib.admm_hip_last_error().decode()


NULL_MSG = "lambda and alpha must not be NULL"
LAMBDA_MSG = "every lambda must be finite and non-negative"
ALPHA_MSG = "every alpha must lie in [0, 1]"
Y_MSG = "every y must be finite and non-negative"
SUM_MSG = "every column of y must have a positive sum"
ZERO_MSG = "lambda = 0 needs nrow(x) > ncol(x) + intercept"
GOOD_Y = [0, 1, 3, 0, 2.5, 0, 1, 1, 0, 0, 7, 0]
REFUSALS = [
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
    (dict(y_values=GOOD_Y[:6] + [0, 1, -0.5, 0, 1, 0]), Y_MSG),
    (dict(y_values=[0, 1, float("nan"), 0, 1, 0] + GOOD_Y[6:]), Y_MSG),
    (dict(y_values=[0, 1, float("inf"), 0, 1, 0] + GOOD_Y[6:]), Y_MSG),
    (dict(y_values=GOOD_Y[:6] + [0.0] * 6), SUM_MSG),
    (dict(y_values=[0.0] * 6 + GOOD_Y[6:]), SUM_MSG),
    (dict(lam_values=[1.0, 0.0], n=3), ZERO_MSG),                              # 3 rows against 2 columns and the intercept
    (dict(lam_values=[0.0, 1.0], n=2, intercept=0), ZERO_MSG),
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


def test_lambda_max_the_state_form_and_the_hook_refuse_before_any_device_is_touched():
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    # lambda = 0 with 6 rows against 2 columns and the intercept, and non-integer counts: passes every check (and then looks for a device)
    assert _call(lib, lam_values=[1.0, 0.0])[0] != INVALID_ARG
    assert _call(lib, n=2, k=1, y_values=[0, 0.25])[0] != INVALID_ARG
    x, y = np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), np.array([0.0, 1.0, 3.0, 0.0, 2.0, 0.0])
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    out = np.full(1, 7.0)

    def lmax(xp, yp, n, k, outp):
        rc = lib.admm_hip_poisson_lambda_max(xp, yp, n, 2, k, 0, 1, outp)
        assert out[0] == 7.0
        return rc, lib.admm_hip_last_error().decode()

    assert lmax(x.ctypes.data, y.ctypes.data, 6, 0, out.ctypes.data_as(dp)) == (INVALID_ARG, "y must have at least one column")
    assert lmax(None, y.ctypes.data, 6, 1, out.ctypes.data_as(dp)) == (INVALID_ARG, "x and y must not be NULL")
    assert lmax(x.ctypes.data, y.ctypes.data, 6, 1, None) == (INVALID_ARG, "output pointers must not be NULL")
    assert lmax(x.ctypes.data, y.ctypes.data, 1, 1, out.ctypes.data_as(dp)) == (INVALID_ARG, "nrow(x) must be at least 2")
    neg = np.array([0.0, 1.0, -1.0, 0.0, 1.0, 0.0])
    assert lmax(x.ctypes.data, neg.ctypes.data, 6, 1, out.ctypes.data_as(dp)) == (INVALID_ARG, Y_MSG)
    assert lmax(x.ctypes.data, np.zeros(6).ctypes.data, 6, 1, out.ctypes.data_as(dp)) == (INVALID_ARG, SUM_MSG)
    beta, niter, o = np.zeros(3), np.zeros(1, np.int32), AdmmOpts(10, 1e-4, 1e-4, 1.0)
    st, nst = np.zeros(5 * 8 * 2), ctypes.c_longlong()
    rc = lib.admm_hip_poisson_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, 1.0, 1.0, ctypes.byref(o), beta.ctypes.data_as(dp), niter.ctypes.data_as(ip),
                                    None, None, 0, None, st.ctypes.data_as(dp), 2, ctypes.byref(nst))
    assert (rc, lib.admm_hip_last_error().decode()) == (INVALID_ARG, "bad state arguments (the iterate dump needs the trace)")
    rc = lib.admm_hip_poisson_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, -1.0, 1.0, ctypes.byref(o), beta.ctypes.data_as(dp), niter.ctypes.data_as(ip),
                                    None, None, 0, None, None, 0, None)
    assert (rc, lib.admm_hip_last_error().decode()) == (INVALID_ARG, LAMBDA_MSG)
    rc = lib.admm_hip_poisson_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, 1.0, 1.5, ctypes.byref(o), beta.ctypes.data_as(dp), niter.ctypes.data_as(ip),
                                    None, None, 0, None, None, 0, None)
    assert (rc, lib.admm_hip_last_error().decode()) == (INVALID_ARG, ALPHA_MSG)
    v, z = np.array([0.5, -1.0]), np.full(2, 7.0)
    for bad_y, t in ((np.array([1.0, -1.0]), 1.0), (np.array([1.0, 2.0]), 0.0), (np.array([1.0, np.nan]), 1.0)):
        assert lib.admm_hip_test_poisson_prox(v.ctypes.data_as(dp), bad_y.ctypes.data_as(dp), 2, t, z.ctypes.data_as(dp)) == INVALID_ARG
        assert np.all(z == 7.0)


def test_python_builder_argument_checks():
    from admm_amd import ADMM_Poisson, admm_poisson
    from admm_amd.api import ADMM_Poisson_fit
    rng = np.random.default_rng(3)
    x = rng.standard_normal((30, 40))                                # n < p is accepted
    Y = rng.poisson(2.0, size=(30, 3)).astype(np.float64)
    m = admm_poisson(x, Y, [10.0, 0.1, 1.0], alpha=[1.0, 0.5, 0.0])
    assert isinstance(m, ADMM_Poisson) and m.intercept is True and (m.n, m.p, m.k) == (30, 40, 3)
    assert m.lam.tolist() == [10.0, 0.1, 1.0] and m.alpha.tolist() == [1.0, 0.5, 0.0]      # pairs, in the order given
    assert (m.maxit, m.eps_abs, m.eps_rel, m.rho) == (10000, 1e-4, 1e-4, 1.0)
    assert m.opts(maxit=7, rho=2.0).maxit == 7 and m.rho == 2.0
    one = admm_poisson(x, Y[:, 0], 2.0)
    assert one.k == 1 and one.lam.tolist() == [2.0] and one.alpha.tolist() == [1.0]
    assert admm_poisson(x, Y, [2.0, 3.0], alpha=0.25).alpha.tolist() == [0.25, 0.25]       # one alpha for every lambda
    assert admm_poisson(x, Y + 0.5, 1.0).k == 3                                             # non-integer counts
    auto = admm_poisson(x, Y, alpha=0.5)
    assert auto.lam is None and auto.nlambda == 100 and auto.lambda_min_ratio == 0.01 and auto.alpha.tolist() == [0.5] * 100
    assert admm_poisson(x[:, :5], Y, nlambda=7).lambda_min_ratio == 0.0001
    assert admm_poisson(x[:, :5], Y, 0.0).lam.tolist() == [0.0]                             # the plain GLM: 30 > 5 + 1
    for bad in (-1.0, np.nan, np.inf, [1.0, -0.5]):
        with pytest.raises(ValueError, match="finite and non-negative"):
            admm_poisson(x, Y, bad)
    with pytest.raises(ValueError, match="lambda = 0 needs nrow\\(x\\) > ncol\\(x\\) \\+ intercept"):
        admm_poisson(x, Y, [1.0, 0.0])
    with pytest.raises(ValueError, match="lambda = 0 needs"):
        admm_poisson(x[:, :29], Y, 0.0)
    assert admm_poisson(x[:, :29], Y, 0.0, intercept=False).lam.tolist() == [0.0]
    for bad in (-0.1, 1.5, np.nan, [1.0, 2.0]):
        with pytest.raises(ValueError, match="every alpha must lie in \\[0, 1\\]"):
            admm_poisson(x, Y, [1.0, 2.0], alpha=bad)
    with pytest.raises(ValueError, match="as long as lam"):
        admm_poisson(x, Y, [1.0, 2.0], alpha=[1.0, 0.5, 0.2])
    with pytest.raises(ValueError, match="at least one value"):
        admm_poisson(x, Y, [])
    with pytest.raises(ValueError, match="alpha = 0 has no lambda_max"):
        admm_poisson(x, Y, alpha=0.0)
    Yb = Y.copy()
    Yb[3, 2] = -1.0
    with pytest.raises(ValueError, match="every y must be finite and non-negative"):
        admm_poisson(x, Yb, 1.0)
    Yb[3, 2] = np.nan
    with pytest.raises(ValueError, match="every y must be finite and non-negative"):
        admm_poisson(x, Yb, 1.0)
    Yb = Y.copy()
    Yb[:, 1] = 0.0
    with pytest.raises(ValueError, match="every column of y must have a positive sum"):
        admm_poisson(x, Yb, 1.0)
    with pytest.raises(ValueError, match="nrow\\(x\\) should be equal to nrow\\(Y\\)"):
        admm_poisson(x, Y[:-1], 1.0)
    with pytest.raises(ValueError, match="single count column and a single cell"):
        admm_poisson(x, Y, 1.0).fit(trace=True)
    with pytest.raises(ValueError, match="single count column and a single cell"):
        admm_poisson(x, Y[:, 0], [1.0, 2.0]).fit(trace=True)
    assert "Poisson" in repr(ADMM_Poisson_fit(np.ones(1), np.ones(1), np.zeros((3, 2, 1)), np.zeros((2, 1)), {}))
