"""CPU: logistic regression (admm_hip_logit) without a device -- the Newton prox of the restatement (tests/logit_oracle.py) against
bisection, the restatement of the loop against a float64 IRLS optimum, the symbols through every layer, what the C ABI refuses before
it looks for a device, and the Python builder's argument checks.

Prox: |z - z*| <= 1e-13 max(1, |v|, t) against the bisected root, t = 1 / rho in [1e-3, 1e3]; because h' >= 1 the error in z is at most
the error in evaluating h, a few ulp of max(|v|, t), and a missing Newton step shows orders of magnitude above the tolerance.

Bound against IRLS (eps_abs = eps_rel = 1e-4, rho in {0.1, 1, 10}, both intercept settings, (400, 8, seed 1) and (2100, 40, seed 2)):
the measured worst relative excess of the objective, nll / nll_IRLS - 1, on exactly these inputs is 1.49e-8 (400 x 8, intercept,
rho = 10; every other case is below 1e-9).  The cap is ten times that, rounded up to a power of ten: 1e-6.  Iterations: 13 - 36."""
import ctypes
import os
import re

import numpy as np
import pytest

import logit_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
SHAPES = [(400, 8, 1), (2100, 40, 2)]
RHOS = [0.1, 1.0, 10.0]
OPTS = {"maxit": 10000, "eps_abs": 1e-4, "eps_rel": 1e-4, "rho": 1.0}
EXCESS_CAP = 1e-6                # see the docstring; tests/test_gpu_logit.py restates it
SYMBOLS = ("admm_hip_logit", "admm_hip_logit_state", "admm_hip_test_logit_prox")
PROX_V = np.concatenate([np.linspace(-60.0, 60.0, 4001), [745.0, -745.0, 800.0, -800.0, 0.0, 1e-300, -1e-300]])
PROX_T = [1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0, 1e3]


def test_symbols_are_declared_exported_bound_and_documented():
    from admm_amd import _lib
    header = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"ADMM_HIP_API int " + name + r"\(", header), name
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)                                   # exported by the shared library
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
        assert "`" + name + "`" in doc, name
    assert len(lib.admm_hip_logit.argtypes) == 10
    assert len(lib.admm_hip_logit_state.argtypes) == len(lib.admm_hip_lad_state.argtypes)
    shim = open(os.path.join(ROOT, "integration", "admm_shim.cpp")).read()
    assert "RcppExport SEXP admm_logit(" in shim and "admm_hip_logit(" in shim


@pytest.mark.parametrize("t", PROX_T)
def test_prox_against_bisection(t):
    rho = 1.0 / t
    z = lo.prox(PROX_V, rho)
    ze = lo.prox_exact(PROX_V, rho)
    rel = np.abs(z - ze) / lo.prox_tol(PROX_V, rho)
    print(f"[logit prox t={t}] worst |z - z*| = {float(rel.max()):.2e} of the tolerance")
    assert np.all(np.isfinite(z)) and float(rel.max()) <= 1.0
    assert np.all(z >= PROX_V) and np.all(z <= PROX_V + 1.0 / rho)          # inside the bracket
    assert np.all(np.diff(z[:4001]) >= 0.0)                                  # non-decreasing in v


def test_prox_is_the_argmin_and_the_root():
    """log(1 + e^-z) + rho / 2 (z - v)^2 is not lower anywhere on a fine grid, and h changes sign across the result."""
    rng = np.random.default_rng(11)
    for _ in range(200):
        rho = float(np.exp(rng.uniform(-5, 5)))
        v = float(rng.standard_normal() * 6 * (1 + 1 / rho))
        z = float(lo.prox(np.array([v]), rho)[0])
        grid = np.linspace(v, v + 1 / rho, 20001)
        obj = lambda u: np.maximum(-u, 0.0) + np.log1p(np.exp(-np.abs(u))) + 0.5 * rho * (u - v) ** 2      # noqa: E731
        assert obj(np.array([z]))[0] <= obj(grid).min() + 1e-12 * (1 + abs(obj(np.array([z]))[0])), (rho, v)
        h = lambda u: u - v - lo._sigma_neg(np.array([u]))[0] / rho                                           # noqa: E731
        w = 1e-12 * max(1.0, abs(v), 1 / rho)
        assert h(z - w) <= 0.0 <= h(z + w), (rho, v, z)


def test_a_fixed_four_steps_miss_the_tolerance_at_t_100():
    """The bound bites: four Newton steps from the stated start are 4e-5 off at t = 100."""
    v, t = PROX_V, 100.0
    hi = v + t
    z = np.where(v > 0.0, v, np.where(hi < 0.0, hi, 0.0))
    for _ in range(4):
        s = lo._sigma_neg(z)
        z = np.minimum(np.maximum(z - (z - v - t * s) / (1.0 + t * s * (1.0 - s)), v), hi)
    assert float(np.max(np.abs(z - lo.prox_exact(v, 1.0 / t)) / lo.prox_tol(v, 1.0 / t))) > 1e3


_IRLS = {}


def _irls(n, p, seed, intercept):
    key = (n, p, seed, intercept)
    if key not in _IRLS:
        _IRLS[key] = lo.logit_irls(*lo.logit_data(n, p, seed), intercept)
    return _IRLS[key]


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("n,p,seed", SHAPES)
def test_restatement_against_the_irls_optimum(n, p, seed, rho, intercept):
    x, y = lo.logit_data(n, p, seed)
    assert 0.3 < y.mean() < 0.5
    got = lo.logit(x, y, intercept, dict(OPTS, rho=rho))
    assert got["niter"] <= 60
    _, best, steps = _irls(n, p, seed, intercept)
    assert steps <= 8                                                 # not separable
    f = lo.nll(x, y, got["beta"])
    excess = f / best - 1.0
    print(f"[logit restatement n={n} p={p} rho={rho} icpt={int(intercept)}] niter {got['niter']}, nll {f:.9e} vs IRLS {best:.9e} (+{excess:.2e})")
    assert -1e-9 <= excess <= EXCESS_CAP
    if not intercept:
        assert got["beta"][0] == 0.0


def test_restated_iteration_counts():
    """What tests/test_gpu_logit.py quotes for rho = 0.1 and rho = 10 at (2100, 40)."""
    x, y = lo.logit_data(2100, 40, 2)
    assert [lo.logit(x, y, True, dict(OPTS, rho=r))["niter"] for r in (0.1, 1.0, 10.0)] == [13, 16, 36]


def _call(lib, **over):
    from admm_amd._lib import AdmmOpts
    keep = dict(x=np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), y=np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0]), beta=np.full(3, 7.0),
                niter=np.full(1, -5, np.int32))
    if "y_values" in over:
        keep["y"] = np.asarray(over.pop("y_values"), dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    v = dict(x=keep["x"].ctypes.data, y=keep["y"].ctypes.data, n=6, p=2, mem=0, intercept=1, opts=(10, 1e-4, 1e-4, 1.0),
             beta=keep["beta"].ctypes.data_as(dp), niter=keep["niter"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    v.update(over)
    o = AdmmOpts(*v["opts"]) if v["opts"] is not None else None
    rc = lib.admm_hip_logit(v["x"], v["y"], v["n"], v["p"], v["mem"], v["intercept"], ctypes.byref(o) if o is not None else None, v["beta"], v["niter"], None)
    if rc == INVALID_ARG:                                      # a refused call touches no output
        assert keep["beta"].tolist() == [7.0] * 3 and keep["niter"].tolist() == [-5]
    return rc, lib.admm_hip_last_error().decode()


LABEL_MSG = "every label in y must be exactly 0 or 1"
CLASS_MSG = "y must hold both classes"
REFUSALS = [
    (dict(y_values=[0, 1, 0.5, 0, 1, 0]), LABEL_MSG),
    (dict(y_values=[0, 1, float("nan"), 0, 1, 0]), LABEL_MSG),
    (dict(y_values=[0, 1, 2.0, 0, 1, 0]), LABEL_MSG),
    (dict(y_values=[0, 1, -1.0, 0, 1, 0]), LABEL_MSG),
    (dict(y_values=[0, 1, float("inf"), 0, 1, 0]), LABEL_MSG),
    (dict(y_values=[0.0] * 6), CLASS_MSG),
    (dict(y_values=[1.0] * 6), CLASS_MSG),
    (dict(n=3, p=2, intercept=1), "nrow(x) must be greater than ncol(x) + 1 (the intercept is fitted)"),
    (dict(n=2, p=2, intercept=0), "nrow(x) must be greater than ncol(x)"),
    (dict(x=None), "x and y must not be NULL"),
    (dict(n=0), "n and p must be positive"),
    (dict(mem=7), "mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE"),
    (dict(opts=None), "opts must not be NULL"),
    (dict(opts=(0, 1e-4, 1e-4, 1.0)), "maxit should be positive"),
    (dict(opts=(10, 1e-4, 1e-4, 0.0)), "rho should be positive"),
    (dict(beta=None), "output pointers must not be NULL"),
]


@pytest.mark.parametrize("over,message", REFUSALS, ids=[f"{k}-" + m[:24] + "/" + ",".join(o) for k, (o, m) in enumerate(REFUSALS)])
def test_bad_calls_are_refused_before_any_device_is_touched(over, message):
    from admm_amd import _lib
    lib = _lib.load()
    assert _call(lib, **dict(over)) == (INVALID_ARG, message)


def test_the_shape_is_refused_before_the_labels_and_negative_zero_is_a_label():
    from admm_amd import _lib
    lib = _lib.load()
    assert _call(lib, y_values=[0.5] * 6, n=3)[1] == "nrow(x) must be greater than ncol(x) + 1 (the intercept is fitted)"
    assert _call(lib, y_values=[-0.0, 1, 1, 0, 1, 0])[0] != INVALID_ARG          # passes every check (and then the call looks for a device)
    assert _call(lib, n=3, p=2, intercept=0, y_values=[0, 1, 1])[0] != INVALID_ARG


def test_state_entry_point_refuses_like_lad_state():
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    x, y = np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    beta, niter, o = np.zeros(3), np.zeros(1, np.int32), AdmmOpts(10, 1e-4, 1e-4, 1.0)
    st, nst = np.zeros(64), ctypes.c_longlong()
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.admm_hip_logit_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, ctypes.byref(o), beta.ctypes.data_as(dp),
                                  niter.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None, 0, None, st.ctypes.data_as(dp), 2, ctypes.byref(nst))
    assert (rc, lib.admm_hip_last_error().decode()) == (INVALID_ARG, "bad state arguments (the iterate dump needs the trace)")
    assert lib.admm_hip_test_logit_prox(None, 4, 1.0, None) == INVALID_ARG
    v = np.zeros(4)
    assert lib.admm_hip_test_logit_prox(v.ctypes.data_as(dp), 4, 0.0, v.ctypes.data_as(dp)) == INVALID_ARG


def test_python_builder_argument_checks():
    from admm_amd import ADMM_Logit, admm_logit
    from admm_amd.api import ADMM_LAD, ADMM_Logit_fit
    rng = np.random.default_rng(3)
    x = rng.standard_normal((30, 12))
    y = (rng.uniform(size=30) < 0.4).astype(np.float64)
    m = admm_logit(x, y)
    assert isinstance(m, ADMM_Logit) and isinstance(m, ADMM_LAD) and m.intercept is True
    assert (m.maxit, m.eps_abs, m.eps_rel, m.rho) == (10000, 1e-4, 1e-4, 1.0)          # as admm_lad
    assert m.opts(maxit=7, rho=2.0).maxit == 7 and m.rho == 2.0
    with pytest.raises(ValueError, match="maxit should be positive"):
        m.opts(maxit=0)
    assert admm_logit(x, y > 0.5).y.dtype == np.float64 and admm_logit(x, y.astype(int)).y.tolist() == y.tolist()      # booleans and integers are labels
    for bad in (0.5, np.nan, 2.0, -1.0):
        yb = y.copy()
        yb[3] = bad
        with pytest.raises(ValueError, match="exactly 0 or 1"):
            admm_logit(x, yb)
    with pytest.raises(ValueError, match="both classes"):
        admm_logit(x, np.zeros(30))
    with pytest.raises(ValueError, match="both classes"):
        admm_logit(x, np.ones(30))
    with pytest.raises(ValueError, match="nrow\\(x\\) should be equal to length\\(y\\)"):
        admm_logit(x, y[:-1])
    with pytest.raises(ValueError, match="the intercept is fitted"):
        admm_logit(x[:13], y[:13])                                                   # n = p + 1
    with pytest.raises(ValueError, match="the intercept is fitted"):
        admm_logit(x[:12], y[:12])                                                   # n = p
    assert admm_logit(x[:13], y[:13], intercept=False).n == 13
    with pytest.raises(ValueError, match="nrow\\(x\\) must be greater than ncol\\(x\\)"):
        admm_logit(x[:12], y[:12], intercept=False)
    assert "logistic" in repr(ADMM_Logit_fit(np.zeros(3), 4, {}))
