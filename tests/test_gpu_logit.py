"""GPU: logistic regression (admm_hip_logit) -- the Newton prox (logit2) through the three LAD branches and every register layout of
the rows kernel, alone through its test hook, and the boundary: label flip, device-resident input, rho, separable labels, refusals.
The CPU restatement, the IRLS optimum and the replay are tests/logit_oracle.py; shapes are those of tests/test_gpu_quantreg.py: the
smallest that reach each branch and each layout.

Bounds: the follow tolerance 1e-8 is the loop's (tests/test_gpu_quantreg.py, tests/test_gpu_huber.py); the objective's excess over IRLS
is capped at 1e-6, ten times the restatement's measured worst case on these inputs, 1.49e-8, rounded up to a power of ten
(tests/test_logit_host.py); the prox within 1e-13 max(1, |v|, t) of the bisected root (a few ulp of max(|v|, t) is the floor, a missing
Newton step is orders of magnitude above); the dumped z within the same tolerance of the restatement's, y bit for bit from it."""
import ctypes

import numpy as np
import pytest

import logit_oracle as lo
from helpers import dense_state_records
from test_gpu_quantreg import BRANCHES, LAYOUTS
from test_logit_host import EXCESS_CAP, PROX_T, PROX_V

pytestmark = pytest.mark.gpu

OPTS = {"maxit": 10000, "eps_abs": 1e-4, "eps_rel": 1e-4, "rho": 1.0}
INVALID_ARG = 1

_cache = {}


def _data(n, p, seed):
    key = ("data", n, p, seed)
    if key not in _cache:
        _cache[key] = lo.logit_data(n, p, seed)
    return _cache[key]


def _irls(n, p, seed, intercept):
    key = ("irls", n, p, seed, intercept)
    if key not in _cache:
        _cache[key] = lo.logit_irls(*_data(n, p, seed), intercept)
    return _cache[key]


def _fit(x, y, intercept=True, maxit=10000, rho=1.0, trace=False, state=0, **opt):
    from admm_amd import admm_logit, options
    with options(**opt):
        return admm_logit(x, y, intercept=intercept).opts(maxit=maxit, rho=rho).fit(trace=trace, state=state)


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_three_branches_against_the_restatement_and_irls(branch, intercept):
    n, p, seed, onepass = BRANCHES[branch]
    x, y = _data(n, p, seed)
    label = f"{branch} n={n} p={p} icpt={int(intercept)}"
    fit = _fit(x, y, intercept=intercept, trace=True, state=dense_state_records(n, 10000), LAD_ONEPASS=onepass)
    assert fit.stats["xupdate_variant"] == (1 if branch == "onepass" else 0)
    assert fit.beta.shape == (p + 1,) and np.all(np.isfinite(fit.beta))
    lo.followed(fit.beta, fit.niter, fit.trace, x, y, intercept, OPTS, tol=1e-8, label=label)
    assert lo.replay(fit.trace, fit.state, y, label=label) >= 8
    _, best, _ = _irls(n, p, seed, intercept)
    excess = lo.nll(x, y, fit.beta) / best - 1.0
    print(f"[logit {label}] niter {fit.niter}, objective +{excess:.2e} over IRLS")
    assert -1e-9 <= excess <= EXCESS_CAP
    if not intercept:
        assert fit.beta[0] == 0.0


@pytest.mark.parametrize("n,p,maxit", LAYOUTS)
def test_every_register_layout_of_the_rows_kernel_with_the_newton_prox(n, p, maxit):
    """Labels that are separable at p / n above one half: the test pins the loop, not the optimum."""
    x, y = _data(n, p, 100 + p)
    label = f"layout n={n} p={p}"
    fit = _fit(x, y, maxit=maxit, trace=True, state=dense_state_records(n, maxit))
    assert fit.stats["xupdate_variant"] == 1
    assert np.all(np.isfinite(fit.beta))
    lo.followed(fit.beta, fit.niter, fit.trace, x, y, True, dict(OPTS, maxit=maxit), tol=1e-8, label=label)
    assert lo.replay(fit.trace, fit.state, y, label=label) >= 8


@pytest.mark.parametrize("t", PROX_T)
def test_the_device_prox_alone_through_the_hook(t):
    from admm_amd import _lib
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    v = np.ascontiguousarray(PROX_V)
    z = np.full(v.size, np.nan)
    assert lib.admm_hip_test_logit_prox(v.ctypes.data_as(dp), v.size, float(t), z.ctypes.data_as(dp)) == 0
    assert np.all(np.isfinite(z))
    ze = lo.prox_exact(v, 1.0 / t)
    rel = np.abs(z - ze) / lo.prox_tol(v, 1.0 / t)
    print(f"[logit device prox t={t}] worst |z - z*| = {float(rel.max()):.2e} of the tolerance 1e-13 max(1, |v|, t)")
    assert float(rel.max()) <= 1.0
    assert np.all(z >= v) and np.all(z <= v + t)
    assert np.all(np.diff(z[:4001]) >= 0.0)                      # non-decreasing in v along the linspace


def test_the_device_prox_stays_finite_far_outside_the_tested_range():
    from admm_amd import _lib
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    v = np.array([1e300, -1e300, 1e35, -1e35, 3e38, -3e38, 1e5, -1e5, -5e5, 0.0])
    for t in (1e-6, 1.0, 1e6):
        z = np.full(v.size, np.nan)
        assert lib.admm_hip_test_logit_prox(v.ctypes.data_as(dp), v.size, t, z.ctypes.data_as(dp)) == 0
        ze = lo.prox_exact(v, 1.0 / t)
        assert np.all(np.isfinite(z)) and np.all(np.abs(z - ze) <= 1e-13 * np.maximum(1.0, np.maximum(np.abs(v), t))), (t, z, ze)


def test_label_flip_negates_the_coefficients():
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = _data(n, p, seed)
    a = _fit(x, y)
    b = _fit(x, 1.0 - y)
    assert a.stats["xupdate_variant"] == b.stats["xupdate_variant"] == 1
    assert a.niter == b.niter
    err = float(np.max(np.abs(a.beta + b.beta)) / np.max(np.abs(a.beta)))
    print(f"[logit flip] niter {a.niter}, |beta + beta_flipped| {err:.2e}")
    assert err <= 1e-12


def test_device_resident_input_is_bit_identical():
    import torch
    from admm_amd import DevicePtr, admm_logit
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = _data(n, p, seed)
    a = _fit(x, y)
    xd = torch.tensor(np.asfortranarray(x).T.copy(), device="cuda")      # p x n row-major == n x p column-major
    yd = torch.tensor(y, device="cuda")
    torch.cuda.synchronize()
    d = admm_logit(DevicePtr(xd.data_ptr()), DevicePtr(yd.data_ptr()), n=n, p=p).fit()
    assert d.niter == a.niter and d.beta.tobytes() == a.beta.tobytes()
    assert np.array_equal(yd.cpu().numpy(), y)                             # the labels are the caller's


@pytest.mark.parametrize("rho,niter", [(0.1, 13), (10.0, 36)])
def test_other_rho(rho, niter):
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = _data(n, p, seed)
    fit = _fit(x, y, rho=rho)
    _, best, _ = _irls(n, p, seed, True)
    excess = lo.nll(x, y, fit.beta) / best - 1.0
    print(f"[logit rho={rho}] niter {fit.niter} (restatement: {niter}), objective +{excess:.2e} over IRLS")
    assert -1e-9 <= excess <= EXCESS_CAP
    assert fit.niter <= 10000


def test_separable_labels_run_out_of_iterations_with_finite_coefficients():
    n, p, seed, _ = BRANCHES["hat"]
    x, _ = _data(n, p, seed)
    y = (x[:, 0] > 0.3).astype(np.float64)
    fit = _fit(x, y, maxit=50)
    assert fit.niter == 51 and np.all(np.isfinite(fit.beta))
    assert fit.beta[1] > 0.0


def test_c_abi_refusals_touch_no_output():
    import torch
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    n, p = 64, 3
    rng = np.random.default_rng(5)
    x = np.asfortranarray(rng.standard_normal((n, p)))
    y = (rng.uniform(size=n) < 0.5).astype(np.float64)
    o = AdmmOpts(100, 1e-4, 1e-4, 1.0)

    def call(xptr, yptr, n_, mem):
        beta, niter = np.full(p + 1, 7.0), np.full(1, -5, np.int32)
        rc = lib.admm_hip_logit(xptr, yptr, n_, p, mem, 1, ctypes.byref(o), beta.ctypes.data_as(dp), niter.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None)
        assert beta.tolist() == [7.0] * (p + 1) and niter.tolist() == [-5]
        return rc, lib.admm_hip_last_error().decode()

    bad = y.copy()
    bad[17] = 2.0
    assert call(x.ctypes.data, bad.ctypes.data, n, 0) == (INVALID_ARG, "every label in y must be exactly 0 or 1")
    xd = torch.tensor(x.T.copy(), device="cuda")
    bd, od, nd = torch.tensor(bad, device="cuda"), torch.ones(n, dtype=torch.float64, device="cuda"), torch.tensor(y, device="cuda")
    nd[5] = float("nan")
    torch.cuda.synchronize()
    assert call(xd.data_ptr(), bd.data_ptr(), n, 1) == (INVALID_ARG, "every label in y must be exactly 0 or 1")
    assert call(xd.data_ptr(), nd.data_ptr(), n, 1) == (INVALID_ARG, "every label in y must be exactly 0 or 1")
    assert call(xd.data_ptr(), od.data_ptr(), n, 1) == (INVALID_ARG, "y must hold both classes")
    zeros = np.zeros(n)
    assert call(x.ctypes.data, zeros.ctypes.data, n, 0) == (INVALID_ARG, "y must hold both classes")
    assert call(x.ctypes.data, y.ctypes.data, p + 1, 0) == (INVALID_ARG, "nrow(x) must be greater than ncol(x) + 1 (the intercept is fitted)")
