"""GPU: ridge logistic regression (admm_hip_logit_ridge) -- the signed Newton prox with the square-loss case on the ridge rows
(kProxLogitR) through the three LAD branches and every register layout of the rows kernels, the lambda grid on one setup, the slotted
route, and the boundary: separable labels, n < p, device-resident input, repeatability, the one-vs-rest helper, refusals.

The CPU restatement, the ridge IRLS optimum and the replay are tests/logit_ridge_oracle.py; the shapes are BRANCHES and LAYOUTS of
tests/test_gpu_quantreg.py, the smallest that reach each branch and each register layout (with the ridge rows 400 x 8 is still the hat
branch, 408 <= 2000, and 2100 x 40 still one-pass / two-pass).

Bounds: the follow tolerance 1e-8 is the loop's (tests/test_gpu_logit.py); the objective's excess over the ridge IRLS optimum is capped
by tests/test_logit_ridge_host.py's EXCESS_CAP; the replay holds the logistic rows to logit_oracle.prox_tol, the ridge rows to 4 ulp of
v (rho / (1 + rho)) and y to the bit.  A kernel that treated sign 0 as the S form would give z = 0 on the ridge rows: the replay and the
excess both fail then.  Between the grid call and its single fits the yardstick is numbers (== / array_equal), between the serial and the
slotted route of the same call it is bytes."""
import ctypes

import numpy as np
import pytest

import logit_multi_oracle as lm
import logit_oracle as lo
import logit_ridge_oracle as lr
from helpers import dense_state_records
from test_gpu_logit_multi import MAX_SLOTS, _layout_problem, _npt
from test_gpu_quantreg import BRANCHES, LAYOUTS
from test_logit_multi_host import problem
from test_logit_ridge_host import EXCESS_CAP, OPTS, cell_data, cell_irls

pytestmark = pytest.mark.gpu

INVALID_ARG = 1
GRID = (10.0, 0.1, 1.0)
LAMBDA_MSG = "every lambda must be finite and positive (lambda = 0 is admm_hip_logit_multi)"

_cache = {}


def _fit(x, Y, lam, intercept=True, maxit=10000, trace=False, state=0, **opt):
    from admm_amd import admm_logit_ridge, options
    with options(**opt):
        return admm_logit_ridge(x, Y, lam, intercept=intercept).opts(maxit=maxit).fit(trace=trace, state=state)


def _excess(x, y, beta, lam, intercept, best):
    return lr.objective_of(x, y, beta, lam, intercept) / best - 1.0


def _serial(tag, x, Y, lam, maxit=10000):
    """the call on its serial route (QUANT_SLOTS=1), fitted once per problem"""
    key = ("serial", tag, tuple(np.atleast_1d(lam)), maxit)
    if key not in _cache:
        f = _fit(x, Y, lam, maxit=maxit, QUANT_SLOTS=1)
        assert f.stats["xupdate_variant"] == 1
        _cache[key] = (f.beta.copy(), f.niter.copy())
    return _cache[key]


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_three_branches_against_the_restatement_and_the_ridge_irls(branch, intercept):
    n, p, seed, onepass = BRANCHES[branch]
    x, y = cell_data(n, p, seed, "data")
    label = f"{branch} n={n} p={p} icpt={int(intercept)}"
    fit = _fit(x, y, 1.0, intercept=intercept, trace=True, state=dense_state_records(n + p, 10000), LAD_ONEPASS=onepass)
    assert fit.stats["xupdate_variant"] == (1 if branch == "onepass" else 0)
    assert fit.beta.shape == (p + 1,) and np.all(np.isfinite(fit.beta))
    lr.followed(fit.beta, fit.niter, fit.trace, x, y, 1.0, intercept, OPTS, tol=1e-8, label=label)
    assert lr.replay(fit.trace, fit.state, y, p, label=label) >= 8
    excess = _excess(x, y, fit.beta, 1.0, intercept, cell_irls(n, p, seed, "data", 1.0, intercept)[2])
    print(f"[logit ridge {label}] niter {fit.niter}, objective +{excess:.2e} over the ridge IRLS")
    assert -1e-9 <= excess <= EXCESS_CAP
    if not intercept:
        assert fit.beta[0] == 0.0


@pytest.mark.parametrize("n,p,maxit", LAYOUTS)
def test_every_register_layout_of_the_rows_kernel(n, p, maxit):
    x, y = lo.logit_data(n, p, 100 + p)
    label = f"layout n={n} p={p}"
    fit = _fit(x, y, 1.0, maxit=maxit, trace=True, state=dense_state_records(n + p, maxit))
    assert fit.stats["xupdate_variant"] == 1
    assert np.all(np.isfinite(fit.beta))
    lr.followed(fit.beta, fit.niter, fit.trace, x, y, 1.0, True, dict(OPTS, maxit=maxit), tol=1e-8, label=label)
    assert lr.replay(fit.trace, fit.state, y, p, label=label) >= 8


def test_every_cell_of_the_grid_call_equals_the_single_fit():
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    beta, niter = _serial((n, p, seed), x, Y, GRID)
    assert beta.shape == (p + 1, lm.K, len(GRID)) and niter.shape == (lm.K, len(GRID)) and np.all(np.isfinite(beta))
    for l, lam in enumerate(GRID):
        for c in range(lm.K):
            one = _fit(x, Y[:, c], lam, QUANT_SLOTS=1)
            assert one.beta.shape == (p + 1, 1, 1) and one.stats["xupdate_variant"] == 1
            assert int(one.niter[0, 0]) == int(niter[c, l]), (c, lam, niter.tolist())
            assert np.array_equal(one.beta[:, 0, 0], beta[:, c, l]), (c, lam)
    print(f"[logit ridge grid] niter {niter.T.tolist()}")
    assert int(niter.max()) <= 10000


@pytest.mark.parametrize("slots", [2, 3, 4])
def test_slots_are_byte_identical_to_the_serial_route(slots):
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    beta1, niter1 = _serial((n, p, seed), x, Y, GRID)
    fit = _fit(x, Y, GRID, QUANT_SLOTS=slots)
    assert fit.stats["xupdate_variant"] == 8 + slots
    assert fit.lam.tolist() == list(GRID)
    assert fit.niter.tobytes() == niter1.tobytes() and fit.beta.tobytes() == beta1.tobytes()
    assert fit.beta[:, 4].tobytes() == fit.beta[:, 5].tobytes() and np.array_equal(fit.niter[4], fit.niter[5])      # the column that is there twice
    assert np.array_equal(fit.beta[:, 6], -fit.beta[:, 0]) and np.array_equal(fit.niter[6], fit.niter[0])          # the flipped column
    assert np.any(fit.beta[:, 0] != 0.0)


def test_automatic_takes_as_many_slots_as_the_layout_admits():
    """QUANT_SLOTS unset: the measured choice (profiles/logit_ridge.md), clipped to the number of columns."""
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    beta1, niter1 = _serial((n, p, seed), x, Y, GRID)
    fit = _fit(x, Y, GRID)
    assert fit.stats["xupdate_variant"] == 12
    assert fit.niter.tobytes() == niter1.tobytes() and fit.beta.tobytes() == beta1.tobytes()
    assert _fit(x, Y[:, :3], 1.0).stats["xupdate_variant"] == 11
    assert _fit(x, Y[:, 0], GRID).stats["xupdate_variant"] == 1          # one column: the serial route, whatever the grid


def _layout_cases():
    for n, p, maxit in LAYOUTS:
        top = MAX_SLOTS[_npt(p)]                                  # kProxLogitR's max_slots row is the S form's
        for want in sorted({max(top, 2), 2}, reverse=True):
            yield pytest.param(n, p, maxit, want, id=f"{n}x{p}-slots{want}")


@pytest.mark.parametrize("n,p,maxit,want", list(_layout_cases()))
def test_slots_on_every_register_layout(n, p, maxit, want):
    """Five label columns at lambda = 1.  Five and six double2 per thread and row leave the form no second slot: serial."""
    x, Y = _layout_problem(n, p)
    top = MAX_SLOTS[_npt(p)]
    beta1, niter1 = _serial(("layout", n, p), x, Y, 1.0, maxit=maxit)
    fit = _fit(x, Y, 1.0, maxit=maxit, QUANT_SLOTS=want)
    assert fit.stats["xupdate_variant"] == (8 + min(want, top) if top >= 2 else 1)
    assert fit.niter.tobytes() == niter1.tobytes() and fit.beta.tobytes() == beta1.tobytes()
    assert np.all(np.isfinite(fit.beta)) and np.any(fit.beta != 0.0)


def test_separable_labels_have_an_estimate():
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = cell_data(n, p, seed, "separable")
    fit = _fit(x, y, 1.0)
    beta, niter = fit.beta[:, 0, 0], int(fit.niter[0, 0])
    excess = _excess(x, y, beta, 1.0, True, cell_irls(n, p, seed, "separable", 1.0, True)[2])
    print(f"[logit ridge separable] niter {niter}, objective +{excess:.2e} over the ridge IRLS")
    assert fit.stats["xupdate_variant"] == 1
    assert niter <= 10000 and np.all(np.isfinite(beta))
    assert -1e-9 <= excess <= EXCESS_CAP


@pytest.mark.parametrize("hat", [None, "0"])
def test_more_columns_than_rows(hat):
    """150 x 200: accepted, converges; LAD_HAT=0 sends the 350 augmented rows through the rows kernel."""
    n, p, seed = 150, 200, 3
    x, y = cell_data(n, p, seed, "data")
    fit = _fit(x, y, (1.0, 10.0), LAD_HAT=hat)
    assert fit.stats["xupdate_variant"] == (0 if hat is None else 1)
    assert fit.beta.shape == (p + 1, 1, 2) and np.all(np.isfinite(fit.beta))
    for l, lam in enumerate((1.0, 10.0)):
        excess = _excess(x, y, fit.beta[:, 0, l], lam, True, cell_irls(n, p, seed, "data", lam, True)[2])
        print(f"[logit ridge 150 x 200 LAD_HAT={hat} lambda={lam}] niter {int(fit.niter[0, l])}, objective +{excess:.2e} over the ridge IRLS")
        assert int(fit.niter[0, l]) <= 10000
        assert -1e-9 <= excess <= EXCESS_CAP


def test_device_resident_input_is_byte_identical_and_the_buffers_stay_the_callers():
    import torch
    from admm_amd import DevicePtr, admm_logit_ridge, options
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    a = _fit(x, Y, GRID, QUANT_SLOTS=4)
    xh = np.asfortranarray(x).T.copy()
    xd = torch.tensor(xh, device="cuda")                                 # p x n row-major == n x p column-major
    yd = torch.tensor(Y.T.copy(), device="cuda")                         # k x n row-major == n x k column-major
    torch.cuda.synchronize()
    with options(QUANT_SLOTS=4):
        d = admm_logit_ridge(DevicePtr(xd.data_ptr()), DevicePtr(yd.data_ptr()), GRID, n=n, p=p, k=lm.K).fit()
    assert d.stats["xupdate_variant"] == a.stats["xupdate_variant"] == 12
    assert d.niter.tobytes() == a.niter.tobytes() and d.beta.tobytes() == a.beta.tobytes()
    assert np.array_equal(yd.cpu().numpy(), Y.T) and np.array_equal(xd.cpu().numpy(), xh)


def test_two_identical_calls_are_byte_identical():
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    a, b = _fit(x, Y, GRID, QUANT_SLOTS=3), _fit(x, Y, GRID, QUANT_SLOTS=3)
    assert a.stats["xupdate_variant"] == b.stats["xupdate_variant"] == 11
    assert a.niter.tobytes() == b.niter.tobytes() and a.beta.tobytes() == b.beta.tobytes()


def test_one_vs_rest_is_the_call_on_the_indicator_matrix():
    from admm_amd import admm_logit_ridge_ovr, options
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    labels = np.where(Y[:, 1] == 1.0, 5, np.where(Y[:, 2] == 1.0, 11, -3))      # three classes, all populated
    classes = np.array([-3, 5, 11])
    assert np.all(np.bincount(np.searchsorted(classes, labels)) > 0)
    with options(QUANT_SLOTS=4):
        ovr = admm_logit_ridge_ovr(x, labels, GRID).fit()
    assert ovr.classes.tolist() == [-3, 5, 11]
    ref = _fit(x, (labels[:, None] == classes[None, :]).astype(np.float64), GRID, QUANT_SLOTS=4)
    assert ovr.stats["xupdate_variant"] == ref.stats["xupdate_variant"] == 11
    assert ovr.niter.tobytes() == ref.niter.tobytes() and ovr.beta.tobytes() == ref.beta.tobytes()


def test_c_abi_refusals_touch_no_output():
    import torch
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    n, p, k = 64, 3, 5
    rng = np.random.default_rng(5)
    x = np.asfortranarray(rng.standard_normal((n, p)))
    Y = np.asfortranarray((rng.uniform(size=(n, k)) < 0.5).astype(np.float64))
    o = AdmmOpts(100, 1e-4, 1e-4, 1.0)
    good = (2.0, 0.5)

    def call(xptr, yptr, k_, mem, lam=good, nlam=None, beta_null=False, niter_null=False):
        lam = np.asarray(lam, dtype=np.float64)
        beta, niter = np.full((p + 1) * k * 2, 7.0), np.full(k * 2, -5, np.int32)
        rc = lib.admm_hip_logit_ridge(xptr, yptr, n, p, k_, mem, 1, lam.ctypes.data_as(dp), len(lam) if nlam is None else nlam, ctypes.byref(o),
                                      None if beta_null else beta.ctypes.data_as(dp), None if niter_null else niter.ctypes.data_as(ip), None)
        assert np.all(beta == 7.0) and np.all(niter == -5)
        return rc, lib.admm_hip_last_error().decode()

    assert call(x.ctypes.data, Y.ctypes.data, k, 0, lam=(2.0, 0.0)) == (INVALID_ARG, LAMBDA_MSG)
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, lam=(-2.0, 0.5)) == (INVALID_ARG, LAMBDA_MSG)
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, lam=(2.0, np.nan)) == (INVALID_ARG, LAMBDA_MSG)
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, nlam=0) == (INVALID_ARG, "lambda must have at least one value")
    assert call(x.ctypes.data, Y.ctypes.data, 0, 0) == (INVALID_ARG, "y must have at least one column")
    two = Y.copy(order="F")
    two[17, 3] = 2.0
    assert call(x.ctypes.data, two.ctypes.data, k, 0) == (INVALID_ARG, "column 3 of y: every label must be exactly 0 or 1")
    xd = torch.tensor(x.T.copy(), device="cuda")
    nan = Y.copy(order="F")
    nan[5, 1] = np.nan
    nd = torch.tensor(nan.T.copy(), device="cuda")
    ones = Y.copy(order="F")
    ones[:, 2] = 1.0
    od = torch.tensor(ones.T.copy(), device="cuda")
    torch.cuda.synchronize()
    assert call(xd.data_ptr(), nd.data_ptr(), k, 1) == (INVALID_ARG, "column 1 of y: every label must be exactly 0 or 1")
    assert call(xd.data_ptr(), od.data_ptr(), k, 1) == (INVALID_ARG, "column 2 of y must hold both classes")
    assert call(x.ctypes.data, ones.ctypes.data, k, 0) == (INVALID_ARG, "column 2 of y must hold both classes")
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, beta_null=True) == (INVALID_ARG, "output pointers must not be NULL")
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, niter_null=True) == (INVALID_ARG, "output pointers must not be NULL")
    # and the same arguments, valid, go through
    lam = np.asarray(good)
    beta, niter = np.full((p + 1) * k * 2, 7.0), np.full(k * 2, -5, np.int32)
    assert lib.admm_hip_logit_ridge(x.ctypes.data, Y.ctypes.data, n, p, k, 0, 1, lam.ctypes.data_as(dp), 2, ctypes.byref(o), beta.ctypes.data_as(dp),
                                    niter.ctypes.data_as(ip), None) == 0
    assert np.all(np.isfinite(beta)) and np.all(niter > 0)
