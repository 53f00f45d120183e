"""GPU: Poisson regression with the elastic-net penalty (admm_hip_poisson) -- the Newton prox of the Poisson loss on the data rows and the
elastic net's on the penalty rows (kProxPoisE) through the three LAD branches and every register layout of the rows kernels, the
(column, lambda, alpha) grid on ONE inverse, the slotted route with its capture of the last z, and the boundary: the empty model, n < p,
the plain GLM (lambda = 0), sparse and large counts, lambda_1, device-resident input, repeatability, refusals.  The tests mirror
tests/test_gpu_logit_enet.py.

The CPU restatement, the reference optimum and the replay are tests/poisson_oracle.py; the shapes are BRANCHES and LAYOUTS of
tests/test_gpu_quantreg.py, the smallest that reach each branch and each register layout (with the penalty rows 400 x 8 is still the hat
branch, 408 <= 2000, and 2100 x 40 still one-pass / two-pass).  One cell, lambda = 0.3 lambda_1 at alpha = 1, unless said otherwise.

Bounds: the follow tolerance 1e-8 is the loop's (tests/test_gpu_logit.py); EXCESS (tests/test_poisson_host.py: the objective's excess
over the reference optimum as a share of the empty model's) is capped by that file's EXCESS_CAP and the zero pattern may differ from
the optimum's in SUPPORT_SLACK = 1 coefficient; the replay holds the data rows to poisson_oracle.prox_tol, the penalty rows to 4 ulp
of soft(v, t) / d with exact zeros exact, and y to the bit.  Between the grid call and its single fits the yardstick is numbers (== /
array_equal), between the serial and the slotted route of the same call it is bytes.

LAMBDA_ONE_RTOL = 1e-12: lambda_1 is the largest of p dot products over the n rows of O(1) - O(100) entries, in float64 on both sides."""
import ctypes

import numpy as np
import pytest

import poisson_oracle as po
from helpers import dense_state_records
from test_gpu_logit_multi import _npt
from test_gpu_quantreg import BRANCHES, LAYOUTS
from test_poisson_host import (EXCESS_CAP, OPTS, PROX_T, PROX_V, PROX_Y, SUPPORT_SLACK, cell_data, cell_lambda, cell_optimum, excess_of, prox_inputs,
                               support_differences)

pytestmark = pytest.mark.gpu

INVALID_ARG = 1
F = 0.3                                                     # the one cell: lambda = F lambda_1, alpha = 1
MAX_SLOTS = {1: 4, 2: 4, 3: 3, 4: 2, 5: 1, 6: 1}            # kProxKinds[kProxPoisE].max_slots: by the double2 a thread holds per row (profiles/poisson.md)
AUTO_SLOTS = 4                                              # kProxKinds[kProxPoisE].auto_slots: as many as the layout admits (profiles/poisson.md)
LAMBDA_ONE_RTOL = 1e-12

_cache = {}


def _fit(x, Y, lam, alpha=1.0, intercept=True, maxit=10000, trace=False, state=0, **opt):
    from admm_amd import admm_poisson, options
    with options(**opt):
        return admm_poisson(x, Y, lam, alpha=alpha, intercept=intercept).opts(maxit=maxit).fit(trace=trace, state=state)


def problem(n, p, seed):
    """-> (x, Y): the design and its 7 count columns (poisson_oracle.count_matrix)"""
    key = ("problem", n, p, seed)
    if key not in _cache:
        x, _ = cell_data(n, p, seed)
        _cache[key] = (x, po.count_matrix(x, seed))
    return _cache[key]


def _layout_problem(n, p):
    """columns 1 ... 5 of the count matrix (the last two are the same column)"""
    key = ("layout", n, p)
    if key not in _cache:
        x, _ = po.poisson_data(n, p, 100 + p)
        _cache[key] = (x, np.asfortranarray(po.count_matrix(x, 100 + p)[:, 1:6]))
    return _cache[key]


def _grid(x, Y):
    """the issue's cells on the 7-column problem: lambda_1 is the largest over the columns"""
    l1 = float(po.lambda_one(x, Y, True).max())
    return (0.5 * l1, 0.1 * l1, 0.2 * l1, 1.0, 0.5 * l1), (1.0, 1.0, 0.5, 0.0, 1.0)


def _serial(tag, x, Y, lam, alpha, maxit=10000):
    """the call on its serial route (QUANT_SLOTS=1), fitted once per problem"""
    key = ("serial", tag, tuple(np.atleast_1d(lam)), tuple(np.atleast_1d(alpha)), maxit)
    if key not in _cache:
        f = _fit(x, Y, lam, alpha, maxit=maxit, QUANT_SLOTS=1)
        assert f.stats["xupdate_variant"] == 1
        _cache[key] = (f.beta.copy(), f.niter.copy())
    return _cache[key]


@pytest.mark.parametrize("t", PROX_T)
def test_device_prox_against_numpy_and_its_equation(t):
    from admm_amd import _lib
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    v, y = prox_inputs(t)
    v, y = np.ascontiguousarray(v), np.ascontiguousarray(y)
    z = np.full(v.size, np.nan)
    assert lib.admm_hip_test_poisson_prox(v.ctypes.data_as(dp), y.ctypes.data_as(dp), v.size, float(t), z.ctypes.data_as(dp)) == 0
    assert np.all(np.isfinite(z))
    rho = 1.0 / t
    w = v + t * y
    tol = po.prox_tol(v, y, rho)
    rel = np.abs(z - po.prox(v, y, rho)) / tol
    e = t * np.exp(z)
    res = np.abs(z + e - w) / (1.0 + e) / tol
    exact = np.abs(z - po.prox_exact(v, y, rho)) / tol
    print(f"[poisson device prox t={t}] worst |z - numpy| = {float(rel.max()):.2e}, |h| / h' = {float(res.max()):.2e}, |z - bisection| = {float(exact.max()):.2e} "
          f"of the tolerance 1e-13 max(1, |v|, t y, t)")
    assert float(rel.max()) <= 1.0 and float(res.max()) <= 1.0 and float(exact.max()) <= 1.0
    assert np.all(z <= w)
    for k in range(len(PROX_Y)):
        assert np.all(np.diff(z[k * PROX_V.size:k * PROX_V.size + 4001]) >= 0.0)      # non-decreasing in v along the linspace


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_three_branches_against_the_restatement_and_the_reference_optimum(branch, intercept):
    n, p, seed, onepass = BRANCHES[branch]
    x, y = cell_data(n, p, seed)
    lam = cell_lambda(n, p, seed, 1.0, F, intercept)
    label = f"{branch} n={n} p={p} icpt={int(intercept)}"
    fit = _fit(x, y, lam, intercept=intercept, trace=True, state=dense_state_records(n + p, 10000), LAD_ONEPASS=onepass)
    assert fit.stats["xupdate_variant"] == (1 if branch == "onepass" else 0)
    assert fit.beta.shape == (p + 1,) and np.all(np.isfinite(fit.beta))
    po.followed(fit.beta, fit.niter, fit.trace, x, y, lam, 1.0, intercept, OPTS, tol=1e-8, label=label)
    assert po.replay(fit.trace, fit.state, y, p, lam, 1.0, label=label) >= 8
    _, b_opt, best = cell_optimum(n, p, seed, lam, 1.0, intercept)
    excess = excess_of(x, y, fit.beta, lam, 1.0, intercept, best)
    diff = support_differences(fit.beta, b_opt)
    print(f"[poisson {label}] niter {fit.niter}, EXCESS {excess:.2e}, support {int(np.sum(fit.beta[1:] != 0.0))}, {diff} differ")
    assert -1e-9 <= excess <= EXCESS_CAP
    assert diff <= SUPPORT_SLACK
    assert np.any(fit.beta[1:] == 0.0) and np.any(fit.beta[1:] != 0.0)
    if not intercept:
        assert fit.beta[0] == 0.0


@pytest.mark.parametrize("n,p,maxit", LAYOUTS)
def test_every_register_layout_of_the_rows_kernel(n, p, maxit):
    x, y = po.poisson_data(n, p, 100 + p)
    lam = F * float(po.lambda_one(x, y, True)[0])
    label = f"layout n={n} p={p}"
    fit = _fit(x, y, lam, maxit=maxit, trace=True, state=dense_state_records(n + p, maxit))
    assert fit.stats["xupdate_variant"] == 1
    assert np.all(np.isfinite(fit.beta))
    po.followed(fit.beta, fit.niter, fit.trace, x, y, lam, 1.0, True, dict(OPTS, maxit=maxit), tol=1e-8, label=label)
    assert po.replay(fit.trace, fit.state, y, p, lam, 1.0, label=label) >= 8


def test_every_cell_of_the_grid_call_equals_the_single_fit():
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    lam, alpha = _grid(x, Y)
    beta, niter = _serial((n, p, seed), x, Y, lam, alpha)
    assert beta.shape == (p + 1, po.K, len(lam)) and niter.shape == (po.K, len(lam)) and np.all(np.isfinite(beta))
    for l in range(len(lam)):
        for c in range(po.K):
            one = _fit(x, Y[:, c], lam[l], alpha[l], QUANT_SLOTS=1)
            assert one.beta.shape == (p + 1, 1, 1) and one.stats["xupdate_variant"] == 1
            assert int(one.niter[0, 0]) == int(niter[c, l]), (c, l, niter.tolist())
            assert np.array_equal(one.beta[:, 0, 0], beta[:, c, l]), (c, l)
    print(f"[poisson grid] niter {niter.T.tolist()}")
    assert int(niter.max()) <= 10000
    assert beta[:, :, 4].tobytes() == beta[:, :, 0].tobytes() and np.array_equal(niter[:, 4], niter[:, 0])      # the repeated cell
    assert beta[:, 4].tobytes() == beta[:, 5].tobytes() and np.array_equal(niter[4], niter[5])                  # the repeated column
    assert np.any(beta[1:, :, 1] == 0.0) and np.all(beta[1:, :, 3] != 0.0)                                      # a lasso cell has zeros, the ridge cell none


@pytest.mark.parametrize("slots", [2, 3, 4])
def test_slots_are_byte_identical_to_the_serial_route(slots):
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    lam, alpha = _grid(x, Y)
    beta1, niter1 = _serial((n, p, seed), x, Y, lam, alpha)
    fit = _fit(x, Y, lam, alpha, QUANT_SLOTS=slots)
    assert fit.stats["xupdate_variant"] == 8 + slots
    assert fit.lam.tolist() == list(lam) and fit.alpha.tolist() == list(alpha)
    assert fit.niter.tobytes() == niter1.tobytes() and fit.beta.tobytes() == beta1.tobytes()
    assert fit.beta[:, :, 4].tobytes() == fit.beta[:, :, 0].tobytes() and np.array_equal(fit.niter[:, 4], fit.niter[:, 0])      # the cell that is there twice
    assert fit.beta[:, 4].tobytes() == fit.beta[:, 5].tobytes() and np.array_equal(fit.niter[4], fit.niter[5])                  # the column that is there twice
    assert np.any(fit.beta[1:, 0] != 0.0) and np.any(fit.beta[1:, 0] == 0.0)


def test_the_automatic_slot_choice():
    """QUANT_SLOTS unset: kProxPoisE's auto_slots (profiles/poisson.md), clipped to the layout's table and to the number of fits."""
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    lam, alpha = _grid(x, Y)
    beta1, niter1 = _serial((n, p, seed), x, Y, lam, alpha)
    fit = _fit(x, Y, lam, alpha)
    assert fit.stats["xupdate_variant"] == (1 if AUTO_SLOTS == 1 else 8 + min(AUTO_SLOTS, MAX_SLOTS[_npt(p)]))
    assert fit.niter.tobytes() == niter1.tobytes() and fit.beta.tobytes() == beta1.tobytes()
    assert _fit(x, Y[:, 0], lam[0]).stats["xupdate_variant"] == 1                 # one fit: the serial route
    assert _fit(x, Y[:, :2], lam[0], QUANT_SLOTS=4).stats["xupdate_variant"] == 10      # clipped to the number of fits
    # one column and several cells is a grid all the same: the slots refill across cells
    assert _fit(x, Y[:, 0], lam, alpha, QUANT_SLOTS=4).stats["xupdate_variant"] == 12


def _layout_cases():
    for n, p, maxit in LAYOUTS:
        top = MAX_SLOTS[_npt(p)]
        for want in sorted({max(top, 2), 2, 4}, reverse=True):
            yield pytest.param(n, p, maxit, want, id=f"{n}x{p}-slots{want}")


@pytest.mark.parametrize("n,p,maxit,want", list(_layout_cases()))
def test_slots_on_every_register_layout(n, p, maxit, want):
    """Five count columns at one cell.  Asking for more than the kind's max_slots row admits is clipped to it (4 at three double2 per thread and
    row runs 3); five and six double2 leave the form no second slot: serial."""
    x, Y = _layout_problem(n, p)
    lam = F * float(po.lambda_one(x, Y, True).max())
    top = MAX_SLOTS[_npt(p)]
    beta1, niter1 = _serial(("layout", n, p), x, Y, lam, 1.0, maxit=maxit)
    fit = _fit(x, Y, lam, maxit=maxit, QUANT_SLOTS=want)
    assert fit.stats["xupdate_variant"] == (8 + min(want, top) if top >= 2 else 1)
    assert fit.niter.tobytes() == niter1.tobytes() and fit.beta.tobytes() == beta1.tobytes()
    assert np.all(np.isfinite(fit.beta)) and np.any(fit.beta != 0.0)


@pytest.mark.parametrize("slots", [1, 4])
def test_the_empty_model_above_lambda_max(slots):
    """Above lambda_1 / alpha every penalised coefficient is exactly 0.0 and the intercept is log mean(y).  The intercept is held to 1e-6
    on the test data's response (the restatement at eps = 1e-4: 3.6e-10 here, 2.3e-8 at 400 x 8, 3.5e-8 at 150 x 200); what the stop rule
    leaves depends on the column -- the restatement's intercepts of the 7-column problem are 3.6e-10 ... 1.0e-6 off and the sparse
    column's (83 % zeros) 6.1e-5 --, so there the exact zeros are asserted and the intercepts' errors printed."""
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = cell_data(n, p, seed)
    lam = cell_lambda(n, p, seed, 1.0, 1.5, True)
    fit = _fit(x, y, (lam, 2.0 * lam), (1.0, 0.5), QUANT_SLOTS=slots)           # 2 lam at alpha 0.5: 1.5 lambda_1 / alpha there too
    assert fit.stats["xupdate_variant"] == (1 if slots == 1 else 8 + 2)
    err = float(np.max(np.abs(fit.beta[0] - np.log(y.mean()))))
    print(f"[poisson empty slots={slots}] niter {fit.niter.T.tolist()}, intercept off by {err:.2e}")
    assert np.all(fit.beta[1:] == 0.0) and err <= 1e-6
    assert int(fit.niter.max()) <= 10000
    x, Y = problem(n, p, seed)
    lam = 1.5 * float(po.lambda_one(x, Y, True).max())
    fit = _fit(x, Y, (lam, 2.0 * lam), (1.0, 0.5), QUANT_SLOTS=slots)
    assert fit.stats["xupdate_variant"] == (1 if slots == 1 else 8 + slots)
    errs = np.max(np.abs(fit.beta[0] - np.log(Y.mean(axis=0))[:, None]), axis=1)
    print(f"[poisson empty, 7 columns, slots={slots}] niter {fit.niter.T.tolist()}, intercepts off by {[f'{e:.1e}' for e in errs]}")
    assert np.all(fit.beta[1:] == 0.0) and np.all(np.isfinite(fit.beta[0]))
    assert int(fit.niter.max()) <= 10000


@pytest.mark.parametrize("hat", [None, "0"])
def test_more_columns_than_rows(hat):
    """150 x 200: accepted, converges; LAD_HAT=0 sends the 350 augmented rows through the rows kernel."""
    n, p, seed = 150, 200, 3
    x, y = cell_data(n, p, seed)
    lam = cell_lambda(n, p, seed, 1.0, F, True)
    fit = _fit(x, y, lam, LAD_HAT=hat)
    assert fit.stats["xupdate_variant"] == (0 if hat is None else 1)
    beta, niter = fit.beta[:, 0, 0], int(fit.niter[0, 0])
    assert fit.beta.shape == (p + 1, 1, 1) and np.all(np.isfinite(beta))
    _, b_opt, best = cell_optimum(n, p, seed, lam, 1.0, True)
    excess = excess_of(x, y, beta, lam, 1.0, True, best)
    diff = support_differences(beta, b_opt)
    print(f"[poisson 150 x 200 LAD_HAT={hat}] niter {niter}, EXCESS {excess:.2e}, support {int(np.sum(beta[1:] != 0.0))}, {diff} differ")
    assert niter <= 10000
    assert -1e-9 <= excess <= EXCESS_CAP
    assert diff <= SUPPORT_SLACK


@pytest.mark.parametrize("intercept", [True, False])
def test_the_plain_glm_at_lambda_zero(intercept):
    n, p, seed = 400, 8, 1
    x, y = cell_data(n, p, seed)
    fit = _fit(x, y, 0.0, intercept=intercept)
    beta, niter = fit.beta[:, 0, 0], int(fit.niter[0, 0])
    _, b_opt, best = cell_optimum(n, p, seed, 0.0, 1.0, intercept)
    excess = excess_of(x, y, beta, 0.0, 1.0, intercept, best)
    print(f"[poisson lambda=0 icpt={int(intercept)}] niter {niter}, EXCESS {excess:.2e}")
    assert niter <= 10000 and np.all(np.isfinite(beta)) and np.all(beta[1:] != 0.0)
    assert -1e-9 <= excess <= EXCESS_CAP


@pytest.mark.parametrize("b0", [-2.0, 4.0])
def test_sparse_and_large_counts(b0):
    """b0 = -2: about 83 % zeros; b0 = 4: mean count about 68 (the prox sees w up to several hundred)."""
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = cell_data(n, p, seed, b0)
    lam = cell_lambda(n, p, seed, 1.0, F, True, b0)
    fit = _fit(x, y, lam)
    beta, niter = fit.beta[:, 0, 0], int(fit.niter[0, 0])
    _, b_opt, best = cell_optimum(n, p, seed, lam, 1.0, True, b0)
    excess = excess_of(x, y, beta, lam, 1.0, True, best)
    diff = support_differences(beta, b_opt)
    print(f"[poisson b0={b0}] mean count {y.mean():.2f}, niter {niter}, EXCESS {excess:.2e}, support {int(np.sum(beta[1:] != 0.0))}, {diff} differ")
    assert fit.stats["xupdate_variant"] == 1
    assert niter <= 10000 and np.all(np.isfinite(beta))
    assert -1e-9 <= excess <= EXCESS_CAP
    assert diff <= SUPPORT_SLACK


@pytest.mark.parametrize("intercept", [True, False])
def test_lambda_max_against_numpy(intercept):
    from admm_amd import admm_poisson
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    got = admm_poisson(x, Y, 1.0, intercept=intercept).lambda_one()
    want = po.lambda_one(x, Y, intercept)
    err = float(np.max(np.abs(got - want) / want))
    print(f"[poisson lambda_1 icpt={int(intercept)}] {got.tolist()}, relative error {err:.2e}")
    assert got.shape == (po.K,) and err <= LAMBDA_ONE_RTOL
    assert got[4] == got[5]                                          # the column that is there twice
    # the automatic grid starts there
    m = admm_poisson(x, Y[:, :2], alpha=0.5, nlambda=3, lambda_min_ratio=0.1, intercept=intercept)
    lam, alpha = m._cells()
    assert np.allclose(lam, got[:2].max() / 0.5 * np.array([1.0, 0.1 ** 0.5, 0.1]), rtol=1e-12) and alpha.tolist() == [0.5] * 3


def test_device_resident_input_is_byte_identical_and_the_buffers_stay_the_callers():
    import torch
    from admm_amd import DevicePtr, admm_poisson, options
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    lam, alpha = _grid(x, Y)
    a = _fit(x, Y, lam, alpha, QUANT_SLOTS=4)
    xh = np.asfortranarray(x).T.copy()
    xd = torch.tensor(xh, device="cuda")                                 # p x n row-major == n x p column-major
    yd = torch.tensor(Y.T.copy(), device="cuda")                         # k x n row-major == n x k column-major
    torch.cuda.synchronize()
    with options(QUANT_SLOTS=4):
        m = admm_poisson(DevicePtr(xd.data_ptr()), DevicePtr(yd.data_ptr()), lam, alpha=alpha, n=n, p=p, k=po.K)
        d = m.fit()
    assert d.stats["xupdate_variant"] == a.stats["xupdate_variant"] == 12
    assert d.niter.tobytes() == a.niter.tobytes() and d.beta.tobytes() == a.beta.tobytes()
    assert m.lambda_one().tobytes() == admm_poisson(x, Y, lam, alpha=alpha).lambda_one().tobytes()
    assert np.array_equal(yd.cpu().numpy(), Y.T) and np.array_equal(xd.cpu().numpy(), xh)


def test_two_identical_calls_are_byte_identical():
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    lam, alpha = _grid(x, Y)
    a, b = _fit(x, Y, lam, alpha, QUANT_SLOTS=3), _fit(x, Y, lam, alpha, QUANT_SLOTS=3)
    assert a.stats["xupdate_variant"] == b.stats["xupdate_variant"] == 11
    assert a.niter.tobytes() == b.niter.tobytes() and a.beta.tobytes() == b.beta.tobytes()


def test_c_abi_refusals_touch_no_output():
    import torch
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    n, p, k = 64, 3, 5
    rng = np.random.default_rng(5)
    x = np.asfortranarray(rng.standard_normal((n, p)))
    Y = np.asfortranarray(rng.poisson(1.5, size=(n, k)).astype(np.float64))
    o = AdmmOpts(100, 1e-4, 1e-4, 1.0)
    good, good_alpha = (2.0, 0.0), (1.0, 0.5)

    def call(xptr, yptr, k_, mem, lam=good, alpha=good_alpha, ncell=None, n_=n, lam_null=False, alpha_null=False, beta_null=False, niter_null=False):
        lam, alpha = np.asarray(lam, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
        beta, niter = np.full((p + 1) * k * 2, 7.0), np.full(k * 2, -5, np.int32)
        rc = lib.admm_hip_poisson(xptr, yptr, n_, p, k_, mem, 1, None if lam_null else lam.ctypes.data_as(dp), None if alpha_null else alpha.ctypes.data_as(dp),
                                  len(lam) if ncell is None else ncell, ctypes.byref(o),
                                  None if beta_null else beta.ctypes.data_as(dp), None if niter_null else niter.ctypes.data_as(ip), None)
        assert np.all(beta == 7.0) and np.all(niter == -5)
        return rc, lib.admm_hip_last_error().decode()

    lam_msg, alpha_msg = "every lambda must be finite and non-negative", "every alpha must lie in [0, 1]"
    y_msg, sum_msg = "every y must be finite and non-negative", "every column of y must have a positive sum"
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, lam=(-2.0, 0.5)) == (INVALID_ARG, lam_msg)
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, lam=(2.0, np.nan)) == (INVALID_ARG, lam_msg)
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, lam=(np.inf, 1.0)) == (INVALID_ARG, lam_msg)
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, alpha=(1.0, 1.5)) == (INVALID_ARG, alpha_msg)
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, alpha=(-0.5, 1.0)) == (INVALID_ARG, alpha_msg)
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, alpha=(np.nan, 1.0)) == (INVALID_ARG, alpha_msg)
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, lam_null=True) == (INVALID_ARG, "lambda and alpha must not be NULL")
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, alpha_null=True) == (INVALID_ARG, "lambda and alpha must not be NULL")
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, ncell=0) == (INVALID_ARG, "lambda must have at least one value")
    assert call(x.ctypes.data, Y.ctypes.data, 0, 0) == (INVALID_ARG, "y must have at least one column")
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, n_=1) == (INVALID_ARG, "nrow(x) must be at least 2")
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, n_=4) == (INVALID_ARG, "lambda = 0 needs nrow(x) > ncol(x) + intercept")
    neg = Y.copy(order="F")
    neg[17, 3] = -1.0
    assert call(x.ctypes.data, neg.ctypes.data, k, 0) == (INVALID_ARG, y_msg)
    xd = torch.tensor(x.T.copy(), device="cuda")
    nan = Y.copy(order="F")
    nan[5, 1] = np.nan
    nd = torch.tensor(nan.T.copy(), device="cuda")
    ngd = torch.tensor(neg.T.copy(), device="cuda")
    inf = Y.copy(order="F")
    inf[63, 4] = np.inf
    fd = torch.tensor(inf.T.copy(), device="cuda")
    zero = Y.copy(order="F")
    zero[:, 2] = 0.0
    zd = torch.tensor(zero.T.copy(), device="cuda")
    torch.cuda.synchronize()
    assert call(xd.data_ptr(), nd.data_ptr(), k, 1) == (INVALID_ARG, y_msg)
    assert call(xd.data_ptr(), ngd.data_ptr(), k, 1) == (INVALID_ARG, y_msg)
    assert call(xd.data_ptr(), fd.data_ptr(), k, 1) == (INVALID_ARG, y_msg)
    assert call(xd.data_ptr(), zd.data_ptr(), k, 1) == (INVALID_ARG, sum_msg)
    assert call(x.ctypes.data, zero.ctypes.data, k, 0) == (INVALID_ARG, sum_msg)
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, beta_null=True) == (INVALID_ARG, "output pointers must not be NULL")
    assert call(x.ctypes.data, Y.ctypes.data, k, 0, niter_null=True) == (INVALID_ARG, "output pointers must not be NULL")
    # lambda_max: the same count validation on device-resident counts, its output untouched
    out = np.full(k, 7.0)
    assert lib.admm_hip_poisson_lambda_max(xd.data_ptr(), nd.data_ptr(), n, p, k, 1, 1, out.ctypes.data_as(dp)) == INVALID_ARG
    assert lib.admm_hip_last_error().decode() == y_msg and np.all(out == 7.0)
    assert lib.admm_hip_poisson_lambda_max(xd.data_ptr(), zd.data_ptr(), n, p, k, 1, 1, out.ctypes.data_as(dp)) == INVALID_ARG
    assert lib.admm_hip_last_error().decode() == sum_msg and np.all(out == 7.0)
    # and the same arguments, valid (non-integer counts included), go through
    lam, alpha = np.asarray(good), np.asarray(good_alpha)
    half = np.asfortranarray(Y + 0.5)
    beta, niter = np.full((p + 1) * k * 2, 7.0), np.full(k * 2, -5, np.int32)
    assert lib.admm_hip_poisson(x.ctypes.data, half.ctypes.data, n, p, k, 0, 1, lam.ctypes.data_as(dp), alpha.ctypes.data_as(dp), 2, ctypes.byref(o),
                                beta.ctypes.data_as(dp), niter.ctypes.data_as(ip), None) == 0
    assert np.all(np.isfinite(beta)) and np.all(niter > 0)
    assert lib.admm_hip_poisson_lambda_max(x.ctypes.data, Y.ctypes.data, n, p, k, 0, 1, out.ctypes.data_as(dp)) == 0
    assert np.all(out > 0.0) and np.all(np.isfinite(out))
