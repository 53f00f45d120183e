"""GPU: logistic regression for several label columns on one setup (admm_hip_logit_multi) -- the unfolded loop with the sign inside
the prox (kProxLogitS) through the three LAD branches, the slotted route of the one-pass branch on every register layout, and the
boundary: one column, two columns, device-resident input, repeatability, the one-vs-rest helper, refusals.

The yardstick is the call's promise: column k has the niter and the coefficients of admm_logit(x, Y[:, k]) under the same options, as
NUMBERS (`==` / array_equal: rounding is symmetric in sign, so only the sign of an exact zero may differ between the folded and the
unfolded loop).  admm_hip_logit itself is pinned to the NumPy restatement and to IRLS by tests/test_gpu_logit.py; the symmetry
argument is checked on the CPU by tests/test_logit_multi_host.py.  Between the serial and the slotted route of THIS call the code per
column is the same, so there the yardstick is bytes.

The label matrices are tests/logit_multi_oracle.py's (7 columns: four thresholded scores, one column twice, the flip of column 0) on
logit_oracle.logit_data's designs; on the two BRANCHES shapes all columns converge, at five distinct iteration counts (12 ... 30), so the
slots refill at different iterations; on the LAYOUTS shapes nothing converges within the small maxit, so the first slots finish in the
same iteration."""
import ctypes

import numpy as np
import pytest

import logit_multi_oracle as lm
import logit_oracle as lo
from test_gpu_quantreg import BRANCHES, LAYOUTS
from test_logit_multi_host import problem

pytestmark = pytest.mark.gpu

INVALID_ARG = 1
MAX_SLOTS = {1: 4, 2: 4, 3: 4, 4: 2, 5: 1, 6: 1}         # kProxKinds[kProxLogitS].max_slots: by the double2 a thread holds per row

_cache = {}


def _npt(p, intercept=True):
    ldxt = (p + (1 if intercept else 0) + 31) // 32 * 32
    return (ldxt // 2 + 511) // 512


def _multi(x, Y, intercept=True, maxit=10000, **opt):
    from admm_amd import admm_logit_multi, options
    with options(**opt):
        return admm_logit_multi(x, Y, intercept=intercept).opts(maxit=maxit).fit()


def _single(key, x, y, intercept=True, maxit=10000, **opt):
    """admm_logit on one column, fitted once per (key, options)"""
    key = ("single", key, intercept, maxit, tuple(sorted(opt.items())))
    if key not in _cache:
        from admm_amd import admm_logit, options
        with options(**opt):
            f = admm_logit(x, y, intercept=intercept).opts(maxit=maxit).fit()
        _cache[key] = (f.beta.copy(), int(f.niter), f.stats["xupdate_variant"])
    return _cache[key]


def _serial(tag, x, Y, maxit=10000):
    """the multi call on its serial route (QUANT_SLOTS=1), fitted once per problem"""
    key = ("serial", tag, maxit)
    if key not in _cache:
        f = _multi(x, Y, maxit=maxit, QUANT_SLOTS=1)
        assert f.stats["xupdate_variant"] == 1
        _cache[key] = (f.beta.copy(), f.niter.copy())
    return _cache[key]


def _layout_problem(n, p):
    """Columns 1 ... 5 of the label matrix (the last two are the same column).  With the NumPy restatement none of them converges within
    the layout's maxit (niter = maxit + 1 on all five shapes); column 0, the balanced one, would at 2600 x 1100 (43 < 61) and is left out."""
    key = ("layout", n, p)
    if key not in _cache:
        x, _ = lo.logit_data(n, p, 100 + p)
        _cache[key] = (x, np.asfortranarray(lm.label_matrix(x, 100 + p)[:, 1:6]))
    return _cache[key]


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_every_column_equals_the_single_fit_on_the_three_branches(branch, intercept):
    n, p, seed, onepass = BRANCHES[branch]
    x, Y = problem(n, p, seed)
    fit = _multi(x, Y, intercept=intercept, QUANT_SLOTS=4, LAD_ONEPASS=onepass)
    assert fit.beta.shape == (p + 1, lm.K) and fit.niter.shape == (lm.K,) and np.all(np.isfinite(fit.beta))
    assert fit.stats["xupdate_variant"] == (8 + min(4, MAX_SLOTS[_npt(p, intercept)]) if branch == "onepass" else 0)
    for c in range(lm.K):
        beta, niter, variant = _single((n, p, seed, Y[:, c].tobytes()), x, Y[:, c], intercept=intercept, LAD_ONEPASS=onepass)
        assert variant == (1 if branch == "onepass" else 0)
        assert int(fit.niter[c]) == niter, (branch, c, fit.niter.tolist())
        assert np.array_equal(fit.beta[:, c], beta), (branch, c, float(np.max(np.abs(fit.beta[:, c] - beta))))
    print(f"[logit multi {branch} icpt={int(intercept)}] niter {fit.niter.tolist()}")
    assert len(set(fit.niter.tolist())) >= 3 and int(fit.niter.max()) < 10000
    if not intercept:
        assert not np.any(fit.beta[0])


@pytest.mark.parametrize("slots", [2, 3, 4])
def test_slots_are_byte_identical_to_the_serial_route(slots):
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    beta1, niter1 = _serial((n, p, seed), x, Y)
    fit = _multi(x, Y, QUANT_SLOTS=slots)
    assert fit.stats["xupdate_variant"] == 8 + slots
    assert fit.niter.tobytes() == niter1.tobytes() and fit.beta.tobytes() == beta1.tobytes()
    assert fit.beta[:, 4].tobytes() == fit.beta[:, 5].tobytes() and fit.niter[4] == fit.niter[5]      # the column that is there twice
    assert np.array_equal(fit.beta[:, 6], -fit.beta[:, 0]) and fit.niter[6] == fit.niter[0]            # the flipped column
    assert np.any(fit.beta[:, 0] != 0.0)


def _layout_cases():
    for n, p, maxit in LAYOUTS:
        top = MAX_SLOTS[_npt(p)]
        for want in sorted({max(top, 2), 2}, reverse=True):
            yield pytest.param(n, p, maxit, want, id=f"{n}x{p}-slots{want}")


@pytest.mark.parametrize("n,p,maxit,want", list(_layout_cases()))
def test_slots_on_every_register_layout(n, p, maxit, want):
    """Five columns, nothing converges within the small maxit: the first slots finish in the same iteration (two refill at once, or one
    refills and the others go idle).  Five and six double2 per thread and row leave the logit form no second slot: serial."""
    x, Y = _layout_problem(n, p)
    top = MAX_SLOTS[_npt(p)]
    beta1, niter1 = _serial(("layout", n, p), x, Y, maxit=maxit)
    assert niter1.tolist() == [maxit + 1] * 5
    fit = _multi(x, Y, maxit=maxit, QUANT_SLOTS=want)
    assert fit.stats["xupdate_variant"] == (8 + min(want, top) if top >= 2 else 1)
    assert fit.niter.tobytes() == niter1.tobytes() and fit.beta.tobytes() == beta1.tobytes()
    assert np.all(np.isfinite(fit.beta))


def test_one_column_and_two_columns():
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    one = _multi(x, Y[:, 1], QUANT_SLOTS=4)
    assert one.stats["xupdate_variant"] == 1                      # a single column runs the serial route
    beta, niter, _ = _single((n, p, seed, Y[:, 1].tobytes()), x, Y[:, 1])
    assert one.beta.shape == (p + 1, 1) and int(one.niter[0]) == niter and np.array_equal(one.beta[:, 0], beta)
    two = _multi(x, Y[:, [3, 1]], QUANT_SLOTS=4)
    assert two.stats["xupdate_variant"] == 10                     # two columns: two slots
    assert int(two.niter[1]) == niter and np.array_equal(two.beta[:, 1], beta)


def test_automatic_takes_as_many_slots_as_the_layout_admits():
    """QUANT_SLOTS unset: the measured choice (profiles/logit_multi.md), clipped to the number of columns."""
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    beta1, niter1 = _serial((n, p, seed), x, Y)
    fit = _multi(x, Y)
    assert fit.stats["xupdate_variant"] == 12
    assert fit.niter.tobytes() == niter1.tobytes() and fit.beta.tobytes() == beta1.tobytes()
    assert _multi(x, Y[:, :3]).stats["xupdate_variant"] == 11


def test_device_resident_input_is_byte_identical_and_the_labels_stay_the_callers():
    import torch
    from admm_amd import DevicePtr, admm_logit_multi, options
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    a = _multi(x, Y, QUANT_SLOTS=4)
    xd = torch.tensor(np.asfortranarray(x).T.copy(), device="cuda")      # p x n row-major == n x p column-major
    yd = torch.tensor(Y.T.copy(), device="cuda")                         # k x n row-major == n x k column-major
    torch.cuda.synchronize()
    with options(QUANT_SLOTS=4):
        d = admm_logit_multi(DevicePtr(xd.data_ptr()), DevicePtr(yd.data_ptr()), n=n, p=p, k=lm.K).fit()
    assert d.stats["xupdate_variant"] == a.stats["xupdate_variant"] == 12
    assert d.niter.tobytes() == a.niter.tobytes() and d.beta.tobytes() == a.beta.tobytes()
    assert np.array_equal(yd.cpu().numpy(), Y.T)


def test_two_identical_calls_are_byte_identical():
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    a, b = _multi(x, Y, QUANT_SLOTS=3), _multi(x, Y, QUANT_SLOTS=3)
    assert a.stats["xupdate_variant"] == b.stats["xupdate_variant"] == 11
    assert a.niter.tobytes() == b.niter.tobytes() and a.beta.tobytes() == b.beta.tobytes()


def test_one_vs_rest_is_the_multi_call_on_the_indicator_matrix():
    from admm_amd import admm_logit_ovr, options
    n, p, seed, _ = BRANCHES["onepass"]
    x, Y = problem(n, p, seed)
    labels = np.where(Y[:, 1] == 1.0, 5, np.where(Y[:, 2] == 1.0, 11, -3))      # three classes, all populated
    classes = np.array([-3, 5, 11])
    assert np.all(np.bincount(np.searchsorted(classes, labels)) > 0)
    with options(QUANT_SLOTS=4):
        ovr = admm_logit_ovr(x, labels).fit()
    assert ovr.classes.tolist() == [-3, 5, 11]
    ref = _multi(x, (labels[:, None] == classes[None, :]).astype(np.float64), QUANT_SLOTS=4)
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

    def call(xptr, yptr, n_, k_, mem, beta_null=False):
        beta, niter = np.full((p + 1) * k, 7.0), np.full(k, -5, np.int32)
        rc = lib.admm_hip_logit_multi(xptr, yptr, n_, p, k_, mem, 1, ctypes.byref(o), None if beta_null else beta.ctypes.data_as(dp),
                                      niter.ctypes.data_as(ip), None)
        assert np.all(beta == 7.0) and np.all(niter == -5)
        return rc, lib.admm_hip_last_error().decode()

    two = Y.copy(order="F")
    two[17, 3] = 2.0
    assert call(x.ctypes.data, two.ctypes.data, n, k, 0) == (INVALID_ARG, "column 3 of y: every label must be exactly 0 or 1")
    xd = torch.tensor(x.T.copy(), device="cuda")
    nan = Y.copy(order="F")
    nan[5, 1] = np.nan
    nd = torch.tensor(nan.T.copy(), device="cuda")
    ones = Y.copy(order="F")
    ones[:, 2] = 1.0
    od = torch.tensor(ones.T.copy(), device="cuda")
    torch.cuda.synchronize()
    assert call(xd.data_ptr(), nd.data_ptr(), n, k, 1) == (INVALID_ARG, "column 1 of y: every label must be exactly 0 or 1")
    assert call(xd.data_ptr(), od.data_ptr(), n, k, 1) == (INVALID_ARG, "column 2 of y must hold both classes")
    assert call(x.ctypes.data, ones.ctypes.data, n, k, 0) == (INVALID_ARG, "column 2 of y must hold both classes")
    assert call(x.ctypes.data, Y.ctypes.data, n, 0, 0) == (INVALID_ARG, "y must have at least one column")
    assert call(x.ctypes.data, Y.ctypes.data, p + 1, k, 0) == (INVALID_ARG, "nrow(x) must be greater than ncol(x) + 1 (the intercept is fitted)")
    assert call(x.ctypes.data, Y.ctypes.data, n, k, 0, beta_null=True) == (INVALID_ARG, "output pointers must not be NULL")
    # and the same arguments, valid, go through
    beta, niter = np.full((p + 1) * k, 7.0), np.full(k, -5, np.int32)
    assert lib.admm_hip_logit_multi(x.ctypes.data, Y.ctypes.data, n, p, k, 0, 1, ctypes.byref(o), beta.ctypes.data_as(dp), niter.ctypes.data_as(ip), None) == 0
    assert np.all(np.isfinite(beta)) and np.all(niter > 0)
