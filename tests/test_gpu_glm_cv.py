"""GPU: K-fold cross-validation of the penalised logistic and Poisson fits (admm_hip_logit_enet_cv, admm_hip_poisson_cv) -- the held-out
case of the row prox through the three LAD branches, the fold slots of the grid on ONE setup, the held-out deviance on the device, the
summary tables, explicit folds, repeatability, device-resident input and the refusals.

The masked restatement, the replay, the NumPy deviance and the summary are tests/glm_cv_oracle.py.  Shapes: BRANCHES of
tests/test_gpu_quantreg.py (400 x 8 on the hat branch, 2100 x 40 one-pass and two-pass), 150 x 200 (n < p) and 403 x 8 (403 + 8 rows: the
tag matrix's leading dimension 416 has padding, and three folds of 135, 134, 134 rows).  k = 3 columns, F = 3 folds (row i in fold
i mod 3 unless said), two cells: (0.3 lambda_1, alpha = 1) and (0.1 lambda_1 / 0.5, alpha = 0.5), lambda_1 the largest over the columns.
Logistic labels: the first three columns of logit_multi_oracle.label_matrix (shares of ones 0.5, 0.3, 0.7) on logit_oracle's design;
Poisson counts: the first three columns of poisson_oracle.count_matrix (b0 = 0.7, 0, -2) on poisson_oracle's design.

Bounds: the follow tolerance 1e-8 is the loop's (tests/test_gpu_logit.py); the replay holds the training rows to the loss's prox_tol,
the penalty rows to 4 ulp, every held-out row's z to v BIT FOR BIT and y to the bit.  Between the grid call and its single fits, and
between its f = 0 slot and the public call, the yardstick is numbers (==); between the serial and the slotted route of the same call,
and between two identical calls, it is bytes.  DEV_RTOL = 1e-10: fold_dev against the NumPy float64 deviance from the RETURNED fold_beta
and the caller's x -- the rounding of <= 40-term dot products and <= 700-term sums is about 1e-13, which leaves three orders for the
scale recovery (the device works on the standardised columns and coefficients, NumPy on the caller's); 150 x 200 has 200-term dot
products, five times the rounding, still two orders inside.  SUMMARY_RTOL = 1e-14: cv_mean and cv_se are sums of three numbers."""
import ctypes

import numpy as np
import pytest

import glm_cv_oracle as cvo
import logit_enet_oracle as le
import logit_multi_oracle as lm
import logit_oracle as lo
import poisson_oracle as po
from helpers import dense_state_records
from test_glm_cv_host import CV_REFUSALS, INVALID_ARG, OPTS, _cv_call
from test_gpu_quantreg import BRANCHES

pytestmark = pytest.mark.gpu

K, NFOLDS = 3, 3
DEV_RTOL, SUMMARY_RTOL = 1e-10, 1e-14
LOSSES = ("logit", "poisson")
SHAPES = {"hat": BRANCHES["hat"][:3], "onepass": BRANCHES["onepass"][:3], "wide": (150, 200, 3), "padded": (403, 8, 5)}

_cache = {}


def _problem(loss, n, p, seed):
    """-> (x, Y n x 3, lam (2,), alpha (2,))"""
    key = ("problem", loss, n, p, seed)
    if key not in _cache:
        if loss == "logit":
            x = lo.logit_data(n, p, seed)[0]
            Y = np.asfortranarray(lm.label_matrix(x, seed)[:, :K])
            l1 = float(le.lambda_one(x, Y, True).max())
        else:
            x = po.poisson_data(n, p, seed)[0]
            Y = np.asfortranarray(po.count_matrix(x, seed)[:, :K])
            l1 = float(po.lambda_one(x, Y, True).max())
        _cache[key] = (x, Y, np.array([0.3 * l1, 0.1 * l1 / 0.5]), np.array([1.0, 0.5]))
    return _cache[key]


def _builder(loss, cv):
    import admm_amd as A
    return getattr(A, ("admm_logit_enet" if loss == "logit" else "admm_poisson") + ("_cv" if cv else ""))


def _cv(loss, x, Y, lam, alpha, nfolds=NFOLDS, fold_id=None, **opt):
    from admm_amd import options
    with options(**opt):
        return _builder(loss, True)(x, Y, lam, alpha=alpha, nfolds=nfolds, fold_id=fold_id).fit()


def _one(loss, x, y, lam, alpha, fold, nfolds=NFOLDS, fold_id=None, state=0, **opt):
    from admm_amd import options
    with options(**opt):
        return _builder(loss, True)(x, y, lam, alpha=alpha, nfolds=nfolds, fold_id=fold_id).fit(trace=True, state=state, fold=fold)


def _public(loss, x, Y, lam, alpha, **opt):
    from admm_amd import options
    with options(**opt):
        return _builder(loss, False)(x, Y, lam, alpha=alpha).fit()


def _serial(loss, shape):
    """the grid call of a shape on its serial route (QUANT_SLOTS=1), fitted once"""
    key = ("serial", loss, shape)
    if key not in _cache:
        _cache[key] = _cv(loss, *_problem(loss, *SHAPES[shape]), QUANT_SLOTS=1)
    return _cache[key]


def _tables(fit):
    return b"".join(np.ascontiguousarray(t).tobytes() for t in (fit.beta, fit.niter, fit.cv_mean, fit.cv_se, fit.fold_dev, fit.fold_niter, fit.fold_beta, fit.idx_min, fit.idx_1se))


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_state_form_on_three_branches_against_the_masked_restatement(branch, loss):
    n, p, seed, onepass = BRANCHES[branch]
    x, Y, lam, alpha = _problem(loss, n, p, seed)
    y, fold = np.ascontiguousarray(Y[:, 0]), 1
    held = cvo.fold_ids(n, NFOLDS) == fold
    label = f"{branch} n={n} p={p} fold={fold}"
    fit = _one(loss, x, y, lam[0], alpha[0], fold, state=dense_state_records(n + p, 10000), LAD_ONEPASS=onepass)
    assert fit.stats["xupdate_variant"] == (1 if branch == "onepass" else 0)
    assert fit.beta.shape == (p + 1,) and np.all(np.isfinite(fit.beta))
    cvo.followed(loss, fit.beta, fit.niter, fit.trace, x, y, lam[0], alpha[0], True, OPTS, held, tol=1e-8, label=label)
    assert cvo.replay(loss, fit.trace, fit.state, y, p, lam[0], alpha[0], held, label=label) >= 8
    # record 0: the markers on exactly the fold's rows (replay asserts the whole tag vector)
    assert np.array_equal(np.flatnonzero(fit.state[0, 1] == cvo.HELD[loss]), np.flatnonzero(held))
    # fold = -1 holds out nothing: the public call's _state form, number for number
    none = _one(loss, x, y, lam[0], alpha[0], -1, LAD_ONEPASS=onepass)
    from admm_amd import options
    with options(LAD_ONEPASS=onepass):
        pub = _builder(loss, False)(x, y, lam[0], alpha=alpha[0]).fit(trace=True)
    assert none.niter == pub.niter and np.array_equal(none.beta, pub.beta) and np.array_equal(none.trace, pub.trace)
    assert none.niter != fit.niter or not np.array_equal(none.beta, fit.beta)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape,slots", [("hat", 1), ("onepass", 1), ("onepass", 4), ("wide", 1), ("padded", 1)])
def test_the_full_data_slot_equals_the_public_call(shape, slots, loss):
    x, Y, lam, alpha = _problem(loss, *SHAPES[shape])
    fit = _serial(loss, shape) if slots == 1 else _cv(loss, x, Y, lam, alpha, QUANT_SLOTS=slots)
    pub = _public(loss, x, Y, lam, alpha, QUANT_SLOTS=slots)
    want = 8 + slots if slots > 1 else (1 if shape == "onepass" else 0)
    assert fit.stats["xupdate_variant"] == pub.stats["xupdate_variant"] == want
    assert fit.beta.shape == pub.beta.shape == (x.shape[1] + 1, K, 2)
    assert np.array_equal(fit.niter, pub.niter) and np.array_equal(fit.beta, pub.beta)
    assert np.all(np.isfinite(fit.fold_dev)) and np.all(fit.fold_niter > 0) and int(fit.fold_niter.max()) <= 10000


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", ["onepass", "twopass", "hat", "wide", "padded"])
def test_every_fit_of_the_grid_call_equals_its_single_fit(shape, loss):
    """Every route a fit can take: the rows kernel (one-pass), the two streaming products with the tail kernel (two-pass: LAD_ONEPASS=0 on
    the one-pass shape), and the hat matrix with the tail kernel at 400 x 8, 150 x 200 and 403 x 8."""
    x, Y, lam, alpha = _problem(loss, *SHAPES["onepass" if shape == "twopass" else shape])
    opt = dict(QUANT_SLOTS=1, LAD_ONEPASS="0") if shape == "twopass" else dict(QUANT_SLOTS=1)
    fit = _cv(loss, x, Y, lam, alpha, **opt) if shape == "twopass" else _serial(loss, shape)
    assert fit.stats["xupdate_variant"] == (1 if shape == "onepass" else 0)
    for l in range(2):
        for c in range(K):
            for f in range(-1, NFOLDS):
                one = _one(loss, x, np.ascontiguousarray(Y[:, c]), lam[l], alpha[l], f, **opt)
                beta, niter = (fit.beta[:, c, l], fit.niter[c, l]) if f < 0 else (fit.fold_beta[f, :, c, l], fit.fold_niter[f, c, l])
                assert one.niter == int(niter), (l, c, f, one.niter, int(niter))
                assert np.array_equal(one.beta, beta), (l, c, f)
    print(f"[glm cv {loss} {shape} grid] niter {fit.niter.T.tolist()}, fold_niter {fit.fold_niter.tolist()}")
    # the folds are other problems than the full-data fit, and than each other
    assert len({fit.fold_beta[f].tobytes() for f in range(NFOLDS)} | {fit.beta.tobytes()}) == NFOLDS + 1


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("slots", [2, 3, 4])
def test_slots_are_byte_identical_to_the_serial_route(slots, loss):
    x, Y, lam, alpha = _problem(loss, *SHAPES["onepass"])
    ref = _serial(loss, "onepass")
    fit = _cv(loss, x, Y, lam, alpha, QUANT_SLOTS=slots)
    assert fit.stats["xupdate_variant"] == 8 + slots
    assert _tables(fit) == _tables(ref)


@pytest.mark.parametrize("loss", LOSSES)
def test_held_out_rows_carry_no_loss(loss):
    """The responses of fold f's rows are changed (labels flipped, counts + 3; every training set stays valid: the other folds keep both
    classes / positive counts).  Fold f's fit does not see them -- fold_beta, fold_niter byte-identical -- and its deviance does."""
    x, Y, lam, alpha = _problem(loss, *SHAPES["onepass"])
    ref = _serial(loss, "onepass")
    f = 2
    rows = cvo.fold_ids(x.shape[0], NFOLDS) == f
    Y2 = Y.copy(order="F")
    Y2[rows] = 1.0 - Y[rows] if loss == "logit" else Y[rows] + 3.0
    fit = _cv(loss, x, Y2, lam, alpha, QUANT_SLOTS=1)
    assert fit.fold_beta[f].tobytes() == ref.fold_beta[f].tobytes() and fit.fold_niter[f].tobytes() == ref.fold_niter[f].tobytes()
    assert np.all(fit.fold_dev[f] != ref.fold_dev[f])
    for g in range(NFOLDS):
        if g != f:
            assert fit.fold_beta[g].tobytes() != ref.fold_beta[g].tobytes()
    assert fit.beta.tobytes() != ref.beta.tobytes()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fold_deviance_and_the_summary_against_numpy(shape, loss):
    x, Y, lam, alpha = _problem(loss, *SHAPES[shape])
    fit = _serial(loss, shape)
    fid = cvo.fold_ids(x.shape[0], NFOLDS)
    assert np.array_equal(fit.fold_id, fid)
    want = cvo.fold_deviance(loss, x, Y, fit.fold_beta, fid)
    err = float(np.max(np.abs(fit.fold_dev - want) / np.abs(want)))
    print(f"[glm cv {loss} {shape}] fold_dev against NumPy: relative error {err:.2e} (bound {DEV_RTOL:.0e}); cv_mean {fit.cv_mean.tolist()}")
    assert fit.fold_dev.shape == (NFOLDS, K, 2) and np.all(np.isfinite(fit.fold_dev)) and np.all(fit.fold_dev > 0.0)
    assert err <= DEV_RTOL
    mean, se, imin, i1se = cvo.cv_summary(fit.fold_dev, lam, alpha)
    assert np.allclose(fit.cv_mean, mean, rtol=SUMMARY_RTOL, atol=0) and np.allclose(fit.cv_se, se, rtol=SUMMARY_RTOL, atol=0)
    assert np.array_equal(fit.idx_min, imin) and np.array_equal(fit.idx_1se, i1se)
    assert np.array_equal(fit.lambda_min, lam[imin]) and np.array_equal(fit.lambda_1se, lam[i1se])


@pytest.mark.parametrize("loss", LOSSES)
def test_explicit_folds_against_the_default_on_the_permuted_problem(loss):
    """403 rows in three folds of 135, 134, 134.  The rows are permuted; with fold_id = None the permuted problem puts its row j in fold
    j mod 3, and the explicit, unsorted fold_id[perm[j]] = j mod 3 states the same folds on the original rows.  The two calls sum their
    rows in other orders, so they agree as two roundings of one computation do: niter equal, every table within the loop's 1e-8."""
    x, Y, lam, alpha = _problem(loss, *SHAPES["padded"])
    n = x.shape[0]
    perm = np.random.default_rng(17).permutation(n)
    fid = np.zeros(n, dtype=np.int64)
    fid[perm] = np.arange(n) % NFOLDS
    assert sorted(np.bincount(fid).tolist()) == [134, 134, 135] and np.any(np.diff(fid) < 0)
    a = _cv(loss, x, Y, lam, alpha, fold_id=fid)
    b = _cv(loss, np.ascontiguousarray(x[perm]), np.asfortranarray(Y[perm]), lam, alpha)
    assert np.array_equal(a.fold_id, fid)
    assert np.array_equal(a.niter, b.niter) and np.array_equal(a.fold_niter, b.fold_niter)
    for name in ("beta", "fold_beta", "fold_dev", "cv_mean", "cv_se"):
        u, v = getattr(a, name), getattr(b, name)
        err = float(np.max(np.abs(u - v)) / np.max(np.abs(v)))
        print(f"[glm cv {loss} explicit folds] {name}: {err:.2e}")
        assert err <= 1e-8, name
    assert np.array_equal(a.idx_min, b.idx_min) and np.array_equal(a.idx_1se, b.idx_1se)
    # and the explicit folds are not the default's
    assert _tables(a) != _tables(_serial(loss, "padded"))


@pytest.mark.parametrize("loss", LOSSES)
def test_two_identical_calls_and_device_resident_input_are_byte_identical(loss):
    import torch
    from admm_amd import DevicePtr, options
    x, Y, lam, alpha = _problem(loss, *SHAPES["onepass"])
    n, p = x.shape
    a, b = _cv(loss, x, Y, lam, alpha, QUANT_SLOTS=3), _cv(loss, x, Y, lam, alpha, QUANT_SLOTS=3)
    assert a.stats["xupdate_variant"] == b.stats["xupdate_variant"] == 11
    assert _tables(a) == _tables(b)
    xh = np.asfortranarray(x).T.copy()
    xd = torch.tensor(xh, device="cuda")                                 # p x n row-major == n x p column-major
    yd = torch.tensor(Y.T.copy(), device="cuda")
    torch.cuda.synchronize()
    with options(QUANT_SLOTS=3):
        d = _builder(loss, True)(DevicePtr(xd.data_ptr()), DevicePtr(yd.data_ptr()), lam, alpha=alpha, nfolds=NFOLDS, n=n, p=p, k=K).fit()
    assert _tables(d) == _tables(a)
    assert np.array_equal(yd.cpu().numpy(), Y.T) and np.array_equal(xd.cpu().numpy(), xh)


@pytest.mark.parametrize("pois,over,message", CV_REFUSALS, ids=[f"{i}-{'poisson' if r[0] else 'logit'}-" + ",".join(r[1]) for i, r in enumerate(CV_REFUSALS)])
def test_refusals_touch_no_output(pois, over, message):
    from admm_amd import _lib
    assert _cv_call(_lib.load(), pois, **dict(over)) == (INVALID_ARG, message)


@pytest.mark.parametrize("loss", LOSSES)
def test_device_resident_responses_are_checked_per_fold_and_valid_calls_go_through(loss):
    import torch
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    n, p, k, F = 12, 2, 2, 3
    x = np.asfortranarray(np.arange(2.0 * n).reshape(n, p) % 5 + 0.1 * np.arange(n)[:, None])
    y0 = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0], dtype=np.float64)
    good = np.concatenate([y0, 1.0 - y0]) if loss == "logit" else np.concatenate([y0, 3.0 * (1.0 - y0)])
    bad = good.copy()
    bad[:n] = [0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0]                   # column 0 lives in fold 1 alone
    msg = "column 0 of y lacks a class in the training rows of fold 1" if loss == "logit" else "column 0 of y has a zero sum over the training rows of fold 1"
    fn = lib.admm_hip_logit_enet_cv if loss == "logit" else lib.admm_hip_poisson_cv
    lam, alpha, o = np.array([1.0, 0.5]), np.array([1.0, 0.5]), AdmmOpts(200, 1e-4, 1e-4, 1.0)
    xd = torch.tensor(x.T.copy(), device="cuda")
    torch.cuda.synchronize()

    def call(yv, mem):
        outs = dict(beta=np.full((p + 1) * k * 2, 7.0), niter=np.full(k * 2, -5, np.int32), cv_mean=np.full(k * 2, 7.0), cv_se=np.full(k * 2, 7.0),
                    fold_dev=np.full(F * k * 2, 7.0), fold_niter=np.full(F * k * 2, -5, np.int32), fold_beta=np.full(F * k * 2 * (p + 1), 7.0),
                    idx_min=np.full(k, -5, np.int32), idx_1se=np.full(k, -5, np.int32))
        ptr = {name: a.ctypes.data_as(ip if a.dtype == np.int32 else dp) for name, a in outs.items()}
        yd = torch.tensor(yv, device="cuda")
        torch.cuda.synchronize()
        rc = fn(xd.data_ptr() if mem else x.ctypes.data, yd.data_ptr() if mem else yv.ctypes.data, n, p, k, mem, 1, None, F, lam.ctypes.data_as(dp), alpha.ctypes.data_as(dp), 2,
                ctypes.byref(o), ptr["beta"], ptr["niter"], ptr["cv_mean"], ptr["cv_se"], ptr["fold_dev"], ptr["fold_niter"], ptr["fold_beta"], ptr["idx_min"], ptr["idx_1se"], None)
        return rc, lib.admm_hip_last_error().decode(), outs

    for mem in (0, 1):
        rc, text, outs = call(bad, mem)
        assert (rc, text) == (INVALID_ARG, msg)
        assert all(np.all(a == (7.0 if a.dtype == np.float64 else -5)) for a in outs.values())
    host, dev = call(good, 0), call(good, 1)
    assert host[0] == dev[0] == 0
    for name, a in host[2].items():
        assert np.all(np.isfinite(a)) and a.tobytes() == dev[2][name].tobytes(), name
    assert np.all(host[2]["niter"] > 0) and np.all(host[2]["fold_niter"] > 0) and np.all(host[2]["idx_min"] >= 0) and np.all(host[2]["idx_1se"] < 2)
    # the optional tables may be NULL
    cvm, cvs, beta, niter = np.zeros(k * 2), np.zeros(k * 2), np.zeros((p + 1) * k * 2), np.zeros(k * 2, np.int32)
    assert fn(x.ctypes.data, good.ctypes.data, n, p, k, 0, 1, None, F, lam.ctypes.data_as(dp), alpha.ctypes.data_as(dp), 2, ctypes.byref(o), beta.ctypes.data_as(dp),
              niter.ctypes.data_as(ip), cvm.ctypes.data_as(dp), cvs.ctypes.data_as(dp), None, None, None, None, None, None) == 0
    assert cvm.tobytes() == host[2]["cv_mean"].tobytes() and cvs.tobytes() == host[2]["cv_se"].tobytes() and beta.tobytes() == host[2]["beta"].tobytes()
