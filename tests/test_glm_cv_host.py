"""CPU: K-fold cross-validation of the penalised logistic and Poisson fits (admm_hip_logit_enet_cv, admm_hip_poisson_cv) without a
device -- the masked restatement (tests/glm_cv_oracle.py: LogitEnet / PoisEnet in which a held-out row takes z = v) against the
reference optimum of the TRAINING rows' objective, the NumPy deviance and the summary tables with the one-standard-error rule on
hand-made numbers, the symbols through every layer, what the C ABI refuses before it looks for a device, and the Python builders
against the recording stand-in of tests/test_dense_builders_host.py.

MASKED: three folds (row i in fold i mod 3), the two cells (0.3 lambda_1, alpha = 1) and (0.1 lambda_1 / 0.5, alpha = 0.5) with
lambda_1 the FULL data's, with the intercept, eps_abs = eps_rel = 1e-4, rho = 1.  Logistic: (400, 8, seed 1), (2100, 40, 2), (150, 200,
3) of logit_oracle.logit_data.  Poisson: the same three at b0 = 0.7, and (400, 8, 1) at b0 = 4 and b0 = -2.  48 masked loops, every one
compared with enet_optimum / poisson_optimum of its training rows on the full data's standardised columns (the folds keep the
full-data standardisation and c^2 = n).

Bounds: the sibling tests' own, imported -- logistic EXCESS_CAP = 1e-4 of the optimum, Poisson EXCESS_CAP = 1.57e-5 of the null model's
gap, SUPPORT_SLACK = 1 coefficient.  Measured on exactly these inputs (printed by the test): logistic worst 3.95e-5 (150 x 200), the
support differing in at most 1 coefficient; Poisson worst 3.5e-6, supports identical; 20 - 104 iterations."""
import ctypes
import os
import re

import numpy as np
import pytest

import glm_cv_oracle as cvo
import test_dense_builders_host as tdb
import test_logit_enet_host as tle
import test_poisson_host as tpo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
OPTS = {"maxit": 10000, "eps_abs": 1e-4, "eps_rel": 1e-4, "rho": 1.0}
assert OPTS == tle.OPTS == tpo.OPTS
EXCESS_CAP = {"logit": tle.EXCESS_CAP, "poisson": tpo.EXCESS_CAP}          # imported, not restated
SUPPORT_SLACK = {"logit": tle.SUPPORT_SLACK, "poisson": tpo.SUPPORT_SLACK}
NFOLDS = 3
CELLS = ((1.0, 0.3), (0.5, 0.1))                                           # (alpha, f): lambda = f lambda_1 / alpha
MASKED = ([("logit", n, p, seed, None) for n, p, seed in tle.SHAPES] + [("poisson", n, p, seed, 0.7) for n, p, seed in tpo.SHAPES]
          + [("poisson", 400, 8, 1, 4.0), ("poisson", 400, 8, 1, -2.0)])
SYMBOLS = ("admm_hip_logit_enet_cv", "admm_hip_logit_enet_cv_state", "admm_hip_poisson_cv", "admm_hip_poisson_cv_state")


def masked_problem(loss, n, p, seed, b0):
    """-> (x, y, [(lambda, alpha)] of CELLS with the full data's lambda_1)"""
    if loss == "logit":
        x, y = tle.cell_data(n, p, seed)
        return x, y, [(tle.cell_lambda(n, p, seed, a, f, True), a) for a, f in CELLS]
    x, y = tpo.cell_data(n, p, seed, b0)
    return x, y, [(tpo.cell_lambda(n, p, seed, a, f, True, b0), a) for a, f in CELLS]


def test_symbols_are_declared_exported_bound_and_documented():
    from admm_amd import _lib
    import admm_amd
    header = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    shim = open(os.path.join(ROOT, "integration", "admm_shim.cpp")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"ADMM_HIP_API int " + name + r"\(", header), name
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
        assert "`" + name + "`" in doc, name
        assert "RcppExport SEXP admm_" + name[len("admm_hip_"):] + "(" in shim and "call(" + name + "," in shim
    # the grid form: the public call's arguments, fold_id and nfolds, and the seven tables; the state form: fold_id, nfolds and fold
    assert len(lib.admm_hip_logit_enet_cv.argtypes) == len(lib.admm_hip_logit_enet.argtypes) + 9 == len(lib.admm_hip_poisson_cv.argtypes) == 23
    assert len(lib.admm_hip_logit_enet_cv_state.argtypes) == len(lib.admm_hip_logit_enet_state.argtypes) + 3 == len(lib.admm_hip_poisson_cv_state.argtypes)
    for name in ("admm_logit_enet_cv", "admm_poisson_cv", "ADMM_LogitEnetCV", "ADMM_PoissonCV"):
        assert hasattr(admm_amd, name) and name in admm_amd.__all__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for limit in ("full-data standardisation", "glmnet re-standardises per fold", "streams all n rows", "start cold", "Deviance only", "no observation weights",
                  "no multi-GPU form"):
        assert limit in design, limit
    assert "`admm_hip_logit_enet_cv`" in open(os.path.join(ROOT, "README.md")).read()


@pytest.mark.parametrize("loss,n,p,seed,b0", MASKED, ids=[f"{m[0]}-{m[1]}x{m[2]}" + ("" if m[4] is None else f"-b0={m[4]}") for m in MASKED])
def test_masked_restatement_against_the_training_rows_optimum(loss, n, p, seed, b0):
    """A fold's loop on the full augmented matrix, its held-out rows taking z = v and staying out of the stop thresholds, converges to
    the optimum of the training rows' objective: excess within the sibling EXCESS_CAP, support within SUPPORT_SLACK.  Every figure is
    printed before anything is asserted.  Measured: logistic 400 x 8 1.2e-8 / 0 coefficients, 2100 x 40 1.2e-8 / 0, 150 x 200 3.95e-5 / 1;
    Poisson 5.2e-7, 5.8e-7, 3.0e-7, 2.1e-6 (b0 = 4), 3.5e-6 (b0 = -2), all with identical supports; 20 - 104 iterations.
    (With the held-out rows left IN the thresholds' norms and sqrt(rows) -- the first statement of this loop -- 150 x 200, (0.3 lambda_1,
    alpha = 1), fold 2 stopped after 80 iterations with two coefficients of size 1e-3 on the wrong side of zero; it now runs 104.)"""
    x, y, cells = masked_problem(loss, n, p, seed, b0)
    fid = cvo.fold_ids(n, NFOLDS)
    rows = []
    for lam, alpha in cells:
        for f in range(NFOLDS):
            held = fid == f
            got = cvo.masked_fit(loss, x, y, lam, alpha, True, OPTS, held)
            opt = cvo.training_optimum(loss, x, y, lam, alpha, True, held)
            rows.append((lam, alpha, f, got["niter"], cvo.training_excess(loss, x, got["beta"], lam, alpha, True, opt), tle.support_differences(got["beta"], opt[1]),
                         bool(np.any(got["beta"][1:] != 0.0))))
            print(f"[glm cv masked {loss} n={n} p={p} b0={b0}] lambda {lam:.4g} alpha {alpha} fold {f}: niter {rows[-1][3]}, excess {rows[-1][4]:.2e}, support differs in {rows[-1][5]}")
    print(f"[glm cv masked {loss} n={n} p={p} b0={b0}] worst excess {max(r[4] for r in rows):.2e} (cap {EXCESS_CAP[loss]:.2e}), support differs in at most "
          f"{max(r[5] for r in rows)}, niter {min(r[3] for r in rows)} - {max(r[3] for r in rows)}")
    for lam, alpha, f, niter, excess, diff, any_nonzero in rows:
        assert niter <= OPTS["maxit"], (lam, alpha, f)
        assert -1e-9 <= excess <= EXCESS_CAP[loss], (lam, alpha, f, excess)
        assert diff <= SUPPORT_SLACK[loss], (lam, alpha, f, diff)
        assert any_nonzero


@pytest.mark.parametrize("loss", ["logit", "poisson"])
def test_nothing_held_out_is_the_sibling_restatement(loss):
    """fold = -1: the masked class with an empty mask is LogitEnet / PoisEnet, number for number."""
    import logit_enet_oracle as le
    import poisson_oracle as po
    x, y, cells = masked_problem(loss, 400, 8, 1, None if loss == "logit" else 0.7)
    lam, alpha = cells[1]
    got = cvo.masked_fit(loss, x, y, lam, alpha, True, OPTS, np.zeros(400, dtype=bool))
    ref = (le.logit_enet if loss == "logit" else po.poisson)(x, y, lam, alpha, True, OPTS)
    assert got["niter"] == int(ref["niter"][0, 0]) and np.array_equal(got["beta"], ref["beta"][:, 0, 0])


def test_a_held_out_row_carries_no_loss():
    """Changing the response of held-out rows changes nothing of the masked loop (the tags hide it), for both losses."""
    for loss, b0 in (("logit", None), ("poisson", 0.7)):
        x, y, cells = masked_problem(loss, 400, 8, 1, b0)
        lam, alpha = cells[0]
        held = cvo.fold_ids(400, NFOLDS) == 1
        y2 = y.copy()
        y2[held] = 1.0 - y[held] if loss == "logit" else y[held] + 3.0
        a, b = (cvo.masked_fit(loss, x, yy, lam, alpha, True, OPTS, held) for yy in (y, y2))
        assert a["niter"] == b["niter"] and a["beta"].tobytes() == b["beta"].tobytes()
        assert np.array_equal(cvo.tags_of(loss, y, 8, held), cvo.tags_of(loss, y2, 8, held))


def test_the_deviance_on_hand_made_numbers():
    ln2 = np.log(2.0)
    # binomial: eta = 0 gives 2 ln 2 for either label; a confident right answer tends to 0, a confident wrong one to 2 |eta|
    d = cvo.row_deviance("logit", [0.0, 0.0, 40.0, -40.0, 40.0, -800.0], [0.0, 1.0, 1.0, 0.0, 0.0, 1.0])
    assert np.allclose(d[:2], 2.0 * ln2, rtol=1e-15) and np.all(d[2:4] < 1e-16) and d[4] == 80.0 and d[5] == 1600.0
    eta = np.array([0.3, -1.2])
    assert np.allclose(cvo.row_deviance("logit", eta, [1.0, 0.0]), -2.0 * np.log([1.0 / (1.0 + np.exp(-0.3)), 1.0 - 1.0 / (1.0 + np.exp(1.2))]), rtol=1e-14)
    # Poisson: mu = y gives 0; y = 0 gives 2 mu (0 log 0 = 0); y = 2, mu = 1: 2 (2 ln 2 - 1)
    d = cvo.row_deviance("poisson", [np.log(3.0), 0.5, 0.0], [3.0, 0.0, 2.0])
    assert abs(d[0]) < 1e-14 and d[1] == 2.0 * np.exp(0.5) and np.isclose(d[2], 2.0 * (2.0 * ln2 - 1.0), rtol=1e-15)
    assert not np.isfinite(cvo.row_deviance("poisson", [800.0], [1.0])[0])    # non-finite values are returned, not hidden
    assert np.isinf(cvo.row_deviance("poisson", [800.0], [0.0])[0])
    # the fold means: two folds, one column, one cell, intercept-only coefficients
    x = np.zeros((4, 1))
    fb = np.zeros((2, 2, 1, 1))
    fb[0, 0, 0, 0], fb[1, 0, 0, 0] = np.log(2.0), 0.0
    got = cvo.fold_deviance("poisson", x, np.array([2.0, 0.0, 2.0, 1.0]), fb, np.array([0, 1, 0, 1]))
    assert np.allclose(got[:, 0, 0], [0.0, 0.5 * (2.0 + 0.0)], atol=1e-15)


def test_the_summary_tables_and_the_one_standard_error_rule():
    # three folds, one column, five cells: alpha 1 at lambda 8, 4, 2 and alpha 0.5 at lambda 16, 1
    lam, alpha = [8.0, 4.0, 2.0, 16.0, 1.0], [1.0, 1.0, 1.0, 0.5, 0.5]
    dev = np.array([[[1.30, 1.00, 1.02, 1.01, 2.0]], [[1.50, 1.10, 1.00, 1.02, 2.0]], [[1.40, 0.90, 1.10, 1.03, 2.0]]])
    mean, se, imin, i1se = cvo.cv_summary(dev, lam, alpha)
    assert np.allclose(mean[0], [1.4, 1.0, 1.04, 1.02, 2.0], rtol=1e-15) and imin.tolist() == [1]
    assert np.isclose(se[0, 1], np.std([1.0, 1.1, 0.9], ddof=1) / np.sqrt(3.0), rtol=1e-14) and se[0, 4] == 0.0
    # bound = 1.0 + 0.0577: lambda 8 (1.4) is outside, lambda 16 is inside but has another alpha: the minimum itself
    assert i1se.tolist() == [1]
    dev[:, 0, 0] = [1.00, 1.10, 1.05]                                       # now lambda 8 (mean 1.05) is inside
    assert cvo.cv_summary(dev, lam, alpha)[3].tolist() == [0]
    # ties: the first cell of the smallest mean; two columns are judged apart
    two = np.concatenate([dev, dev[:, :, ::-1]], axis=1)
    two[:, 0, :] = 1.0
    _, _, imin, i1se = cvo.cv_summary(two, lam, alpha)
    assert imin.tolist() == [0, 3] and i1se.tolist() == [0, 3]


# ---- the C ABI: refusals before any device is touched
def _cv_call(lib, pois, **over):
    from admm_amd._lib import AdmmOpts
    n, p, k, ncell, F = 12, 2, 2, 2, 3
    y0 = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0], dtype=np.float64)
    keep = dict(x=np.asfortranarray(np.arange(2.0 * n).reshape(n, p) % 5), y=np.concatenate([y0, 1.0 - y0]) if not pois else np.concatenate([y0, 3.0 * (1.0 - y0)]),
                lam=np.array([1.0, 0.5]), alpha=np.array([1.0, 0.5]), fold_id=(np.arange(n) % F).astype(np.int32))
    for name in ("y", "lam", "fold_id"):
        if name + "_values" in over:
            keep[name] = np.asarray(over.pop(name + "_values"), dtype=keep[name].dtype)
    outs = dict(beta=np.full((p + 1) * k * ncell, 7.0), niter=np.full(k * ncell, -5, np.int32), cv_mean=np.full(k * ncell, 7.0), cv_se=np.full(k * ncell, 7.0),
                fold_dev=np.full(F * k * ncell, 7.0), fold_niter=np.full(F * k * ncell, -5, np.int32), fold_beta=np.full(F * k * ncell * (p + 1), 7.0),
                idx_min=np.full(k, -5, np.int32), idx_1se=np.full(k, -5, np.int32))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    v = dict(n=n, nfolds=F, fold_id=keep["fold_id"].ctypes.data_as(ip), cv_mean=outs["cv_mean"].ctypes.data_as(dp))
    v.update(over)
    o = AdmmOpts(10, 1e-4, 1e-4, 1.0)
    ptr = {name: a.ctypes.data_as(ip if a.dtype == np.int32 else dp) for name, a in outs.items()}
    fn = lib.admm_hip_poisson_cv if pois else lib.admm_hip_logit_enet_cv
    rc = fn(keep["x"].ctypes.data, keep["y"].ctypes.data, v["n"], p, k, 0, 1, v["fold_id"], v["nfolds"], keep["lam"].ctypes.data_as(dp), keep["alpha"].ctypes.data_as(dp), ncell,
            ctypes.byref(o), ptr["beta"], ptr["niter"], v["cv_mean"], ptr["cv_se"], ptr["fold_dev"], ptr["fold_niter"], ptr["fold_beta"], ptr["idx_min"], ptr["idx_1se"], None)
    if rc == INVALID_ARG:                                      # a refused call touches no output
        assert all(np.all(a == (7.0 if a.dtype == np.float64 else -5)) for a in outs.values())
    return rc, lib.admm_hip_last_error().decode()


FOLDS_MSG, ID_MSG, EMPTY_MSG = "nfolds must be within [2, n]", "fold_id entries must be within [0, nfolds)", "every fold needs at least one held-out row"
CV_REFUSALS = [
    (False, dict(nfolds=1), FOLDS_MSG),
    (True, dict(nfolds=0), FOLDS_MSG),
    (False, dict(nfolds=13), FOLDS_MSG),
    (False, dict(fold_id_values=[0, 1, 2, 0, 1, 2, 0, 1, 3, 0, 1, 2]), ID_MSG),
    (True, dict(fold_id_values=[0, 1, 2, 0, 1, 2, 0, -1, 2, 0, 1, 2]), ID_MSG),
    (False, dict(fold_id_values=[0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0]), EMPTY_MSG),
    (True, dict(fold_id_values=[0, 2, 0, 0, 2, 0, 0, 2, 0, 0, 2, 0]), EMPTY_MSG),
    (False, dict(cv_mean=None), "cv_mean and cv_se must not be NULL"),
    # column 0's ones all in fold 1 (rows 1, 4, 7, 10): its training rows hold zeros only
    (False, dict(y_values=[0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0] + [0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0]), "column 0 of y lacks a class in the training rows of fold 1"),
    (False, dict(y_values=[0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0] + [1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1]), "column 1 of y lacks a class in the training rows of fold 1"),
    (True, dict(y_values=[0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0] + [0, 0, 2, 0, 0, 5, 0, 0, 1, 0, 0, 0.5]), "column 1 of y has a zero sum over the training rows of fold 2"),
    (True, dict(lam_values=[1.0, 0.0], n=3), "lambda = 0 needs nrow(x) > ncol(x) + intercept"),                      # the public call's checks come first
    # 5 rows against 2 columns and the intercept pass the public check; fold 0 leaves 2 training rows
    (True, dict(lam_values=[1.0, 0.0], y_values=[1.0] * 24, n=5, nfolds=2, fold_id_values=[0, 1, 0, 1, 0] + [0] * 7),
     "lambda = 0 needs more training rows than ncol(x) + intercept in every fold"),
    (False, dict(lam_values=[1.0, 0.0]), "every lambda must be finite and positive"),
    (False, dict(n=1), "nrow(x) must be at least 2"),
]


@pytest.mark.parametrize("pois,over,message", CV_REFUSALS, ids=[f"{i}-{'poisson' if r[0] else 'logit'}-" + ",".join(r[1]) for i, r in enumerate(CV_REFUSALS)])
def test_bad_cv_calls_are_refused_before_any_device_is_touched(pois, over, message):
    from admm_amd import _lib
    assert _cv_call(_lib.load(), pois, **dict(over)) == (INVALID_ARG, message)


def test_the_state_forms_refuse_a_fold_outside_its_range():
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    x = np.asfortranarray(np.arange(24.0).reshape(12, 2) % 5)
    y = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0], dtype=np.float64)
    beta, niter, o = np.full(3, 7.0), np.full(1, -5, np.int32), AdmmOpts(10, 1e-4, 1e-4, 1.0)
    for fn in (lib.admm_hip_logit_enet_cv_state, lib.admm_hip_poisson_cv_state):
        for fold, nfolds, msg in ((3, 3, "fold must be within [-1, nfolds)"), (-2, 3, "fold must be within [-1, nfolds)"), (0, 1, FOLDS_MSG)):
            rc = fn(x.ctypes.data, y.ctypes.data, 12, 2, 0, 1, None, nfolds, fold, 1.0, 1.0, ctypes.byref(o), beta.ctypes.data_as(dp), niter.ctypes.data_as(ip), None,
                    None, 0, None, None, 0, None)
            assert (rc, lib.admm_hip_last_error().decode()) == (INVALID_ARG, msg) and np.all(beta == 7.0) and niter[0] == -5


# ---- the Python builders against the recording stand-in
CV_SIGNATURES = {
    "admm_hip_logit_enet_cv": "x y n p k mem intercept fold_id nfolds lam alpha count opts beta niter cv_mean cv_se fold_dev fold_niter fold_beta idx_min idx_1se stats",
    "admm_hip_logit_enet_cv_state": f"{tdb._HEAD} intercept fold_id nfolds fold lam alpha {tdb._OUT}{tdb._BOTH}",
}
CV_SIGNATURES["admm_hip_poisson_cv"] = CV_SIGNATURES["admm_hip_logit_enet_cv"]
CV_SIGNATURES["admm_hip_poisson_cv_state"] = CV_SIGNATURES["admm_hip_logit_enet_cv_state"]


@pytest.fixture
def rec(monkeypatch):
    from admm_amd import _lib
    real = _lib.load()
    for name, text in CV_SIGNATURES.items():
        monkeypatch.setitem(tdb.SIGNATURES, name, text.split())
    r = tdb.Recorder(real)
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


@pytest.mark.parametrize("name,ycol", [("logit_enet", "Y"), ("poisson", "counts")])
def test_what_the_cv_builders_send_and_what_fit_returns(rec, name, ycol):
    import admm_amd as A
    from admm_amd import api
    d = tdb.data()
    N, P, K = tdb.N, tdb.P, tdb.K
    build = getattr(A, "admm_" + name + "_cv")
    sym = "admm_hip_" + name + "_cv"
    cls = getattr(api, "ADMM_LogitEnetCV_fit" if name == "logit_enet" else "ADMM_PoissonCV_fit")
    ids = (np.arange(N)[::-1] % 4).astype(np.int64)
    # the grid form with explicit folds
    fit = build(d["x"], d[ycol], [2.0, 0.5], alpha=[1.0, 0.25], nfolds=4, fold_id=ids).opts(maxit=tdb.MAXIT, rho=tdb.RHO).fit()
    assert [s for s, _ in rec.calls] == [sym]
    got = rec.calls[0][1]
    assert (got["n"], got["p"], got["k"], got["mem"], got["intercept"], got["nfolds"], got["count"]) == (N, P, K, 0, 1, 4, 2)
    assert got["lam"] == [2.0, 0.5] and got["alpha"] == [1.0, 0.25] and [got["fold_id"][i] for i in range(N)] == ids.tolist()
    assert got["opts"] == (tdb.MAXIT, 1e-4, 1e-4, tdb.RHO)
    assert type(fit) is cls and isinstance(fit, api.ADMM_LogitEnet_fit)
    assert fit.beta.shape == (P + 1, K, 2) and fit.niter.shape == (K, 2) and fit.niter.dtype == np.int32
    assert fit.cv_mean.shape == fit.cv_se.shape == (K, 2) and fit.fold_dev.shape == fit.fold_niter.shape == (4, K, 2) and fit.fold_beta.shape == (4, P + 1, K, 2)
    assert fit.idx_min.shape == fit.idx_1se.shape == (K,) and fit.idx_min.dtype == np.int32
    assert fit.lambda_min.tolist() == [2.0] * K and fit.lambda_1se.tolist() == [2.0] * K           # zero-filled indices: cell 0
    assert fit.fold_id.tolist() == ids.tolist() and fit.trace is None and fit.state is None
    # fold_id = None goes as NULL; the automatic grid asks for lambda_1 first
    del rec.calls[:]
    fit = build(d["x"], d[ycol], alpha=0.5, nlambda=3, nfolds=5).fit()
    assert [s for s, _ in rec.calls] == ["admm_hip_" + name + "_lambda_max", sym]
    got = rec.calls[1][1]
    top = tdb.LAMBDA_ONE / 0.5
    assert got["fold_id"] is None and got["nfolds"] == 5 and got["count"] == 3
    np.testing.assert_allclose(got["lam"], np.exp(np.linspace(np.log(top), np.log(top * 1e-4), 3)), rtol=1e-15)
    assert fit.fold_id.tolist() == (np.arange(N) % 5).tolist() and fit.fold_dev.shape == (5, K, 3)
    # the state form: one column, one cell, one fold
    del rec.calls[:]
    fit = build(d["x"], d[ycol][:, 0], 0.7, alpha=0.25, nfolds=3).opts(maxit=tdb.MAXIT).fit(trace=True, state=tdb.STATE, fold=2)
    assert [s for s, _ in rec.calls] == [sym + "_state"]
    got = rec.calls[0][1]
    assert (got["n"], got["p"], got["mem"], got["intercept"], got["nfolds"], got["fold"], got["lam"], got["alpha"]) == (N, P, 0, 1, 3, 2, 0.7, 0.25)
    assert got["fold_id"] is None and got["trace_cap"] == tdb.MAXIT + 8 and got["state_cap"] == tdb.STATE
    assert type(fit) is cls and fit.beta.shape == (P + 1,) and type(fit.niter) is int
    assert fit.trace.shape == (0, 12) and fit.state.shape == (0, 5, N + P) and not hasattr(fit, "cv_mean")


def test_cv_builder_argument_checks(rec):
    import admm_amd as A
    d = tdb.data()
    N = tdb.N
    for bad in (1, 0, N + 1):
        with pytest.raises(ValueError, match="nfolds must be within"):
            A.admm_logit_enet_cv(d["x"], d["Y"], 1.0, nfolds=bad)
    with pytest.raises(ValueError, match="fold_id must hold nrow\\(x\\) integers"):
        A.admm_poisson_cv(d["x"], d["counts"], 1.0, nfolds=3, fold_id=np.zeros(N - 1, dtype=int))
    with pytest.raises(ValueError, match="fold_id must hold nrow\\(x\\) integers"):
        A.admm_poisson_cv(d["x"], d["counts"], 1.0, nfolds=3, fold_id=np.zeros(N))
    with pytest.raises(ValueError, match="within \\[0, nfolds\\)"):
        A.admm_logit_enet_cv(d["x"], d["Y"], 1.0, nfolds=3, fold_id=np.arange(N) % 4)
    with pytest.raises(ValueError, match="every fold needs at least one held-out row"):
        A.admm_logit_enet_cv(d["x"], d["Y"], 1.0, nfolds=3, fold_id=np.arange(N) % 2)
    with pytest.raises(ValueError, match="every lambda must be finite and positive"):
        A.admm_logit_enet_cv(d["x"], d["Y"], 0.0)
    m = A.admm_poisson_cv(d["x"], d["counts"], [1.0, 2.0])
    assert isinstance(m, A.ADMM_Poisson) and m.nfolds == 10 and m.fold_id is None
    for kw in (dict(trace=True), dict(state=2)):
        with pytest.raises(ValueError, match="^trace and state are recorded for a single count column and a single cell$"):
            m.fit(**kw)
    one = A.admm_logit_enet_cv(d["x"], d["Y"][:, 0], 1.0, nfolds=3)
    for fold in (3, -2):
        with pytest.raises(ValueError, match="fold must be within"):
            one.fit(trace=True, fold=fold)
    assert rec.calls == []
