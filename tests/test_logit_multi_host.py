"""CPU: logistic regression for several label columns on one setup (admm_hip_logit_multi) without a device -- the symmetry argument
the call rests on, the label matrices the GPU tests use, the one-vs-rest helper, the symbol through every layer and what the C ABI
refuses before it looks for a device.

The symmetry: admm_hip_logit_multi runs the UNFOLDED loop (the matrix [X_std | 1], the label's sign inside the prox) and promises
column k = admm_hip_logit on column k, which runs the folded one (X~ = diag(s) [X_std | 1]).  tests/logit_multi_oracle.py restates the
unfolded loop in NumPy from logit_oracle's prox and the oracle's control; here every iterate (times s), every decision record, niter
and the coefficients must be array_equal to logit_oracle.logit's, on the hat-matrix shape and the general one.

The label matrices (logit_multi_oracle.label_matrix on logit_oracle.logit_data's designs, seeds 1 and 2): niter of the restatement,
eps 1e-4, rho 1, intercept fitted --
    (400, 8):    13 17 16 21 17 17 13
    (2100, 40):  12 18 17 30 15 15 12
all far below maxit = 10000 and five distinct values each, so the slots of the GPU tests refill at different iterations."""
import ctypes
import os
import re

import numpy as np
import pytest

import logit_multi_oracle as lm
import logit_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
SHAPES = [(400, 8, 1), (2100, 40, 2)]                 # test_gpu_quantreg.BRANCHES: the hat-matrix shape and the general one
OPTS = {"maxit": 10000, "eps_abs": 1e-4, "eps_rel": 1e-4, "rho": 1.0}
NITER = {(400, 8, 1): [13, 17, 16, 21, 17, 17, 13], (2100, 40, 2): [12, 18, 17, 30, 15, 15, 12]}

_cache = {}


def problem(n, p, seed):
    """-> (x, Y): the design and its 7 label columns, shared with tests/test_gpu_logit_multi.py"""
    key = (n, p, seed)
    if key not in _cache:
        x, _ = lo.logit_data(n, p, seed)
        _cache[key] = (x, lm.label_matrix(x, seed))
    return _cache[key]


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("n,p,seed", SHAPES)
def test_the_unfolded_loop_is_the_folded_one_number_for_number(n, p, seed, intercept):
    x, Y = problem(n, p, seed)
    details = [{"trace": [], "state": []} for _ in range(lm.K)]
    multi = lm.logit_multi(x, Y, intercept, OPTS, details)
    assert multi["beta"].shape == (p + 1, lm.K)
    for c in range(lm.K):
        d = {"trace": [], "state": []}
        one = lo.logit(x, Y[:, c], intercept, OPTS, d)
        s = 2.0 * Y[:, c] - 1.0
        assert int(multi["niter"][c]) == int(one["niter"]), c
        assert np.array_equal(multi["beta"][:, c], one["beta"]), c
        assert np.array_equal(np.asarray(details[c]["trace"]), np.asarray(d["trace"])), c          # every decision
        folded = np.asarray(d["state"]).reshape(len(d["state"]), 5, n)                               # x | z | y | adj_z | adj_y
        unfolded = np.asarray(details[c]["state"]).reshape(len(details[c]["state"]), 5, n)
        assert len(folded) >= 8 and np.array_equal(unfolded, folded * s), c                          # every iterate, times the sign


@pytest.mark.parametrize("n,p,seed", SHAPES)
def test_the_label_matrices_converge_at_different_iterations(n, p, seed):
    x, Y = problem(n, p, seed)
    assert Y.shape == (n, lm.K) and Y.flags.f_contiguous and np.all((Y == 0.0) | (Y == 1.0))
    assert np.all(Y.sum(axis=0) > 0) and np.all(Y.sum(axis=0) < n)
    assert np.array_equal(Y[:, 4], Y[:, 5]) and np.array_equal(Y[:, 6], 1.0 - Y[:, 0])
    assert len({Y[:, c].tobytes() for c in range(lm.K)}) == lm.K - 1                                  # nothing else coincides
    niter = lm.logit_multi(x, Y, True, OPTS)["niter"]
    print(f"[logit multi labels n={n} p={p}] ones {Y.mean(axis=0).round(2).tolist()}, niter {niter.tolist()}")
    assert niter.tolist() == NITER[(n, p, seed)]
    assert np.all(niter < 10000) and len(set(niter.tolist())) >= 3
    assert niter[4] == niter[5] and niter[6] == niter[0]


class _StubLib:
    """Stands in for the shared library: records the call of admm_hip_logit_multi and fills recognisable outputs."""

    def __init__(self):
        self.calls = []

    def admm_hip_logit_multi(self, xp, yp, n, p, k, mem, intercept, opts, beta, niter, stats):
        Y = np.ctypeslib.as_array((ctypes.c_double * (n * k)).from_address(yp.value)).reshape((n, k), order="F").copy()
        self.calls.append(dict(n=n, p=p, k=k, mem=mem, intercept=intercept, Y=Y))
        for i in range((p + 1) * k):
            beta[i] = float(i)
        for c in range(k):
            niter[c] = 10 + c
        return 0


def test_one_vs_rest_sorts_the_classes_and_builds_the_indicator_matrix(monkeypatch):
    from admm_amd import admm_logit_multi, admm_logit_ovr, api
    rng = np.random.default_rng(3)
    n, p = 40, 3
    x = rng.standard_normal((n, p))
    labels = rng.permutation(np.repeat([7, -2, 30], [15, 12, 13]))
    stub = _StubLib()
    monkeypatch.setattr(api._lib, "load", lambda: stub)
    model = admm_logit_ovr(x, labels, intercept=False).opts(maxit=50)
    assert model.classes.tolist() == [-2, 7, 30] and model.k == 3 and model.intercept is False and model.maxit == 50
    fit = model.fit()
    call, = stub.calls
    assert (call["n"], call["p"], call["k"], call["mem"], call["intercept"]) == (n, p, 3, 0, 0)
    for c, cls in enumerate([-2, 7, 30]):
        assert np.array_equal(call["Y"][:, c], (labels == cls).astype(np.float64))
    assert fit.classes.tolist() == [-2, 7, 30]
    assert fit.beta.shape == (p + 1, 3) and fit.beta[1, 2] == 2.0 * (p + 1) + 1.0                     # column-major, as the C ABI writes it
    assert fit.niter.tolist() == [10, 11, 12]
    # the same call through the matrix builder
    admm_logit_multi(x, call["Y"], intercept=False).fit()
    assert np.array_equal(stub.calls[1]["Y"], call["Y"]) and stub.calls[1]["k"] == 3
    # float labels that are whole numbers are integers; two classes are enough
    assert admm_logit_ovr(x, np.where(labels == 7, 1.0, 0.0)).classes.tolist() == [0, 1]
    with pytest.raises(ValueError, match="at least two classes"):
        admm_logit_ovr(x, np.full(n, 4))
    with pytest.raises(ValueError, match="labels must be integers"):
        admm_logit_ovr(x, labels + 0.5)
    with pytest.raises(ValueError, match="nrow\\(x\\) should be equal to length\\(y\\)"):
        admm_logit_ovr(x, labels[:-1])
    assert len(stub.calls) == 2                                                                       # a refusal calls nothing


def test_the_matrix_builder_checks_its_arguments():
    from admm_amd import admm_logit_multi
    rng = np.random.default_rng(4)
    x = rng.standard_normal((30, 4))
    Y = (rng.uniform(size=(30, 5)) < 0.5).astype(np.float64)
    m = admm_logit_multi(x, Y)
    assert (m.n, m.p, m.k, m.intercept, m.maxit, m.eps_abs, m.eps_rel, m.rho) == (30, 4, 5, True, 10000, 1e-4, 1e-4, 1.0)
    assert admm_logit_multi(x, Y[:, 0]).k == 1                                                         # a vector is one column
    bad = Y.copy()
    bad[3, 2] = 0.5
    with pytest.raises(ValueError, match="column 2 of y: every label must be exactly 0 or 1"):
        admm_logit_multi(x, bad)
    bad = Y.copy()
    bad[:, 4] = 1.0
    bad[:, 1] = 0.0
    with pytest.raises(ValueError, match="column 1 of y must hold both classes"):
        admm_logit_multi(x, bad)
    with pytest.raises(ValueError, match="y must have at least one column"):
        admm_logit_multi(x, Y[:, :0])
    with pytest.raises(ValueError, match="nrow\\(x\\) must be greater than ncol\\(x\\) \\+ 1"):
        admm_logit_multi(x[:5], Y[:5])
    with pytest.raises(ValueError, match="nrow\\(x\\) should be equal to length\\(y\\)"):
        admm_logit_multi(x, Y[:-1])


def test_the_header_the_loader_and_the_shim_agree_on_the_signature():
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts, AdmmStats
    header = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    m = re.search(r"ADMM_HIP_API int admm_hip_logit_multi\((.*?)\);", header, flags=re.S)
    assert m, "admm_hip_logit_multi is not declared"
    params = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert params == ["const double* x", "const double* y", "int n", "int p", "int k", "int mem", "int intercept", "const admm_opts* opts",
                      "double* beta_out", "int* niter_out", "admm_stats* stats"]
    assert "admm_hip_logit_multi" in _lib.EXPORTS
    lib = _lib.load()
    V, I = ctypes.c_void_p, ctypes.c_int
    assert list(lib.admm_hip_logit_multi.argtypes) == [V, V, I, I, I, I, I, ctypes.POINTER(AdmmOpts), ctypes.POINTER(ctypes.c_double),
                                                       ctypes.POINTER(ctypes.c_int), ctypes.POINTER(AdmmStats)]
    assert lib.admm_hip_logit_multi.restype is ctypes.c_int
    shim = open(os.path.join(ROOT, "integration", "admm_shim.cpp")).read()
    body = shim[shim.index("RcppExport SEXP admm_logit_multi(SEXP x_, SEXP y_, SEXP intercept_, SEXP opts_)"):]
    body = body[:body.index("END_RCPP")]
    call = re.search(r"admm_hip_logit_multi\((.*?)\)\);", body, flags=re.S).group(1)
    assert len(re.split(r",(?![^()]*\))", call)) == len(params)
    assert "x.nrow(), x.ncol(), y.ncol(), ADMM_MEM_HOST" in call
    assert "`admm_hip_logit_multi`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for src in ("api.hip", "calls.h", "calls.hip", "solvers.h"):
        text = open(os.path.join(ROOT, "admm_amd", "csrc", src)).read()
        assert ("solve_logit_multi(" if src == "solvers.h" else "logit_multi(") in text, src


def test_c_abi_refusals_before_any_device_touch_no_output():
    """Host labels are validated on the host, ahead of the device: these refusals are the same with and without a GPU."""
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    n, p, k = 64, 3, 5
    rng = np.random.default_rng(5)
    x = np.asfortranarray(rng.standard_normal((n, p)))
    Y = np.asfortranarray((rng.uniform(size=(n, k)) < 0.5).astype(np.float64))
    o = AdmmOpts(100, 1e-4, 1e-4, 1.0)

    def call(Y_, n_, k_, beta_null=False):
        beta, niter = np.full((p + 1) * k, 7.0), np.full(k, -5, np.int32)
        rc = lib.admm_hip_logit_multi(x.ctypes.data, Y_.ctypes.data, n_, p, k_, 0, 1, ctypes.byref(o), None if beta_null else beta.ctypes.data_as(dp),
                                      niter.ctypes.data_as(ip), None)
        assert np.all(beta == 7.0) and np.all(niter == -5)
        return rc, lib.admm_hip_last_error().decode()

    bad = Y.copy(order="F")
    bad[17, 3] = 2.0
    bad[2, 4] = np.nan                                           # a later column: the first offender is named
    assert call(bad, n, k) == (INVALID_ARG, "column 3 of y: every label must be exactly 0 or 1")
    ones = Y.copy(order="F")
    ones[:, 2] = 1.0
    assert call(ones, n, k) == (INVALID_ARG, "column 2 of y must hold both classes")
    assert call(Y, n, 0) == (INVALID_ARG, "y must have at least one column")
    assert call(Y, p + 1, k) == (INVALID_ARG, "nrow(x) must be greater than ncol(x) + 1 (the intercept is fitted)")
    assert call(Y, n, k, beta_null=True) == (INVALID_ARG, "output pointers must not be NULL")
