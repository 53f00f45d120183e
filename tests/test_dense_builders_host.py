"""CPU: what the dense builders (admm_bp, admm_lad and the losses on LAD's loop) send to libadmm_hip.so and what their fit() returns,
without a device.  admm_amd._lib.load is replaced by a stand-in whose every symbol records (symbol, arguments) and returns 0; a
*_lambda_max stand-in also writes LAMBDA_ONE into its k outputs, so the automatic lambda grid is finite.  Every recorded call must
pass the argument types of the real library (loaded once, before the patch), and fit() runs to its end on the zero-filled buffers.

SIGNATURES names the parameters of every symbol the builders may call, in the order of include/admm_hip.h; CASES states per builder
and form (the grid form, and trace=True with state=STATE where there is one) the symbols called, the values at the named positions
and the shape of what comes back.  Data: n = 30, p = 4, k = 3 (admm_bp: the transposed shape, 4 x 30), seed 11; .opts(maxit=7, rho=2.0)."""
import ctypes

import numpy as np
import pytest

N, P, K = 30, 4, 3
MAXIT, RHO, STATE = 7, 2.0, 2
LAMBDA_ONE = 8.0
GRID_NAMES = ("tau", "delta", "lam", "alpha")

_HEAD, _OUT = "x y n p mem", "opts beta niter stats"
_TRACE, _BOTH = " trace trace_cap ntrace", " trace trace_cap ntrace state state_cap nstate"
SIGNATURES = {name: text.split() for name, text in {
    "admm_hip_bp_state": f"{_HEAD} {_OUT}{_BOTH}",
    "admm_hip_parbp_traced": f"{_HEAD} nthread {_OUT}{_TRACE}",
    "admm_hip_lad_state": f"{_HEAD} intercept {_OUT}{_BOTH}",
    "admm_hip_quantreg": f"{_HEAD} intercept tau count {_OUT}",
    "admm_hip_quantreg_state": f"{_HEAD} intercept tau {_OUT}{_BOTH}",
    "admm_hip_huber": f"{_HEAD} intercept delta tau count {_OUT}",
    "admm_hip_huber_state": f"{_HEAD} intercept delta tau {_OUT}{_BOTH}",
    "admm_hip_logit": f"{_HEAD} intercept {_OUT}",
    "admm_hip_logit_state": f"{_HEAD} intercept {_OUT}{_BOTH}",
    "admm_hip_logit_multi": f"x y n p k mem intercept {_OUT}",
    "admm_hip_logit_ridge": f"x y n p k mem intercept lam count {_OUT}",
    "admm_hip_logit_ridge_state": f"{_HEAD} intercept lam {_OUT}{_BOTH}",
    "admm_hip_logit_enet": f"x y n p k mem intercept lam alpha count {_OUT}",
    "admm_hip_logit_enet_lambda_max": "x y n p k mem intercept out",
    "admm_hip_logit_enet_state": f"{_HEAD} intercept lam alpha {_OUT}{_BOTH}",
    "admm_hip_poisson": f"x y n p k mem intercept lam alpha count {_OUT}",
    "admm_hip_poisson_lambda_max": "x y n p k mem intercept out",
    "admm_hip_poisson_state": f"{_HEAD} intercept lam alpha {_OUT}{_BOTH}",
}.items()}


class Recorder:
    """The stand-in library: getattr gives a function that checks its arguments against the real symbol's types, records the call as
    {parameter name: value} (what a pointer argument points to is read NOW, while the caller's buffers live) and returns 0."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, symbol):
        names, types = SIGNATURES[symbol], getattr(self.real, symbol).argtypes

        def call(*args):
            assert len(args) == len(types) == len(names), (symbol, len(args), len(types))
            for i, (t, a) in enumerate(zip(types, args)):
                t.from_param(a)                                  # raises where ctypes would refuse the argument
            got = dict(zip(names, args))
            count = got.get("count", 1)
            for g in GRID_NAMES:
                if g in got and not isinstance(got[g], float):
                    got[g] = [got[g][i] for i in range(count)]
            o = got["opts"]._obj if "opts" in got else None
            got["opts"] = None if o is None else (o.maxit, o.eps_abs, o.eps_rel, o.rho)
            if symbol.endswith("_lambda_max"):
                for c in range(got["k"]):
                    got["out"][c] = LAMBDA_ONE
            self.calls.append((symbol, got))
            return 0
        return call


@pytest.fixture(scope="module")
def real_lib():
    from admm_amd import _lib
    return _lib.load()


@pytest.fixture
def rec(real_lib, monkeypatch):
    from admm_amd import _lib
    r = Recorder(real_lib)
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


def data():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, P))
    y = rng.standard_normal(N)
    Y = (rng.uniform(size=(N, K)) < 0.5).astype(np.float64)
    Y[0], Y[1] = 0.0, 1.0                                          # both classes in every column
    labels = np.arange(N) % K + 5                                  # classes 5, 6, 7
    counts = rng.poisson(2.0, size=(N, K)).astype(np.float64) + 1.0
    return dict(x=x, y=y, Y=Y, labels=labels, counts=counts, xw=np.ascontiguousarray(x.T), yw=y[:P].copy())


# Per case: id -> (model(d), fit kwargs, symbols called, named values of the LAST call, fit class name,
#                  beta shape, niter (int: a Python int; a tuple: the shape of an int32 array), has trace / state attributes, state dim or None, classes)
def _cases():
    import admm_amd as A
    P1 = P + 1
    tr = dict(trace=True, state=STATE)
    base = dict(n=N, p=P, mem=0, intercept=1)
    c = {}
    c["bp"] = (lambda d: A.admm_bp(d["xw"], d["yw"]), {}, ["admm_hip_bp_state"], dict(n=P, p=N, mem=0, trace=None, trace_cap=0, state=None, state_cap=0),
               "ADMM_BP_fit", (N, 1), int, True, None, None)
    c["bp/trace"] = (c["bp"][0], tr, ["admm_hip_bp_state"], dict(n=P, p=N, mem=0, trace_cap=MAXIT + 8, state_cap=STATE), "ADMM_BP_fit", (N, 1), int, True, N, None)
    c["parbp"] = (lambda d: A.admm_bp(d["xw"], d["yw"]).parallel(2), {}, ["admm_hip_parbp_traced"], dict(n=P, p=N, mem=0, nthread=2, trace=None, trace_cap=0),
                  "ADMM_BP_fit", (N, 1), int, True, None, None)
    c["parbp/trace"] = (c["parbp"][0], tr, ["admm_hip_parbp_traced"], dict(n=P, p=N, mem=0, nthread=2, trace_cap=MAXIT + 8), "ADMM_BP_fit", (N, 1), int, True, None, None)
    c["lad"] = (lambda d: A.admm_lad(d["x"], d["y"]), {}, ["admm_hip_lad_state"], dict(base, trace=None, trace_cap=0, state=None, state_cap=0),
                "ADMM_LAD_fit", (P1,), int, True, None, None)
    c["lad/no-intercept"] = (lambda d: A.admm_lad(d["x"], d["y"], intercept=False), {}, ["admm_hip_lad_state"], dict(base, intercept=0), "ADMM_LAD_fit", (P1,), int, True, None, None)
    c["lad/trace"] = (c["lad"][0], tr, ["admm_hip_lad_state"], dict(base, trace_cap=MAXIT + 8, state_cap=STATE), "ADMM_LAD_fit", (P1,), int, True, N, None)
    c["quantreg"] = (lambda d: A.admm_quantreg(d["x"], d["y"], [0.25, 0.5, 0.75]), {}, ["admm_hip_quantreg"], dict(base, tau=[0.25, 0.5, 0.75], count=3),
                     "ADMM_QuantReg_fit", (P1, 3), (3,), True, None, None)
    c["quantreg/trace"] = (lambda d: A.admm_quantreg(d["x"], d["y"], 0.3), tr, ["admm_hip_quantreg_state"], dict(base, tau=0.3, trace_cap=MAXIT + 8, state_cap=STATE),
                           "ADMM_QuantReg_fit", (P1, 1), (1,), True, N, None)
    c["huber"] = (lambda d: A.admm_huber(d["x"], d["y"], [1.0, 2.0], 0.4), {}, ["admm_hip_huber"], dict(base, delta=[1.0, 2.0], tau=[0.4, 0.4], count=2),
                  "ADMM_Huber_fit", (P1, 2), (2,), True, None, None)
    c["huber/trace"] = (lambda d: A.admm_huber(d["x"], d["y"], 1.5, 0.4), tr, ["admm_hip_huber_state"], dict(base, delta=1.5, tau=0.4, trace_cap=MAXIT + 8, state_cap=STATE),
                        "ADMM_Huber_fit", (P1, 1), (1,), True, N, None)
    c["logit"] = (lambda d: A.admm_logit(d["x"], d["Y"][:, 0]), {}, ["admm_hip_logit"], base, "ADMM_Logit_fit", (P1,), int, True, None, None)
    c["logit/trace"] = (c["logit"][0], tr, ["admm_hip_logit_state"], dict(base, trace_cap=MAXIT + 8, state_cap=STATE), "ADMM_Logit_fit", (P1,), int, True, N, None)
    c["logit_multi"] = (lambda d: A.admm_logit_multi(d["x"], d["Y"]), {}, ["admm_hip_logit_multi"], dict(base, k=K), "ADMM_LogitMulti_fit", (P1, K), (K,), False, None, None)
    c["logit_ovr"] = (lambda d: A.admm_logit_ovr(d["x"], d["labels"]), {}, ["admm_hip_logit_multi"], dict(base, k=K), "ADMM_LogitMulti_fit", (P1, K), (K,), False, None, [5, 6, 7])
    for name, sym, ycol, cls, grid, one in (("logit_ridge", "admm_hip_logit_ridge", "Y", "ADMM_LogitRidge_fit", dict(lam=[2.0, 0.5]), dict(lam=0.7)),
                                            ("logit_enet", "admm_hip_logit_enet", "Y", "ADMM_LogitEnet_fit", dict(lam=[2.0, 0.5], alpha=[1.0, 0.25]), dict(lam=0.7, alpha=0.25)),
                                            ("poisson", "admm_hip_poisson", "counts", "ADMM_Poisson_fit", dict(lam=[2.0, 0.5], alpha=[1.0, 0.25]), dict(lam=0.7, alpha=0.25))):
        build = getattr(A, "admm_" + name)
        c[name] = (lambda d, b=build, g=grid, yc=ycol: b(d["x"], d[yc], **g), {}, [sym], dict(base, k=K, count=2, **grid), cls, (P1, K, 2), (K, 2), True, None, None)
        c[name + "/trace"] = (lambda d, b=build, g=one, yc=ycol: b(d["x"], d[yc][:, 0], **g), tr, [sym + "_state"], dict(base, trace_cap=MAXIT + 8, state_cap=STATE, **one),
                              cls, (P1,), int, True, N + P, None)
        if name != "poisson":
            c[name + "_ovr"] = (lambda d, b=getattr(A, "admm_" + name + "_ovr"), g=grid: b(d["x"], d["labels"], **g), {}, [sym], dict(base, k=K, count=2, **grid),
                                cls, (P1, K, 2), (K, 2), True, None, [5, 6, 7])
        if name != "logit_ridge":                                  # lam=None: lambda_1 from the device, then the fit on the log-spaced grid
            top = LAMBDA_ONE / 0.5
            auto = np.exp(np.linspace(np.log(top), np.log(top * 1e-4), 3)).tolist()
            c[name + "/auto"] = (lambda d, b=build, yc=ycol: b(d["x"], d[yc], alpha=0.5, nlambda=3), {}, [sym + "_lambda_max", sym],
                                 dict(base, k=K, count=3, lam=auto, alpha=[0.5] * 3), cls, (P1, K, 3), (K, 3), True, None, None)
            c[name + "/auto/trace"] = (lambda d, b=build, yc=ycol: b(d["x"], d[yc][:, 0], alpha=0.5, nlambda=1), tr, [sym + "_lambda_max", sym + "_state"],
                                       dict(base, lam=top, alpha=0.5, trace_cap=MAXIT + 8, state_cap=STATE), cls, (P1,), int, True, N + P, None)
    return c


CASES = _cases()


@pytest.mark.parametrize("case", sorted(CASES))
def test_what_the_builder_sends_and_what_fit_returns(rec, case):
    from admm_amd import api
    build, kw, symbols, sent, cls, beta_shape, niter_kind, has_records, state_dim, classes = CASES[case]
    model = build(data()).opts(maxit=MAXIT, rho=RHO)
    assert isinstance(model, api.ADMM_BP) and (case.startswith(("bp", "parbp")) or isinstance(model, api.ADMM_LAD))
    fit = model.fit(**kw)
    assert [s for s, _ in rec.calls] == symbols
    symbol, got = rec.calls[-1]
    for name, want in sent.items():
        if isinstance(want, (list, float)) and want is not None and name in GRID_NAMES:
            np.testing.assert_allclose(got[name], want, rtol=1e-15, atol=0, err_msg=name)
        else:
            assert got[name] == want, (name, got[name], want)
    eps = 1e-4
    assert got["opts"] == (MAXIT, eps, eps, RHO)
    for s, g in rec.calls[:-1]:                                    # the lambda_max call before the fit
        assert (g["n"], g["p"], g["k"], g["mem"], g["intercept"]) == (N, P, sent.get("k", 1), 0, 1)
    # what comes back
    assert type(fit) is getattr(api, cls)
    assert fit.beta.shape == beta_shape and fit.beta.dtype == np.float64
    if cls in ("ADMM_QuantReg_fit", "ADMM_Huber_fit"):             # a fresh row-major copy of the transposed buffer
        assert fit.beta.flags["C_CONTIGUOUS"] and fit.beta.flags["OWNDATA"]
    elif len(beta_shape) > 1 and cls != "ADMM_BP_fit":             # the library's column-major buffer, reshaped
        assert fit.beta.flags["F_CONTIGUOUS"]
    if niter_kind is int:
        assert type(fit.niter) is int and fit.niter == 0
    else:
        assert isinstance(fit.niter, np.ndarray) and fit.niter.shape == niter_kind and fit.niter.dtype == np.int32
    assert isinstance(fit.stats, dict) and "t_total" in fit.stats
    assert hasattr(fit, "trace") == has_records and hasattr(fit, "state") == has_records
    if has_records:
        if kw:
            assert fit.trace.shape == (0, 12) and fit.trace.dtype == np.float64
        else:
            assert fit.trace is None
        if state_dim is None:
            assert fit.state is None
        else:
            assert fit.state.shape == (0, 5, state_dim) and fit.state.dtype == np.float64
    if classes is None:
        assert not hasattr(fit, "classes")
    else:
        assert fit.classes.tolist() == classes
    for name in GRID_NAMES:                                        # the returned grid: equal to what was sent, and a copy
        if hasattr(fit, name):
            mine = getattr(model, name)
            if mine is not None:
                assert np.array_equal(getattr(fit, name), mine) and not np.shares_memory(getattr(fit, name), mine)
            if isinstance(sent.get(name), list):
                np.testing.assert_allclose(getattr(fit, name), sent[name], rtol=1e-15, atol=0)


def test_logit_multi_fit_takes_no_arguments(rec):
    import admm_amd as A
    d = data()
    for m in (A.admm_logit_multi(d["x"], d["Y"]), A.admm_logit_ovr(d["x"], d["labels"])):
        with pytest.raises(TypeError):
            m.fit(trace=True)
        with pytest.raises(TypeError):
            m.fit(False, 0)
    assert rec.calls == []


def test_state_without_trace_is_ignored_for_a_single_fit(rec):
    import admm_amd as A
    d = data()
    y1, c1 = d["Y"][:, 0], d["counts"][:, 0]
    for build, symbol in ((lambda: A.admm_bp(d["xw"], d["yw"]), "admm_hip_bp_state"), (lambda: A.admm_lad(d["x"], d["y"]), "admm_hip_lad_state"),
                          (lambda: A.admm_quantreg(d["x"], d["y"], 0.3), "admm_hip_quantreg"), (lambda: A.admm_huber(d["x"], d["y"], 1.5), "admm_hip_huber"),
                          (lambda: A.admm_logit(d["x"], y1), "admm_hip_logit"), (lambda: A.admm_logit_ridge(d["x"], y1, 0.7), "admm_hip_logit_ridge"),
                          (lambda: A.admm_logit_enet(d["x"], y1, 0.7), "admm_hip_logit_enet"), (lambda: A.admm_poisson(d["x"], c1, 0.7), "admm_hip_poisson")):
        del rec.calls[:]
        fit = build().fit(state=STATE)
        assert [s for s, _ in rec.calls] == [symbol]
        got = rec.calls[0][1]
        assert got.get("state") is None and got.get("state_cap", 0) == 0 and got.get("trace") is None
        assert fit.trace is None and fit.state is None


def test_trace_without_state_records_no_iterates(rec):
    import admm_amd as A
    d = data()
    for m in (A.admm_bp(d["xw"], d["yw"]), A.admm_lad(d["x"], d["y"]), A.admm_quantreg(d["x"], d["y"], 0.3), A.admm_logit(d["x"], d["Y"][:, 0]),
              A.admm_logit_ridge(d["x"], d["Y"][:, 0], 0.7), A.admm_poisson(d["x"], d["counts"][:, 0], 0.7)):
        del rec.calls[:]
        fit = m.fit(trace=True)
        got = rec.calls[-1][1]
        assert got["trace_cap"] == m.maxit + 8 and got["state"] is None and got["state_cap"] == 0 and got["nstate"] is None
        assert fit.trace.shape == (0, 12) and fit.state is None


SINGLE = {
    "quantreg": (lambda A, d: A.admm_quantreg(d["x"], d["y"], [0.25, 0.75]), "single tau"),
    "huber": (lambda A, d: A.admm_huber(d["x"], d["y"], [1.0, 2.0]), "single fit"),
    "logit_ridge/columns": (lambda A, d: A.admm_logit_ridge(d["x"], d["Y"], 0.7), "single label column and a single lambda"),
    "logit_ridge/lambdas": (lambda A, d: A.admm_logit_ridge(d["x"], d["Y"][:, 0], [0.7, 0.2]), "single label column and a single lambda"),
    "logit_ridge_ovr": (lambda A, d: A.admm_logit_ridge_ovr(d["x"], d["labels"], 0.7), "single label column and a single lambda"),
    "logit_enet/columns": (lambda A, d: A.admm_logit_enet(d["x"], d["Y"], 0.7), "single label column and a single cell"),
    "logit_enet/auto": (lambda A, d: A.admm_logit_enet(d["x"], d["Y"][:, 0], alpha=0.5, nlambda=3), "single label column and a single cell"),
    "logit_enet_ovr": (lambda A, d: A.admm_logit_enet_ovr(d["x"], d["labels"], alpha=0.5, nlambda=1), "single label column and a single cell"),
    "poisson/columns": (lambda A, d: A.admm_poisson(d["x"], d["counts"], 0.7), "single count column and a single cell"),
    "poisson/auto": (lambda A, d: A.admm_poisson(d["x"], d["counts"][:, 0], alpha=0.5, nlambda=3), "single count column and a single cell"),
}


@pytest.mark.parametrize("case", sorted(SINGLE))
def test_records_of_a_grid_are_refused_before_any_library_call(rec, case):
    import admm_amd as A
    build, noun = SINGLE[case]
    for kw in (dict(trace=True), dict(state=STATE), dict(trace=True, state=STATE)):
        with pytest.raises(ValueError, match="^trace and state are recorded for a " + noun + "$"):
            build(A, data()).fit(**kw)
    assert rec.calls == []                                         # the *_lambda_max of the automatic grid included


def test_lambda_one_goes_to_the_loss_own_symbol(rec):
    import admm_amd as A
    d = data()
    for m, symbol in ((A.admm_logit_enet(d["x"], d["Y"], 0.7), "admm_hip_logit_enet_lambda_max"), (A.admm_poisson(d["x"], d["counts"], 0.7), "admm_hip_poisson_lambda_max"),
                      (A.admm_logit_enet_ovr(d["x"], d["labels"], 0.7), "admm_hip_logit_enet_lambda_max")):
        del rec.calls[:]
        out = m.lambda_one()
        assert out.shape == (K,) and out.dtype == np.float64 and np.all(out == LAMBDA_ONE)
        assert [s for s, _ in rec.calls] == [symbol]
        got = rec.calls[0][1]
        assert (got["n"], got["p"], got["k"], got["mem"], got["intercept"]) == (N, P, K, 0, 1)


REPRS = {
    "ADMM_BP_fit": (lambda F, sp: F(sp.csc_matrix(np.zeros((6, 1))), 3, {}), "ADMM Basis Pursuit fitting result\n\n$beta\n<6 x 1> sparse matrix\n\n$niter\n3"),
    "ADMM_LAD_fit": (lambda F, sp: F(np.array([1.0, 2.0]), 3, {}), "ADMM LAD fitting result\n\n$beta\n[1. 2.]\n\n$niter\n3"),
    "ADMM_QuantReg_fit": (lambda F, sp: F(np.array([0.5]), np.zeros((3, 1)), np.array([4]), {}),
                          "ADMM quantile regression fitting result\n\n$tau\n[0.5]\n\n$beta\n<3 x 1> matrix\n\n$niter\n[4]"),
    "ADMM_Huber_fit": (lambda F, sp: F(np.array([1.5]), np.array([0.5]), np.zeros((3, 1)), np.array([4]), {}),
                       "ADMM Huber regression fitting result\n\n$delta\n[1.5]\n\n$tau\n[0.5]\n\n$beta\n<3 x 1> matrix\n\n$niter\n[4]"),
    "ADMM_Logit_fit": (lambda F, sp: F(np.array([1.0, 2.0]), 3, {}), "ADMM logistic regression fitting result\n\n$beta\n[1. 2.]\n\n$niter\n3"),
    "ADMM_LogitMulti_fit": (lambda F, sp: F(np.zeros((3, 2)), np.array([4, 5]), {}), "ADMM logistic regression fitting result\n\n$beta\n<3 x 2> matrix\n\n$niter\n[4 5]"),
    "ADMM_LogitRidge_fit": (lambda F, sp: F(np.array([2.0]), np.zeros((3, 2, 1)), np.array([[4], [5]]), {}),
                            "ADMM ridge logistic regression fitting result\n\n$lambda\n[2.]\n\n$beta\n<3 x 2 x 1> array\n\n$niter\n[[4]\n [5]]"),
    "ADMM_LogitEnet_fit": (lambda F, sp: F(np.array([2.0]), np.array([0.5]), np.zeros(3), 4, {}),
                           "ADMM elastic-net logistic regression fitting result\n\n$lambda\n[2.]\n\n$alpha\n[0.5]\n\n$beta\n<3> array\n\n$niter\n4"),
    "ADMM_Poisson_fit": (lambda F, sp: F(np.array([2.0]), np.array([0.5]), np.zeros((3, 2, 1)), np.array([[4], [5]]), {}),
                         "ADMM Poisson regression fitting result\n\n$lambda\n[2.]\n\n$alpha\n[0.5]\n\n$beta\n<3 x 2 x 1> array\n\n$niter\n[[4]\n [5]]"),
}


@pytest.mark.parametrize("cls", sorted(REPRS))
def test_fit_classes_are_built_positionally_and_print_as_before(cls, capsys):
    import scipy.sparse as sp
    from admm_amd import api
    make, text = REPRS[cls]
    fit = make(getattr(api, cls), sp)
    assert repr(fit) == text and fit.stats == {}
    fit.show()
    assert capsys.readouterr().out == text + "\n"
