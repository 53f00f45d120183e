"""CPU: quantile regression (admm_hip_quantreg) without a device -- the CPU restatement of the loop (tests/quantile_oracle.py) against
LAD and against the quantile linear programme, what the C ABI refuses before it looks for a device, the Python builder's argument
checks, and the QUANT_SLOTS option.

Bounds against the LP (eps_abs = eps_rel = 1e-4, rho = 1, maxit 10 000): measured relative excess of the check loss 3.4e-5 ... 2.2e-4 and
|fraction of negative residuals - tau| <= 0.005 on these data; the bounds 1e-3 and 0.01 leave a factor 4 / 2 for other data orders."""
import ctypes

import numpy as np
import pytest

import quantile_oracle as qo

INVALID_ARG = 1
SHAPES = [(400, 8, 1), (2100, 40, 2)]
TAUS = [0.1, 0.25, 0.5, 0.9]


def test_restatement_at_the_median_without_intercept_is_lad_bit_for_bit():
    from oracle import entry
    for n, p, seed in SHAPES:
        x, y = qo.issue_data(n, p, seed)
        ref = entry.admm_lad(x, y, False, entry.LAD_OPTS)
        got = qo.quantreg(x, y, 0.5, False, entry.LAD_OPTS)
        assert got["niter"] == ref["niter"]
        assert np.array_equal(got["beta"], ref["beta"])


_LP = {}


def _lp(n, p, seed, tau, intercept):
    key = (n, p, seed, tau, intercept)
    if key not in _LP:
        x, y = qo.issue_data(n, p, seed)
        _LP[key] = qo.quantile_lp(x, y, tau, intercept)
    return _LP[key]


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("n,p,seed", SHAPES)
def test_restatement_against_the_quantile_lp(n, p, seed, tau, intercept):
    from oracle import entry
    x, y = qo.issue_data(n, p, seed)
    got = qo.quantreg(x, y, tau, intercept, entry.LAD_OPTS)
    assert got["niter"] <= entry.LAD_OPTS["maxit"]                     # converged
    _, best = _lp(n, p, seed, tau, intercept)
    f = qo.check_loss(x, y, got["beta"], tau)
    excess = f / best - 1.0
    frac = qo.neg_fraction(x, y, got["beta"])
    print(f"[quantreg restatement n={n} p={p} tau={tau} icpt={int(intercept)}] niter {got['niter']}, objective {f:.6e} vs LP {best:.6e} (+{excess:.2e}), "
          f"negative residuals {frac:.4f}")
    assert -1e-9 <= excess <= 1e-3
    if intercept:
        assert abs(frac - tau) <= 0.01
    else:
        assert got["beta"][0] == 0.0


def _call(lib, **over):
    from admm_amd._lib import AdmmOpts
    keep = dict(x=np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), y=np.arange(6.0), tau=np.array([0.25, 0.5]), beta=np.zeros(16), niter=np.zeros(8, np.int32))
    dp = ctypes.POINTER(ctypes.c_double)
    v = dict(x=keep["x"].ctypes.data, y=keep["y"].ctypes.data, n=6, p=2, mem=0, intercept=1, tau=keep["tau"].ctypes.data_as(dp), ntau=2,
             opts=(10, 1e-4, 1e-4, 1.0), beta=keep["beta"].ctypes.data_as(dp), niter=keep["niter"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    if "tau_values" in over:
        keep["tau"] = np.asarray(over.pop("tau_values"), dtype=np.float64)
        v["tau"], v["ntau"] = keep["tau"].ctypes.data_as(dp), len(keep["tau"])
    v.update(over)
    o = AdmmOpts(*v["opts"]) if v["opts"] is not None else None
    rc = lib.admm_hip_quantreg(v["x"], v["y"], v["n"], v["p"], v["mem"], v["intercept"], v["tau"], v["ntau"],
                               ctypes.byref(o) if o is not None else None, v["beta"], v["niter"], None)
    return rc, lib.admm_hip_last_error().decode()


REFUSALS = [
    (dict(tau=None), "tau must not be NULL"),
    (dict(ntau=0), "the number of quantiles must be within [1, 4096]"),
    (dict(tau_values=np.full(4097, 0.5)), "the number of quantiles must be within [1, 4096]"),
    (dict(tau_values=[0.5, 0.0]), "every tau must lie strictly between 0 and 1"),
    (dict(tau_values=[1.0]), "every tau must lie strictly between 0 and 1"),
    (dict(tau_values=[-0.2]), "every tau must lie strictly between 0 and 1"),
    (dict(tau_values=[0.5, float("nan")]), "every tau must lie strictly between 0 and 1"),
    (dict(tau_values=[float("inf")]), "every tau must lie strictly between 0 and 1"),
    (dict(n=3, p=2, intercept=1), "nrow(x) must be greater than ncol(x) + 1 (the intercept is fitted)"),
    (dict(n=2, p=2, intercept=0), "nrow(x) must be greater than ncol(x)"),
    (dict(x=None), "x and y must not be NULL"),
    (dict(n=0), "n and p must be positive"),
    (dict(mem=7), "mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE"),
    (dict(opts=None), "opts must not be NULL"),
    (dict(opts=(0, 1e-4, 1e-4, 1.0)), "maxit should be positive"),
    (dict(opts=(10, -1.0, 1e-4, 1.0)), "eps_abs and eps_rel should be nonnegative"),
    (dict(opts=(10, 1e-4, 1e-4, 0.0)), "rho should be positive"),
    (dict(beta=None), "output pointers must not be NULL"),
]


@pytest.mark.parametrize("over,message", REFUSALS, ids=[m[:28] + "/" + ",".join(o) for o, m in REFUSALS])
def test_bad_calls_are_refused_before_any_device_is_touched(over, message):
    from admm_amd import _lib
    lib = _lib.load()
    assert _call(lib, **dict(over)) == (INVALID_ARG, message)


def test_a_shape_that_lad_takes_is_refused_when_the_intercept_is_fitted():
    """n = p + 1: admm_hip_lad's rule (n > p) holds, admm_hip_quantreg with the intercept needs one more row."""
    from admm_amd import _lib
    lib = _lib.load()
    assert _call(lib, n=3, p=2, intercept=1)[0] == INVALID_ARG
    assert _call(lib, n=3, p=2, intercept=0)[0] != INVALID_ARG          # passes every check (and then looks for a device)


def test_state_entry_point_refuses_like_lad_state():
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    x, y = np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), np.arange(6.0)
    beta, niter, o = np.zeros(3), np.zeros(1, np.int32), AdmmOpts(10, 1e-4, 1e-4, 1.0)
    st, nst = np.zeros(64), ctypes.c_longlong()
    dp = ctypes.POINTER(ctypes.c_double)

    def call(tau, state_cap):
        rc = lib.admm_hip_quantreg_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, tau, ctypes.byref(o), beta.ctypes.data_as(dp),
                                         niter.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None, 0, None,
                                         st.ctypes.data_as(dp), state_cap, ctypes.byref(nst))
        return rc, lib.admm_hip_last_error().decode()
    assert call(0.5, 2) == (INVALID_ARG, "bad state arguments (the iterate dump needs the trace)")
    assert call(1.5, 0) == (INVALID_ARG, "every tau must lie strictly between 0 and 1")


def test_python_builder_argument_checks():
    from admm_amd import ADMM_QuantReg, admm_quantreg
    from admm_amd.api import ADMM_LAD, ADMM_QuantReg_fit
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal((30, 12)), rng.standard_normal(30)
    m = admm_quantreg(x, y)
    assert isinstance(m, ADMM_QuantReg) and isinstance(m, ADMM_LAD)
    assert m.tau.tolist() == [0.5] and m.intercept is True
    assert (m.maxit, m.eps_abs, m.eps_rel, m.rho) == (10000, 1e-4, 1e-4, 1.0)          # as admm_lad
    assert admm_quantreg(x, y, [0.9, 0.1, 0.9]).tau.tolist() == [0.9, 0.1, 0.9]          # unsorted, repeats
    assert m.opts(maxit=7, rho=2.0).maxit == 7 and m.rho == 2.0
    with pytest.raises(ValueError, match="maxit should be positive"):
        m.opts(maxit=0)
    for bad in (0.0, 1.0, -0.1, [0.5, np.nan], [0.2, np.inf]):
        with pytest.raises(ValueError, match="strictly between 0 and 1"):
            admm_quantreg(x, y, bad)
    with pytest.raises(ValueError, match="between 1 and 4096"):
        admm_quantreg(x, y, [])
    with pytest.raises(ValueError, match="between 1 and 4096"):
        admm_quantreg(x, y, np.full(4097, 0.5))
    with pytest.raises(ValueError, match="nrow\\(x\\) should be equal to length\\(y\\)"):
        admm_quantreg(x, y[:-1])
    with pytest.raises(ValueError, match="the intercept is fitted"):
        admm_quantreg(x[:13], y[:13])                                                # n = p + 1: LAD's rule holds, this one does not
    assert admm_quantreg(x[:13], y[:13], intercept=False).n == 13
    with pytest.raises(ValueError, match="nrow\\(x\\) must be greater than ncol\\(x\\)"):
        admm_quantreg(x[:12], y[:12], intercept=False)
    with pytest.raises(ValueError, match="single tau"):
        admm_quantreg(x, y, [0.2, 0.8]).fit(trace=True)
    assert "quantile" in repr(ADMM_QuantReg_fit(np.array([0.5]), np.zeros((3, 1)), np.array([4]), {}))


def test_quant_slots_option_is_known_and_bounded():
    from admm_amd import _lib
    lib = _lib.load()
    _lib.options.reset()
    try:
        for v in (b"0", b"1", b"2", b"8"):
            assert lib.admm_hip_option_set(b"QUANT_SLOTS", v) == 0
            assert lib.admm_hip_option_get(b"ADMM_HIP_QUANT_SLOTS") == v
        assert lib.admm_hip_option_set(b"QUANT_SLOTS", b"9") == INVALID_ARG
        assert lib.admm_hip_option_set(b"QUANT_SLOTS", b"-1") == INVALID_ARG
        assert lib.admm_hip_option_get(b"QUANT_SLOTS") == b"8"              # a refused value changes nothing
    finally:
        _lib.options.reset()
