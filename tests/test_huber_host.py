"""CPU: Huber / expectile regression (admm_hip_huber) without a device -- the prox against a brute-force argmin, the CPU restatement
of the loop (tests/huber_oracle.py) against a float64 IRLS optimum and against least squares, the symbols through every layer, what
the C ABI refuses before it looks for a device, and the Python builder's argument checks.

Bound against IRLS (eps_abs = eps_rel = 1e-4, rho = 1): the measured worst relative excess of the objective on exactly these inputs is
1.07e-5; the cap 1e-4 leaves a factor ~10 and a wrong prox (a knee or a weight off) misses it by orders of magnitude."""
import ctypes
import os
import re

import numpy as np
import pytest

import huber_oracle as ho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
SHAPES = [(400, 8, 1), (2100, 40, 2)]
TAUS = [0.5, 0.2, 0.9]
DELTAS = [0.3, 1.345, 5.0, np.inf]
OPTS = {"maxit": 10000, "eps_abs": 1e-4, "eps_rel": 1e-4, "rho": 1.0}
SYMBOLS = ("admm_hip_huber", "admm_hip_huber_state")


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
    assert len(lib.admm_hip_huber.argtypes) == 13
    assert len(lib.admm_hip_huber_state.argtypes) == len(lib.admm_hip_quantreg_state.argtypes) + 1


def test_prox_is_the_argmin_of_the_weighted_huber_function():
    """w H_delta(z) + rho / 2 (z - v)^2 over a fine grid around the prox: nothing on the grid is lower, and the neighbours are higher."""
    rng = np.random.default_rng(7)
    for trial in range(400):
        rho = float(np.exp(rng.uniform(-3, 3)))
        tau = float(rng.uniform(0.02, 0.98))
        delta = np.inf if trial % 4 == 0 else float(np.exp(rng.uniform(-3, 2)))
        v = float(rng.standard_normal() * 4 * (delta if np.isfinite(delta) else 1.0) * (1 + 2.0 / rho))
        z = float(ho.prox(np.array([v]), rho, tau, delta)[0])

        def obj(t):
            a = np.abs(t)
            with np.errstate(invalid="ignore", over="ignore"):
                h = np.where(a <= delta, 0.5 * t * t, delta * a - 0.5 * delta * delta)
            return np.where(t >= 0, 2.0 * (1.0 - tau), 2.0 * tau) * h + 0.5 * rho * (t - v) ** 2

        span = abs(v) + 1.0
        grid = np.linspace(-span, span, 200001)
        zb = float(grid[np.argmin(obj(grid))])
        assert abs(z - zb) <= 2 * span / 200000 + 1e-12, (rho, tau, delta, v, z, zb)
        assert obj(np.array([z]))[0] <= obj(grid).min() + 1e-12 * (1 + abs(obj(np.array([z]))[0])), (rho, tau, delta, v)
        assert z == 0.0 or np.sign(z) == np.sign(v)
        assert abs(z) <= abs(v)


def test_prox_branches_meet_at_the_knees_and_at_zero():
    rho, tau, delta = 0.7, 0.3, 1.2
    hi, lo = 2 * (1 - tau) / rho, 2 * tau / rho
    v = np.array([delta * (1 + hi), -delta * (1 + lo), 0.0, -0.0])
    z = ho.prox(v, rho, tau, delta)
    assert np.allclose(z[:2], [delta, -delta], rtol=1e-15) and z[2] == 0.0 and z[3] == 0.0
    big = ho.prox(np.array([1e300, -1e300, 3.0, -3.0]), rho, tau, np.inf)          # delta = inf: only the central branch
    assert np.array_equal(big, np.array([1e300 / (1 + hi), -1e300 / (1 + lo), 3.0 / (1 + hi), -3.0 / (1 + lo)]))


_IRLS = {}


def _irls(n, p, seed, delta, tau, intercept):
    key = (n, p, seed, delta, tau, intercept)
    if key not in _IRLS:
        _IRLS[key] = ho.huber_irls(*ho.issue_data(n, p, seed), delta, tau, intercept)
    return _IRLS[key]


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("n,p,seed", SHAPES)
def test_restatement_against_the_irls_optimum(n, p, seed, tau, delta, intercept):
    x, y = ho.issue_data(n, p, seed)
    got = ho.huber(x, y, delta, tau, intercept, OPTS)
    assert got["niter"] <= 60                                        # tens of iterations, where LAD needs hundreds
    _, best = _irls(n, p, seed, delta, tau, intercept)
    f = ho.huber_loss(x, y, got["beta"], delta, tau)
    excess = f / best - 1.0
    print(f"[huber restatement n={n} p={p} tau={tau} delta={delta} icpt={int(intercept)}] niter {got['niter']}, objective {f:.6e} vs IRLS {best:.6e} (+{excess:.2e})")
    assert -1e-9 <= excess <= 1e-4
    if not intercept:
        assert got["beta"][0] == 0.0


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("n,p,seed", SHAPES)
def test_restatement_at_tau_half_delta_inf_is_least_squares(n, p, seed, intercept):
    x, y = ho.issue_data(n, p, seed)
    got = ho.huber(x, y, np.inf, 0.5, intercept, OPTS)
    A = np.hstack([np.ones((n, 1)), x]) if intercept else x
    b = np.linalg.lstsq(A, y, rcond=None)[0]
    ref = b if intercept else np.concatenate([[0.0], b])
    err = float(np.max(np.abs(got["beta"] - ref)) / np.max(np.abs(ref)))
    print(f"[huber = lstsq n={n} p={p} icpt={int(intercept)}] niter {got['niter']}, err {err:.2e}")
    assert err <= 1e-10


def test_restated_iteration_counts_of_the_slot_grid():
    """What tests/test_gpu_huber.py relies on: the seven fits of its grid finish at different iterations, and none within one
    iteration of its maxit = 18 split."""
    x, y = ho.issue_data(2100, 40, 2)
    grid = [(0.3, 0.5), (np.inf, 0.5), (0.3, 0.9), (1.345, 0.2), (0.3, 0.5), (5.0, 0.2), (1.345, 0.9)]
    counts = [ho.huber(x, y, d, t, True, OPTS)["niter"] for d, t in grid]
    assert counts == [16, 10, 50, 20, 16, 24, 31]


def _call(lib, **over):
    from admm_amd._lib import AdmmOpts
    keep = dict(x=np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), y=np.arange(6.0), delta=np.array([1.345, np.inf]), tau=np.array([0.25, 0.5]),
                beta=np.zeros(16), niter=np.zeros(8, np.int32))
    dp = ctypes.POINTER(ctypes.c_double)
    v = dict(x=keep["x"].ctypes.data, y=keep["y"].ctypes.data, n=6, p=2, mem=0, intercept=1, delta=keep["delta"].ctypes.data_as(dp),
             tau=keep["tau"].ctypes.data_as(dp), nfit=2,
             opts=(10, 1e-4, 1e-4, 1.0), beta=keep["beta"].ctypes.data_as(dp), niter=keep["niter"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    given = {name: np.asarray(over.pop(name + "_values"), dtype=np.float64) for name in ("delta", "tau") if name + "_values" in over}
    if given:                                                  # one length for both: the array not given is filled with a legal value
        nfit = len(next(iter(given.values())))
        keep["delta"] = given.get("delta", np.full(nfit, 1.0))
        keep["tau"] = given.get("tau", np.full(nfit, 0.5))
        v.update(delta=keep["delta"].ctypes.data_as(dp), tau=keep["tau"].ctypes.data_as(dp), nfit=nfit)
    v.update(over)
    o = AdmmOpts(*v["opts"]) if v["opts"] is not None else None
    rc = lib.admm_hip_huber(v["x"], v["y"], v["n"], v["p"], v["mem"], v["intercept"], v["delta"], v["tau"], v["nfit"],
                            ctypes.byref(o) if o is not None else None, v["beta"], v["niter"], None)
    return rc, lib.admm_hip_last_error().decode()


DELTA_MSG = "every delta must be positive (+inf: expectile regression)"
TAU_MSG = "every tau must lie strictly between 0 and 1"
REFUSALS = [
    (dict(delta=None), "delta must not be NULL"),
    (dict(nfit=0), "the number of fits must be within [1, 4096]"),
    (dict(delta_values=np.full(4097, 1.0)), "the number of fits must be within [1, 4096]"),
    (dict(delta_values=[1.0, 0.0]), DELTA_MSG),
    (dict(delta_values=[-2.0]), DELTA_MSG),
    (dict(delta_values=[1.0, float("nan")]), DELTA_MSG),
    (dict(delta_values=[float("-inf")]), DELTA_MSG),
    (dict(tau_values=[0.5, 0.0]), TAU_MSG),
    (dict(tau_values=[1.0]), TAU_MSG),
    (dict(tau_values=[-0.2]), TAU_MSG),
    (dict(tau_values=[0.5, float("nan")]), TAU_MSG),
    (dict(tau_values=[float("inf")]), TAU_MSG),
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


@pytest.mark.parametrize("over,message", REFUSALS, ids=[f"{k}-" + m[:24] + "/" + ",".join(o) for k, (o, m) in enumerate(REFUSALS)])
def test_bad_calls_are_refused_before_any_device_is_touched(over, message):
    from admm_amd import _lib
    lib = _lib.load()
    assert _call(lib, **dict(over)) == (INVALID_ARG, message)


def test_the_order_of_the_refusals():
    """delta before the count, the count before the values, delta's values before tau's, the values before the shape."""
    from admm_amd import _lib
    lib = _lib.load()
    assert _call(lib, delta=None, nfit=0)[1] == "delta must not be NULL"
    assert _call(lib, nfit=0, n=0)[1] == "the number of fits must be within [1, 4096]"
    assert _call(lib, delta_values=[-1.0], tau_values=[2.0])[1] == DELTA_MSG
    assert _call(lib, tau_values=[2.0], n=3)[1] == TAU_MSG


def test_accepted_arguments_pass_every_check():
    """+inf is a legal delta and a NULL tau means 0.5: both pass every check (and then the call looks for a device)."""
    from admm_amd import _lib
    lib = _lib.load()
    assert _call(lib, delta_values=[float("inf"), 1e-3])[0] != INVALID_ARG
    assert _call(lib, tau=None)[0] != INVALID_ARG
    assert _call(lib, n=3, p=2, intercept=0)[0] != INVALID_ARG


def test_state_entry_point_refuses_like_quantreg_state():
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    x, y = np.asfortranarray(np.arange(12.0).reshape(6, 2) % 5), np.arange(6.0)
    beta, niter, o = np.zeros(3), np.zeros(1, np.int32), AdmmOpts(10, 1e-4, 1e-4, 1.0)
    st, nst = np.zeros(64), ctypes.c_longlong()
    dp = ctypes.POINTER(ctypes.c_double)

    def call(delta, tau, state_cap):
        rc = lib.admm_hip_huber_state(x.ctypes.data, y.ctypes.data, 6, 2, 0, 1, delta, tau, ctypes.byref(o), beta.ctypes.data_as(dp),
                                      niter.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None, 0, None,
                                      st.ctypes.data_as(dp), state_cap, ctypes.byref(nst))
        return rc, lib.admm_hip_last_error().decode()
    assert call(1.345, 0.5, 2) == (INVALID_ARG, "bad state arguments (the iterate dump needs the trace)")
    assert call(1.345, 1.5, 0) == (INVALID_ARG, TAU_MSG)
    assert call(0.0, 0.5, 0) == (INVALID_ARG, DELTA_MSG)


def test_python_builder_argument_checks():
    from admm_amd import ADMM_Huber, admm_huber
    from admm_amd.api import ADMM_LAD, ADMM_Huber_fit
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal((30, 12)), rng.standard_normal(30)
    m = admm_huber(x, y)
    assert isinstance(m, ADMM_Huber) and isinstance(m, ADMM_LAD)
    assert m.delta.tolist() == [1.345] and m.tau.tolist() == [0.5] and m.intercept is True
    assert (m.maxit, m.eps_abs, m.eps_rel, m.rho) == (10000, 1e-4, 1e-4, 1.0)          # as admm_lad
    assert m.opts(maxit=7, rho=2.0).maxit == 7 and m.rho == 2.0
    with pytest.raises(ValueError, match="maxit should be positive"):
        m.opts(maxit=0)
    # broadcasting: a scalar against an array either way, equal lengths kept as given (unsorted, repeats)
    a = admm_huber(x, y, [3.0, 0.3, 3.0], 0.2)
    assert a.delta.tolist() == [3.0, 0.3, 3.0] and a.tau.tolist() == [0.2, 0.2, 0.2]
    b = admm_huber(x, y, np.inf, [0.9, 0.1])
    assert b.delta.tolist() == [np.inf, np.inf] and b.tau.tolist() == [0.9, 0.1]
    c = admm_huber(x, y, [1.0, 2.0], [0.9, 0.1])
    assert c.delta.tolist() == [1.0, 2.0] and c.tau.tolist() == [0.9, 0.1]
    assert c.delta.flags["C_CONTIGUOUS"] and c.delta.flags["WRITEABLE"]
    with pytest.raises(ValueError, match="one common length"):
        admm_huber(x, y, [1.0, 2.0], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="scalars or 1-D arrays"):
        admm_huber(x, y, np.ones((2, 2)))
    for bad in (0.0, -1.0, [1.0, np.nan], -np.inf):
        with pytest.raises(ValueError, match="every delta must be positive"):
            admm_huber(x, y, bad)
    for bad in (0.0, 1.0, -0.1, [0.5, np.nan], [0.2, np.inf]):
        with pytest.raises(ValueError, match="strictly between 0 and 1"):
            admm_huber(x, y, 1.345, bad)
    with pytest.raises(ValueError, match="between 1 and 4096"):
        admm_huber(x, y, [])
    with pytest.raises(ValueError, match="between 1 and 4096"):
        admm_huber(x, y, 1.0, np.full(4097, 0.5))
    with pytest.raises(ValueError, match="nrow\\(x\\) should be equal to length\\(y\\)"):
        admm_huber(x, y[:-1])
    with pytest.raises(ValueError, match="the intercept is fitted"):
        admm_huber(x[:13], y[:13])                                                   # n = p + 1: LAD's rule holds, this one does not
    assert admm_huber(x[:13], y[:13], intercept=False).n == 13
    with pytest.raises(ValueError, match="nrow\\(x\\) must be greater than ncol\\(x\\)"):
        admm_huber(x[:12], y[:12], intercept=False)
    with pytest.raises(ValueError, match="single fit"):
        admm_huber(x, y, [0.2, 0.8]).fit(trace=True)
    assert "Huber" in repr(ADMM_Huber_fit(np.array([1.0]), np.array([0.5]), np.zeros((3, 1)), np.array([4]), {}))
