"""Box-constrained, weighted elastic net (admm_hip_boxenet), everything that needs no GPU: what the C ABI refuses before it looks for a
device, the declared and exported symbols, the Python builder (broadcasting, messages), the host's lambda_0 against
tests/box_oracle.py, the degenerate cases of the restated prox, and the restated float64 path on the shape B1 against a projected
coordinate descent that shares nothing with ADMM."""
import ctypes
import os
import re

import numpy as np
import pytest

import box_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 2
F = np.float32
INF = np.inf


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _call(entry="boxenet", n=6, p=4, lower=None, upper=None, pf=None, alpha=-1.0, x="ok", opts=(10, 1e-5, 1e-5, -1.0),
          nlambda_auto=5, lmin_ratio=0.01, mem=0):
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    xa = np.asfortranarray(np.ones((n, p)))
    ya = np.ones(n)
    lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64)
    hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64)
    u = None if pf is None else np.ascontiguousarray(pf, dtype=np.float64)
    o = AdmmOpts(*opts)
    lam_out, beta, nit = np.zeros(nlambda_auto + 1), np.zeros((p + 1) * (nlambda_auto + 1), dtype=np.float32), np.zeros(nlambda_auto + 1, dtype=np.int32)
    head = (ctypes.c_void_p(xa.ctypes.data) if x == "ok" else None, ctypes.c_void_p(ya.ctypes.data), n, p, mem,
            _dp(lo), _dp(hi), _dp(u), alpha, None, 0, nlambda_auto, lmin_ratio, 1, 1, ctypes.byref(o))
    if entry == "boxenet":
        rc = lib.admm_hip_boxenet(*head, lam_out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                  beta.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nit.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None)
    else:
        h = ctypes.c_void_p()
        rc = lib.admm_hip_boxenet_plan_create(*head, ctypes.byref(h), None)
        assert h.value is None or rc == 0
        if h.value is not None:
            lib.admm_hip_lasso_plan_destroy(h)
    return rc, lib.admm_hip_last_error().decode()


REFUSALS = [
    # n <= p: the wide solver is named
    (dict(n=4, p=4), "not built for bounds"),
    (dict(n=3, p=4), "not built for bounds"),
    # bounds that cross zero the wrong way or hold NaN
    (dict(lower=(0.0, 0.1, 0.0, 0.0)), "lower bounds must be <= 0"),
    (dict(lower=(0.0, np.nan, 0.0, 0.0)), "lower bounds must be <= 0"),
    (dict(lower=(0.0, INF, 0.0, 0.0)), "lower bounds must be <= 0"),
    (dict(upper=(0.0, 0.0, -1e-300, 0.0)), "upper bounds must be >= 0"),
    (dict(upper=(np.nan, 0.0, 1.0, 0.0)), "upper bounds must be >= 0"),
    (dict(upper=(1.0, 1.0, 1.0, -INF)), "upper bounds must be >= 0"),
    # the factors
    (dict(pf=(1.0, -0.5, 1.0, 1.0)), "penalty factors must be finite and non-negative"),
    (dict(pf=(1.0, np.nan, 1.0, 1.0)), "penalty factors must be finite and non-negative"),
    (dict(pf=(INF, 1.0, 1.0, 1.0)), "penalty factors must be finite and non-negative"),
    (dict(pf=(0.0, 0.0, 0.0, 0.0)), "at least one penalty factor must be positive"),
    # alpha
    (dict(alpha=1.01), "within [0, 1]"),
    (dict(alpha=INF), "within [0, 1]"),
    (dict(alpha=np.nan), "within [0, 1]"),
    # what check_common / PathSpec::check() refuse for every path entry point
    (dict(x=None), "x and y must not be NULL"),
    (dict(n=0), "n and p must be positive"),
    (dict(mem=7), "mem must be"),
    (dict(opts=(0, 1e-5, 1e-5, -1.0)), "maxit should be positive"),
    (dict(opts=(10, -1.0, 1e-5, -1.0)), "nonnegative"),
    (dict(nlambda_auto=0), "need a lambda grid"),
    (dict(lmin_ratio=1.0), "lambda_min_ratio"),
]
# An attached communicator is refused too, but none can be attached without a device (admm_hip_comm_init looks for one first): that
# refusal has no CPU test.


@pytest.mark.parametrize("entry", ["boxenet", "boxenet_plan_create"])
def test_c_abi_refuses_bad_box_calls_before_it_looks_for_a_device(entry):
    for spoil, fragment in REFUSALS:
        rc, msg = _call(entry, **spoil)
        assert rc == INVALID_ARG and fragment in msg, (entry, spoil, rc, msg)


@pytest.mark.parametrize("entry", ["boxenet", "boxenet_plan_create"])
def test_refine_is_refused_for_the_box_constrained_elastic_net(entry):
    from admm_amd import _lib
    with _lib.options(REFINE="1"):
        rc, msg = _call(entry)
    assert rc == INVALID_ARG and "REFINE" in msg and "box-constrained" in msg


def test_legal_calls_pass_the_checks():
    for kw in (dict(), dict(alpha=0.0), dict(alpha=1.0), dict(alpha=0.5, pf=(0.0, 0.0, 0.0, 2.0)), dict(alpha=-3.0),
               dict(lower=(-INF, 0.0, -0.1, 0.0), upper=(INF, 0.25, 0.1, 0.0)), dict(lower=(0.0,) * 4), dict(upper=(0.0,) * 4),
               dict(lower=(-0.0,) * 4, upper=(1e300,) * 4, pf=(1.0, 0.0, 0.5, 3.0), alpha=0.3)):
        for entry in ("boxenet", "boxenet_plan_create"):
            rc, msg = _call(entry, **kw)
            assert rc in (0, NO_DEVICE), (entry, kw, rc, msg)


def test_symbols_are_declared_and_exported():
    from admm_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "admm_hip.h")).read(), flags=re.S)
    for sym in ("admm_hip_boxenet", "admm_hip_boxenet_plan_create", "admm_hip_host_box_lambda0"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym) and sym in _lib.EXPORTS
    import admm_amd
    assert "admm_boxenet" in admm_amd.__all__ and "ADMM_BoxEnet" in admm_amd.__all__


def test_builder_broadcasts_scalars_and_refuses_what_the_c_abi_refuses():
    from admm_amd import admm_boxenet, ADMM_BoxEnet, ADMM_Lasso
    rng = np.random.default_rng(5)
    x = rng.standard_normal((20, 6))
    y = rng.standard_normal(20)
    m = admm_boxenet(x, y)
    assert isinstance(m, ADMM_BoxEnet) and isinstance(m, ADMM_Lasso) and m.lower is None and m.upper is None
    assert m.alpha is None and m.penalty_factor is None and m.intercept and m.standardize
    assert m._box_args() == (None, None, None, -1.0)
    m = admm_boxenet(x, y, lower=0)                                       # scikit-learn's positive=True
    assert m.lower.tolist() == [0.0] * 6 and m.upper is None and m.lower.dtype == np.float64
    m = admm_boxenet(x, y, lower=[-1, 0, -INF, 0, -2, 0], upper=0.5, intercept=False, standardize=False)
    assert m.lower.tolist() == [-1, 0, -INF, 0, -2, 0] and m.upper.tolist() == [0.5] * 6 and not m.intercept and not m.standardize
    m.penalty(nlambda=4, lambda_min_ratio=0.1, alpha=0.5, penalty_factor=2)
    assert m.alpha == 0.5 and m.penalty_factor.tolist() == [2.0] * 6 and m.nlambda == 4
    assert m._box_args()[3] == 0.5 and all(a is not None for a in m._box_args()[:3])
    m.penalty(penalty_factor=[1, 0, 2, 3, 0, 1])
    assert m.alpha is None and m.penalty_factor.tolist() == [1, 0, 2, 3, 0, 1] and m._box_args()[3] == -1.0
    assert m.penalty(alpha=0).alpha == 0.0 and m.penalty(alpha=1).alpha == 1.0 and m.penalty_factor is None
    for kw, frag in ((dict(lower=0.1), r"lower bounds must be <= 0"), (dict(lower=[0, 0, np.nan, 0, 0, 0]), r"lower bounds must be <= 0"),
                     (dict(upper=-0.1), r"upper bounds must be >= 0"), (dict(upper=[1, 1, 1, np.nan, 1, 1]), r"upper bounds must be >= 0"),
                     (dict(lower=[0.0] * 5), "lower should be a scalar or have one entry per column"),
                     (dict(upper=[0.0] * 7), "upper should be a scalar or have one entry per column")):
        with pytest.raises(ValueError, match=frag):
            admm_boxenet(x, y, **kw)
    g = admm_boxenet(x, y, lower=-1, upper=1)
    for kw, frag in ((dict(penalty_factor=[1.0] * 5), "penalty_factor should be a scalar or have one entry per column"),
                     (dict(penalty_factor=[1, 1, -1, 1, 1, 1]), "finite and non-negative"),
                     (dict(penalty_factor=[1, 1, np.nan, 1, 1, 1]), "finite and non-negative"),
                     (dict(penalty_factor=INF), "finite and non-negative"),
                     (dict(penalty_factor=0), "at least one penalty factor must be positive"),
                     (dict(alpha=1.5), r"within \[0, 1\]"), (dict(alpha=-0.5), r"within \[0, 1\]"), (dict(alpha=float("nan")), r"within \[0, 1\]")):
        with pytest.raises(ValueError, match=frag):
            g.penalty(**kw)
    with pytest.raises(ValueError, match="not built for bounds"):
        admm_boxenet(x[:6], y[:6])
    for call in (lambda: g.parallel(2), lambda: g.cv(3), lambda: g.fit_responses(np.zeros((20, 2)))):
        with pytest.raises(ValueError, match="not available for the box-constrained elastic net"):
            call()


# ---- lambda_0 of the automatic grid

def _lib_lambda0(c, lo=None, hi=None, u=None, alpha=None):
    from admm_amd import _lib
    lib = _lib.load()
    c = np.ascontiguousarray(c, dtype=np.float32)
    lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.float32)
    hi = None if hi is None else np.ascontiguousarray(hi, dtype=np.float32)
    u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    out = ctypes.c_float()
    rc = lib.admm_hip_host_box_lambda0(_fp(c), c.size, _fp(lo), _fp(hi), _dp(u), -1.0 if alpha is None else float(alpha), ctypes.byref(out))
    assert rc == 0, lib.admm_hip_last_error().decode()
    return np.float32(out.value)


def _b1():
    n, p, seed = bo.B1
    x, y = bo.synth_box(n, p, seed)
    return (x, y) + bo.box_pattern(p)


def test_host_lambda0_is_the_oracles_as_floats():
    x, y, lower, upper, u = _b1()
    p = x.shape[1]
    r = bo.box_path(x, y, lower, upper, u, nlambda=1, maxit=1)             # (only for X'y and the bounds in solver units)
    c, lo, hi = r["solver"].XY, r["lo"], r["hi"]
    for alpha in (None, 0.5):
        want = bo.box_lambda0(c, u, lo, hi, alpha)
        assert _lib_lambda0(c, lo, hi, u, alpha).tobytes() == want.tobytes(), alpha
    # no bounds, unit factors: max |c| to the bit, with NULL or with explicit arrays
    top = np.max(np.abs(c))
    assert _lib_lambda0(c).tobytes() == top.tobytes()
    assert _lib_lambda0(c, np.full(p, -INF), np.full(p, INF), np.ones(p)).tobytes() == top.tobytes()
    assert _lib_lambda0(c, alpha=0.5).tobytes() == F(np.float64(top) / (np.float64(F(0.5)) + 0.0001)).tobytes()
    # a column whose only large c_j is on the closed side of its bound does not set lambda_0
    c2 = np.array([1.0, -2.0, 50.0, 0.5, -40.0, 3.0], dtype=F)
    lo2 = np.array([-INF, -INF, -INF, 0.0, 0.0, -INF], dtype=F)
    hi2 = np.array([INF, INF, 0.0, INF, INF, INF], dtype=F)                 # c = 50 may only go down, c = -40 only up
    assert _lib_lambda0(c2, lo2, hi2) == F(3.0) == bo.box_lambda0(c2, np.ones(6), lo2, hi2)
    assert _lib_lambda0(c2) == F(50.0)
    u2 = np.array([1.0, 0.25, 1.0, 1.0, 1.0, 0.0])                        # the unpenalised column plays no part; -2 / 0.25 = 8
    assert _lib_lambda0(c2, lo2, hi2, u2) == F(8.0) == bo.box_lambda0(c2, u2, lo2, hi2)


def test_restated_prox_without_bounds_and_factors_is_the_soft_threshold_and_the_enet_prox():
    from oracle.solvers import _enet_f, _soft_d
    rng = np.random.default_rng(23)
    p = 230
    none_lo, none_hi = np.full(p, -INF, F), np.full(p, INF, F)
    for lam, rho in ((3.0, 7.0), (40.0, 11.5), (0.25, 2.0)):
        v = (rng.standard_normal(p) * 2).astype(F)
        pen = np.float64(lam) / np.float64(rho)
        assert bo.box_prox(v, np.ones(p), none_lo, none_hi, lam, rho).tobytes() == _soft_d(v, pen, F).tobytes()
        for alpha in (0.0, 0.5, 0.3, 1.0):
            assert bo.box_prox(v, np.ones(p), none_lo, none_hi, lam, rho, alpha).tobytes() == _enet_f(v, pen, alpha).tobytes()
        # with bounds it is that prox moved into the box, and u scales the threshold
        lo, hi = np.where(np.arange(p) % 2 == 0, F(0), F(-0.5)).astype(F), np.full(p, 0.75, F)
        u = rng.uniform(0.5, 2.0, p)
        z = bo.box_prox(v, u, lo, hi, lam, rho)
        assert z.tobytes() == np.clip(_soft_d(v, np.float64(lam) * u / np.float64(rho), F), lo, hi).tobytes()
        assert np.all(z >= lo) and np.all(z <= hi) and np.any(z == lo) and np.any(z == hi)


def test_bounds_round_towards_the_inside_of_the_box():
    lo64 = np.array([-0.1, -1.0 / 3.0, -INF, 0.0, -1e300, -1e-50, -0.25])
    hi64 = np.array([0.1, 1.0 / 3.0, INF, 0.0, 1e300, 1e-50, 0.25])
    lo, hi = bo.round_inwards(lo64, hi64)
    assert lo.dtype == F and hi.dtype == F
    assert np.all(lo.astype(np.float64) >= lo64) and np.all(hi.astype(np.float64) <= hi64)
    tight = np.isfinite(lo64) & (np.abs(lo64) < 1e30) & (lo64 != 0)          # one float further out would leave the box
    assert np.all(np.nextafter(lo[tight], F(-INF)).astype(np.float64) < lo64[tight])
    assert np.all(np.nextafter(hi[tight], F(INF)).astype(np.float64) > hi64[tight])
    assert lo[2] == -INF and hi[2] == INF and lo[4] == -np.finfo(F).max and hi[4] == np.finfo(F).max and lo[6] == F(-0.25)


def test_float64_restatement_on_b1_reaches_the_coordinate_descent_optimum():
    """The float64 restatement at eps 1e-9 against plain projected coordinate descent on the same objective, lambda indices 0, 4, 9 of
    its own grid, Lasso prox, the test pattern: max |b - b_cd| <= 1e-5 in standardised units.  A prototype measured 5.2e-7; the bound
    leaves a factor of 20 for another BLAS."""
    x, y, lower, upper, u = _b1()
    r = bo.box_path(x, y, lower, upper, u, eps=1e-9, T=np.float64)
    assert r["niter"].max() <= 10000
    b = r["beta_std"][:, -1]
    fixed = r["lo"] == r["hi"]
    at_lo, at_hi = (b == r["lo"]) & ~fixed, (b == r["hi"]) & ~fixed
    print(f"[box restatement B1 f64] niter {r['niter'].tolist()}  at a lower bound {int(at_lo.sum())}, at an upper {int(at_hi.sum())}, "
          f"at a non-zero bound {int(((at_lo | at_hi) & (b != 0)).sum())}")
    assert at_lo.sum() > 0 and at_hi.sum() > 0 and ((at_lo | at_hi) & (b != 0)).sum() > 0 and np.all(b[fixed] == 0)
    worst = 0.0
    for l in (0, 4, 9):
        opt = bo.box_cd_optimum(r["Xs"], r["Ys"], r["lam_int"][l], u, r["lo"], r["hi"])
        gap = float(np.abs(r["beta_std"][:, l] - opt).max())
        worst = max(worst, gap)
        print(f"[box restatement B1 f64] lambda index {l}: max |b - b_cd| = {gap:.2e}")
        assert gap <= 1e-5, (l, gap)
    kkt = bo.box_kkt(r["Xs"], r["Ys"], r["beta_std"], r["lam_int"], u, r["lo"], r["hi"])
    print(f"[box restatement B1 f64] largest KKT violation over the path {kkt.max():.2e} (units of lambda_int[0])")
