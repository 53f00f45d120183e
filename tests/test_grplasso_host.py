"""Group lasso (admm_hip_grplasso), everything that needs no GPU: what the C ABI refuses before it looks for a device, the
Python builder's handling of labels, column order and weights, the declared / exported symbols, and the NumPy restatement of
the iteration (tests/group_oracle.py) held to the project's own Lasso KKT bounds on the shape S1."""
import ctypes
import os
import re

import numpy as np
import pytest

import group_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 2


def _call(entry="grplasso", n=6, p=4, group=(0, 0, 1, 2), weights=None, ngroups=3, x="ok", opts=(10, 1e-5, 1e-5, -1.0),
          nlambda_auto=5, lmin_ratio=0.01, mem=0):
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    xa = np.asfortranarray(np.ones((n, p)))
    ya = np.ones(n)
    g = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    o = AdmmOpts(*opts)
    lam_out, beta, nit = np.zeros(nlambda_auto + 1), np.zeros((p + 1) * (nlambda_auto + 1), dtype=np.float32), np.zeros(nlambda_auto + 1, dtype=np.int32)
    head = (ctypes.c_void_p(xa.ctypes.data) if x == "ok" else None, ctypes.c_void_p(ya.ctypes.data), n, p, mem,
            None if g is None else g.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
            None if w is None else w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ngroups,
            None, 0, nlambda_auto, lmin_ratio, 1, 1, ctypes.byref(o))
    if entry == "grplasso":
        rc = lib.admm_hip_grplasso(*head, lam_out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                   beta.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nit.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None)
    else:
        h = ctypes.c_void_p()
        rc = lib.admm_hip_grplasso_plan_create(*head, ctypes.byref(h), None)
        assert h.value is None or rc == 0
    return rc, lib.admm_hip_last_error().decode()


REFUSALS = [
    (dict(group=None), "group must not be NULL"),
    (dict(group=(1, 1, 2, 3), ngroups=4), "start at 0"),
    (dict(group=(0, 1, 0, 2)), "non-decreasing"),
    (dict(group=(0, 0, 2, 3), ngroups=4), "no gaps"),
    (dict(ngroups=4), "ngroups does not match"),
    (dict(ngroups=2), "ngroups does not match"),
    (dict(weights=(1.0, -0.5, 1.0)), "finite and non-negative"),
    (dict(weights=(1.0, np.nan, 1.0)), "finite and non-negative"),
    (dict(weights=(1.0, np.inf, 1.0)), "finite and non-negative"),
    (dict(weights=(0.0, 0.0, 0.0)), "at least one group weight must be positive"),
    (dict(n=1200, p=1100, group=[0] * 1025 + list(range(1, 76)), ngroups=76), "more than ADMM_HIP_GROUP_MAX (1024) columns"),
    (dict(n=4, p=4), "built for n > p only"),
    (dict(n=3, p=4), "built for n > p only"),
    # what check_common / PathSpec::check() refuse for every path entry point
    (dict(x=None), "x and y must not be NULL"),
    (dict(n=0), "n and p must be positive"),
    (dict(mem=7), "mem must be"),
    (dict(opts=(0, 1e-5, 1e-5, -1.0)), "maxit should be positive"),
    (dict(opts=(10, -1.0, 1e-5, -1.0)), "nonnegative"),
    (dict(nlambda_auto=0), "need a lambda grid"),
    (dict(lmin_ratio=1.0), "lambda_min_ratio"),
]


@pytest.mark.parametrize("entry", ["grplasso", "grplasso_plan_create"])
def test_c_abi_refuses_bad_group_calls_before_it_looks_for_a_device(entry):
    for spoil, fragment in REFUSALS:
        rc, msg = _call(entry, **spoil)
        assert rc == INVALID_ARG and fragment in msg, (entry, spoil if "group" not in spoil or len(spoil.get("group") or ()) < 9 else "cap", rc, msg)


def test_a_group_of_exactly_the_cap_is_accepted_by_the_checks():
    # 1024 columns pass the argument checks: the call gets as far as the device (or runs, where there is one)
    rc, msg = _call(n=1200, p=1100, group=[0] * 1024 + list(range(1, 77)), ngroups=77, opts=(1, 1e-5, 1e-5, -1.0), nlambda_auto=1)
    assert rc in (0, NO_DEVICE), (rc, msg)


def test_refine_is_refused_for_the_group_lasso():
    from admm_amd import _lib
    with _lib.options(REFINE="1"):
        rc, msg = _call()
    assert rc == INVALID_ARG and "REFINE" in msg


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a machine without a GPU")
def test_valid_group_calls_find_no_device():
    for entry in ("grplasso", "grplasso_plan_create"):
        for kw in (dict(), dict(weights=(0.0, 2.0, 0.5)), dict(group=(0, 1, 2, 3), ngroups=4)):
            rc, msg = _call(entry, **kw)
            assert rc == NO_DEVICE, (entry, kw, rc, msg)


def test_symbols_are_declared_and_exported():
    from admm_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "admm_hip.h")).read(), flags=re.S)
    for sym in ("admm_hip_grplasso", "admm_hip_grplasso_plan_create"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym) and sym in _lib.EXPORTS
    assert re.search(r"#define\s+ADMM_HIP_GROUP_MAX\s+1024\b", hdr) and _lib.GROUP_MAX == 1024


def test_builder_renumbers_labels_reorders_columns_and_restores_coefficients():
    from admm_amd import admm_grplasso, ADMM_GrpLasso, ADMM_Lasso
    rng = np.random.default_rng(5)
    x = rng.standard_normal((20, 6))
    y = rng.standard_normal(20)
    # contiguous labels of any kind: numbered in order of first appearance, x untouched
    m = admm_grplasso(x, y, ["b", "b", "a", "c", "c", "c"])
    assert isinstance(m, ADMM_GrpLasso) and isinstance(m, ADMM_Lasso)
    assert m.group.dtype == np.int32 and m.group.tolist() == [0, 0, 1, 2, 2, 2] and m.ngroups == 3
    assert list(m.group_labels) == ["b", "a", "c"] and m._perm is None and m.x is x
    assert m.group_weights is None and np.allclose(m.effective_weights(), np.sqrt([2, 1, 3]))
    # scattered labels: columns gathered group by group (stable), coefficients put back where the caller had them
    s = admm_grplasso(x, y, [7, 3, 7, 3, 9, 7])
    assert s.group.tolist() == [0, 0, 0, 1, 1, 2] and list(s.group_labels) == [7, 3, 9]
    assert s._perm.tolist() == [0, 2, 5, 1, 3, 4]
    assert np.array_equal(np.asarray(s.x), x[:, [0, 2, 5, 1, 3, 4]])
    lib_beta = np.arange(14, dtype=np.float32).reshape(7, 2)            # row 0 intercept, row 1 + k = library column k
    back = s._restore(lib_beta)
    assert np.array_equal(back[0], lib_beta[0])
    for k, j in enumerate(s._perm):
        assert np.array_equal(back[1 + j], lib_beta[1 + k])
    # weights: one per group in order of first appearance
    s.penalty(nlambda=4, lambda_min_ratio=0.1, group_weights=[1.0, 0.0, 2.5])
    assert s.group_weights.tolist() == [1.0, 0.0, 2.5] and s.nlambda == 4 and s.lambda_min_ratio == 0.1
    s.opts(maxit=50, eps_abs=1e-6)
    assert s.maxit == 50
    for bad, frag in (([1.0, 2.0], "one entry per group"), ([1.0, -1.0, 1.0], "non-negative"), ([1.0, np.nan, 1.0], "finite"),
                      ([0.0, 0.0, 0.0], "positive")):
        with pytest.raises(ValueError, match=frag):
            s.penalty(group_weights=bad)


def test_builder_refusals():
    from admm_amd import admm_grplasso, DevicePtr
    rng = np.random.default_rng(6)
    x = rng.standard_normal((20, 6))
    y = rng.standard_normal(20)
    with pytest.raises(ValueError, match="n > p only"):
        admm_grplasso(x[:6], y[:6], [0] * 6)
    with pytest.raises(ValueError, match="length ncol"):
        admm_grplasso(x, y, [0, 0, 1])
    with pytest.raises(ValueError, match="adjacent"):
        admm_grplasso(DevicePtr(4096), DevicePtr(8192), [0, 1, 0, 1, 2, 2], n=20, p=6)
    d = admm_grplasso(DevicePtr(4096), DevicePtr(8192), [4, 4, 1, 1, 2, 2], n=20, p=6)      # adjacent groups: used in place
    assert d.group.tolist() == [0, 0, 1, 1, 2, 2] and d._perm is None
    with pytest.raises(ValueError, match="more than 1024"):
        admm_grplasso(rng.standard_normal((1030, 1025)), rng.standard_normal(1030), [0] * 1025)
    m = admm_grplasso(x, y, [0, 0, 1, 1, 2, 2])
    for call in (lambda: m.parallel(2), lambda: m.cv(3), lambda: m.fit_responses(np.zeros((20, 2)))):
        with pytest.raises(ValueError, match="not available for the group lasso"):
            call()


@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_meets_the_lasso_kkt_bounds_on_s1(weighted):
    """The float32 restatement of the iteration, on S1 (n = 600, p = 230), 10 lambdas down to 0.01, eps 1e-5: the project's Lasso
    KKT bounds in group form.  Recorded with seed 11: default weights (viol - 1) ratio 8.2e-5, on ratio 1.07e-3; one weight 0 and
    one 0.5: 1.1e-4, 1.1e-3, unp 7.0e-4."""
    x, y = go.synth_groups(600, go.S1_SIZES, seed=11)
    w = go.default_weights(go.S1_SIZES)
    if weighted:
        w[3], w[9] = 0.0, 0.5
    r = go.grp_path(x, y, go.S1_SIZES, w, nlambda=10, lmin_ratio=0.01, eps=1e-5)
    viol, on, unp = go.group_kkt(r["Xs"], r["Ys"], r["beta_std"], r["lam_int"], go.S1_SIZES, w)
    over, on_max, unp_max = go.kkt_maxima(viol, on, unp, r["lam"])
    print(f"[grplasso restatement S1 weighted={weighted}] (viol-1)*ratio {over:.3e}  on*ratio {on_max:.3e}  unp {unp_max:.3e}  niter {r['niter'].tolist()}")
    assert r["niter"].max() <= 10000
    assert over < 2e-3 and on_max < 2e-3 and viol.max() < 1.3
    st = go.group_starts(go.S1_SIZES)
    nact = [sum(bool(np.any(r["beta_std"][st[k]:st[k + 1], l] != 0)) for k in range(len(w)) if w[k] > 0) for l in range(10)]
    assert nact[0] <= 1 and nact[9] >= nact[5] >= nact[2] >= 1
    if weighted:
        assert np.all(np.any(r["beta_std"][st[3]:st[4]] != 0, axis=0))      # the unpenalised group is in the model at every lambda
        assert unp_max < 2e-3


def test_singleton_groups_of_weight_one_restate_the_lasso_oracle_exactly():
    """Groups of one column with weight 1 are the Lasso: the restatement reproduces oracle/entry.py admm_lasso bit for bit."""
    from oracle import entry
    x, y = go.synth_groups(120, [1] * 17, seed=3)
    ref = entry.admm_lasso(x, y, None, 6, 0.05, True, True, entry.LASSO_OPTS)
    r = go.grp_path(x, y, [1] * 17, np.ones(17), nlambda=6, lmin_ratio=0.05)
    assert np.array_equal(ref["lambda"], r["lam"]) and np.array_equal(ref["niter"], r["niter"])
    assert ref["beta"].tobytes() == r["beta"].tobytes()
