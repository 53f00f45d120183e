"""Sparse-group lasso (admm_hip_sgl), everything that needs no GPU: what the C ABI refuses before it looks for a device, the declared
and exported symbols, the Python builder (labels, l1_weights under a column permutation, alpha), the host's lambda_0 against the
bisection of tests/sgl_oracle.py, the two degenerate cases of the restated prox, and the restated path on the shape S1."""
import ctypes
import os
import re

import numpy as np
import pytest

import group_oracle as go
import sgl_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 2
F = np.float32


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _call(entry="sgl", n=6, p=4, group=(0, 0, 1, 2), weights=None, ngroups=3, l1=None, alpha=0.5, x="ok", opts=(10, 1e-5, 1e-5, -1.0),
          nlambda_auto=5, lmin_ratio=0.01, mem=0):
    from admm_amd import _lib
    from admm_amd._lib import AdmmOpts
    lib = _lib.load()
    xa = np.asfortranarray(np.ones((n, p)))
    ya = np.ones(n)
    g = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    u = None if l1 is None else np.ascontiguousarray(l1, dtype=np.float64)
    o = AdmmOpts(*opts)
    lam_out, beta, nit = np.zeros(nlambda_auto + 1), np.zeros((p + 1) * (nlambda_auto + 1), dtype=np.float32), np.zeros(nlambda_auto + 1, dtype=np.int32)
    head = (ctypes.c_void_p(xa.ctypes.data) if x == "ok" else None, ctypes.c_void_p(ya.ctypes.data), n, p, mem,
            None if g is None else g.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(w), ngroups, _dp(u), alpha,
            None, 0, nlambda_auto, lmin_ratio, 1, 1, ctypes.byref(o))
    if entry == "sgl":
        rc = lib.admm_hip_sgl(*head, lam_out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                              beta.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nit.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None)
    else:
        h = ctypes.c_void_p()
        rc = lib.admm_hip_sgl_plan_create(*head, ctypes.byref(h), None)
        assert h.value is None or rc == 0
    return rc, lib.admm_hip_last_error().decode()


REFUSALS = [
    # the grouping, as PathSpec::check_groups checks it
    (dict(group=None), "group must not be NULL"),
    (dict(group=(1, 1, 2, 3), ngroups=4), "start at 0"),
    (dict(group=(0, 1, 0, 2)), "non-decreasing"),
    (dict(group=(0, 0, 2, 3), ngroups=4), "no gaps"),
    (dict(ngroups=4), "ngroups does not match"),
    (dict(ngroups=2), "ngroups does not match"),
    (dict(n=1200, p=1100, group=[0] * 1025 + list(range(1, 76)), ngroups=76), "more than ADMM_HIP_GROUP_MAX (1024) columns"),
    # the mixing parameter
    (dict(alpha=-0.01), "within [0, 1]"),
    (dict(alpha=1.01), "within [0, 1]"),
    (dict(alpha=np.nan), "within [0, 1]"),
    (dict(alpha=np.inf), "within [0, 1]"),
    # the two kinds of weights
    (dict(weights=(1.0, -0.5, 1.0)), "group weights must be finite and non-negative"),
    (dict(weights=(1.0, np.nan, 1.0)), "group weights must be finite and non-negative"),
    (dict(weights=(1.0, np.inf, 1.0)), "group weights must be finite and non-negative"),
    (dict(l1=(1.0, 1.0, -1.0, 1.0)), "l1 weights must be finite and non-negative"),
    (dict(l1=(1.0, np.nan, 1.0, 1.0)), "l1 weights must be finite and non-negative"),
    (dict(l1=(np.inf, 1.0, 1.0, 1.0)), "l1 weights must be finite and non-negative"),
    # no positive penalty anywhere
    (dict(alpha=0.0, weights=(0.0, 0.0, 0.0)), "positive penalty"),
    (dict(alpha=1.0, l1=(0.0, 0.0, 0.0, 0.0)), "positive penalty"),
    (dict(alpha=0.5, weights=(0.0, 0.0, 0.0), l1=(0.0, 0.0, 0.0, 0.0)), "positive penalty"),
    # n > p only
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


@pytest.mark.parametrize("entry", ["sgl", "sgl_plan_create"])
def test_c_abi_refuses_bad_sgl_calls_before_it_looks_for_a_device(entry):
    for spoil, fragment in REFUSALS:
        rc, msg = _call(entry, **spoil)
        assert rc == INVALID_ARG and fragment in msg, (entry, spoil if len(spoil.get("group") or ()) < 9 else "cap", rc, msg)


@pytest.mark.parametrize("entry", ["sgl", "sgl_plan_create"])
def test_refine_is_refused_for_the_sparse_group_lasso(entry):
    from admm_amd import _lib
    with _lib.options(REFINE="1"):
        rc, msg = _call(entry)
    assert rc == INVALID_ARG and "REFINE" in msg


def test_calls_with_some_positive_penalty_pass_the_checks():
    # one positive weight of either kind is enough; a 1024-column group is allowed: the call gets as far as the device (or runs)
    for kw in (dict(), dict(alpha=0.0), dict(alpha=1.0), dict(alpha=1.0, l1=(0.0, 0.0, 0.0, 2.0), weights=(0.0, 0.0, 0.0)),
               dict(alpha=0.0, weights=(0.0, 0.5, 0.0), l1=(0.0, 0.0, 0.0, 0.0)), dict(alpha=0.3, weights=(0.0, 0.0, 0.0)),
               dict(n=1200, p=1100, group=[0] * 1024 + list(range(1, 77)), ngroups=77, opts=(1, 1e-5, 1e-5, -1.0), nlambda_auto=1)):
        for entry in ("sgl", "sgl_plan_create"):
            rc, msg = _call(entry, **kw)
            assert rc in (0, NO_DEVICE), (entry, kw if "n" not in kw else "cap", rc, msg)


def test_symbols_are_declared_and_exported():
    from admm_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "admm_hip.h")).read(), flags=re.S)
    for sym in ("admm_hip_sgl", "admm_hip_sgl_plan_create", "admm_hip_host_sgl_lambda0"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym) and sym in _lib.EXPORTS
    import admm_amd
    assert "admm_sgl" in admm_amd.__all__ and "ADMM_SGL" in admm_amd.__all__


def test_builder_labels_l1_weights_under_a_permutation_and_alpha():
    from admm_amd import admm_sgl, ADMM_SGL, ADMM_GrpLasso, DevicePtr
    rng = np.random.default_rng(5)
    x = rng.standard_normal((20, 6))
    y = rng.standard_normal(20)
    m = admm_sgl(x, y, ["b", "b", "a", "c", "c", "c"])
    assert isinstance(m, ADMM_SGL) and isinstance(m, ADMM_GrpLasso) and m.alpha == 0.95            # the SGL package's default
    assert m.group.tolist() == [0, 0, 1, 2, 2, 2] and list(m.group_labels) == ["b", "a", "c"] and m._perm is None and m.x is x
    assert m.l1_weights is None and m.group_weights is None
    m.penalty(nlambda=4, lambda_min_ratio=0.1, l1_weights=[1, 2, 3, 4, 5, 6], group_weights=[1.0, 0.0, 2.5])
    assert m.l1_weights.tolist() == [1, 2, 3, 4, 5, 6] and m.group_weights.tolist() == [1.0, 0.0, 2.5] and m.nlambda == 4
    args = m._group_args()
    assert len(args) == 5 and args[2] == 3 and args[4] == 0.95
    # scattered labels: the l1 weights are the caller's, per caller column, and travel with the columns
    s = admm_sgl(x, y, [7, 3, 7, 3, 9, 7], alpha=0.5).penalty(l1_weights=[10, 11, 12, 13, 14, 15])
    assert s._perm.tolist() == [0, 2, 5, 1, 3, 4] and s.group.tolist() == [0, 0, 0, 1, 1, 2]
    assert s.l1_weights.tolist() == [10, 12, 15, 11, 13, 14]
    assert np.array_equal(np.asarray(s.x), x[:, s._perm])
    back = s._restore(np.arange(14, dtype=np.float32).reshape(7, 2))
    for k, j in enumerate(s._perm):
        assert back[1 + j].tolist() == [2.0 * (1 + k), 2.0 * (1 + k) + 1]
    # alpha outside [0, 1] or not a number
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"within \[0, 1\]"):
            admm_sgl(x, y, [0, 0, 1, 1, 2, 2], alpha=bad)
    assert admm_sgl(x, y, [0] * 6, alpha=0).alpha == 0.0 and admm_sgl(x, y, [0] * 6, alpha=1).alpha == 1.0
    # weights
    g = admm_sgl(x, y, [0, 0, 1, 1, 2, 2], alpha=0.5)
    for kw, frag in ((dict(l1_weights=[1.0] * 5), "one entry per column"), (dict(l1_weights=[1, 1, -1, 1, 1, 1]), "non-negative"),
                     (dict(l1_weights=[1, 1, np.nan, 1, 1, 1]), "finite"), (dict(group_weights=[1.0, 2.0]), "one entry per group"),
                     (dict(group_weights=[1.0, -1.0, 1.0]), "non-negative"),
                     (dict(group_weights=[0.0] * 3, l1_weights=[0.0] * 6), "positive penalty")):
        with pytest.raises(ValueError, match=frag):
            g.penalty(**kw)
    g.penalty(group_weights=[0.0] * 3)                                   # the l1 part still penalises: accepted at alpha = 0.5
    with pytest.raises(ValueError, match="positive penalty"):
        admm_sgl(x, y, [0, 0, 1, 1, 2, 2], alpha=0.0).penalty(group_weights=[0.0] * 3)
    with pytest.raises(ValueError, match="positive penalty"):
        admm_sgl(x, y, [0, 0, 1, 1, 2, 2], alpha=1.0).penalty(l1_weights=[0.0] * 6)
    # the group lasso's own refusals hold
    with pytest.raises(ValueError, match="n > p only"):
        admm_sgl(x[:6], y[:6], [0] * 6)
    with pytest.raises(ValueError, match="adjacent"):
        admm_sgl(DevicePtr(4096), DevicePtr(8192), [0, 1, 0, 1, 2, 2], n=20, p=6)
    for call in (lambda: g.parallel(2), lambda: g.cv(3), lambda: g.fit_responses(np.zeros((20, 2)))):
        with pytest.raises(ValueError, match="not available for the sparse-group lasso"):
            call()


# ---- lambda_0 of the automatic grid

def _lib_lambda0(c, sizes, alpha, u=None, w=None):
    from admm_amd import _lib
    lib = _lib.load()
    c = np.ascontiguousarray(c, dtype=np.float32)
    g = np.ascontiguousarray(np.repeat(np.arange(len(sizes)), sizes), dtype=np.int32)
    u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    out = ctypes.c_float()
    rc = lib.admm_hip_host_sgl_lambda0(c.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), c.size, g.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                       _dp(w), len(sizes), _dp(u), float(alpha), ctypes.byref(out))
    assert rc == 0, lib.admm_hip_last_error().decode()
    return np.float32(out.value)


def _lambda0_cases():
    rng = np.random.default_rng(21)
    cases = []
    for sizes in (go.S1_SIZES, [1] * 9, [4] * 6, [37, 1, 2, 64, 3], [1024, 1, 5]):
        p = int(np.sum(sizes))
        c = (rng.standard_normal(p) * 30).astype(F)
        u = rng.uniform(0.5, 2.0, p)
        w = go.default_weights(sizes) * rng.uniform(0.5, 1.5, len(sizes))
        cases.append(("plain", sizes, c, None, None))
        cases.append(("weighted", sizes, c, u, w))
        # one group weight zero, l1 weights zero here and there (in that group too: it can then not be emptied for alpha > 0 either)
        u0, w0 = u.copy(), w.copy()
        w0[len(sizes) // 2] = 0.0
        u0[rng.choice(p, size=max(1, p // 5), replace=False)] = 0.0
        cases.append(("zeros", sizes, c, u0, w0))
        # c_g = 0 on the largest group, and ties: equal |c| / u inside a group
        c0 = c.copy()
        st = go.group_starts(sizes)
        k = int(np.argmax(sizes))
        c0[st[k]:st[k + 1]] = 0
        cases.append(("zero-c", sizes, c0, u, w))
        ct = np.full(p, 8.0, dtype=F) * np.where(rng.random(p) < 0.5, -1, 1).astype(F)
        ut = np.where(rng.random(p) < 0.5, 1.0, 2.0)
        cases.append(("ties", sizes, ct, ut, None))
        cases.append(("all-tied", sizes, ct, None, None))
    return cases


def test_host_lambda0_is_the_oracles_bisection_to_the_last_float():
    """Both sides solve f_g in double, so they differ by the final rounding to float at the most: one float spacing."""
    worst = 0.0
    for name, sizes, c, u, w in _lambda0_cases():
        for alpha in (0.0, 0.3, 0.95, 1.0):
            l1, wg, _ = so.sgl_weights(sizes, alpha, u, w)
            if not (np.any(l1 > 0) or np.any(wg > 0)):
                continue
            ref = so.sgl_lambda0(c, sizes, l1, wg)
            got = _lib_lambda0(c, sizes, alpha, u, w)
            gap = abs(np.float64(got) - ref) / np.spacing(F(ref))
            worst = max(worst, float(gap))
            assert gap <= 1.0, (name, len(sizes), alpha, got, ref)
    print(f"[sgl lambda0] largest |library - bisection| = {worst:.3f} float spacings")


def test_host_lambda0_degenerate_cases_are_bit_equal():
    rng = np.random.default_rng(22)
    for sizes in (go.S1_SIZES, [4] * 6, [1] * 9, [1024, 1, 5]):
        p = int(np.sum(sizes))
        c = (rng.standard_normal(p) * 30).astype(F)
        st = go.group_starts(sizes)
        gn = np.array([np.sqrt(sum(np.float64(v) * np.float64(v) for v in c[st[k]:st[k + 1]])) for k in range(len(sizes))])     # in column order, as the host
        for w in (None, go.default_weights(sizes) * rng.uniform(0.5, 1.5, len(sizes))):
            ww = go.default_weights(sizes) if w is None else w.copy()
            if w is not None:
                ww[0] = 0.0
            want = F(np.max(gn[ww > 0] / ww[ww > 0]))                          # group_lambda0: sqrt(sum c^2) / w over the penalised groups
            assert _lib_lambda0(c, sizes, 0.0, None, None if w is None else ww).tobytes() == want.tobytes(), (len(sizes), "alpha 0")
            assert _lib_lambda0(c, sizes, 0.0, rng.uniform(0, 2, p), None if w is None else ww).tobytes() == want.tobytes()      # u plays no part
        assert _lib_lambda0(c, sizes, 1.0).tobytes() == np.max(np.abs(c)).tobytes(), (len(sizes), "alpha 1")               # device_absmax
        assert _lib_lambda0(c, sizes, 1.0, None, rng.uniform(0, 2, len(sizes))).tobytes() == np.max(np.abs(c)).tobytes()   # w plays no part


# ---- the restated prox and path

def test_restated_prox_alpha_zero_is_the_group_prox_and_alpha_one_the_soft_threshold():
    from oracle.solvers import _soft_d
    rng = np.random.default_rng(23)
    sizes = go.S1_SIZES
    p = int(np.sum(sizes))
    u = rng.uniform(0.5, 2.0, p)
    w = go.default_weights(sizes)
    w[3], w[9] = 0.0, 0.5
    for lam, rho in ((3.0, 7.0), (40.0, 11.5), (0.25, 2.0)):
        v = (rng.standard_normal(p) * 2).astype(F)
        l1, wg, _ = so.sgl_weights(sizes, 0.0, u, w)
        assert np.all(l1 == 0) and np.array_equal(wg, w)
        z = so.sgl_prox(v, sizes, l1, wg, lam, rho)[0]
        assert z.tobytes() == go.group_prox(v, sizes, w, lam, rho)[0].tobytes()
        l1, wg, _ = so.sgl_weights(sizes, 1.0, None, w)
        assert np.all(wg == 0) and np.all(l1 == 1)
        z = so.sgl_prox(v, sizes, l1, wg, lam, rho)[0]
        assert z.tobytes() == _soft_d(v, np.float64(lam) / np.float64(rho), F).tobytes()
        l1, wg, _ = so.sgl_weights(sizes, 1.0, u, w)
        assert so.sgl_prox(v, sizes, l1, wg, lam, rho)[0].tobytes() == _soft_d(v, np.float64(lam) * u / np.float64(rho), F).tobytes()


@pytest.mark.parametrize("alpha", [0.5, 0.95])
def test_restated_path_on_s1_selects_inside_groups_and_meets_its_kkt_bounds(alpha):
    """The float32 restatement on S1 (n = 600, S1_SIZES, seed 11, default weights, 10 lambdas down to 0.01, eps 1e-5).  Sanity bounds
    on the restatement, not on the library: off <= 1e-4, on <= 5e-3.  A scratch restatement gave on 1.3e-3 (alpha 0.5) and 6.7e-4
    (0.95), off 0, an empty model at lambda[0] and from lambda[1] on at least two multi-column groups with zero and non-zero
    coefficients side by side; this one prints its own figures."""
    x, y = go.synth_groups(600, go.S1_SIZES, seed=11)
    r = so.sgl_path(x, y, go.S1_SIZES, alpha, nlambda=10, lmin_ratio=0.01, eps=1e-5)
    s = r["solver"]
    off, on, unp = so.sgl_kkt(r["Xs"], r["Ys"], r["beta_std"], r["lam_int"], go.S1_SIZES, s.l1, s.wg)
    off_max, on_max, unp_max = so.sgl_kkt_maxima(off, on, unp, r["lam"])
    nact = [so.active_groups(r["beta_std"][:, l], go.S1_SIZES) for l in range(10)]
    nmixed = [len(so.mixed_groups(r["beta_std"][:, l], go.S1_SIZES)) for l in range(10)]
    print(f"[sgl restatement S1 alpha={alpha}] off*ratio {off_max:.3e}  on*ratio {on_max:.3e}  unp {unp_max:.3e}  niter {r['niter'].tolist()}  "
          f"active groups {nact}  groups with zeros and non-zeros {nmixed}")
    assert r["niter"].max() <= 10000
    assert off_max <= 1e-4 and on_max <= 5e-3 and unp_max == 0.0
    assert nact[0] <= 1 and nact[9] >= nact[5] >= nact[2] >= 1
    assert min(nmixed[1:]) >= 1                      # within-group sparsity at every lambda past the first: what the penalty is for
