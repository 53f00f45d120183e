"""GPU: the tall plan's decide-first x-update on the exact 29-bit copy of the cached inverse (ADMM_HIP_SYMV_PACK=1, the default;
lasso_tall.hip, symv_kernels.h: symv1_packed_kernel, format in symv_pack.h) against the fp32 stream (SYMV_PACK=0).  The copy decodes to
the bits of the matrix and the code behind the decode is the fp32 kernel's, so a path must return the same lambda grid, coefficients,
iteration counts and decision trace, byte for byte, and the same number of tiles must leave early.

n = 2700, p = 2100 (tests/test_gpu_refine.py's shape), 6 lambdas.  Which stream a plan uses, and what the pack kernel met, comes from
admm_hip_test_tall_pack_info."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, P, NLAM, LMR = 2700, 2100, 6, 0.02
_cache = {}


def _data():
    if "gauss" not in _cache:
        rng = np.random.default_rng(N + P)
        x = np.asfortranarray(rng.standard_normal((N, P)) * 2.0)
        beta = np.zeros(P)
        beta[:P // 20] = rng.uniform(size=P // 20)
        _cache["gauss"] = (x, x @ beta + rng.standard_normal(N))
    return _cache["gauss"]


def _blocks(split, coupling):
    """Two column blocks, columns < split supported on the first half of the rows and the others on the second half: exactly orthogonal
    (coupling 0), or with the second block leaking `coupling` x N(0, 1) into the first half."""
    key = ("blocks", split, coupling)
    if key not in _cache:
        rng = np.random.default_rng(split)
        x = np.zeros((N, P), order="F")
        h = N // 2
        x[:h, :split] = rng.standard_normal((h, split))
        x[h:, split:] = rng.standard_normal((N - h, P - split))
        if coupling:
            x[:h, split:] = coupling * rng.standard_normal((h, P - split))
        beta = np.zeros(P)
        beta[::40] = 1.0
        _cache[key] = (x, x @ beta + rng.standard_normal(N))
    return _cache[key]


def _groups(p):
    sizes, out, g = [1, 2, 5, 40, 3, 1, 17, 64], [], 0
    while len(out) < p:
        out += [g] * min(sizes[g % len(sizes)], p - len(out))
        g += 1
    return np.asarray(out)


def _model(kind, x, y, **data_opts):
    import admm_amd
    pen = dict(nlambda=NLAM, lambda_min_ratio=LMR)
    if kind == "lasso":
        return admm_amd.admm_lasso(x, y, **data_opts).penalty(**pen)
    if kind == "enet":
        return admm_amd.admm_enet(x, y, **data_opts).penalty(alpha=0.5, **pen)
    return admm_amd.admm_grplasso(x, y, _groups(x.shape[1]), **data_opts).penalty(**pen)


def _ll4(fn):
    from admm_amd import _lib
    out = (ctypes.c_longlong * 4)()
    _lib.check(getattr(_lib.load(), fn)(out))
    return [int(v) for v in out]


def _early_exits():
    from admm_amd import _lib
    n = ctypes.c_longlong(-1)
    _lib.check(_lib.load().admm_hip_test_tall_early_exits(ctypes.byref(n)))
    return int(n.value)


def _path(model, **opts):
    """(fit, decision trace, tiles that left early, pack info) of one path of a fresh plan under the options."""
    from admm_amd import options
    from admm_amd.api import LassoPlan
    with options(**opts):
        plan = LassoPlan(model)
        info = _ll4("admm_hip_test_tall_pack_info")
    try:
        plan.enable_trace(1 << 13)
        fit = plan.run()
        return fit, plan.read_trace(), _early_exits(), info
    finally:
        plan.close()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_same_path(a, b):
    (fa, ta, ea, _), (fb, tb, eb, _) = a, b
    assert _same(fa.lambda_, fb.lambda_) and _same(fa.niter, fb.niter) and _same(fa.beta_dense, fb.beta_dense)
    assert len(ta) == len(tb) > NLAM and _same(ta, tb)
    assert ea == eb > 0                                                  # the discarded launches' tiles leave on either stream
    assert int(fa.stats["xupdate_variant"]) == int(fb.stats["xupdate_variant"]) == 1
    assert int(np.asarray(fa.niter).min()) >= 1 and np.isfinite(fa.beta_dense).all()


@pytest.mark.parametrize("kind", ["lasso", "enet", "grplasso"])
def test_the_packed_stream_gives_the_fp32_streams_path_to_the_bit(kind):
    x, y = _data()
    off = _path(_model(kind, x, y), SYMV_PACK=0)
    on = _path(_model(kind, x, y))                                       # the default
    print(kind, "pack info off / on:", off[3], on[3])
    assert off[3] == [0, 0, 0, 0]
    assert on[3][0] == 1 and on[3][2] == 0 and on[3][3] > 0 and on[3][3] % 7424 == 0
    _assert_same_path(off, on)


def test_exactly_orthogonal_blocks_use_the_zero_code():
    """The inverse of a block-diagonal system has whole blocks of zeros: tiles of nothing but zeros (base 0) and tiles with both."""
    x, y = _blocks(1050, 0.0)
    kw = dict(intercept=False, standardize=False)
    off = _path(_model("lasso", x, y, **kw), SYMV_PACK=0)
    on = _path(_model("lasso", x, y, **kw))
    print("orthogonal blocks, pack info:", on[3])
    assert on[3][0] == 1 and on[3][2] == 0
    _assert_same_path(off, on)


def test_entries_outside_the_window_go_through_the_lists_or_send_the_plan_back_to_fp32():
    """A second block of two columns, the last two, that leaks 1e-12 into the first: the two last rows of the inverse are tiny against
    everything else in their tiles, two entries per column.  The default lists (32) overflow in the tiles of the last row strip: the plan
    keeps the fp32 stream and says so.  A list that holds them: the packed stream, the tiny entries through the lists.  A capacity of 0:
    the fp32 stream again.  The same path always."""
    x, y = _blocks(P - 2, 1e-12)
    kw = dict(intercept=False, standardize=False)
    off = _path(_model("lasso", x, y, **kw), SYMV_PACK=0)
    dflt = _path(_model("lasso", x, y, **kw))
    wide = _path(_model("lasso", x, y, **kw), SYMV_PACK_ESC=4096)
    none = _path(_model("lasso", x, y, **kw), SYMV_PACK_ESC=0)
    print("leaking blocks, pack info default / 4096 / 0:", dflt[3], wide[3], none[3])
    assert dflt[3][0] == 0 and dflt[3][1] > 32 and dflt[3][2] >= 1       # overflowed: the fp32 fallback, reported
    assert wide[3][0] == 1 and wide[3][1] == dflt[3][1] and wide[3][2] == 0
    assert none[3][0] == 0 and none[3][1] == dflt[3][1] and none[3][2] >= dflt[3][2]
    for other in (dflt, wide, none):
        _assert_same_path(off, other)
