"""GPU: tiles of the tall x-update leave early when the launch they belong to is discarded (symv_kernels.h: SymvVerdict;
lasso_tall.hip: tall_decide publishes the verdict word).  How many tiles leave is a matter of timing; what the path returns must
not be: the same plan run with the check on, a plan with it off (ADMM_HIP_SYMV_VERDICT=0) and the first plan run a second time
(the verdict words of its first run are still in memory and must not match) return lambda, niter and beta identical to the bit.
"On" is the default (level 2: the tiles look in their prologue and between the chunks of their column loop) and, for the Lasso,
also level 1 (prologue only); the count below is of the tiles that left in their prologue.

Shapes: n = 4400, p = 4200 cut into 32-column segments (SYMV_SCHED "32,32,0") is 1220 tiles -- more than the 1024 workgroups a
256-CU device holds at once, so some tiles start after the decision of their launch has been published; p = 2304 under the
default schedule is resident as a whole.  8 lambdas, lambda_min_ratio 0.01: a discarded launch after every converged lambda, the last of them the launch
of the final decision."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NLAM, LMR = 8, 0.01
_cache = {}


def _data(n, p):
    if (n, p) not in _cache:
        rng = np.random.default_rng(n + p)
        x = np.asfortranarray(rng.standard_normal((n, p)) * 2.0)
        beta = np.zeros(p)
        beta[:p // 20] = rng.uniform(size=p // 20)
        _cache[(n, p)] = (x, x @ beta + rng.standard_normal(n))
    return _cache[(n, p)]


def _groups(p):
    """Adjacent groups of mixed sizes: singletons, small ones, one that spans several workgroups of the tail."""
    sizes, out, g = [1, 2, 5, 40, 3, 1, 17, 64], [], 0
    while len(out) < p:
        out += [g] * min(sizes[g % len(sizes)], p - len(out))
        g += 1
    return np.asarray(out)


def _model(kind, x, y):
    import admm_amd
    if kind == "lasso":
        return admm_amd.admm_lasso(x, y).penalty(nlambda=NLAM, lambda_min_ratio=LMR)
    if kind == "enet":
        return admm_amd.admm_enet(x, y).penalty(nlambda=NLAM, lambda_min_ratio=LMR, alpha=0.5)
    return admm_amd.admm_grplasso(x, y, _groups(x.shape[1])).penalty(nlambda=NLAM, lambda_min_ratio=LMR)


def _early_exits():
    from admm_amd import _lib
    n = ctypes.c_longlong(-1)
    _lib.check(_lib.load().admm_hip_test_tall_early_exits(ctypes.byref(n)))
    return int(n.value)


def _three_fits(kind, n, p, sched, level):
    """(fit, tiles that left early) of: the check on; off; on again on the first plan."""
    from admm_amd import options
    from admm_amd.api import LassoPlan
    x, y = _data(n, p)
    opts = {} if sched is None else {"SYMV_SCHED": sched}
    out = []
    with options(SYMV_VERDICT=level, **opts):
        plan_on = LassoPlan(_model(kind, x, y))
    with options(SYMV_VERDICT=0, **opts):
        plan_off = LassoPlan(_model(kind, x, y))
    try:
        for plan in (plan_on, plan_off, plan_on):
            fit = plan.run()
            out.append((fit, _early_exits()))
    finally:
        plan_on.close()
        plan_off.close()
    return out


def _check(kind, n, p, sched, level=None):
    (on, n_on), (off, n_off), (again, n_again) = _three_fits(kind, n, p, sched, level)
    print(f"{kind} n={n} p={p} sched={sched} level={level}: niter {list(map(int, on.niter))}, x-update launches {on.stats['xupdate_launches']}, "
          f"tiles that left early: on {n_on}, off {n_off}, on again {n_again}")
    assert int(on.stats["xupdate_variant"]) == 1                        # the lower-triangle kernel
    assert n_off == 0
    assert int(on.niter.min()) >= 1
    for other in (off, again):
        assert np.array_equal(on.lambda_, other.lambda_)
        assert np.array_equal(on.niter, other.niter)
        a, b = np.ascontiguousarray(on.beta_dense), np.ascontiguousarray(other.beta_dense)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind", ["lasso", "enet", "grplasso"])
def test_more_tiles_than_resident_slots(kind):
    _check(kind, 4400, 4200, "32,32,0")


def test_more_tiles_than_resident_slots_prologue_check_only():
    _check("lasso", 4400, 4200, "32,32,0", level=1)


def test_everything_resident_default_schedule():
    _check("lasso", 2500, 2304, None)
